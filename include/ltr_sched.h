/*
 * ltr_sched.h -- test and measurement hooks of the in-kernel list-length scheduling and of the lazy step's launch.
 *
 * Exported by the same libltr_hip.so as include/ltr_hip.h, with its conventions (0 = OK, < 0 = LTR_ERR_*), and like
 * every ltr_debug_* hook left out of a build with -DLTR_NO_DEBUG_HOOKS.
 */
#ifndef LTR_SCHED_H
#define LTR_SCHED_H

#include "ltr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Tests only (host arithmetic, no device needed): the place in the list-length order that block id nred + i of a grid of
 * `nred` reducer workgroups + B query workgroups takes under the in-kernel scheduling, i = 0 .. B - 1: group[i], the sample
 * group (G = ceil(B / 64) of them), and rank[i], the member rank inside it by descending list length.  cus > 0: the rounds
 * of `cus` workgroups are dealt in snake order (the register tile); nred > 0: a lazy launch, the workgroups on the reducers'
 * CUs take the last places (the quiet rule: fewer reducers than CUs, and a grid of fewer than eight rounds of
 * `cus` workgroups -- LTR_ERR_SHAPE beyond). */
LTR_DEBUG_HOOK int ltr_debug_sched_slots(int B, int G, int cus, int nred, int *group, int *rank);
/* Tests only (host arithmetic): the same for the register tile's dealing by hosting CU -- exactly what its kernel computes for
 * query workgroup i, block id nred + i, of a grid of whole rounds: B a multiple of 64 and 2, 3 or 4 times `cus`, G = B / 64,
 * 0 <= nred < cus reducer workgroups in front, quiet != 0: the quiet rule is on (needs nred > 0).  LTR_ERR_SHAPE where that
 * dealing does not apply (the kernel then keeps the one of ltr_debug_sched_slots). */
LTR_DEBUG_HOOK int ltr_debug_sched_slots_cu(int B, int G, int cus, int nred, int quiet, int *group, int *rank);
/* Measurements only: the hold-backs of the lazy launch's query workgroups in units of 512 cycles, low byte: everybody's,
 * next byte: the workgroups' on the reducers' CUs; < 0: the library's own choice again.  Returns the old value. */
LTR_DEBUG_HOOK int ltr_debug_lazy_holdback(int packed);

#ifdef __cplusplus
}
#endif

#endif /* LTR_SCHED_H */
