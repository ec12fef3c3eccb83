/*
 * ltr_bf16_general.h -- C ABI of the GENERAL fused step of the Linear(F, 1) scorer on a bf16 feature batch: scores,
 * pairwise loss, d loss / d score and the query's weight-gradient row in ONE launch, one workgroup per query, for the
 * lists and rows the register tile of include/ltr_linear_bf16.h cannot hold (more than 256 documents, or more than 16
 * sweeps of a 512-thread workgroup: 80 documents at 704 features).  The rows are read twice, the second time in
 * reverse (the L2 still holds the tail of the first pass); no score matrix is written and read back, and one launch
 * replaces the three of scorer, loss and weight gradient.
 *
 * Exported by the same libltr_hip.so as include/ltr_hip.h, with its conventions and the numerics of
 * include/ltr_linear_bf16.h: X holds bf16 values, (B, L, F) contiguous, 16-byte aligned; bf16 -> fp32 is exact; W,
 * bias, labels, n, scores, losses, partial rows and every product and sum are fp32.  Rows j >= n[b] of X are never
 * read (NaN there changes nothing).  Fixed summation order, no atomics: bit-identical run to run.  No allocation, no
 * synchronisation, no host read of n: the call records under stream capture.  Errors are decided on the host, before
 * any launch, in the order stated.
 */
#ifndef LTR_BF16_GENERAL_H
#define LTR_BF16_GENERAL_H

#include <stddef.h>
#include <stdint.h>

#include "ltr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * 1 where ltr_bf16_general_linear_partials takes (kind, B, L, F), 0 otherwise: one of the seven pairwise kinds, B > 0,
 * F % 8 == 0, F <= 1024, 0 < L <= ltr_max_list_len() (4096), and the query's LDS block -- the pair pass's, W, the
 * gradient vector and at least one row of the weight-gradient fold -- fits the CU.  It does for every such shape of six
 * kinds; LambdaNDCG2's pair pass keeps 36 bytes per document, and its block ends at 4084 documents at 8 features and at
 * 3884 at 1024.  The launch shape follows the batch size and the device's CU count, as the fp32
 * general kernel's does.
 */
int ltr_bf16_general_linear_plan(int kind, int B, int L, int F);

/*
 * The fused step, argument for argument ltr_linear_partials_bf16: loss[b], the per-query rows partials (B, partial
 * pitch of F) = [d loss[b] / dW | d loss[b] / d bias | zeros] -- sized by ltr_linear_workspace_bytes(B, L, F) and
 * consumed by every ltr_linear_reduce_* entry point -- and, when scores_out != NULL, scores_out[b, j] = the score for
 * j < n[b], 0 behind.  Every shape on the plan is taken, those of the register tile included.
 * Errors: LTR_ERR_KIND (kind, rel_dtype); LTR_ERR_SHAPE (B < 0, L <= 0, F <= 0, F % 8 != 0, F > 1024);
 * LTR_ERR_LIST_TOO_LONG (L > 4096); LTR_ERR_CONFIG for a shape off ltr_bf16_general_linear_plan (the LDS block does
 * not fit); B == 0 returns LTR_OK; LTR_ERR_NULL for X, W, rel, n, loss, partials.
 */
int ltr_bf16_general_linear_partials(int kind, float sigma, const uint16_t *X, const float *W, const float *bias,
                                     const void *rel, int rel_dtype, const int64_t *n, int B, int L, int F,
                                     float *loss, float *scores_out, float *partials, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LTR_BF16_GENERAL_H */
