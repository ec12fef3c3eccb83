/*
 * ltr_longpair.h -- C ABI of the seven pairwise losses on lists longer than ltr_max_list_len() documents.
 *
 * Exported by the same libltr_hip.so as include/ltr_hip.h, with its conventions: device pointers owned by the
 * caller, work enqueued on `stream` without host synchronisation, 0 = OK, < 0 = LTR_ERR_* (ltr_hip.h),
 * > 0 = a hipError_t; scores fp32, labels int64 / int32 / fp32 by `rel_dtype`, n int64 clamped to [0, L].
 */
#ifndef LTR_LONGPAIR_H
#define LTR_LONGPAIR_H

#include <stddef.h>
#include <stdint.h>

#include "ltr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ltr_pairwise_loss_f32 (ltr_hip.h: same kinds, same loss[b], same dscores, dscores may be NULL) without its bound
 * of ltr_max_list_len() = 4096 documents.  The reference bounds none of these losses.
 *   L <= ltr_max_list_len(): the call IS ltr_pairwise_loss_f32 (workspace unused, may be NULL; the size query
 *   returns 0) -- the convention of the ltr_*_long_f32 ranking entry points.
 *   Longer lists, up to ltr_max_pair_list_len() = 65 536: a query is cut into owner tiles of `owner_docs` documents
 *   (ltr_long_pair_geometry), one workgroup each; the workgroup keeps its documents in registers and streams all
 *   n[b] documents of the query through LDS, `chunk_docs` at a time, so every unordered pair is evaluated twice,
 *   once from each end: no atomics, every sum in a fixed order (per chunk, then over the chunks, then over the
 *   tiles in tile order) -- bit-identical run to run.  The rankings inside LambdaNDCG1 / 2 come from the long key
 *   sort of ltr_rank_by_score_long_f32 with ties in document-index order, maxDCG from the label sort.
 *   ltr_long_pair_geometry describes the pair pass of ltr_lambdarank_long_f32 (ltr_lambdarank_long.h) as well: its
 *   tiles of ranks are `owner_docs` wide and its anchors are streamed `chunk_docs` at a time.
 *   The work is QUADRATIC: L^2 pair evaluations per query, 4.3e9 at the bound, which also keeps ranks and pair
 *   counts exact in fp32.  Past the bound: ListMLE (ltr_listwise.h) and ListNet (ltr_listwise_softmax_f32) are
 *   O(L log L) / O(L) and take lists up to ltr_max_sort_list_len() / of any length.
 *   Workspace (caller's device memory, any contents), T = ceil(L / owner_docs), A(x) = x rounded up to a multiple
 *   of 256:
 *     ltr_pairwise_loss_long_workspace_bytes(kind, B, L) = A(4 B T)                         (the loss partials)
 *       + for LTR_NDCG1 / LTR_NDCG2:  A(8 B L) + ltr_sort_workspace_bytes(1, B, L)          (gain / rank pairs, the sort);
 *     0 for L <= ltr_max_list_len() and for invalid arguments.
 *   No host synchronisation, nothing allocated: capturable.
 *   Errors, in this order: LTR_ERR_KIND for a bad kind or rel_dtype, then B < 0 / L <= 0 (LTR_ERR_SHAPE),
 *   L > ltr_max_pair_list_len() (LTR_ERR_LIST_TOO_LONG); B == 0 is a no-op; LTR_ERR_NULL (scores, rel, n, loss), then
 *   LTR_ERR_WORKSPACE for a missing or short workspace on the long path.
 *   fp64 scores are not part of this: ltr_pairwise_loss_f64 keeps ltr_max_list_len_f64().
 */
int ltr_max_pair_list_len(void);
void ltr_long_pair_geometry(int *owner_docs, int *chunk_docs);
size_t ltr_pairwise_loss_long_workspace_bytes(int kind, int B, int L);
int ltr_pairwise_loss_long_f32(int kind, float sigma, const float *scores, const void *rel, int rel_dtype,
                               const int64_t *n, int B, int L, float *loss, float *dscores /* may be NULL */,
                               void *workspace, size_t workspace_bytes, void *stream);
/* Tests only: != 0 makes ltr_pairwise_loss_long_f32 (and its size query) take the long path at every L >= 1;
 * returns the old value. */
LTR_DEBUG_HOOK int ltr_debug_long_pairs_all(int on);

#ifdef __cplusplus
}
#endif
#endif /* LTR_LONGPAIR_H */
