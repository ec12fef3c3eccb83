/*
 * ltr_lambdarank_long.h -- C ABI of LambdaRank (include/ltr_lambdarank.h) on lists longer than ltr_max_list_len()
 * documents.
 *
 * Exported by the same libltr_hip.so as include/ltr_hip.h, with its conventions: device pointers owned by the
 * caller, work enqueued on `stream` without host synchronisation, 0 = OK, < 0 = LTR_ERR_* (ltr_hip.h),
 * > 0 = a hipError_t; scores fp32, labels int64 / int32 / fp32 by `rel_dtype`, n int64 clamped to [0, L].
 */
#ifndef LTR_LAMBDARANK_LONG_H
#define LTR_LAMBDARANK_LONG_H

#include <stddef.h>
#include <stdint.h>

#include "ltr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ltr_lambdarank_f32 (ltr_lambdarank.h: the same loss[b], the same dscores, dscores may be NULL) without its bound of
 * ltr_max_list_len() = 4096 documents.  The loss is exactly the one ltr_lambdarank.h specifies: ranks by fp32 score,
 * descending, ties by document index (no tie mode, no seed); K_b = n_b for k <= 0, else min(k, n_b); d(r), the float
 * gain formula, maxDCG == 0 -> 1, w_ij, the stable softplus; the ranking and the weights are constants of the gradient.
 *   L <= ltr_max_list_len(): the call IS ltr_lambdarank_f32 (workspace unused, may be NULL; the size query returns
 *   0) -- the convention of ltr_pairwise_loss_long_f32 (ltr_longpair.h).
 *   Longer lists, up to ltr_max_pair_list_len() = 65 536 for every k (one bound: ranks and counts stay exact in fp32,
 *   and the case without a cutoff stays at the pairwise long path's 4.3e9 pair evaluations per query):
 *     the ranking from the long key sort (ties in document-index order), maxDCG@K_b from the label sort;
 *     (score, label) and (G, d) written BY RANK, d = 0 from rank K_b on;
 *     a query is cut into tiles of 1024 ranks, one workgroup each, which keeps its ranks in registers and streams
 *     the anchors [0, K_b) through LDS, 1024 at a time (the `owner_docs` and `chunk_docs` of ltr_long_pair_geometry,
 *     ltr_longpair.h: one geometry for both pair passes): the whole gradient of a rank >= K_b, the part within the top
 *     K_b of an anchor, and the loss of every pair, counted once by its lower-ranked member;
 *     the anchors' pairs with the tail [K_b, n_b) are those same evaluations with the other sign (what a pair gives
 *     one document it takes from the other), so they are spread over the tail as its tiles are: every tile that owns
 *     ranks of the tail leaves, per anchor, minus the sum of what its owners received, added within the workgroup in
 *     a fixed order, and these partial gradients are added afterwards in tile order;
 *     a finish kernel adds the loss partials in tile order, scales the gradient by sigma / ln 2 once per rank and
 *     scatters it from rank to document.
 *   About K_b n_b pair evaluations per query with a cutoff, each pair once; WITHOUT one, or with a cutoff near n_b,
 *   the work is QUADRATIC, n_b^2, as for ltr_pairwise_loss_long_f32.
 *   Padded slots of scores and rel are never read; dscores is exactly 0 for j >= n_b; dscores == NULL is forward only
 *   and gives the same loss bits.  No atomics, every sum in a fixed order (per 1024 partners, then over those sums,
 *   then over tiles in tile order): bit-identical run to run.  No host synchronisation, nothing allocated: capturable.
 *   Workspace (caller's device memory, any contents), T = ceil(L / 1024), A(x) = x rounded up to a multiple of 256,
 *   Kc = k for 0 < k < L, else 0 (no tail: every document is an anchor):
 *     ltr_lambdarank_long_workspace_bytes(k, B, L) = ltr_sort_workspace_bytes(1, B, L)    (the sort, the maxDCG partials)
 *       + 2 A(8 B L)                                             ((score, label) and (G, d) by rank)
 *       + 2 A(4 B L)                                             (the document behind each rank; the gradient by rank)
 *       + A(4 B T)                                               (the loss partials)
 *       + A(4 B Kc (T - floor(Kc / 1024)))                       (the anchors' partial gradients per tile of the tail);
 *     0 for L <= ltr_max_list_len() and for invalid arguments.
 *   Errors, in this order, all decided on the host before any launch: LTR_ERR_KIND for a bad rel_dtype; LTR_ERR_SHAPE
 *   for B < 0, L <= 0 or a sigma that is not finite; LTR_ERR_LIST_TOO_LONG for L > ltr_max_pair_list_len(); B == 0 is
 *   a no-op; LTR_ERR_NULL (scores, rel, n, loss); LTR_ERR_WORKSPACE for a missing or short workspace on the long path;
 *   then the sticky device status (ltr_device_status).
 */
size_t ltr_lambdarank_long_workspace_bytes(int k, int B, int L);
int ltr_lambdarank_long_f32(const float *scores, const void *rel, int rel_dtype, const int64_t *n,
                            int k, float sigma, int B, int L,
                            float *loss, float *dscores /* may be NULL */,
                            void *workspace, size_t workspace_bytes, void *stream);
/* Tests only: != 0 makes ltr_lambdarank_long_f32 (and its size query) take the long path at every L >= 1;
 * returns the old value. */
LTR_DEBUG_HOOK int ltr_debug_lambdarank_long_all(int on);

#ifdef __cplusplus
}
#endif
#endif /* LTR_LAMBDARANK_LONG_H */
