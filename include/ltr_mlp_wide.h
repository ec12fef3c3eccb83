/*
 * ltr_mlp_wide.h -- C ABI of the ReLU-MLP scorer on WIDE feature rows: scores and parameter gradients of
 *     Linear(F, H1) / ReLU / Linear(H1, H2) / ReLU / Linear(H2, 1)
 * over a (B, L, F) feature batch of any list length, for up to 704 features (Yahoo-shaped rows: 699 -> 700).
 * The wide-row counterpart of include/ltr_mlp_rows.h (which stops at 224 features, where a wave's W1 fragments and its
 * dW1 tile still fit its registers): the kernels here walk the feature dimension in chunks.
 *
 * Exported by the same libltr_hip.so as include/ltr_hip.h, with its conventions: device pointers owned by the
 * caller, work enqueued on `stream` without host synchronisation, 0 = OK, < 0 = LTR_ERR_* (ltr_hip.h),
 * > 0 = a hipError_t; fp32 throughout, n int64 clamped to [0, L], torch nn.Linear parameter layouts.
 */
#ifndef LTR_MLP_WIDE_H
#define LTR_MLP_WIDE_H

#include <stddef.h>
#include <stdint.h>

#include "ltr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The contract of ltr_mlp_rows.h with another feature limit.  Both calls stream the flat (B * L, F) row matrix in
 * tiles of 32 consecutive rows through v_mfma_f32_16x16x4_f32 chains and know about queries only through the mask
 * `row % L < n[row / L]`.
 *   Network limits: F % 4 == 0, 0 < F <= 704, 0 < H1 <= 64, 0 < H2 <= 16.  (F <= 224 is accepted as well; the row
 *   kernels of ltr_mlp_rows.h are the faster route there.)
 *   Any L >= 1; B * L must fit an int.  Violations: LTR_ERR_SHAPE.
 *   Rows j >= n[b] of X and entries j >= n[b] of g are never read (NaN there changes nothing); their scores are 0
 *   and they add nothing to the gradients.  n == NULL: every row is real.
 *   ltr_mlp_wide_grad_f32 writes grads[ltr_mlp_param_count(F, H1, H2)] = [dW1 | db1 | dW2 | db2 | dW3 | db3] (the
 *   layout of ltr_mlp_pairwise_f32) of  sum_{b, j < n[b]} g[b, j] * s[b, j].  The activations are recomputed, nothing
 *   is kept between the two calls.  Two kernels: the first runs the network forward and backward down to
 *   d loss / d hidden-1 and leaves that tile in the workspace, 256 bytes per flat row; the second multiplies it with
 *   column slices of X (which it reads a second time) into dW1.  Every workgroup owns a fixed set of tiles and writes
 *   one partial vector into the workspace, further launches add the partial vectors in a fixed order: no atomics,
 *   bit-identical run to run.
 *   ltr_mlp_wide_grad_workspace_bytes: the partial vectors (they grow with B * L up to the size of a full persistent
 *   grid) plus 256 * B * L bytes (rounded up to whole tiles) of d loss / d hidden-1; 0 for invalid arguments.
 *   No allocation, no synchronisation, no host read of n: both calls record under stream capture.
 *   Errors, decided on the host in this order: LTR_ERR_SHAPE; LTR_ERR_NULL for a parameter (or grads); B == 0
 *   writes no scores / zero gradients and returns LTR_OK; LTR_ERR_NULL for X, scores_out, g; LTR_ERR_WORKSPACE
 *   for a missing or short workspace.
 */
int ltr_mlp_wide_scores_f32(const float *X, const float *W1, const float *b1, const float *W2, const float *b2,
                            const float *W3, const float *b3, const int64_t *n, int B, int L, int F, int H1, int H2,
                            float *scores_out, void *stream);
size_t ltr_mlp_wide_grad_workspace_bytes(int B, int L, int F, int H1, int H2);
int ltr_mlp_wide_grad_f32(const float *X, const float *W1, const float *b1, const float *W2, const float *b2,
                          const float *W3, const float *b3, const float *g, const int64_t *n, int B, int L, int F,
                          int H1, int H2, float *grads, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LTR_MLP_WIDE_H */
