/*
 * ltr_mlp_rows.h -- C ABI of the ReLU-MLP scorer on its own: scores and parameter gradients of
 *     Linear(F, H1) / ReLU / Linear(H1, H2) / ReLU / Linear(H2, 1)
 * over a (B, L, F) feature batch of ANY list length.  What ltr_linear_scores_f32 / ltr_linear_grad_f32 are to the
 * Linear(F, 1) scorer: the pieces every fused MLP step falls back to past its list-length limits
 * (ltr_mlp_max_list_len), and the two halves of pytorchltr_amd.fused.MLPScorer.
 *
 * Exported by the same libltr_hip.so as include/ltr_hip.h, with its conventions: device pointers owned by the
 * caller, work enqueued on `stream` without host synchronisation, 0 = OK, < 0 = LTR_ERR_* (ltr_hip.h),
 * > 0 = a hipError_t; fp32 throughout, n int64 clamped to [0, L], torch nn.Linear parameter layouts.
 */
#ifndef LTR_MLP_ROWS_H
#define LTR_MLP_ROWS_H

#include <stddef.h>
#include <stdint.h>

#include "ltr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * A document's score, and its share of the parameter gradients, depend on its own feature row and on the upstream
 * d loss / d score alone, so both kernels stream the flat (B * L, F) row matrix in tiles of 32 consecutive rows
 * through v_mfma_f32_16x16x4_f32 chains and know about queries only through the mask `row % L < n[row / L]`.
 *   Network limits (those of ltr_mlp_pairwise_f32): F % 4 == 0, 0 < F <= 224, 0 < H1 <= 64, 0 < H2 <= 16.
 *   Any L >= 1; B * L must fit an int.  Violations: LTR_ERR_SHAPE.
 *   Rows j >= n[b] of X and entries j >= n[b] of g are never read (NaN there changes nothing); their scores are 0
 *   and they add nothing to the gradients.  n == NULL: every row is real.
 *   ltr_mlp_rows_grad_f32 writes grads[ltr_mlp_param_count(F, H1, H2)] = [dW1 | db1 | dW2 | db2 | dW3 | db3] (the
 *   layout of ltr_mlp_pairwise_f32) of  sum_{b, j < n[b]} g[b, j] * s[b, j].  The activations are recomputed, nothing
 *   is kept between the two calls.  Every workgroup owns a fixed set of tiles and writes one partial vector into the
 *   workspace, a second launch adds the partial vectors in a fixed order: no atomics, bit-identical run to run.
 *   ltr_mlp_rows_grad_workspace_bytes: the partial vectors (0 for invalid arguments; grows with B * L up to the
 *   size of a full persistent grid).
 *   No allocation, no synchronisation, no host read of n: both calls record under stream capture.
 *   Errors, decided on the host in this order: LTR_ERR_SHAPE; LTR_ERR_NULL for a parameter (or grads); B == 0
 *   writes no scores / zero gradients and returns LTR_OK; LTR_ERR_NULL for X, scores_out, g; LTR_ERR_WORKSPACE
 *   for a missing or short workspace.
 */
int ltr_mlp_rows_scores_f32(const float *X, const float *W1, const float *b1, const float *W2, const float *b2,
                            const float *W3, const float *b3, const int64_t *n, int B, int L, int F, int H1, int H2,
                            float *scores_out, void *stream);
size_t ltr_mlp_rows_grad_workspace_bytes(int B, int L, int F, int H1, int H2);
int ltr_mlp_rows_grad_f32(const float *X, const float *W1, const float *b1, const float *W2, const float *b2,
                          const float *W3, const float *b3, const float *g, const int64_t *n, int B, int L, int F,
                          int H1, int H2, float *grads, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LTR_MLP_ROWS_H */
