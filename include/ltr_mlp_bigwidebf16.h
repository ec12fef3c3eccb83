/*
 * ltr_mlp_bigwidebf16.h -- C ABI of the stand-alone ReLU-MLP scorer with wide hidden layers on wide bf16 rows: scores
 * and parameter gradients of
 *     Linear(F, H1) / ReLU / Linear(H1, H2) / ReLU / Linear(H2, 1),   H1 <= 256, H2 <= 64, F <= 704
 * over a bf16 (B, L, F) feature batch of ANY list length.  The function and the conventions of
 * include/ltr_mlp_bigwide.h (whose kernels take fp32 rows), with the numerics of include/ltr_mlp_bf16.h; the published
 * MLP baselines (128-32, 256-64) on a bf16 split of Istella (220 -> 224 features) and Yahoo (699 -> 704) are the
 * networks this serves.
 *
 * Exported by the same libltr_hip.so as include/ltr_hip.h, with its conventions: device pointers owned by the
 * caller, work enqueued on `stream` without host synchronisation, 0 = OK, < 0 = LTR_ERR_* (ltr_hip.h),
 * > 0 = a hipError_t; n int64 clamped to [0, L], torch nn.Linear parameter layouts, fp32 parameters, scores and
 * gradients.
 */
#ifndef LTR_MLP_BIGWIDEBF16_H
#define LTR_MLP_BIGWIDEBF16_H

#include <stddef.h>
#include <stdint.h>

#include "ltr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * X holds bf16 values (the upper 16 bits of an fp32 word) and stays bf16 from memory to the matrix instruction.  The
 * kernels stream the flat (B * L, F) row matrix in tiles of 32 consecutive rows, one eight-wave workgroup per CU, the
 * feature dimension in chunks of 128 (four K = 32 steps of v_mfma_f32_16x16x32_bf16), and know about queries only
 * through the mask `row % L < n[row / L]`.
 *   Numerics: W1 (fp32 master weights) is rounded to bf16, nearest even, on its way into the first layer: the scores
 *   are those of the network with the rounded W1, accumulated in fp32; everything behind the first layer is fp32.
 *   dW1 is the gradient with respect to that rounded W1; d loss / d hidden-1 enters it as the two-term bf16 split
 *   hi + lo (relative error 2^-17).
 *   Network limits: F % 8 == 0 (a row is whole 16-byte pieces), 0 < F <= 704, 0 < H1 <= 256, 0 < H2 <= 64 -- the narrow
 *   rows of ltr_mlp_bigbf16_* and the small networks of ltr_mlp_widebf16_* included, on which the results agree with
 *   theirs to rounding.  Both entry points take the same range.  Any L >= 1; B * L must fit an int.  Violations:
 *   LTR_ERR_SHAPE.
 *   Rows j >= n[b] of X and entries j >= n[b] of g are never read (NaN there changes nothing); their scores are 0
 *   and they add nothing to the gradients.  n == NULL: every row is real.
 *   ltr_mlp_bigwidebf16_grad writes grads[ltr_mlp_param_count(F, H1, H2)] = [dW1 | db1 | dW2 | db2 | dW3 | db3] (the
 *   layout of ltr_mlp_pairwise_f32) of  sum_{b, j < n[b]} g[b, j] * s[b, j].  The activations are recomputed, nothing
 *   is kept between the two calls.  Two kernels: the forward and the backward down to d loss / d hidden-1, which goes
 *   to the workspace (16 ceil(H1 / 16) floats a row) next to one partial vector of the small sums per workgroup; then
 *   dW1 over (row range) x (column slice), one partial dW1 per row range.  Two further launches add the partial
 *   results in a fixed order: no atomics, bit-identical run to run.
 *   ltr_mlp_bigwidebf16_grad_workspace_bytes: the d hidden-1 rows (they grow with B * L) plus both sets of partial
 *   results (0 for invalid arguments).
 *   No allocation, no synchronisation, no host read of n: both calls record under stream capture.
 *   Errors, decided on the host in this order: LTR_ERR_SHAPE; LTR_ERR_NULL for a parameter (or grads); B == 0
 *   writes no scores / zero gradients and returns LTR_OK; LTR_ERR_NULL for X, scores_out, g; LTR_ERR_WORKSPACE
 *   for a missing or short workspace.
 */
int ltr_mlp_bigwidebf16_scores(const uint16_t *X, const float *W1, const float *b1, const float *W2, const float *b2,
                               const float *W3, const float *b3, const int64_t *n, int B, int L, int F, int H1, int H2,
                               float *scores_out, void *stream);
size_t ltr_mlp_bigwidebf16_grad_workspace_bytes(int B, int L, int F, int H1, int H2);
int ltr_mlp_bigwidebf16_grad(const uint16_t *X, const float *W1, const float *b1, const float *W2, const float *b2,
                             const float *W3, const float *b3, const float *g, const int64_t *n, int B, int L, int F,
                             int H1, int H2, float *grads, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LTR_MLP_BIGWIDEBF16_H */
