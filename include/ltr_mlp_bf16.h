/*
 * ltr_mlp_bf16.h -- C ABI of the stand-alone ReLU-MLP scorer on a bf16 feature batch: scores and parameter gradients of
 *     Linear(F, H1) / ReLU / Linear(H1, H2) / ReLU / Linear(H2, 1)
 * over a (B, L, F) batch of ANY list length whose features are kept as bf16 in device memory (half the bytes of the
 * fp32 batch of include/ltr_mlp_rows.h), with the first layer on v_mfma_f32_16x16x32_bf16.
 *
 * Exported by the same libltr_hip.so as include/ltr_hip.h, with its conventions: device pointers owned by the
 * caller, work enqueued on `stream` without host synchronisation, 0 = OK, < 0 = LTR_ERR_* (ltr_hip.h),
 * > 0 = a hipError_t; n int64 clamped to [0, L], torch nn.Linear parameter layouts.
 */
#ifndef LTR_MLP_BF16_H
#define LTR_MLP_BF16_H

#include <stddef.h>
#include <stdint.h>

#include "ltr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The two calls of ltr_mlp_rows.h with one other operand type: X holds bf16 values (the upper 16 bits of an fp32, as
 * torch.bfloat16 stores them), (B, L, F) contiguous.  Parameters, g, scores and gradients are fp32: the parameters are
 * the fp32 master weights.
 *   NUMERICS.  The network computed is the fp32 one EXCEPT that W1 is rounded to bf16, round to nearest even, once
 *   per launch: scores = mlp(X; bf16(W1), b1, W2, b2, W3, b3), and the gradients are those of that function, dW1
 *   being the gradient with respect to the rounded W1 (a straight-through update of the master weights).  Products of
 *   layer 1 are exact (bf16 x bf16 fits fp32) and accumulate in fp32; H1, layers 2 and 3, biases and ReLUs are fp32.
 *   In the dW1 product X is exact and d loss / d H1 enters as a sum of two bf16 terms (relative error 2^-17).
 *   Network limits: F % 8 == 0 (every row starts on 16 bytes), 0 < F <= 224, 0 < H1 <= 64, 0 < H2 <= 16.
 *   Any L >= 1; B * L must fit an int.  Violations: LTR_ERR_SHAPE.  X and W1 must be 16-byte aligned.
 *   Rows j >= n[b] of X and entries j >= n[b] of g are never read (NaN there changes nothing); their scores are 0
 *   and they add nothing to the gradients.  n == NULL: every row is real.
 *   ltr_mlp_bf16_grad writes grads[ltr_mlp_param_count(F, H1, H2)] = [dW1 | db1 | dW2 | db2 | dW3 | db3] of
 *   sum_{b, j < n[b]} g[b, j] * s[b, j].  The activations are recomputed.  Every workgroup owns a fixed set of tiles of
 *   32 flat rows and writes one partial vector into the workspace, a second launch adds the partial vectors in a fixed
 *   order: no atomics, bit-identical run to run.
 *   ltr_mlp_bf16_grad_workspace_bytes: the partial vectors (0 for invalid arguments).
 *   No allocation, no synchronisation, no host read of n: both calls record under stream capture.
 *   Errors, decided on the host in this order: LTR_ERR_SHAPE; LTR_ERR_NULL for a parameter (or grads); B == 0
 *   writes no scores / zero gradients and returns LTR_OK; LTR_ERR_NULL for X, scores_out, g; LTR_ERR_WORKSPACE
 *   for a missing or short workspace.
 */
int ltr_mlp_bf16_scores(const uint16_t *X, const float *W1, const float *b1, const float *W2, const float *b2,
                        const float *W3, const float *b3, const int64_t *n, int B, int L, int F, int H1, int H2,
                        float *scores_out, void *stream);
size_t ltr_mlp_bf16_grad_workspace_bytes(int B, int L, int F, int H1, int H2);
int ltr_mlp_bf16_grad(const uint16_t *X, const float *W1, const float *b1, const float *W2, const float *b2,
                      const float *W3, const float *b3, const float *g, const int64_t *n, int B, int L, int F,
                      int H1, int H2, float *grads, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LTR_MLP_BF16_H */
