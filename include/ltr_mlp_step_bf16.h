/*
 * ltr_mlp_step_bf16.h -- C ABI of the fused training step of the ReLU-MLP scorer
 *     Linear(F, H1) / ReLU / Linear(H1, H2) / ReLU / Linear(H2, 1)
 * on a (B, L, F) batch whose features are kept as bf16 in device memory: scores, per-query losses and the six
 * parameter gradients by ONE MFMA launch plus the fixed-order reduction, for the seven pairwise losses, ListNet, ListMLE
 * and LambdaRank.  What ltr_mlp_pairwise_f32 (ltr_hip.h), ltr_mlp_listwise_f32 (ltr_listwise.h), ltr_mlp_lambdarank_f32
 * (ltr_mlp_lambdarank.h) and ltr_mlp_train_step_f32 (ltr_mlp_train.h) are to an fp32 batch, on the data path of
 * ltr_mlp_bf16.h: X stays bf16 from memory to v_mfma_f32_16x16x32_bf16.
 *
 * Exported by the same libltr_hip.so as include/ltr_hip.h, with its conventions: device pointers owned by the
 * caller, work enqueued on `stream` without host synchronisation, 0 = OK, < 0 = LTR_ERR_* (ltr_hip.h),
 * > 0 = a hipError_t; n int64 clamped to [0, L], torch nn.Linear parameter layouts.
 */
#ifndef LTR_MLP_STEP_BF16_H
#define LTR_MLP_STEP_BF16_H

#include <stddef.h>
#include <stdint.h>

#include "ltr_hip.h"
#include "ltr_mlp_train.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * `family` / `code` name the loss as ltr_mlp_train_step_f32 takes them: LTR_MLP_TRAIN_PAIRWISE with a kind LTR_HINGE ..
 * LTR_NDCG2, LTR_MLP_TRAIN_LISTWISE with LTR_LISTWISE_LISTNET / _LISTMLE, LTR_MLP_TRAIN_LAMBDARANK (code ignored).
 * sigma: the pairwise kinds and LambdaRank; k: ListMLE and LambdaRank (<= 0: no cutoff); tie, use_seed, seed, seed_dev:
 * the tie arguments of ltr_mlp_listwise_f32 (ListMLE only).  X: bf16 values (the upper 16 bits of an fp32, as
 * torch.bfloat16 stores them), (B, L, F) contiguous, 16-byte aligned.  Parameters, losses, scores and gradients are
 * fp32: the parameters are the fp32 master weights.  rel, rel_dtype, n, grad_out (NULL: 1 / B), loss[B], scores_out
 * (may be NULL; (B, L), written for documents < n[b] only), grads[ltr_mlp_param_count], loss_sum (may be NULL): as in
 * the fp32 entry points.
 *   NUMERICS: those of ltr_mlp_bf16.h.  The network is the fp32 one EXCEPT that W1 is rounded to bf16, round to nearest
 *   even, once per workgroup: scores = mlp(X; bf16(W1), b1, W2, b2, W3, b3); the loss and the gradients are those of
 *   that function, dW1 being the gradient with respect to the rounded W1 (a straight-through update of the master
 *   weights).  Products of layer 1 are exact and accumulate in fp32; H1, layers 2 and 3, the loss and everything in
 *   the backward pass but the dW1 product are fp32.  In the dW1 product X is exact and d loss / d H1 enters as a sum of
 *   two bf16 terms (relative error 2^-17).
 *   LIMITS: the networks of ltr_mlp_bf16.h -- F % 8 == 0, 0 < F <= 224, 0 < H1 <= 64, 0 < H2 <= 16 (else
 *   LTR_ERR_SHAPE); L <= 128 (else LTR_ERR_LIST_TOO_LONG: the stand-alone kernels of ltr_mlp_bf16.h take any length);
 *   F <= 160 (wider rows are off the plan, LTR_ERR_CONFIG: their kernels would not keep two workgroups per CU).
 *   Rows j >= n[b] of X are never read (NaN there changes nothing).  No atomics: bit-identical run to run.  No
 *   allocation, no host read of n: the call records under stream capture.
 *   ltr_mlp_step_bf16_plan: 1 where the step takes (family, code, B, L, F, H1, H2) -- the limits above and the loss
 *   slot's LDS next to the network's -- else 0 (also B == 0, an unknown family or code).
 *   ltr_mlp_step_bf16_workspace_bytes: one partial vector per workgroup (0 for invalid arguments).
 *   Errors, decided on the host in this order: LTR_ERR_KIND (family, code, label dtype), LTR_ERR_SHAPE (the network,
 *   a LambdaRank sigma that is not finite), LTR_ERR_LIST_TOO_LONG, LTR_ERR_NULL for a parameter or grads; B == 0
 *   zeroes grads (and loss_sum) and returns LTR_OK; LTR_ERR_NULL for X, rel, n, loss; LTR_ERR_WORKSPACE;
 *   LTR_ERR_CONFIG for a shape off the plan.
 */
int ltr_mlp_step_bf16_plan(int family, int code, int B, int L, int F, int H1, int H2);
size_t ltr_mlp_step_bf16_workspace_bytes(int B, int F, int H1, int H2);
int ltr_mlp_step_bf16(int family, int code, int k, float sigma, const uint16_t *X, const float *W1, const float *b1,
                      const float *W2, const float *b2, const float *W3, const float *b3, const void *rel, int rel_dtype,
                      const int64_t *n, const int32_t *tie, int use_seed, uint64_t seed, const int64_t *seed_dev,
                      const float *grad_out, int B, int L, int F, int H1, int H2, float *loss, float *scores_out,
                      float *grads, float *loss_sum, void *workspace, size_t workspace_bytes, void *stream);

/*
 * ltr_mlp_train_step_f32 on a bf16 batch: the MFMA launch of ltr_mlp_step_bf16, then the reduce-and-update launch of
 * ltr_mlp_train.h.  Arguments, update rules, state and errors are ltr_mlp_train_step_f32's, with the limits above in the
 * place of the fp32 step's; W1_rows (where w1_pitch < F) is the fp32 W1 zero-padded to F columns.
 */
int ltr_mlp_train_step_bf16(int family, int code, int k, float sigma, const uint16_t *X, float *W1, float *b1, float *W2,
                            float *b2, float *W3, float *b3, int w1_pitch, const float *W1_rows, const void *rel,
                            int rel_dtype, const int64_t *n, const int32_t *tie, int use_seed, uint64_t seed,
                            const int64_t *seed_dev, const float *grad_out, int B, int L, int F, int H1, int H2,
                            float *loss, float *scores_out, float *loss_sum, float *state,
                            const struct ltr_mlp_optim *optim, float *grads_out, void *workspace,
                            size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LTR_MLP_STEP_BF16_H */
