/*
 * ltr_mlp_lambdarank.h -- C ABI of the guide's MLP scorer fused with LambdaRank (the loss of ltr_lambdarank.h).
 *
 * Exported by the same libltr_hip.so as include/ltr_hip.h, with its conventions: device pointers owned by the
 * caller, work enqueued on `stream` without host synchronisation, 0 = OK, < 0 = LTR_ERR_* (ltr_hip.h),
 * > 0 = a hipError_t; labels int64 / int32 / fp32 by `rel_dtype`, n int64 clamped to [0, L].
 */
#ifndef LTR_MLP_LAMBDARANK_H
#define LTR_MLP_LAMBDARANK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Linear(F, H1) / ReLU / Linear(H1, H2) / ReLU / Linear(H2, 1) fused with LambdaRank: the training step of
 * ltr_mlp_listwise_f32 (ltr_listwise.h) with the row function of ltr_lambdarank_f32 (ltr_lambdarank.h) in the loss
 * slot of the same two f32 MFMA kernels -- scores, per-query losses and the gradient of sum_b weight[b] * loss[b]
 * w.r.t. all six parameter tensors in one launch plus the cross-workgroup reduction.  Conventions, parameter layout
 * and workspace are those of ltr_mlp_listwise_f32: ltr_mlp_param_count(F, H1, H2) floats of `grads` as
 * [dW1 | db1 | dW2 | db2 | dW3 | db3], ltr_mlp_workspace_bytes(B, F, H1, H2) bytes of workspace, weight[b] =
 * grad_out[b] or 1 / B for grad_out == NULL, loss_sum (may be NULL) = sum_b loss[b] written by the reduction launch,
 * scores_out (may be NULL) valid for j < n_b.
 *   The loss: ltr_lambdarank_f32 on the scores of this call -- ranks by score with equal scores in document-index
 *     order (no tie mode, no seed), K_b = n_b for k <= 0, else min(k, n_b), the NDCG@K_b swap weights, the ranking and
 *     the weights constants of the gradient; n_b <= 1 gives loss 0 and a zero gradient; a query without a positive gain
 *     has maxDCG 1.  The block sums run at the workgroup size of the MLP kernels (256 or 512 threads), so the loss
 *     agrees with ltr_lambdarank_f32 on scores_out to rounding, not bit for bit.  Rows j >= n_b of X and rel never
 *     reach a result.
 *   Shapes: F % 4 == 0, F <= 224, H1 <= 64, H2 <= 16; L <= 256 for F <= 144 (the 4-wave tile layout), L <= 128 above
 *     (the 8-wave layout).  ltr_debug_mlp_layout steers the layout as it does for ltr_mlp_pairwise_f32.
 *   No atomics on floats, every sum in a fixed order: bit-identical run to run.  Nothing is allocated: capturable.
 * ltr_mlp_lambdarank_plan: 1 where the fused kernels take (B, L, F, H1, H2), else 0: B, L, H1 or H2 <= 0, H1 > 64,
 *   H2 > 16, F <= 0, F % 4 != 0, F > 224, L past the layout's longest list, or the LDS of a layout the call may run on
 *   (its static part plus the ranked row) does not fit.
 *   Errors, in this order: LTR_ERR_KIND for a bad rel_dtype, then LTR_ERR_SHAPE (B < 0, L / F / H1 / H2 <= 0,
 *   F % 4 != 0, F > 224, H1 > 64, H2 > 16, a sigma that is not finite -- what ltr_lambdarank_f32 refuses),
 *   LTR_ERR_LIST_TOO_LONG; B == 0 is a no-op (nothing is written); LTR_ERR_NULL (X, the six parameters, rel, n,
 *   loss_out, grads), LTR_ERR_WORKSPACE, then LTR_ERR_CONFIG for a shape the plan declines.
 */
int ltr_mlp_lambdarank_plan(int B, int L, int F, int H1, int H2);
int ltr_mlp_lambdarank_f32(int k, float sigma, const float *X, const float *W1, const float *b1,
                           const float *W2, const float *b2, const float *W3, const float *b3,
                           const void *rel, int rel_dtype, const int64_t *n, const float *grad_out,
                           int B, int L, int F, int H1, int H2, float *loss_out, float *scores_out,
                           float *grads, float *loss_sum, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LTR_MLP_LAMBDARANK_H */
