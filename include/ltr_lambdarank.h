/*
 * ltr_lambdarank.h -- C ABI of LambdaRank, the pairwise logistic loss weighted by the change of NDCG@k when the two
 * documents of a pair swap ranks (Burges et al. 2006; the objective behind LambdaMART), and of the Linear(F, 1)
 * scorer fused with it.
 *
 * Exported by the same libltr_hip.so as include/ltr_hip.h, with its conventions: device pointers owned by the
 * caller, work enqueued on `stream` without host synchronisation, 0 = OK, < 0 = LTR_ERR_* (ltr_hip.h),
 * > 0 = a hipError_t; scores fp32, labels int64 / int32 / fp32 by `rel_dtype`, n int64 clamped to [0, L].
 */
#ifndef LTR_LAMBDARANK_H
#define LTR_LAMBDARANK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * LambdaRank of every query b, over its real documents j < n_b = clamp(n[b], 0, L):
 *   r_j: the 0-based rank of document j by score, descending; equal scores by document index (the rule of the
 *     Lambda losses of ltr_pairwise_loss_f32; there is no tie mode and no seed).
 *   K_b = n_b for k <= 0, else min(k, n_b).
 *   d(r) = 1 / log2(2 + r) for r < K_b, 0 for r >= K_b.
 *   g_j = 2^y_j - 1 (labels compared and exponentiated as fp32: a grade of -1 has the gain -0.5);
 *   maxDCG = sum_{r < K_b} g_(r) d(r) over the gains in descending label order; maxDCG == 0 -> 1;  G_j = g_j / maxDCG.
 *   w_ij = |G_i - G_j| |d(r_i) - d(r_j)|  = |NDCG@K_b - NDCG@K_b with i and j swapped|
 *   loss[b] = sum_{(i, j): y_i > y_j} w_ij log2(1 + exp(-sigma (s_i - s_j)))            (0 for n_b <= 1)
 *   The ranking and the weights are constants of the gradient: with
 *   lambda_ij = sigma w_ij / ln 2 * sigmoid(-sigma (s_i - s_j)) for every pair with y_i > y_j,
 *   dscores[b, i] -= lambda_ij, dscores[b, j] += lambda_ij;  0 for j >= n_b.
 * dscores may be NULL (forward only; the same loss bits).  The softplus never takes exp of a positive argument.  A
 * pair with both documents at ranks >= K_b has weight 0 and is not visited: about K_b n_b pairs are evaluated, not
 * n_b^2 / 2.  Padded slots of scores and rel are never read.  One workgroup per query, one launch, no workspace, up to
 * ltr_max_list_len() documents.  No atomics, every sum in a fixed order: bit-identical run to run.  Nothing is
 * allocated: capturable.
 *   Errors, in this order, all decided on the host before any launch: LTR_ERR_KIND for a bad rel_dtype; LTR_ERR_SHAPE
 *   for B < 0, L <= 0 or a sigma that is not finite; LTR_ERR_LIST_TOO_LONG for L > ltr_max_list_len(); B == 0 is a
 *   no-op; LTR_ERR_NULL (scores, rel, n, loss).
 */
int ltr_lambdarank_f32(const float *scores, const void *rel, int rel_dtype, const int64_t *n,
                       int k, float sigma, int B, int L,
                       float *loss, float *dscores /* may be NULL */, void *stream);

/*
 * The Linear(F, 1) scorer fused with LambdaRank: ltr_linear_listwise_partials_f32 (ltr_listwise.h) with the row
 * function of ltr_lambdarank_f32 in its loss slot -- scores, loss, gradient and the per-query weight-gradient rows in
 * ONE launch, one workgroup per query.  X, W, bias, loss_out, scores_out (may be NULL) and partials are those of
 * ltr_linear_listwise_partials_f32: s[b, j] = X[b, j, :] . W + bias[0] for j < n_b (rows j >= n_b of X and rel are
 * never read), X (B, L, F) fp32 with F % 4 == 0 and 16-byte aligned, partials B rows of (F + 4) & ~3 floats, 16-byte
 * aligned, which ltr_linear_reduce_f32 / _bcast_f32 / _loss_f32 / _accum_f32 (ltr_hip.h) take;
 * ltr_linear_workspace_bytes(B, L, F) bytes are enough.  k and sigma as above.
 *   Both calls run one row function in one launch shape, so loss_out equals ltr_lambdarank_f32 on scores_out bit for
 *   bit.  No atomics, every sum in a fixed order: bit-identical run to run.  Nothing is allocated: capturable.
 * ltr_linear_lambdarank_plan: 1 where the fused kernel takes (B, L, F), else 0: B, L or F <= 0,
 *   L > ltr_max_list_len(), F % 4 != 0, or the query's LDS (the ranked row, W, the cross-row buffer) does not fit.
 *   Errors, in this order, all decided on the host before any launch: LTR_ERR_KIND for a bad rel_dtype; LTR_ERR_SHAPE
 *   for B < 0, L <= 0, F <= 0 or a sigma that is not finite; LTR_ERR_LIST_TOO_LONG for L > ltr_max_list_len();
 *   B == 0 is a no-op; LTR_ERR_NULL (X, W, rel, n, loss_out, partials); LTR_ERR_CONFIG for a shape the plan declines or
 *   X / partials not 16-byte aligned; then the sticky device status (ltr_device_status).
 */
int ltr_linear_lambdarank_plan(int B, int L, int F);
int ltr_linear_lambdarank_partials_f32(int k, float sigma, const float *X, const float *W,
                       const float *bias, const void *rel, int rel_dtype, const int64_t *n,
                       int B, int L, int F,
                       float *loss_out, float *scores_out, float *partials, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LTR_LAMBDARANK_H */
