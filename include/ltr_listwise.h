/*
 * ltr_listwise.h -- C ABI of ListMLE, the Plackett-Luce listwise loss (Xia et al. 2008; top-k: Xia et al. 2009), and
 * of the Linear(F, 1) scorer and the MLP scorer fused with the two listwise losses, ListNet and ListMLE.
 *
 * Exported by the same libltr_hip.so as include/ltr_hip.h, with its conventions: device pointers owned by the
 * caller, work enqueued on `stream` without host synchronisation, 0 = OK, < 0 = LTR_ERR_* (ltr_hip.h),
 * > 0 = a hipError_t; scores fp32, labels int64 / int32 / fp32 by `rel_dtype`, n int64 clamped to [0, L].
 */
#ifndef LTR_LISTWISE_H
#define LTR_LISTWISE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ListMLE of every query b, over its real documents j < n_b = clamp(n[b], 0, L):
 *   pi orders them by label, descending (labels compared as fp32); equal labels by the tie mode of
 *   ltr_rank_by_score_long_f32: use_seed != 0 hashed words from `seed` (`seed_dev`, device int64[1], overrides it
 *   when not NULL; ltr_tie_hash_word up to ltr_max_list_len() documents, ltr_tie_hash_word_long above), else
 *   tie != NULL explicit priorities (L), else document-index order.  Every row shares the tie words.
 *   K_b = n_b for k <= 0, else min(k, n_b) (top-k ListMLE: the first K_b factors of the likelihood).
 *   LSE_m = log sum_{i = m}^{n_b - 1} exp(s[pi(i)])
 *   loss[b] = sum_{m < K_b} (LSE_m - s[pi(m)])                                  (0 for n_b <= 1)
 *   dscores[b, pi(i)] = -[i < K_b] + sum_{m <= min(i, K_b - 1)} exp(s[pi(i)] - LSE_m),  0 for j >= n_b
 * dscores may be NULL (forward only).  Every exp takes a non-positive argument: LSE comes from a running
 * (max, sum) suffix scan and the gradient from the affine recurrence C_i = [i < K_b] + C_{i-1} exp(LSE_i - LSE_{i-1}),
 * C_i <= i + 1.  Sums run in a fixed order, no atomics: bit-identical run to run for a fixed seed or tie mode.
 *   L <= ltr_max_list_len(): one workgroup per query, one launch, no workspace (may be NULL).  Longer lists (up to
 *   ltr_max_sort_list_len()), and every list under ltr_debug_long_sort_all: the long path's key sort on the labels,
 *   then tile epilogues, in the caller's workspace of ltr_listmle_workspace_bytes(B, L) bytes (0 where no workspace
 *   is needed, and for invalid arguments).  Nothing is allocated: capturable.
 *   Errors, in this order: LTR_ERR_KIND for a bad rel_dtype, then B < 0 / L <= 0 (LTR_ERR_SHAPE),
 *   L > ltr_max_sort_list_len() (LTR_ERR_LIST_TOO_LONG); B == 0 is a no-op; LTR_ERR_NULL (scores, rel, n, loss),
 *   then LTR_ERR_WORKSPACE on the long path.
 */
size_t ltr_listmle_workspace_bytes(int B, int L);
int ltr_listmle_f32(const float *scores, const void *rel, int rel_dtype, const int64_t *n, int k, const int32_t *tie,
                    int use_seed, uint64_t seed, const int64_t *seed_dev, int B, int L, float *loss, float *dscores,
                    void *workspace, size_t workspace_bytes, void *stream);

/*
 * The Linear(F, 1) scorer fused with a listwise loss: scores, loss, gradient and the per-query weight-gradient rows
 * in ONE launch, one workgroup per query.  The rows of a query are read twice, for the scores and for the
 * weight-gradient row; the second read is meant to hit the L2 / last-level cache (not measured yet).
 *   loss = LTR_LISTWISE_LISTNET: the listwise softmax cross-entropy of ltr_listwise_softmax_f32 (ltr_hip.h); k and
 *     the tie arguments are ignored.  LTR_LISTWISE_LISTMLE: ltr_listmle_f32 above, same k, same tie modes -- the
 *     same row function, so loss_out equals ltr_listmle_f32 on the scores of this call bit for bit.
 *   s[b, j] = X[b, j, :] . W + bias[0] (bias may be NULL: 0) for j < n_b; rows j >= n_b of X and rel are never read.
 *   X (B, L, F) fp32 with F % 4 == 0, 16-byte aligned; W (F).
 *   loss_out (B); scores_out (B, L) or NULL: s[b, j], 0 for j >= n_b (the convention of ltr_linear_scores_f32 with n).
 *   partials: B rows of (F + 4) & ~3 floats, 16-byte aligned: [d loss[b] / dW_0 .. dW_{F-1} | d loss[b] / d bias |
 *     zeros] -- the per-query rows ltr_linear_reduce_f32 / _bcast_f32 / _loss_f32 / _accum_f32 (ltr_hip.h) take;
 *     ltr_linear_workspace_bytes(B, L, F) bytes are enough.  A query with n_b = 0 gets a row of zeros and loss 0.
 *   No atomics, every sum in a fixed order: bit-identical run to run for a fixed tie mode.  Nothing is allocated:
 *   capturable.
 * ltr_linear_listwise_plan: 1 where the fused kernel takes (loss, B, L, F), else 0: a bad loss, B, L or F <= 0,
 *   L > ltr_max_list_len(), F % 4 != 0, or the query's LDS (the ranked row, W, the cross-row buffer) does not fit.
 *   Errors, in this order: LTR_ERR_KIND for a bad loss or rel_dtype, then B < 0 / L <= 0 / F <= 0 (LTR_ERR_SHAPE),
 *   L > ltr_max_list_len() (LTR_ERR_LIST_TOO_LONG); B == 0 is a no-op; LTR_ERR_NULL (X, W, rel, n, loss_out,
 *   partials), LTR_ERR_CONFIG for a shape the plan declines or X / partials not 16-byte aligned, then the sticky
 *   device status (ltr_device_status).
 */
enum { LTR_LISTWISE_LISTNET = 0, LTR_LISTWISE_LISTMLE = 1 };
int ltr_linear_listwise_plan(int loss, int B, int L, int F);
int ltr_linear_listwise_partials_f32(int loss, int k, const float *X, const float *W, const float *bias,
                                     const void *rel, int rel_dtype, const int64_t *n, const int32_t *tie, int use_seed,
                                     uint64_t seed, const int64_t *seed_dev, int B, int L, int F, float *loss_out,
                                     float *scores_out, float *partials, void *stream);

/*
 * The guide's MLP scorer, Linear(F, H1) / ReLU / Linear(H1, H2) / ReLU / Linear(H2, 1), fused with a listwise loss:
 * the training step of ltr_mlp_pairwise_f32 (ltr_hip.h) with ListNet or ListMLE in the loss slot of the same two f32
 * MFMA kernels -- scores, per-query losses and the gradient of sum_b weight[b] * loss[b] w.r.t. all six parameter
 * tensors in one launch plus the cross-workgroup reduction.  Conventions, parameter layout and workspace are those of
 * ltr_mlp_pairwise_f32: ltr_mlp_param_count(F, H1, H2) floats of `grads` as [dW1 | db1 | dW2 | db2 | dW3 | db3],
 * ltr_mlp_workspace_bytes(B, F, H1, H2) bytes of workspace, weight[b] = grad_out[b] or 1 / B for grad_out == NULL,
 * loss_sum (may be NULL) = sum_b loss[b] written by the reduction launch, scores_out (may be NULL) valid for j < n_b.
 *   loss = LTR_LISTWISE_LISTNET: the listwise softmax cross-entropy of ltr_listwise_softmax_f32; k and the tie
 *     arguments are ignored; a query with n_b = 0 has loss 0 and a zero gradient.  LTR_LISTWISE_LISTMLE:
 *     ltr_listmle_f32 above -- the same row function, same k ("first K factors"), same tie modes (seed, device seed,
 *     explicit priorities, index order); n_b <= 1 gives loss 0 and a zero gradient.  The scans are chunked by the
 *     workgroup size (256 or 512 threads), so the loss agrees with ltr_listmle_f32 on scores_out to rounding, not bit
 *     for bit.  Rows j >= n_b of X and rel never reach a result.
 *   Shapes: F % 4 == 0, F <= 224, H1 <= 64, H2 <= 16; L <= 256 for F <= 144 (the 4-wave tile layout), L <= 128 above
 *     (the 8-wave layout).  ltr_debug_mlp_layout steers the layout as it does for ltr_mlp_pairwise_f32.
 *   No atomics on floats, every sum in a fixed order: bit-identical run to run for a fixed tie mode.  Nothing is
 *   allocated: capturable.
 * ltr_mlp_listwise_plan: 1 where the fused kernels take (loss, B, L, F, H1, H2), else 0: a bad loss, B, L, H1 or
 *   H2 <= 0, H1 > 64, H2 > 16, F <= 0, F % 4 != 0, F > 224, L past the layout's longest list, or the LDS of a layout
 *   the call may run on (its static part plus the ranked row) does not fit.
 *   Errors, in this order: LTR_ERR_KIND for a bad loss or rel_dtype, then LTR_ERR_SHAPE (B < 0, L / F / H1 / H2 <= 0,
 *   F % 4 != 0, F > 224, H1 > 64, H2 > 16), LTR_ERR_LIST_TOO_LONG; B == 0 is a no-op (nothing is written);
 *   LTR_ERR_NULL (X, the six parameters, rel, n, loss_out, grads), LTR_ERR_WORKSPACE, then LTR_ERR_CONFIG for a shape
 *   the plan declines.
 */
int ltr_mlp_listwise_plan(int loss, int B, int L, int F, int H1, int H2);
int ltr_mlp_listwise_f32(int loss, int k, const float *X, const float *W1, const float *b1, const float *W2,
                         const float *b2, const float *W3, const float *b3, const void *rel, int rel_dtype,
                         const int64_t *n, const int32_t *tie, int use_seed, uint64_t seed, const int64_t *seed_dev,
                         const float *grad_out, int B, int L, int F, int H1, int H2, float *loss_out, float *scores_out,
                         float *grads, float *loss_sum, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LTR_LISTWISE_H */
