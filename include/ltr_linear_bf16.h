/*
 * ltr_linear_bf16.h -- C ABI of the Linear(F, 1) scorer on a bf16 feature batch: the streaming score and
 * weight-gradient kernels, the fused step (scores, pairwise loss, d loss / d score and the query's weight-gradient
 * row in one pass over the features) and the collate that makes such batches.  The features are kept as bf16 in
 * device memory: half the bytes of the fp32 batch of include/ltr_hip.h, on the one path of the library that feature
 * bytes limit.
 *
 * Exported by the same libltr_hip.so as include/ltr_hip.h, with its conventions: device pointers owned by the
 * caller, work enqueued on `stream` without host synchronisation, 0 = OK, < 0 = LTR_ERR_* (ltr_hip.h),
 * > 0 = a hipError_t; n int64 clamped to [0, L].
 *
 *   NUMERICS.  X holds bf16 values (the upper 16 bits of an fp32, as torch.bfloat16 stores them), (B, L, F)
 *   contiguous, 16-byte aligned.  bf16 -> fp32 is exact (a 16-bit shift); W, bias, labels, n, scores, losses, partial
 *   rows and gradients are fp32, and every product and sum is fp32: the result is the fp32 network on the values X
 *   holds, up to summation order.  No weight is rounded.
 *   F % 8 == 0 (every row starts on 16 bytes) and F <= 1024, else LTR_ERR_SHAPE; B * L must fit an int.
 *   Rows j >= n[b] of X are never read (NaN there changes nothing).
 *   No allocation, no synchronisation, no host read of n: every call records under stream capture.
 *   Errors are decided on the host, before any launch, in the order each entry point states.
 */
#ifndef LTR_LINEAR_BF16_H
#define LTR_LINEAR_BF16_H

#include <stddef.h>
#include <stdint.h>

#include "ltr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * scores[b, j] = X[b, j, :] . W + bias for j < n[b], 0 for the padded documents (ltr_linear_scores_f32 on bf16 rows).
 * bias == NULL: 0; n == NULL: every row is real.
 * Errors: LTR_ERR_SHAPE (B < 0, L <= 0, F <= 0, F % 8 != 0, F > 1024); B == 0 returns LTR_OK; LTR_ERR_NULL for X, W,
 * scores.
 */
int ltr_linear_scores_bf16(const uint16_t *X, const float *W, const float *bias, const int64_t *n, int B, int L,
                           int F, float *scores, void *stream);

/*
 * dW_db[F + 1] = [sum_{b, j < n[b]} g[b, j] X[b, j, :] | sum g[b, j]] (ltr_linear_grad_f32 on bf16 rows): one partial
 * vector per (query, chunk of 256 rows) in the workspace, added in a fixed order by a second launch: no atomics,
 * bit-identical run to run.  Entries j >= n[b] of g are never read.
 * ltr_linear_grad_workspace_bytes_bf16: the partial vectors (0 for invalid arguments or B == 0).
 * Errors: LTR_ERR_SHAPE; LTR_ERR_NULL for dW_db; B == 0 writes zeros and returns LTR_OK; LTR_ERR_NULL for X, g;
 * LTR_ERR_WORKSPACE for a missing or short workspace.
 */
size_t ltr_linear_grad_workspace_bytes_bf16(int B, int L, int F);
int ltr_linear_grad_bf16(const uint16_t *X, const float *g, const int64_t *n, int B, int L, int F, float *dW_db,
                         void *workspace, size_t workspace_bytes, void *stream);

/*
 * LTR_PLAN_REGISTER_TILE where ltr_linear_partials_bf16 takes (kind, B, L, F), LTR_PLAN_NONE otherwise: F % 8 == 0,
 * L <= 256, a query's rows fit 16 sweeps of a 512-thread workgroup (ceil(L / floor(512 / (F / 8))) <= 16) and its
 * LDS block 64 KiB.  That holds for every L <= 256 at F <= 224 and every L <= 128 at F <= 512, for all seven kinds;
 * a shape on the plan stays on it with a shorter list.
 */
int ltr_linear_bf16_plan(int kind, int B, int L, int F);

/*
 * The fused step of ltr_linear_partials_f32 on bf16 features, which cross HBM once: loss[b], the per-query rows
 * partials (B, partial pitch of F) = [d loss[b] / dW | d loss[b] / d bias | zeros] -- the layout of
 * ltr_linear_partials_f32, sized by ltr_linear_workspace_bytes(B, L, F) and consumed by every ltr_linear_reduce_*
 * entry point -- and, when scores_out != NULL, scores_out[b, j] = the score for j < n[b], 0 behind.
 * Errors: LTR_ERR_KIND (kind, rel_dtype); LTR_ERR_SHAPE (B < 0, L <= 0, F <= 0, F % 8 != 0, F > 1024);
 * LTR_ERR_LIST_TOO_LONG for a list longer than the plan takes at any F (L > 256); LTR_ERR_SHAPE for any other shape
 * off ltr_linear_bf16_plan; B == 0 returns LTR_OK; LTR_ERR_NULL for X, W, rel, n, loss, partials.
 */
int ltr_linear_partials_bf16(int kind, float sigma, const uint16_t *X, const float *W, const float *bias,
                             const void *rel, int rel_dtype, const int64_t *n, int B, int L, int F, float *loss,
                             float *scores_out, float *partials, void *stream);

/*
 * ltr_collate_pad_f32 (dense branch) with bf16 xs / out_x: ragged rows + offsets -> zero-padded (B, L, F), (B, L), n.
 * A copy: any F >= 1.  Errors as there.
 */
int ltr_collate_pad_bf16(const uint16_t *xs, const int64_t *ys, const int64_t *offsets, const int64_t *qidx,
                         const int64_t *sel, int Q, int B, int L, int F, uint16_t *out_x, int64_t *out_y,
                         int64_t *out_n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LTR_LINEAR_BF16_H */
