/*
 * ltr_eval.h -- C ABI of evaluate(): many ranking metrics of a batch from ONE ranking per query.
 *
 * Exported by the same libltr_hip.so as include/ltr_hip.h, with its conventions: device pointers owned by the
 * caller, work enqueued on `stream` without host synchronisation, 0 = OK, < 0 = LTR_ERR_* (ltr_hip.h),
 * > 0 = a hipError_t; scores fp32, labels int64 / int32 / fp32 by `rel_dtype`, n int64 clamped to [0, L].
 */
#ifndef LTR_EVAL_H
#define LTR_EVAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Metric ops.  A request is M (op, k) pairs; k = 0 means no cutoff (the whole list: k = L), k > L acts as k = L.
 * Ranks r start at 1; the ranking is that of ltr_rank_by_score_long_f32 in the same tie mode.
 *   LTR_EVAL_DCG, LTR_EVAL_NDCG: ltr_dcg_long_f32 with normalize 0 / 1 at the same k (k = 0: the last column of
 *     its curve), `use_exp` as there; labels of padded documents are counted, maxDCG == 0 -> 1.
 *   LTR_EVAL_ARP: ltr_arp_long_f32 (k ignored).
 * The others look at the real documents j < n[b] only.  A document is relevant iff its label >= relevance_level;
 * R = the number of relevant real documents; every one of them is 0 when R == 0 (and so when n[b] == 0):
 *   LTR_EVAL_MAP     sum over relevant ranks r <= k of (relevant documents in the top r) / r, divided by R
 *   LTR_EVAL_MRR     1 / (rank of the first relevant document), 0 when that rank is > k
 *   LTR_EVAL_P       relevant documents in the top min(k, n) divided by k
 *   LTR_EVAL_RECALL  relevant documents in the top k divided by R
 *   LTR_EVAL_ERR     sum over r <= k of (1 / r) R_r prod_{i < r} (1 - R_i),  R_i = (2^g - 1) / 2^gmax with
 *                    g = label clamped to [0, gmax], gmax = err_max_grade (Chapelle et al. 2009)
 */
enum ltr_eval_op {
    LTR_EVAL_DCG = 0,
    LTR_EVAL_NDCG = 1,
    LTR_EVAL_ARP = 2,
    LTR_EVAL_MAP = 3,
    LTR_EVAL_MRR = 4,
    LTR_EVAL_P = 5,
    LTR_EVAL_RECALL = 6,
    LTR_EVAL_ERR = 7
};
#define LTR_EVAL_MAX_METRICS 32

/*
 * out (M, B) fp32: out[i * B + b] = metric spec[2 i] at cutoff spec[2 i + 1] of query b.  `spec` is a HOST array of
 * M (op, k) int32 pairs; it is copied into the kernel arguments, so it may be freed when the call returns.
 * Tie modes as ltr_rank_by_score_long_f32: use_seed != 0 hashed words from `seed` (`seed_dev`, device int64[1],
 * overrides it when not NULL), else tie != NULL explicit priorities (L), else document-index order.  One ranking
 * per query serves all M metrics.
 *   L <= ltr_max_list_len(): one workgroup per query, one launch, no workspace (may be NULL).  Longer lists (up to
 *   ltr_max_sort_list_len()): the sort of ltr_dcg_long_f32 (the labels sorted too when an NDCG is requested), tile
 *   epilogues and a per-query finish, in the caller's workspace of ltr_eval_workspace_bytes(B, L, spec, M) bytes
 *   (0 where no workspace is needed, and for invalid arguments).  Fixed-order sums, no atomics, nothing allocated:
 *   bit-identical run to run, and capturable.
 *   Errors, in this order: LTR_ERR_KIND for a bad rel_dtype or an unknown op, LTR_ERR_SHAPE for M outside
 *   [1, LTR_EVAL_MAX_METRICS] or a k < 0, then B < 0 / L <= 0 (LTR_ERR_SHAPE), L > ltr_max_sort_list_len()
 *   (LTR_ERR_LIST_TOO_LONG); B == 0 is a no-op; LTR_ERR_NULL, then LTR_ERR_WORKSPACE on the long path.
 */
size_t ltr_eval_workspace_bytes(int B, int L, const int32_t *spec, int M);
int ltr_eval_f32(const float *scores, const void *rel, int rel_dtype, const int64_t *n, const int32_t *tie, int use_seed,
                 uint64_t seed, const int64_t *seed_dev, int B, int L, const int32_t *spec, int M, float relevance_level,
                 int use_exp, float err_max_grade, float *out, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LTR_EVAL_H */
