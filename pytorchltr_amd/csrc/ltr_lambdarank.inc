// ltr_lambdarank.inc -- LambdaRank, the pairwise logistic loss weighted by the change of NDCG@k under a swap of the two
// documents (included by ltr_kernels.hip after ltr_linear_listwise.inc; C ABI: include/ltr_lambdarank.h; DESIGN.md 25).
//
// With r_j the rank of document j by score (ties by document index), K the cutoff, d(r) = 1 / log2(2 + r) for r < K
// and 0 from K on, G_j = (2^y_j - 1) / maxDCG@K:
//   loss[b] = sum_{y_i > y_j} |G_i - G_j| |d(r_i) - d(r_j)| log2(1 + exp(-sigma (s_i - s_j)))
// A pair with both members at ranks >= K has weight 0, so only pairs with a member among the K anchors -- the ranks
// below the cutoff -- are visited: about K n_b of them instead of n_b^2 / 2.  The row function lambdarank_row
// (ltr_lambdarank_row.inc) works in rank order on the ranked-row core's LDS layout:
//   ranks by score and by label (metric_ranks), maxDCG@K from the label ranks, (score, label) scattered into rank
//   order, then (G, d) by rank;
//   pass A: every thread owns ranks r (strided) and walks the anchors a < K in order: the whole gradient of a rank
//     >= K, the part within the top K of a rank < K; a pair's loss is added once, by its lower member;
//   pass B (K < n_b, gradient only): one wave per anchor, its lanes stride over the ranks [K, n_b) and a wave sum is
//     added to the anchor's gradient.  The anchor x tail pairs are evaluated twice -- the price of having no scatter
//     across threads.  With K = n_b pass B is empty and pass A is the full pass.
// The anchors' (score, label) and (G, d) are two float2 LDS arrays read at a wave-uniform index (a broadcast).  No
// atomics, every sum in a fixed order: bit-identical run to run.  lambdarank_kernel, one workgroup per query in the
// core's launch shapes, and the LambdaRank slot of linear_listwise_kernel (ltr_linear_listwise.inc) call the same row
// function in the same shape: their losses agree bit for bit.

#include "ltr_lambdarank.h"

namespace {

struct LambdaRankParams {
    MetricParams m;          // the batch (no tie words: document-index order; m.scores, m.out unused: scores below)
    const float *scores;
    float *loss, *dscores;   // (B), (B, L) or null
    int k;                   // <= 0: no cutoff
    float sigma;
};

// (the launch bounds, and so the register budgets, of the ranked-row core's kernels: same shapes, same occupancy)
template <int DPT>
__global__ void __launch_bounds__(1024, (DPT <= 0 ? 8 : 4))
lambdarank_kernel(LambdaRankParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const MetricParams &m = p.m;
    const int b = blockIdx.x;
    const int L = m.L;
    const int tid = threadIdx.x;
    const int T = blockDim.x;
    const int nb = clamp_n(m.n[b], L);
    const int K = p.k > 0 ? min(p.k, nb) : nb;

    const RankedRowLds q = ranked_row_lds(smem, L, DPT <= 0);
    const size_t row = (size_t)b * L;
    for (int j = tid; j < nb; j += T) q.sy[j] = make_float2(p.scores[row + j], load_label(m.rel, m.rel_dtype, row + j));
    lambdarank_row<DPT>(m, q, nb, K, p.sigma, p.loss + b, p.dscores != nullptr);
    if (!p.dscores) return;
    const float *gr = reinterpret_cast<const float *>(q.rank_y);
    for (int j = tid; j < L; j += T) p.dscores[row + j] = j < nb ? gr[q.rank_s[j]] : 0.f;
}

// The guards both entry points share, in the documented order up to the empty batch; `F`: the fused call's (1 otherwise).
inline int check_lambdarank(int rel_dtype, float sigma, int B, int L, int F)
{
    if (bad_label_dtype(rel_dtype)) return LTR_ERR_KIND;
    if (B < 0 || L <= 0 || F <= 0 || !std::isfinite(sigma)) return LTR_ERR_SHAPE;
    return L > kMaxListLen ? LTR_ERR_LIST_TOO_LONG : LTR_OK;
}

}  // namespace

extern "C" {

int ltr_lambdarank_f32(const float *scores, const void *rel, int rel_dtype, const int64_t *n, int k, float sigma, int B,
                       int L, float *loss, float *dscores, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (const int rc = check_lambdarank(rel_dtype, sigma, B, L, 1)) return rc;
    if (B == 0) return LTR_OK;
    if (!scores || !rel || !n || !loss) return LTR_ERR_NULL;
    LambdaRankParams p{};
    p.m.rel = rel; p.m.n = n; p.m.B = B; p.m.L = L; p.m.rel_dtype = rel_dtype;
    p.scores = scores; p.loss = loss; p.dscores = dscores; p.k = k; p.sigma = sigma;
    const MetricShape sh = metric_shape(p.m);
    return launch_ranked(sh, B, 0, (hipStream_t)stream, p, [](auto D) { return &lambdarank_kernel<decltype(D)::value>; });
}

int ltr_linear_lambdarank_plan(int B, int L, int F)
{
    if (B <= 0 || L <= 0 || F <= 0 || L > kMaxListLen || F % 4 != 0) return 0;
    MetricParams m{};
    m.B = B; m.L = L;
    LinearListwiseShape s;
    return linear_listwise_shape(kLossLambdaRank, m, F, s) ? 1 : 0;
}

int ltr_linear_lambdarank_partials_f32(int k, float sigma, const float *X, const float *W, const float *bias,
                                       const void *rel, int rel_dtype, const int64_t *n, int B, int L, int F,
                                       float *loss_out, float *scores_out, float *partials, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (const int rc = check_lambdarank(rel_dtype, sigma, B, L, F)) return rc;
    if (B == 0) return LTR_OK;
    if (!X || !W || !rel || !n || !loss_out || !partials) return LTR_ERR_NULL;
    if (!ltr_linear_lambdarank_plan(B, L, F) || (uintptr_t)X % 16 != 0 || (uintptr_t)partials % 16 != 0)
        return LTR_ERR_CONFIG;
    if (const int st = status_peek()) return st;           // a kernel of an earlier call gave up
    LinearListwiseParams p{};
    p.m.rel = rel; p.m.n = n; p.m.B = B; p.m.L = L; p.m.rel_dtype = rel_dtype;
    p.X = X; p.W = W; p.bias = bias; p.loss = loss_out; p.scores_out = scores_out; p.part = partials;
    p.F = F; p.k = k; p.sigma = sigma;
    return launch_linear_listwise<kLossLambdaRank>(p, (hipStream_t)stream);
}

}  // extern "C"
