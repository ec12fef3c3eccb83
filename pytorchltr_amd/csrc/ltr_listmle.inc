// ltr_listmle.inc -- ListMLE, the Plackett-Luce listwise loss (included by ltr_kernels.hip after ltr_eval.inc;
// C ABI: include/ltr_listwise.h).
//
// One ranking by label, then two linear scans over the ranked scores x_i = s[pi(i)]:
//   1. the suffix (max, sum) scan: (M_i, S_i) with S_i = sum_{m >= i} exp(x_m - M_i), M_i = max_{m >= i} x_m, so
//      LSE_i = M_i + log S_i.  The pair is kept as (M_i, log S_i): LSE_i - x_i = (M_i - x_i) + log S_i loses nothing
//      to a large common shift of the scores.
//   2. the gradient scan: D_i = [i < K] + D_{i-1} exp(LSE_i - LSE_{i-1}) (D_{-1} = 0), an affine recurrence
//      D_i = a_i D_{i-1} + b_i scanned as the composition of the maps (a_i, b_i); D_i <= i + 1, every a_i <= 1.  Then
//      dscores[pi(i)] = exp(x_i - LSE_i) D_i - [i < K].
// Both scans are one pass per thread over a contiguous chunk, then block_pair_scan of the chunk aggregates (the ranked-row
// core's pair scan, ltr_ranked.inc); every sum runs in a fixed order (no atomics): bit-identical run to run.
//
// Up to kMaxListLen documents: listmle_kernel, one workgroup per query on the ranked-row core: its launch shape, its
// ranking (with the labels in the score slot) and its LDS layout; the row itself is listmle_row (ltr_listmle_row.inc), which the fused
// Linear step (ltr_linear_listwise.inc) and the fused MLP step (ltr_mlp_listwise.inc) run on scores they have just computed.
// Longer lists (and every list under ltr_debug_long_sort_all): the long path's key sort on label keys with the call's
// tie words (long_sort<KEY_LABELS_TIED>), then per tile of kEpiTile ranks:
//   1. listmle_long_gather_kernel: the ranked scores x_r, and the tile's (max, sum) aggregate;
//   2. listmle_long_lse_kernel: the aggregates of the tiles after it combined in a fixed order, the in-tile suffix
//      scan -> (M_r, log S_r), and the tile's loss partial;
//   3. listmle_long_affine_kernel (gradient only): the tile's composed map (a, b);
//   4. listmle_long_grad_kernel (gradient only): the maps of the tiles before it composed in order, the in-tile scan,
//      dscores scattered through the ranking;
//   5. listmle_long_finish_kernel, per query: the loss partials added in a fixed order.
// All memory is the caller's workspace: capturable.

#include "ltr_listwise.h"
#include "ltr_listmle_row.inc"

namespace {

struct ListMLEParams {
    MetricParams m;          // the batch and the tie words (m.scores, m.out unused: scores below)
    const float *scores;
    float *loss, *dscores;   // (B), (B, L) or null
    int k;                   // <= 0: every factor
};

// (the launch bounds, and so the register budgets, of the ranked-row core's kernels: same shapes, same occupancy)
template <int DPT>
__global__ void __launch_bounds__(1024, (DPT <= 0 ? 8 : 4))
listmle_kernel(ListMLEParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const MetricParams &m = p.m;
    const int b = blockIdx.x;
    const int L = m.L;
    const int tid = threadIdx.x;
    const int T = blockDim.x;
    const int nb = clamp_n(m.n[b], L);
    const int K = p.k > 0 ? min(p.k, nb) : nb;

    // the core's LDS layout, with (label, score) pairs where the metrics keep (score, label): metric_ranks ranks the x slot
    const RankedRowLds q = ranked_row_lds(smem, L, DPT <= 0);
    const size_t row = (size_t)b * L;
    for (int j = tid; j < nb; j += T) q.sy[j] = make_float2(load_label(m.rel, m.rel_dtype, row + j), p.scores[row + j]);
    listmle_row<DPT>(m, q, nb, K, p.loss + b, p.dscores != nullptr);
    if (!p.dscores) return;
    for (int j = tid; j < L; j += T) p.dscores[row + j] = j < nb ? q.curve[q.rank_s[j]] : 0.f;
}

// ---- the sort path ----
struct ListMLELongParams {
    LongKeyParams key;                       // label keys, the call's tie words
    const unsigned long long *sorted;        // (B, L)
    const float *scores;
    float *loss, *dscores;
    int k, B, tiles;                         // tiles per query: ceil(L / kEpiTile)
    float *xs, *mx, *ls;                     // (B, L): ranked scores, M_r, log S_r
    float2 *tagg, *taff;                     // (B, tiles): (max, sum) aggregates, composed maps
    float *tloss;                            // (B, tiles)
};

__device__ __forceinline__ int listmle_k(const ListMLELongParams &p, int nb) { return p.k > 0 ? min(p.k, nb) : nb; }

// 1. the ranked scores of the tile and their (max, sum) aggregate
__global__ void __launch_bounds__(kEpiThreads) listmle_long_gather_kernel(ListMLELongParams p)
{
    __shared__ float t[kEpiTile];
    __shared__ float pair[32];
    const EpiTile et = epi_tile(p.key, p.tiles);
    const int tid = threadIdx.x;
    for (int x = tid; x < et.real; x += kEpiThreads) {
        const float v = p.scores[et.base + long_doc(p.key, p.sorted[et.base + et.r0 + x], et.seed)];
        t[x] = v;
        p.xs[et.base + et.r0 + x] = v;
    }
    __syncthreads();
    float m = -INFINITY, s = 0.f, tm, ts;
    for (int e = 0; e < kEpiE; ++e) {
        const int x = tid * kEpiE + e;
        if (x < et.real) ms_add(m, s, t[x], 1.f);
    }
    block_pair_scan<MaxSum>(m, s, tm, ts, pair);
    if (tid == 0) p.tagg[(size_t)et.q * p.tiles + et.tile] = make_float2(tm, ts);
}

// 2. (M_r, log S_r) of the tile's ranks: the tiles after it first (in a fixed order), then the in-tile suffix scan
__global__ void __launch_bounds__(kEpiThreads) listmle_long_lse_kernel(ListMLELongParams p)
{
    __shared__ float t[kEpiTile];
    __shared__ float pair[32];
    __shared__ float red[32];
    const EpiTile et = epi_tile(p.key, p.tiles);
    const int tid = threadIdx.x;
    const int K = listmle_k(p, et.nb);
    for (int x = tid; x < et.real; x += kEpiThreads) t[x] = p.xs[et.base + et.r0 + x];
    // the tiles after this one: thread-contiguous runs of them, then the workgroup's combination
    const int after = max(0, min(p.tiles, (et.nb + kEpiTile - 1) / kEpiTile) - et.tile - 1);
    const int ach = (after + kEpiThreads - 1) / kEpiThreads;
    float im = -INFINITY, is = 0.f, inm, ins;
    for (int i = tid * ach; i < min(after, (tid + 1) * ach); ++i) {
        const float2 a = p.tagg[(size_t)et.q * p.tiles + et.tile + 1 + i];
        ms_add(im, is, a.x, a.y);
    }
    block_pair_scan<MaxSum>(im, is, inm, ins, pair);                   // (its barriers publish t)
    // the tile: thread t owns the reversed ranks [t kEpiE, (t + 1) kEpiE)
    float m = -INFINITY, s = 0.f, tm, ts;
    for (int e = 0; e < kEpiE; ++e) {
        const int x = et.real - 1 - (tid * kEpiE + e);
        if (x >= 0) ms_add(m, s, t[x], 1.f);
    }
    block_pair_scan<MaxSum>(m, s, tm, ts, pair);
    float rm = inm, rs = ins, acc = 0.f;
    ms_add(rm, rs, m, s);
    for (int e = 0; e < kEpiE; ++e) {
        const int x = et.real - 1 - (tid * kEpiE + e);
        if (x >= 0) {
            ms_add(rm, rs, t[x], 1.f);
            const float l = logf(rs);
            p.mx[et.base + et.r0 + x] = rm;
            p.ls[et.base + et.r0 + x] = l;
            if (et.r0 + x < K) acc += (rm - t[x]) + l;
        }
    }
    acc = block_sum(acc, red);
    if (tid == 0) p.tloss[(size_t)et.q * p.tiles + et.tile] = acc;
}

// the map (a_r, b_r) of rank r < nb (the arrays of listmle_long_lse_kernel)
__device__ __forceinline__ float2 listmle_long_map(const ListMLELongParams &p, size_t base, int r, int K)
{
    const float a = r > 0 ? lse_step(p.mx[base + r], p.ls[base + r], p.mx[base + r - 1], p.ls[base + r - 1]) : 0.f;
    return make_float2(a, r < K ? 1.f : 0.f);
}

// 3. the tile's composed map
__global__ void __launch_bounds__(kEpiThreads) listmle_long_affine_kernel(ListMLELongParams p)
{
    __shared__ float pair[32];
    const EpiTile et = epi_tile(p.key, p.tiles);
    const int tid = threadIdx.x;
    const int K = listmle_k(p, et.nb);
    float a = 1.f, b = 0.f, ta, tb;
    for (int e = 0; e < kEpiE; ++e) {
        const int x = tid * kEpiE + e;
        if (x < et.real) {
            const float2 f = listmle_long_map(p, et.base, et.r0 + x, K);
            aff_then(a, b, f.x, f.y);
        }
    }
    block_pair_scan<Affine>(a, b, ta, tb, pair);
    if (tid == 0) p.taff[(size_t)et.q * p.tiles + et.tile] = make_float2(ta, tb);
}

// 4. D_r of the tile's ranks (the maps of the tiles before it composed in order), dscores through the ranking
__global__ void __launch_bounds__(kEpiThreads) listmle_long_grad_kernel(ListMLELongParams p)
{
    __shared__ float pair[32];
    const EpiTile et = epi_tile(p.key, p.tiles);
    const int tid = threadIdx.x;
    const int K = listmle_k(p, et.nb);
    // padded documents sit at their own index past the real ones
    for (int x = et.real + tid; x < et.span; x += kEpiThreads) p.dscores[et.base + et.r0 + x] = 0.f;
    const int before = min(et.tile, (et.nb + kEpiTile - 1) / kEpiTile);
    const int bch = (before + kEpiThreads - 1) / kEpiThreads;
    float pa = 1.f, pb = 0.f, ta, tb;
    for (int i = tid * bch; i < min(before, (tid + 1) * bch); ++i) {
        const float2 f = p.taff[(size_t)et.q * p.tiles + i];
        aff_then(pa, pb, f.x, f.y);
    }
    block_pair_scan<Affine>(pa, pb, ta, tb, pair);
    const float din = tb;                                              // D at the end of the tiles before (D_{-1} = 0)
    float a = 1.f, b = 0.f, ea, eb;
    for (int e = 0; e < kEpiE; ++e) {
        const int x = tid * kEpiE + e;
        if (x < et.real) {
            const float2 f = listmle_long_map(p, et.base, et.r0 + x, K);
            aff_then(a, b, f.x, f.y);
        }
    }
    block_pair_scan<Affine>(a, b, ea, eb, pair);
    float d = __builtin_fmaf(a, din, b);
    for (int e = 0; e < kEpiE; ++e) {
        const int x = tid * kEpiE + e;
        if (x < et.real) {
            const int r = et.r0 + x;
            const float2 f = listmle_long_map(p, et.base, r, K);
            d = __builtin_fmaf(f.x, d, f.y);
            const float g = lse_prob(p.xs[et.base + r], p.mx[et.base + r], p.ls[et.base + r]) * d - f.y;
            p.dscores[et.base + long_doc(p.key, p.sorted[et.base + r], et.seed)] = g;
        }
    }
}

// 5. per query: the loss partials in a fixed order
__global__ void __launch_bounds__(kEpiThreads) listmle_long_finish_kernel(ListMLELongParams p)
{
    __shared__ float red[32];
    const int q = blockIdx.x, tid = threadIdx.x;
    float a = 0.f;
    for (int t = tid; t < p.tiles; t += kEpiThreads) a += p.tloss[(size_t)q * p.tiles + t];
    a = block_sum(a, red);
    if (tid == 0) p.loss[q] = a;
}

// ---- host side ----
// The workspace of ltr_listmle_workspace_bytes (include/ltr_listwise.h states the byte formula): the long path's keys
// and inverse tie map, three (B, L) float arrays, two (B, tiles) float2 and one float array, into p.
inline LongWorkspace listmle_long_workspace(Carver &c, int B, int L, ListMLELongParams &p)
{
    const LongWorkspace ws = long_workspace(c, B, L, false);
    const size_t BL = (size_t)B * (size_t)L, bt = (size_t)B * (size_t)long_epi_tiles(L);
    p.xs = c.take<float>(BL); c.align256();
    p.mx = c.take<float>(BL); c.align256();
    p.ls = c.take<float>(BL); c.align256();
    p.tagg = c.take<float2>(bt);
    p.taff = c.take<float2>(bt); c.align256();
    p.tloss = c.take<float>(bt);
    return ws;
}

int long_listmle(const float *scores, const void *rel, int rel_dtype, const int64_t *n, int k, const int32_t *tie,
                 int use_seed, uint64_t seed, const int64_t *seed_dev, int B, int L, float *loss, float *dscores,
                 void *workspace, size_t workspace_bytes, hipStream_t s)
{
    ListMLELongParams p{};
    Carver carver(workspace);
    const LongWorkspace ws = listmle_long_workspace(carver, B, L, p);
    if (!workspace || workspace_bytes < carver.off) return LTR_ERR_WORKSPACE;
    p.key = long_key_params(nullptr, rel, rel_dtype, n, tie, use_seed, seed, seed_dev, L, ws, s);
    p.scores = scores; p.loss = loss; p.dscores = dscores;
    p.k = k; p.B = B;
    p.tiles = long_epi_tiles(L);
    const size_t bt = (size_t)B * (size_t)p.tiles;
    p.sorted = long_sort<KEY_LABELS_TIED>(p.key, B, ws, nullptr, s);
    const dim3 grid((unsigned)bt), block(kEpiThreads);
    hipLaunchKernelGGL(listmle_long_gather_kernel, grid, block, 0, s, p);
    hipLaunchKernelGGL(listmle_long_lse_kernel, grid, block, 0, s, p);
    if (dscores) {
        hipLaunchKernelGGL(listmle_long_affine_kernel, grid, block, 0, s, p);
        hipLaunchKernelGGL(listmle_long_grad_kernel, grid, block, 0, s, p);
    }
    hipLaunchKernelGGL(listmle_long_finish_kernel, dim3((unsigned)B), block, 0, s, p);
    return (int)hipGetLastError();
}

int launch_listmle(const ListMLEParams &p0, hipStream_t stream)
{
    ListMLEParams p = p0;
    const MetricShape sh = metric_shape(p.m);
    return launch_ranked(sh, p.m.B, 0, stream, p, [](auto D) { return &listmle_kernel<decltype(D)::value>; });
}

}  // namespace

extern "C" {

size_t ltr_listmle_workspace_bytes(int B, int L)
{
    if (check_lists(B, L, kMaxSortListLen) != LTR_OK) return 0;
    if (!long_path(L)) return 0;
    ListMLELongParams p{};
    Carver sizes(nullptr);
    listmle_long_workspace(sizes, B, L, p);
    return sizes.off;
}

int ltr_listmle_f32(const float *scores, const void *rel, int rel_dtype, const int64_t *n, int k, const int32_t *tie,
                    int use_seed, uint64_t seed, const int64_t *seed_dev, int B, int L, float *loss, float *dscores,
                    void *workspace, size_t workspace_bytes, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (bad_label_dtype(rel_dtype)) return LTR_ERR_KIND;
    if (const int rc = check_lists(B, L, kMaxSortListLen)) return rc;
    if (B == 0) return LTR_OK;
    if (!scores || !rel || !n || !loss) return LTR_ERR_NULL;
    const hipStream_t s = (hipStream_t)stream;
    if (long_path(L))
        return long_listmle(scores, rel, rel_dtype, n, k, tie, use_seed, seed, seed_dev, B, L, loss, dscores, workspace,
                            workspace_bytes, s);
    ListMLEParams p{};
    p.m.rel = rel; p.m.n = n; p.m.B = B; p.m.L = L; p.m.rel_dtype = rel_dtype;
    set_tie(p.m, tie, use_seed, seed, seed_dev);
    p.scores = scores; p.loss = loss; p.dscores = dscores; p.k = k;
    return launch_listmle(p, s);
}

}  // extern "C"
