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
// Both scans are one pass per thread over a contiguous chunk, a DPP wave scan of the chunk aggregates and one LDS hop
// across waves; every sum runs in a fixed order (no atomics): bit-identical run to run.
//
// Up to kMaxListLen documents: listmle_kernel, one workgroup per query in metric_kernel's launch shape (metric_shape),
// its ranking (metric_ranks, with the labels in the score slot) and LDS layout.
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

namespace {

// ---- the two scan operators ----
// (max, sum) pairs: (m, s) stands for s exp(m).  Commutative; no exp of a positive argument; (-inf, 0) is the identity.
__device__ __forceinline__ void ms_add(float &m, float &s, float m2, float s2)
{
    const float hi = fmaxf(m, m2), lo = fminf(m, m2);
    const float e = lo == -INFINITY ? 0.f : expf(lo - hi);
    s = m >= m2 ? s + s2 * e : s * e + s2;
    m = hi;
}

// affine maps D -> a D + b: (a, b) = (a1, b1) then (a2, b2).  Identity (1, 0).
__device__ __forceinline__ void aff_then(float &a, float &b, float a2, float b2)
{
    b = __builtin_fmaf(a2, b, b2);
    a = a * a2;
}

// the value of lane (lane - shift) within the DPP pattern CTRL, or `idle` where there is none
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_from(float idle, float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(idle), __float_as_int(v), CTRL, ROW_MASK, 0xF, false));
}

// Inclusive wave scans in lane order: row_shr 1, 2, 4, 8 within the rows of 16 lanes, then row_bcast15 / row_bcast31
// carry the rows' totals forward (rows 1, 3 take row 0, 2; rows 2, 3 take rows 0-1).
#define LTR_MS_STEP(CTRL, RM)                                                                                        \
    do {                                                                                                             \
        const float m2_ = dpp_from<CTRL, RM>(-INFINITY, m), s2_ = dpp_from<CTRL, RM>(0.f, s);                       \
        ms_add(m, s, m2_, s2_);                                                                                      \
    } while (0)
__device__ __forceinline__ void wave_scan_ms(float &m, float &s)
{
    LTR_MS_STEP(0x111, 0xF); LTR_MS_STEP(0x112, 0xF); LTR_MS_STEP(0x114, 0xF); LTR_MS_STEP(0x118, 0xF);
    LTR_MS_STEP(0x142, 0xA); LTR_MS_STEP(0x143, 0xC);
}
#undef LTR_MS_STEP

#define LTR_AFF_STEP(CTRL, RM)                                                                                       \
    do {                                                                                                             \
        float a1_ = dpp_from<CTRL, RM>(1.f, a), b1_ = dpp_from<CTRL, RM>(0.f, b);                                    \
        aff_then(a1_, b1_, a, b);                                                                                    \
        a = a1_; b = b1_;                                                                                            \
    } while (0)
__device__ __forceinline__ void wave_scan_aff(float &a, float &b)
{
    LTR_AFF_STEP(0x111, 0xF); LTR_AFF_STEP(0x112, 0xF); LTR_AFF_STEP(0x114, 0xF); LTR_AFF_STEP(0x118, 0xF);
    LTR_AFF_STEP(0x142, 0xA); LTR_AFF_STEP(0x143, 0xC);
}
#undef LTR_AFF_STEP

// Workgroup scans in thread order of one value per thread: (x, y) becomes the combination of the threads before it
// (exclusive), (tx, ty) the whole workgroup's, the same bits in every thread.  `pair`: LDS of 2 x 16 floats.
// Contain barriers: call from uniform code.
__device__ __forceinline__ void block_scan_ms(float &x, float &y, float &tx, float &ty, float *pair)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    float im = x, is = y;
    wave_scan_ms(im, is);
    float em = __shfl_up(im, 1, kWave), es = __shfl_up(is, 1, kWave);
    if (lane == 0) { em = -INFINITY; es = 0.f; }
    __syncthreads();
    if (lane == 63) { pair[2 * w] = im; pair[2 * w + 1] = is; }
    __syncthreads();
    float m = -INFINITY, s = 0.f;
    for (int i = 0; i < w; ++i) ms_add(m, s, pair[2 * i], pair[2 * i + 1]);
    tx = m; ty = s;
    for (int i = w; i < nw; ++i) ms_add(tx, ty, pair[2 * i], pair[2 * i + 1]);
    ms_add(m, s, em, es);
    x = m; y = s;
}

__device__ __forceinline__ void block_scan_aff(float &x, float &y, float &tx, float &ty, float *pair)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    float ia = x, ib = y;
    wave_scan_aff(ia, ib);
    float ea = __shfl_up(ia, 1, kWave), eb = __shfl_up(ib, 1, kWave);
    if (lane == 0) { ea = 1.f; eb = 0.f; }
    __syncthreads();
    if (lane == 63) { pair[2 * w] = ia; pair[2 * w + 1] = ib; }
    __syncthreads();
    float a = 1.f, b = 0.f;
    for (int i = 0; i < w; ++i) aff_then(a, b, pair[2 * i], pair[2 * i + 1]);
    tx = a; ty = b;
    for (int i = w; i < nw; ++i) aff_then(tx, ty, pair[2 * i], pair[2 * i + 1]);
    aff_then(a, b, ea, eb);
    x = a; y = b;
}

// a_i = exp(LSE_i - LSE_{i-1}) from the (M, log S) pairs of ranks i and i - 1 (<= 1; clamped against rounding)
__device__ __forceinline__ float lse_step(float m, float ls, float mp, float lsp)
{
    return expf(fminf((m - mp) + (ls - lsp), 0.f));
}

// exp(x - LSE) <= 1
__device__ __forceinline__ float lse_prob(float x, float m, float ls) { return expf(fminf((x - m) - ls, 0.f)); }

struct ListMLEParams {
    MetricParams m;          // the batch and the tie words (m.scores, m.out unused: scores below)
    const float *scores;
    float *loss, *dscores;   // (B), (B, L) or null
    int k;                   // <= 0: every factor
};

// (metric_kernel's launch bounds and so its register budgets: same shapes, same occupancy)
template <int DPT>
__global__ void __launch_bounds__(1024, (DPT <= 0 ? 8 : 4))
listmle_kernel(ListMLEParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const MetricParams &m = p.m;
    const int b = blockIdx.x;
    const int L = m.L;
    const int L4 = (L + 3) & ~3;
    const int tid = threadIdx.x;
    const int T = blockDim.x;
    const int nb = clamp_n(m.n[b], L);
    const int K = p.k > 0 ? min(p.k, nb) : nb;

    // metric_kernel's LDS layout: (label, score) pairs where it keeps (score, label) -- metric_ranks ranks the x slot
    float2 *sy = reinterpret_cast<float2 *>(smem);
    int *rank_s = reinterpret_cast<int *>(smem + 8 * (size_t)L4);
    float *xs = reinterpret_cast<float *>(rank_s + L4);                // ranked scores (rank_y's slot)
    float *curve = reinterpret_cast<float *>(smem + 16 * (size_t)L4);
    float *red = curve + 2 * L4;
    float *pair = red + 32;
    float *mx = reinterpret_cast<float *>(smem), *ls = mx + L4;        // (M_i, log S_i), over sy once it is read

    const size_t row = (size_t)b * L;
    for (int j = tid; j < nb; j += T) sy[j] = make_float2(load_label(m.rel, m.rel_dtype, row + j), p.scores[row + j]);
    for (int j = tid; j < L4; j += T) rank_s[j] = 0;
    __syncthreads();
    metric_ranks<DPT>(m, smem, sy, rank_s, reinterpret_cast<int *>(xs), curve, nb, false);
    __syncthreads();
    for (int j = tid; j < nb; j += T) xs[rank_s[j]] = sy[j].y;
    __syncthreads();

    // 1. suffix (max, sum) scan: thread t owns ranks nb - 1 - [t ch, (t + 1) ch), walked downwards
    const int ch = (nb + T - 1) / T;
    const int lo = min(nb, tid * ch), hi = min(nb, lo + ch);
    float cm = -INFINITY, cs = 0.f, tm, ts;
    for (int q = lo; q < hi; ++q) ms_add(cm, cs, xs[nb - 1 - q], 1.f);
    block_scan_ms(cm, cs, tm, ts, pair);
    for (int q = lo; q < hi; ++q) {
        const int i = nb - 1 - q;
        ms_add(cm, cs, xs[i], 1.f);
        mx[i] = cm;
        ls[i] = logf(cs);
    }
    __syncthreads();
    float acc = 0.f;
    for (int i = tid; i < K; i += T) acc += (mx[i] - xs[i]) + ls[i];
    acc = block_sum(acc, red);
    if (tid == 0) p.loss[b] = acc;
    if (!p.dscores) return;

    // 2. gradient scan: thread t owns ranks [t ch, (t + 1) ch), walked upwards
    float ca = 1.f, cb = 0.f, ta, tb;
    for (int i = lo; i < hi; ++i)
        aff_then(ca, cb, i > 0 ? lse_step(mx[i], ls[i], mx[i - 1], ls[i - 1]) : 0.f, i < K ? 1.f : 0.f);
    block_scan_aff(ca, cb, ta, tb, pair);
    float d = cb;                                                      // D before the chunk (D_{-1} = 0)
    for (int i = lo; i < hi; ++i) {
        const float bi = i < K ? 1.f : 0.f;
        d = __builtin_fmaf(i > 0 ? lse_step(mx[i], ls[i], mx[i - 1], ls[i - 1]) : 0.f, d, bi);
        curve[i] = lse_prob(xs[i], mx[i], ls[i]) * d - bi;
    }
    __syncthreads();
    for (int j = tid; j < L; j += T) p.dscores[row + j] = j < nb ? curve[rank_s[j]] : 0.f;
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
    const int q = blockIdx.x / p.tiles, tile = blockIdx.x - q * p.tiles;
    const int L = p.key.L, tid = threadIdx.x;
    const size_t base = (size_t)q * L;
    const int nb = clamp_n(p.key.n[q], L);
    const unsigned long long seed = long_seed(p.key);
    const int r0 = tile * kEpiTile;
    const int len = max(0, min(kEpiTile, nb - r0));
    for (int x = tid; x < len; x += kEpiThreads) {
        const float v = p.scores[base + long_doc(p.key, p.sorted[base + r0 + x], seed)];
        t[x] = v;
        p.xs[base + r0 + x] = v;
    }
    __syncthreads();
    float m = -INFINITY, s = 0.f, tm, ts;
    for (int e = 0; e < kEpiE; ++e) {
        const int x = tid * kEpiE + e;
        if (x < len) ms_add(m, s, t[x], 1.f);
    }
    block_scan_ms(m, s, tm, ts, pair);
    if (tid == 0) p.tagg[(size_t)q * p.tiles + tile] = make_float2(tm, ts);
}

// 2. (M_r, log S_r) of the tile's ranks: the tiles after it first (in a fixed order), then the in-tile suffix scan
__global__ void __launch_bounds__(kEpiThreads) listmle_long_lse_kernel(ListMLELongParams p)
{
    __shared__ float t[kEpiTile];
    __shared__ float pair[32];
    __shared__ float red[32];
    const int q = blockIdx.x / p.tiles, tile = blockIdx.x - q * p.tiles;
    const int L = p.key.L, tid = threadIdx.x;
    const size_t base = (size_t)q * L;
    const int nb = clamp_n(p.key.n[q], L);
    const int K = listmle_k(p, nb);
    const int r0 = tile * kEpiTile;
    const int len = max(0, min(kEpiTile, nb - r0));
    for (int x = tid; x < len; x += kEpiThreads) t[x] = p.xs[base + r0 + x];
    // the tiles after this one: thread-contiguous runs of them, then the workgroup's combination
    const int after = max(0, min(p.tiles, (nb + kEpiTile - 1) / kEpiTile) - tile - 1);
    const int ach = (after + kEpiThreads - 1) / kEpiThreads;
    float im = -INFINITY, is = 0.f, inm, ins;
    for (int i = tid * ach; i < min(after, (tid + 1) * ach); ++i) {
        const float2 a = p.tagg[(size_t)q * p.tiles + tile + 1 + i];
        ms_add(im, is, a.x, a.y);
    }
    block_scan_ms(im, is, inm, ins, pair);                             // (its barriers publish t)
    // the tile: thread t owns the reversed ranks [t kEpiE, (t + 1) kEpiE)
    float m = -INFINITY, s = 0.f, tm, ts;
    for (int e = 0; e < kEpiE; ++e) {
        const int x = len - 1 - (tid * kEpiE + e);
        if (x >= 0) ms_add(m, s, t[x], 1.f);
    }
    block_scan_ms(m, s, tm, ts, pair);
    float rm = inm, rs = ins, acc = 0.f;
    ms_add(rm, rs, m, s);
    for (int e = 0; e < kEpiE; ++e) {
        const int x = len - 1 - (tid * kEpiE + e);
        if (x >= 0) {
            ms_add(rm, rs, t[x], 1.f);
            const float l = logf(rs);
            p.mx[base + r0 + x] = rm;
            p.ls[base + r0 + x] = l;
            if (r0 + x < K) acc += (rm - t[x]) + l;
        }
    }
    acc = block_sum(acc, red);
    if (tid == 0) p.tloss[(size_t)q * p.tiles + tile] = acc;
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
    const int q = blockIdx.x / p.tiles, tile = blockIdx.x - q * p.tiles;
    const int L = p.key.L, tid = threadIdx.x;
    const size_t base = (size_t)q * L;
    const int nb = clamp_n(p.key.n[q], L);
    const int K = listmle_k(p, nb);
    const int r0 = tile * kEpiTile;
    const int len = max(0, min(kEpiTile, nb - r0));
    float a = 1.f, b = 0.f, ta, tb;
    for (int e = 0; e < kEpiE; ++e) {
        const int x = tid * kEpiE + e;
        if (x < len) {
            const float2 f = listmle_long_map(p, base, r0 + x, K);
            aff_then(a, b, f.x, f.y);
        }
    }
    block_scan_aff(a, b, ta, tb, pair);
    if (tid == 0) p.taff[(size_t)q * p.tiles + tile] = make_float2(ta, tb);
}

// 4. D_r of the tile's ranks (the maps of the tiles before it composed in order), dscores through the ranking
__global__ void __launch_bounds__(kEpiThreads) listmle_long_grad_kernel(ListMLELongParams p)
{
    __shared__ float pair[32];
    const int q = blockIdx.x / p.tiles, tile = blockIdx.x - q * p.tiles;
    const int L = p.key.L, tid = threadIdx.x;
    const size_t base = (size_t)q * L;
    const int nb = clamp_n(p.key.n[q], L);
    const int K = listmle_k(p, nb);
    const unsigned long long seed = long_seed(p.key);
    const int r0 = tile * kEpiTile;
    const int len = max(0, min(kEpiTile, nb - r0));
    // padded documents sit at their own index past the real ones
    for (int x = max(len, 0) + tid; x < min(kEpiTile, L - r0); x += kEpiThreads) p.dscores[base + r0 + x] = 0.f;
    const int before = min(tile, (nb + kEpiTile - 1) / kEpiTile);
    const int bch = (before + kEpiThreads - 1) / kEpiThreads;
    float pa = 1.f, pb = 0.f, ta, tb;
    for (int i = tid * bch; i < min(before, (tid + 1) * bch); ++i) {
        const float2 f = p.taff[(size_t)q * p.tiles + i];
        aff_then(pa, pb, f.x, f.y);
    }
    block_scan_aff(pa, pb, ta, tb, pair);
    const float din = tb;                                              // D at the end of the tiles before (D_{-1} = 0)
    float a = 1.f, b = 0.f, ea, eb;
    for (int e = 0; e < kEpiE; ++e) {
        const int x = tid * kEpiE + e;
        if (x < len) {
            const float2 f = listmle_long_map(p, base, r0 + x, K);
            aff_then(a, b, f.x, f.y);
        }
    }
    block_scan_aff(a, b, ea, eb, pair);
    float d = __builtin_fmaf(a, din, b);
    for (int e = 0; e < kEpiE; ++e) {
        const int x = tid * kEpiE + e;
        if (x < len) {
            const int r = r0 + x;
            const float2 f = listmle_long_map(p, base, r, K);
            d = __builtin_fmaf(f.x, d, f.y);
            const float g = lse_prob(p.xs[base + r], p.mx[base + r], p.ls[base + r]) * d - f.y;
            p.dscores[base + long_doc(p.key, p.sorted[base + r], seed)] = g;
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
// the long path's keys and inverse tie map, three (B, L) float arrays, two (B, tiles) float2 and one float array
inline size_t listmle_long_workspace_bytes(int B, int L)
{
    const size_t BL = (size_t)B * (size_t)L, bt = (size_t)B * (size_t)long_epi_tiles(L);
    return align256(16 * BL) + align256(4 * (size_t)L) + 3 * align256(4 * BL) + align256(16 * bt) + 4 * bt;
}

int long_listmle(const float *scores, const void *rel, int rel_dtype, const int64_t *n, int k, const int32_t *tie,
                 int use_seed, uint64_t seed, const int64_t *seed_dev, int B, int L, float *loss, float *dscores,
                 void *workspace, size_t workspace_bytes, hipStream_t s)
{
    if (!workspace || workspace_bytes < listmle_long_workspace_bytes(B, L)) return LTR_ERR_WORKSPACE;
    const LongWorkspace ws = long_workspace(workspace, B, L);
    ListMLELongParams p{};
    p.key = long_key_params(nullptr, rel, rel_dtype, n, tie, use_seed, seed, seed_dev, L, ws, s);
    p.scores = scores; p.loss = loss; p.dscores = dscores;
    p.k = k; p.B = B;
    p.tiles = long_epi_tiles(L);
    const size_t BL = (size_t)B * (size_t)L, bt = (size_t)B * (size_t)p.tiles;
    unsigned char *w = reinterpret_cast<unsigned char *>(ws.inv) + align256(4 * (size_t)L);
    p.xs = reinterpret_cast<float *>(w);
    p.mx = reinterpret_cast<float *>(w + align256(4 * BL));
    p.ls = reinterpret_cast<float *>(w + 2 * align256(4 * BL));
    p.tagg = reinterpret_cast<float2 *>(w + 3 * align256(4 * BL));
    p.taff = p.tagg + bt;
    p.tloss = reinterpret_cast<float *>(w + 3 * align256(4 * BL) + align256(16 * bt));
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
    const dim3 grid((unsigned)p.m.B), block((unsigned)sh.threads);
#define LTR_LAUNCH(D)                                                                           \
    do {                                                                                        \
        LTR_ENSURE_LDS((listmle_kernel<D>), sh.lds);                                            \
        hipLaunchKernelGGL((listmle_kernel<D>), grid, block, sh.lds, stream, p);                \
    } while (0)
    switch (sh.dpt) {
    case 0: LTR_LAUNCH(0); break;
    case -2: LTR_LAUNCH(-2); break;
    case -4: LTR_LAUNCH(-4); break;
    case 1: LTR_LAUNCH(1); break;
    case 2: LTR_LAUNCH(2); break;
    default: LTR_LAUNCH(4); break;
    }
#undef LTR_LAUNCH
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

size_t ltr_listmle_workspace_bytes(int B, int L)
{
    if (check_lists(B, L, kMaxSortListLen) != LTR_OK) return 0;
    return long_path(L) ? listmle_long_workspace_bytes(B, L) : 0;
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
    if (use_seed) { p.m.use_seed = 1; p.m.tie_seed = seed; p.m.tie_seed_dev = seed_dev; }
    else p.m.tie = tie;
    p.scores = scores; p.loss = loss; p.dscores = dscores; p.k = k;
    return launch_listmle(p, s);
}

}  // extern "C"
