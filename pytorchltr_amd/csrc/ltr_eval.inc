// ltr_eval.inc -- evaluate(): M ranking metrics of every query from ONE ranking of it
// (included by ltr_kernels.hip after ltr_longsort.inc; C ABI: include/ltr_eval.h).
//
// Up to kMaxListLen documents: eval_kernel, one workgroup per query in metric_kernel's launch shape
// (metric_shape).  It stages the row, ranks it with metric_ranks (the labels too when an NDCG is
// asked for) and forms the DCG-family metrics and ARP exactly as metric_kernel does, term for term
// and in the same order of summation, so they equal dcg / ndcg / arp bit for bit.  Then it scatters
// the real documents' labels into LDS in rank order and takes only the prefix data the request
// needs: one inclusive scan of the relevance indicator (MAP, P, recall, R; the first relevant rank is
// the number of leading zeros of that scan) and one multiplicative scan of (1 - R_i) (ERR).  The
// metric list is a run-time loop over the spec (kernel arguments, staged in LDS): six instantiations in all.
//
// Longer lists (and every list under ltr_debug_long_sort_all): the key sort of ltr_longsort.inc --
// of the labels first when an NDCG is asked for --, then, per tile of kEpiTile ranks,
//   1. eval_long_partial_kernel: relevant count, prod (1 - R_i), first relevant rank and the
//      DCG / ARP / P / recall sums of the tile (the IDEAL instance: ideal DCG over the label sort);
//   2. eval_long_prefix_kernel (MAP, ERR only): the tile's AP / ERR terms, with the count and the
//      product of the tiles before it taken from step 1's partials in a fixed order;
//   3. eval_long_finish_kernel, per query: the tile sums added in a fixed order, each metric's formula.
// No atomics: bit-identical from run to run.  All memory is the caller's workspace: capturable.

#include "ltr_eval.h"

namespace {

// what a request needs, from its ops (eval_needs, on the host)
enum {
    EVAL_NEED_DCG = 1,       // a DCG or NDCG: every label of the row is read (padded ones count)
    EVAL_NEED_IDEAL = 2,     // an NDCG: the ideal ranking
    EVAL_NEED_REL = 4,       // a trec_eval metric: labels in rank order, the relevant-count scan
    EVAL_NEED_ERR = 8,       // the product scan of (1 - R_i)
    EVAL_NEED_MRR = 16,      // the first relevant rank
    EVAL_NEED_PREFIX = 32    // MAP or ERR: terms that depend on the tiles before (long path)
};

struct EvalParams {
    MetricParams m;                          // the batch, the tie words, use_exp, msplit (m.out unused)
    float *out;                              // (M, B)
    int M, need;
    float rel_level, err_gmax;
    int2 spec[LTR_EVAL_MAX_METRICS];         // (op, k); k = 0: the whole list
};

__device__ __forceinline__ float err_prob(float y, float gmax)
{
    const float g = fminf(fmaxf(y, 0.f), gmax);
    return (exp2f(g) - 1.0f) / exp2f(gmax);
}

// Inclusive scan of buf[0..len) in place, sum or (MUL) product; thread t owns a contiguous chunk.
// `scratch`: LDS of >= 16 floats.  Contains barriers: call from uniform code, after buf is written.
template <bool MUL>
__device__ void block_scan(float *buf, int len, float *scratch)
{
    const int T = blockDim.x, tid = threadIdx.x;
    const float id = MUL ? 1.f : 0.f;
    const int ch = (len + T - 1) / T;
    const int lo = min(len, tid * ch), hi = min(len, lo + ch);
    float s = id;
    for (int i = lo; i < hi; ++i) s = MUL ? s * buf[i] : s + buf[i];
    float incl = s;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const float up = __shfl_up(incl, off, kWave);
        if ((tid & 63) >= off) incl = MUL ? incl * up : incl + up;
    }
    float excl = __shfl_up(incl, 1, kWave);
    if ((tid & 63) == 0) excl = id;
    __syncthreads();
    if ((tid & 63) == 63) scratch[tid >> 6] = incl;
    __syncthreads();
    float run = id;
    for (int i = 0; i < (tid >> 6); ++i) run = MUL ? run * scratch[i] : run + scratch[i];
    run = MUL ? run * excl : run + excl;
    for (int i = lo; i < hi; ++i) {
        run = MUL ? run * buf[i] : run + buf[i];
        buf[i] = run;
    }
    __syncthreads();
}

// Product (MUL) or minimum over the workgroup, every thread gets it; fixed order (a butterfly, then the
// waves in order).  `red`: LDS of >= 16 floats.  Contains barriers: call from uniform code.
template <bool MUL>
__device__ __forceinline__ float block_reduce(float v, float *red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float u = __shfl_xor(v, o, kWave);
        v = MUL ? v * u : fminf(v, u);
    }
    const int nw = blockDim.x >> 6;
    if (nw == 1) return v;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = red[0];
    for (int i = 1; i < nw; ++i) t = MUL ? t * red[i] : fminf(t, red[i]);
    return t;
}

// A trec_eval metric from its parts: s = the summed terms (MAP, ERR) or the relevant count in the top
// min(k, n) (P, recall); R = relevant documents; first = 0-based rank of the first of them; kc = min(k, n).
__device__ __forceinline__ float eval_rel_metric(int op, int k, int L, int kc, float s, float R, int first)
{
    if (R == 0.0f) return 0.f;
    switch (op) {
    case LTR_EVAL_MAP: return s / R;
    case LTR_EVAL_MRR: return first < kc ? 1.f / (float)(first + 1) : 0.f;
    case LTR_EVAL_P: return s / (float)(k > 0 ? k : L);
    case LTR_EVAL_RECALL: return s / R;
    default: return s;                                                // LTR_EVAL_ERR
    }
}

// (the launch bounds, and so the register budgets, of metric_kernel: same shapes, same occupancy)
template <int DPT>
__global__ void __launch_bounds__(1024, (DPT <= 0 ? 8 : 4))
eval_kernel(EvalParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const MetricParams &m = p.m;
    const int b = blockIdx.x;
    const int L = m.L;
    const int L4 = (L + 3) & ~3;
    const int tid = threadIdx.x;
    const int T = blockDim.x;
    const int nb = clamp_n(m.n[b], L);

    // metric_kernel's LDS layout
    float2 *sy = reinterpret_cast<float2 *>(smem);
    int *rank_s = reinterpret_cast<int *>(smem + 8 * (size_t)L4);
    int *rank_y = rank_s + L4;
    float *curve = reinterpret_cast<float *>(smem + 16 * (size_t)L4);
    float *icurve = curve + L4;
    float *red = icurve + L4;
    float *scan_scratch = red + 32;
    // the spec, staged behind metric_kernel's layout (launch_eval adds its bytes), read one wave-uniform entry at a time
    // (indexed in the kernel arguments, the sort path's eight-wave bound of 80 SGPRs spilled three more of them
    // into VGPR lanes)
    int2 *spec = reinterpret_cast<int2 *>(smem + (DPT <= 0 ? metric_lds_bytes_sort(L) : metric_lds_bytes(L)));
    if (tid < p.M) spec[tid] = p.spec[tid];

    const size_t row = (size_t)b * L;
    const int nload = (p.need & EVAL_NEED_DCG) ? L : nb;
    for (int j = tid; j < nload; j += T) sy[j] = make_float2(m.scores[row + j], load_label(m.rel, m.rel_dtype, row + j));
    for (int j = tid; j < 2 * L4; j += T) rank_s[j] = 0;
    __syncthreads();
    metric_ranks<DPT>(m, smem, sy, rank_s, rank_y, curve, nb, (p.need & EVAL_NEED_IDEAL) != 0);
    __syncthreads();

    // ---- dcg / ndcg / arp: metric_kernel's terms and sums ----
    for (int i = 0; i < p.M; ++i) {
        const int op = __builtin_amdgcn_readfirstlane(spec[i].x);
        if (op > LTR_EVAL_ARP) continue;
        float v;
        if (op == LTR_EVAL_ARP) {
            float srp = 0.f, nrp = 0.f;
            for (int k = tid; k < nb; k += T) {
                const float y = sy[k].y;
                srp += (float)(rank_s[k] + 1) * y;
                nrp += y;
            }
            srp = block_sum(srp, red);
            nrp = block_sum(nrp, red);
            if (nrp == 0.0f) nrp = 1.0f;
            v = srp / nrp;
        } else {
            const bool norm = op == LTR_EVAL_NDCG;
            const int k = __builtin_amdgcn_readfirstlane(spec[i].y);
            const int kk = k > 0 ? min(k, L) : 0;
            float part = 0.f, ipart = 0.f;
            for (int k = tid; k < L; k += T) {
                const float y = sy[k].y;
                const float gain = m.use_exp ? (exp2f(y) - 1.0f) : y;
                const int r = k < nb ? rank_s[k] : k;
                const float term = gain / log2f((float)r + 2.0f);
                int ry = 0;
                float iterm = 0.f;
                if (norm) {
                    ry = k < nb ? rank_y[k] : k;
                    iterm = gain / log2f((float)ry + 2.0f);
                }
                if (kk > 0) {
                    part += (r < kk) ? term : 0.f;
                    ipart += (norm && ry < kk) ? iterm : 0.f;
                } else {
                    curve[r] = term;
                    if (norm) icurve[ry] = iterm;
                }
            }
            if (kk > 0) {
                part = block_sum(part, red);
                if (norm) {
                    ipart = block_sum(ipart, red);
                    if (ipart == 0.0f) ipart = 1.0f;
                    part = part / ipart;
                }
                v = part;
            } else {
                // the last column of dcg / ndcg's curve: the same scan
                __syncthreads();
                block_inclusive_scan(curve, L, scan_scratch);
                if (norm) block_inclusive_scan(icurve, L, scan_scratch);
                v = curve[L - 1];
                if (norm) {
                    float id = icurve[L - 1];
                    if (id == 0.0f) id = 1.0f;
                    v /= id;
                }
                __syncthreads();                                       // read before the next metric writes
            }
        }
        if (tid == 0) p.out[(size_t)i * m.B + b] = v;
    }
    if (!(p.need & EVAL_NEED_REL)) return;

    // ---- trec_eval metrics: labels of the real documents in rank order, then the scans they need ----
    float *lab = curve, *cnt = icurve;
    float *keep = reinterpret_cast<float *>(rank_y);                   // prod_{i <= r} (1 - R_i)
    __syncthreads();
    for (int k = tid; k < nb; k += T) lab[rank_s[k]] = sy[k].y;
    __syncthreads();
    for (int r = tid; r < nb; r += T) {
        cnt[r] = lab[r] >= p.rel_level ? 1.f : 0.f;
        if (p.need & EVAL_NEED_ERR) keep[r] = 1.f - err_prob(lab[r], p.err_gmax);
    }
    __syncthreads();
    block_scan<false>(cnt, nb, scan_scratch);
    if (p.need & EVAL_NEED_ERR) block_scan<true>(keep, nb, scan_scratch);
    const float R = nb > 0 ? cnt[nb - 1] : 0.f;
    int first = nb;
    if (p.need & EVAL_NEED_MRR) {
        float lead = 0.f;                                              // ranks before the first relevant one
        for (int r = tid; r < nb; r += T) lead += cnt[r] == 0.0f ? 1.f : 0.f;
        first = (int)block_sum(lead, red);
    }
    for (int i = 0; i < p.M; ++i) {
        const int op = __builtin_amdgcn_readfirstlane(spec[i].x), k = __builtin_amdgcn_readfirstlane(spec[i].y);
        if (op <= LTR_EVAL_ARP) continue;
        const int kc = k > 0 ? min(k, nb) : nb;
        float s = 0.f;
        if (op == LTR_EVAL_MAP || op == LTR_EVAL_ERR) {
            for (int r = tid; r < kc; r += T) {
                const float y = lab[r];
                if (op == LTR_EVAL_MAP) s += y >= p.rel_level ? cnt[r] / (float)(r + 1) : 0.f;
                else s += err_prob(y, p.err_gmax) / (float)(r + 1) * (r > 0 ? keep[r - 1] : 1.f);
            }
            s = block_sum(s, red);
        } else if (op != LTR_EVAL_MRR) {
            s = kc > 0 ? cnt[kc - 1] : 0.f;
        }
        if (tid == 0) p.out[(size_t)i * m.B + b] = eval_rel_metric(op, k, L, kc, s, R, first);
    }
}

// ---- the sort path ----
struct EvalLongParams {
    LongMetricParams l;                      // keys, sorted keys, use_exp, ideal (l.part, l.out unused)
    int M, need, B, tiles;                   // tiles per query: ceil(L / kEpiTile)
    float rel_level, err_gmax;
    float *part, *ipart;                     // (M, B, tiles) per-metric tile sums (ipart: ideal DCG, ARP's label sum)
    float *cnt, *keep, *first;               // (B, tiles) relevant count, prod (1 - R_i), first relevant rank
    float *out;                              // (M, B)
    int2 spec[LTR_EVAL_MAX_METRICS];
};

// The label of the document at rank r (< nb) of query `base`.
__device__ __forceinline__ float eval_long_label(const EvalLongParams &p, size_t base, int r, unsigned long long seed)
{
    return load_label(p.l.k.rel, p.l.k.rel_dtype, base + long_doc(p.l.k, p.l.sorted[base + r], seed));
}

template <bool IDEAL>
__global__ void __launch_bounds__(kEpiThreads) eval_long_partial_kernel(EvalLongParams p)
{
    __shared__ float lab[kEpiTile];          // labels of the tile's ranks (real documents)
    __shared__ float term[kEpiTile];         // DCG terms of the tile's ranks (padded documents included)
    __shared__ float red[32];
    const int q = blockIdx.x / p.tiles, tile = blockIdx.x - q * p.tiles;
    const int L = p.l.k.L, tid = threadIdx.x;
    const size_t base = (size_t)q * L;
    const int nb = clamp_n(p.l.k.n[q], L);
    const unsigned long long seed = long_seed(p.l.k);
    const int r0 = tile * kEpiTile;
    const int len = min(kEpiTile, L - r0);
    const bool dcg = (p.need & EVAL_NEED_DCG) != 0;
    float c = 0.f, keep = 1.f, first = 3.0e38f;
    for (int x = tid; x < kEpiTile; x += kEpiThreads) {
        const int r = r0 + x;
        float y = 0.f, t = 0.f;
        if (x < len) {
            if (IDEAL) {
                t = long_dcg_term(p.l, base, r, nb, seed);
            } else {
                y = r < nb ? eval_long_label(p, base, r, seed) : (dcg ? load_label(p.l.k.rel, p.l.k.rel_dtype, base + r) : 0.f);
                if (dcg) t = (p.l.use_exp ? (exp2f(y) - 1.0f) : y) / log2f((float)r + 2.0f);   // long_dcg_term
                if (r < nb) {
                    const bool rel = y >= p.rel_level;
                    c += rel ? 1.f : 0.f;
                    if (rel) first = fminf(first, (float)r);
                    keep *= 1.f - err_prob(y, p.err_gmax);
                }
            }
        }
        lab[x] = y;
        term[x] = t;
    }
    const size_t tslot = (size_t)q * p.tiles + tile;
    if (!IDEAL) {
        c = block_sum(c, red);
        if (p.need & EVAL_NEED_ERR) keep = block_reduce<true>(keep, red);
        if (p.need & EVAL_NEED_MRR) first = block_reduce<false>(first, red);
        if (tid == 0) {
            p.cnt[tslot] = c;
            p.keep[tslot] = keep;
            p.first[tslot] = first;
        }
    }
    __syncthreads();
    const size_t mstride = (size_t)p.B * p.tiles;
    for (int i = 0; i < p.M; ++i) {
        const int op = p.spec[i].x, k = p.spec[i].y;
        if (IDEAL ? op != LTR_EVAL_NDCG : (op == LTR_EVAL_MAP || op == LTR_EVAL_MRR || op == LTR_EVAL_ERR)) continue;
        float a = 0.f, a2 = 0.f;
        if (op == LTR_EVAL_DCG || op == LTR_EVAL_NDCG) {
            const int lim = k > 0 ? min(k, L) : L;
            for (int x = tid; x < kEpiTile; x += kEpiThreads) a += (r0 + x < lim) ? term[x] : 0.f;   // longsort_partial_kernel's order
        } else if (op == LTR_EVAL_ARP) {
            for (int x = tid; x < kEpiTile; x += kEpiThreads) {
                const int r = r0 + x;
                if (r < nb) {
                    a += (float)(r + 1) * lab[x];
                    a2 += lab[x];
                }
            }
            a2 = block_sum(a2, red);
        } else {                                                       // P, recall: relevant in the top min(k, n)
            const int kc = k > 0 ? min(k, nb) : nb;
            for (int x = tid; x < kEpiTile; x += kEpiThreads) a += (r0 + x < kc && lab[x] >= p.rel_level) ? 1.f : 0.f;
        }
        a = block_sum(a, red);
        if (tid == 0) {
            if (IDEAL) p.ipart[i * mstride + tslot] = a;
            else p.part[i * mstride + tslot] = a;
            if (op == LTR_EVAL_ARP) p.ipart[i * mstride + tslot] = a2;
        }
    }
}

// MAP and ERR terms of one tile: the relevant count and the product of (1 - R_i) of the ranks before
// the tile come from the tiles before it, added / multiplied in a fixed order.
__global__ void __launch_bounds__(kEpiThreads) eval_long_prefix_kernel(EvalLongParams p)
{
    __shared__ float lab[kEpiTile];
    __shared__ float cnt[kEpiTile];          // relevant documents in the top r + 1, within the tile
    __shared__ float keep[kEpiTile];         // prod (1 - R_i) over the tile's ranks <= r
    __shared__ float red[32];
    const int q = blockIdx.x / p.tiles, tile = blockIdx.x - q * p.tiles;
    const int L = p.l.k.L, tid = threadIdx.x;
    const size_t base = (size_t)q * L;
    const int nb = clamp_n(p.l.k.n[q], L);
    const unsigned long long seed = long_seed(p.l.k);
    const int r0 = tile * kEpiTile;
    const bool err = (p.need & EVAL_NEED_ERR) != 0;
    for (int x = tid; x < kEpiTile; x += kEpiThreads) {
        const int r = r0 + x;
        const float y = r < nb ? eval_long_label(p, base, r, seed) : 0.f;
        lab[x] = y;
        cnt[x] = (r < nb && y >= p.rel_level) ? 1.f : 0.f;
        keep[x] = r < nb ? 1.f - err_prob(y, p.err_gmax) : 1.f;
    }
    float c0 = 0.f, k0 = 1.f;
    for (int t = tid; t < tile; t += kEpiThreads) {
        c0 += p.cnt[(size_t)q * p.tiles + t];
        k0 *= p.keep[(size_t)q * p.tiles + t];
    }
    c0 = block_sum(c0, red);
    if (err) k0 = block_reduce<true>(k0, red);
    __syncthreads();
    block_scan<false>(cnt, kEpiTile, red);
    if (err) block_scan<true>(keep, kEpiTile, red);
    const size_t tslot = (size_t)q * p.tiles + tile;
    const size_t mstride = (size_t)p.B * p.tiles;
    for (int i = 0; i < p.M; ++i) {
        const int op = p.spec[i].x, k = p.spec[i].y;
        if (op != LTR_EVAL_MAP && op != LTR_EVAL_ERR) continue;
        const int kc = k > 0 ? min(k, nb) : nb;
        float a = 0.f;
        for (int x = tid; x < kEpiTile; x += kEpiThreads) {
            const int r = r0 + x;
            if (r >= kc) break;
            if (op == LTR_EVAL_MAP) a += lab[x] >= p.rel_level ? (c0 + cnt[x]) / (float)(r + 1) : 0.f;
            else a += err_prob(lab[x], p.err_gmax) / (float)(r + 1) * (k0 * (x > 0 ? keep[x - 1] : 1.f));
        }
        a = block_sum(a, red);
        if (tid == 0) p.part[i * mstride + tslot] = a;
    }
}

// Per query: the tile sums in a fixed order, then each metric's formula.
__global__ void __launch_bounds__(kEpiThreads) eval_long_finish_kernel(EvalLongParams p)
{
    __shared__ float red[32];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int L = p.l.k.L;
    const int nb = clamp_n(p.l.k.n[q], L);
    const size_t row = (size_t)q * p.tiles;
    const size_t mstride = (size_t)p.B * p.tiles;
    float R = 0.f, first = 3.0e38f;
    for (int t = tid; t < p.tiles; t += kEpiThreads) {
        R += p.cnt[row + t];
        first = fminf(first, p.first[row + t]);
    }
    R = block_sum(R, red);
    if (p.need & EVAL_NEED_MRR) first = block_reduce<false>(first, red);
    for (int i = 0; i < p.M; ++i) {
        const int op = p.spec[i].x, k = p.spec[i].y;
        float a = 0.f, c = 0.f;
        if (op != LTR_EVAL_MRR) {
            for (int t = tid; t < p.tiles; t += kEpiThreads) {
                a += p.part[i * mstride + row + t];
                if (op == LTR_EVAL_NDCG || op == LTR_EVAL_ARP) c += p.ipart[i * mstride + row + t];
            }
            a = block_sum(a, red);
            if (op == LTR_EVAL_NDCG || op == LTR_EVAL_ARP) c = block_sum(c, red);
        }
        float v;
        if (op == LTR_EVAL_DCG) {
            v = a;
        } else if (op == LTR_EVAL_NDCG || op == LTR_EVAL_ARP) {
            if (c == 0.0f) c = 1.0f;                                   // dcg.py:37, arp.py:41
            v = a / c;
        } else {
            const int kc = k > 0 ? min(k, nb) : nb;
            v = eval_rel_metric(op, k, L, kc, a, R, first < (float)L ? (int)first : L);
        }
        if (tid == 0) p.out[(size_t)i * p.B + q] = v;
    }
}

// ---- host side ----
inline bool eval_bad_op(int op) { return op < LTR_EVAL_DCG || op > LTR_EVAL_ERR; }

inline int eval_needs(const int32_t *spec, int M)
{
    int need = 0;
    for (int i = 0; i < M; ++i) {
        const int op = spec[2 * i];
        if (op == LTR_EVAL_DCG || op == LTR_EVAL_NDCG) need |= EVAL_NEED_DCG;
        if (op == LTR_EVAL_NDCG) need |= EVAL_NEED_IDEAL;
        if (op > LTR_EVAL_ARP) need |= EVAL_NEED_REL;
        if (op == LTR_EVAL_ERR) need |= EVAL_NEED_ERR | EVAL_NEED_PREFIX;
        if (op == LTR_EVAL_MAP) need |= EVAL_NEED_PREFIX;
        if (op == LTR_EVAL_MRR) need |= EVAL_NEED_MRR;
    }
    return need;
}

// the byte formula of include/ltr_eval.h: the long path's keys and inverse tie map, then 2 M + 3 (B, tiles) arrays
inline size_t eval_long_workspace_bytes(int B, int L, int M)
{
    return align256(16 * (size_t)B * (size_t)L) + align256(4 * (size_t)L) +
           4 * (size_t)B * (size_t)long_epi_tiles(L) * (size_t)(2 * M + 3);
}

int long_eval(const float *scores, const void *rel, int rel_dtype, const int64_t *n, const int32_t *tie, int use_seed,
              uint64_t seed, const int64_t *seed_dev, int B, int L, const int32_t *spec, int M, int need,
              float relevance_level, int use_exp, float err_max_grade, float *out, void *workspace,
              size_t workspace_bytes, hipStream_t s)
{
    if (!workspace || workspace_bytes < eval_long_workspace_bytes(B, L, M)) return LTR_ERR_WORKSPACE;
    const LongWorkspace ws = long_workspace(workspace, B, L);
    EvalLongParams p{};
    p.l.k = long_key_params(scores, rel, rel_dtype, n, tie, use_seed, seed, seed_dev, L, ws, s);
    p.l.use_exp = use_exp;
    p.M = M; p.need = need; p.B = B;
    p.tiles = long_epi_tiles(L);
    p.rel_level = relevance_level;
    p.err_gmax = err_max_grade;
    const size_t arr = (size_t)B * p.tiles;
    p.part = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(ws.inv) + align256(4 * (size_t)L));
    p.ipart = p.part + (size_t)M * arr;
    p.cnt = p.ipart + (size_t)M * arr;
    p.keep = p.cnt + arr;
    p.first = p.keep + arr;
    p.out = out;
    for (int i = 0; i < M; ++i) p.spec[i] = make_int2(spec[2 * i], spec[2 * i + 1]);
    const dim3 grid((unsigned)arr), block(kEpiThreads);
    if (need & EVAL_NEED_IDEAL) {
        // the ideal ranking first (its sort shares the key buffers): labels, index words
        EvalLongParams ip = p;
        ip.l.k.scores = nullptr; ip.l.k.mode = TIE_INDEX; ip.l.k.tie = nullptr; ip.l.k.seed_dev = nullptr;
        ip.l.ideal = 1;
        ip.l.sorted = long_sort(ip.l.k, B, ws, nullptr, s);
        hipLaunchKernelGGL(eval_long_partial_kernel<true>, grid, block, 0, s, ip);
    }
    p.l.sorted = long_sort(p.l.k, B, ws, nullptr, s);
    hipLaunchKernelGGL(eval_long_partial_kernel<false>, grid, block, 0, s, p);
    if (need & EVAL_NEED_PREFIX) hipLaunchKernelGGL(eval_long_prefix_kernel, grid, block, 0, s, p);
    hipLaunchKernelGGL(eval_long_finish_kernel, dim3((unsigned)B), block, 0, s, p);
    return (int)hipGetLastError();
}

int launch_eval(const EvalParams &p0, hipStream_t stream)
{
    EvalParams p = p0;
    const MetricShape sh = metric_shape(p.m);
    const dim3 grid((unsigned)p.m.B), block((unsigned)sh.threads);
    const size_t lds = sh.lds + sizeof(p.spec);            // + the spec (eval_kernel)
#define LTR_LAUNCH(D)                                                                           \
    do {                                                                                        \
        LTR_ENSURE_LDS((eval_kernel<D>), lds);                                                  \
        hipLaunchKernelGGL((eval_kernel<D>), grid, block, lds, stream, p);                      \
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

// The host checks of ltr_eval_f32 up to the lists (include/ltr_eval.h states the order).
inline int eval_check(int rel_dtype, const int32_t *spec, int M)
{
    if (bad_label_dtype(rel_dtype)) return LTR_ERR_KIND;
    const bool counted = M >= 1 && M <= LTR_EVAL_MAX_METRICS;
    if (spec && counted)
        for (int i = 0; i < M; ++i)
            if (eval_bad_op(spec[2 * i])) return LTR_ERR_KIND;
    if (!counted) return LTR_ERR_SHAPE;
    if (spec)
        for (int i = 0; i < M; ++i)
            if (spec[2 * i + 1] < 0) return LTR_ERR_SHAPE;
    return LTR_OK;
}

}  // namespace

extern "C" {

size_t ltr_eval_workspace_bytes(int B, int L, const int32_t *spec, int M)
{
    if (!spec || eval_check(LTR_LABEL_I64, spec, M) != LTR_OK || check_lists(B, L, kMaxSortListLen) != LTR_OK) return 0;
    return long_path(L) ? eval_long_workspace_bytes(B, L, M) : 0;
}

int ltr_eval_f32(const float *scores, const void *rel, int rel_dtype, const int64_t *n, const int32_t *tie, int use_seed,
                 uint64_t seed, const int64_t *seed_dev, int B, int L, const int32_t *spec, int M, float relevance_level,
                 int use_exp, float err_max_grade, float *out, void *workspace, size_t workspace_bytes, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (const int rc = eval_check(rel_dtype, spec, M)) return rc;
    if (const int rc = check_lists(B, L, kMaxSortListLen)) return rc;
    if (B == 0) return LTR_OK;
    if (!scores || !rel || !n || !spec || !out) return LTR_ERR_NULL;
    const hipStream_t s = (hipStream_t)stream;
    const int need = eval_needs(spec, M);
    if (long_path(L))
        return long_eval(scores, rel, rel_dtype, n, tie, use_seed, seed, seed_dev, B, L, spec, M, need, relevance_level,
                         use_exp, err_max_grade, out, workspace, workspace_bytes, s);
    EvalParams p{};
    p.m.scores = scores; p.m.rel = rel; p.m.n = n; p.m.B = B; p.m.L = L; p.m.rel_dtype = rel_dtype; p.m.use_exp = use_exp;
    if (use_seed) { p.m.use_seed = 1; p.m.tie_seed = seed; p.m.tie_seed_dev = seed_dev; }
    else p.m.tie = tie;
    p.out = out;
    p.M = M; p.need = need;
    p.rel_level = relevance_level;
    p.err_gmax = err_max_grade;
    for (int i = 0; i < M; ++i) p.spec[i] = make_int2(spec[2 * i], spec[2 * i + 1]);
    return launch_eval(p, s);
}

}  // extern "C"
