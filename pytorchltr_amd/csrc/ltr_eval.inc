// ltr_eval.inc -- evaluate(): M ranking metrics of every query from ONE ranking of it
// (included by ltr_kernels.hip after ltr_longsort.inc; C ABI: include/ltr_eval.h).
//
// Up to kMaxListLen documents: eval_kernel, one workgroup per query on the ranked-row core (ltr_ranked.inc): its
// launch shape, LDS layout and ranking (the labels too when an NDCG is asked for), and its ranked_dcg / ranked_arp --
// the very functions metric_kernel calls, so the DCG-family metrics and ARP equal dcg / ndcg / arp bit for bit.  Then it scatters
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

// (the launch bounds, and so the register budgets, of the ranked-row core's kernels: same shapes, same occupancy)
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
    const RankedRowLds q = ranked_row_lds(smem, L, DPT <= 0);
    // the spec, staged behind the core's layout (launch_eval adds its bytes), read one wave-uniform entry at a time
    // (indexed in the kernel arguments, the sort path's eight-wave bound of 80 SGPRs spilled three more of them
    // into VGPR lanes)
    int2 *spec = reinterpret_cast<int2 *>(q.free);
    if (tid < p.M) spec[tid] = p.spec[tid];

    const size_t row = (size_t)b * L;
    const int nload = (p.need & EVAL_NEED_DCG) ? L : nb;
    for (int j = tid; j < nload; j += T) q.sy[j] = make_float2(m.scores[row + j], load_label(m.rel, m.rel_dtype, row + j));
    for (int j = tid; j < 2 * L4; j += T) q.rank_s[j] = 0;
    __syncthreads();
    metric_ranks<DPT>(m, q, nb, (p.need & EVAL_NEED_IDEAL) != 0);
    __syncthreads();

    // ---- dcg / ndcg / arp ----
    for (int i = 0; i < p.M; ++i) {
        const int op = __builtin_amdgcn_readfirstlane(spec[i].x);
        if (op > LTR_EVAL_ARP) continue;
        float v;
        if (op == LTR_EVAL_ARP) {
            v = ranked_arp(q, nb);
        } else {
            const bool norm = op == LTR_EVAL_NDCG;
            const int k = __builtin_amdgcn_readfirstlane(spec[i].y);
            const int kk = k > 0 ? min(k, L) : 0;
            v = ranked_dcg(q, L, nb, kk, norm, m.use_exp);
            if (kk == 0) {
                // the last column of dcg / ndcg's curve
                v = q.curve[L - 1];
                if (norm) {
                    float id = q.icurve[L - 1];
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
    float *lab = q.curve, *cnt = q.icurve;
    float *keep = reinterpret_cast<float *>(q.rank_y);                 // prod_{i <= r} (1 - R_i)
    __syncthreads();
    for (int k = tid; k < nb; k += T) lab[q.rank_s[k]] = q.sy[k].y;
    __syncthreads();
    for (int r = tid; r < nb; r += T) {
        cnt[r] = lab[r] >= p.rel_level ? 1.f : 0.f;
        if (p.need & EVAL_NEED_ERR) keep[r] = 1.f - err_prob(lab[r], p.err_gmax);
    }
    __syncthreads();
    block_scan<OpAdd>(cnt, nb, q.scan);
    if (p.need & EVAL_NEED_ERR) block_scan<OpMul>(keep, nb, q.scan);
    const float R = nb > 0 ? cnt[nb - 1] : 0.f;
    int first = nb;
    if (p.need & EVAL_NEED_MRR) {
        float lead = 0.f;                                              // ranks before the first relevant one
        for (int r = tid; r < nb; r += T) lead += cnt[r] == 0.0f ? 1.f : 0.f;
        first = (int)block_sum(lead, q.red);
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
            s = block_sum(s, q.red);
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
    const EpiTile t = epi_tile(p.l.k, p.tiles);
    const int L = p.l.k.L, tid = threadIdx.x;
    const int nb = t.nb, r0 = t.r0;
    const bool dcg = (p.need & EVAL_NEED_DCG) != 0;
    float c = 0.f, keep = 1.f, first = OpMin::id;
    for (int x = tid; x < kEpiTile; x += kEpiThreads) {
        const int r = r0 + x;
        float y = 0.f, dt = 0.f;
        if (x < t.span) {
            if (IDEAL) {
                dt = long_dcg_term(p.l, t.base, r, nb, t.seed);
            } else {
                // (the label once for the term and the counts: long_dcg_term's label and dcg_term)
                y = x < t.real ? eval_long_label(p, t.base, r, t.seed) : (dcg ? load_label(p.l.k.rel, p.l.k.rel_dtype, t.base + r) : 0.f);
                if (dcg) dt = dcg_term(y, r, p.l.use_exp);
                if (x < t.real) {
                    const bool rel = y >= p.rel_level;
                    c += rel ? 1.f : 0.f;
                    if (rel) first = fminf(first, (float)r);
                    keep *= 1.f - err_prob(y, p.err_gmax);
                }
            }
        }
        lab[x] = y;
        term[x] = dt;
    }
    const size_t tslot = (size_t)t.q * p.tiles + t.tile;
    if (!IDEAL) {
        c = block_sum(c, red);
        if (p.need & EVAL_NEED_ERR) keep = block_reduce<OpMul>(keep, red);
        if (p.need & EVAL_NEED_MRR) first = block_reduce<OpMin>(first, red);
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
                if (x < t.real) {
                    a += (float)(r0 + x + 1) * lab[x];
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
    const EpiTile t = epi_tile(p.l.k, p.tiles);
    const int tid = threadIdx.x;
    const int nb = t.nb, r0 = t.r0;
    const bool err = (p.need & EVAL_NEED_ERR) != 0;
    for (int x = tid; x < kEpiTile; x += kEpiThreads) {
        const bool real = x < t.real;
        const float y = real ? eval_long_label(p, t.base, r0 + x, t.seed) : 0.f;
        lab[x] = y;
        cnt[x] = (real && y >= p.rel_level) ? 1.f : 0.f;
        keep[x] = real ? 1.f - err_prob(y, p.err_gmax) : 1.f;
    }
    float c0 = 0.f, k0 = 1.f;
    for (int i = tid; i < t.tile; i += kEpiThreads) {
        c0 += p.cnt[(size_t)t.q * p.tiles + i];
        k0 *= p.keep[(size_t)t.q * p.tiles + i];
    }
    c0 = block_sum(c0, red);
    if (err) k0 = block_reduce<OpMul>(k0, red);
    __syncthreads();
    block_scan<OpAdd>(cnt, kEpiTile, red);
    if (err) block_scan<OpMul>(keep, kEpiTile, red);
    const size_t tslot = (size_t)t.q * p.tiles + t.tile;
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
    float R = 0.f, first = OpMin::id;
    for (int t = tid; t < p.tiles; t += kEpiThreads) {
        R += p.cnt[row + t];
        first = fminf(first, p.first[row + t]);
    }
    R = block_sum(R, red);
    if (p.need & EVAL_NEED_MRR) first = block_reduce<OpMin>(first, red);
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

// The workspace of ltr_eval_workspace_bytes (include/ltr_eval.h states the byte formula): the long path's keys and
// inverse tie map, then 2 M + 3 (B, tiles) arrays, into p.
inline LongWorkspace eval_long_workspace(Carver &c, int B, int L, int M, EvalLongParams &p)
{
    const LongWorkspace ws = long_workspace(c, B, L, false);
    const size_t arr = (size_t)B * (size_t)long_epi_tiles(L);
    p.part = c.take<float>((size_t)M * arr);
    p.ipart = c.take<float>((size_t)M * arr);
    p.cnt = c.take<float>(arr);
    p.keep = c.take<float>(arr);
    p.first = c.take<float>(arr);
    return ws;
}

int long_eval(const float *scores, const void *rel, int rel_dtype, const int64_t *n, const int32_t *tie, int use_seed,
              uint64_t seed, const int64_t *seed_dev, int B, int L, const int32_t *spec, int M, int need,
              float relevance_level, int use_exp, float err_max_grade, float *out, void *workspace,
              size_t workspace_bytes, hipStream_t s)
{
    EvalLongParams p{};
    Carver carver(workspace);
    const LongWorkspace ws = eval_long_workspace(carver, B, L, M, p);
    if (!workspace || workspace_bytes < carver.off) return LTR_ERR_WORKSPACE;
    p.l.k = long_key_params(scores, rel, rel_dtype, n, tie, use_seed, seed, seed_dev, L, ws, s);
    p.l.use_exp = use_exp;
    p.M = M; p.need = need; p.B = B;
    p.tiles = long_epi_tiles(L);
    p.rel_level = relevance_level;
    p.err_gmax = err_max_grade;
    const size_t arr = (size_t)B * p.tiles;
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
    // (+ the spec, staged behind the core's layout)
    return launch_ranked(sh, p.m.B, sizeof(p.spec), stream, p, [](auto D) { return &eval_kernel<decltype(D)::value>; });
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
    if (!long_path(L)) return 0;
    EvalLongParams p{};
    Carver sizes(nullptr);
    eval_long_workspace(sizes, B, L, M, p);
    return sizes.off;
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
    set_tie(p.m, tie, use_seed, seed, seed_dev);
    p.out = out;
    p.M = M; p.need = need;
    p.rel_level = relevance_level;
    p.err_gmax = err_max_grade;
    for (int i = 0; i < M; ++i) p.spec[i] = make_int2(spec[2 * i], spec[2 * i + 1]);
    return launch_eval(p, s);
}

}  // extern "C"
