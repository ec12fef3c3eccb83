// ltr_longpair.inc -- the seven pairwise losses on lists longer than one workgroup's LDS (included by
// ltr_kernels.hip behind ltr_longsort.inc; C ABI: include/ltr_longpair.h; DESIGN.md 16).
//
// The one-workgroup-per-query loss kernels keep a whole query in LDS, which stops at 4096 documents.  Past
// that a query is cut into owner tiles of kPairOwn documents, one workgroup each:
//   * a thread OWNS kPairDpt documents of its tile -- score, label, the prepared (gain, rank) pair of the
//     LambdaNDCG kinds, the gradient -- in registers;
//   * the workgroup streams ALL n[b] documents of the query through LDS, kPairChunk at a time; every thread
//     reads the same LDS address per step (broadcast) and evaluates its kPairDpt pairs against it with the
//     pair terms of pairwise_core (pair_hinge, here with an exact gate / pair_oriented / pair_rowweight);
//   * every unordered pair is therefore evaluated TWICE, once from each end: the price for a gradient that is
//     complete in registers -- no atomics, no exchange between workgroups, bit-identical run to run;
//   * loss and gradient are summed per chunk and the chunk sums added afterwards (two levels: at most
//     kPairChunk * kPairDpt terms, then at most 64 chunk sums), so no running sum is 65 536 terms long;
//   * the workgroup writes the raw gradient of its documents and one loss partial; a finish kernel adds the
//     tile partials in tile order, applies the loss modifier and scales the gradient.
// The LambdaNDCG kinds first leave per document what ndcg_prepare_kernel leaves for the split-query launch, at every
// length from the two sorts: the ranking from the long key sort (ties in document-index order) and maxDCG from the
// label sort and the DCG tile partials of ltr_dcg_long_f32.
// LambdaNDCG2's delta_{|rank_i - rank_j|} is evaluated inline (two v_log_f32, two v_rcp_f32): the table does
// not fit LDS at 65 536 ranks (DESIGN.md 16).
// All memory is the caller's workspace; nothing synchronises with the host: capturable.
// The geometry, the owner-tile core (tile decode, float4 rounds, tile epilogue, partial sum) and the NDCG preparation
// (the two sorts, the maxDCG head) below also serve LambdaRank's pass, ltr_lambdarank_long.inc.  The chunk loop around
// the rounds stays with each kernel: lifted into a shared function it cost 3.5 to 9 % of the tile kernels' time
// (DESIGN.md 16).

#include "ltr_longpair.h"

namespace {

constexpr int kMaxPairListLen = 65536;       // <= 4.3e9 pair evaluations per query; ranks and counts exact in fp32
constexpr int kPairThreads = 256;
constexpr int kPairWaves = kPairThreads / 64;
constexpr int kPairDpt = 4;                  // owner documents per thread
constexpr int kPairOwn = kPairThreads * kPairDpt;
constexpr int kPairChunk = 1024;             // documents staged in LDS per step (8 KiB; 16 KiB for LambdaNDCG2)
static_assert(kPairChunk % 8 == 0 && kPairChunk % kPairThreads == 0, "whole float4 groups, whole staging rounds");

// past one workgroup's LDS, or forced there by a debug hook
inline bool long_or_forced(int L, const int &hook) { return L > kMaxListLen || __atomic_load_n(&hook, __ATOMIC_RELAXED) != 0; }
int g_long_pairs_all = 0;                    // ltr_debug_long_pairs_all
inline bool long_pairs(int L) { return long_or_forced(L, g_long_pairs_all); }
__host__ __device__ inline int long_pair_tiles(int L) { return (L + kPairOwn - 1) / kPairOwn; }

// ---- the owner-tile core ----
struct OwnerTile { int b, tile, nb, o0; size_t row; };    // query, tile, n[b], the tile's first owner, b * L

// Block -> (query, tile) of a launch over the tiles [tile0, tile0 + ntiles) of every query.  False (uniform): the
// tile starts at or past n[b], and the finish kernel never reads its partial.
__device__ __forceinline__ bool owner_tile(const int64_t *n, int L, int tile0, int ntiles, OwnerTile &t)
{
    t.b = blockIdx.x / ntiles;
    t.tile = tile0 + (blockIdx.x - t.b * ntiles);
    t.nb = clamp_n(n[t.b], L);
    t.o0 = t.tile * kPairOwn;
    t.row = (size_t)t.b * L;
    return t.o0 < t.nb;
}

// The broadcast rounds over s[0, len) of a float4 chunk: wave-uniform LDS addresses, four ds_read_b128 per round,
// then the remainder (< 4 documents) one by one.  round(v, m): v is an array of the 4 or 1 documents from m on.
template <typename Round>
__device__ __forceinline__ void float4_rounds(const float4 *s, int len, Round round)
{
    const int full = len - len % 4;
    for (int m = 0; m < full; m += 4) {
        float4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = s[m + j];
        round(v, m);
    }
    for (int m = full; m < len; ++m) {
        const float4 v[1] = {s[m]};
        round(v, m);
    }
}

// The tile epilogue: the workgroup's loss in a fixed order, into part[b][tile].
__device__ __forceinline__ void tile_loss(float ltot, float *red, float *part, const OwnerTile &t, int tiles)
{
    const float total = block_sum(ltot, red);
    if (threadIdx.x == 0) part[(size_t)t.b * tiles + t.tile] = total;
}

// The finish kernels' loss of query b: the partials of the tiles below nb, in tile order.
__device__ __forceinline__ float tile_loss_sum(const float *part, int b, int tiles, int nb)
{
    float total = 0.f;
    for (int t = 0; t < long_pair_tiles(nb); ++t) total += part[(size_t)b * tiles + t];
    return total;
}

// ---- the preparation of the NDCG-weighted losses: two sorts around the maxDCG tile partials ----
struct RankedKeys { LongKeyParams k; const unsigned long long *sorted; };

// The label sort (the ideal ranking: label keys, index words), the caller's launch partial(keys, sorted) that leaves
// the maxDCG terms per epilogue tile in ws.part, then the ranking by score, ties in document-index order.
template <typename Partial>
RankedKeys long_ndcg_sorts(const float *scores, const void *rel, int rel_dtype, const int64_t *n, int B, int L,
                           const LongWorkspace &ws, hipStream_t s, Partial partial)
{
    const LongKeyParams ik = long_key_params(nullptr, rel, rel_dtype, n, nullptr, 0, 0, nullptr, L, ws, s);
    partial(ik, long_sort(ik, B, ws, nullptr, s));
    const LongKeyParams sk = long_key_params(scores, rel, rel_dtype, n, nullptr, 0, 0, nullptr, L, ws, s);
    return {sk, long_sort(sk, B, ws, nullptr, s)};
}

// The head of the epilogues over the sorted score keys: 1 / maxDCG of query q from its tile partials, added in tile
// order by every thread; maxDCG == 0 -> 1 (pairwise_lambda.py:227).
__device__ __forceinline__ float inv_maxdcg(const float *part, int q, int ptiles)
{
    float maxdcg = 0.f;
    for (int i = 0; i < ptiles; ++i) maxdcg += part[(size_t)q * ptiles + i];
    if (maxdcg == 0.0f) maxdcg = 1.0f;
    return 1.0f / maxdcg;
}

// ---- preparation of the LambdaNDCG kinds from the sorted score keys ----
// prep[b][doc] = (a_doc, 0) for LambdaNDCG1, (G_doc / maxDCG, rank_doc) for LambdaNDCG2 (prepare_ndcg's formulas);
// maxDCG: the tile sums of the label sort's DCG terms over the real documents, added in tile order.
template <int KIND>
__global__ void __launch_bounds__(kEpiThreads)
longpair_prep_kernel(LongKeyParams k, const unsigned long long *__restrict__ sorted, const float *__restrict__ part,
                     int ptiles, float2 *__restrict__ prep)
{
    const EpiTile t = epi_tile(k, ptiles);
    const float inv = inv_maxdcg(part, t.q, ptiles);
    for (int x = threadIdx.x; x < t.real; x += kEpiThreads) {
        const int r = t.r0 + x;
        const int doc = long_doc(k, sorted[t.base + r], t.seed);
        const float G = ndcg_gain(load_label(k.rel, k.rel_dtype, t.base + doc)) * inv;
        prep[t.base + doc] = KIND == LTR_NDCG1 ? make_float2(G * inv_discount((float)r), 0.f) : make_float2(G, (float)r);
    }
}

// ---- the pair tile kernel ----
// pair_hinge with the gate decided on the exact score difference.  In fp32, d = s_k - s_m can round to exactly 1
// from above, and the pair is then active here and inactive in an fp64 evaluation (DESIGN.md 7 item 3).  At 4096
// documents that is a pair in 10^7; a 65 536-document list has 4.3e9 of them, so here the gate is taken on the
// difference of the scores widened to fp64 -- the fp64 evaluation's own d, exact unless the scores are 2^29 apart
// in magnitude -- at the cost of one v_add_f64 and two v_cmp_*_f64 for one v_cmp_ge_f32.
// Active pairs have u >= 0 in fp32 as well (rounding is monotone); term and derivative are pair_hinge's.
__device__ __forceinline__ void pair_hinge_exact(float sk, double skd, float yk, float sm, double smd, float ym,
                                                 float &g, float &l)
{
    const float d = sk - sm;
    const double dd = skd - smd;
    const bool gt = yk > ym, lt = yk < ym;
    const float u = gt ? (1.0f - d) : (1.0f + d);
    const bool act = (gt & (dd <= 1.0)) | (lt & (dd >= -1.0));
    l += (gt & act) ? u : 0.0f;
    g += act ? (gt ? -1.0f : 1.0f) : 0.0f;
}

template <int KIND> struct PairDoc { using type = float2; };                      // (score, label or a_m)
template <> struct PairDoc<LTR_NDCG2> { using type = float4; };                   // (score, label, gain, rank)

template <int KIND>
__global__ void __launch_bounds__(kPairThreads)
longpair_tile_kernel(LossParams p, const float2 *__restrict__ prep, float *__restrict__ part, int tiles)
{
    using Doc = typename PairDoc<KIND>::type;
    __shared__ __attribute__((aligned(16))) Doc s[kPairChunk];
    __shared__ float red[32];
    OwnerTile t;
    if (!owner_tile(p.n, p.L, 0, tiles, t)) return;
    const int tid = threadIdx.x, L = p.L, nb = t.nb, k0 = t.o0;
    const size_t row = t.row;
    const float c1 = p.sigma * kLog2e;
    constexpr bool kAllPairs = KIND == LTR_ARP1 || KIND == LTR_NDCG1;

    float sk[kPairDpt], yk[kPairDpt], Gk[kPairDpt], rk[kPairDpt], gk[kPairDpt];
    double skd[kPairDpt];                                   // the hinge kinds' gate (pair_hinge_exact)
#pragma unroll
    for (int c = 0; c < kPairDpt; ++c) {
        const int k = k0 + tid + c * kPairThreads;
        const bool valid = k < nb;
        // an idle owner: a_k = 0 (no loss) for the all-pairs kinds, a NaN label (both orientation tests fail) otherwise
        sk[c] = valid ? p.scores[row + k] : 0.f;
        yk[c] = valid ? load_label(p.rel, p.rel_dtype, row + k) : (kAllPairs ? 0.f : __builtin_nanf(""));
        skd[c] = (double)sk[c];
        Gk[c] = 0.f; rk[c] = 0.f; gk[c] = 0.f;
        if (KIND == LTR_NDCG1 || KIND == LTR_NDCG2) {
            const float2 v = valid ? prep[row + k] : make_float2(0.f, 0.f);
            if (KIND == LTR_NDCG1) yk[c] = v.x;
            else { Gk[c] = v.x; rk[c] = v.y; }
        }
    }

    float ltot = 0.f;
    for (int m0 = 0; m0 < nb; m0 += kPairChunk) {
        const int len = min(kPairChunk, nb - m0);
        __syncthreads();                                    // the chunk before this one has been read
        for (int x = tid; x < len; x += kPairThreads) {
            const size_t j = row + m0 + x;
            const float sc = p.scores[j];
            if constexpr (KIND == LTR_NDCG2) {
                const float2 v = prep[j];
                s[x] = make_float4(sc, load_label(p.rel, p.rel_dtype, j), v.x, v.y);
            } else if constexpr (KIND == LTR_NDCG1) {
                s[x] = make_float2(sc, prep[j].x);
            } else {
                s[x] = make_float2(sc, load_label(p.rel, p.rel_dtype, j));
            }
        }
        __syncthreads();
        float lc = 0.f, gc[kPairDpt];
#pragma unroll
        for (int c = 0; c < kPairDpt; ++c) gc[c] = 0.f;
        // one streamed document against the kPairDpt owned ones
        auto visit = [&](float sm, float ym, float Gm, float rm) {
            const double smd = (double)sm;
#pragma unroll
            for (int c = 0; c < kPairDpt; ++c) {
                if (KIND == LTR_NDCG2) {
                    // delta_d = |1 / D(d) - 1 / D(d + 1)|, d = |rank_k - rank_m| (fill_ndcg2_delta's entry; delta_0 = 0)
                    const float d = fabsf(rk[c] - rm);
                    const float delta = d >= 1.0f ? fabsf(inv_discount(d) - inv_discount(d + 1.0f)) : 0.f;
                    pair_oriented(sk[c], yk[c], sm, ym, delta * fabsf(Gk[c] - Gm), c1, gc[c], lc);
                } else if (KIND == LTR_HINGE || KIND == LTR_DCG_HINGE) {
                    pair_hinge_exact(sk[c], skd[c], yk[c], sm, smd, ym, gc[c], lc);
                } else if (KIND == LTR_LOGISTIC) {
                    pair_oriented(sk[c], yk[c], sm, ym, 1.0f, c1, gc[c], lc);
                } else if (KIND == LTR_ARP2) {
                    pair_oriented(sk[c], yk[c], sm, ym, fabsf(yk[c] - ym), c1, gc[c], lc);
                } else {
                    pair_rowweight(sk[c], yk[c], sm, ym, c1, gc[c], lc);
                }
            }
        };
        if constexpr (KIND == LTR_NDCG2) {
            float4_rounds(s, len, [&](const auto &v, int) {
#pragma unroll
                for (const float4 &d : v) visit(d.x, d.y, d.z, d.w);
            });
        } else {
            // the float2 kinds: eight documents per round of four ds_read_b128
            const float4 *s4 = reinterpret_cast<const float4 *>(s);
            const int full = len - len % 8;
            for (int m = 0; m < full; m += 8) {
                float4 v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = s4[m / 2 + j];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    visit(v[j].x, v[j].y, 0.f, 0.f);
                    visit(v[j].z, v[j].w, 0.f, 0.f);
                }
            }
            for (int m = full; m < len; ++m) visit(s[m].x, s[m].y, 0.f, 0.f);
        }
        ltot += lc;
#pragma unroll
        for (int c = 0; c < kPairDpt; ++c) gk[c] += gc[c];
    }

    tile_loss(ltot, red, part, t, tiles);
    if (p.dscores != nullptr) {
#pragma unroll
        for (int c = 0; c < kPairDpt; ++c) {
            const int k = k0 + tid + c * kPairThreads;
            if (k < L) p.dscores[row + k] = k < nb ? gk[c] : 0.f;
        }
    }
}

// grid (B, ceil(L / 256)), like pairwise_loss_finish_kernel: the tile partials in tile order, the loss modifier,
// the gradient scale (1, sigma / ln 2, or the DCG-hinge factor) applied in place, zeros for j >= n[b].
template <int KIND>
__global__ void __launch_bounds__(256)
longpair_finish_kernel(LossParams p, const float *__restrict__ part, int tiles)
{
    const int b = blockIdx.x;
    const int L = p.L;
    const int nb = clamp_n(p.n[b], L);
    float total = tile_loss_sum(part, b, tiles, nb);        // every thread, same order
    float gscale = 1.0f;
    if (KIND == LTR_DCG_HINGE) {
        const float lg = logf(2.0f + total);
        gscale = 1.0f / ((2.0f + total) * lg * lg);
        total = -1.0f / lg;
    } else if (KIND != LTR_HINGE) {
        gscale = p.sigma / kLn2;
    }
    if (threadIdx.x == 0 && blockIdx.y == 0) p.loss[b] = total;
    if (p.dscores != nullptr) {
        const int k = blockIdx.y * blockDim.x + threadIdx.x;
        if (k < L) {
            float *g = p.dscores + (size_t)b * L + k;
            *g = k < nb ? *g * gscale : 0.f;
        }
    }
}

// ---- host side ----
struct LongPairWorkspace {
    float *part;          // (B, tiles) loss partials
    float2 *prep;         // (B, L), the LambdaNDCG kinds
    LongWorkspace sort;   // ... and their sort workspace (ltr_sort_workspace_bytes(1, B, L))
};

// The workspace of ltr_pairwise_loss_long_workspace_bytes (include/ltr_longpair.h states the byte formula).
inline LongPairWorkspace long_pair_workspace(Carver &c, int kind, int B, int L)
{
    LongPairWorkspace w{};
    w.part = c.take<float>((size_t)B * (size_t)long_pair_tiles(L)); c.align256();
    if (kind == LTR_NDCG1 || kind == LTR_NDCG2) {
        w.prep = c.take<float2>((size_t)B * (size_t)L); c.align256();
        w.sort = long_workspace(c, B, L, true);
    }
    return w;
}

template <int KIND>
void launch_long_pair_prep(const LossParams &p, const LongPairWorkspace &w, hipStream_t s)
{
    const int B = p.B, etiles = long_epi_tiles(p.L);
    const dim3 grid((unsigned)((size_t)B * etiles)), block(kEpiThreads);
    // maxDCG: the DCG terms of the ideal ranking over the real documents, per tile
    const RankedKeys r = long_ndcg_sorts(p.scores, p.rel, p.rel_dtype, p.n, B, p.L, w.sort, s,
                                         [&](const LongKeyParams &ik, const unsigned long long *ideal) {
        LongMetricParams ip{};
        ip.k = ik; ip.sorted = ideal;
        ip.ideal = 1; ip.use_exp = 1; ip.lim = -1;
        ip.tiles = ip.ptiles = etiles;
        ip.part = w.sort.part;
        hipLaunchKernelGGL(longsort_partial_kernel<METRIC_DCG>, grid, block, 0, s, ip);
    });
    hipLaunchKernelGGL((longpair_prep_kernel<KIND>), grid, block, 0, s, r.k, r.sorted, (const float *)w.sort.part, etiles, w.prep);
}

template <int KIND>
int launch_long_pair(const LossParams &p, const LongPairWorkspace &w, hipStream_t s)
{
    if constexpr (KIND == LTR_NDCG1 || KIND == LTR_NDCG2) launch_long_pair_prep<KIND>(p, w, s);
    const int tiles = long_pair_tiles(p.L);
    hipLaunchKernelGGL((longpair_tile_kernel<KIND>), dim3((unsigned)((size_t)p.B * tiles)), dim3(kPairThreads), 0, s, p,
                       (const float2 *)w.prep, w.part, tiles);
    hipLaunchKernelGGL((longpair_finish_kernel<KIND>), dim3((unsigned)p.B, (unsigned)((p.L + 255) / 256)), dim3(256), 0, s,
                       p, (const float *)w.part, tiles);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int ltr_max_pair_list_len(void) { return kMaxPairListLen; }

void ltr_long_pair_geometry(int *owner_docs, int *chunk_docs)
{
    if (owner_docs) *owner_docs = kPairOwn;
    if (chunk_docs) *chunk_docs = kPairChunk;
}

LTR_DEBUG_HOOK int ltr_debug_long_pairs_all(int on)
{
    return __atomic_exchange_n(&g_long_pairs_all, on ? 1 : 0, __ATOMIC_RELAXED);
}

size_t ltr_pairwise_loss_long_workspace_bytes(int kind, int B, int L)
{
    if (check_kind(kind, LTR_LABEL_I64) != LTR_OK || check_lists(B, L, kMaxPairListLen) != LTR_OK) return 0;
    if (!long_pairs(L)) return 0;
    Carver sizes(nullptr);
    long_pair_workspace(sizes, kind, B, L);
    return sizes.off;
}

int ltr_pairwise_loss_long_f32(int kind, float sigma, const float *scores, const void *rel, int rel_dtype,
                               const int64_t *n, int B, int L, float *loss, float *dscores, void *workspace,
                               size_t workspace_bytes, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (const int rc = check_kind(kind, rel_dtype)) return rc;
    if (const int rc = check_lists(B, L, kMaxPairListLen)) return rc;
    if (B == 0) return LTR_OK;
    if (!scores || !rel || !n || !loss) return LTR_ERR_NULL;
    if (!long_pairs(L))
        return ltr_pairwise_loss_f32(kind, sigma, scores, rel, rel_dtype, n, B, L, loss, dscores, stream);
    Carver carver(workspace);
    const LongPairWorkspace w = long_pair_workspace(carver, kind, B, L);
    if (!workspace || workspace_bytes < carver.off) return LTR_ERR_WORKSPACE;
    LossParams p{};
    p.scores = scores; p.rel = rel; p.n = n; p.loss = loss; p.dscores = dscores;
    p.B = B; p.L = L; p.sigma = sigma; p.rel_dtype = rel_dtype;
    return with_kind(kind, [&](auto K) { return launch_long_pair<K>(p, w, (hipStream_t)stream); });
}

}  // extern "C"
