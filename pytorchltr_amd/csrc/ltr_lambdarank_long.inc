// ltr_lambdarank_long.inc -- LambdaRank on lists longer than one workgroup's LDS (included by ltr_kernels.hip behind
// ltr_longsort.inc, ltr_longpair.inc and ltr_lambdarank.inc; C ABI: include/ltr_lambdarank_long.h; DESIGN.md 26).
//
// The loss is the one of ltr_lambdarank.inc; lambdarank_kernel keeps a whole query in LDS, which stops at 4096
// documents.  Past that everything is laid out BY RANK in the caller's workspace and the pair pass is built on the
// owner-tile core of ltr_longpair.inc (its geometry, tile decode, float4 rounds and loss partials; the two sorts and
// the maxDCG head of its NDCG preparation):
//   1. the ranking: the long key sort on the scores, ties in document-index order;
//   2. maxDCG@K_b: the label sort, then tile partials of gain x discount over the ranks below K_b = min(k, n_b), added
//      in tile order (lambdarank_row's terms: ndcg_gain, inv_discount, one fma per rank);
//   3. an epilogue over the sorted score keys writes (score, label) and (G, d) by rank -- d = 0 from rank K_b on --
//      and the document behind each rank;
//   4. the pair pass, one workgroup per tile of kPairOwn ranks: a thread OWNS kPairDpt ranks in registers, the workgroup
//      streams the anchors [0, K_b) through LDS, kPairChunk at a time, every thread reading the same LDS address per
//      step (broadcast), and evaluates lambdarank_pair itself.  That is every pair an owner has: the whole gradient
//      of a rank >= K_b, the part within the top K_b of an anchor, and the loss of every pair, counted once by its
//      lower-ranked member (a < r).
//      The anchors' pairs with the tail [K_b, n_b) are these same evaluations seen from the other end: what a pair
//      gives its tail owner, it takes from its anchor (lambda_ij leaves i and enters j; the terms are the same
//      bits with the other sign).  So a tile that owns ranks of the tail also sums, per streamed anchor, what its
//      tail owners received -- in the thread over its ranks, over the wave by DPP, over the waves through LDS in wave
//      order -- and stores MINUS that as the tile's partial gradient of the anchor.  The anchor x tail part is thus
//      spread over the tail as the tail's tiles are: 63 workgroups per query at k = 10 and 65 536 documents, each
//      evaluating its 1024 x 10 pairs once; nothing walks the whole tail, no pair is evaluated a second time, and no
//      atomics.  Owner groups of a wave that lie wholly past n_b are skipped by a wave-uniform branch;
//   5. finish: the loss partials in tile order; per rank the pair pass's gradient plus, for an anchor, the tail tiles'
//      partials in tile order, scaled by sigma / ln 2 once, scattered from rank to document; zeros past n_b.
// Sums are two-level (per chunk, then over the chunks; tile partials in tile order).  No atomics, no host
// synchronisation, all memory the caller's: bit-identical run to run, capturable.

#include "ltr_lambdarank_long.h"

namespace {

constexpr int kLrSub = 256;                      // anchors whose wave sums are handed over at a time (4 KiB)
static_assert(kLrSub % 4 == 0 && kLrSub <= kPairThreads && kPairChunk % kLrSub == 0, "one thread per handed-over anchor");

int g_lambdarank_long_all = 0;                   // ltr_debug_lambdarank_long_all
inline bool lambdarank_long(int L) { return long_or_forced(L, g_lambdarank_long_all); }

struct LambdaRankLongParams {
    const float *scores;
    const void *rel;
    const int64_t *n;
    float *loss, *dscores;   // (B), (B, L) or null
    int rel_dtype, B, L;
    int k;                   // <= 0: no cutoff
    float sigma;
    // the workspace (lambdarank_long_workspace)
    float2 *sl, *gd;         // (B, L) by rank: (score, label), (G, d)
    int *doc;                // (B, L) the document behind each rank
    float *graw;             // (B, L) by rank: the owners' gradient in units of sigma / ln 2
    float *part;             // (B, tiles) loss partials
    float *ganch;            // (B, ttiles, kcap): the anchors' partial gradients from the tiles that own ranks of the tail
    int tiles;               // long_pair_tiles(L)
    int kcap;                // k where a tail can exist (0 < k < L), else 0
    int ttile0, ttiles;      // the first tile with a rank >= kcap, floor(kcap / kPairOwn); tiles - ttile0
};

__device__ __forceinline__ int lambdarank_cutoff(int k, int nb) { return k > 0 ? min(k, nb) : nb; }

// 2. tile partials of maxDCG@K_b over the label-sorted keys (the label is in the key)
__global__ void __launch_bounds__(kEpiThreads)
lambdarank_long_maxdcg_kernel(LongKeyParams k, const unsigned long long *__restrict__ sorted, int cutoff,
                              float *__restrict__ part, int ptiles)
{
    __shared__ float red[32];
    const EpiTile t = epi_tile(k, ptiles);
    const int K = lambdarank_cutoff(cutoff, t.nb);
    float a = 0.f;
    for (int x = threadIdx.x; x < kEpiTile; x += kEpiThreads) {
        const int r = t.r0 + x;
        if (r >= K) break;
        a = __builtin_fmaf(ndcg_gain(long_key_value(sorted[t.base + r])), inv_discount((float)r), a);
    }
    a = block_sum(a, red);
    if (threadIdx.x == 0) part[(size_t)t.q * ptiles + t.tile] = a;
}

// 3. the by-rank arrays from the sorted score keys
__global__ void __launch_bounds__(kEpiThreads)
lambdarank_long_byrank_kernel(LongKeyParams k, const unsigned long long *__restrict__ sorted,
                              const float *__restrict__ part, int ptiles, LambdaRankLongParams p)
{
    const EpiTile t = epi_tile(k, ptiles);
    const int K = lambdarank_cutoff(p.k, t.nb);
    const float inv = inv_maxdcg(part, t.q, ptiles);
    for (int x = threadIdx.x; x < t.real; x += kEpiThreads) {
        const int r = t.r0 + x;
        const int doc = long_doc(k, sorted[t.base + r], t.seed);
        const float y = load_label(p.rel, p.rel_dtype, t.base + doc);
        p.sl[t.base + r] = make_float2(p.scores[t.base + doc], y);
        p.gd[t.base + r] = make_float2(ndcg_gain(y) * inv, r < K ? inv_discount((float)r) : 0.f);
        p.doc[t.base + r] = doc;
    }
}

// 4. the pair pass: the ranks [tile kPairOwn, ...) of query b against the anchors [0, K_b), for the tiles
// [tile0, tile0 + ntiles) of every query.  FEEDS: these tiles may own ranks of the tail and then leave the anchors' share
// of their pairs (the host launches the tiles below floor(k / kPairOwn), a forward-only call and a call without a cutoff
// with FEEDS = false: no wave sums, half the LDS, fewer registers).  Both forms add the loss in the same order.
template <bool FEEDS>
__global__ void __launch_bounds__(kPairThreads)
lambdarank_long_pass_kernel(LambdaRankLongParams p, int tile0, int ntiles)
{
    constexpr int SUB = FEEDS ? kLrSub : kPairChunk;                              // anchors between two hand-overs of wave sums
    __shared__ __attribute__((aligned(16))) float4 s[kPairChunk];                 // (score, label, G, d) by rank
    __shared__ __attribute__((aligned(16))) float wsum[FEEDS ? kPairWaves : 1][FEEDS ? kLrSub : 4];   // per anchor and wave
    __shared__ float red[32];
    OwnerTile t;
    if (!owner_tile(p.n, p.L, tile0, ntiles, t)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nb = t.nb, o0 = t.o0;
    const int K = lambdarank_cutoff(p.k, nb);
    const size_t row = t.row;
    const float c1 = p.sigma * kLog2e;
    const bool grad = p.dscores != nullptr;
    // this tile owns ranks of the tail: it also leaves the anchors' share of its pairs (K < n_b: K = kcap)
    const bool feeds = FEEDS && grad && K < nb && o0 + kPairOwn > K;
    float *anch = feeds ? p.ganch + ((size_t)t.b * p.ttiles + (size_t)(t.tile - p.ttile0)) * (size_t)p.kcap : nullptr;

    float2 own[kPairDpt], ogd[kPairDpt];
    float gk[kPairDpt];
    int nc = 0;                                             // owner groups of this wave with a rank below n_b
#pragma unroll
    for (int c = 0; c < kPairDpt; ++c) {
        const int r = o0 + tid + c * kPairThreads;
        const bool valid = r < nb;
        // an idle owner: a NaN label, so both orientation tests of lambdarank_pair fail
        own[c] = valid ? p.sl[row + r] : make_float2(0.f, __builtin_nanf(""));
        ogd[c] = valid ? p.gd[row + r] : make_float2(0.f, 0.f);
        gk[c] = 0.f;
        nc += (o0 + (tid & ~63) + c * kPairThreads) < nb ? 1 : 0;
    }
    nc = __builtin_amdgcn_readfirstlane(nc);

    float ltot = 0.f;
    for (int m0 = 0; m0 < K; m0 += kPairChunk) {
        const int len = min(kPairChunk, K - m0);
        __syncthreads();                                    // the chunk before this one has been read
        for (int x = tid; x < len; x += kPairThreads) {
            const float2 a = p.sl[row + m0 + x], g = p.gd[row + m0 + x];
            s[x] = make_float4(a.x, a.y, g.x, g.y);
        }
        __syncthreads();
        float lc = 0.f, gc[kPairDpt];
#pragma unroll
        for (int c = 0; c < kPairDpt; ++c) gc[c] = 0.f;
        // one streamed anchor `a` against the owned ranks; returns what this thread's tail owners received from it
        auto visit = [&](float4 v, int a) {
            float tail = 0.f;
#pragma unroll
            for (int c = 0; c < kPairDpt; ++c) {
                if (c < nc) {
                    const int r = o0 + tid + c * kPairThreads;
                    float d = 0.f;
                    lambdarank_pair(own[c], ogd[c], make_float2(v.x, v.y), make_float2(v.z, v.w), c1, a < r, d, lc);
                    gc[c] += d;
                    if (FEEDS) tail += r >= K ? d : 0.f;
                }
            }
            return tail;
        };
        for (int q0 = 0; q0 < len; q0 += SUB) {
            const int qlen = min(SUB, len - q0);
            float4_rounds(s + q0, qlen, [&](const auto &v, int m) {
                constexpr int N = sizeof(v) / sizeof(float4);
                float w[N];
#pragma unroll
                for (int j = 0; j < N; ++j) w[j] = visit(v[j], m0 + q0 + m + j);
                if (feeds) {                                // uniform; one ds_write_b128 per full round
#pragma unroll
                    for (int j = 0; j < N; ++j) w[j] = wave_sum(w[j]);
                    if (lane == 0) __builtin_memcpy(__builtin_assume_aligned(&wsum[wave][m], sizeof(w)), w, sizeof(w));
                }
            });
            if (feeds) {
                __syncthreads();
                if (tid < qlen) {
                    float a = wsum[0][tid];
#pragma unroll
                    for (int w = 1; w < kPairWaves; ++w) a += wsum[w][tid];       // wave order
                    anch[m0 + q0 + tid] = -a;
                }
                __syncthreads();                            // before the next hand-over overwrites the sums
            }
        }
        ltot += lc;
#pragma unroll
        for (int c = 0; c < kPairDpt; ++c) gk[c] += gc[c];
    }

    tile_loss(ltot, red, p.part, t, p.tiles);
    if (!grad) return;
#pragma unroll
    for (int c = 0; c < kPairDpt; ++c) {
        const int r = o0 + tid + c * kPairThreads;
        if (r < nb) p.graw[row + r] = gk[c];
    }
}

// 5. grid (B, ceil(L / 256)): the loss partials in tile order; thread x < n_b finishes RANK x -- the pair pass's gradient
// plus, for an anchor, the partials of the tiles that own ranks of the tail, in tile order, scaled by sigma / ln 2 once --
// and stores it at the rank's document; thread x >= n_b zeroes the padded slot x (the documents behind the ranks below
// n_b are exactly the slots below n_b).
__global__ void __launch_bounds__(256)
lambdarank_long_finish_kernel(LambdaRankLongParams p)
{
    const int b = blockIdx.x;
    const int L = p.L;
    const int nb = clamp_n(p.n[b], L);
    const int K = lambdarank_cutoff(p.k, nb);
    if (blockIdx.y == 0 && threadIdx.x == 0) p.loss[b] = tile_loss_sum(p.part, b, p.tiles, nb);
    if (p.dscores == nullptr) return;
    const int x = blockIdx.y * blockDim.x + threadIdx.x;
    if (x >= L) return;
    const size_t row = (size_t)b * L;
    if (x >= nb) {
        p.dscores[row + x] = 0.f;
        return;
    }
    float g = p.graw[row + x];
    if (x < K && K < nb)
        for (int t = p.ttile0; t < long_pair_tiles(nb); ++t) g += p.ganch[((size_t)b * p.ttiles + (size_t)(t - p.ttile0)) * (size_t)p.kcap + x];
    p.dscores[row + p.doc[row + x]] = g * (p.sigma * kLog2e);
}

// ---- host side ----
struct LambdaRankLongWorkspace {
    float *part, *graw, *ganch;
    float2 *sl, *gd;
    int *doc;
    int kcap, ttile0, ttiles;
    LongWorkspace sort;      // ltr_sort_workspace_bytes(1, B, L): the key ping-pong and the maxDCG tile partials
};

// The workspace of ltr_lambdarank_long_workspace_bytes (include/ltr_lambdarank_long.h states the byte formula).
inline LambdaRankLongWorkspace lambdarank_long_workspace(Carver &c, int k, int B, int L)
{
    LambdaRankLongWorkspace w{};
    const size_t BL = (size_t)B * (size_t)L;
    w.kcap = (k > 0 && k < L) ? k : 0;
    w.ttile0 = w.kcap / kPairOwn;
    w.ttiles = w.kcap ? long_pair_tiles(L) - w.ttile0 : 0;
    w.sl = c.take<float2>(BL); c.align256();
    w.gd = c.take<float2>(BL); c.align256();
    w.doc = c.take<int>(BL); c.align256();
    w.graw = c.take<float>(BL); c.align256();
    w.part = c.take<float>((size_t)B * (size_t)long_pair_tiles(L)); c.align256();
    w.ganch = c.take<float>((size_t)B * (size_t)w.ttiles * (size_t)w.kcap); c.align256();
    w.sort = long_workspace(c, B, L, true);
    return w;
}

int launch_lambdarank_long(LambdaRankLongParams p, const LambdaRankLongWorkspace &w, hipStream_t s)
{
    const int B = p.B, L = p.L;
    p.sl = w.sl; p.gd = w.gd; p.doc = w.doc; p.graw = w.graw; p.part = w.part; p.ganch = w.ganch;
    p.tiles = long_pair_tiles(L);
    p.kcap = w.kcap; p.ttile0 = w.ttile0; p.ttiles = w.ttiles;
    const int etiles = long_epi_tiles(L);
    const dim3 egrid((unsigned)((size_t)B * etiles)), eblock(kEpiThreads);
    // maxDCG: the ideal ranking's terms below the cutoff per tile; then everything by rank
    const RankedKeys r = long_ndcg_sorts(p.scores, p.rel, p.rel_dtype, p.n, B, L, w.sort, s,
                                         [&](const LongKeyParams &ik, const unsigned long long *ideal) {
        hipLaunchKernelGGL(lambdarank_long_maxdcg_kernel, egrid, eblock, 0, s, ik, ideal, p.k, w.sort.part, etiles);
    });
    hipLaunchKernelGGL(lambdarank_long_byrank_kernel, egrid, eblock, 0, s, r.k, r.sorted, (const float *)w.sort.part, etiles, p);
    // the tiles that cannot own a rank of the tail, then those that can (none in a forward-only call or without a cutoff)
    const int split = (p.dscores != nullptr && p.kcap > 0) ? p.ttile0 : p.tiles;
    if (split > 0)
        hipLaunchKernelGGL(lambdarank_long_pass_kernel<false>, dim3((unsigned)((size_t)B * split)), dim3(kPairThreads), 0, s,
                           p, 0, split);
    if (split < p.tiles)
        hipLaunchKernelGGL(lambdarank_long_pass_kernel<true>, dim3((unsigned)((size_t)B * (p.tiles - split))),
                           dim3(kPairThreads), 0, s, p, split, p.tiles - split);
    hipLaunchKernelGGL(lambdarank_long_finish_kernel, dim3((unsigned)B, (unsigned)((L + 255) / 256)), dim3(256), 0, s, p);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

LTR_DEBUG_HOOK int ltr_debug_lambdarank_long_all(int on)
{
    return __atomic_exchange_n(&g_lambdarank_long_all, on ? 1 : 0, __ATOMIC_RELAXED);
}

size_t ltr_lambdarank_long_workspace_bytes(int k, int B, int L)
{
    if (check_lists(B, L, kMaxPairListLen) != LTR_OK || !lambdarank_long(L)) return 0;
    Carver sizes(nullptr);
    lambdarank_long_workspace(sizes, k, B, L);
    return sizes.off;
}

int ltr_lambdarank_long_f32(const float *scores, const void *rel, int rel_dtype, const int64_t *n, int k, float sigma,
                            int B, int L, float *loss, float *dscores, void *workspace, size_t workspace_bytes,
                            void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (bad_label_dtype(rel_dtype)) return LTR_ERR_KIND;
    if (B < 0 || L <= 0 || !std::isfinite(sigma)) return LTR_ERR_SHAPE;
    if (L > kMaxPairListLen) return LTR_ERR_LIST_TOO_LONG;
    if (B == 0) return LTR_OK;
    if (!scores || !rel || !n || !loss) return LTR_ERR_NULL;
    if (!lambdarank_long(L)) return ltr_lambdarank_f32(scores, rel, rel_dtype, n, k, sigma, B, L, loss, dscores, stream);
    Carver carver(workspace);
    const LambdaRankLongWorkspace w = lambdarank_long_workspace(carver, k, B, L);
    if (!workspace || workspace_bytes < carver.off) return LTR_ERR_WORKSPACE;
    if (const int st = status_peek()) return st;           // a kernel of an earlier call gave up
    LambdaRankLongParams p{};
    p.scores = scores; p.rel = rel; p.n = n; p.loss = loss; p.dscores = dscores;
    p.rel_dtype = rel_dtype; p.B = B; p.L = L; p.k = k; p.sigma = sigma;
    return launch_lambdarank_long(p, w, (hipStream_t)stream);
}

}  // extern "C"
