// ltr_longsort.inc -- rankings and ranking metrics on lists longer than one workgroup's LDS
// (included by ltr_kernels.hip; C ABI: the ltr_*_long_f32 entry points of include/ltr_hip.h).
//
// The one-workgroup-per-query metric kernel keeps a whole query in LDS, which stops at 4096
// documents.  Past that, every document becomes one 64-bit key
//     (score-order bits of rank_key, capped at 0xFFFFFFFE) << 32 | tie word
// -- padded documents (j >= n[b]) get 0xFFFFFFFF << 32 | j, so they follow every real document
// in index order --, the keys are unique, and any correct sort of them is THE ranking:
//   1. a chunk sort: one workgroup sorts kSortChunk keys of a query in LDS (bitonic network) and
//      writes one sorted run;
//   2. ceil(log2(L / kSortChunk)) merge passes, global to global: every workgroup merges one
//      kMergeTile-key slice of the output of a pair of runs, its slice found by a merge-path
//      search (equal work per workgroup, however few the queries); runs never cross queries and
//      all queries share each pass's launch;
//   3. epilogues over the sorted keys: the ranking itself (fused into the last pass), or tile
//      partial sums of DCG terms / ARP products, a fixed-order finish per query (@k, arp), or a
//      segmented prefix scan for the DCG curve (tile sums, then each tile adds the sum of the
//      tiles before it).  No atomics anywhere: the results are bit-identical run to run.
// All memory comes from the caller's workspace (keys ping-pong, the inverse of an explicit tie
// permutation, the tile partials), so the path records under stream capture as it is.

namespace {

constexpr int kMaxSortListLen = 1 << 24;     // the low key word holds a position (< 2^24 keeps fp32 ranks exact)
constexpr int kSortChunk = 8192;             // keys one workgroup sorts in LDS (64 KiB)
constexpr int kChunkThreads = 1024;
constexpr int kMergeTile = 4096;             // output keys of one merge workgroup (32 KiB of LDS)
constexpr int kMergeThreads = 512;
constexpr int kMergeE = kMergeTile / kMergeThreads;
constexpr int kEpiTile = 4096;               // sorted positions of one epilogue workgroup
constexpr int kEpiThreads = 256;
constexpr int kEpiE = kEpiTile / kEpiThreads;
constexpr unsigned long long kPadKeyHi = 0xFFFFFFFFull << 32;

enum { TIE_INDEX = 0, TIE_EXPLICIT = 1, TIE_SEED = 2 };

// The long tie word: a keyed bijection of the 32-bit positions (include/ltr_hip.h states it), so
// it is inverted to recover the document instead of carrying a payload next to the key.
constexpr unsigned odd_inverse(unsigned a)
{
    unsigned x = a;                              // Newton: every step doubles the correct low bits
    for (int i = 0; i < 5; ++i) x *= 2u - a * x;
    return x;
}
constexpr unsigned kLongM1 = 0x9E3779B1u, kLongM2 = 0x85EBCA6Bu;
constexpr unsigned kLongM1Inv = odd_inverse(kLongM1), kLongM2Inv = odd_inverse(kLongM2);
static_assert(kLongM1 * kLongM1Inv == 1u && kLongM2 * kLongM2Inv == 1u, "odd constants must be invertible");

__host__ __device__ inline unsigned tie_hash_word_long(unsigned long long seed, unsigned j)
{
    unsigned x = (j ^ (unsigned)seed) * kLongM1;
    x ^= x >> 16;
    x *= kLongM2;
    return x ^ (unsigned)(seed >> 32);
}

__host__ __device__ inline unsigned tie_hash_word_long_inverse(unsigned long long seed, unsigned w)
{
    unsigned x = (w ^ (unsigned)(seed >> 32)) * kLongM2Inv;
    x ^= x >> 16;                                // an xorshift by >= 16 is its own inverse
    return (x * kLongM1Inv) ^ (unsigned)seed;
}

// Where the keys come from and how a key's low word maps back to its document.
struct LongKeyParams {
    const float *scores;          // score keys; null: label keys (the ideal ranking, index words)
    const void *rel;
    int rel_dtype;
    const int64_t *n;
    const int32_t *tie;           // TIE_EXPLICIT: (L) priorities
    const int *inv_tie;           //   and their inverse (workspace)
    unsigned long long seed;      // TIE_SEED
    const int64_t *seed_dev;      //   overrides seed when not null
    int mode;
    int L;
};

__device__ __forceinline__ unsigned long long long_seed(const LongKeyParams &k)
{
    if (k.mode != TIE_SEED) return 0ull;
    return k.seed_dev ? (unsigned long long)k.seed_dev[0] : k.seed;
}

// Where a key's high word comes from: KEY_SCORES, the scores (or, when k.scores is null, the labels with index words:
// the ideal ranking); KEY_LABELS_TIED, the labels with the call's tie words (ListMLE's ranking, ltr_listmle.inc).
enum { KEY_SCORES = 0, KEY_LABELS_TIED = 1 };

template <int SRC = KEY_SCORES>
__device__ __forceinline__ unsigned long long long_key(const LongKeyParams &k, size_t base, int j, int nb,
                                                       unsigned long long seed)
{
    if (j >= nb) return kPadKeyHi | (unsigned)j;
    const bool tied = SRC == KEY_LABELS_TIED || k.scores;
    const float v = (SRC == KEY_SCORES && k.scores) ? k.scores[base + j] : load_label(k.rel, k.rel_dtype, base + j);
    unsigned hi = (unsigned)(rank_key(v, 0) >> 32);
    hi = hi < 0xFFFFFFFFu ? hi : 0xFFFFFFFEu;    // (one NaN payload) real documents stay ahead of the padding
    unsigned w = (unsigned)j;
    if (tied && k.mode == TIE_EXPLICIT) w = (unsigned)k.tie[j];
    else if (tied && k.mode == TIE_SEED) w = tie_hash_word_long(seed, (unsigned)j);
    return ((unsigned long long)hi << 32) | w;
}

// The document behind a real document's key (clamped into the row: an explicit tie array that is
// not a permutation gives a wrong order, never an out-of-row read).
__device__ __forceinline__ int long_doc(const LongKeyParams &k, unsigned long long key, unsigned long long seed)
{
    const unsigned w = (unsigned)key;
    unsigned d = w;
    if (k.mode == TIE_EXPLICIT) d = w < (unsigned)k.L ? (unsigned)k.inv_tie[w] : 0u;
    else if (k.mode == TIE_SEED) d = tie_hash_word_long_inverse(seed, w);
    return (int)(d < (unsigned)k.L ? d : (unsigned)(k.L - 1));
}

// The value a label key was made from (rank_key inverted; -0.0 comes back as +0.0, same gain).
__device__ __forceinline__ float long_key_value(unsigned long long key)
{
    const unsigned asc = ~(unsigned)(key >> 32);
    return __uint_as_float((asc & 0x80000000u) ? (asc & 0x7FFFFFFFu) : ~asc);
}

__global__ void __launch_bounds__(256) longsort_inverse_tie_kernel(const int32_t *__restrict__ tie, int L, int *__restrict__ inv)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < L) {
        const unsigned t = (unsigned)tie[j];
        if (t < (unsigned)L) inv[t] = j;
    }
}

// 1. one sorted run of kSortChunk keys per workgroup.  RANK_OUT (a query that is one chunk): the
// ranking is written instead of the keys.  SRC: long_key's key source.
template <bool RANK_OUT, int SRC = KEY_SCORES>
__global__ void __launch_bounds__(kChunkThreads)
longsort_chunk_kernel(LongKeyParams k, int chunks, unsigned long long *__restrict__ keys_out, int64_t *__restrict__ ranking)
{
    __shared__ unsigned long long s[kSortChunk];
    const int q = blockIdx.x / chunks, c = blockIdx.x - q * chunks;
    const int L = k.L, tid = threadIdx.x;
    const size_t base = (size_t)q * L;
    const int j0 = c * kSortChunk;
    const int len = min(kSortChunk, L - j0);
    const int nb = clamp_n(k.n[q], L);
    const unsigned long long seed = long_seed(k);
    int P = 64;
    while (P < len) P <<= 1;
    for (int x = tid; x < P; x += kChunkThreads) s[x] = x < len ? long_key<SRC>(k, base, j0 + x, nb, seed) : ~0ull;
    __syncthreads();
    for (int kk = 2; kk <= P; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < (P >> 1); i += kChunkThreads) {
                const int lo = 2 * i - (i & (j - 1)), hi = lo + j;
                const unsigned long long a = s[lo], b = s[hi];
                if ((a > b) == ((lo & kk) == 0)) { s[lo] = b; s[hi] = a; }
            }
            __syncthreads();
        }
    }
    for (int x = tid; x < len; x += kChunkThreads) {
        const int r = j0 + x;
        if (RANK_OUT) ranking[base + r] = r < nb ? long_doc(k, s[x], seed) : r;
        else keys_out[base + r] = s[x];
    }
}

// 2. one merge pass: runs of W keys (per query) are merged pairwise into runs of 2W.  Workgroup t
// of a query produces output keys [t * kMergeTile, ...) of its pair (2W is a multiple of the tile).
template <bool RANK_OUT>
__global__ void __launch_bounds__(kMergeThreads)
longsort_merge_kernel(LongKeyParams k, int tiles, int W, const unsigned long long *__restrict__ in,
                      unsigned long long *__restrict__ out, int64_t *__restrict__ ranking)
{
    __shared__ unsigned long long s[kMergeTile];
    __shared__ int split[2];
    const int q = blockIdx.x / tiles, t = blockIdx.x - q * tiles;
    const int L = k.L, tid = threadIdx.x;
    const size_t base = (size_t)q * L;
    const int o0 = t * kMergeTile;
    const int pair0 = o0 - o0 % (2 * W);
    const int aEnd = min(pair0 + W, L), bEnd = min(pair0 + 2 * W, L);
    const int lenA = aEnd - pair0, lenB = bEnd - aEnd;
    const int d0 = o0 - pair0, d1 = min(d0 + kMergeTile, lenA + lenB);
    const unsigned long long *A = in + base + pair0, *Bk = in + base + aEnd;
    if (tid < 2) {
        // merge path: how many of the first d outputs come from run A (keys are unique)
        const int d = tid ? d1 : d0;
        int lo = max(0, d - lenB), hi = min(d, lenA);
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (A[mid] < Bk[d - 1 - mid]) lo = mid + 1;
            else hi = mid;
        }
        split[tid] = lo;
    }
    __syncthreads();
    const int a0 = split[0], a1 = split[1];
    const int na = a1 - a0, nbk = (d1 - a1) - (d0 - a0);
    const int total = na + nbk;
    for (int x = tid; x < na; x += kMergeThreads) s[x] = A[a0 + x];
    for (int x = tid; x < nbk; x += kMergeThreads) s[na + x] = Bk[d0 - a0 + x];
    __syncthreads();
    unsigned long long v[kMergeE];
    const int dd = tid * kMergeE;
    if (dd < total) {
        const unsigned long long *sa = s, *sb = s + na;
        int lo = max(0, dd - nbk), hi = min(dd, na);
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sa[mid] < sb[dd - 1 - mid]) lo = mid + 1;
            else hi = mid;
        }
        int i = lo, j = dd - lo;
#pragma unroll
        for (int e = 0; e < kMergeE; ++e) {
            if (dd + e < total) {
                const bool take_a = i < na && (j >= nbk || sa[i] < sb[j]);
                v[e] = take_a ? sa[i] : sb[j];
                i += take_a ? 1 : 0;
                j += take_a ? 0 : 1;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < kMergeE; ++e)
        if (dd + e < total) s[dd + e] = v[e];
    __syncthreads();
    if (RANK_OUT) {
        const int nb = clamp_n(k.n[q], L);
        const unsigned long long seed = long_seed(k);
        for (int x = tid; x < total; x += kMergeThreads) {
            const int r = pair0 + d0 + x;
            ranking[base + r] = r < nb ? long_doc(k, s[x], seed) : r;
        }
    } else {
        for (int x = tid; x < total; x += kMergeThreads) out[base + pair0 + d0 + x] = s[x];
    }
}

// 3. epilogues (the semantics of the one-workgroup kernels: padded labels counted by dcg, gains 2^y - 1 or y,
// discount 1 / log2(r + 2), arp over the real documents).
// The tile of one epilogue workgroup: query q (its row at `base`, nb real documents, tie seed), tile `tile` of the
// `tiles` per query of the launch: sorted positions [r0, r0 + span) of the row, the first `real` of them real documents.
struct EpiTile { int q, tile, r0, span, real, nb; size_t base; unsigned long long seed; };
__device__ __forceinline__ EpiTile epi_tile(const LongKeyParams &k, int tiles)
{
    EpiTile t;
    t.q = blockIdx.x / tiles;
    t.tile = blockIdx.x - t.q * tiles;
    t.base = (size_t)t.q * k.L;
    t.nb = clamp_n(k.n[t.q], k.L);
    t.seed = long_seed(k);
    t.r0 = t.tile * kEpiTile;
    t.span = min(kEpiTile, k.L - t.r0);
    t.real = max(0, min(kEpiTile, t.nb - t.r0));
    return t;
}

struct LongMetricParams {
    LongKeyParams k;                     // the keys `sorted` holds
    const unsigned long long *sorted;    // (B, L)
    int ideal;                           // label keys: the gain comes from the key itself
    int lim;                             // dcg: positions [0, lim) count; < 0: the real documents, [0, n[b])
    int use_exp, normalize;
    int tiles;                           // tiles per query in this launch
    int ptiles;                          // row stride of the partials: ceil(L / kEpiTile)
    float *part, *part2;                 // (B, ptiles) tile sums (part2: ideal dcg / arp's label sum)
    float *out;
};

// the DCG term of label y at position r (dcg.py:91-93)
__device__ __forceinline__ float dcg_term(float y, int r, int use_exp)
{
    const float gain = use_exp ? (exp2f(y) - 1.0f) : y;
    return gain / log2f((float)r + 2.0f);
}

// ... of sorted position r: a padded document's own label, else the label behind the key (ideal: in the key)
__device__ __forceinline__ float long_dcg_term(const LongMetricParams &p, size_t base, int r, int nb,
                                               unsigned long long seed)
{
    float y;
    if (r >= nb) y = load_label(p.k.rel, p.k.rel_dtype, base + r);
    else if (p.ideal) y = long_key_value(p.sorted[base + r]);
    else y = load_label(p.k.rel, p.k.rel_dtype, base + long_doc(p.k, p.sorted[base + r], seed));
    return dcg_term(y, r, p.use_exp);
}

template <int OP>
__global__ void __launch_bounds__(kEpiThreads) longsort_partial_kernel(LongMetricParams p)
{
    __shared__ float red[32];
    const EpiTile t = epi_tile(p.k, p.tiles);
    const int tid = threadIdx.x;
    const int lim = (OP == METRIC_ARP || p.lim < 0) ? t.nb : min(p.lim, p.k.L);
    float a = 0.f, c = 0.f;
    for (int x = tid; x < kEpiTile; x += kEpiThreads) {
        const int r = t.r0 + x;
        if (r >= lim) break;
        if (OP == METRIC_ARP) {
            const float y = load_label(p.k.rel, p.k.rel_dtype, t.base + long_doc(p.k, p.sorted[t.base + r], t.seed));
            a += (float)(r + 1) * y;                                   // arp.py:31-42
            c += y;
        } else {
            a += long_dcg_term(p, t.base, r, t.nb, t.seed);
        }
    }
    a = block_sum(a, red);
    if (OP == METRIC_ARP) c = block_sum(c, red);
    if (tid == 0) {
        p.part[(size_t)t.q * p.ptiles + t.tile] = a;
        if (OP == METRIC_ARP) p.part2[(size_t)t.q * p.ptiles + t.tile] = c;
    }
}

// metric@k (dcg / ndcg) and arp: the tile sums of a query added in a fixed order.
template <int OP>
__global__ void __launch_bounds__(kEpiThreads) longsort_finish_kernel(LongMetricParams p)
{
    __shared__ float red[32];
    const int q = blockIdx.x, tid = threadIdx.x;
    const bool two = OP == METRIC_ARP || p.normalize;
    float a = 0.f, c = 0.f;
    for (int i = tid; i < p.tiles; i += kEpiThreads) {
        a += p.part[(size_t)q * p.ptiles + i];
        if (two) c += p.part2[(size_t)q * p.ptiles + i];
    }
    a = block_sum(a, red);
    c = block_sum(c, red);
    if (tid == 0) {
        if (two && c == 0.0f) c = 1.0f;                                // arp.py:41, dcg.py:37
        p.out[q] = two ? a / c : a;
    }
}

// The dcg curve (k == 0): each tile scans its terms and adds the sum of the tiles before it
// (longsort_partial_kernel's sums).  DIVIDE: the ideal pass -- out = dcg / (idcg or 1).
template <bool DIVIDE>
__global__ void __launch_bounds__(kEpiThreads) longsort_curve_kernel(LongMetricParams p)
{
    __shared__ float term[kEpiTile];
    __shared__ float red[32];
    const EpiTile t = epi_tile(p.k, p.tiles);
    const int tid = threadIdx.x;
    for (int x = tid; x < kEpiTile; x += kEpiThreads)
        term[x] = x < t.span ? long_dcg_term(p, t.base, t.r0 + x, t.nb, t.seed) : 0.f;
    float off = 0.f;
    for (int i = tid; i < t.tile; i += kEpiThreads) off += p.part[(size_t)t.q * p.ptiles + i];
    off = block_sum(off, red);
    __syncthreads();
    block_inclusive_scan(term, kEpiTile, red, off);                    // (kEpiE positions per thread)
    for (int x = tid; x < t.span; x += kEpiThreads) {
        float *o = p.out + t.base + t.r0 + x;
        if (DIVIDE) {
            float id = term[x];
            if (id == 0.0f) id = 1.0f;                                 // dcg.py:37
            *o = *o / id;
        } else {
            *o = term[x];
        }
    }
}

// ---- host side ----
inline int long_epi_tiles(int L) { return (L + kEpiTile - 1) / kEpiTile; }

struct LongWorkspace {
    unsigned long long *k0, *k1;
    int *inv;
    float *part, *part2;
};

// The workspace of ltr_sort_workspace_bytes (include/ltr_hip.h states the byte formula): the key ping-pong and the
// inverse tie map, each rounded up to 256 bytes -- evaluate() and ListMLE carve theirs on behind these --, then
// (parts) the two (B, tiles) tile sums of dcg / arp.
inline LongWorkspace long_workspace(Carver &c, int B, int L, bool parts)
{
    const size_t BL = (size_t)B * (size_t)L, bt = parts ? (size_t)B * (size_t)long_epi_tiles(L) : 0;
    LongWorkspace r;
    r.k0 = c.take<unsigned long long>(BL);
    r.k1 = c.take<unsigned long long>(BL); c.align256();
    r.inv = c.take<int>((size_t)L); c.align256();
    r.part = c.take<float>(bt);
    r.part2 = c.take<float>(bt);
    return r;
}

// Sorts every query's keys (SRC: long_key's key source).  ranking != null: the ranking is written by the last
// launch and nothing is returned; else the buffer that holds the sorted keys.
template <int SRC = KEY_SCORES>
inline const unsigned long long *long_sort(const LongKeyParams &k, int B, const LongWorkspace &ws, int64_t *ranking,
                                           hipStream_t stream)
{
    const int L = k.L;
    const int chunks = (L + kSortChunk - 1) / kSortChunk;
    if (chunks == 1 && ranking) {
        hipLaunchKernelGGL(longsort_chunk_kernel<true>, dim3((unsigned)B), dim3(kChunkThreads), 0, stream, k, 1,
                           (unsigned long long *)nullptr, ranking);
        return nullptr;
    }
    hipLaunchKernelGGL((longsort_chunk_kernel<false, SRC>), dim3((unsigned)((size_t)B * chunks)), dim3(kChunkThreads), 0,
                       stream, k, chunks, ws.k0, (int64_t *)nullptr);
    unsigned long long *src = ws.k0, *dst = ws.k1;
    const int tiles = (L + kMergeTile - 1) / kMergeTile;
    const dim3 grid((unsigned)((size_t)B * tiles));
    for (int W = kSortChunk; W < L; W *= 2) {
        if (ranking && 2 * (long long)W >= L) {
            hipLaunchKernelGGL(longsort_merge_kernel<true>, grid, dim3(kMergeThreads), 0, stream, k, tiles, W,
                               (const unsigned long long *)src, (unsigned long long *)nullptr, ranking);
            return nullptr;
        }
        hipLaunchKernelGGL(longsort_merge_kernel<false>, grid, dim3(kMergeThreads), 0, stream, k, tiles, W,
                           (const unsigned long long *)src, dst, (int64_t *)nullptr);
        unsigned long long *x = src; src = dst; dst = x;
    }
    return src;
}

inline LongKeyParams long_key_params(const float *scores, const void *rel, int rel_dtype, const int64_t *n,
                                     const int32_t *tie, int use_seed, uint64_t seed, const int64_t *seed_dev, int L,
                                     const LongWorkspace &ws, hipStream_t stream)
{
    LongKeyParams k{};
    k.scores = scores; k.rel = rel; k.rel_dtype = rel_dtype; k.n = n; k.L = L;
    if (use_seed) {
        k.mode = TIE_SEED; k.seed = seed; k.seed_dev = seed_dev;
    } else if (tie) {
        k.mode = TIE_EXPLICIT; k.tie = tie; k.inv_tie = ws.inv;
        hipLaunchKernelGGL(longsort_inverse_tie_kernel, dim3(grid_for((size_t)L, 256)), dim3(256), 0, stream, tie, L, ws.inv);
    }
    return k;
}

// The sort path of the _long_ entry points past kMaxListLen (op = METRIC_*; arguments checked by metric_entry).
int long_metric(int op, const float *scores, const void *rel, int rel_dtype, const int64_t *n, const int32_t *tie,
                int use_seed, uint64_t seed, const int64_t *seed_dev, int B, int L, int k, int use_exp, int normalize,
                void *out, void *workspace, size_t workspace_bytes, hipStream_t s)
{
    Carver carver(workspace);
    const LongWorkspace ws = long_workspace(carver, B, L, op != METRIC_RANK);
    if (!workspace || workspace_bytes < carver.off) return LTR_ERR_WORKSPACE;
    if (op == METRIC_RANK) {
        long_sort(long_key_params(scores, nullptr, LTR_LABEL_F32, n, tie, use_seed, seed, seed_dev, L, ws, s), B, ws,
                  (int64_t *)out, s);
        return (int)hipGetLastError();
    }
    LongMetricParams p{};
    p.k = long_key_params(scores, rel, rel_dtype, n, tie, use_seed, seed, seed_dev, L, ws, s);
    p.ptiles = long_epi_tiles(L);
    p.part = ws.part;
    p.part2 = ws.part2;
    p.out = (float *)out;
    if (op == METRIC_DCG) {
        p.use_exp = use_exp;
        p.normalize = normalize;
        const int kk = k > 0 ? (k < L ? k : L) : 0;
        p.lim = kk > 0 ? kk : L;
        p.tiles = long_epi_tiles(p.lim);
        const dim3 grid((unsigned)((size_t)B * p.tiles)), block(kEpiThreads);
        // the ideal ranking: the same sort keyed on labels (index words; equal labels have equal gains)
        LongMetricParams ip = p;
        ip.k.scores = nullptr; ip.k.mode = TIE_INDEX; ip.k.tie = nullptr; ip.k.seed_dev = nullptr;
        ip.ideal = 1;
        ip.part = ws.part2;
        p.sorted = long_sort(p.k, B, ws, nullptr, s);
        if (kk > 0) {
            hipLaunchKernelGGL(longsort_partial_kernel<METRIC_DCG>, grid, block, 0, s, p);
            if (normalize) {
                ip.sorted = long_sort(ip.k, B, ws, nullptr, s);
                hipLaunchKernelGGL(longsort_partial_kernel<METRIC_DCG>, grid, block, 0, s, ip);
            }
            hipLaunchKernelGGL(longsort_finish_kernel<METRIC_DCG>, dim3((unsigned)B), block, 0, s, p);
        } else {
            hipLaunchKernelGGL(longsort_partial_kernel<METRIC_DCG>, grid, block, 0, s, p);
            hipLaunchKernelGGL(longsort_curve_kernel<false>, grid, block, 0, s, p);
            if (normalize) {
                ip.sorted = long_sort(ip.k, B, ws, nullptr, s);
                hipLaunchKernelGGL(longsort_partial_kernel<METRIC_DCG>, grid, block, 0, s, ip);
                hipLaunchKernelGGL(longsort_curve_kernel<true>, grid, block, 0, s, ip);
            }
        }
        return (int)hipGetLastError();
    }
    p.tiles = p.ptiles;
    p.sorted = long_sort(p.k, B, ws, nullptr, s);
    hipLaunchKernelGGL(longsort_partial_kernel<METRIC_ARP>, dim3((unsigned)((size_t)B * p.tiles)), dim3(kEpiThreads), 0, s, p);
    hipLaunchKernelGGL(longsort_finish_kernel<METRIC_ARP>, dim3((unsigned)B), dim3(kEpiThreads), 0, s, p);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int ltr_max_sort_list_len(void) { return kMaxSortListLen; }

size_t ltr_sort_workspace_bytes(int op, int B, int L)
{
    if (op < METRIC_RANK || op > METRIC_ARP || B < 0 || L <= 0 || L > kMaxSortListLen) return 0;
    Carver sizes(nullptr);
    long_workspace(sizes, B, L, op != METRIC_RANK);
    return sizes.off;
}

uint32_t ltr_tie_hash_word_long(uint64_t seed, uint32_t position) { return tie_hash_word_long(seed, position); }

LTR_DEBUG_HOOK int ltr_debug_long_sort_all(int on)
{
    return __atomic_exchange_n(&g_long_sort_all, on ? 1 : 0, __ATOMIC_RELAXED);
}

// ---- rank_by_score / dcg / arp on long lists (the other forms: ltr_kernels.hip; one body, metric_entry) ----
int ltr_rank_by_score_long_f32(const float *scores, const int64_t *n, const int32_t *tie, int use_seed, uint64_t seed,
                               const int64_t *seed_dev, int B, int L, int64_t *ranking, void *workspace,
                               size_t workspace_bytes, void *stream)
{
    return metric_entry<METRIC_RANK>(scores, nullptr, 0, n, tie, use_seed, seed, seed_dev, B, L, 0, 0, 0, ranking,
                                     kMaxSortListLen, workspace, workspace_bytes, stream);
}

int ltr_dcg_long_f32(const float *scores, const void *rel, int rel_dtype, const int64_t *n, const int32_t *tie,
                     int use_seed, uint64_t seed, const int64_t *seed_dev, int B, int L, int k, int use_exp,
                     int normalize, float *out, void *workspace, size_t workspace_bytes, void *stream)
{
    return metric_entry<METRIC_DCG>(scores, rel, rel_dtype, n, tie, use_seed, seed, seed_dev, B, L, k, use_exp, normalize,
                                    out, kMaxSortListLen, workspace, workspace_bytes, stream);
}

int ltr_arp_long_f32(const float *scores, const void *rel, int rel_dtype, const int64_t *n, const int32_t *tie,
                     int use_seed, uint64_t seed, const int64_t *seed_dev, int B, int L, float *out, void *workspace,
                     size_t workspace_bytes, void *stream)
{
    return metric_entry<METRIC_ARP>(scores, rel, rel_dtype, n, tie, use_seed, seed, seed_dev, B, L, 0, 0, 0, out,
                                    kMaxSortListLen, workspace, workspace_bytes, stream);
}

}  // extern "C"
