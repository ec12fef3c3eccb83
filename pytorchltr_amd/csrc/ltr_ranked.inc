// ltr_ranked.inc -- the ranked-row core: stage one query, rank it, reduce and scan over the ranks
// (included by ltr_kernels.hip; DESIGN.md 4.4.1).  What metric_kernel (ltr_kernels.hip), eval_kernel (ltr_eval.inc),
// listmle_kernel (ltr_listmle.inc) and the long path's epilogues (ltr_longsort.inc) share: the tie description, the
// LDS layout and ranking of a staged query, three workgroup scans, the ARP and DCG / NDCG terms, the launch shape and
// its one dispatch, and the workspace carver.

// The thread index as the row helpers of this file and of ltr_listmle_row.inc read it: threadIdx.x.  A translation unit
// that inlines them into a long persistent loop may define LTR_ROW_TID_OPAQUE (ltr_mlp.hip does, and says why): the read
// then goes through an empty asm, the same value, which the optimiser cannot hoist out of that loop.
__device__ __forceinline__ unsigned row_tid()
{
    unsigned t = threadIdx.x;
#ifdef LTR_ROW_TID_OPAQUE
    asm volatile("" : "+v"(t));
#endif
    return t;
}

struct MetricParams {
    const float *scores;
    const void *rel;
    const int64_t *n;
    const int32_t *tie;   // (L) tie priorities (a permutation of 0..L-1) or null = index order
    unsigned long long tie_seed;   // use_seed: tie words hashed from (seed, position), see tie_hash_word
    const int64_t *tie_seed_dev;   //   the seed read from device memory instead (a device generator's draw)
    int use_seed;
    void *out;
    int B, L;
    int rel_dtype;
    int k;           // dcg: cutoff (0 = full curve)
    int use_exp;
    int normalize;
    int msplit;
};

// Tie mode of a call: use_seed != 0 hashed words from seed / seed_dev, else tie (null: document index order).
// (The long path's equivalent: long_key_params, ltr_longsort.inc.)
inline void set_tie(MetricParams &p, const int32_t *tie, int use_seed, uint64_t seed, const int64_t *seed_dev)
{
    if (use_seed) { p.use_seed = 1; p.tie_seed = seed; p.tie_seed_dev = seed_dev; }
    else p.tie = tie;
}

__device__ __forceinline__ unsigned long long tie_seed(const MetricParams &p)
{
    return p.use_seed ? (p.tie_seed_dev ? (unsigned long long)p.tie_seed_dev[0] : p.tie_seed) : 0ull;
}

// tie word of document i: hashed from the seed, a caller-drawn priority, or the index
__device__ __forceinline__ int tie_word(const MetricParams &p, unsigned long long seed, int i)
{
    return p.use_seed ? (int)tie_hash_word(seed, (unsigned)i) : (p.tie ? p.tie[i] : i);
}

// ---- the LDS of one staged query ----
// Byte offsets, with L4 = L rounded up to 4:  sy float2[L4] | rank_s int[L4] | rank_y int[L4] | the work region |
// 32 + 64 floats | (sort path) invt int[L4].  The work region is what the ranking needs -- the counting rank's packed
// keys, 16 B per document, or the sort's 8 B x sort_pow2(L) -- and once the ranks are taken it holds, from its start:
// curve float[L4] | icurve float[L4] | red float[32] | scan float[64].
struct RankedRowLayout { size_t ranks, work, red, invt, end; };
__host__ __device__ constexpr RankedRowLayout ranked_row_layout(int L, bool sort)
{
    const size_t L4 = (size_t)((L + 3) & ~3);
    RankedRowLayout o{};
    o.ranks = 8 * L4;
    o.work = o.ranks + 8 * L4;
    o.red = o.work + 8 * L4;
    o.invt = o.work + (sort ? 8 * (size_t)sort_pow2(L) : 16 * L4) + (32 + 64) * 4;
    o.end = o.invt + (sort ? 4 * L4 : 0);
    return o;
}
__host__ __device__ inline size_t metric_lds_bytes(int L) { return ranked_row_layout(L, false).end; }
__host__ __device__ inline size_t metric_lds_bytes_sort(int L) { return ranked_row_layout(L, true).end; }

struct RankedRowLds {
    float2 *sy;               // (score, label) of document k; ListMLE: (label, score), and (M_i, log S_i) as two
                              //   float[L4] over it once it is read
    int *rank_s, *rank_y;     // rank by score / by label (the ideal ranking); ListMLE keeps the ranked scores in rank_y
    float *curve, *icurve;    // DCG / ideal DCG terms by rank (the start of the work region)
    float *red, *scan;        // scratch of block_sum / of the scans
    int *invt;                // sort path: priority -> document of an explicit tie permutation
    unsigned char *free;      // the first byte behind the layout (eval_kernel: its spec)
};
__device__ __forceinline__ RankedRowLds ranked_row_lds(unsigned char *smem, int L, bool sort)
{
    const RankedRowLayout o = ranked_row_layout(L, sort);
    const int L4 = (L + 3) & ~3;
    RankedRowLds r;
    r.sy = reinterpret_cast<float2 *>(smem);
    r.rank_s = reinterpret_cast<int *>(smem + o.ranks);
    r.rank_y = r.rank_s + L4;
    r.curve = reinterpret_cast<float *>(smem + o.work);
    r.icurve = r.curve + L4;
    r.red = reinterpret_cast<float *>(smem + o.red);
    r.scan = r.red + 32;
    r.invt = reinterpret_cast<int *>(smem + o.invt);
    r.free = smem + o.end;
    return r;
}

// The ranking of one staged query (q.sy: the first nb documents): q.rank_s[k] = rank of document k by sy[k].x, and
// with_y: q.rank_y[k] by sy[k].y (the ideal ranking); ranks < nb, ties by the tie words of p.  Both paths work in the
// work region: the sort (DPT <= 0) sorts through it, the counting rank (DPT > 0) keeps its packed keys there.
template <int DPT>
__device__ __forceinline__ void metric_ranks(const MetricParams &p, const RankedRowLds &q, int nb, bool with_y)
{
    const int L = p.L;
    const int tid = row_tid();
    const int T = blockDim.x;
    const int msplit = p.msplit;
    const int owners = T / msplit;
    const int o = tid % owners;
    const int slice = tid / owners;
    const int mlen = (nb + msplit - 1) / msplit;
    const int m0 = __builtin_amdgcn_readfirstlane(slice * mlen);
    const int m1 = __builtin_amdgcn_readfirstlane(min(nb, m0 + mlen));
    const unsigned long long seed = tie_seed(p);
    if (DPT <= 0) {
        // long lists: bitonic sort of (score, index) keys -- and of (label, index) for the ideal ranking -- through the
        // work region; T = min(1024, P), E = P / T registers per thread (DPT = 0, -2, -4 stands for E = 1, 2, 4)
        constexpr int E = DPT == 0 ? 1 : (DPT == -2 ? 2 : 4);
        unsigned long long *xbuf = reinterpret_cast<unsigned long long *>(q.curve);
        int Pq = 64;                                    // smallest power of two >= n of this query
        while (Pq < nb) Pq <<= 1;
        // random tie-break: the low key word is the document's tie priority; q.invt maps priority -> document
        int *invt = nullptr;
        const int low_mask = p.use_seed ? 0xFFF : 0;
        if (p.tie && !p.use_seed) {
            invt = q.invt;
            for (int j = tid; j < L; j += T) invt[p.tie[j]] = j;
            __syncthreads();
        }
        unsigned long long v[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = e * T + tid;
            v[e] = (i < nb) ? rank_key(q.sy[i].x, tie_word(p, seed, i)) : ~0ull;
        }
        sort_ranks<E>(v, Pq, nb, q.rank_s, xbuf, invt, low_mask);
        if (with_y) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int i = e * T + tid;
                v[e] = (i < nb) ? rank_key(q.sy[i].y, tie_word(p, seed, i)) : ~0ull;
            }
            sort_ranks<E>(v, Pq, nb, q.rank_y, xbuf, invt, low_mask);
        }
    } else {
        // counting rank on packed keys (see count_ranks_keyed)
        ulonglong2 *keys = reinterpret_cast<ulonglong2 *>(q.curve);
        for (int k = tid; k < nb; k += T) {
            const float2 v = q.sy[k];
            const int t = tie_word(p, seed, k);
            keys[k] = make_ulonglong2(rank_key(v.x, t), rank_key(v.y, t));
        }
        __syncthreads();
        if (with_y)
            count_ranks_keyed<(DPT > 0 ? DPT : 1), true>(keys, nb, owners, o, m0, m1, msplit > 1, q.rank_s, q.rank_y);
        else
            count_ranks_keyed<(DPT > 0 ? DPT : 1), false>(keys, nb, owners, o, m0, m1, msplit > 1, q.rank_s, q.rank_y);
    }
}

// ---- workgroup scans: thread t owns a contiguous chunk, a wave scan of the chunk totals, one LDS hop across the
// waves, then the chunk is replayed.  All contain barriers: call from uniform code, after buf is written. ----

// Inclusive prefix sum of buf[0..L) in place (LDS), `carry` added in front.  A thread's start is formed as
// woff + incl - s (the DCG curves' rounding: neither block_scan<OpAdd> nor a changed order gives the same bits).
// `scan_scratch`: LDS of >= 16 floats.
__device__ void block_inclusive_scan(float *buf, int L, float *scan_scratch, float carry = 0.f)
{
    const int T = blockDim.x, tid = row_tid();
    const int ch = (L + T - 1) / T;
    const int lo = min(L, tid * ch), hi = min(L, lo + ch);
    float s = 0.f;
    for (int i = lo; i < hi; ++i) s += buf[i];
    // exclusive scan of per-thread sums: wave scan + cross-wave offsets
    float incl = s;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const float up = __shfl_up(incl, off, kWave);
        if ((tid & 63) >= off) incl += up;
    }
    __syncthreads();
    if ((tid & 63) == 63) scan_scratch[tid >> 6] = incl;
    __syncthreads();
    float woff = 0.f;
    for (int i = 0; i < (tid >> 6); ++i) woff += scan_scratch[i];
    // (woff + incl - s is never -0: adding the default carry of +0 changes no bit)
    float run = carry + (woff + incl - s);
    for (int i = lo; i < hi; ++i) { run += buf[i]; buf[i] = run; }
    __syncthreads();
}

// Inclusive scan of buf[0..len) in place under a scalar operator (OpAdd, OpMul of ltr_common.inc); a thread's start
// is the waves before it, in order, combined with the lanes before it.  `scratch`: LDS of >= 16 floats.
template <typename Op>
__device__ void block_scan(float *buf, int len, float *scratch)
{
    const int T = blockDim.x, tid = row_tid();
    const int ch = (len + T - 1) / T;
    const int lo = min(len, tid * ch), hi = min(len, lo + ch);
    float s = Op::id;
    for (int i = lo; i < hi; ++i) s = Op::f(s, buf[i]);
    float incl = s;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const float up = __shfl_up(incl, off, kWave);
        if ((tid & 63) >= off) incl = Op::f(incl, up);
    }
    float excl = __shfl_up(incl, 1, kWave);
    if ((tid & 63) == 0) excl = Op::id;
    __syncthreads();
    if ((tid & 63) == 63) scratch[tid >> 6] = incl;
    __syncthreads();
    float run = Op::id;
    for (int i = 0; i < (tid >> 6); ++i) run = Op::f(run, scratch[i]);
    run = Op::f(run, excl);
    for (int i = lo; i < hi; ++i) {
        run = Op::f(run, buf[i]);
        buf[i] = run;
    }
    __syncthreads();
}

// the value of lane (lane - shift) within the DPP pattern CTRL, or `idle` where there is none
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_from(float idle, float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(idle), __float_as_int(v), CTRL, ROW_MASK, 0xF, false));
}

// Scans of pairs (x, y) under a two-component operator Op: the identity (Op::idx, Op::idy), Op::then(x, y, x2, y2) --
// (x, y) becomes itself followed by (x2, y2) -- and Op::after(x, y, px, py) -- (x, y) becomes (px, py) followed by
// itself.  (An operator whose rounding depends on the argument order states both; ltr_listmle.inc has the two in use.)
// Inclusive wave scan in lane order: row_shr 1, 2, 4, 8 within the rows of 16 lanes, then row_bcast15 / row_bcast31
// carry the rows' totals forward (rows 1, 3 take row 0, 2; rows 2, 3 take rows 0-1).
template <typename Op, int CTRL, int ROW_MASK>
__device__ __forceinline__ void wave_pair_scan_step(float &x, float &y)
{
    const float px = dpp_from<CTRL, ROW_MASK>(Op::idx, x), py = dpp_from<CTRL, ROW_MASK>(Op::idy, y);
    Op::after(x, y, px, py);
}
template <typename Op>
__device__ __forceinline__ void wave_pair_scan(float &x, float &y)
{
    wave_pair_scan_step<Op, 0x111, 0xF>(x, y); wave_pair_scan_step<Op, 0x112, 0xF>(x, y);
    wave_pair_scan_step<Op, 0x114, 0xF>(x, y); wave_pair_scan_step<Op, 0x118, 0xF>(x, y);
    wave_pair_scan_step<Op, 0x142, 0xA>(x, y); wave_pair_scan_step<Op, 0x143, 0xC>(x, y);
}

// Workgroup scan in thread order of one pair per thread: (x, y) becomes the combination of the threads before it
// (exclusive), (tx, ty) the whole workgroup's, the same bits in every thread.  `pair`: LDS of 2 x 16 floats.
template <typename Op>
__device__ __forceinline__ void block_pair_scan(float &x, float &y, float &tx, float &ty, float *pair)
{
    const unsigned t = row_tid();
    const int lane = t & 63, w = t >> 6, nw = blockDim.x >> 6;
    float ix = x, iy = y;
    wave_pair_scan<Op>(ix, iy);
    float ex = __shfl_up(ix, 1, kWave), ey = __shfl_up(iy, 1, kWave);
    if (lane == 0) { ex = Op::idx; ey = Op::idy; }
    __syncthreads();
    if (lane == 63) { pair[2 * w] = ix; pair[2 * w + 1] = iy; }
    __syncthreads();
    float ax = Op::idx, ay = Op::idy;
    for (int i = 0; i < w; ++i) Op::then(ax, ay, pair[2 * i], pair[2 * i + 1]);
    tx = ax; ty = ay;
    for (int i = w; i < nw; ++i) Op::then(tx, ty, pair[2 * i], pair[2 * i + 1]);
    Op::then(ax, ay, ex, ey);
    x = ax; y = ay;
}

// ---- the metric terms of a ranked row (q.sy staged, q.rank_s / q.rank_y taken).  dcg / ndcg / arp and evaluate()
// are equal bit for bit because both call these. ----

// arp.py:31-42: sum((r+1) * rel_r) / sum(rel_r) over ranks r < n; 0 -> 1 guard
__device__ __forceinline__ float ranked_arp(const RankedRowLds &q, int nb)
{
    const int tid = row_tid(), T = blockDim.x;
    float srp = 0.f, nrp = 0.f;
    for (int k = tid; k < nb; k += T) {
        const float y = q.sy[k].y;
        srp += (float)(q.rank_s[k] + 1) * y;
        nrp += y;
    }
    srp = block_sum(srp, q.red);
    nrp = block_sum(nrp, q.red);
    if (nrp == 0.0f) nrp = 1.0f;
    return srp / nrp;
}

// dcg.py:85-94 (padded labels are read and counted), norm: divided by the ideal DCG (dcg.py:36-37).
// kk > 0: returns the metric at kk.  kk == 0: leaves the cumulative curves in q.curve (and, norm, q.icurve).
__device__ __forceinline__ float ranked_dcg(const RankedRowLds &q, int L, int nb, int kk, bool norm, int use_exp)
{
    const int tid = row_tid(), T = blockDim.x;
    float part = 0.f, ipart = 0.f;
    for (int k = tid; k < L; k += T) {
        const float y = q.sy[k].y;
        const float gain = use_exp ? (exp2f(y) - 1.0f) : y;          // dcg.py:91-92
        const int r = k < nb ? q.rank_s[k] : k;
        const float term = gain / log2f((float)r + 2.0f);             // dcg.py:93
        int ry = 0;
        float iterm = 0.f;
        if (norm) {
            ry = k < nb ? q.rank_y[k] : k;                            // ideal ranking, dcg.py:36
            iterm = gain / log2f((float)ry + 2.0f);
        }
        if (kk > 0) {
            part += (r < kk) ? term : 0.f;
            ipart += (norm && ry < kk) ? iterm : 0.f;
        } else {
            q.curve[r] = term;
            if (norm) q.icurve[ry] = iterm;
        }
    }
    if (kk > 0) {
        part = block_sum(part, q.red);
        if (norm) {
            ipart = block_sum(ipart, q.red);
            if (ipart == 0.0f) ipart = 1.0f;                           // dcg.py:37
            part = part / ipart;
        }
        return part;
    }
    __syncthreads();
    block_inclusive_scan(q.curve, L, q.scan);                          // cumsum, dcg.py:94
    if (norm) block_inclusive_scan(q.icurve, L, q.scan);
    return 0.f;
}

#ifndef LTR_RANKED_ROW_ONLY      // (ltr_mlp.hip takes the row above -- layout, ranking, scans -- without the core's launches)
// ---- the launch ----
// The launch shape of the one-workgroup kernels: the DPT instantiation (0, -2, -4: the sort path with 1, 2, 4 keys
// per thread; 1, 2, 4: the counting rank), the workgroup size and the dynamic LDS; sets p.msplit.
struct MetricShape { int dpt; int threads; size_t lds; };
inline MetricShape metric_shape(MetricParams &p)
{
    if (p.L > kSortRankMinLen) {
        const int P = sort_pow2(p.L);
        int T = P < 1024 ? P : 1024;                    // E = P / T <= 4 keys per thread
        // (many rounds of queries per CU: half the threads with two keys each -- narrower workgroups, more queries in flight, see
        // choose_loss_shape.  Round 6, us: ndcg@10 65 536 x 512 1105 -> 854, 65 536 x 300 953 -> 737, 16 384 x 1000 749 -> 552,
        // arp 65 536 x 300 530 -> 384; 1024 x 512: 25.9 / 25.5, 256 x 1000: 21.7 -> 26.7 -- hence from 16 queries per CU on.  Four
        // keys per thread: 65 536 x 512 889, 8192 x 2000 747 -> 804 -- not taken.)
        if (P <= 1024 && P >= 128 && (long)p.B >= 16L * device_cu_count()) T = P / 2;
        p.msplit = 1;
        return {P == T ? 0 : (P == 2 * T ? -2 : -4), T, metric_lds_bytes_sort(p.L)};
    }
    LaunchShape s = choose_shape(p.B, p.L);
    // (many rounds of queries per CU: ONE wave per query, two documents per thread -- what bounds the launch then is the number of
    // queries a CU has in flight, see choose_loss_shape.  Lists of 128, round 6: ndcg@10 65 536 queries 116 -> 99 us, 2^20: 1667 ->
    // 1359, arp 2^20: 1216 -> 804; at 1024 queries the two-wave shape stays, 6.6 against 8.0)
    if (p.L > 64 && p.L <= 128 && (long)p.B >= 64L * device_cu_count()) { s.owners = 64; s.dpt = 2; s.msplit = 1; }
    p.msplit = s.msplit;
    return {s.dpt == 1 || s.dpt == 2 ? s.dpt : 4, s.owners * s.msplit, metric_lds_bytes(p.L)};
}

// One workgroup per query of the B in the shape sh, sh.lds + extra_lds bytes of dynamic LDS.  kernel_of(D) gives the
// kernel's instantiation for the DPT value D (a std::integral_constant), which is launched with the arguments p.
template <typename Params, typename KernelOf>
int launch_ranked(const MetricShape &sh, int B, size_t extra_lds, hipStream_t stream, const Params &p, KernelOf kernel_of)
{
    const dim3 grid((unsigned)B), block((unsigned)sh.threads);
    const size_t lds = sh.lds + extra_lds;
    auto launch = [&](auto D) -> int {
        const auto kernel = kernel_of(D);
        LTR_ENSURE_LDS(*kernel, lds);                   // (one attribute record per instantiation)
        hipLaunchKernelGGL(kernel, grid, block, lds, stream, p);
        return (int)hipGetLastError();
    };
    switch (sh.dpt) {
    case 0: return launch(std::integral_constant<int, 0>{});
    case -2: return launch(std::integral_constant<int, -2>{});
    case -4: return launch(std::integral_constant<int, -4>{});
    case 1: return launch(std::integral_constant<int, 1>{});
    case 2: return launch(std::integral_constant<int, 2>{});
    }
    return launch(std::integral_constant<int, 4>{});
}

#endif  // LTR_RANKED_ROW_ONLY

// ---- workspaces ----
// A bump allocator over a caller's workspace.  A consumer states its workspace once, as a sequence of take / align256
// calls: run over a null base it yields the byte count (`off`), over the real base the pointers as well.
struct Carver {
    unsigned char *base;
    size_t off = 0;
    explicit Carver(void *ws) : base(reinterpret_cast<unsigned char *>(ws)) {}
    template <typename T> T *take(size_t count)
    {
        off += sizeof(T) * count;
        return base ? reinterpret_cast<T *>(base + off - sizeof(T) * count) : nullptr;
    }
    void align256() { off = (off + 255) & ~(size_t)255; }
};
