// ltr_cluster.inc -- Linear(F,1) scorer fused with the pairwise loss for LONG lists, features read
// ONCE (included by ltr_linear.hip after ltr_linear.inc and ltr_areas.inc).
//
// The general fused kernel (linear_pairwise_kernel) gives a query to one workgroup: its rows do
// not fit the workgroup's registers, so the features are read twice (scores, then dW), and the
// longest query's pair pass sets the duration of the launch.  Here a query is a CLUSTER of up to
// Pmax workgroups on block ids CONGRUENT MOD 8 (round 5: the dispatcher deals block ids round-robin
// over the eight XCDs, so the members of a cluster share one XCD and its L2 -- see "XCD-local
// clusters" below).  Workgroup `part` keeps rows [part*rpw, (part+1)*rpw)
// of the query in registers (the register-tile layout of linear_regtile_kernel) and the cluster
// runs the step in three exchanges through device memory:
//   1. scores of my rows -> sbuf[b, :]                  ; counter 1, wait for the whole cluster
//   1b. (NDCG kinds, round 4) score ranks of my rows + my rows' terms of maxDCG -> rbuf / mxp ; counter 4, wait
//   2. my share of the query's pair units (the split-query decomposition of pairwise_core_sym)
//      -> gradient slice + raw pair sum                ; counter 2, wait
//   3. d loss / d s for MY rows = sum of the slices; dW share from the registers -> pvec
//                                                      ; counter 3, the LAST workgroup of the cluster
//      adds the shares in part order into the (F+1, B) partials of the plain path.
// The waits are spin loops on agent-scope atomics.  They cannot deadlock: every XCD starts its
// workgroups in block-id order and a workgroup only waits for members of its own cluster (which are
// CONSECUTIVE in its XCD's order), so all members of the oldest unfinished cluster of an XCD are
// resident; workgroups with nothing to do (part >= P) leave at once.  A bounded spin count turns a hypothetical stall into a NaN loss instead of a
// hung GPU.  Deterministic: fixed orders everywhere, no float atomics.
// Same results as the plain path to fp32 summation order (tests/test_gpu_fused.py).
#pragma once

namespace {

constexpr int kClThreads = 1024;
constexpr int kClNI = 12;         // row sweeps held in registers (12 float4 per thread)
constexpr int kClNISmall = 8;
constexpr int kClMaxParts = 16;
constexpr int kClSpinLimit = 1 << 20;
constexpr int kClCntStride = 64;              // ints between the counters of two queries (256 B: own cache line / channel)
constexpr int kClCntScope = __HIP_MEMORY_SCOPE_SYSTEM;
constexpr int kClNIWide = 19;          // (swept 12 / 19: 64 x 512 x 700 38 -> 27 us; 116 VGPRs of the 128 a 1024-thread workgroup may use)
constexpr int kClSleep = 8;          // (swept 2 / 8 / 64: 64 costs 2-3 us per launch)

// XCD-local clusters (round 5, verdict r4 item 2).  Block id i runs on XCD (i + k) mod 8 (k: where the
// dispatcher's round-robin stood; profiles/r05_exchange_latency.txt), so a cluster laid out on block ids
// 8 * (ql * Pmax + part) + x  (x = block id mod 8, query position = 8 * ql + x) lives on ONE XCD.  What its
// members hand each other then only has to reach that XCD's L2: PLAIN stores (write-back: the line stays in
// the L2, dword stores merge there instead of being one fabric write each) read by sc1 loads (which
// bypass the reader's L1) -- a round trip of 0.52 us instead of 1.0, and the slices / scores are re-read from
// the L2 instead of the fabric.  Nothing in the ISA promises the placement, so every launch CHECKS it: the
// arrival on the first counter carries the member's HW_REG_XCC_ID (cluster_wait_placed); unless all P
// arrivals of a cluster name one XCD the cluster re-publishes its
// scores write-through behind one more counter and keeps to write-through (sc1) stores for the rest of the
// step -- the round-4 protocol, correct under any placement.
constexpr int kClXcds = 8;
constexpr int kClCntPair = 1, kClCntFinal = 2, kClCntNdcg = 3, kClCntRepub = 4;      // (counter 0: the first wait, with the placement)

struct ClusterParams {
    LinearParams lp;                         // part = the (F+1, B) partials of the plain path
    float *sbuf;                             // (B, L) scores; behind them, at offsets the kernel computes (one base pointer
                                             // in scalar registers instead of six): slices() (B * Pmax, L) gradient slices of
                                             // the parts, wl() (B * Pmax) raw pair sums, pvec() (B * Pmax, pitch) dW | db
                                             // shares, NDCG kinds: rbuf() (B, L) score ranks (as floats) -- the rank exchange,
                                             // round 4 -- and mxp() (B * Pmax) the parts' terms of maxDCG
    __host__ __device__ float *slices() const { return sbuf + (size_t)lp.B * lp.L; }
    __host__ __device__ float *wl() const { return slices() + (size_t)lp.B * Pmax * lp.L; }
    __host__ __device__ float *pvec() const { return wl() + (((size_t)lp.B * Pmax + 3) & ~(size_t)3); }
    __host__ __device__ float *rbuf() const { return pvec() + (size_t)lp.B * Pmax * pitch; }
    __host__ __device__ float *mxp() const { return rbuf() + (size_t)lp.B * lp.L; }
    int *cnt;                                // kClCntStride * B ints (3 counters per query) in the library's exchange area: zero when
                                             // allocated, zero between launches (self-resetting)
    int Pmax, rpw, pitch;
    unsigned scratch_bytes;                  // LDS scratch behind sy (see the kernel)
    int *status;                             // process status word (pinned host page) or null
    int spin_limit;                          // polls before a wait gives up; < 0: give up at once (tests)
    int mode;                                // tests: bit 0 = treat every cluster as spread over several XCDs (the write-through
                                             // protocol), bit 1 = the hinge kinds by the pair pass even on integer grades 0 .. 4
};

// The data the workgroups of a cluster hand each other goes through agent-coherent accesses
// (relaxed agent-scope atomics: loads / stores with sc1, served at the level all XCDs share), so no
// cache-wide fence is needed -- an agent-scope release / acquire writes back / invalidates the
// XCD's whole L2, in a spin loop on every iteration (the first version, with per-thread fences,
// acquire loads in the spin loop and a hipMemsetAsync for the counters, took 1.2 ms at C4).
__device__ __forceinline__ void st_shared(float *ptr, float v)
{
    __hip_atomic_store(ptr, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float ld_shared(const float *ptr)
{
    return __hip_atomic_load(ptr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// local: the cluster was seen on one XCD -- a plain store (kept in that XCD's L2, where the members' sc1 loads find it)
__device__ __forceinline__ void st_member(float *ptr, float v, bool local)
{
    if (local) *ptr = v;
    else st_shared(ptr, v);
}
__device__ __forceinline__ unsigned cluster_xcc_id()
{
    unsigned v;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
    return v & 7u;
}

// sum_{s < count} base[s * stride], in order, with the coherent loads of NF terms in flight (a
// memory-side round trip is 1.3-2 us on this fabric: a cluster of ten members summed four at a time waits for three)
// (eight in the light 8-sweep members -- 32 x 1000 x 220 DCG-hinge 22.2 -> 20.4 us --, four where the tile leaves no
// registers: the 12-sweep members spill with eight, C4 59.5 -> 63.5)
template <int NF = 4>
__device__ __forceinline__ float sum_shared(const float *base, size_t stride, int count)
{
    float acc = 0.f;
    int s = 0;
    for (; s + NF <= count; s += NF) {
        float v[NF];
#pragma unroll
        for (int u = 0; u < NF; ++u) v[u] = ld_shared(base + (size_t)(s + u) * stride);
#pragma unroll
        for (int u = 0; u < NF; ++u) acc += v[u];
    }
    if (s < count) {
        // the tail, still all in flight: clamped addresses, terms past the end dropped
        float v[NF];
#pragma unroll
        for (int u = 0; u < NF; ++u) v[u] = ld_shared(base + (size_t)min(s + u, count - 1) * stride);
#pragma unroll
        for (int u = 0; u < NF; ++u) acc += (s + u < count) ? v[u] : 0.f;
    }
    return acc;
}

__device__ __forceinline__ bool cluster_wait(int *counter, int want, int tid, int spin_limit)
{
    // every wave waits for its own stores to be acknowledged, the barrier collects the waves, then
    // tid 0 signals and spins (relaxed loads); the trailing barrier releases the workgroup
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    __shared__ int s_ok;
    if (tid == 0) {
        __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, kClCntScope);
        int ok = 0;
        for (int it = 0; it < spin_limit; ++it) {
            if (__hip_atomic_load(counter, __ATOMIC_RELAXED, kClCntScope) >= want) { ok = 1; break; }
            __builtin_amdgcn_s_sleep(kClSleep);
        }
        s_ok = ok;
    }
    __syncthreads();
    return s_ok != 0;
}

// The first wait of a step: the arrival also carries the member's XCD number x -- the counter word holds the count
// (bits 0-7), the sum of the x (bits 8-15) and the sum of the x * x (bits 16-31) of its P <= 16 arrivals: all of them
// came from MY XCD exactly when sum = P x and sum of squares = P x * x (zero variance).  `local` = that.
__device__ __forceinline__ unsigned cluster_wait_placed(int *counter, int want, int tid, int spin_limit)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    __shared__ int s_ok0;
    if (tid == 0) {
        const int x = (int)cluster_xcc_id();
        __hip_atomic_fetch_add(counter, 1 | (x << 8) | ((x * x) << 16), __ATOMIC_RELAXED, kClCntScope);
        int ok = 0;
        for (int it = 0; it < spin_limit; ++it) {
            const int v = __hip_atomic_load(counter, __ATOMIC_RELAXED, kClCntScope);
            if ((v & 0xff) >= want) {
                ok = 1 | ((((v >> 8) & 0xff) == want * x && ((unsigned)v >> 16) == (unsigned)(want * x * x)) ? 2 : 0);
                break;
            }
            __builtin_amdgcn_s_sleep(kClSleep);
        }
        s_ok0 = ok;
    }
    __syncthreads();
    return (unsigned)__builtin_amdgcn_readfirstlane(s_ok0);      // bit 0: everybody arrived, bit 1: all on my XCD (wave-uniform)
}

// ---------------------------------------------------------------------------------------------------------------
// The hinge kinds BY SORTED RUNS (round 5).  With integer grades 0 .. 4 (every public LTR collection) the pair pass of
// loss/pairwise_additive.py:107-113 is a counting problem: in a list sorted by score (descending), the lower-graded
// documents j that violate the margin against document i -- fl(1 - fl(s_i - s_j)) >= 0, the pair pass's own fp32
// predicate -- are a PREFIX (the predicate is monotone in s_j), the higher-graded documents k whose margin document i
// violates a SUFFIX.  So   d loss / d s_i = #{k above, active} - #{j below, active}   is a binary search for the
// boundary (with that predicate: the same integers as the pair pass, bit for bit) and a look-up in a table of prefix
// counts per grade threshold; and because the gradients of a query sum to zero,
//        sum over active pairs of (1 - (s_i - s_j)) = #active + sum_i (s_i - c) g_i      for any c
// gives the pair sum without a single pair (c = the middle of the score range: no cancellation against the mean).
// The list need not be sorted as a whole: every member ranks ITS rows among themselves before it publishes its scores
// (rows x rows key compares: 72 x 72 where the pair pass had 72 x 1000 / 2 thirteen-instruction steps) and publishes the
// local ranks WITH the scores -- one exchange -- so that every member holds the query as P sorted runs with a prefix
// table each, and a document's counts are the sums over the runs: rows x P x 2 searches of <= 8 steps.  At n = 1000
// the pair share of a member was 4.7 us mean / 7.2 max of VALU-bound work, then a second wait, P gradient slices of n
// floats written and summed; all of that is gone: every member owns the gradient of its rows outright.
// Queries with a grade outside 0 .. 4 (or float labels) take the pair pass as before.
//
// LDS: in the scratch region (>= 32 * L4 bytes on 512 threads) sorted scores float[L4] | table u64[L4 + 1] | counts
// int[2 rpw], after the exchange; behind gloc my rows' keys u64[rpw] | local ranks int[rpw], before it.
constexpr int kClGrades = 5;
constexpr int kClRunsLightMinL = 1000;       // (see choose_cluster_shape)
constexpr int kRunsMaxNI = 8;
constexpr int kRunsPark = 2;
// bytes of the scratch region the sorted runs use (scores, table, counts); tile vectors are parked behind them
__host__ __device__ inline size_t runs_park_offset(size_t L4, size_t rpw)
{
    return (4 * L4 + 8 * (L4 + 1) + 8 * rpw + 15) & ~(size_t)15;
}

__device__ __forceinline__ unsigned long long grade_below_word(float y)
{
    // one 16-bit counter per threshold g = 1 .. 4: "grade < g"
    return (unsigned long long)(y < 1.0f) | ((unsigned long long)(y < 2.0f) << 16) |
           ((unsigned long long)(y < 3.0f) << 32) | ((unsigned long long)(y < 4.0f) << 48);
}
// documents with grade < g counted in the table word t that covers p positions; g = 0: none, g = 5: all p
__device__ __forceinline__ int grade_below(unsigned long long t, int g, int p)
{
    if (g <= 0) return 0;
    if (g >= kClGrades) return p;
    return (int)((t >> (16 * (g - 1))) & 0xffffull);
}

struct RunsLds { float *ss; unsigned long long *tab; int *cnts; int *myrank; unsigned long long *keys; };
// ss / tab / cnts in the scratch region (after the exchange), keys / myrank behind gloc (they are written while the partial
// dots still occupy the scratch)
__device__ __forceinline__ RunsLds carve_runs(float *scratch, float *gloc, int L4, int rpw)
{
    RunsLds r;
    r.ss = scratch;
    r.tab = reinterpret_cast<unsigned long long *>(scratch + L4);
    r.cnts = reinterpret_cast<int *>(r.tab + L4 + 1);
    r.keys = reinterpret_cast<unsigned long long *>(gloc + rpw + (rpw & 1));
    r.myrank = reinterpret_cast<int *>(r.keys + rpw);
    return r;
}

// Before the exchange: the rank of my row lr among my rows (score descending, index ascending) from u.keys[lr] =
// rank_key(score, lr) (written by the caller, behind a barrier) -> u.myrank[lr] (kept for the write-through protocol) and,
// with the score, straight to the cluster (plain stores: sbuf / rbuf).  Lanes hold candidates, a wave takes every
// (T / 64)-th row: one compare + ballot + s_bcnt1 per 64 pairs, no LDS atomics, no barrier behind it (the wait has one).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned dpp_move_u(unsigned v)
{
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, false);
}
// inclusive prefix sum over the 64 lanes of a wave on the DPP path (row shifts, then the row totals broadcast)
__device__ __forceinline__ unsigned wave_scan_incl(unsigned v)
{
    v += dpp_move_u<0x111, 0xF>(v);      // row_shr:1
    v += dpp_move_u<0x112, 0xF>(v);      // row_shr:2
    v += dpp_move_u<0x114, 0xF>(v);      // row_shr:4
    v += dpp_move_u<0x118, 0xF>(v);      // row_shr:8
    v += dpp_move_u<0x142, 0xA>(v);      // row_bcast15: rows 1 and 3 add the row in front
    v += dpp_move_u<0x143, 0xC>(v);      // row_bcast31: rows 2 and 3 add rows 0 + 1
    return v;
}

template <int T>
__device__ __forceinline__ void cluster_local_ranks(const RunsLds &u, const float *sc, float *sbuf, float *rbuf, int rows, int tid)
{
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (rows <= 128) {
        // the candidates in registers (lane l holds rows l and 64 + l), a row's own key out of them by v_readlane: no LDS
        // round trip per row (the first version's 2.6 us)
        const unsigned long long c0 = (lane < rows) ? u.keys[lane] : ~0ull;
        const unsigned long long c1 = (64 + lane < rows) ? u.keys[64 + lane] : ~0ull;
        // lane k keeps the result of the wave's k-th row (rows wave, wave + T/64, ...): one store per array behind the loop
        // instead of three per row from lane 0, and no LDS read of the score inside it
        int mine = 0;
        int k = 0;
        for (int i = wave; i < rows; i += (T >> 6), ++k) {
            const unsigned long long src = (i < 64) ? c0 : c1;
            const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)src, i & 63);
            const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(src >> 32), i & 63);
            const unsigned long long ki = ((unsigned long long)hi << 32) | lo;
            const int cs = __popcll(__ballot(c0 < ki)) + __popcll(__ballot(c1 < ki));     // (the all-ones filler never counts)
            mine = (lane == k) ? cs : mine;
        }
        const int i = wave + lane * (T >> 6);
        if (i < rows) { u.myrank[i] = mine; rbuf[i] = (float)mine; sbuf[i] = sc[i]; }
    } else {
        for (int i = wave; i < rows; i += (T >> 6)) {
            const unsigned long long ki = u.keys[i];
            int cs = 0;
            for (int cb = 0; cb < rows; cb += 64) {
                const unsigned long long cand = (cb + lane < rows) ? u.keys[cb + lane] : ~0ull;
                cs += __popcll(__ballot(cand < ki));
            }
            if (lane == 0) { u.myrank[i] = cs; rbuf[i] = (float)cs; sbuf[i] = sc[i]; }
        }
    }
}

// After the exchange (every member has published the scores and local ranks of its rows): reads them, leaves
// q.sy[k].x = every score, returns this member's share of the query's raw pair sum (every thread); gloc[lr] = d raw / d s
// of my rows (integers, unscaled).  NS = searches a thread runs side by side.  Contains barriers.
template <int T, int NS>
__device__ __forceinline__ float cluster_hinge_from_runs(const QueryLds &q, const RunsLds &u, const float *scores,
                                                         const float *lrank, int nb, int rpw, int P, int r0, int r1,
                                                         float *gloc, int tid, long long *trace = nullptr)
{
#ifdef LTR_TRACE
#define RUNS_STAMP(i) do { if (trace && tid == 0) trace[i] = (long long)wall_clock64(); } while (0)
#else
#define RUNS_STAMP(i) do { } while (0)
#endif
    const int rows = max(0, r1 - r0);
    const int lane = tid & 63, wave = tid >> 6;
    // the runs: member m's rows sorted by score in slots [m rpw, m rpw + len_m); two documents' loads in flight per thread
    for (int k0 = tid; k0 < nb; k0 += 2 * T) {
        const int k1 = k0 + T;
        const bool two = k1 < nb;
        const float s0 = ld_shared(scores + k0), f0 = ld_shared(lrank + k0);
        const float s1 = ld_shared(scores + (two ? k1 : k0)), f1 = ld_shared(lrank + (two ? k1 : k0));
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            if (e == 1 && !two) break;
            const int k = e ? k1 : k0;
            const float sv = e ? s1 : s0;
            const int m = k / rpw;
            const int len = min(rpw, nb - m * rpw);
            const int pos = m * rpw + min(max((int)(e ? f1 : f0), 0), len - 1);   // (a failed wait leaves garbage: stay inside the run)
            q.sy[k].x = sv;
            u.ss[pos] = sv;
            u.tab[pos] = grade_below_word(q.sy[k].y);
        }
    }
    for (int t2 = tid; t2 < 2 * rows; t2 += T) u.cnts[t2] = 0;
    __syncthreads();
    RUNS_STAMP(4);
    {   // INCLUSIVE prefix sums of the grade words inside every run (tab[slot] = counts among the run's slots <= slot): a
        // wave per run, lanes = slots, the four 16-bit counters as two independent 32-bit words on the DPP path -- no
        // cross-wave stage (the first version scanned the whole list: one more barrier and LDS round trip)
        for (int m = __builtin_amdgcn_readfirstlane(wave); m < P; m += (T >> 6)) {
            const int base = m * rpw;
            const int len = min(rpw, nb - base);
            unsigned long long carry = 0ull;
            for (int cb = 0; cb < len; cb += 64) {
                const bool in = cb + lane < len;
                const unsigned long long w = in ? u.tab[base + cb + lane] : 0ull;
                const unsigned long long incl = carry + ((unsigned long long)wave_scan_incl((unsigned)w) |
                                                         ((unsigned long long)wave_scan_incl((unsigned)(w >> 32)) << 32));
                if (in) u.tab[base + cb + lane] = incl;
                carry = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(incl >> 32), 63) << 32) |
                        (unsigned)__builtin_amdgcn_readlane((int)(unsigned)incl, 63);
            }
        }
    }
    __syncthreads();
    RUNS_STAMP(5);
    // Searches.  A thread keeps ONE of my rows and takes every G-th run, both sides of two runs side by side -- side 0 = my
    // document as the higher-graded one (the active lower-graded documents of a run are a prefix of it), side 1 = as the
    // lower-graded one (the active higher-graded documents are a suffix): either way the boundary is the number of leading
    // slots on which `active == (side == 0)`, a fixed-step search without branches, positions as LDS byte addresses of the
    // slot in front of the candidate (one add, one min and the load per step and search).  The LDS round trips of a lone
    // chain and the index arithmetic of a (row, run, side) decode per search were 2.7 us of the first version; with
    // (row, side) per thread and three runs side by side 2.2 (the longest queries needed two rounds of searches); G = T /
    // rows groups (7 at 72 rows: 504 threads busy) make it one round for every query of up to 14 runs.
    {
        static_assert(NS == 4, "two runs x two sides");
        const int G = max(1, T / max(rows, 1));
        const int top = 1 << (31 - __builtin_clz(max(rpw, 1)));
        const unsigned ss0 = (unsigned)(size_t)(__attribute__((address_space(3))) float *)u.ss;
        for (int e0 = tid; e0 < G * rows; e0 += T) {
            const int g = e0 / max(rows, 1);
            const int lr = e0 - g * rows;
            const float2 v = q.sy[r0 + lr];
            const int y = (int)v.y;
            // (a top / bottom grade has nobody above / below: that side's searches run on empty runs)
            const bool mine0 = y > 0, mine1 = y < kClGrades - 1;
            const int sh0 = 16 * (y - 1), sh1 = 16 * y;                // the table counters of "grade < y" / "grade <= y"
            int sum0 = 0, sum1 = 0;
            for (int m0 = g; m0 < P; m0 += 2 * G) {
                // (an empty or absent run reads the word in front of the array -- LDS of this workgroup -- and takes nothing)
                unsigned cur[4], end[4], beg[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int m = m0 + j * G;
                    const int base = (m < P) ? m * rpw : 0;
                    const int len = (m < P) ? max(0, min(rpw, nb - base)) : 0;
                    beg[j] = ss0 + 4u * (unsigned)base;
                    cur[2 * j] = cur[2 * j + 1] = beg[j];
                    end[2 * j] = beg[j] + (mine0 ? 4u * (unsigned)len : 0u);        // candidates are slots < end
                    end[2 * j + 1] = beg[j] + (mine1 ? 4u * (unsigned)len : 0u);
                }
                for (unsigned step = 4u * (unsigned)top; step >= 4u; step >>= 1) {
                    float o[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        o[j] = *(const __attribute__((address_space(3))) float *)(size_t)(min(cur[j] + step, end[j]) - 4u);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const unsigned cand = cur[j] + step;
                        const float uu = __builtin_fmaf((j & 1) ? 1.0f : -1.0f, v.x - o[j], 1.0f);
                        const int take = (int)(cand <= end[j]) & ((int)(uu >= 0.0f) ^ (j & 1));
                        cur[j] = take ? cand : cur[j];
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    // counters of the run's first pos slots, and of the whole run (the table is indexed like the slots: 8 bytes
                    // per slot where the scores have 4)
                    const unsigned b0 = beg[j >> 1];
                    const unsigned long long tp = (cur[j] > b0) ? u.tab[((cur[j] - ss0) >> 2) - 1] : 0ull;
                    const unsigned long long tl = (end[j] > b0) ? u.tab[((end[j] - ss0) >> 2) - 1] : 0ull;
                    const int sh = (j & 1) ? sh1 : sh0;
                    const int cp_ = (int)((tp >> sh) & 0xffffull), cl_ = (int)((tl >> sh) & 0xffffull);
                    // side 0: lower-graded documents among the leading active slots; side 1: higher-graded documents from the
                    // first active slot on = (len - pos) - #{grade <= y from there on}
                    if (j & 1) sum1 += (int)((end[j] - cur[j]) >> 2) - (cl_ - cp_);
                    else sum0 += cp_;
                }
            }
            if (sum0) atomicAdd(&u.cnts[2 * lr], sum0);
            if (sum1) atomicAdd(&u.cnts[2 * lr + 1], sum1);
        }
    }
    __syncthreads();
    RUNS_STAMP(6);
    // my rows' gradients and my share of the pair sum: #active (counted at the higher-graded side) + sum (s - c) g with c =
    // the median score of the first run (any constant every member agrees on: the gradients sum to zero -- but fl(s - c)
    // must keep the scores' digits: with the query's first score for c, one outlier at 1e5 in that place cost the loss
    // up to 2e-3; half a run of outliers is no outlier); fixed order
    float term = 0.f;
    {
        const float c = (nb > 0) ? u.ss[min(rpw, nb) >> 1] : 0.0f;
        for (int lr = tid; lr < rows; lr += T) {
            const int below = u.cnts[2 * lr], above = u.cnts[2 * lr + 1];
            const float g = (float)(above - below);
            gloc[lr] = g;
            term += (float)below + (q.sy[r0 + lr].x - c) * g;
        }
    }
    const float share = block_sum(term, q.red);
    __syncthreads();                                            // (red and the scratch may be written again)
    return share;
#undef RUNS_STAMP
}

// The counters reset themselves: the last workgroup of a cluster (the one that adds the shares) zeroes the
// cluster's three counters, so a launch finds them as it needs them -- round 2 zeroed them with a launch of their
// own in front of every step (4.7 us).  They live in the exchange area the library owns (ltr_areas.inc:
// exchange_area_get), zeroed when it is allocated and never handed to anybody else: round 3 kept them in the
// caller's workspace behind a magic word, which a recycled allocation could leave intact over dirty counters
// (ADVICE r3).  A launch that gave up leaves them dirty: the host zeroes the area once the status has been cleared.

constexpr int kClMinW512 = 6;          // <= 80 VGPRs: three 512-thread workgroups per CU (logistic C4 shape 99 -> 84 us)
// (LambdaNDCG2 at list lengths near 1000 needs 57 KB of LDS: two workgroups per CU whatever the registers -- its
// kernels may use 128 VGPRs instead of spilling 20 under the 80 of the others: 256 x 1000 x 220 148 -> 125 us; LambdaNDCG1
// is FASTER spilling 12 registers at three workgroups per CU than clean at two: 113 vs 125)
constexpr int kClMinW512N1 = 6;
constexpr int kClMinW512N2 = 4;
template <int KIND, int T, int NI>
__global__ void __launch_bounds__(T, (T == 512 ? (KIND == LTR_NDCG2 ? kClMinW512N2 : (KIND == LTR_NDCG1 ? kClMinW512N1 : kClMinW512)) : 4))
linear_cluster_kernel(ClusterParams cp)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const LinearParams &p = cp.lp;
    const int L = p.L, F = p.F;
    const int tid = threadIdx.x;
    // block id -> (query position, part): the members of a query on block ids congruent mod 8 (one XCD)
    const int xslot = blockIdx.x & (kClXcds - 1);
    const int xidx = blockIdx.x >> 3;
    const int ql = xidx / cp.Pmax;
    const int part = xidx - ql * cp.Pmax;
    // (boustrophedon: the list-length order below hands out the longest queries first -- XCD x takes ranks x, 15 - x,
    // 16 + x, ...: every XCD the same share of long and short queries; straight order cost C4 62.4 -> 59.9 us)
    const int qpos = ql * kClXcds + ((ql & 1) ? kClXcds - 1 - xslot : xslot);
    if (qpos >= p.B) return;                               // (the grid is padded to whole groups of eight queries)
    int b, nb;
    if (p.sched) {
        b = sched_query_sampled(p.n, p.B, L, p.sched, tid, nb, qpos);
    } else {
        b = qpos;
        nb = clamp_n(p.n[b], L);
    }
#ifdef LTR_TRACE
#define CL_STAMP(i) do { if (tid == 0) reinterpret_cast<long long *>(p.scores_out)[(size_t)blockIdx.x * 16 + (i)] = (long long)wall_clock64(); } while (0)
#else
#define CL_STAMP(i) do { } while (0)
#endif
    const int rpw = cp.rpw;
    int P = (nb + rpw - 1) / rpw;
    if (P < 1) P = 1;                                     // an empty query still reports its loss
#ifdef LTR_TRACE
    if (part >= P) {
        if (tid == 0) {
            reinterpret_cast<long long *>(p.scores_out)[(size_t)blockIdx.x * 16 + 0] = (long long)wall_clock64();
            reinterpret_cast<long long *>(p.scores_out)[(size_t)blockIdx.x * 16 + 15] = -1;
        }
        return;
    }
#endif
    if (part >= P) return;
    CL_STAMP(0);
    const int r0 = part * rpw;
    const int r1 = min(nb, r0 + rpw);                     // my rows: [r0, r1)
    const int L4 = (L + 63) & ~63;
    const int C = F >> 2;
    const int CP = C + 1;
    const int R = T / C;                                  // rows per sweep
    const bool active = tid < R * C;
    const int r = tid / C;
    const int c = tid - r * C;
    constexpr int msplit = T >> 6;

    // LDS: sy[L4] | (NDCG2: q4[L4], delta[L4+4]) | scratch = max(gradient slices of the waves, partial dots,
    // dW shares, rank arrays + sort buffer, sorted runs + tables) | red[32] | gloc[rpw] | keys[rpw] (8 bytes) | local ranks[rpw]
    QueryLds q;
    q.sy = reinterpret_cast<float2 *>(smem);
    q.q4 = nullptr;
    q.delta = nullptr;
    size_t off = 8 * (size_t)L4;
    if (KIND == LTR_NDCG2) {                              // (score, label, gain, rank) and the delta table
        q.q4 = reinterpret_cast<float4 *>(smem + off);
        off += 16 * (size_t)L4;
        q.delta = reinterpret_cast<float *>(smem + off);
        off += 4 * ndcg2_delta_floats((size_t)L4);
    }
    q.gpart = reinterpret_cast<float *>(smem + off);
    q.rank_s = reinterpret_cast<int *>(q.gpart);          // the rank arrays and sort buffer live in the scratch
    q.rank_y = q.rank_s + L4;
    q.gbytes = (unsigned)cp.scratch_bytes;
    q.red = reinterpret_cast<float *>(smem + off + cp.scratch_bytes);
    float *pd = q.gpart;                                  // [rpw][C+1] partial dots (before the pair pass)
    float4 *dred = reinterpret_cast<float4 *>(q.gpart);   // [R][C] dW shares (after it)
    float *gloc = q.red + 32;                             // [rpw] d loss / d s of my rows
    const size_t row = (size_t)b * L;

    stage_labels(q.sy, p.rel, p.rel_dtype, row, L, nb, tid, T);
    const float4 w = active ? reinterpret_cast<const float4 *>(p.W)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float bias = p.bias ? p.bias[0] : 0.f;

    // ---- my rows, one burst ----
    // (buffer loads through a descriptor of exactly my rows: anything past them -- and the idle threads -- read 0;
    // one offset register instead of a 64-bit address per sweep)
    float4 x[NI];
    {
        const uintptr_t xaddr = reinterpret_cast<uintptr_t>(p.X + (row + (size_t)r0) * (size_t)F);
        const unsigned xlo = __builtin_amdgcn_readfirstlane((unsigned)xaddr);
        const unsigned xhi = __builtin_amdgcn_readfirstlane((unsigned)(xaddr >> 32));
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
            reinterpret_cast<void *>(((uintptr_t)xhi << 32) | xlo), 0,
            __builtin_amdgcn_readfirstlane(max(0, r1 - r0) * F * 4), 0x00020000);
        const int voff = active ? (r * C + c) * 16 : 0x7ff00000;
        const int sweep = __builtin_amdgcn_readfirstlane(R * C * 16);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const ltr_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, i * sweep, 0);
            x[i] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
        }
    }
    // The hinge kinds on integer grades 0 .. 4: by sorted runs (above) instead of the pair pass.  Every member sees the
    // same labels, so the cluster decides alike without talking (each thread checks the labels it staged itself -- here,
    // behind the tile burst: in front of it the check waited for the labels before the first row was requested; the waves'
    // verdicts meet behind the barrier that follows the dots).
    // (the light 8-sweep members -- their queries have the most members and the longest pair shares -- and the 1024-thread
    // members for wide rows; the 12-sweep tile sits at its register bound: with this path compiled in it spills two tile
    // vectors INSIDE the load burst, C4 59.9 -> 62.0 us -- as the 19-sweep tile did (the C5 shard 29.0 -> 33.2) until the
    // searches kept three registers per search)
    constexpr bool kRuns = (KIND == LTR_HINGE || KIND == LTR_DCG_HINGE) && ((T == 512 && NI <= kRunsMaxNI) || T == 1024);
    if constexpr (kRuns) {
        // (the 1024-thread members for wide rows: only while a member's rows fit the registers of the local ranking -- 64 x 512 x
        // 700, 95 rows: 28.7 -> 28.2 us, 64 x 1000 x 700 45.6 -> 41.2; with 133 rows on the LDS path 64 x 512 x 520 21.4 -> 23.8)
        int fits = (p.rel_dtype != LTR_LABEL_F32 && !(cp.mode & 2) && (T == 512 || rpw <= 128)) ? 1 : 0;
        for (int k = tid; k < nb; k += T) {
            const float y = q.sy[k].y;
            fits &= (y >= 0.0f && y <= (float)(kClGrades - 1)) ? 1 : 0;
        }
        const bool wave_fits = __ballot(fits != 0) == ~0ull;
        if ((tid & 63) == 0) reinterpret_cast<int *>(q.red)[tid >> 6] = wave_fits ? 1 : 0;
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int lr = r + i * R;
        if (active && r0 + lr < r1) pd[(size_t)lr * CP + c] = vdot(x[i], w);
    }
    __syncthreads();
    bool byrank = false;
    if constexpr (kRuns) {
        int all = 1;
        for (int w2 = 0; w2 < (T >> 6); ++w2) all &= reinterpret_cast<const int *>(q.red)[w2];
        byrank = __builtin_amdgcn_readfirstlane(all) != 0;
    }
    const RunsLds runs = carve_runs(q.gpart, gloc, L4, rpw);
    {
        const int h = tid & 3;
        for (int lr = tid >> 2; lr < r1 - r0; lr += T >> 2) {
            const float *pr = pd + (size_t)lr * CP;
            float acc = 0.f;
            for (int cc = h; cc < C; cc += 4) acc += pr[cc];
            acc = quad_sum(acc);
            if (h == 0) {
                const float sc = acc + bias;
                gloc[lr] = sc;                                    // (kept for the write-through protocol)
                // (plain stores: for the members on my XCD -- checked below; by runs the scores go out with the local ranks)
                if (kRuns && byrank) runs.keys[lr] = rank_key(sc, lr);
                else cp.sbuf[row + r0 + lr] = sc;
            }
        }
    }
    CL_STAMP(1);
    if (kRuns && byrank) {
        __syncthreads();
        cluster_local_ranks<T>(runs, gloc, cp.sbuf + row + r0, cp.rbuf() + row + r0, max(0, r1 - r0), tid);
    }
    int *cnt = cp.cnt + (size_t)kClCntStride * b;
    CL_STAMP(2);
    // the step's state in ONE scalar register (the 12-sweep members sit at their 80 VGPRs and 106 SGPRs): bit 0 = no
    // wait gave up so far, bit 1 = the cluster is on one XCD (plain stores)
    unsigned st = cluster_wait_placed(cnt + 0, P, tid, cp.spin_limit);
    if (cp.mode & 1) st &= 1u;
#define local ((st & 2u) != 0)
#define ok ((st & 1u) != 0)
    if (!local) {
        // the cluster is spread over several XCDs (never seen on gfx950; tests force it): the scores again, write-through,
        // behind a counter of their own -- and write-through stores from here on
        for (int lr = tid; lr < r1 - r0; lr += T) {
            st_shared(cp.sbuf + row + r0 + lr, gloc[lr]);
            if (kRuns && byrank) st_shared(cp.rbuf() + row + r0 + lr, (float)runs.myrank[lr]);
        }
        if (!cluster_wait(cnt + kClCntRepub, P, tid, cp.spin_limit)) st &= 2u;
    }
    CL_STAMP(3);

    // ---- every score of the query, then my share of its pair units ----
    if (!(kRuns && byrank)) {
        for (int k = tid; k < nb; k += T) q.sy[k].x = ld_shared(cp.sbuf + row + k);
        __syncthreads();
    }
    if constexpr (KIND == LTR_NDCG1 || KIND == LTR_NDCG2) {
        // Round 4: a member ranks ITS rows only (keyed counting rank against the whole query: rows x n 64-bit
        // compares over the workgroup), hands the score ranks to the cluster through device memory (one more
        // counter) and its rows' terms of maxDCG with them -- until round 3 every member took both rankings of the
        // whole query itself (~12 us per member: the kernel only paid for B <= #CUs / 4).
        ulonglong2 *keys = reinterpret_cast<ulonglong2 *>(q.rank_s + 2 * L4);
        for (int k = tid; k < nb; k += T) {
            const float2 v = q.sy[k];
            keys[k] = make_ulonglong2(rank_key(v.x, k), rank_key(v.y, k));
        }
        const int rows = max(0, r1 - r0);
        for (int lr = tid; lr < rows; lr += T) { q.rank_s[r0 + lr] = 0; q.rank_y[lr] = 0; }
        if (KIND == LTR_NDCG2) fill_ndcg2_delta(q.delta, nb, L4, tid, T);
        __syncthreads();
        {
            int owners = 64;
            while (owners < rows && owners < T) owners *= 2;
            const int ms = T / owners;
            const int sl = __builtin_amdgcn_readfirstlane(tid / owners);
            const int mlen = (nb + ms - 1) / ms;
            const int m0 = __builtin_amdgcn_readfirstlane(min(nb, sl * mlen));
            const int m1 = __builtin_amdgcn_readfirstlane(min(nb, m0 + mlen));
            for (int o = tid & (owners - 1); o < rows; o += owners) {
                const ulonglong2 kk = keys[r0 + o];
                int cs = 0, cy = 0;
#pragma unroll 4
                for (int m = m0; m < m1; ++m) {
                    const ulonglong2 v = keys[m];
                    cs += (v.x < kk.x);
                    cy += (v.y < kk.y);
                }
                atomicAdd(&q.rank_s[r0 + o], cs);
                atomicAdd(&q.rank_y[o], cy);
            }
        }
        __syncthreads();
        float mxl = 0.f;
        for (int lr = tid; lr < rows; lr += T) {
            st_member(cp.rbuf() + row + r0 + lr, (float)q.rank_s[r0 + lr], local);
            mxl = __builtin_fmaf(ndcg_gain(q.sy[r0 + lr].y), inv_discount((float)q.rank_y[lr]), mxl);
        }
        mxl = block_sum(mxl, q.red);                      // (fixed order: deterministic)
        if (tid == 0) st_member(cp.mxp() + (size_t)b * cp.Pmax + part, mxl, local);
        if (!cluster_wait(cnt + kClCntNdcg, P, tid, cp.spin_limit)) st &= 2u;
        float maxdcg = sum_shared(cp.mxp() + (size_t)b * cp.Pmax, 1, P);       // every thread, part order
        if (maxdcg == 0.0f) maxdcg = 1.0f;                // loss/pairwise_lambda.py:227
        const float inv_maxdcg = 1.0f / maxdcg;
        for (int k = tid; k < nb; k += T) {
            const float2 v = q.sy[k];
            const float G = ndcg_gain(v.y) * inv_maxdcg;   // _ndcg_gains, :221-228
            const float rk = (k >= r0 && k < r1) ? (float)q.rank_s[k] : ld_shared(cp.rbuf() + row + k);
            if (KIND == LTR_NDCG1) q.sy[k].y = G * inv_discount(rk);
            else q.q4[k] = make_float4(v.x, v.y, G, rk);
        }
        __syncthreads();                                   // (the rank arrays and keys are dead: gpart may be written)
    }
    const size_t slot = (size_t)b * cp.Pmax + part;
    float runs_share = 0.f;
    if (kRuns && byrank) {
        // The 12-sweep tile sits at the 80 VGPRs of three workgroups per CU: with this path compiled in, the allocator spilled
        // two tile vectors for their WHOLE life -- stored to scratch inside the load burst, behind a wait for them.  The live
        // range is split by hand instead: kPark vectors wait in the part of the LDS scratch the runs leave free.
        constexpr int kPark = (NI > kClNISmall) ? kRunsPark : 0;
        float4 *park = reinterpret_cast<float4 *>(reinterpret_cast<unsigned char *>(q.gpart) + runs_park_offset(L4, rpw));
#pragma unroll
        for (int e = 0; e < kPark; ++e) park[e * T + tid] = x[NI - 1 - e];
        const float share = cluster_hinge_from_runs<T, 4>(q, runs, cp.sbuf + row, cp.rbuf() + row, nb, rpw, P, r0, r1, gloc, tid
#ifdef LTR_TRACE
            , reinterpret_cast<long long *>(p.scores_out) + (size_t)blockIdx.x * 16
#endif
            );
#pragma unroll
        for (int e = 0; e < kPark; ++e) x[NI - 1 - e] = park[e * T + tid];
        // (stored with the dW share below: a store in front of the dW fold's __syncthreads() -- a fence -- makes this wave wait
        // for its acknowledgement and the other waves for this wave)
        runs_share = share;
        if (!ok && tid == 0 && cp.status)
            __hip_atomic_store(cp.status, (int)LTR_ERR_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        CL_STAMP(7);
        CL_STAMP(8);
        // (gloc = the UNSCALED integer gradients of my rows; the DCG modifier's scale needs the whole query's pair sum:
        // the last workgroup of the cluster applies it to the summed shares)
    } else {
    // Every workgroup of the cluster takes pair units (limiting the pair pass to fewer of them, by the
    // rule of the split-query launch, lost 0-20 %).
    if (part < P) {
        float unused = 1.0f;
        const bool intlab = (KIND == LTR_HINGE || KIND == LTR_DCG_HINGE) && p.rel_dtype != LTR_LABEL_F32;
        const float raw = intlab ? pairwise_core_sym<KIND, 0, false, true>(q, nb, L4, p.sigma, unused, part, P, true)
                                 : pairwise_core_sym<KIND>(q, nb, L4, p.sigma, unused, part, P, true);
        float *wg = cp.slices() + slot * L;
        for (int k = tid; k < nb; k += T) {
            float g = 0.f;
#pragma unroll 4
            for (int s = 0; s < msplit; ++s) g += q.gpart[(size_t)s * L4 + k];
            st_member(wg + k, g, local);
        }
        if (tid == 0) st_member(cp.wl() + slot, raw, local);
    }
    CL_STAMP(7);
    if (!cluster_wait(cnt + kClCntPair, P, tid, cp.spin_limit)) st &= 2u;
    CL_STAMP(8);

    // ---- loss of the query; d loss / d s of my rows ----
    float total = sum_shared(cp.wl() + (size_t)b * cp.Pmax, 1, P);     // every thread, same order
    float gscale = 1.0f;
    if (KIND == LTR_DCG_HINGE) {
        const float lg = logf(2.0f + total);
        gscale = 1.0f / ((2.0f + total) * lg * lg);
        total = -1.0f / lg;
    } else if (KIND != LTR_HINGE) {
        gscale = p.sigma / kLn2;
    }
    if (part == 0 && tid == 0) p.loss[b] = ok ? total : __builtin_nanf("");
    if (!ok && tid == 0) {
        // a wait gave up (a partner never became resident): the step is invalid -- say so where
        // the host sees it (sticky status word -> LTR_ERR_TIMEOUT from the next ltr_linear_* call)
        // and poison the query's outputs so that nothing downstream can use them by accident
        // (the counters are dirty now: the host zeroes the exchange area once the status has been cleared)
        if (cp.status) __hip_atomic_store(cp.status, (int)LTR_ERR_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        p.loss[b] = __builtin_nanf("");
    }
    for (int lr = tid; lr < r1 - r0; lr += T) {
        const float g = sum_shared<(NI <= kClNISmall ? 8 : 4)>(cp.slices() + (size_t)b * cp.Pmax * L + r0 + lr, (size_t)L, P);
        gloc[lr] = g * gscale;
    }
    __syncthreads();
    }

    // ---- dW share from the registers; the bias is the feature column of ones ----
    float *bred = reinterpret_cast<float *>(dred + (size_t)R * C);
    if (active) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        float gb = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int lr = r + i * R;
            if (r0 + lr < r1) {
                const float g = gloc[lr];
                vfma(acc, g, x[i]);
                gb += g;
            }
        }
        dred[(size_t)r * C + c] = acc;
        if (c == 0) bred[r] = gb;
    }
    __syncthreads();
    {
        float *pv = cp.pvec() + slot * cp.pitch;
        const float *dr = reinterpret_cast<const float *>(dred);
        if (kRuns && byrank && tid == 0) st_member(cp.wl() + slot, runs_share, local);
        for (int f = tid; f < F; f += T) {
            float s0 = ok ? 0.f : __builtin_nanf("");        // a failed wait poisons the share
            for (int rr = 0; rr < R; ++rr) s0 += dr[(size_t)rr * F + f];
            st_member(pv + f, s0, local);
        }
        if (tid == T - 1) {
            float sb = ok ? 0.f : __builtin_nanf("");
            for (int rr = 0; rr < R; ++rr) sb += bred[rr];
            st_member(pv + F, sb, local);
        }

    }
    CL_STAMP(9);
    // ---- the last workgroup of the cluster adds the shares, in part order ----
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    __shared__ int s_last;
    if (tid == 0)
        s_last = (__hip_atomic_fetch_add(cnt + kClCntFinal, 1, __ATOMIC_RELAXED, kClCntScope) == P - 1) ? 1 : 0;
    __syncthreads();
    if (s_last) {
        float fs = 1.0f;
        if (kRuns && byrank) {
            // by runs: the query's pair sum is complete only now -- its loss, and the DCG modifier's scale on the
            // summed (unscaled) shares
            float total = sum_shared(cp.wl() + (size_t)b * cp.Pmax, 1, P);
            if (KIND == LTR_DCG_HINGE) {
                const float lg = logf(2.0f + total);
                fs = 1.0f / ((2.0f + total) * lg * lg);
                total = -1.0f / lg;
            }
            if (tid == 0) p.loss[b] = ok ? total : __builtin_nanf("");
        }
        float *out = p.part + (size_t)b * partial_pitch(F);     // this query's row of the partials
        for (int f = tid; f < partial_pitch(F); f += T)
            out[f] = (f <= F) ? fs * sum_shared<(NI <= kClNISmall ? 16 : 4)>(cp.pvec() + (size_t)b * cp.Pmax * cp.pitch + f, (size_t)cp.pitch, P) : 0.f;
        // every member of the cluster is past its waits: leave the counters as the next launch needs them
        if (tid < 5) __hip_atomic_store(cnt + tid, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    CL_STAMP(10);
#ifdef LTR_TRACE
    if (tid == 0) reinterpret_cast<long long *>(p.scores_out)[(size_t)blockIdx.x * 16 + 15] = ((long long)b << 32) | (part << 8) | P;
#endif
#undef local
#undef ok
}

struct ClusterShape { int Pmax, rpw, pitch, threads, ni; unsigned lds_scratch; size_t lds; size_t scratch_floats; };

constexpr int kClMinL = 256;

// Shapes the cluster kernel takes: lists the symmetric pair pass covers, rows of whole float4 that fit the
// 1024-thread tile, and a batch that is small enough for the plain path to be out of balance.
// labels: 1 = an integer label dtype (the hinge kinds can run by sorted runs), 0 = float labels, -1 = not known (plan queries)
bool choose_cluster_shape(int kind, int B, int L, int F, ClusterShape &s, int labels = -1)
{
    if (L <= kClMinL || L > kSymMaxLen) return false;
    if (F % 4 != 0 || F / 4 > kClThreads) return false;
    const int C = F / 4;
    // 512-thread workgroups where a sweep of them still covers whole rows well: two fit a CU (the
    // kernel needs ~85 VGPRs) and overlap one's loads with the other's pair pass; wide rows keep 1024
    s.threads = (C <= 128) ? 512 : kClThreads;
    if (C > s.threads) return false;
    const int R = s.threads / C;
    // sweeps in registers: 19 for wide rows (fewer parts); 12 for long lists on mid-size batches, 8
    // otherwise (more, lighter workgroups: 32 x 1000 x 220 logistic 32 -> 28 us, 192 x 600 x 136 45 -> 37;
    // but C4 hinge 64 -> 73 with 8)
    if (s.threads == 1024) s.ni = kClNIWide;
    else s.ni = kClNISmall;
    s.rpw = s.ni * R;
    s.Pmax = (L + s.rpw - 1) / s.rpw;
    // the light workgroups while a query needs at most 6 of them, or on the smallest batches (many
    // workgroups fill the chip); otherwise 12 sweeps: fewer parts, less exchanged per query
    const int light_b = device_cu_count() / 4;
    // Round 5: the hinge kinds on integer labels run the light members by sorted runs, not by the pair pass -- on the longest
    // lists they then beat the 12-sweep members at every batch size (cold sweep of 36 cells, B = 160 .. 384, us, 12 sweeps ->
    // light: 256 x 1000 x 220 59.0 -> 56.0 (C4), 160 x 1000 x 220 41.7 -> 38.4, 256 x 1000 x 136 46.9 -> 38.5, 384 x 1000 x 136
    // 57.8 -> 50.0; at L = 800 / 900 it is a wash, -5 ... +5 %, and the rule stays as it was)
    // (from 160 queries on: 128 x 1000 x 220 31.4 on 12 sweeps, 32.9 light)
    const bool runs_light = (kind == LTR_HINGE || kind == LTR_DCG_HINGE) && labels == 1 && L >= kClRunsLightMinL && B >= 160;
    if (s.ni == kClNISmall && (s.Pmax > kClMaxParts || (s.Pmax > 6 && B > light_b && !runs_light))) {
        s.ni = kClNI;
        s.rpw = s.ni * R;
        s.Pmax = (L + s.rpw - 1) / s.rpw;
    }
    if (s.Pmax < 2 || s.Pmax > kClMaxParts) return false;
    // rows of >= 112 float4 on 512-thread members: four rows per sweep, so long lists become 14-16 members of 48 rows
    // each -- 200 x 768 x 512 hinge / logistic 93.6 / 104.5 us against 63.4 / 77.8 on the parts kernel (200 x 768 x 448:
    // 84.7 / 96.1 against 59.9 / 75.7); fine while the members are few (128 x 600 x 512 39 / 44 against 54 / 50)
    if (s.threads == 512 && C >= 112 && s.Pmax > 13 && 2 * B > device_cu_count()) return false;
    // Measured against the one-workgroup-per-query kernel (us, hinge / logistic; profiles/README.md),
    // 512-thread workgroups:
    //   B x 1000 x 220:  32: 76/135 -> 24/28   128: 83/141 -> 35/51   256: 85/143 -> 64/83   384: 87/146 -> 80/130   512: 102/151 -> 106/168
    //   B x 1000 x 136:  128: 78/138 -> 33/53  256: 80/139 -> 53/76   384: 82/141 -> 66/96
    //   B x 700 x 220:   128: 50/78 -> 30/41   256: 51/79 -> 44/53    384: 54/81 -> 56/70
    //   B x 600 x 136:   192: 42/64 -> 28/37   256: 42/65 -> 35/40    384: 43/66 -> 40/47    512: 55/75 -> 53/64
    //   B x 512 x 220:   128: 33/47 -> 22/29   192: 34/49 -> 27/37    256: 35/49 -> 35/41    384: 40/51 -> 44/54
    //   B x 400 x 136:   192: 26/37 -> 23/28   256: 27/37 -> 32/35    384: 30/39 -> 42/46
    //   B x 300 x 220:   192: 21/26 -> 20/23   256: 22/27 -> 25/26    384: 28/32 -> 34/36
    // 1024-thread workgroups (rows wider than 128 float4):
    //   B x 512 x 700:   32: 50/64 -> 25/28    64: 54/68 -> 27/29    128: 56/71 -> 57/60    256: 66/79 -> 95/101
    //   64 x 1000 x 700: 125/182 -> 52/58
    // The register tiles leave room for ~20 waves per CU (85 VGPRs), so a launch runs in rounds of
    // ~22 us workgroups: it pays while the batch is small and the lists long.
    {
        const int cus = device_cu_count();
        const bool heavy = !(kind == LTR_HINGE || kind == LTR_DCG_HINGE);
        int limit;
        if (s.threads == 512) {
            if (L >= 768) limit = cus + cus / 2;
            else if (L >= 512) limit = heavy ? cus + cus / 2 : cus;
            else limit = heavy ? cus : cus - cus / 4;
        } else {
            limit = heavy ? cus / 2 : cus / 4;
        }
        // NDCG kinds: until round 3 every member repeated the two rankings (~12 us) and the kernel only paid for
        // B <= #CUs / 4; with the rank exchange (a member ranks its rows, round 4) they follow the heavy kinds
        // Measured cold against what the dispatcher took before (general / parts kernel; NDCG1 / NDCG2, us):
        //   32 x 1000 x 220 60.6 / 63.7 (the old cluster kernel) -> 35.9 / 37.2    128 x 1000 x 220 92 / 108 -> 62 / 80
        //   256 x 1000 x 220 164 / 158 -> 113 / 148     384 x 1000 x 220 169 / 162 -> 145 / 192 (!)
        //   128 x 512 x 136 60 / 59 -> 31 / 31    256 x 512 x 136 61 / 60 -> 38 / 38    384 x 512 x 136 64 / 62 -> 52 / 53
        //   128 x 1000 x 136 82 / 122 -> 71 / 70    256 x 1000 x 136 157 / 151 -> 104 / 123    384 x 1000 x 136 156 / 150 -> 125 / 158 (!)
        //   256 x 700 x 136 94 / 91 -> 58 / 59     192 x 700 x 220 79 / 87 -> 55 / 61
        //   wide rows (1024-thread members): 64 x 512 x 700 41 / 42 against 38 / 38 on the parts kernel, 128 x 512 x 700 69 / 72
        //   against 53 / 53 -- the parts kernel keeps them
        // -> LambdaNDCG2 on the longest lists up to one query per CU, wide rows only on the smallest batches.
        if (kind == LTR_NDCG1 || kind == LTR_NDCG2) {
            if (s.threads != 512) limit = cus / 8;
            else if (C > 96) limit = 0;              // (200 x 768 x 512: 147 / 166 against 96 / 120 on the parts kernel)
            else if (kind == LTR_NDCG2 && L >= 768) limit = cus;
        }
        if (B > limit) return false;
    }
    s.pitch = (F + 1 + 3) & ~3;
    const size_t L4 = (size_t)((L + 63) & ~63);
    size_t scratch = 4 * L4 * (size_t)(s.threads / 64);                 // gradient slices of the waves
    const size_t pd = 4 * (size_t)s.rpw * (C + 1);
    const size_t dr = 16 * (size_t)R * C + 4 * (size_t)R;
    if (pd > scratch) scratch = pd;
    if (dr > scratch) scratch = dr;
    const bool ndcg = (kind == LTR_NDCG1 || kind == LTR_NDCG2);
    if (ndcg && scratch < 24 * L4) scratch = 24 * L4;               // rank arrays + packed keys / sort buffer
    if ((kind == LTR_HINGE || kind == LTR_DCG_HINGE) && s.threads == 512) {
        // the sorted runs, and behind them the tile vectors the 12-sweep members park while they search
        const size_t need = runs_park_offset(L4, (size_t)s.rpw) + (s.ni > kClNISmall ? (size_t)kRunsPark * 16 * s.threads : 0);
        if (scratch < need) scratch = need;
    }
    scratch = (scratch + 15) & ~(size_t)15;
    s.lds_scratch = (unsigned)scratch;
    s.lds = 8 * L4 + scratch + 32 * 4 + 4 * (size_t)s.rpw + 16 + 12 * (size_t)s.rpw + 8;      // (+ keys / local ranks of the sorted runs)
    if (kind == LTR_NDCG2) s.lds += 16 * L4 + 4 * ndcg2_delta_floats(L4);
    if (s.lds > kLdsBudget) return false;
    if ((size_t)kClCntStride * 4 * (size_t)B > kExClusterCtrlBytes) return false;
    s.scratch_floats = (size_t)B * L + (size_t)B * s.Pmax * L + (((size_t)B * s.Pmax + 3) & ~(size_t)3) +
                       (size_t)B * s.Pmax * s.pitch + 64 + 4 +
                       (size_t)B * L + (size_t)B * s.Pmax + 4;                      // rank exchange (NDCG kinds, hinge kinds by ranks), maxDCG terms
    return true;
}

template <int KIND>
int launch_cluster_kind(const ClusterParams &cp, const ClusterShape &s, hipStream_t stream)
{
    const dim3 grid((unsigned)(((cp.lp.B + kClXcds - 1) / kClXcds) * kClXcds * cp.Pmax));   // whole groups of eight queries
    if (s.threads == 512 && s.ni == kClNISmall) {
        LTR_ENSURE_LDS((linear_cluster_kernel<KIND, 512, kClNISmall>), s.lds);
        hipLaunchKernelGGL((linear_cluster_kernel<KIND, 512, kClNISmall>), grid, dim3(512), s.lds, stream, cp);
    } else if (s.threads == 512) {
        LTR_ENSURE_LDS((linear_cluster_kernel<KIND, 512, kClNI>), s.lds);
        hipLaunchKernelGGL((linear_cluster_kernel<KIND, 512, kClNI>), grid, dim3(512), s.lds, stream, cp);
    } else {
        LTR_ENSURE_LDS((linear_cluster_kernel<KIND, 1024, kClNIWide>), s.lds);
        hipLaunchKernelGGL((linear_cluster_kernel<KIND, 1024, kClNIWide>), grid, dim3(1024), s.lds, stream, cp);
    }
    return (int)hipGetLastError();
}

inline int &cluster_force_timeout() { static int v = 0; return v; }
inline int &cluster_debug_mode() { static int v = 0; return v; }

int launch_cluster(int kind, const LinearParams &p, const ClusterShape &s, float *scratch, hipStream_t stream)
{
    ClusterParams cp;
    cp.lp = p;
    cp.status = status_device_ptr(stream);
    cp.spin_limit = cluster_force_timeout() ? -1 : kClSpinLimit;
    cp.mode = cluster_debug_mode();
    cp.Pmax = s.Pmax; cp.rpw = s.rpw; cp.pitch = s.pitch; cp.scratch_bytes = s.lds_scratch;
    cp.sbuf = scratch;
    // the counters: in the exchange area of this (device, stream), behind the parts kernel's control block
    unsigned char *gran = nullptr, *misc = nullptr;
    if (const int rc = exchange_area_get(stream, 16, kExCtrlBytes, &gran, &misc)) return rc;
    cp.cnt = reinterpret_cast<int *>(misc + kExPartsCtrlBytes);
    return with_kind(kind, [&](auto K) { return launch_cluster_kind<K>(cp, s, stream); });
}

}  // namespace
