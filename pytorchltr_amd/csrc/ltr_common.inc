// ltr_common.inc -- device helpers, the two pair passes and the host-side launch helpers shared by
// every translation unit of libltr_hip.so (ltr_kernels.hip, ltr_linear.hip, ltr_mlp.hip, ltr_linear_bf16.hip).  Everything
// here lives in an anonymous namespace: each translation unit gets its own copy, nothing is exported.
// The one piece of process-wide state, the device status page, is owned by ltr_kernels.hip and
// reached through two hidden (non-exported) functions.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <type_traits>

#include "ltr_hip.h"

// defined in ltr_kernels.hip (hidden visibility: internal to the shared library)
extern "C" __attribute__((visibility("hidden"))) int *ltr_internal_status_device_ptr(void *stream);
extern "C" __attribute__((visibility("hidden"))) int ltr_internal_status_peek(void);
// defined in ltr_areas.inc: every exchange area is zeroed before its next use (a launch gave up)
extern "C" __attribute__((visibility("hidden"))) void ltr_internal_exchange_mark_dirty(void);

namespace {

constexpr int kWave = 64;
constexpr int kMaxListLen = 4096;
constexpr int kSymMaxLen = 1024;   // longest list the symmetric pair pass takes in the fused kernels (LDS: one slice per wave)
constexpr int kLossSymMaxLen = 2048;   // ... in the loss-only kernels (round 4: eight waves above 1024 documents; an untruncated
                                       // MSLR-WEB30K batch reaches 1251, where the both-ends pass was 4-7x slower)
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

// ---------------------------------------------------------------------------------
// Device status word.  The only kernels that can fail at run time are the ones whose workgroups
// wait for each other (ltr_cluster.inc): a wait that gives up must not end as a silent NaN.  One
// pinned, device-mapped host page per process holds a sticky status word; a kernel that gives up
// stores LTR_ERR_TIMEOUT there (system-scope store, rare path), and the linear-scorer entry
// points return it -- without any synchronisation: a host read of pinned memory -- on the NEXT
// call; ltr_device_status() reads / clears it explicitly.  Allocated lazily outside stream capture;
// until then (or when the allocation fails) the kernels only poison their outputs with NaN.
// ---------------------------------------------------------------------------------
// Every launcher reports its launch with hipGetLastError(), which returns (and clears) the LAST error
// of the calling thread -- including one an unrelated earlier call left behind.  The entry points
// therefore drop stale state first, so that a non-zero return is about THIS call.
#define LTR_CLEAR_STALE_ERROR() ((void)hipGetLastError())

inline int *status_device_ptr(hipStream_t stream) { return ltr_internal_status_device_ptr((void *)stream); }
inline int status_peek() { return ltr_internal_status_peek(); }

// ---------------------------------------------------------------------------------
// small device helpers
// ---------------------------------------------------------------------------------
__device__ __forceinline__ float load_label(const void *rel, int dtype, size_t idx)
{
    // wave-uniform switch; int64 -> fp32 narrowing happens in registers (no cast kernel)
    if (dtype == LTR_LABEL_I64) return (float)((const int64_t *)rel)[idx];
    if (dtype == LTR_LABEL_F32) return ((const float *)rel)[idx];
    return (float)((const int32_t *)rel)[idx];
}

// Stage one query's (score, label) pairs into LDS.  The label-dtype switch is hoisted out of
// the loop (wave-uniform), int64 -> fp32 narrowing happens in registers (no cast kernel).
template <typename LabelT>
__device__ __forceinline__ void stage_rows_t(float2 *sy, const float *__restrict__ srow,
                                             const LabelT *__restrict__ yrow, int L, int nb,
                                             int tid, int T)
{
    for (int m = tid; m < L; m += T) {
        const float sv = srow[m];
        const float yv = (float)yrow[m];
        if (m < nb) sy[m] = make_float2(sv, yv);
    }
}

__device__ __forceinline__ void stage_rows(float2 *sy, const float *srow, const void *rel,
                                           int dtype, size_t row, int L, int nb, int tid, int T)
{
    if (dtype == LTR_LABEL_I64)
        stage_rows_t(sy, srow, (const int64_t *)rel + row, L, nb, tid, T);
    else if (dtype == LTR_LABEL_F32)
        stage_rows_t(sy, srow, (const float *)rel + row, L, nb, tid, T);
    else
        stage_rows_t(sy, srow, (const int32_t *)rel + row, L, nb, tid, T);
}

// Labels only (the fused scorer kernels compute the scores themselves).
template <typename LabelT>
__device__ __forceinline__ void stage_labels_t(float2 *sy, const LabelT *__restrict__ yrow, int L,
                                               int nb, int tid, int T)
{
    for (int m = tid; m < L; m += T) {
        const float yv = (float)yrow[m];
        if (m < nb) sy[m].y = yv;
    }
}

__device__ __forceinline__ void stage_labels(float2 *sy, const void *rel, int dtype, size_t row,
                                             int L, int nb, int tid, int T)
{
    if (dtype == LTR_LABEL_I64) stage_labels_t(sy, (const int64_t *)rel + row, L, nb, tid, T);
    else if (dtype == LTR_LABEL_F32) stage_labels_t(sy, (const float *)rel + row, L, nb, tid, T);
    else stage_labels_t(sy, (const int32_t *)rel + row, L, nb, tid, T);
}

__device__ __forceinline__ int clamp_n(int64_t n, int L)
{
    return n < 0 ? 0 : (n > (int64_t)L ? L : (int)n);
}

// Which query a workgroup takes (one workgroup per query: the fused scorer+loss kernels and the
// loss kernel).  The hardware starts block ids in
// order, round-robin over the 8 XCDs and, inside an XCD, over its 32 CUs (a CU hosts ids i, i+256,
// i+512, ...), and a launch of a few workgroups per CU lasts as long as its most loaded CU / its
// last workgroup.  Measured at C2/C3 shapes (n ~ U[1,128], B = 1024; profiles/README.md): batch in
// random order 13.5-14.0 us (hinge) / 23.7 (LambdaNDCG2) / 18.2 (logistic); the same batch sorted
// by n descending 12.2 / 20.0 / 15.3 -- long lists first, and every CU gets one list of each
// quartile.  A full sort of n[] inside every workgroup costs more than that (tried: counting
// sort, 8 000-15 000 cycles), so the order is approximated with 64-query samples: the batch is cut
// into G = ceil(B/64) interleaved groups (group g = chunks of 8 consecutive ids, G chunks apart),
// each group is ranked by n descending, and block id `pos` -- member number m of its group -- takes
// the group's m-th longest list.  Early ids get every group's longest lists, late ids the shortest:
// 12.1 / 20.3 / 15.5 us with the permutation applied on the host.  ONE wave finds the query
// without LDS traffic: one n per lane (8 x 64-byte segments), a radix select over the bits of n
// with ballots (uniform control flow, ~100 instructions), ties by lane order.  A bijection inside
// each group and a pure function of n[]; every output is indexed by the query, so results do not
// depend on it.  (Which member rank a block id takes: sched_slot -- and, for the register tile on
// grids of whole rounds of the CUs, sched_slot_cu, which deals by the CU that hosts the id.)
constexpr int kSchedMaxPerCu = 4;        // register-tile kernel (B = 8 x #CUs: 22.1 -> 23.9 us with it)
constexpr int kLossSchedMaxPerCu = 16;   // loss kernel, general fused kernel
// (2 for the register tile, behind sched_slot_cu: the model's most loaded CU drops by 2-8 rows more, the lazy step does not
// follow -- C2 12.04-12.13 -> 12.16-12.17 us, C3 and 768 queries equal; EXPERIMENTS.md)
constexpr int kSchedLowBits = 3;         // low bits of n the selection ignores

// Block id -> place in the list-length order: the sample group and the member rank (0 = the group's longest list) block `id` of a
// grid of `nred` leading workgroups without a query + B query workgroups takes.  Host and device: the ONE copy of the arithmetic
// (the CPU tier enumerates it through ltr_debug_sched_slots).  A bijection of the ids nred .. nred + B - 1 onto the
// (group, rank < the group's size) pairs for every B, G = ceil(B / 64), cus >= 0 and nred >= 0.
struct SchedSlot { int group, rank; };
// (nred > 0, a lazy launch: block id i sits on CU slot i mod cus and the reducers -- ids below nred, fewer than the CUs -- leave
// theirs first, so the query workgroups with i mod cus < nred share a CU with a reducer at work or take its place: the QUIET ones)
// id = t * cus + r for id < 8 cus, by three compares: a grid is a few rounds of `cus` workgroups, and an integer division is some
// forty scalar instructions and a reciprocal's latency in front of the tile burst of every workgroup (a subtraction LOOP is
// turned back into that division by the compiler)
__host__ __device__ inline int sched_round(int id, int cus, int &r)
{
    int t = 0;
    r = id;
    if (r >= 4 * cus) { r -= 4 * cus; t += 4; }
    if (r >= 2 * cus) { r -= 2 * cus; t += 2; }
    if (r >= cus) { r -= cus; t += 1; }
    return t;
}
__host__ __device__ inline bool sched_quiet(int id, int cus, int nred)
{
    if (nred <= 0 || nred >= cus || id < cus) return false;
    int r;
    sched_round(id, cus, r);
    return r < nred;
}
__host__ __device__ inline SchedSlot sched_slot(int id, int B, int G, int cus, int nred)
{
    int pos = id - nred;
    // (the quiet workgroups take the last places of the order -- the batch's shortest lists --, everybody else the places in front
    // of them, both in id order)
    if (nred > 0 && nred < cus) {
        int r, re;
        const int t = sched_round(id, cus, r);
        const int below = t > 0 ? (t - 1) * nred + (r < nred ? r : nred) : 0;      // quiet ids below `id`
        if (t > 0 && r < nred) {
            const int te = sched_round(nred + B, cus, re);
            const int Q = te > 0 ? (te - 1) * nred + (re < nred ? re : nred) : 0;  // quiet ids in the grid
            pos = B - Q + below;
        } else {
            pos -= below;
        }
    }
    const int u = pos >> 3;
    int jp = u / G;
    SchedSlot s;
    s.group = u - jp * G;
    // (cus > 0: snake over the rounds of one workgroup per CU.  8 G block ids take one eighth of every group -- `jp`,
    // the jp-th longest eighth --, a round of `cus` CUs is `per` of those steps, and a CU hosts ids i, i + #CUs, ...:
    // dealt straight, the CUs of the first half of every round get the longer half of EVERY round's lists (B = 1024,
    // n ~ U[1,128]: 288 rows against 224 per CU); with the odd rounds dealt backwards every CU's queries sum to the same bytes)
    if (cus > 0) {
        const int per = cus / (8 * G);                           // steps per round (256 CUs, G = 16: 2)
        if (per >= 2) {
            const int rd = jp / per, base = rd * per;
            const int back = (rd ^ (rd >> 1)) & 1;               // straight, back, back, straight: the last round ends on the shortest lists
            // (only a round in which EVERY group is complete: dealt backwards, an incomplete one sends blocks to member ranks its
            // short groups do not have -- B = 385 .. 447 and 449 .. 511 on 256 CUs took a query index no lane had written)
            if (back && (base + per) * 8 * G <= B) jp = base + (per - 1 - (jp - base));
        }
    }
    s.rank = jp * 8 + (pos & 7);
    return s;
}

// The register tile's dealing where the grid is WHOLE rounds of the CUs: a launch lasts as long as its most loaded CU, and what
// sched_slot hands a CU is uneven by its arithmetic, not by the sampling.  (a) rank = jp * 8 + (pos & 7) and the block ids of a
// CU share pos & 7: a CU gets the longest list of each eighth T times over, another the shortest T times (plain launch, the
// five batches of bench.py, 256 CUs: rows per CU max / mean 1.20-1.27, one whole XCD +10.6 %).  (b) under the quiet rule
// the non-quiet CUs host every (cus - nred)-th place, and the snake flips rounds of `cus`: C2's lazy launch, 220 non-quiet
// CUs, max / mean 1.29-1.38 (383-398 rows against a mean of 285-299).
// Here the ORDER INDEX o in [0, B) means (group, rank) = (o % G, o / G) -- every group complete, B % 64 == 0 --: index 0 is about
// the longest list and consecutive indices walk the groups at one rank.  Block id i sits on CU slot i % cus in round i / cus
// (scripts/cu_bytes.py --lazy confirms it on the GPU), so with `lead` workgroups without a query in front of the grid
// (the lazy launch's reducers, fewer than the CUs) every slot hosts exactly T = B / cus query workgroups:
//   quiet rule off: slot r's query workgroups are, in id order, its rounds t = 0 .. T - 1; NQ = cus slots, c = r;
//   quiet rule on:  the slots r >= lead are the NQ = cus - lead non-quiet ones, c = r - lead, t = i / cus; the quiet workgroups
//                   (r < lead, i >= cus) take the last B - T NQ order indices in id order -- the shortest lists, as in sched_slot.
// Slot c deals itself o = t NQ + p_t(c) with permutations p_t of [0, NQ) whose sum over t does not depend on c:
//   T = 4: straight, back, back, straight; T = 2: straight, back -- p(c) = c or NQ - 1 - c, the sum is exact;
//   T = 3: straight, then the two halves of the slots by parity -- c = 2 h + e, H = ceil(NQ / 2):
//          p_1 = e ? NQ - H - 1 - h : NQ - 1 - h,  p_2 = e ? NQ - 1 - h : H - 1 - h: the sum is exact for odd NQ and one place
//          apart between even and odd slots otherwise (straight-back-back and straight-back-straight leave NQ - 1 places).
// Lists linear in rank, n = 2 (64 - rank), 256 CUs: every CU 260 rows at T = 4 (sched_slot: 232-288), 130 at T = 2, 194-196 at
// T = 3; 36 reducers and the quiet rule: 294-298 over the 220 non-quiet CUs (sched_slot: 232-384).  bench.py's batches, rows
// per CU max / mean: plain 1.125-1.186, the quiet lazy launch's non-quiet CUs 1.087-1.123 (tests/test_sched_balance.py).
// id -> (t, r) by sched_round's compares and ONE division, o / G, as in sched_slot.
__host__ __device__ inline bool sched_cu_deal_applies(int B, int cus, int lead, bool quiet)
{
    if (cus <= 0 || (B & 63) != 0 || lead < 0 || lead >= cus || (quiet && lead == 0)) return false;
    return B == 2 * cus || B == 3 * cus || B == 4 * cus;
}
__host__ __device__ inline SchedSlot sched_slot_cu(int id, int B, int G, int cus, int lead, bool quiet)
{
    int r;
    int t = sched_round(id, cus, r);                             // (id < lead + B < 5 cus)
    const bool three = B == 3 * cus;
    const int T = three ? 3 : (B == 2 * cus ? 2 : 4);
    int NQ = cus, c = r, o;
    if (quiet) { NQ -= lead; c -= lead; }
    else if (r < lead) t -= 1;                                   // (a reducer had this slot's round 0)
    if (c < 0) {
        o = T * NQ + (t - 1) * lead + r;                         // quiet: the tail of the order, in id order
    } else {
        int p = c;
        if (three) {
            const int H = (NQ + 1) >> 1, h = c >> 1, e = c & 1;
            if (t == 1) p = (e ? NQ - H : NQ) - 1 - h;
            else if (t == 2) p = (e ? NQ : H) - 1 - h;
        } else if ((t ^ (t >> 1)) & 1) {
            p = NQ - 1 - c;
        }
        o = t * NQ + p;
    }
    SchedSlot s;
    s.rank = o / G;
    s.group = o - s.rank * G;
    return s;
}

// `pos`: the workgroup's place among the query workgroups -- or, for the register tile (round_cus > 0), its block id in a grid
// with `lead` workgroups without a query in front (`quiet`: the quiet rule is on, sched_quiet)
__device__ __forceinline__ int sched_query_sampled(const int64_t *__restrict__ n, int B, int L, int G, int tid,
                                                   int &nb_out, int pos, int round_cus = 0, int lead = 0, bool quiet = false)
{
    __shared__ int s_sel[2];
    if (tid < 64) {
        const int lane = tid;
        const SchedSlot slot = sched_cu_deal_applies(B, round_cus, lead, quiet) ? sched_slot_cu(pos, B, G, round_cus, lead, quiet)
                             : sched_slot(quiet ? pos : pos - lead, B, G, round_cus, quiet ? lead : 0);
        const int gam = slot.group;
        int rho = slot.rank;                                     // this block's member number
        const int id = ((lane >> 3) * G + gam) * 8 + (lane & 7); // member `lane` of the group
        unsigned long long cand = __ballot(id < B);              // a prefix of the lanes (ids grow with lane)
        const int key = clamp_n(n[min(id, B - 1)], L);
        // (all lists equally long, e.g. full lists: cand stays the whole group and rho the lane)
        const bool flat = __ballot(key != __builtin_amdgcn_readfirstlane(key)) == 0ull;
        // (the kSchedLowBits low bits of n are ignored: an approximate order balances as well and
        // every bit is one more dependent ballot round in front of the first load)
        for (int bt = flat ? -1 : 31 - __builtin_clz(L); bt >= kSchedLowBits; --bt) {   // descending n: set bits first
            const unsigned long long m = __ballot(((key >> bt) & 1) != 0) & cand;
            const int c = __popcll(m);
            if (rho < c) cand = m;
            else { rho -= c; cand &= ~m; }
        }
        // cand = the lanes holding the selected n; the rho-th of them in lane order takes the block
        const int below = __popcll(cand & ((1ull << lane) - 1ull));
        if ((((cand >> lane) & 1ull) != 0ull) && below == rho) { s_sel[0] = id; s_sel[1] = key; }
    }
    __syncthreads();
    nb_out = __builtin_amdgcn_readfirstlane(s_sel[1]);           // saves the dependent n[b] load
    return __builtin_amdgcn_readfirstlane(s_sel[0]);
}

// Cross-lane adds on the DPP path (no LDS round trip; HIP's __shfl_* lower to ds_bpermute).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_move(float v)
{
    // lanes outside ROW_MASK (or without a valid source) receive 0
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xF, false));
}

// Sum over the 4 lanes of a quad; every lane of the quad gets the result.
__device__ __forceinline__ float quad_sum(float v)
{
    v += dpp_move<0xB1, 0xF>(v);      // quad_perm [1,0,3,2]
    v += dpp_move<0x4E, 0xF>(v);      // quad_perm [2,3,0,1]
    return v;
}

// Sum over the 64 lanes of the wave; every lane gets the result (DPP row ops + one readlane).
__device__ __forceinline__ float wave_sum(float v)
{
    v = quad_sum(v);
    v += dpp_move<0x141, 0xF>(v);     // row_half_mirror: 8-lane sums
    v += dpp_move<0x140, 0xF>(v);     // row_mirror: every lane holds its 16-lane row sum
    v += dpp_move<0x142, 0xA>(v);     // row_bcast15 -> rows 1 and 3 add the previous row
    v += dpp_move<0x143, 0xC>(v);     // row_bcast31 -> rows 2 and 3 add rows 0+1: lane 63 = total
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// Sum over the whole workgroup; every thread gets the result.  Deterministic order.
// `red` is an LDS scratch of >= 16 floats.  Contains barriers: call from uniform code.
// Workgroup barrier that orders LDS traffic only.  __syncthreads() carries a workgroup-scope fence: the compiler puts an
// s_waitcnt in front of it for every store, atomic and LDS-DMA of the wave that is still in flight (loads into registers may
// stay out) -- a wave that has just stored something, or drawn a ticket, waits for the acknowledgement (0.5-2 us under a
// streaming load) and the other waves wait for that wave.  Use where the data handed over lives in LDS only.
__device__ __forceinline__ void lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

__device__ __forceinline__ float block_sum(float v, float *red)
{
    v = wave_sum(v);
    const int nw = blockDim.x >> 6;
    if (nw == 1) return v;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
    for (int i = 0; i < nw; ++i) t += red[i];
    return t;
}

// Scalar operators of the workgroup reductions and scans below and in ltr_ranked.inc: the identity and the combination.
struct OpAdd { static constexpr float id = 0.f; static __device__ __forceinline__ float f(float a, float b) { return a + b; } };
struct OpMul { static constexpr float id = 1.f; static __device__ __forceinline__ float f(float a, float b) { return a * b; } };
struct OpMin { static constexpr float id = 3.0e38f; static __device__ __forceinline__ float f(float a, float b) { return fminf(a, b); } };

// block_sum for another operator (OpMul, OpMin): a butterfly within the wave, then the waves in order; every thread
// gets the result.  `red`: LDS of >= 16 floats.  Contains barriers: call from uniform code.
template <typename Op>
__device__ __forceinline__ float block_reduce(float v, float *red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = Op::f(v, __shfl_xor(v, o, kWave));
    const int nw = blockDim.x >> 6;
    if (nw == 1) return v;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = red[0];
    for (int i = 1; i < nw; ++i) t = Op::f(t, red[i]);
    return t;
}

// Two sums in one pass (same barriers): used for (loss, sum of gradients).
__device__ __forceinline__ void block_sum2(float &a, float &b, float *red)
{
    a = wave_sum(a);
    b = wave_sum(b);
    const int nw = blockDim.x >> 6;
    if (nw == 1) return;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { red[2 * (threadIdx.x >> 6)] = a; red[2 * (threadIdx.x >> 6) + 1] = b; }
    __syncthreads();
    float ta = 0.f, tb = 0.f;
    for (int i = 0; i < nw; ++i) { ta += red[2 * i]; tb += red[2 * i + 1]; }
    a = ta;
    b = tb;
}

// log2(1 + e) for e in [0, 1]; two-term series below 2^-10 where 1+e would round e away.
__device__ __forceinline__ float log2_1p(float e)
{
    const float direct = __builtin_amdgcn_logf(1.0f + e);      // v_log_f32 == log2
    const float series = e * (1.0f - 0.5f * e) * kLog2e;
    return e < 0.0009765625f ? series : direct;
}

// log2(1 + e) with u = 1 + e (rounded) and r = 1 / u at hand: log2(u) + (e - (u - 1)) * r * log2(e) puts
// the rounding of the sum back (both differences are exact), so it holds for every e >= 0 without a
// series branch.
__device__ __forceinline__ float log2_1p_comp(float e, float u, float r)
{
    return __builtin_fmaf((e - (u - 1.0f)) * r, kLog2e, __builtin_amdgcn_logf(u));
}

// ---------------------------------------------------------------------------------
// counting rank: for every owned document k < nb,
//   rank_s[k] = #{m < nb : s_m > s_k or (s_m == s_k and m < k)}     (score, descending)
//   rank_y[k] = the same on labels (only if WITH_Y)
// This is rank_by_score (utils/tensor_operations.py:48-64) restricted to the real
// documents; padded documents rank at their own index (key -inf, index tie-break).
// rank arrays must be zeroed by the caller when msplit > 1 (partial counts are added).
// ---------------------------------------------------------------------------------
template <int DPT, bool WITH_Y>
__device__ __forceinline__ void count_ranks(const float2 *sy, int nb, int owners, int o,
                                            int m0, int m1, bool partial, int *rank_s,
                                            int *rank_y)
{
    for (int base = 0; base < nb; base += owners * DPT) {
        const int wave_first = base + (o & ~63);
        if (wave_first >= nb) continue;                       // wave-uniform
        float sk[DPT], yk[DPT];
        int cs[DPT], cy[DPT], kk[DPT];
#pragma unroll
        for (int c = 0; c < DPT; ++c) {
            kk[c] = base + o + c * owners;
            const bool valid = kk[c] < nb;
            const float2 v = valid ? sy[kk[c]] : make_float2(0.f, 0.f);
            sk[c] = v.x; yk[c] = v.y; cs[c] = 0; cy[c] = 0;
        }
#pragma unroll 4
        for (int m = m0; m < m1; ++m) {
            const float2 v = sy[m];
#pragma unroll
            for (int c = 0; c < DPT; ++c) {
                const bool before = m < kk[c];
                cs[c] += (v.x > sk[c]) | ((v.x == sk[c]) & before);
                if (WITH_Y) cy[c] += (v.y > yk[c]) | ((v.y == yk[c]) & before);
            }
        }
#pragma unroll
        for (int c = 0; c < DPT; ++c) {
            if (kk[c] < nb) {
                if (partial) {
                    atomicAdd(&rank_s[kk[c]], cs[c]);
                    if (WITH_Y) atomicAdd(&rank_y[kk[c]], cy[c]);
                } else {
                    rank_s[kk[c]] = cs[c];
                    if (WITH_Y) rank_y[kk[c]] = cy[c];
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------
// pair terms.  Conventions: owner document k (registers), streamed document m (LDS).
//   c1 = sigma * log2(e)   so that exp(-sigma*d) = exp2(-c1*d)
// Gradient accumulators are in units of sigma/ln2 (applied once per document at the end).
// ---------------------------------------------------------------------------------

// Hinge (loss/pairwise_additive.py:107-113): term(i,j) = max(0, 1-(s_i-s_j)) if y_i > y_j.
// The reference zeroes `loss < 0` (strict), so at exactly the margin the gradient flows.
__device__ __forceinline__ void pair_hinge(float sk, float yk, float sm, float ym, float &g,
                                           float &l)
{
    const float d = sk - sm;
    const bool gt = yk > ym, lt = yk < ym;
    const float u = gt ? (1.0f - d) : (1.0f + d);
    const bool act = (gt | lt) & (u >= 0.0f);
    l += (gt & act) ? u : 0.0f;
    g += act ? (gt ? -1.0f : 1.0f) : 0.0f;
}

// Logistic / ARP2 / NDCG2: term(i,j) = W_ij * log2(1 + exp(-sigma (s_i - s_j))) if y_i > y_j
// (loss/pairwise_additive.py:158-163, loss/pairwise_lambda.py:135-140, :198-218), W symmetric.
// Stable for any finite input (the reference overflows beyond |sigma d| ~ 88).
__device__ __forceinline__ void pair_oriented(float sk, float yk, float sm, float ym, float W,
                                              float c1, float &g, float &l)
{
    const bool gt = yk > ym, lt = yk < ym;
    const float t = (sk - sm) * c1;
    const float z = gt ? t : -t;                       // log2e * sigma * (s_winner - s_loser)
    const float e = __builtin_amdgcn_exp2f(-fabsf(z));
    const float r = __builtin_amdgcn_rcpf(1.0f + e);
    const float psi = (z >= 0.0f) ? e * r : r;         // sigmoid(-sigma (s_win - s_lose))
    const float lg = log2_1p(e) + fmaxf(-z, 0.0f);     // log2(1 + exp(-sigma (s_win - s_lose)))
    const float Wm = (gt | lt) ? W : 0.0f;
    l += gt ? Wm * lg : 0.0f;
    g += (gt ? -Wm : Wm) * psi;
}

// ARP1 / NDCG1: term(i,j) = a_i * log2(1 + exp(-sigma (s_i - s_j))) for ALL i, j < n
// (-log2(sigmoid ** a_i), loss/pairwise_lambda.py:114-117, :165-173).
__device__ __forceinline__ void pair_rowweight(float sk, float ak, float sm, float am, float c1,
                                               float &g, float &l)
{
    const float t = (sk - sm) * c1;
    const float e = __builtin_amdgcn_exp2f(-fabsf(t));
    const float r = __builtin_amdgcn_rcpf(1.0f + e);
    const float sneg = (t >= 0.0f) ? e * r : r;        // sigmoid(-sigma (s_k - s_m))
    const float lg = log2_1p(e) + fmaxf(-t, 0.0f);
    l += ak * lg;
    g += am - (ak + am) * sneg;                        // -a_k sig(-x) + a_m sig(x)
}

// lists longer than this take the sort path (DPT == 0 instantiation of metric_kernel)
constexpr int kSortRankMinLen = 256;
__host__ __device__ constexpr int sort_pow2(int L)
{
    int P = 64;
    while (P < L) P <<= 1;
    return P;
}

// ---------------------------------------------------------------------------------
// Ranks of long lists by a bitonic sort instead of the O(n^2) counting rank.
// Every document becomes one 64-bit key: (order-reversed score bits << 32) | index, so that an
// ascending unsigned sort is exactly "score descending, index ascending" -- the tie rule of the
// counting rank (-0.0 is folded into +0.0 first so that it ties with it, as the float compare
// does).  Slots past n hold the all-ones sentinel and stay at the tail.  Element i = e*T + tid
// lives in register e of thread tid; a compare-exchange partner at distance j is in the same
// thread (j >= T), reached through LDS (64 <= j < T, one buffer, two barriers), or a lane
// shuffle (j < 64).  P = E*T is a power of two >= n.  O(P log^2 P) work: L = 1000 ranks in
// ~1/7 of the counting rank's time on MI355X.  NaN scores sort first (the counting rank gave
// them colliding ranks).
// ---------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long rank_key(float v, int idx)
{
    const unsigned bits = __float_as_uint(v + 0.0f);
    const unsigned asc = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
    return ((unsigned long long)(~asc) << 32) | (unsigned)idx;
}

// Tie priorities from a seed (the reference's ONE random permutation per call shared by all rows,
// utils/tensor_operations.py:43-45, without drawing and shipping a permutation): list position j gets
// the key word  hash19(seed, j) << 12 | j  -- distinct for every j < 4096, ordered by a 19-bit hash of
// (seed, j), the position itself decoded from the low 12 bits.  Equal scores then rank in the order of
// the hashes: a pseudo-random permutation of the tied documents, the same for every row, free.
__host__ __device__ inline unsigned tie_hash_word(unsigned long long seed, unsigned j)
{
    unsigned h = (unsigned)seed ^ (j * 0x9E3779B1u);
    h ^= (unsigned)(seed >> 32);
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return ((h >> 13) << 12) | (j & 0xFFFu);
}
constexpr int kTieHashMaxLen = 4096;

// inv (LDS, may be null): the low key word is a tie priority, inv[priority] = document index;
// low_mask != 0: the document index is the low key word & low_mask (hashed tie words).
template <int E>
__device__ __forceinline__ void sort_ranks(unsigned long long (&v)[E], int P, int nb, int *rank_out,
                                           unsigned long long *xbuf, const int *inv = nullptr, int low_mask = 0)
{
    const int tid = threadIdx.x;
    const int T = blockDim.x;
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (j >= T) {
                const int je = j / T;                          // partner register
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    if ((e & je) == 0 && (e | je) < E) {
                        const int i = e * T + tid;
                        const bool up = (i & k) == 0;
                        const unsigned long long a = v[e], b = v[e | je];
                        const bool swap = (a > b) == up;
                        v[e] = swap ? b : a;
                        v[e | je] = swap ? a : b;
                    }
                }
            } else {
                unsigned long long other[E];
                if (j >= 64) {
                    __syncthreads();                           // previous readers of xbuf are done
#pragma unroll
                    for (int e = 0; e < E; ++e) xbuf[e * T + tid] = v[e];
                    __syncthreads();
#pragma unroll
                    for (int e = 0; e < E; ++e) other[e] = xbuf[(e * T + tid) ^ j];
                } else {
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v[e], j);
                        const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v[e] >> 32), j);
                        other[e] = ((unsigned long long)hi << 32) | lo;
                    }
                }
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const int i = e * T + tid;
                    const bool keep_min = ((i & j) == 0) == ((i & k) == 0);
                    const bool smaller = v[e] < other[e];
                    v[e] = (smaller == keep_min) ? v[e] : other[e];
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
        if (v[e] != ~0ull) {
            const int low = (int)(unsigned)v[e];
            const int idx = inv ? inv[low] : (low_mask ? (low & low_mask) : low);
            if (idx < nb) rank_out[idx] = e * T + tid;
        }
    }
}

// Counting rank on packed keys: with (order-reversed value bits << 32 | index) keys (rank_key) the
// tie rule is part of the key, so "m comes before k" is ONE unsigned 64-bit compare and the count
// one add-with-carry -- about 2.5x fewer VALU instructions per pair than comparing floats and
// indices separately.  keys[k] = (score key, label key), built by the caller for k < nb.
template <int DPT, bool WITH_Y>
__device__ __forceinline__ void count_ranks_keyed(const ulonglong2 *keys, int nb, int owners, int o,
                                                  int m0, int m1, bool partial, int *rank_s,
                                                  int *rank_y)
{
    for (int base = 0; base < nb; base += owners * DPT) {
        const int wave_first = base + (o & ~63);
        if (wave_first >= nb) continue;                       // wave-uniform
        unsigned long long kx[DPT], ky[DPT];
        int cs[DPT], cy[DPT], kk[DPT];
#pragma unroll
        for (int c = 0; c < DPT; ++c) {
            kk[c] = base + o + c * owners;
            const ulonglong2 v = keys[kk[c] < nb ? kk[c] : 0];
            kx[c] = v.x; ky[c] = v.y; cs[c] = 0; cy[c] = 0;
        }
#pragma unroll 4
        for (int m = m0; m < m1; ++m) {
            const ulonglong2 v = keys[m];
#pragma unroll
            for (int c = 0; c < DPT; ++c) {
                cs[c] += (v.x < kx[c]);
                if (WITH_Y) cy[c] += (v.y < ky[c]);
            }
        }
#pragma unroll
        for (int c = 0; c < DPT; ++c) {
            if (kk[c] < nb) {
                if (partial) {
                    atomicAdd(&rank_s[kk[c]], cs[c]);
                    if (WITH_Y) atomicAdd(&rank_y[kk[c]], cy[c]);
                } else {
                    rank_s[kk[c]] = cs[c];
                    if (WITH_Y) rank_y[kk[c]] = cy[c];
                }
            }
        }
    }
}

struct LossParams {
    const float *scores;
    const void *rel;
    const int64_t *n;
    float *loss;
    float *dscores;
    int B, L;
    float sigma;
    int rel_dtype;
    int msplit;
    int sched;          // > 0: number of 64-query sample groups of the list-length scheduling
};

// LDS carve (bytes), L4 = L rounded up to 4:
//   sy    float2[L4]          (score, label) -- for NDCG1 the label slot is overwritten by a_k
//   q4    float4[L4]          NDCG2 only: (score, label, gain G, rank)
//   delta float [ndcg2_delta_floats(L4)]  NDCG2 only: |1/D(d) - 1/D(d+1)|, D(d) = log2(2+d); on the symmetric
//                             path twice as long, zero beyond the list (see fill_ndcg2_delta)
//   gpart float [msplit*L4]   per-slice gradient partials; aliased by the two int rank arrays
//   red   float [32]
__host__ __device__ constexpr size_t ndcg2_delta_floats(size_t L4)
{
    return (L4 <= (size_t)kLossSymMaxLen ? 2 * L4 : L4) + 4;
}

// KIND codes of the fused MLP step's listwise loss slot (ltr_mlp_listwise.inc), outside enum ltr_loss_kind: internal to
// the MLP kernels' KIND parameter, never part of the C ABI (whose listwise codes are LTR_LISTWISE_*, ltr_listwise.h).
constexpr int LTR_MLP_LISTNET = 16;
constexpr int LTR_MLP_LISTMLE = 17;
constexpr int LTR_MLP_LAMBDARANK = 18;     // (ltr_mlp_lambdarank_f32, include/ltr_mlp_lambdarank.h)
constexpr size_t kRowScratchBytes = (32 + 64) * 4;      // red + scan of the ranked-row layout (ltr_ranked.inc)

__host__ __device__ constexpr size_t loss_lds_bytes(int kind, int L, int msplit)
{
    const size_t L4 = (size_t)((L + 3) & ~3);
    // the listwise slot of the MLP kernels: ListNet keeps sy and the reduction scratch, ListMLE the whole ranked-row
    // layout of the counting rank (ranked_row_layout(L, false).end: sy, two rank arrays, 16 B of keys per document),
    // and so does LambdaRank
    if (kind == LTR_MLP_LISTNET) return 8 * L4 + kRowScratchBytes;
    if (kind == LTR_MLP_LISTMLE || kind == LTR_MLP_LAMBDARANK) return 32 * L4 + kRowScratchBytes;
    size_t bytes = 8 * L4;
    if (kind == LTR_NDCG2) bytes += 16 * L4 + 4 * ndcg2_delta_floats(L4);
    size_t g = 4 * L4 * (size_t)msplit;
    if ((kind == LTR_NDCG1 || kind == LTR_NDCG2) && g < 8 * L4) g = 8 * L4;
    // room behind the rank arrays for the packed keys of the counting rank (16 B per document)
    if ((kind == LTR_NDCG1 || kind == LTR_NDCG2) && L4 <= (size_t)kLossSymMaxLen && g < 24 * L4) g = 24 * L4;
    return bytes + g + 48 * 4;        // red: 32 floats + 16 deferred maxDCG shares of a 16-wave workgroup (below)
}

// LDS views of one query, carved from the dynamic segment (see loss_lds_bytes).
struct QueryLds {
    float2 *sy;
    float4 *q4;
    float *delta;
    float *gpart;
    int *rank_s;
    int *rank_y;
    float *red;
    unsigned gbytes;      // bytes of the gpart region (the sort path borrows its tail)
};

template <int KIND>
__device__ __forceinline__ QueryLds carve_query_lds(unsigned char *base, int L4, int msplit)
{
    QueryLds q;
    q.sy = reinterpret_cast<float2 *>(base);
    unsigned char *cur = base + 8 * (size_t)L4;
    q.q4 = nullptr;
    q.delta = nullptr;
    if (KIND == LTR_MLP_LISTNET || KIND == LTR_MLP_LISTMLE || KIND == LTR_MLP_LAMBDARANK) {
        // (label, score) pairs in sy -- LambdaRank: (score, label); the rest of the block is carved by the listwise
        // slot (mlp_listwise_slot / mlp_lambdarank_slot, ltr_mlp_listwise.inc)
        q.gpart = nullptr; q.rank_s = nullptr; q.rank_y = nullptr; q.gbytes = 0;
        q.red = nullptr;
        return q;
    }
    if (KIND == LTR_NDCG2) {
        q.q4 = reinterpret_cast<float4 *>(cur);
        cur += 16 * (size_t)L4;
        q.delta = reinterpret_cast<float *>(cur);
        cur += 4 * ndcg2_delta_floats((size_t)L4);
    }
    q.gpart = reinterpret_cast<float *>(cur);
    q.rank_s = reinterpret_cast<int *>(cur);      // aliases gpart (dead before gpart is written)
    q.rank_y = q.rank_s + L4;
    size_t g = 4 * (size_t)L4 * msplit;
    if ((KIND == LTR_NDCG1 || KIND == LTR_NDCG2) && g < 8 * (size_t)L4) g = 8 * (size_t)L4;
    if ((KIND == LTR_NDCG1 || KIND == LTR_NDCG2) && L4 <= kLossSymMaxLen && g < 24 * (size_t)L4) g = 24 * (size_t)L4;
    cur += g;
    q.gbytes = (unsigned)g;
    q.red = reinterpret_cast<float *>(cur);
    return q;
}

// The discount-difference table of LambdaNDCG2 (loss/pairwise_lambda.py:206-211): delta[d] =
// |1/D(d) - 1/D(d+1)| for 1 <= d < nb.  delta[0] is never the distance of two different documents
// (ranks are a permutation) and is kept 0; on the symmetric path (L4 <= kSymMaxLen) the table runs on
// to 2 nb with zeros: an inert document (index >= n) carries the rank 2 nb - 1, so its distance to any
// real rank lands in [nb, 2 nb) and to another inert one at 0 -- the weight of every pair with an inert
// end is 0 without a mask in the pair step.
// 1 / D(r), D(r) = log2(2 + r) >= 1 (v_log_f32 and v_rcp_f32: 1 ulp each, no range handling needed)
__device__ __forceinline__ float inv_discount(float r)
{
    return __builtin_amdgcn_rcpf(__builtin_amdgcn_logf(2.0f + r));
}

// gain 2^y - 1 (loss/pairwise_lambda.py:221-228); v_exp_f32 is exact on the integer grades
__device__ __forceinline__ float ndcg_gain(float y)
{
    return __builtin_amdgcn_exp2f(y) - 1.0f;
}

__device__ __forceinline__ void fill_ndcg2_delta(float *delta, int nb, int L4, int tid, int T)
{
    const int dn = (L4 <= kLossSymMaxLen) ? 2 * nb : nb;
    for (int d = tid; d < dn; d += T) {
        const float v = fabsf(inv_discount((float)d) - inv_discount((float)d + 1.0f));
        delta[d] = (d >= 1 && d < nb) ? v : 0.0f;
    }
}

// NDCG kinds: ranks by score and by label, maxDCG, gains.  On return (barrier passed)
//   NDCG1: sy[k].y = a_k = G_k / log2(2 + rank_k);   NDCG2: q4[k] = (s, y, G, rank), delta table.
// TW > 0: the workgroup has TW waves (compile-time): the maxDCG sum takes one barrier instead of two.
// DEFER (needs TW > 0; the caller runs pairwise_core_sym<KIND, TW, true> next): every pair term of both
// NDCG kinds carries the factor 1 / maxDCG, so the gains stay UNNORMALISED here (NDCG1: a_k = g_k / D(rank_k),
// NDCG2: q4[k].z = g_k = 2^y - 1), each wave leaves its share of maxDCG in red[8 + wave], and the pair pass
// applies 1 / maxDCG once to the query's loss and to the gradient scale -- one barrier and one dependent
// phase fewer per query; the delta table (query-independent up to its length) is filled before the first
// barrier instead of after the last.
template <int KIND, int DPT, int TW = 0, bool DEFER = false>
__device__ __forceinline__ void prepare_ndcg(const QueryLds &q, int nb, int owners, int o, int m0,
                                             int m1, bool partial)
{
    const int tid = threadIdx.x;
    const int T = TW > 0 ? TW * 64 : (int)blockDim.x;
    float2 *sy = q.sy;
    static_assert(!DEFER || (TW > 0 && TW <= 16), "deferred normalisation: compile-time wave count, red[8 .. 16) / red[32 .. 48)");
    // Lists longer than kSortRankMinLen: both rankings by a bitonic sort of packed (key, index)
    // words (see sort_ranks) when the exchange buffer fits behind the rank arrays in the gpart
    // region -- it always does on the symmetric path (L <= 1024); otherwise the counting rank.
    const int L4r = (int)(q.rank_y - q.rank_s);
    if (DEFER && KIND == LTR_NDCG2) fill_ndcg2_delta(q.delta, nb, L4r, tid, T);
    int Pq = 64;
    while (Pq < nb) Pq <<= 1;
    // (every thread writes its register(s) to the exchange buffer: max(Pq, T) or 4T words)
    const unsigned xwords = (unsigned)(Pq <= T ? T : 4 * T);
    const bool sorted = nb > kSortRankMinLen && Pq <= 4 * T &&
                        q.gbytes >= 8u * (unsigned)L4r + 8u * xwords;
    if (sorted) {
        unsigned long long *xbuf = reinterpret_cast<unsigned long long *>(q.rank_s + 2 * L4r);
        if (Pq <= T) {
            unsigned long long v[1];
            v[0] = (tid < nb) ? rank_key(sy[tid].x, tid) : ~0ull;
            sort_ranks<1>(v, Pq, nb, q.rank_s, xbuf);
            v[0] = (tid < nb) ? rank_key(sy[tid].y, tid) : ~0ull;
            sort_ranks<1>(v, Pq, nb, q.rank_y, xbuf);
        } else {
            unsigned long long v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (e * T + tid < nb) ? rank_key(sy[e * T + tid].x, e * T + tid) : ~0ull;
            sort_ranks<4>(v, Pq, nb, q.rank_s, xbuf);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (e * T + tid < nb) ? rank_key(sy[e * T + tid].y, e * T + tid) : ~0ull;
            sort_ranks<4>(v, Pq, nb, q.rank_y, xbuf);
        }
    } else if (q.gbytes >= 24u * (unsigned)L4r) {
        ulonglong2 *keys = reinterpret_cast<ulonglong2 *>(q.rank_s + 2 * L4r);   // behind the ranks
        for (int k = tid; k < nb; k += T) {
            const float2 v = sy[k];
            keys[k] = make_ulonglong2(rank_key(v.x, k), rank_key(v.y, k));
        }
        __syncthreads();
        count_ranks_keyed<DPT, true>(keys, nb, owners, o, m0, m1, partial, q.rank_s, q.rank_y);
    } else {
        count_ranks<DPT, true>(sy, nb, owners, o, m0, m1, partial, q.rank_s, q.rank_y);
    }
    __syncthreads();
    // _max_dcg (loss/pairwise_lambda.py:231-241): labels sorted descending over the
    // first n documents, gains 2^y - 1, discounts log2(2 + r).
    if (DEFER) {
        float part = 0.f;
        for (int k = tid; k < nb; k += T) {
            const float2 v = sy[k];
            const float g = ndcg_gain(v.y);
            part = __builtin_fmaf(g, inv_discount((float)q.rank_y[k]), part);
            const int r = q.rank_s[k];
            if (KIND == LTR_NDCG1)
                sy[k].y = g * inv_discount((float)r);        // a_k * maxDCG
            else
                q.q4[k] = make_float4(v.x, v.y, g, (float)r);
        }
        const float ws = wave_sum(part);
        if ((tid & 63) == 0) q.red[(TW > 8 ? 32 : 8) + (tid >> 6)] = ws;       // (16 waves: behind the pair pass's slots)
        __syncthreads();                                    // ranks dead from here: gpart may be written
        return;
    }
    float part = 0.f;
    for (int k = tid; k < nb; k += T)
        part = __builtin_fmaf(ndcg_gain(sy[k].y), inv_discount((float)q.rank_y[k]), part);
    float maxdcg;
    if (TW > 0) {
        const float ws = wave_sum(part);
        if ((tid & 63) == 0) q.red[tid >> 6] = ws;
        __syncthreads();
        maxdcg = 0.f;
#pragma unroll
        for (int i = 0; i < (TW > 0 ? TW : 1); ++i) maxdcg += q.red[i];
    } else {
        maxdcg = block_sum(part, q.red);
    }
    if (maxdcg == 0.0f) maxdcg = 1.0f;                     // pairwise_lambda.py:227
    const float inv_maxdcg = 1.0f / maxdcg;
    for (int k = tid; k < nb; k += T) {
        const float2 v = sy[k];
        const float G = ndcg_gain(v.y) * inv_maxdcg;        // _ndcg_gains, :221-228
        const int r = q.rank_s[k];
        if (KIND == LTR_NDCG1)
            sy[k].y = G * inv_discount((float)r);           // a_k = G_k / D(rank_k)
        else
            q.q4[k] = make_float4(v.x, v.y, G, (float)r);
    }
    if (KIND == LTR_NDCG2) fill_ndcg2_delta(q.delta, nb, L4r, tid, T);
    __syncthreads();                                        // ranks dead from here: gpart may be written
}

// The per-query core shared by the loss kernel and the fused scorer kernel.
// Precondition: q.sy[0..nb) = (score, label) is staged and visible (barrier passed); for the
// NDCG kinds q.rank_s[0..2*L4) is zeroed.  Postcondition (after the trailing barrier):
// q.gpart[slice*L4 + k] holds the slice partials of d(pair sum)/d s_k in units of `gscale`;
// returns the final per-query loss (modifier applied) to every thread and, in `gsum`, the sum
// over documents of d loss / d s_k (= d loss / d bias of a linear scorer; ~0 by construction).
template <int KIND, int DPT, bool PIPE = true>
__device__ __forceinline__ float pairwise_core(const QueryLds &q, int nb, int L4, int msplit,
                                               float sigma, float &gscale, float &gsum)
{
    const int tid = threadIdx.x;
    const int T = blockDim.x;
    const int owners = T / msplit;                 // multiple of 64: slices are whole waves
    const int o = tid % owners;
    const int slice = tid / owners;
    float2 *sy = q.sy;

    // slice of the streamed index this thread's wave walks
    // (slices are whole waves, so these bounds are wave-uniform: keep them in SGPRs)
    const int mlen = ((nb + msplit - 1) / msplit + 1) & ~1;        // even: slices start 16-B aligned
    const int m0 = __builtin_amdgcn_readfirstlane(min(nb, slice * mlen));
    const int m1 = __builtin_amdgcn_readfirstlane(min(nb, m0 + mlen));
    const float c1 = sigma * kLog2e;

    if (KIND == LTR_NDCG1 || KIND == LTR_NDCG2)
        prepare_ndcg<KIND, DPT>(q, nb, owners, o, m0, m1, msplit > 1);

    // ---- pair pass ----
    float lacc = 0.f, gacc = 0.f;
    for (int base = 0; base < nb; base += owners * DPT) {
        const int wave_first = base + (o & ~63);
        if (wave_first >= nb) continue;                          // wave-uniform
        float sk[DPT], yk[DPT], Gk[DPT], rk[DPT], gk[DPT];
        int kk[DPT];
#pragma unroll
        for (int c = 0; c < DPT; ++c) {
            kk[c] = base + o + c * owners;
            const bool valid = kk[c] < nb;
            gk[c] = 0.f; Gk[c] = 0.f; rk[c] = 0.f;
            if (KIND == LTR_NDCG2) {
                const float4 v = valid ? q.q4[kk[c]] : make_float4(0.f, __builtin_nanf(""), 0.f, 0.f);
                sk[c] = v.x; yk[c] = v.y; Gk[c] = v.z; rk[c] = v.w;
            } else if (KIND == LTR_ARP1 || KIND == LTR_NDCG1) {
                const float2 v = valid ? sy[kk[c]] : make_float2(0.f, 0.f);   // a_k = 0: no loss
                sk[c] = v.x; yk[c] = v.y;
            } else {
                // NaN label: both orientation tests fail -> an idle owner contributes nothing
                const float2 v = valid ? sy[kk[c]] : make_float2(0.f, __builtin_nanf(""));
                sk[c] = v.x; yk[c] = v.y;
            }
        }
        // One streamed document against the DPT owned ones.
        auto visit = [&](float sm, float ym, float Gm, float rm) {
#pragma unroll
            for (int c = 0; c < DPT; ++c) {
                if (KIND == LTR_NDCG2) {
                    const int d = (int)fabsf(rk[c] - rm);
                    const float W = q.delta[d] * fabsf(Gk[c] - Gm);
                    pair_oriented(sk[c], yk[c], sm, ym, W, c1, gk[c], lacc);
                } else if (KIND == LTR_HINGE || KIND == LTR_DCG_HINGE) {
                    pair_hinge(sk[c], yk[c], sm, ym, gk[c], lacc);
                } else if (KIND == LTR_LOGISTIC) {
                    pair_oriented(sk[c], yk[c], sm, ym, 1.0f, c1, gk[c], lacc);
                } else if (KIND == LTR_ARP2) {
                    pair_oriented(sk[c], yk[c], sm, ym, fabsf(yk[c] - ym), c1, gk[c], lacc);
                } else {
                    pair_rowweight(sk[c], yk[c], sm, ym, c1, gk[c], lacc);
                }
            }
        };
        // Streamed documents come from LDS in 64-byte chunks (4 x ds_read_b128, wave-uniform
        // address = broadcast), software-pipelined one chunk ahead so the LDS latency hides under
        // the pair arithmetic instead of stalling every iteration.
        constexpr int MU = (KIND == LTR_NDCG2) ? 4 : 8;                  // documents per chunk
        const float4 *src = (KIND == LTR_NDCG2) ? q.q4 : reinterpret_cast<const float4 *>(sy);
        constexpr int VPD = (KIND == LTR_NDCG2) ? 1 : 2;                 // documents per float4
        // PIPE = false (register-tight callers): plain loop, no prefetch registers
        const int mfull = PIPE ? m0 + ((m1 - m0) / MU) * MU : m0;        // m0 is even (see mlen)
        if (mfull > m0) {
            float4 cur[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) cur[j] = src[m0 / VPD + j];
            for (int m = m0; m < mfull; m += MU) {
                const int mn = (m + MU < mfull) ? (m + MU) : m;          // last chunk: harmless re-read
                float4 nxt[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) nxt[j] = src[mn / VPD + j];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (KIND == LTR_NDCG2) {
                        visit(cur[j].x, cur[j].y, cur[j].z, cur[j].w);
                    } else {
                        visit(cur[j].x, cur[j].y, 0.f, 0.f);
                        visit(cur[j].z, cur[j].w, 0.f, 0.f);
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) cur[j] = nxt[j];
            }
        }
        for (int m = mfull; m < m1; ++m) {                               // remainder (< MU documents)
            if (KIND == LTR_NDCG2) {
                const float4 v = q.q4[m];
                visit(v.x, v.y, v.z, v.w);
            } else {
                const float2 v = sy[m];
                visit(v.x, v.y, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int c = 0; c < DPT; ++c)
            if (kk[c] < nb) { q.gpart[(size_t)slice * L4 + kk[c]] = gk[c]; gacc += gk[c]; }
    }

    // ---- per-query reduction (loss and gradient sum in one pass) and loss modifier ----
    float total = lacc;
    block_sum2(total, gacc, q.red);           // its barriers publish gpart when there are >= 2 waves
    if (T == kWave) __syncthreads();
    gscale = 1.0f;
    if (KIND == LTR_DCG_HINGE) {
        // _loss_modifier (loss/pairwise_additive.py:132-133): -1/ln(2+H);
        // d/dH = 1/((2+H) ln^2(2+H))
        const float lg = logf(2.0f + total);
        gscale = 1.0f / ((2.0f + total) * lg * lg);
        total = -1.0f / lg;
    } else if (KIND != LTR_HINGE) {
        gscale = sigma / kLn2;
    }
    gsum = gacc * gscale;
    return total;
}

// ---------------------------------------------------------------------------------
// Symmetric pair pass (list_len <= kSymMaxLen): every UNORDERED pair is evaluated once.
// Documents are cut into 64-wide tiles; a job is an unordered tile pair (a, b).  A wave keeps
// the "home" tile a in registers (lane i = document 64a+i) and a "visitor" tile b that ROTATES
// through the lanes: at step j lane i holds visitor 64b + ((i+j) & 63) -- its score, label and
// its gradient accumulator travel together, one v_mov_b32_dpp wave_rol:1 each per step (no LDS,
// no atomics).  One evaluation of the pair term updates the home gradient (+c) and the visitor
// gradient (-c): every loss on this path depends on score DIFFERENCES only, so the two
// contributions are exact negatives.  Diagonal jobs take j = 1..32 (the last step on half the
// lanes), off-diagonal jobs j = 0..63: 32*nt^2 steps in all, split evenly over the waves; each
// wave flushes into its PRIVATE gpart slice (deterministic).  This halves the VALU work of the
// both-ends formulation (pairwise_core), which remains the path for longer lists.
// Inert documents (index >= n[b]) carry NaN sentinels: NaN label for the oriented kinds (both
// label tests fail), NaN score for the row-weight kinds (detected with x == x).
// Precondition: sy[0..nb) staged (q4/delta/a_k prepared for the NDCG kinds), Lt = 64*ceil(L/64).
// Postcondition (after the trailing barrier): gpart[w*Lt + k], w < blockDim/64, hold partials of
// d(pair sum)/d s_k in units of gscale; returns the per-query loss.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ float wave_rol1(float v)
{
    // lane i <- lane (i+1) & 63; every lane has a valid source, so no "old" value is needed
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x134, 0xF, 0xF, true));
}

__device__ __forceinline__ int wave_rol1i(int v)
{
    return __builtin_amdgcn_mov_dpp(v, 0x134, 0xF, 0xF, true);
}

// LDS read at base + |a - b| (a, b: byte offsets): the address is ONE v_sad_u32
typedef __attribute__((address_space(3))) const float ltr_lds_cfloat;
__device__ __forceinline__ float lds_at_absdiff(unsigned base, int a, int b)
{
    unsigned addr;
    asm("v_sad_u32 %0, %1, %2, %3" : "=v"(addr) : "v"(a), "v"(b), "s"(base));
    return *reinterpret_cast<ltr_lds_cfloat *>(addr);
}

// part / parts: this workgroup is one of `parts` that share the query's pair units (split-query
// launch); raw: return the plain pair sum (no loss modifier, gscale untouched).
// TW > 0: the workgroup has TW waves (compile-time: no dispatch-packet read, shifts instead of
// divisions) and, when it owns the whole query, only as many of them take pair units as the query
// has work for (at least kSymMinSteps steps per wave, a power of two of waves).  Measured (C2,
// fused hinge step, us): 1 step per wave 11.3, 4: 11.6, 8: 11.9, 16: 12.3 -- the pass is latency-
// bound, more waves with fewer steps each win, so the default is 1 (every wave that can get a step).
// Idle waves still publish a zero gradient slice.
constexpr int kSymMinSteps = 1;
#ifdef LTR_TRACE
#define LTR_SYM_STAMP(i) do { if (trace && threadIdx.x == 0) trace[i] = (long long)wall_clock64(); } while (0)
#else
#define LTR_SYM_STAMP(i) do { } while (0)
#endif
// DEFER: the NDCG gains arrive unnormalised with the waves' maxDCG shares in red[8 .. 8 + TW)
// (prepare_ndcg<..., DEFER = true>); 1 / maxDCG is applied to the loss and to gscale here.
// INTLAB (hinge kinds): the labels are integers (an integer label dtype), so the sign of the label
// difference is ONE v_med3 of the difference clamped to [-1, 1] instead of two compares and two selects
// (13 -> 11 VALU per step); inert documents then carry (score -inf, label -3e38): against a real document
// they are the lower-labelled side with an infinitely wide margin -- inactive from either end -- and against
// each other the margin term is a NaN that v_max drops and no compare passes.
template <int KIND, int TW = 0, bool DEFER = false, bool INTLAB = false>
__device__ __forceinline__ float pairwise_core_sym(const QueryLds &q, int nb, int Lt, float sigma,
                                                   float &gscale, int part = 0, int parts = 1,
                                                   bool raw = false, long long *trace = nullptr)
{
    const int tid = threadIdx.x;
    const int T = TW > 0 ? TW * 64 : (int)blockDim.x;
    const int lane = tid & 63;
    const int wl = __builtin_amdgcn_readfirstlane(tid >> 6);
    int w = part * (T >> 6) + wl;                            // wave index among all parts
    int W = parts * (T >> 6);
    const int nt = (nb + 63) >> 6;
    const float c1 = sigma * kLog2e;
    constexpr bool kRowWeight = (KIND == LTR_ARP1 || KIND == LTR_NDCG1);
    constexpr bool kIntHinge = INTLAB && (KIND == LTR_HINGE || KIND == LTR_DCG_HINGE);
    const float kNaN = __builtin_nanf("");
    // LambdaNDCG2: ranks travel as byte offsets into the delta table; an inert document's rank is
    // 2 nb - 1 (see fill_ndcg2_delta)
    const int zrank = 4 * (2 * nb - 1);
    const unsigned dbase = (KIND == LTR_NDCG2)
        ? (unsigned)(size_t)(__attribute__((address_space(3))) float *)q.delta : 0u;
    auto delta_at = [&](int ra, int rb) { return lds_at_absdiff(dbase, ra, rb); };
    float *gw = q.gpart + (size_t)wl * Lt;
    for (int i = lane; i < 64 * nt; i += 64) gw[i] = 0.f;

    float lacc = 0.f;
    // Steps per job: off-diagonal 64 (j = 0..63); diagonal 32 (j = 1..32), except that the last,
    // partially filled tile only has pairs at j < hc (hc = its document count) while hc <= 32.
    const int hc_last = nb - 64 * (nt - 1);
    const int dlast = (hc_last - 1 < 32) ? (hc_last - 1) : 32;
    const int S = (nt > 0) ? (32 * nt * nt - (32 - dlast)) : 0;
    int u, u1;
    if (TW > 0 && parts == 1 && (TW & (TW - 1)) == 0) {
        // waves that take units: the largest power of two <= S / kSymMinSteps, in [1, TW]
        int sh = 0;
        while ((2 << sh) <= TW && (2 << sh) * kSymMinSteps <= S) ++sh;
        W = 1 << sh;
        u = (wl * S) >> sh;
        u1 = (wl < W) ? ((wl + 1) * S) >> sh : u;
        if (wl >= W) u = u1 = 0;
        w = wl;
    } else if (TW > 0 && parts == 1) {
        u = (wl * S) / TW;                                   // (division by a constant)
        u1 = ((wl + 1) * S) / TW;
    } else {
        u = (w * S) / W;
        u1 = ((w + 1) * S) / W;
    }
    // decode the first unit of this wave into (a, b, j): row a of the job triangle holds its
    // diagonal job (32 steps, dlast in the last row) and 64 steps for every b > a -- walk the rows
    // (<= nt iterations), then the column is a division (a job-by-job walk cost up to nt^2/2
    // iterations per wave, a quarter of a split-launch part's whole work at n = 1000)
    int a = 0, rem = u;
    while (a < nt - 1) {
        const int rowlen = 32 + 64 * (nt - 1 - a);
        if (rem < rowlen) break;
        rem -= rowlen;
        ++a;
    }
    int b = a;
    {
        const int dl = (a == nt - 1) ? dlast : 32;
        if (rem >= dl && a < nt - 1) {
            rem -= dl;
            b = a + 1 + (rem >> 6);
            rem &= 63;
        }
    }
    int j = ((a == b) ? 1 : 0) + rem;
    LTR_SYM_STAMP(0);                                        // slices zeroed, units decoded

    while (u < u1) {
        const bool diag = (a == b);
        const int jend = diag ? (1 + ((a == nt - 1) ? dlast : 32)) : 64;
        // ---- load the home tile of this segment ----
        const int hidx = 64 * a + lane;
        const bool hvalid = hidx < nb;
        float sh, yh = 0.f, Gh = 0.f;
        int rh = 0;                                              // LambdaNDCG2: 4 * rank (a byte offset into delta)
        if (KIND == LTR_NDCG2) {
            const float4 hv = q.q4[hvalid ? hidx : 0];
            sh = hv.x; Gh = hv.z; rh = hvalid ? ((int)hv.w << 2) : zrank;
        } else {
            const float2 hv = q.sy[hvalid ? hidx : 0];
            if (kRowWeight) { sh = hvalid ? hv.x : kNaN; yh = hv.y; }
            else if (kIntHinge) { sh = hvalid ? hv.x : -__builtin_inff(); yh = hvalid ? hv.y : -3.0e38f; }
            else { sh = hv.x; yh = hvalid ? hv.y : kNaN; }
        }
        float gh = 0.f;
        // A visitor chain: the visitor tile rotated by `rot` lanes, its gradient accumulator travelling
        // with it.  LambdaNDCG2: the discount difference delta(|rank_home - rank_visitor|) comes
        // from an LDS table; it is fetched ONE STEP AHEAD (the next visitor's rank is one rotation
        // away), so the LDS round trip is off the dependency chain of the step.
        struct Vis { float sv, yv, Gv, gv, dcur; int rv; };
        auto load_vis = [&](Vis &V, int rot) {
            const int vidx = 64 * b + ((lane + rot) & 63);
            const bool vvalid = vidx < nb;
            V.Gv = 0.f; V.rv = 0; V.gv = 0.f; V.dcur = 0.f; V.yv = 0.f;
            if (KIND == LTR_NDCG2) {
                const float4 vv = q.q4[vvalid ? vidx : 0];
                V.sv = vv.x; V.Gv = vv.z; V.rv = vvalid ? ((int)vv.w << 2) : zrank;
                V.dcur = delta_at(rh, V.rv);
            } else {
                const float2 vv = q.sy[vvalid ? vidx : 0];
                if (kRowWeight) { V.sv = vvalid ? vv.x : kNaN; V.yv = vv.y; }
                else if (kIntHinge) { V.sv = vvalid ? vv.x : -__builtin_inff(); V.yv = vvalid ? vv.y : -3.0e38f; }
                else { V.sv = vv.x; V.yv = vvalid ? vv.y : kNaN; }
            }
        };
        // one evaluation of the pair (home, visitor); `half`: only lanes < 32 count (j == 32)
        auto visit = [&](Vis &V, bool half) {
            const float sv = V.sv, yv = V.yv;
            const bool on = half ? (lane < 32) : true;
            float c;                                             // d term / d s_home
            if (KIND == LTR_HINGE || KIND == LTR_DCG_HINGE) {
                // sgn = -1 when the home document is the higher-labelled one, +1 when the visitor is,
                // 0 when the labels are equal or one of them is the NaN sentinel (ordered compares);
                // margin term u = |sgn| + sgn*(s_home - s_vis): 0 for an inert pair; the pair counts
                // iff u >= 0 (non-strict, as the reference leaves the gradient at the margin) -- one
                // compare feeding selects, no scalar mask arithmetic in the dependency chain
                float sgn;
                if (kIntHinge) {
                    sgn = __builtin_amdgcn_fmed3f(yv - yh, -1.0f, 1.0f);
                } else {
                    sgn = (yh < yv) ? 1.0f : 0.0f;
                    sgn = (yh > yv) ? -1.0f : sgn;
                }
                if (half) sgn = on ? sgn : 0.0f;
                const float uu = __builtin_fmaf(sgn, sh - sv, __builtin_fabsf(sgn));
                lacc += __builtin_fmaxf(uu, 0.0f);
                c = (uu >= 0.0f) ? sgn : 0.0f;
            } else if (KIND == LTR_NDCG2) {
                // The pair's weight is delta(|rank distance|) * |G_home - G_vis|, and the gains order the
                // two documents exactly as their labels do (equal labels = equal gains = weight 0; an inert
                // document: delta = 0), so the signed weight Ws = delta * (G_home - G_vis) carries the
                // orientation: "the higher-labelled document scores higher" <=> t * Ws >= 0.  No label
                // compare, no mask; e = exp2(-|t|) does not depend on the orientation at all.
                const float t = (sh - sv) * c1;
                float Ws = V.dcur * (Gh - V.Gv);
                if (half) Ws = on ? Ws : 0.0f;
                const float e = __builtin_amdgcn_exp2f(-fabsf(t));
                const float u = 1.0f + e;
                const float r = __builtin_amdgcn_rcpf(u);
                // log2(1 + e) = log2(u) + (e - (u - 1)) / u * log2(e): the rounding of 1 + e put back
                // (exact differences), so small e needs no series and no select
                const float l1 = log2_1p_comp(e, u, r);
                const bool ahead = t * Ws >= 0.0f;
                const float psi = ahead ? e * r : r;             // sigmoid(-sigma (s_win - s_lose))
                const float lg = l1 + (ahead ? 0.0f : fabsf(t)); // log2(1 + exp(-sigma (s_win - s_lose)))
                lacc = __builtin_fmaf(fabsf(Ws), lg, lacc);
                c = -Ws * psi;
            } else if (!kRowWeight) {
                const bool gt = yh > yv, lt = yh < yv;
                float Wp = 1.0f;
                if (KIND == LTR_ARP2) Wp = fabsf(yh - yv);
                const float t = (sh - sv) * c1;
                const float z = gt ? t : -t;
                const float e = __builtin_amdgcn_exp2f(-fabsf(z));
                const float u = 1.0f + e;
                const float r = __builtin_amdgcn_rcpf(u);
                const float psi = (z >= 0.0f) ? e * r : r;
                const float lg = log2_1p_comp(e, u, r) + fmaxf(-z, 0.0f);
                const float Wm = (on & (gt | lt)) ? Wp : 0.0f;
                lacc += Wm * lg;
                c = (gt ? -Wm : Wm) * psi;
            } else {
                const float x = (sh - sv) * c1;
                const bool ok = on & (x == x);                   // NaN score = inert document
                const float e = __builtin_amdgcn_exp2f(-fabsf(x));
                const float u = 1.0f + e;
                const float r = __builtin_amdgcn_rcpf(u);
                const float sneg = (x >= 0.0f) ? e * r : r;
                const float l1 = log2_1p_comp(e, u, r);
                // a_home (l1 + max(-x, 0)) + a_vis (l1 + max(x, 0)): the hinge part goes to ONE of the two
                const float ysum = yh + yv;
                const float both = __builtin_fmaf(ysum, l1, ((x >= 0.0f) ? yv : yh) * fabsf(x));
                lacc += ok ? both : 0.0f;
                c = ok ? (yv - ysum * sneg) : 0.0f;
            }
            gh += c;
            V.gv -= c;
        };
        auto rotate = [&](Vis &V) {
            V.sv = wave_rol1(V.sv); V.gv = wave_rol1(V.gv);
            if (KIND == LTR_NDCG2) { V.Gv = wave_rol1(V.Gv); V.rv = wave_rol1i(V.rv); }
            else V.yv = wave_rol1(V.yv);
        };
        // a full step of a chain (the discount of the NEXT step requested first)
        auto step = [&](Vis &V) {
            float dnext = 0.f;
            if (KIND == LTR_NDCG2) dnext = delta_at(rh, wave_rol1i(V.rv));
            visit(V, false);
            rotate(V);
            V.dcur = dnext;
        };
        auto flush_vis = [&](const Vis &V, int rot) {
            const int fidx = 64 * b + ((lane + rot) & 63);       // the visitor now in this lane
            if (fidx < nb) gw[fidx] += V.gv;
        };

        const int steps = min(jend - j, u1 - u);
        u += steps;
        const int jstop = j + steps;
        // full steps (every lane), then at most one half step (diagonal job, j == 32): the LAST step
        const bool has_half = diag && jstop == 33;
        // (Two visitor chains per lane -- the steps [j, j+n/2) and [j+n/2, jstop) interleaved, two
        // independent dependency chains -- were measured and dropped: correct, but 2-10 % slower in
        // every kernel (C2 fused hinge 10.5 -> 11.2 us, LambdaNDCG2 16.2 -> 16.6, 256 x 1000 hinge
        // loss 49.7 -> 56.2): the second chain's registers and moves cost more than its ILP buys.)
        {
            Vis A;
            load_vis(A, j);
            const int jfull = has_half ? 32 : jstop;
            for (; j < jfull; ++j) step(A);
            if (has_half) { visit(A, true); rotate(A); ++j; }
            if (hvalid) gw[hidx] += gh;
            flush_vis(A, j);
        }
        if (j == jend) {
            if (++b == nt) { ++a; b = a; }
            j = (a == b) ? 1 : 0;
        }
    }
    if (kRowWeight && part == 0)              // the i == j terms: a_i * log2(1 + e^0) = a_i
        for (int k = tid; k < nb; k += T) lacc += q.sy[k].y;
    LTR_SYM_STAMP(1);                                        // steps done, accumulators flushed (wave 0)

    float total;
    if (TW > 0) {
        // every wave parks its sum in its own slot (the upper half of `red`: no reuse hazard with the
        // block sums of prepare_ndcg), ONE barrier publishes the sums and the gradient slices
        const float ws = wave_sum(lacc);
        if (lane == 0) q.red[16 + wl] = ws;
        __syncthreads();
        LTR_SYM_STAMP(2);                                    // barrier passed
        total = 0.f;
#pragma unroll
        for (int i = 0; i < (TW > 0 ? TW : 1); ++i) total += q.red[16 + i];
    } else {
        total = block_sum(lacc, q.red);       // its barriers publish gpart when there are >= 2 waves
        if (T == kWave) __syncthreads();
    }
    if (raw) return total;
    gscale = 1.0f;
    if (KIND == LTR_DCG_HINGE) {
        const float lg = logf(2.0f + total);
        gscale = 1.0f / ((2.0f + total) * lg * lg);
        total = -1.0f / lg;
    } else if (KIND != LTR_HINGE) {
        gscale = sigma / kLn2;
    }
    if (DEFER && (KIND == LTR_NDCG1 || KIND == LTR_NDCG2)) {
        float maxdcg = 0.f;
#pragma unroll
        for (int i = 0; i < (TW > 0 ? TW : 1); ++i) maxdcg += q.red[(TW > 8 ? 32 : 8) + i];
        if (maxdcg == 0.0f) maxdcg = 1.0f;                  // pairwise_lambda.py:227
        const float inv_maxdcg = 1.0f / maxdcg;
        total *= inv_maxdcg;
        gscale *= inv_maxdcg;
    }
    return total;
}

constexpr int kSplitMax = 8;
constexpr int kSplitMinSteps = 16;
__host__ __device__ inline int split_parts_for(int nb, int nsplit, int waves)
{
    // a part should have at least ~16 pair steps per wave to be worth a workgroup (swept 8..96 with the
    // list-length order in place: C4 hinge 34.7 us at 96, 31.7 at 48, 28.4 at 16)
    const int nt = (nb + 63) >> 6;
    const int units = 32 * nt * nt;
    int e = units / (kSplitMinSteps * waves);
    e = e < 1 ? 1 : e;
    return e < nsplit ? e : nsplit;
}


// ---------------------------------------------------------------------------------
// host side: launch-shape heuristic and dispatch
// ---------------------------------------------------------------------------------
// (64 bytes short of the CU's 160 KB: kernels that use sched_query_sampled carry 8 bytes of static
// LDS, and static + dynamic must fit together)
constexpr size_t kLdsBudget = 160 * 1024 - 64;
// Raise a kernel's dynamic-LDS limit above the 64 KiB default once per device (the attribute is
// sticky), so steady-state launches -- including hipGraph capture -- issue no extra API calls.
constexpr int kMaxDevices = 64;
#define LTR_ENSURE_LDS(KERNEL, BYTES)                                                           \
    do {                                                                                        \
        static size_t cfg_[kMaxDevices] = {};                                                   \
        int dev_ = 0;                                                                           \
        (void)hipGetDevice(&dev_);                                                              \
        if ((size_t)(BYTES) > 64 * 1024 && dev_ >= 0 && dev_ < kMaxDevices &&                   \
            (size_t)(BYTES) > cfg_[dev_]) {                                                     \
            hipError_t e_ = hipFuncSetAttribute(reinterpret_cast<const void *>(&KERNEL),        \
                                                hipFuncAttributeMaxDynamicSharedMemorySize,     \
                                                (int)kLdsBudget);                               \
            if (e_ != hipSuccess) return (int)e_;                                               \
            cfg_[dev_] = kLdsBudget;                                                            \
        }                                                                                       \
    } while (0)

inline int device_cu_count()
{
    static int cached[kMaxDevices] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= kMaxDevices) dev = 0;
    if (cached[dev] == 0) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
            v = 256;
        cached[dev] = v;
    }
    return cached[dev];
}

// Number of sample groups for sched_query_sampled, or 0 = plain order: worth it with more than one
// workgroup per CU and up to `max_per_cu` of them (beyond that the order stops mattering).
inline int sched_groups(int B, int max_per_cu)
{
    const int cus = device_cu_count();
    return (B > cus + cus / 8 && (long long)B <= (long long)max_per_cu * cus) ? (B + 63) / 64 : 0;
}

// The loss kernel and the general fused kernel: the pass costs ~0.3 us per launch, which short
// lists do not win back (L = 64: 5.0 -> 5.2 us at B = 1024); lists of 128 need a full chip
// (B >= 4 x #CUs: hinge 7.0 -> 6.7, LambdaNDCG2 15.0 -> 13.2), longer ones always gain (L = 512,
// B = 1024: hinge 37 -> 28 us, logistic 75 -> 55, LambdaNDCG2 148 -> 120; profiles/README.md).
inline int sched_groups_for_lists(int B, int L)
{
    if (L <= 64) return 0;
    if (L < 256 && B < 4 * device_cu_count()) return 0;
    return sched_groups(B, kLossSchedMaxPerCu);
}


inline bool bad_label_dtype(int d) { return d != LTR_LABEL_I64 && d != LTR_LABEL_F32 && d != LTR_LABEL_I32; }

// The run-time loss kind as a template argument: f(std::integral_constant<int, KIND>{}) for each of the
// seven kinds, LTR_ERR_KIND for anything else.
template <class Fn>
int with_kind(int kind, Fn &&f)
{
    switch (kind) {
    case LTR_HINGE: return f(std::integral_constant<int, LTR_HINGE>{});
    case LTR_DCG_HINGE: return f(std::integral_constant<int, LTR_DCG_HINGE>{});
    case LTR_LOGISTIC: return f(std::integral_constant<int, LTR_LOGISTIC>{});
    case LTR_ARP1: return f(std::integral_constant<int, LTR_ARP1>{});
    case LTR_ARP2: return f(std::integral_constant<int, LTR_ARP2>{});
    case LTR_NDCG1: return f(std::integral_constant<int, LTR_NDCG1>{});
    case LTR_NDCG2: return f(std::integral_constant<int, LTR_NDCG2>{});
    default: return LTR_ERR_KIND;
    }
}

// Argument guards shared by the entry points; each returns the first failing code, or LTR_OK.
// A loss kind and a label dtype:
inline int check_kind(int kind, int rel_dtype)
{
    return (kind < LTR_HINGE || kind > LTR_NDCG2 || bad_label_dtype(rel_dtype)) ? LTR_ERR_KIND : LTR_OK;
}
// A (B, L) batch of lists of at most max_len documents:
inline int check_lists(int B, int L, int max_len)
{
    if (B < 0 || L <= 0) return LTR_ERR_SHAPE;
    return L > max_len ? LTR_ERR_LIST_TOO_LONG : LTR_OK;
}

inline unsigned grid_for(size_t items, int block)
{
    size_t g = (items + (size_t)block - 1) / (size_t)block;
    if (g < 1) g = 1;
    if (g > 2048) g = 2048;          // 256 CUs x 8 blocks, grid-stride the rest
    return (unsigned)g;
}

// Per-query partials of the fused Linear steps (ltr_linear.inc, ltr_linear_listwise.inc): row b of a (B, PF) row-major matrix, PF = partial_pitch(F) floats:
// [d loss[b]/dW_0 .. dW_{F-1} | d loss[b]/d bias | zero padding to a multiple of 4].  A query's row is
// ONE contiguous, 16-byte aligned run, so a workgroup stores it with a single coalesced wave-store
// (round 1 kept it column-major in b: 137 scattered 4-byte stores per query, 5.4x write amplification).
__host__ __device__ inline int partial_pitch(int F) { return (F + 4) & ~3; }

// small vector helpers shared by the fused scorer kernels
typedef unsigned int ltr_u32x4 __attribute__((ext_vector_type(4)));
template <int VEC> struct VecT;
template <> struct VecT<4> { using type = float4; };
template <> struct VecT<1> { using type = float; };

__device__ __forceinline__ float vdot(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
// the same dot product as one packed multiply, one packed fma and one add
typedef float ltr_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float vdot_pk(float4 a, float4 b)
{
    ltr_f32x2 lo = {a.x, a.y}, hi = {a.z, a.w}, wlo = {b.x, b.y}, whi = {b.z, b.w};
    ltr_f32x2 pr = lo * wlo;
    pr = __builtin_elementwise_fma(hi, whi, pr);
    return pr.x + pr.y;
}
__device__ __forceinline__ float vdot(float a, float b) { return a * b; }
__device__ __forceinline__ void vfma(float4 &acc, float g, float4 x) { acc.x += g * x.x; acc.y += g * x.y; acc.z += g * x.z; acc.w += g * x.w; }
__device__ __forceinline__ void vfma(float &acc, float g, float x) { acc += g * x; }
__device__ __forceinline__ void vadd(float4 &a, float4 b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
__device__ __forceinline__ void vadd(float &a, float b) { a += b; }
template <typename V> __device__ __forceinline__ V vzero();
template <> __device__ __forceinline__ float4 vzero<float4>() { return make_float4(0.f, 0.f, 0.f, 0.f); }
template <> __device__ __forceinline__ float vzero<float>() { return 0.f; }

// the same on a 16-byte vector of EIGHT bf16 (the Linear scorer on bf16 feature batches: the fused tile of
// ltr_linear_bf16.inc and the streaming layer of ltr_scorer.inc).  A bf16 is the upper half of an fp32, so widening is a
// shift or a mask and exact; the weights and every product and sum stay fp32.
struct LbW8 { float4 a, b; };              // the weights (or a dW accumulator) of one column vector: columns 0-3, 4-7

__device__ __forceinline__ float lb_lo(unsigned v) { return __uint_as_float(v << 16); }
__device__ __forceinline__ float lb_hi(unsigned v) { return __uint_as_float(v & 0xffff0000u); }

__device__ __forceinline__ float lb_dot(ltr_u32x4 v, const LbW8 &w)
{
    float s0 = lb_lo(v.x) * w.a.x, s1 = lb_hi(v.x) * w.a.y;
    s0 = fmaf(lb_lo(v.y), w.a.z, s0); s1 = fmaf(lb_hi(v.y), w.a.w, s1);
    s0 = fmaf(lb_lo(v.z), w.b.x, s0); s1 = fmaf(lb_hi(v.z), w.b.y, s1);
    s0 = fmaf(lb_lo(v.w), w.b.z, s0); s1 = fmaf(lb_hi(v.w), w.b.w, s1);
    return s0 + s1;
}

__device__ __forceinline__ void lb_fma(LbW8 &acc, float g, ltr_u32x4 v)
{
    acc.a.x = fmaf(g, lb_lo(v.x), acc.a.x); acc.a.y = fmaf(g, lb_hi(v.x), acc.a.y);
    acc.a.z = fmaf(g, lb_lo(v.y), acc.a.z); acc.a.w = fmaf(g, lb_hi(v.y), acc.a.w);
    acc.b.x = fmaf(g, lb_lo(v.z), acc.b.x); acc.b.y = fmaf(g, lb_hi(v.z), acc.b.y);
    acc.b.z = fmaf(g, lb_lo(v.w), acc.b.z); acc.b.w = fmaf(g, lb_hi(v.w), acc.b.w);
}

__device__ __forceinline__ LbW8 lb_zero()
{
    LbW8 z;
    z.a = make_float4(0.f, 0.f, 0.f, 0.f);
    z.b = z.a;
    return z;
}

// what every bf16 Linear entry point takes: a row starts on 16 bytes, at most 128 column vectors, rows indexed by an int
constexpr int kLbMaxF = 1024;
inline bool lb_shape_bad(int B, int L, int F)
{
    return B < 0 || L <= 0 || F <= 0 || F % 8 != 0 || F > kLbMaxF || (long long)B * L > 0x7fffffffLL;
}

}  // namespace
