// ltr_mlp.inc -- fused ReLU-MLP scorer (F -> H1 -> H2 -> 1) + pairwise loss + backward on MFMA.
// Included by ltr_mlp.hip (uses ltr_common.inc's LDS carve, label staging and symmetric pair pass); this file is the
// 8-wave kernel and its launchers -- the reduction is in ltr_mlp_reduce.inc, the step's host side in ltr_mlp_step.inc.
//
// SURVEY.md section 8 f-2: the documented training step
//     loss_fn(model(xs), ys, n).mean().backward()          docs/source/getting-started.rst:40-101
// with `model` = Linear(F,50) / ReLU / Linear(50,10) / ReLU / Linear(10,1).  One launch computes the
// per-query losses and the gradient of sum_b weight[b]*loss[b] w.r.t. all six parameter tensors.
//
// Mapping.  A persistent workgroup of 8 waves (two per SIMD) takes a list of queries that an
// in-kernel counting sort on n[] deals out in snake order (deterministic load balance).
// Documents are cut into 16-row subtiles; wave w owns subtile w (L <= 128) and carries it through
// the whole network with activations TRANSPOSED (features x documents), so that the D fragment of
// one v_mfma_f32_16x16x4_f32 (lane: document = lane&15, feature = 4*(lane>>4)+reg) is directly
// the B operand of the next layer -- no LDS round trip inside the forward chain or the dH chain:
//     H1^T = relu(W1 . X^T + b1)      A = W1 rows from LDS (b128), B = X rows from HBM (b128),
//                                     loaded ONCE per query and kept in registers
//     H2^T = relu(W2 . H1^T + b2)     A = W2 from LDS,             B = H1^T fragments
//     s    = w3 . H2^T + b3           4 FMAs + two cross-row adds
//     (barrier) symmetric pair pass over the query's scores -> d loss / d s   (barrier)
//     dH2^T = w3 (x) ds . [H2 > 0]    registers
//     dH1^T = W2^T . dH2^T . [H1 > 0] A = W2^T from LDS,           B = dH2^T fragments
// Weight gradients contract over documents, which the fragments hold on lane&15:
//     dW2 += dH2^T . H1               A = dH2, B = H1: this wave's own rows of LDS
//     dW1 += dH1^T . X                cut by FEATURES: the waves drop their X fragments of two
//                                     16-feature chunks into a shared LDS image, then each wave
//                                     multiplies one chunk by one 16-row tile of dH1 over all
//                                     documents; chunk registers then take the next query's X
// dW1 tiles are disjoint between the waves and live in registers across all the queries of the
// workgroup; the small sums fold over the waves in LDS; one partial vector per workgroup is
// written at the end and mlp_reduce_kernel (ltr_mlp_reduce.inc) adds the partials in a fixed order (deterministic).
// f32 MFMA is an exact k-ordered fma chain (no reduced precision): dtype stays "f32".
// DESIGN.md section 10 has the measurements and the history of this kernel.
#pragma once
#include <type_traits>

#include "ltr_listwise.h"
#include "ltr_mlp_lambdarank.h"

typedef float mlp_f4 __attribute__((ext_vector_type(4)));

constexpr int kMlpThreads = 512;      // 8 waves = two per SIMD: one wave's MFMA stream covers the
constexpr int kMlpWaves = 8;          // other's LDS waits, barriers and VALU phases
constexpr int kMlpMaxLen = 128;      // one subtile of 16 documents per wave
constexpr int kMlpH1 = 64;           // hidden-1 rows the tiles cover (H1 <= 64)
constexpr int kMlpH2 = 16;           // hidden-2 rows (H2 <= 16)
constexpr int kMlpHS = 72;           // LDS row stride of the H1 / dH1 block (floats)
constexpr int kMlpDS = 16;           // LDS row stride of the dH2 block
constexpr int kMlpW2S = 68;          // LDS row stride of W2   [16][68]
constexpr int kMlpW2TS = 20;         // LDS row stride of W2^T [64][20]
constexpr int kMlpSched = 1024;       // queries per scheduling block
constexpr int kMlpListCap = 256;      // most queries one workgroup's list holds (else round-robin)
constexpr int kMlpTS = 20;           // row stride of the X transpose images [128][20]

struct MlpParams {
    const float *X, *W1, *b1, *W2, *b2, *W3, *b3;
    const void *rel;
    const int64_t *n;
    const float *grad_out;
    float *loss, *scores_out, *part;
    int B, L, F, H1, H2;
    float sigma;
    int rel_dtype;
    int P;                           // parameter count = length of one partial vector
    int pitch;                       // floats between consecutive partial vectors (P rounded up to 4)
    int fwd_only;                    // 1: scores only (evaluation) -- no pair pass, no backward
    MlpListwiseArgs lw{};            // KIND = LTR_MLP_LISTNET / LTR_MLP_LISTMLE, and LTR_MLP_LAMBDARANK's k (ltr_mlp_listwise.inc)
};

__host__ __device__ inline int mlp_param_count(int F, int H1, int H2)
{
    return H1 * F + H1 + H2 * H1 + 2 * H2 + 1;
}

// LDS floats ahead of the per-query block of the loss code
__host__ __device__ inline int mlp_bucket(int F)
{
    const int ntile = (F + 15) >> 4;
    return ntile <= 3 ? 3 : (ntile <= 5 ? 5 : (ntile <= 9 ? 9 : 14));
}

__host__ __device__ inline size_t mlp_static_floats(int F)
{
    const size_t FS = (size_t)16 * mlp_bucket(F) + 4;
    return kMlpH1 * FS + (size_t)kMlpMaxLen * kMlpHS + kMlpH2 * kMlpW2S + kMlpH1 * kMlpW2TS +
           (size_t)kMlpMaxLen * kMlpDS + kMlpH1 + 2 * kMlpH2 + kMlpMaxLen +
           (size_t)4 * kMlpMaxLen * kMlpTS + kMlpListCap + 4;
}

__host__ __device__ inline size_t mlp_lds_bytes(int kind, int F)
{
    return ((mlp_static_floats(F) * 4 + 15) & ~(size_t)15) + loss_lds_bytes(kind, kMlpMaxLen, kMlpWaves);
}

__device__ __forceinline__ mlp_f4 mfma16(float a, float b, mlp_f4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// (lds_barrier(), ltr_common.inc: __syncthreads() would expose the HBM latency of the next query's feature prefetch at every
// barrier of the dW1 loop)

// Sum over the 16 lanes of a DPP row; every lane of the row gets the result.
__device__ __forceinline__ float row16_sum(float v)
{
    v = quad_sum(v);
    v += dpp_move<0x141, 0xF>(v);
    v += dpp_move<0x140, 0xF>(v);
    return v;
}

// -DLTR_MLP_TRACE: thread 0 of every workgroup accumulates the cycles spent per phase into
// ((long long *)scores_out)[16 * blockIdx + slot] (tuning only; scores are not written then).
#ifdef LTR_MLP_TRACE
#define MLP_STAMP(slot) do { if (tid == 0) { const long long now_ = (long long)__builtin_readcyclecounter(); \
    reinterpret_cast<long long *>(p.scores_out)[16 * (size_t)blockIdx.x + (slot)] += now_ - last_; last_ = now_; } } while (0)
#else
#define MLP_STAMP(slot) do { } while (0)
#endif

// ---- which queries a workgroup takes.  The cost of a query grows with n[b], and with a handful
// of queries per workgroup a round-robin split leaves the slowest workgroup ~30 % above the mean
// on ragged batches.  Instead every block of kMlpSched queries is ordered by (n descending, index
// ascending) and dealt out in snake order (position i*G + w, direction alternating with i).  A
// pure function of n[]: the assignment, and with it every partial sum, is identical from run to
// run.  A workgroup only needs the queries at ITS positions of that order (`per` of them per
// block, 2-4 in practice), so nothing is sorted: a histogram of n (LDS atomics) and its suffix sums
// give, for a position, the n value v whose run contains it and the rank k inside the run; the
// k-th query (by index) with n == v comes from ballots (matches per wave and per stride, through
// LDS, + the popcount below the lane); every thread holds the queries tid + e*T.  Three barriers per
// block of 1024 queries (per-wave histograms, the suffix sums in every wave's registers): at the
// start of a kernel a barrier round costs ~1 k cycles (waves start apart), so a bisection over v
// with a ballot count per step -- no
// histogram, but 10 barriers -- was slower (12 k cycles against 7 k), and so was the whole selection
// by ONE wave without any barrier (16 queries per lane: 21 k); the first version, a full
// ranking with one bit mask per n value, took 14 k cycles = 10 % of the kernel.
// Returns the number of queries written to qlist[], or -1 = no list (query i of this workgroup is
// blockIdx + i*gridDim: one query per workgroup, more than the list holds, or `plain`).
// `scratch`: LDS, (T/64)*(MAXN+4) + 2*(kMlpSched/64) ints; qlist: kMlpListCap + 4 ints.  Ends with a barrier.
template <int T, int MAXN = kMlpMaxLen>
__device__ __forceinline__ int mlp_schedule(const int64_t *__restrict__ n, int B, int L, int *qlist,
                                            unsigned *scratch, bool plain)
{
    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const int G = (int)gridDim.x;
    const int per = (kMlpSched + G - 1) / G;                         // list slots per block
    const int nblk = (B + kMlpSched - 1) / kMlpSched;
    if (plain || B <= G || nblk * per > kMlpListCap) {
        int nq = -1;
        if (B <= G) {
            if (tid == 0) { qlist[0] = (int)blockIdx.x; }
            nq = ((int)blockIdx.x < B) ? 1 : 0;
        }
        __syncthreads();
        return nq;
    }
    if ((long long)B <= 4LL * G) {
        // A few queries per workgroup (the named batch: two): the order only has to balance the workgroups,
        // so the approximate, one-wave selection of the fused-linear kernels does (sched_query_sampled: 64
        // sampled lengths per position, ballots only, one barrier) -- ~1 k cycles per position against the
        // ~8 k of the exact selection below.  Position i of workgroup g: i * G + g, every other round in
        // reverse (long lists meet short ones).
        const int groups = (B + 63) / 64;
        int total = 0;
        for (int i = 0; i * G < B; ++i) {
            const int pos = i * G + ((i & 1) == 0 ? (int)blockIdx.x : G - 1 - (int)blockIdx.x);
            if (pos < B) {                                             // uniform
                int nb_unused;
                const int b = sched_query_sampled(n, B, L, groups, tid, nb_unused, pos);
                if (tid == 0) qlist[total] = b;
                ++total;
                __syncthreads();                                       // (the selection's LDS words are reused)
            }
        }
        __syncthreads();
        return total;
    }
    constexpr int E = kMlpSched / T;                                 // queries per thread: tid + e*T
    constexpr int NW = T / 64;
    constexpr int PC = 2;                                            // positions looked up per round
    constexpr int NBIN = MAXN + 1;                                   // n = 0 .. MAXN (a multiple of 64)
    constexpr int BPL = MAXN / 64;                                   // bins per lane of the scan
    constexpr int HP = NBIN + 3;                                     // row pitch of the per-wave histograms
    int *hist = reinterpret_cast<int *>(scratch);                    // [NW][HP] one histogram per wave
    int *wtot = hist + NW * HP;                                      // [PC][E][NW] matches per wave
    int total = 0;                                                   // (uniform) slots filled so far
    for (int sblk = 0; sblk < nblk; ++sblk) {
        const int base = sblk * kMlpSched;
        const int cnt = min(kMlpSched, B - base);
        int myv[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int j = tid + e * T;
            myv[e] = (j < cnt) ? clamp_n(n[base + j], L) : -1;
        }
        // every wave counts into its OWN histogram row: zeroing and adding are then ordered by the
        // wave's own LDS queue, no barrier in between (three barriers per block instead of five)
        int *myh = hist + wv * HP;
        for (int i = lane; i < NBIN; i += 64) myh[i] = 0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            // the lanes that hold the same value as the first lane count themselves with ONE add
            // (a batch of full lists would otherwise send every atomic to one address: 11 k
            // cycles); the others add one by one (ragged batches: ~8 queries per value)
            const int v0 = __builtin_amdgcn_readfirstlane(myv[e]);
            const unsigned long long m0 = __ballot(myv[e] == v0);
            if (lane == 0 && v0 >= 0) atomicAdd(&myh[v0], __popcll(m0));
            if (myv[e] >= 0 && myv[e] != v0) atomicAdd(&myh[myv[e]], 1);
        }
        __syncthreads();
        // start[v] = number of queries with n > v, in registers: lane l of EVERY wave holds the bins
        // BPL*l .. BPL*l + BPL-1 (suffix scan over the lanes' groups)
        int st[BPL], sttop = 0;
        {
            int hb[BPL], sum = 0;
#pragma unroll
            for (int k = 0; k < BPL; ++k) {
                hb[k] = 0;
#pragma unroll
                for (int ww = 0; ww < NW; ++ww) hb[k] += hist[ww * HP + BPL * lane + k];
                sum += hb[k];
            }
            int top = 0;
#pragma unroll
            for (int ww = 0; ww < NW; ++ww) top += hist[ww * HP + MAXN];
            // inclusive prefix sum over the lanes on the DPP path (row shifts, then the row broadcasts;
            // __shfl_* would be six dependent ds_bpermute round trips), suffix = total - prefix + own
            int x = sum;
            x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, false);      // row_shr:1
            x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, false);      // row_shr:2
            x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, false);      // row_shr:4
            x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, false);      // row_shr:8
            x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false);      // row_bcast:15 -> rows 1, 3
            x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false);      // row_bcast:31 -> rows 2, 3
            const int all = __builtin_amdgcn_readlane(x, 63);
            int above = all - x + top;          // queries in the bins behind this lane's group
#pragma unroll
            for (int k = BPL - 1; k >= 0; --k) {
                st[k] = above;
                above += hb[k];
            }
            (void)sttop;                        // start[MAXN] = 0: nothing is longer than MAXN
        }
        for (int i0 = 0; i0 < per; i0 += PC) {
            int vsel[PC], ksel[PC];
            unsigned long long bal[PC][E];
#pragma unroll
            for (int c = 0; c < PC; ++c) {
                const int i = i0 + c;
                const bool fwd = ((i + sblk) & 1) == 0;
                const int pos = i * G + (fwd ? (int)blockIdx.x : G - 1 - (int)blockIdx.x);
                vsel[c] = -2;                                  // (never equal to a query's n or the -1 filler)
                ksel[c] = 0;
                if (i < per && pos < cnt) {                    // uniform
                    // start[] falls as v grows: the run that contains `pos` belongs to the smallest
                    // v with start[v] <= pos = the number of v with start[v] > pos (a ballot per
                    // 64 values, every wave for itself)
                    int v = 0;
#pragma unroll
                    for (int k = 0; k < BPL; ++k) v += __popcll(__ballot(st[k] > pos));
                    vsel[c] = v;
                    // start[v]: bin v sits in lane v / BPL, slot v % BPL (v == MAXN: 0)
                    int sv = 0;
                    const int vl = __builtin_amdgcn_readfirstlane((v < MAXN ? v : 0) / BPL);
#pragma unroll
                    for (int k = 0; k < BPL; ++k) {
                        const int got = __builtin_amdgcn_readlane(st[k], vl);
                        if (v < MAXN && (v % BPL) == k) sv = got;
                    }
                    ksel[c] = pos - sv;
                }
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    bal[c][e] = __ballot(myv[e] == vsel[c]);
                    if (lane == 0) wtot[(c * E + e) * NW + wv] = __popcll(bal[c][e]);
                }
            }
            __syncthreads();
#pragma unroll
            for (int c = 0; c < PC; ++c) {
                if (vsel[c] < 0) continue;                     // uniform
                int before = 0;                                // matches in front of this wave's (e, wave) cell
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    int cell = 0;
#pragma unroll
                    for (int k = 0; k < NW; ++k) {
                        const int t = wtot[(c * E + e) * NW + k];
                        before += (k < wv) ? t : 0;
                        cell += (k >= wv) ? t : 0;
                    }
                    if (myv[e] == vsel[c]) {
                        const int rank = before + __popcll(bal[c][e] & ((1ull << lane) - 1ull));
                        if (rank == ksel[c]) qlist[total + c] = base + tid + e * T;
                    }
                    before += cell;
                }
            }
            // (slots are filled densely: positions past the end of a block are the last ones of it)
#pragma unroll
            for (int c = 0; c < PC; ++c) total += (vsel[c] >= 0) ? 1 : 0;
            __syncthreads();
        }
    }
    return total;
}

template <int KIND, int NT, bool FWD = false>
__global__ void __launch_bounds__(kMlpThreads)
mlp_pairwise_kernel(MlpParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    constexpr int T = kMlpThreads;
#ifdef LTR_MLP_TRACE
    long long last_ = (long long)__builtin_readcyclecounter();
#endif
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15;
    const int g = lane >> 4;
    const int L = p.L, F = p.F, H1 = p.H1, H2 = p.H2;
    constexpr int FS = 16 * NT + 4;                 // LDS pitch of W1 (zero padded to the bucket)
    constexpr int Lt = kMlpMaxLen;
    constexpr bool kListwise = KIND == LTR_MLP_LISTNET || KIND == LTR_MLP_LISTMLE;   // sy holds (label, score)
    constexpr bool kLambdaRank = KIND == LTR_MLP_LAMBDARANK;                         // (score, label), its own slot

    float *W1s = reinterpret_cast<float *>(smem);                 // [64][FS]
    float *H1s = W1s + (size_t)kMlpH1 * FS;                       // [128][72]  H1, later dH1
    float *W2s = H1s + (size_t)kMlpMaxLen * kMlpHS;               // [16][68]
    float *W2Ts = W2s + kMlpH2 * kMlpW2S;                         // [64][20]
    float *dH2s = W2Ts + kMlpH1 * kMlpW2TS;                       // [128][16]
    float *b1s = dH2s + (size_t)kMlpMaxLen * kMlpDS;              // [64]
    float *b2s = b1s + kMlpH1;                                    // [16]
    float *w3s = b2s + kMlpH2;                                    // [16]
    float *gfin = w3s + kMlpH2;                                   // [128]
    float *tps = gfin + kMlpMaxLen;                               // [2 buffers][2 chunks][128][20]
    int *qlist = reinterpret_cast<int *>(tps + 4 * kMlpMaxLen * kMlpTS);   // [kMlpListCap + 4] this workgroup's queries
    const size_t qoff = (mlp_static_floats(F) * 4 + 15) & ~(size_t)15;
    const QueryLds q = carve_query_lds<KIND>(smem + qoff, Lt, kMlpWaves);

    const mlp_f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    // ---- accumulators that live across queries ----
    // dW1 is cut by FEATURES for its GEMM (see below): round r gives this wave the 16-feature
    // chunk 2r + (w>>2) and the 16 hidden rows of tile (w&3); with an odd chunk count the last
    // chunk goes to waves 0..3 (one per SIMD), tile w.
    constexpr int NR = NT / 2;
    mlp_f4 accU[NR > 0 ? NR : 1];        // [round]: dW1[j1 = 16*(w&3)+4g+i][f = 16*(2r+(w>>2))+c16]
    mlp_f4 accL = zero4;                 // odd NT, waves 0..3: dW1[j1 = 16w+4g+i][f = 16*(NT-1)+c16]
    mlp_f4 accW2[4];                     // dW2[j2 = 4g+i][j1 = 16T+c16]
    mlp_f4 accB1[4];                     // db1[j1 = 16t+4g+i], partial over this lane's documents
    mlp_f4 accB2 = zero4, accW3 = zero4; // db2 / dW3 [j2 = 4g+i], same
    float accB3 = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        accW2[t] = zero4;
        accB1[t] = zero4;
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) accU[r] = zero4;

    // X fragments of this wave's subtile (documents 16w .. 16w+15), the whole row block: lane
    // (document c16, features 16c+4g .. +3) of chunk c.  They are the B operands of layer 1 and,
    // sent through a shared LDS transpose image, of the dW1 GEMM -- X crosses HBM once.  Chunk c
    // of the NEXT query is requested as soon as the dW1 loop has put chunk c of the current one
    // into LDS, so the HBM latency hides behind the remaining MFMA work.  Lanes outside the query
    // (document >= n, feature >= F) load a clamped, always valid address and are zeroed by a
    // select at the use (a per-lane branch around a load would fence the prefetch).
    mlp_f4 xa[NT];
    const int rowA = 16 * w + c16;
    auto load_chunk = [&](const float *Xn, int nq, int c) {
        const int f0 = 16 * c + 4 * g;
        const int fc = f0 < F ? f0 : 0;
        xa[c] = *reinterpret_cast<const mlp_f4 *>(Xn + (size_t)(rowA < nq ? rowA : 0) * F + fc);
    };
    auto masked = [&](mlp_f4 v, bool ok) {
        mlp_f4 r;
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = ok ? v[i] : 0.f;
        return r;
    };
    // W1 on its way to LDS: 16-byte units, all loads of a thread issued here, the LDS stores
    // follow after the scheduling block below (whose own latency they overlap)
    constexpr int FS4 = FS >> 2;
    constexpr int KW = (kMlpH1 * (4 * NT + 1) + T - 1) / T;
    mlp_f4 stage[KW];
    {
        const int F4 = F >> 2;
#pragma unroll
        for (int k = 0; k < KW; ++k) {
            const int i = tid + k * T;
            const int j = i / FS4, f4 = i - j * FS4;
            const bool ok = i < kMlpH1 * FS4 && j < H1 && f4 < F4;
            stage[k] = masked(*reinterpret_cast<const mlp_f4 *>(p.W1 + (ok ? (size_t)j * F + 4 * f4 : 0)), ok);
        }
    }

    // the small tensors the same way (W2 twice: row-major and transposed image)
    constexpr int KW2 = (kMlpH1 * kMlpW2TS + T - 1) / T;      // >= ceil(kMlpH2 * kMlpW2S / T) too
    float w2a[KW2], w2b[KW2], small[3];
#pragma unroll
    for (int k = 0; k < KW2; ++k) {
        const int i = tid + k * T;
        const int ka = i / kMlpW2S, ja = i - ka * kMlpW2S;     // W2s[ka][ja]
        const bool oka = i < kMlpH2 * kMlpW2S && ka < H2 && ja < H1;
        const float va = p.W2[oka ? (size_t)ka * H1 + ja : 0];
        w2a[k] = oka ? va : 0.f;
        const int jb = i / kMlpW2TS, kb = i - jb * kMlpW2TS;   // W2Ts[jb][kb]
        const bool okb = i < kMlpH1 * kMlpW2TS && kb < H2 && jb < H1;
        const float vb = p.W2[okb ? (size_t)kb * H1 + jb : 0];
        w2b[k] = okb ? vb : 0.f;
    }
    {
        const float v1 = p.b1[tid < H1 ? tid : 0], v2 = p.b2[tid < H2 ? tid : 0], v3 = p.W3[tid < H2 ? tid : 0];
        small[0] = tid < H1 ? v1 : 0.f;
        small[1] = tid < H2 ? v2 : 0.f;
        small[2] = tid < H2 ? v3 : 0.f;
    }
    const float b3 = p.b3[0];

    // ---- which queries this workgroup takes (mlp_schedule; masks borrow the H1 block, which the
    // barriers of the weight staging below separate from its first use) ----
    const int G = (int)gridDim.x;
    const int nq = mlp_schedule<T>(p.n, p.B, L, qlist, reinterpret_cast<unsigned *>(H1s), FWD);
    MLP_STAMP(13);                              // (sched)
    auto query_at = [&](int qi) { return nq < 0 ? (int)blockIdx.x + qi * G : qlist[qi]; };
    const int nqueries = nq < 0 ? (p.B - (int)blockIdx.x + G - 1) / G : nq;

    float ynext = 0.f;                             // label of document `tid` of the next query
    int nb_next = 0;
    if (nqueries > 0) {
        const int b0 = query_at(0);
        nb_next = clamp_n(p.n[b0], L);
        const float *Xn = p.X + (size_t)b0 * L * (size_t)F;
#pragma unroll
        for (int c = 0; c < NT; ++c) load_chunk(Xn, nb_next, c);
        if (tid < L) ynext = load_label(p.rel, p.rel_dtype, (size_t)b0 * L + tid);
    }

    // ---- weights -> LDS, zero padded to the tile shapes (once per workgroup); the first query's
    // features and labels are already in flight ----
#pragma unroll
    for (int k = 0; k < KW; ++k) {
        const int i = tid + k * T;
        if (i < kMlpH1 * FS4) reinterpret_cast<mlp_f4 *>(W1s)[i] = stage[k];
    }
#pragma unroll
    for (int k = 0; k < KW2; ++k) {
        const int i = tid + k * T;
        if (i < kMlpH2 * kMlpW2S) W2s[i] = w2a[k];
        if (i < kMlpH1 * kMlpW2TS) W2Ts[i] = w2b[k];
    }
    if (tid < kMlpH1) b1s[tid] = small[0];
    if (tid < kMlpH2) {
        b2s[tid] = small[1];
        w3s[tid] = small[2];
    }
    __syncthreads();
    const mlp_f4 w3v = *reinterpret_cast<const mlp_f4 *>(w3s + 4 * g);

    MLP_STAMP(0);                                  // scheduling + weights staged

    for (int qi = 0; qi < nqueries; ++qi) {
        const int b = __builtin_amdgcn_readfirstlane(query_at(qi));
        const int nb = __builtin_amdgcn_readfirstlane(nb_next);
        const size_t row0 = (size_t)b * L;
        if (tid < nb) { if (kListwise) q.sy[tid].x = ynext; else q.sy[tid].y = ynext; }
        if (KIND == LTR_NDCG1 || KIND == LTR_NDCG2)
            for (int m = tid; m < 2 * Lt; m += T) q.rank_s[m] = 0;
        const bool on = __builtin_amdgcn_readfirstlane(16 * w < nb);    // this wave has documents
        const bool vA = rowA < nb;
        const bool more = qi + 1 < nqueries;       // the query after this one (if any)
        const int bn = __builtin_amdgcn_readfirstlane(more ? query_at(qi + 1) : b);
        if (more) nb_next = clamp_n(p.n[bn], L);

        MLP_STAMP(1);                              // labels staged
        // ---- layer 1: H1^T = relu(W1 . X^T + b1), a straight-line MFMA stream ----
        mlp_f4 h1[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) h1[t] = *reinterpret_cast<const mlp_f4 *>(b1s + 16 * t + 4 * g);
        if (on) {
#pragma unroll
            for (int c = 0; c < NT; ++c) {
                const int f0 = 16 * c + 4 * g;
                mlp_f4 wa[4];
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    wa[t] = *reinterpret_cast<const mlp_f4 *>(W1s + (size_t)(16 * t + c16) * FS + f0);
                const mlp_f4 va = masked(xa[c], f0 < F && vA);
#pragma unroll
                for (int s = 0; s < 4; ++s) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) h1[t] = mfma16(wa[t][s], va[s], h1[t]);
                }
            }
        }
        MLP_STAMP(2);                              // layer 1 MFMAs
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int i = 0; i < 4; ++i) h1[t][i] = fmaxf(h1[t][i], 0.f);
            if (!FWD) *reinterpret_cast<mlp_f4 *>(H1s + (size_t)rowA * kMlpHS + 16 * t + 4 * g) = h1[t];
        }

        // ---- layer 2: H2^T = relu(W2 . H1^T + b2); two chains hide the MFMA latency ----
        mlp_f4 h2 = *reinterpret_cast<const mlp_f4 *>(b2s + 4 * g);
        {
            mlp_f4 h2b = zero4;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const mlp_f4 a = *reinterpret_cast<const mlp_f4 *>(W2s + c16 * kMlpW2S + 16 * t + 4 * g);
                h2 = mfma16(a[0], h1[t][0], h2);
                h2b = mfma16(a[1], h1[t][1], h2b);
                h2 = mfma16(a[2], h1[t][2], h2);
                h2b = mfma16(a[3], h1[t][3], h2b);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) h2[i] = fmaxf(h2[i] + h2b[i], 0.f);
        }
        // ---- layer 3 (one output): s = w3 . H2^T + b3 ----
        {
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) s = __builtin_fmaf(w3v[i], h2[i], s);
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 32);
            s += b3;
            if (g == 0 && rowA < nb) {
                if (kListwise) q.sy[rowA].y = s; else q.sy[rowA].x = s;
#ifndef LTR_MLP_TRACE
                if (p.scores_out) p.scores_out[row0 + rowA] = s;
#endif
            }
#ifndef LTR_MLP_TRACE
            if (FWD && g == 0 && rowA >= nb && rowA < L) p.scores_out[row0 + rowA] = 0.f;
#endif
        }
        if (FWD) {
            // evaluation: nothing else to do for this query; its fragment registers are free, so
            // the next query's features are requested right away (uniform branch, no barrier:
            // the only LDS written per query here is this wave's own H1 rows)
            if (more) {
                const float *Xn = p.X + (size_t)bn * L * (size_t)F;
#pragma unroll
                for (int c = 0; c < NT; ++c) load_chunk(Xn, nb_next, c);
            }
            continue;
        }
        __syncthreads();
        MLP_STAMP(3);                              // layers 2, 3 + barrier

        // ---- the loss slot over the whole query: the pair pass, or the listwise row (ltr_mlp_listwise.inc) ----
        if constexpr (kListwise) {
            mlp_listwise_slot<KIND, T, Lt>(smem + qoff, p.lw, nb, p.grad_out ? p.grad_out[b] : 1.0f / (float)p.B,
                                           p.loss + b, gfin);
        } else if constexpr (kLambdaRank) {
            mlp_lambdarank_slot<T, Lt>(smem + qoff, p.lw.k, p.sigma, nb, p.grad_out ? p.grad_out[b] : 1.0f / (float)p.B,
                                       p.loss + b, gfin);
        } else {
            float gscale;
            if (KIND == LTR_NDCG1 || KIND == LTR_NDCG2) {
                constexpr int owners = 128;
                constexpr int ms = T / owners;
                const int mlen = (nb + ms - 1) / ms;
                const int m0 = __builtin_amdgcn_readfirstlane(min(nb, (tid / owners) * mlen));
                const int m1 = __builtin_amdgcn_readfirstlane(min(nb, m0 + mlen));
                prepare_ndcg<KIND, 1>(q, nb, owners, tid % owners, m0, m1, ms > 1);
            }
            const float total = pairwise_core_sym<KIND, kMlpWaves>(q, nb, Lt, p.sigma, gscale);
            if (tid == 0) p.loss[b] = total;
            const float weight = (p.grad_out ? p.grad_out[b] : 1.0f / (float)p.B) * gscale;
            for (int k = tid; k < Lt; k += T) {
                float gk = 0.f;
                if (k < nb) {
#pragma unroll
                    for (int s = 0; s < kMlpWaves; ++s) gk += q.gpart[(size_t)s * Lt + k];
                }
                gfin[k] = gk * weight;
            }
        }
        __syncthreads();
        MLP_STAMP(4);                              // pair pass

        // ---- backward through layers 3 and 2 (registers) ----
        mlp_f4 dh2;
        {
            const float ds = gfin[rowA];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                accW3[i] = __builtin_fmaf(ds, h2[i], accW3[i]);
                dh2[i] = (h2[i] > 0.f) ? ds * w3v[i] : 0.f;
                accB2[i] += dh2[i];
            }
            if (g == 0) accB3 += ds;
            *reinterpret_cast<mlp_f4 *>(dH2s + (size_t)rowA * kMlpDS + 4 * g) = dh2;
        }
        __syncthreads();

        // ---- dW2 += dH2^T . H1 over this wave's documents ----
        if (on) {
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                const int rk = 16 * w + 4 * st + g;
                const float a = dH2s[(size_t)rk * kMlpDS + c16];
#pragma unroll
                for (int tt = 0; tt < 4; ++tt)
                    accW2[tt] = mfma16(a, H1s[(size_t)rk * kMlpHS + 16 * tt + c16], accW2[tt]);
            }
        }
        // ---- dH1^T = (W2^T . dH2^T) . [H1 > 0] ----
        mlp_f4 dh1[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            dh1[t] = zero4;
            const mlp_f4 a = *reinterpret_cast<const mlp_f4 *>(W2Ts + (16 * t + c16) * kMlpW2TS + 4 * g);
#pragma unroll
            for (int i = 0; i < 4; ++i) dh1[t] = mfma16(a[i], dh2[i], dh1[t]);
        }
        __syncthreads();                          // every wave is done reading H1s
        MLP_STAMP(5);                              // dH2, dW2, dH1 MFMAs
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            // relu mask from the H1 copy in LDS (this lane's own float4, written above), which
            // frees the layer-1 fragments during the pair pass
            float *hA = H1s + (size_t)rowA * kMlpHS + 16 * t + 4 * g;
            const mlp_f4 mA = *reinterpret_cast<const mlp_f4 *>(hA);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                dh1[t][i] = (mA[i] > 0.f) ? dh1[t][i] : 0.f;
                accB1[t][i] += dh1[t][i];
            }
            *reinterpret_cast<mlp_f4 *>(hA) = dh1[t];
        }
        __syncthreads();

        MLP_STAMP(6);                              // dH1 -> LDS
        // ---- dW1 += dH1^T . X.  This GEMM contracts over the documents, so it is cut by
        // features instead of by documents: every wave drops its X fragments of two 16-feature
        // chunks into a shared LDS image [chunk][document][20] (written as (document, 4
        // features), read as (feature c16, document 4s+g)), and after one barrier each wave
        // multiplies ONE chunk by one 16-row tile of dH1 (A operand, LDS) over all documents.  The
        // dW1 accumulators are therefore disjoint between the waves (no fold).  The image is
        // double-buffered: the next round is filled before this round's MFMAs, and a chunk's
        // registers take the next query's features as soon as it is in LDS.
        {
            // the next query's label first: it is then ahead of the feature loads in the
            // in-order vmcnt queue and the label staging at the loop top does not wait for them
            if (more && tid < L) ynext = load_label(p.rel, p.rel_dtype, (size_t)bn * L + tid);
            const float *Xn = p.X + (size_t)(more ? bn : b) * L * (size_t)F;
            constexpr int CH = kMlpMaxLen * kMlpTS;           // floats per chunk image
            const int ksteps = (nb + 3) >> 2;                  // 4-document k-steps
            const int kgroups = (ksteps + 3) >> 2;             // groups of 4 k-steps (16 documents)
            const int cw = w >> 2, mw = w & 3;
            auto put = [&](int c, float *img) {
                const bool fv = 16 * c + 4 * g < F;
                *reinterpret_cast<mlp_f4 *>(img + rowA * kMlpTS + 4 * g) = masked(xa[c], fv && vA);
                if (more) load_chunk(Xn, nb_next, c);
            };
            // groups of 4 k-steps on two accumulator chains, operands of the next group requested
            // before the MFMAs of this one (documents past n contribute exact zeros, so the last
            // group needs no guard)
            // A operand: this wave multiplies the SAME 16-row tile of dH1 (tile w & 3) in every
            // round and in the odd last chunk, so its 32 k-steps are read from LDS once per query
            // into registers (NT <= 9; the widest bucket has no registers to spare) -- that halves
            // the LDS reads of the loop, which run at the LDS bandwidth limit otherwise
            // (2 reads per 32-cycle MFMA x 8 waves = 128 B/clk).
            constexpr bool kRegA = (NT <= 9);
            float afr[kRegA ? 32 : 1];
            if (kRegA) {
                const float *asrc = H1s + 16 * mw + c16;
#pragma unroll
                for (int st = 0; st < 32; ++st)
                    afr[st] = (st < ksteps) ? asrc[(4 * st + g) * kMlpHS] : 0.f;
            }
            auto gemm_unit = [&](const float *bsrc, const float *asrc, mlp_f4 acc) {
                mlp_f4 e = acc, o = zero4;
                if (kRegA) {
                    // groups of 4 k-steps; B values of the next group requested before the MFMAs
                    float bx[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) bx[k] = bsrc[(4 * k + g) * kMlpTS];
#pragma unroll
                    for (int s4 = 0; s4 < 8; ++s4) {
                        if (s4 < kgroups) {                    // uniform
                            float nbx[4];
                            const int base = 16 * (s4 + 1 < kgroups ? s4 + 1 : s4) + g;
#pragma unroll
                            for (int k = 0; k < 4; ++k) nbx[k] = bsrc[(base + 4 * k) * kMlpTS];
                            e = mfma16(afr[4 * s4 + 0], bx[0], e);
                            o = mfma16(afr[4 * s4 + 1], bx[1], o);
                            e = mfma16(afr[4 * s4 + 2], bx[2], e);
                            o = mfma16(afr[4 * s4 + 3], bx[3], o);
#pragma unroll
                            for (int k = 0; k < 4; ++k) bx[k] = nbx[k];
                        }
                    }
                } else {
                    float a[4], bx[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int rk = 4 * k + g;
                        a[k] = asrc[rk * kMlpHS];
                        bx[k] = bsrc[rk * kMlpTS];
                    }
#pragma unroll 1
                    for (int s4 = 0; s4 < kgroups; ++s4) {
                        float na[4], nbx[4];
                        const int base = 16 * (s4 + 1 < kgroups ? s4 + 1 : s4) + g;
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            na[k] = asrc[(base + 4 * k) * kMlpHS];
                            nbx[k] = bsrc[(base + 4 * k) * kMlpTS];
                        }
                        e = mfma16(a[0], bx[0], e);
                        o = mfma16(a[1], bx[1], o);
                        e = mfma16(a[2], bx[2], e);
                        o = mfma16(a[3], bx[3], o);
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            a[k] = na[k];
                            bx[k] = nbx[k];
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) e[i] += o[i];
                return e;
            };
            put(0, tps);
            if (NT > 1) put(1, tps + CH);
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                lds_barrier();
                float *cur = tps + (r & 1) * 2 * CH;
                float *nxt = tps + ((r + 1) & 1) * 2 * CH;
                if (2 * r + 2 < NT) put(2 * r + 2, nxt);
                if (2 * r + 3 < NT) put(2 * r + 3, nxt + CH);
                if (16 * (2 * r) < F)                          // uniform: chunks past F are all zero
                    accU[r] = gemm_unit(cur + cw * CH + c16, H1s + 16 * mw + c16, accU[r]);
            }
            if (NT & 1) {
                lds_barrier();
                if (w < 4) accL = gemm_unit(tps + (NR & 1) * 2 * CH + c16, H1s + 16 * w + c16, accL);
            }
        }
        lds_barrier();                            // H1s / sy / gfin are rewritten by the next query
        MLP_STAMP(7);                              // dW1 MFMAs
    }

    // ---- this workgroup's partial vector [dW1 | db1 | dW2 | db2 | dW3 | db3]: the dW1 tiles are
    // disjoint between the waves and go straight out; the small per-document-partitioned sums are
    // folded over the waves in LDS in a fixed order ----
    if (FWD) return;
    float *dst = p.part + (size_t)blockIdx.x * p.pitch;
    {
        const int cw = w >> 2, mw = w & 3;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int f = 16 * (2 * r + cw) + c16;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int j1 = 16 * mw + 4 * g + i;
                if (j1 < H1 && f < F) dst[(size_t)j1 * F + f] = accU[r][i];
            }
        }
        if ((NT & 1) && w < 4) {
            const int f = 16 * (NT - 1) + c16;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int j1 = 16 * w + 4 * g + i;
                if (j1 < H1 && f < F) dst[(size_t)j1 * F + f] = accL[i];
            }
        }
    }
    // every wave drops its sums into its own LDS slice ([16][66] dW2 image + 97 scalars), all at
    // once; then each output is the sum of the 8 slices in wave order (fixed, hence deterministic)
    constexpr int RP2 = kMlpH1 + 2;               // pitch of the dW2 image [16][66]
    constexpr int SL = kMlpH2 * RP2 + 100;        // floats per wave slice
    float *slice = W1s + (size_t)w * SL;          // W1s + H1s are dead now (8 * SL floats fit)
    float *slv = slice + kMlpH2 * RP2;            // [64] db1 | [16] db2 | [16] dW3 | [1] db3
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) accB1[t][i] = row16_sum(accB1[t][i]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        accB2[i] = row16_sum(accB2[i]);
        accW3[i] = row16_sum(accW3[i]);
    }
    accB3 = wave_sum(accB3);
    __syncthreads();                              // the last query's LDS traffic is over
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) slice[(4 * g + i) * RP2 + 16 * tt + c16] = accW2[tt][i];
        if (c16 == 0) {
#pragma unroll
            for (int t = 0; t < 4; ++t) slv[16 * t + 4 * g + i] = accB1[t][i];
            slv[64 + 4 * g + i] = accB2[i];
            slv[80 + 4 * g + i] = accW3[i];
        }
    }
    if (lane == 0) slv[96] = accB3;
    __syncthreads();
    MLP_STAMP(8);                                  // fold
    {
        const int oB1 = H1 * F, oW2 = oB1 + H1, oB2 = oW2 + H2 * H1, oW3 = oB2 + H2, oB3 = oW3 + H2;
        auto folded = [&](int off) {
            float t = 0.f;
#pragma unroll
            for (int k = 0; k < kMlpWaves; ++k) t += W1s[(size_t)k * SL + off];
            return t;
        };
        for (int i = tid; i < H2 * H1; i += T) {
            const int k = i / H1, j = i - k * H1;
            dst[oW2 + i] = folded(k * RP2 + j);
        }
        for (int i = tid; i < H1; i += T) dst[oB1 + i] = folded(kMlpH2 * RP2 + i);
        if (tid < H2) {
            dst[oB2 + tid] = folded(kMlpH2 * RP2 + 64 + tid);
            dst[oW3 + tid] = folded(kMlpH2 * RP2 + 80 + tid);
        }
        if (tid == 0) dst[oB3] = folded(kMlpH2 * RP2 + 96);
    }
    MLP_STAMP(9);                                  // partial vector written
}

// ---- host side ----
inline int mlp_grid(int B)
{
    const int cus = device_cu_count();
    return B < cus ? B : cus;
}

template <int KIND, int NT, bool FWD = false>
int launch_mlp_nt(const MlpParams &p, int grid, hipStream_t stream)
{
    const size_t lds = mlp_lds_bytes(KIND, p.F);
    LTR_ENSURE_LDS((mlp_pairwise_kernel<KIND, NT, FWD>), lds);
    hipLaunchKernelGGL((mlp_pairwise_kernel<KIND, NT, FWD>), dim3((unsigned)grid), dim3(kMlpThreads), lds,
                       stream, p);
    return (int)hipGetLastError();
}

inline int launch_mlp_scores(const MlpParams &p, int grid, hipStream_t stream)
{
    switch (mlp_bucket(p.F)) {
    case 3: return launch_mlp_nt<LTR_HINGE, 3, true>(p, grid, stream);
    case 5: return launch_mlp_nt<LTR_HINGE, 5, true>(p, grid, stream);
    case 9: return launch_mlp_nt<LTR_HINGE, 9, true>(p, grid, stream);
    default: return launch_mlp_nt<LTR_HINGE, 14, true>(p, grid, stream);
    }
}

template <int KIND>
int launch_mlp_kind(const MlpParams &p, int grid, hipStream_t stream)
{
    switch (mlp_bucket(p.F)) {
    case 3: return launch_mlp_nt<KIND, 3>(p, grid, stream);
    case 5: return launch_mlp_nt<KIND, 5>(p, grid, stream);
    case 9: return launch_mlp_nt<KIND, 9>(p, grid, stream);
    default: return launch_mlp_nt<KIND, 14>(p, grid, stream);
    }
}
