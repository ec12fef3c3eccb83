// ltr_linear_bf16_general.inc -- the GENERAL fused step of the Linear(F, 1) scorer on a bf16 feature batch
// (include/ltr_bf16_general.h): what linear_pairwise_kernel (ltr_linear.inc) is to the fp32 register tile, for the lists
// and rows the bf16 register tile (ltr_linear_bf16.inc) cannot hold -- up to kMaxListLen documents, up to 1024 features.
// Included by ltr_linear_bf16.hip behind ltr_linear_bf16.inc.  DESIGN.md section 36.
//
// One workgroup per query, a plain grid of B workgroups; the rows cross the memory system twice (phase 1, phase 3), the
// second time in reverse so that the L2 still holds what phase 1 read last.  X is bf16 in 16-byte vectors of eight values,
// C = F / 8 of them per row; widening is exact, W, scores, loss, gradients and every sum are fp32 (LbW8, lb_dot, lb_fma:
// ltr_common.inc).  Fixed summation order, no atomics: bit-identical run to run.  Rows j >= n[b] are never read: every load
// is predicated on its row.
//
//   phase 1  scores.  A wave per row would leave most lanes idle (F = 136: 17 vectors, 47 of 64 lanes), so the lanes of a
//            wave are (row, column vector): G = the smallest power of two >= C (at most 64) lanes form a group, a wave
//            takes 64 / G rows at once, lane l owns column vector l % G of row l / G (lanes with l % G >= C load nothing;
//            C > 64: the lanes stride the row).  kLbgP1Unr row groups are in flight per wave.  The G partial dots are
//            folded inside the group by DPP adds -- no LDS round trip --, the group's last lane writes the score.  G is a
//            kernel argument (wave-uniform), not a template parameter: the fold is at most six uniform branches.
//   phase 2  the project's pair pass, as linear_pairwise_body calls it: pairwise_core_sym up to kSymMaxLen documents,
//            pairwise_core (both ends, one or four documents per thread) beyond; workgroup size and msplit from
//            choose_linear_shape, the fp32 kernel's chooser.
//   phase 3  dW_b.  Threads are (row r, column vector c) over the flat tile, R row groups, LbW8 accumulators; the R
//            partial rows are folded through LDS in order by 2 C threads, one float4 each, and stored coalesced into the
//            query's row of the partials -- [dW_b | d bias | zeros], what every ltr_linear_reduce_* entry point consumes.
// LDS: linear_lds_bytes' layout -- the query block, W (fp32), d loss / d s, the phase-3 fold [R][2 C] float4.
#pragma once

#include "ltr_bf16_general.h"

namespace {

constexpr int kLbgP1Unr = 4;
constexpr int kLbgP3Unr = 4;

struct LbGeneralParams {
    const uint16_t *X;
    const float *W, *bias;
    const void *rel;
    const int64_t *n;
    float *loss, *scores_out, *part;
    int B, L, F;
    float sigma;
    int rel_dtype;
    int msplit;         // gradient slices of the both-ends pass
    int rows_r;         // R: row groups of phase 3
    int lg;             // log2 G: lanes per row in phase 1
};

// Sum over the aligned group of 1 << lg lanes (lg wave-uniform, 0 .. 6); the LAST lane of every group holds it.
__device__ __forceinline__ float lbg_group_sum(float v, int lg)
{
    if (lg >= 1) v += dpp_move<0xB1, 0xF>(v);       // quad_perm [1,0,3,2]
    if (lg >= 2) v += dpp_move<0x4E, 0xF>(v);       // quad_perm [2,3,0,1]
    if (lg >= 3) v += dpp_move<0x141, 0xF>(v);      // row_half_mirror: 8-lane sums
    if (lg >= 4) v += dpp_move<0x140, 0xF>(v);      // row_mirror: 16-lane sums
    if (lg >= 5) v += dpp_move<0x142, 0xA>(v);      // row_bcast15: rows 1 and 3 add the row in front
    if (lg >= 6) v += dpp_move<0x143, 0xC>(v);      // row_bcast31: lane 63 holds the wave's sum
    return v;
}

__device__ __forceinline__ LbW8 lbg_weights(const float *wl, int c)
{
    LbW8 w;
    w.a = reinterpret_cast<const float4 *>(wl)[2 * c];
    w.b = reinterpret_cast<const float4 *>(wl)[2 * c + 1];
    return w;
}

// DPT == 0: symmetric pair pass (L <= kSymMaxLen), LDS rows padded to 64-wide tiles and one gradient slice per wave;
// DPT in {1, 4}: both-ends pass.  The workgroup size is a launch parameter (256, 512 or 1024: choose_linear_shape).
template <int KIND, int DPT>
__device__ __forceinline__ void bf16_general_linear_body(const LbGeneralParams &p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool kSym = (DPT == 0);
    const int L = p.L, F = p.F;
    const int b = (int)blockIdx.x;
    const int nb = clamp_n(p.n[b], L);
    const int L4 = kSym ? ((L + 63) & ~63) : ((L + 3) & ~3);     // LDS row stride of the query block
    const int C = F >> 3;                         // column vectors per row
    const int tid = threadIdx.x;
    const int T = blockDim.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int nwaves = T >> 6;
    const int msplit = kSym ? (T >> 6) : p.msplit;
    const int R = p.rows_r;

    const QueryLds q = carve_query_lds<KIND>(smem, L4, msplit);
    const size_t off = (loss_lds_bytes(KIND, L4, msplit) + 15) & ~(size_t)15;
    float *wl = reinterpret_cast<float *>(smem + off);            // [F] W
    float *gfin = wl + F;                                         // [L4] d loss / d s
    float4 *dred = reinterpret_cast<float4 *>(gfin + L4);         // [R][2 C] phase-3 fold

    const size_t row = (size_t)b * L;
    const ltr_u32x4 *Xq = reinterpret_cast<const ltr_u32x4 *>(p.X + row * (size_t)F);     // row l: Xq[l * C .. l * C + C)
    const ltr_u32x4 zero = {0u, 0u, 0u, 0u};

    for (int f = tid; f < F; f += T) wl[f] = p.W[f];
    stage_labels(q.sy, p.rel, p.rel_dtype, row, L, nb, tid, T);
    if (KIND == LTR_NDCG1 || KIND == LTR_NDCG2)
        for (int m = tid; m < 2 * L4; m += T) q.rank_s[m] = 0;
    const float bias = p.bias ? p.bias[0] : 0.f;
    __syncthreads();

    // ---- phase 1: scores = X . W + bias, lanes as (row, column vector), kLbgP1Unr row groups in flight per wave ----
    {
        const int lg = __builtin_amdgcn_readfirstlane(p.lg);
        const int G = 1 << lg;
        const int rpw = 64 >> lg;                 // rows a wave takes at once
        const int cg = lane & (G - 1);            // this lane's (first) column vector
        const int rl = lane >> lg;                // ... and its row inside the wave's row group
        const bool once = C <= G;                 // one vector per lane: its weights stay in registers
        LbW8 w0 = lb_zero();
        if (once && cg < C) w0 = lbg_weights(wl, cg);
        constexpr int UNR = kLbgP1Unr;
        const int ngroups = (nb + rpw - 1) / rpw;
        for (int g0 = wave; g0 < ngroups; g0 += nwaves * UNR) {
            float acc[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) acc[u] = 0.f;
            for (int c = cg; c < C; c += G) {
                ltr_u32x4 x[UNR];
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    const int l = (g0 + u * nwaves) * rpw + rl;
                    x[u] = (l < nb) ? Xq[(size_t)l * C + c] : zero;
                }
                const LbW8 w = once ? w0 : lbg_weights(wl, c);
#pragma unroll
                for (int u = 0; u < UNR; ++u) acc[u] += lb_dot(x[u], w);
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int l = (g0 + u * nwaves) * rpw + rl;
                const float s = lbg_group_sum(acc[u], lg) + bias;
                if (cg == G - 1 && l < nb) q.sy[l].x = s;
            }
        }
    }
    __syncthreads();
    if (p.scores_out)
        for (int l = tid; l < L; l += T) p.scores_out[row + l] = (l < nb) ? q.sy[l].x : 0.f;

    // ---- phase 2: pair pass ----
    float gscale, gsum = 0.f;
    float total;
    if constexpr (kSym) {
        if (KIND == LTR_NDCG1 || KIND == LTR_NDCG2) {
            int owners = 64;
            while (owners < L4 && owners < T) owners *= 2;
            const int ms = T / owners;
            const int mlen = (nb + ms - 1) / ms;
            const int m0 = __builtin_amdgcn_readfirstlane(min(nb, (tid / owners) * mlen));
            const int m1 = __builtin_amdgcn_readfirstlane(min(nb, m0 + mlen));
            prepare_ndcg<KIND, 1>(q, nb, owners, tid % owners, m0, m1, ms > 1);
        }
        total = pairwise_core_sym<KIND>(q, nb, L4, p.sigma, gscale);
    } else {
        total = pairwise_core<KIND, (DPT > 0 ? DPT : 1)>(q, nb, L4, msplit, p.sigma, gscale, gsum);
    }
    float gs = 0.f;
    for (int k = tid; k < nb; k += T) {
        float g = 0.f;
        for (int s = 0; s < msplit; ++s) g += q.gpart[(size_t)s * L4 + k];
        g *= gscale;
        gfin[k] = g;
        gs += g;
    }
    if (kSym) gsum = block_sum(gs, q.red);        // d / d bias; its barriers also publish gfin
    else __syncthreads();

    // ---- phase 3: dW_b[f] = sum_l gfin[l] X[b, l, f]: thread (r, c), rows r, r + R, ... counted from the LAST row ----
    {
        const int r = tid / C;
        const int c = tid - r * C;
        if (r < R) {
            LbW8 acc = lb_zero();
            constexpr int UNR = kLbgP3Unr;
            for (int l0 = r; l0 < nb; l0 += R * UNR) {
                ltr_u32x4 x[UNR];
                float g[UNR];
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    const int lf = l0 + u * R;
                    const bool ok = lf < nb;
                    const int l = ok ? nb - 1 - lf : 0;
                    g[u] = ok ? gfin[l] : 0.f;
                    x[u] = ok ? Xq[(size_t)l * C + c] : zero;
                }
#pragma unroll
                for (int u = 0; u < UNR; ++u) lb_fma(acc, g[u], x[u]);
            }
            dred[(r * C + c) * 2] = acc.a;
            dred[(r * C + c) * 2 + 1] = acc.b;
        }
        lds_barrier();
        // float4 number t of the query's row: half t % 2 of column vector t / 2 -- the R row groups' partials in order;
        // thread 2 C adds the bias column and the padding.  One coalesced 16-byte store per thread.
        float4 *part4 = reinterpret_cast<float4 *>(p.part + (size_t)b * partial_pitch(F));
        if (tid < 2 * C) {
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int rr = 0; rr < R; ++rr) vadd(s, dred[rr * 2 * C + tid]);
            part4[tid] = s;
        }
        // (from a thread that always exists: 2 C == T at 1024 features in a 256-thread workgroup)
        if (tid == (2 * C < T ? 2 * C : T - 1)) part4[2 * C] = make_float4(gsum, 0.f, 0.f, 0.f);
    }
    // (the loss is stored behind the last barrier: a store in front of one makes its wave wait for the acknowledgement)
    if (tid == 0) p.loss[b] = total;
}

// Waves per SIMD the instantiations are compiled for: the symmetric and one-row passes six (<= 80 VGPRs: three
// 512-thread workgroups per CU) -- under the 64 VGPRs of eight waves every one of them spills 27-32 registers, the pair
// pass's, and at seven 10-13 --, LambdaNDCG2's one-row pass five (<= 96: two spilled at 80), the four-documents-per-thread
// pass four (<= 128).  Nothing spills (tests/test_bf16_general_host.py holds the compiler to it).
__host__ __device__ constexpr int lbg_waves(int kind, int dpt) { return dpt > 1 ? 4 : ((kind == LTR_NDCG2 && dpt == 1) ? 5 : 6); }

template <int KIND, int DPT>
__global__ void __launch_bounds__(1024, lbg_waves(KIND, DPT))
bf16_general_linear_kernel(LbGeneralParams p)
{
    bf16_general_linear_body<KIND, DPT>(p);
}

// The launch shape of (kind, B, L, F): choose_linear_shape on rows of F / 8 column vectors; false = off the plan
inline bool lbg_takes(int kind, int B, int L, int F, LinearShape &s)
{
    if (kind < LTR_HINGE || kind > LTR_NDCG2 || F <= 0 || F % 8 != 0 || F > kLbMaxF || L <= 0 || L > kMaxListLen) return false;
    return choose_linear_shape(kind, B > 0 ? B : 1, L, F, 8, s);
}

template <int KIND, int DPT>
int lbg_launch_dpt(const LbGeneralParams &p, const LinearShape &s, hipStream_t stream)
{
    LTR_ENSURE_LDS((bf16_general_linear_kernel<KIND, DPT>), s.lds);
    hipLaunchKernelGGL((bf16_general_linear_kernel<KIND, DPT>), dim3((unsigned)p.B), dim3((unsigned)s.threads), s.lds, stream, p);
    return (int)hipGetLastError();
}

template <int KIND>
int lbg_launch(const LbGeneralParams &p, const LinearShape &s, hipStream_t stream)
{
    switch (s.dpt) {
    case 0: return lbg_launch_dpt<KIND, 0>(p, s, stream);
    case 1: return lbg_launch_dpt<KIND, 1>(p, s, stream);
    case 4: return lbg_launch_dpt<KIND, 4>(p, s, stream);
    default: return LTR_ERR_CONFIG;
    }
}

}  // namespace

extern "C" {

int ltr_bf16_general_linear_plan(int kind, int B, int L, int F)
{
    LinearShape s;
    return (B > 0 && lbg_takes(kind, B, L, F, s)) ? 1 : 0;
}

int ltr_bf16_general_linear_partials(int kind, float sigma, const uint16_t *X, const float *W, const float *bias,
                                     const void *rel, int rel_dtype, const int64_t *n, int B, int L, int F, float *loss,
                                     float *scores_out, float *partials, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (const int rc = check_kind(kind, rel_dtype)) return rc;
    if (lb_shape_bad(B, L, F)) return LTR_ERR_SHAPE;
    if (L > kMaxListLen) return LTR_ERR_LIST_TOO_LONG;
    LinearShape s;
    if (!lbg_takes(kind, B, L, F, s)) return LTR_ERR_CONFIG;
    if (B == 0) return LTR_OK;
    if (!X || !W || !rel || !n || !loss || !partials) return LTR_ERR_NULL;
    LbGeneralParams p;
    p.X = X; p.W = W; p.bias = bias; p.rel = rel; p.n = n;
    p.loss = loss; p.scores_out = scores_out; p.part = partials;
    p.B = B; p.L = L; p.F = F; p.sigma = sigma; p.rel_dtype = rel_dtype;
    p.msplit = s.msplit; p.rows_r = s.R;
    p.lg = 0;
    while (p.lg < 6 && (1 << p.lg) < F / 8) ++p.lg;
    return with_kind(kind, [&](auto K) { return lbg_launch<K>(p, s, (hipStream_t)stream); });
}

}  // extern "C"
