// ltr_linear_bf16.inc -- the fused step of the Linear(F, 1) scorer on a bf16 feature batch (include/ltr_linear_bf16.h):
// a register tile in the mapping of linear_regtile2_body (ltr_linear.inc) on 16-byte vectors of EIGHT bf16, its plan
// (ltr_linear_bf16_plan) and its entry point (ltr_linear_partials_bf16).  Included by ltr_linear_bf16.hip behind
// ltr_common.inc, which has the vector helpers (LbW8, lb_dot, lb_fma) and the shape predicate (lb_shape_bad) that this
// file shares with the streaming score and weight-gradient kernels: those are ltr_scorer.inc, in ltr_mlp.hip.
// DESIGN.md section 23.
//
// Numerics: a bf16 is the upper half of an fp32, so widening is a shift (v << 16) or a mask (v & 0xffff0000) and exact;
// W stays fp32 in registers, every product and sum is an fp32 VALU operation.  Nothing is rounded anywhere: the result
// is the fp32 network on the values the batch holds, up to summation order.
//
//   tile    one workgroup per query: thread t owns the vectors t, t + R C, ... of the query's n[b] F contiguous bf16
//           (C = F / 8 column vectors per row, R = 512 / C rows per sweep), requested in ONE burst of NI buffer loads
//           whose descriptor ends behind the last real row (rows past it read as 0, in hardware); four VGPRs per vector
//           of eight values -- half the registers of the fp32 tile.  Scores: per-thread partial dots through a padded
//           LDS matrix, a quad of lanes folds a row.  The pair pass is the code of ltr_common.inc, called as
//           linear_pairwise_body calls it.  dW_b: NI x 8 FMAs per thread against the registers the tile is still in,
//           one LDS fold over the R row groups, one coalesced store of the row.
#pragma once

#include "ltr_linear_bf16.h"

namespace {

constexpr int kLbThreads = 512;            // the tile's workgroup
constexpr int kLbMaxListLen = 256;         // the symmetric pair pass with one label per thread
constexpr int kLbMaxSweeps = 16;

struct LbTileParams {
    const uint16_t *X;
    const float *W, *bias;
    const void *rel;
    const int64_t *n;
    float *loss, *scores_out, *part;
    int B, L, F;
    float sigma;
    int rel_dtype;
};

__host__ __device__ inline int lb_cp(int C) { return ((C + 3) & ~7) + 4; }     // pitch of the partial-dot matrix: 4 (mod 8) words

// LDS of the tile (bytes): the query block of the symmetric pair pass (rows padded to 64-wide tiles, one gradient slice
// per wave), gfin [NI R], then the partial-dot matrix [L][CP], later the dW partials [2][512] float4
__host__ __device__ inline size_t lb_tile_lds_bytes(int kind, int L, int F, int NI)
{
    const size_t L4 = (size_t)((L + 63) & ~63);
    const size_t C = (size_t)F / 8;
    const size_t R = (size_t)kLbThreads / C;
    const size_t bytes = (loss_lds_bytes(kind, (int)L4, kLbThreads / 64) + 15) & ~(size_t)15;
    const size_t Lg = ((size_t)NI * R + 3) & ~(size_t)3;
    const size_t pd = 4 * (size_t)L * (size_t)lb_cp((int)C);
    const size_t dr = 32 * (size_t)kLbThreads;
    return bytes + 4 * Lg + (((pd > dr ? pd : dr) + 15) & ~(size_t)15);
}

template <int KIND, int NI>
__device__ __forceinline__ void linear_bf16_tile_body(const LbTileParams &p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int T = kLbThreads;
    constexpr int msplit = T >> 6;
    const int L = p.L;
    const int b = (int)blockIdx.x;
    const int nb = clamp_n(p.n[b], L);
    const int C = p.F >> 3;                         // column vectors per row
    const int F = C << 3;
    const int R = T / C;                            // rows per sweep
    const int CP = lb_cp(C);
    const int L4 = (L + 63) & ~63;                  // LDS row stride of the query block
    const int tid = threadIdx.x;
    const bool active = tid < R * C;
    const int rq = tid / C;
    const int c = tid - rq * C;                     // (inactive threads: a valid column, r below never matches)
    const int r = active ? rq : (1 << 20);

    const QueryLds q = carve_query_lds<KIND>(smem, L4, msplit);
    const size_t off = (loss_lds_bytes(KIND, L4, msplit) + 15) & ~(size_t)15;
    const int Lg = (NI * R + 3) & ~3;
    float *gfin = reinterpret_cast<float *>(smem + off);      // [Lg] d loss / d s, 0 past n[b]
    float *pd = gfin + Lg;                                    // [L][CP] partial dots ...
    float4 *dred = reinterpret_cast<float4 *>(pd);            // ... later [2][T] dW partials
    const size_t row = (size_t)b * L;

    // ---- W, then the whole tile in one burst, then the labels ----
    LbW8 w;
    w.a = reinterpret_cast<const float4 *>(p.W)[2 * c];
    w.b = reinterpret_cast<const float4 *>(p.W)[2 * c + 1];
    const float bias = p.bias ? p.bias[0] : 0.f;
    // (descriptor inputs through readfirstlane: the compiler must be able to prove them wave-uniform, or it wraps every
    // buffer load in a waterfall loop.  The descriptor ends behind the query's n[b] real rows: anything past it is 0.)
    const uintptr_t xaddr = reinterpret_cast<uintptr_t>(p.X + row * (size_t)F);
    const unsigned xlo = __builtin_amdgcn_readfirstlane((unsigned)xaddr);
    const unsigned xhi = __builtin_amdgcn_readfirstlane((unsigned)(xaddr >> 32));
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<void *>(((uintptr_t)xhi << 32) | xlo), 0,
        __builtin_amdgcn_readfirstlane(nb * F * 2), 0x00020000);
    const int voff = active ? tid * 16 : 0x7ffffff0;           // out of range -> 0
    const int sweep = R * C * 16;                              // bytes per sweep
    ltr_u32x4 x[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) x[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff + i * sweep, 0, 0);
    stage_labels(q.sy, p.rel, p.rel_dtype, row, L, nb, tid, T);
    if (KIND == LTR_NDCG1 || KIND == LTR_NDCG2)
        for (int m = tid; m < 2 * L4; m += T) q.rank_s[m] = 0;

    // ---- scores: partial dots -> LDS, a quad per row folds them ----
    {
        float *pdw = pd + (active ? rq : 0) * CP + c;          // row r, column c; sweeps are R * CP words apart
#pragma unroll
        for (int i = 0; i < NI; ++i)
            if (r < nb - i * R) pdw[i * R * CP] = lb_dot(x[i], w);
        // (opaque to the compiler: left alone it keeps the sixteen widened values of every vector -- 8 NI registers --
        // alive through the pair pass for the dW products instead of the 4 NI the tile is)
#pragma unroll
        for (int i = 0; i < NI; ++i) asm volatile("" : "+v"(x[i]));
    }
    __syncthreads();
    {
        const int h = tid & 3;
        for (int l = tid >> 2; l < nb; l += T >> 2) {
            const float *pr = pd + l * CP;
            float acc = 0.f;
            for (int cc = h; cc < C; cc += 4) acc += pr[cc];
            acc = quad_sum(acc);
            if (h == 0) q.sy[l].x = acc + bias;
        }
    }
    __syncthreads();
    if (p.scores_out)
        for (int l = tid; l < L; l += T) p.scores_out[row + l] = (l < nb) ? q.sy[l].x : 0.f;

    // ---- pair pass: as linear_pairwise_body's symmetric branch ----
    float gscale;
    if (KIND == LTR_NDCG1 || KIND == LTR_NDCG2) {
        int owners = 64;
        while (owners < L4 && owners < T) owners *= 2;
        const int ms = T / owners;
        const int mlen = (nb + ms - 1) / ms;
        const int m0 = __builtin_amdgcn_readfirstlane(min(nb, (tid / owners) * mlen));
        const int m1 = __builtin_amdgcn_readfirstlane(min(nb, m0 + mlen));
        prepare_ndcg<KIND, 1>(q, nb, owners, tid % owners, m0, m1, ms > 1);
    }
    const float total = pairwise_core_sym<KIND>(q, nb, L4, p.sigma, gscale);
    float gs = 0.f;
    for (int k = tid; k < Lg; k += T) {
        float g = 0.f;
        if (k < nb) {
#pragma unroll
            for (int s = 0; s < msplit; ++s) g += q.gpart[s * L4 + k];
            g *= gscale;
        }
        gfin[k] = g;
        gs += g;
    }
    const float gsum = block_sum(gs, q.red);        // d / d bias; its barriers also publish gfin

    // ---- dW_b: same column, NI rows per thread, straight from the registers ----
    {
        const int rr = active ? rq : 0;
        LbW8 acc = lb_zero();
#pragma unroll
        for (int i = 0; i < NI; ++i) lb_fma(acc, gfin[rr + i * R], x[i]);
        dred[tid] = acc.a;                         // (inactive threads hold zeros and are not read)
        dred[T + tid] = acc.b;
    }
    __syncthreads();
    {
        // float4 number t of the query's row: column vector t / 2, its half t % 2 -- the R row groups' partials in order;
        // thread 2 C adds the bias column and the padding.  One coalesced 16-byte store per thread.
        float4 *part4 = reinterpret_cast<float4 *>(p.part + (size_t)b * partial_pitch(F));
        if (tid < 2 * C) {
            const float4 *src = dred + (tid & 1) * T + (tid >> 1);
            float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;
            int rr = 0;
            for (; rr + 1 < R; rr += 2) { vadd(s0, src[rr * C]); vadd(s1, src[(rr + 1) * C]); }
            if (rr < R) vadd(s0, src[rr * C]);
            vadd(s0, s1);
            part4[tid] = s0;
        }
        if (tid == 2 * C) part4[2 * C] = make_float4(gsum, 0.f, 0.f, 0.f);
    }
    // (the loss is stored behind the last barrier: a store in front of a __syncthreads() makes its wave wait for the
    // acknowledgement, and the other waves for that wave)
    if (tid == 0) p.loss[b] = total;
}

// Occupancy the instantiations are sized for (waves per SIMD; a workgroup is two waves per SIMD), by sweeps:
//   NI =  5 (20 tile VGPRs): 8 waves, <= 64 VGPRs -- four workgroups per CU
//   NI = 10 (40 tile VGPRs): 6 waves, <= 80 VGPRs -- three workgroups per CU
//   NI = 16 (64 tile VGPRs): 4 waves, <= 128 VGPRs -- two workgroups per CU
// tests/test_linear_bf16_host.py holds the compiler to them (and to an empty scratch segment).
__host__ __device__ constexpr int lb_tile_waves(int NI) { return NI <= 5 ? 8 : (NI <= 10 ? 6 : 4); }

template <int KIND, int NI>
__global__ void __launch_bounds__(kLbThreads, lb_tile_waves(NI))
linear_bf16_tile_kernel(LbTileParams p)
{
    linear_bf16_tile_body<KIND, NI>(p);
}

// The sweeps a (L, F) tile needs, rounded up to an instantiation: 5, 10 or 16; 0 = off the plan
inline int lb_tile_sweeps(int L, int F)
{
    if (F <= 0 || F % 8 != 0 || F > kLbMaxF || L <= 0 || L > kLbMaxListLen) return 0;
    const int R = kLbThreads / (F / 8);
    const int ni = (L + R - 1) / R;
    return ni <= 5 ? 5 : (ni <= 10 ? 10 : (ni <= kLbMaxSweeps ? kLbMaxSweeps : 0));
}

inline bool lb_tile_takes(int kind, int L, int F, int &ni, size_t &lds)
{
    ni = lb_tile_sweeps(L, F);
    if (ni == 0) return false;
    lds = lb_tile_lds_bytes(kind, L, F, ni);
    return lds <= 64 * 1024;
}

template <int KIND, int NI>
int lb_launch_tile_ni(const LbTileParams &p, size_t lds, hipStream_t stream)
{
    hipLaunchKernelGGL((linear_bf16_tile_kernel<KIND, NI>), dim3((unsigned)p.B), dim3(kLbThreads), lds, stream, p);
    return (int)hipGetLastError();
}

template <int KIND>
int lb_launch_tile(const LbTileParams &p, int ni, size_t lds, hipStream_t stream)
{
    switch (ni) {
    case 5: return lb_launch_tile_ni<KIND, 5>(p, lds, stream);
    case 10: return lb_launch_tile_ni<KIND, 10>(p, lds, stream);
    case 16: return lb_launch_tile_ni<KIND, 16>(p, lds, stream);
    default: return LTR_ERR_CONFIG;
    }
}

}  // namespace

extern "C" {

int ltr_linear_bf16_plan(int kind, int B, int L, int F)
{
    if (kind < LTR_HINGE || kind > LTR_NDCG2 || B <= 0) return LTR_PLAN_NONE;
    int ni;
    size_t lds;
    return lb_tile_takes(kind, L, F, ni, lds) ? LTR_PLAN_REGISTER_TILE : LTR_PLAN_NONE;
}

int ltr_linear_partials_bf16(int kind, float sigma, const uint16_t *X, const float *W, const float *bias,
                             const void *rel, int rel_dtype, const int64_t *n, int B, int L, int F, float *loss,
                             float *scores_out, float *partials, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (const int rc = check_kind(kind, rel_dtype)) return rc;
    if (lb_shape_bad(B, L, F)) return LTR_ERR_SHAPE;
    if (L > kLbMaxListLen) return LTR_ERR_LIST_TOO_LONG;
    int ni;
    size_t lds;
    if (!lb_tile_takes(kind, L, F, ni, lds)) return LTR_ERR_SHAPE;
    if (B == 0) return LTR_OK;
    if (!X || !W || !rel || !n || !loss || !partials) return LTR_ERR_NULL;
    LbTileParams p;
    p.X = X; p.W = W; p.bias = bias; p.rel = rel; p.n = n;
    p.loss = loss; p.scores_out = scores_out; p.part = partials;
    p.B = B; p.L = L; p.F = F; p.sigma = sigma; p.rel_dtype = rel_dtype;
    return with_kind(kind, [&](auto K) { return lb_launch_tile<K>(p, ni, lds, (hipStream_t)stream); });
}

}  // extern "C"
