// ltr_mlp_bigbf16.inc -- the stand-alone ReLU-MLP scorer (F -> H1 -> H2 -> 1) with WIDE HIDDEN LAYERS (H1 <= 256,
// H2 <= 64) on a BF16 feature batch of at most 160 features, lists of any length (include/ltr_mlp_bigbf16.h): the bf16
// front of mlp_big_body (ltr_mlp_big.inc), with layer 1 and the dW1 product on v_mfma_f32_16x16x32_bf16.  Included by
// ltr_mlp.hip behind ltr_mlp_big.inc (the body: one eight-wave workgroup per CU, wave w owns the hidden-1 blocks w and
// w + 8, the H1 tile and W2 in LDS, everything from the store of the H1 tile to the dH1 write) and ltr_mlp_bf16.inc (the
// bf16 vector types; the numerics are that file's).
//
// What this front supplies:
//   Image.  X stays bf16 from HBM to the MFMA: [32][32 KS + 8] bf16 (pitch 64 KS + 16 bytes, an odd number of 16-byte
//     units), KS = K-steps of the bucket >= ceil(F / 32); 16-byte fills of 8 values one tile ahead, a padded row's
//     lanes redirected and zeroed (the body's fill), the columns F .. 32 KS - 1 zeroed once.
//   Layer 1.  ONE v_mfma_f32_16x16x32_bf16 per K-step and subtile where the f32 front issues eight K = 4 steps: A = the
//     block's W1 fragment (lane l: W1[j0 + (l & 15)][32 s + 8 (l >> 4) + j], j = 0 .. 7, rounded to bf16 -- nearest
//     even -- when it is loaded), B = one 16-byte row read of the image.  C/D is laid out as v_mfma_f32_16x16x4_f32's,
//     so the store of the H1 tile and everything up to dH1 is the body's f32 code.
//   dW1.  Per owned block and 16-feature chunk TWO K = 32 steps over all 32 rows of the tile: A = the block's dH1 columns
//     of the H1 tile (rows 8g .. 8g + 7 of the tile through the body's one pointer `own`: its in-order-DS rule holds
//     unchanged) as hi = bf16(d), lo = bf16(d - hi); B = a transposed column read of the SAME image by
//     ds_read_b64_tr_b16 (MlpFrontBf16::dw1's addressing) -- no second image.  The rows of a subtile without a real
//     document enter as zeros (their H1 rows hold an earlier tile's values; their image rows are zeros as well).
// Register budget per wave, two blocks: W1 2 KS 4, dW1 2 (2 KS) 4, dW2 32 VGPRs -- 16 + 32 + 32 at KS = 2, 40 + 80 + 32 at
// KS = 5, 56 + 112 + 32 at KS = 7, next to about 100 for operands and addresses.  The gradient kernel of KS = 5
// therefore fetches a block's W1 fragments again for every tile from the L2 (the f32 words, rounded again: the same
// values; streamed two K-steps ahead of their MFMA), as the widest f32 bucket does, and ends at 255 VGPRs without
// scratch; the small sums stay in LDS (the body's).  Buckets KS = 2 and 5: F <= 64, 160.  A KS = 7 bucket (224
// features) was compiled and is NOT shipped: its gradient kernel keeps 144 registers of dW1 and dW2 and spills 142 more
// in the backward phase.  DESIGN.md section 33 has the resource table and the measurements.
#pragma once

#include "ltr_mlp_bigbf16.h"

// compiled without the packed fp32 instructions, as ltr_mlp_big.inc is
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

constexpr int kBbMaxKS = 5;          // 160 features
constexpr int kBbW1RegsKS = 2;       // the widest bucket whose gradient kernel keeps both blocks' W1 fragments in registers
constexpr int kBbW1Ahead = 2;        // K-steps of W1 in flight where it is fetched again per tile

template <int KS>
struct MlpBigFrontBf16 {
    typedef uint16_t elem;
    typedef mb_bf8 w1frag;                          // bf16(W1[j1A][32s + 8g .. +7])
    static constexpr int EU = 8;                    // bf16 per 16 bytes
    static constexpr int IP = 32 * KS + 8;          // image pitch (bf16 elements)
    static constexpr int FU = 4 * KS;
    static constexpr int NW1 = KS;
    static constexpr int NC = 2 * KS;               // dW1 chunks of 16 features
    static constexpr bool w1_regs(bool grad) { return !(grad && KS > kBbW1RegsKS); }
    static constexpr size_t lds_bytes(bool grad)
    {
        return mlp_big_lds_bytes_of((size_t)kMsRows * IP * sizeof(uint16_t), grad);
    }

    // W1 rounded to bf16 here (F % 8 == 0: all eight values of a fragment or none)
    static __device__ __forceinline__ void load_w1(w1frag (&wf)[KS], const MlpStreamParams &p, int j1A, int g)
    {
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int f0 = 32 * s + 8 * g;
            const bool ok = j1A < p.H1 && f0 < p.F;
            const float *src = p.W1 + (ok ? (size_t)j1A * p.F + f0 : 0);
            const mlp_f4 v0 = *reinterpret_cast<const mlp_f4 *>(src);
            const mlp_f4 v1 = *reinterpret_cast<const mlp_f4 *>(src + 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                wf[s][i] = (__bf16)(ok ? v0[i] : 0.f);
                wf[s][4 + i] = (__bf16)(ok ? v1[i] : 0.f);
            }
        }
    }
    // h[u] += W1 block . X^T over subtiles u0 .. u0 + NS - 1: one K = 32 step per K-step and subtile, the B fragments one
    // K-step ahead behind a scheduling fence (as the f32 front: the gradient kernel has no registers for all of them)
    template <int NS>
    static __device__ __forceinline__ void layer1(mlp_f4 (&h)[NS], const w1frag (&wf)[KS], const uint16_t *img, int u0,
                                                  int c16, int g)
    {
        const uint16_t *bsrc = img + (16 * u0 + c16) * IP + 8 * g;
        mb_bf8 xb[NS], xn[NS];
#pragma unroll
        for (int u = 0; u < NS; ++u) xb[u] = *reinterpret_cast<const mb_bf8 *>(bsrc + 16 * u * IP);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
#pragma unroll
            for (int u = 0; u < NS; ++u)
                if (s + 1 < KS) xn[u] = *reinterpret_cast<const mb_bf8 *>(bsrc + 16 * u * IP + 32 * (s + 1));
#pragma unroll
            for (int u = 0; u < NS; ++u) h[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s], xb[u], h[u], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < NS; ++u) xb[u] = xn[u];
        }
    }
    // layer 1 where the fragments do not stay in registers: the block's f32 words stream from the L2 kW1Ahead K-steps in
    // front of the MFMA that takes them (8 registers a step in flight, not 8 KS), rounded on their way in
    template <int NS>
    static __device__ __forceinline__ void layer1_refetch(mlp_f4 (&h)[NS], const MlpStreamParams &p, int j1A,
                                                          const uint16_t *img, int u0, int c16, int g)
    {
        constexpr int D = kBbW1Ahead < KS ? kBbW1Ahead : KS;
        const bool okr = j1A < p.H1;
        const float *wsrc = p.W1 + (okr ? (size_t)j1A * p.F : 0) + 8 * g;
        mlp_f4 raw[D][2];
        auto fetch = [&](int s, mlp_f4 (&r)[2]) {
            const float *src = (okr && 32 * s + 8 * g < p.F) ? wsrc + 32 * s : p.W1;
            r[0] = *reinterpret_cast<const mlp_f4 *>(src);
            r[1] = *reinterpret_cast<const mlp_f4 *>(src + 4);
        };
#pragma unroll
        for (int s = 0; s < D; ++s) fetch(s, raw[s]);
        const uint16_t *bsrc = img + (16 * u0 + c16) * IP + 8 * g;
        mb_bf8 xb[NS], xn[NS];
#pragma unroll
        for (int u = 0; u < NS; ++u) xb[u] = *reinterpret_cast<const mb_bf8 *>(bsrc + 16 * u * IP);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const bool ok = okr && 32 * s + 8 * g < p.F;
            mb_bf8 wf;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                wf[i] = (__bf16)(ok ? raw[s % D][0][i] : 0.f);
                wf[4 + i] = (__bf16)(ok ? raw[s % D][1][i] : 0.f);
            }
            if (s + D < KS) fetch(s + D, raw[s % D]);
#pragma unroll
            for (int u = 0; u < NS; ++u)
                if (s + 1 < KS) xn[u] = *reinterpret_cast<const mb_bf8 *>(bsrc + 16 * u * IP + 32 * (s + 1));
#pragma unroll
            for (int u = 0; u < NS; ++u) h[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xb[u], h[u], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < NS; ++u) xb[u] = xn[u];
        }
    }
    // dW1[block] += dH1^T . X over the 32 rows of the tile
    template <int NS>
    static __device__ __forceinline__ void dw1(mlp_f4 (&acc)[NC], const uint16_t *img, const float *own, int u0, int c16,
                                               int g)
    {
        // ---- A: dH1[row 8g + j of the tile][j1 = c16] as hi + lo in bf16; the rows of a skipped subtile (NS == 1:
        //      lanes whose g >> 1 is not u0) are zeros ----
        const bool mine = NS == 2 || (g >> 1) == u0;
        const float *asrc = own + 8 * g * kBgHP + c16;
        mb_bf8 ahi, alo;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = asrc[j * kBgHP];
            const float d = mine ? v : 0.f;
            const __bf16 hi = (__bf16)d;
            ahi[j] = hi;
            alo[j] = (__bf16)(d - (float)hi);
        }
        // ---- B: image columns 16c .. 16c + 15 of the rows 8g .. 8g + 7, two transposed blocks of 4 rows: lane 4q + r of
        //      a 16-lane group addresses row q of the block, columns 4r .. 4r + 3 ----
        const uint16_t *xsrc = img + (8 * g + (c16 >> 2)) * IP + 4 * (c16 & 3);
        typedef mb_s4 __attribute__((address_space(3))) *lds_s4;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const mb_s4 lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(xsrc + 16 * c));
            const mb_s4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(xsrc + 16 * c + 4 * IP));
            const mb_bf4 l4 = __builtin_bit_cast(mb_bf4, lo4), h4 = __builtin_bit_cast(mb_bf4, hi4);
            const mb_bf8 xb = {l4[0], l4[1], l4[2], l4[3], h4[0], h4[1], h4[2], h4[3]};
            acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahi, xb, acc[c], 0, 0, 0);
            acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(alo, xb, acc[c], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);                     // (one chunk of B fragments in flight, not 2 KS: with two
                                                                   // the KS = 5 gradient kernel spills one register)
        }
    }
};
static_assert(MlpBigFrontBf16<kBbMaxKS>::lds_bytes(true) <= kLdsBudget, "one workgroup per CU");

template <int KS, bool GRAD>
__global__ void __launch_bounds__(kBgThreads, 1)
mlp_bigbf16_kernel(MlpStreamParams p)
{
    mlp_big_body<MlpBigFrontBf16<KS>, GRAD>(p);
}

// ---- host side ----
struct MlpBigBf16Host {
    static constexpr int kAlign = 8, kMaxF = 32 * kBbMaxKS, kMaxH1 = kBgH1, kMaxH2 = kBgH2;
    static int grid(long long rows, int, bool) { return mlp_stream_grid(rows, 1); }
    template <int KS, bool GRAD>
    static int launch_ks(const MlpStreamParams &p, int grid, hipStream_t stream)
    {
        const size_t lds = MlpBigFrontBf16<KS>::lds_bytes(GRAD);
        LTR_ENSURE_LDS((mlp_bigbf16_kernel<KS, GRAD>), lds);
        hipLaunchKernelGGL((mlp_bigbf16_kernel<KS, GRAD>), dim3((unsigned)grid), dim3(kBgThreads), lds, stream, p);
        return (int)hipGetLastError();
    }
    template <bool GRAD>
    static int launch(const MlpStreamParams &p, int grid, hipStream_t stream)
    {
        const int ks = (p.F + 31) / 32;
        if (ks <= 2) return launch_ks<2, GRAD>(p, grid, stream);
        return launch_ks<5, GRAD>(p, grid, stream);
    }
};

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

extern "C" {

int ltr_mlp_bigbf16_scores(const uint16_t *X, const float *W1, const float *b1, const float *W2, const float *b2,
                           const float *W3, const float *b3, const int64_t *n, int B, int L, int F, int H1, int H2,
                           float *scores_out, void *stream)
{
    return mlp_stream_scores<MlpBigBf16Host>(X, W1, b1, W2, b2, W3, b3, n, B, L, F, H1, H2, scores_out, stream);
}

size_t ltr_mlp_bigbf16_grad_workspace_bytes(int B, int L, int F, int H1, int H2)
{
    return mlp_stream_grad_workspace_bytes<MlpBigBf16Host>(B, L, F, H1, H2);
}

int ltr_mlp_bigbf16_grad(const uint16_t *X, const float *W1, const float *b1, const float *W2, const float *b2,
                         const float *W3, const float *b3, const float *g, const int64_t *n, int B, int L, int F,
                         int H1, int H2, float *grads, void *workspace, size_t workspace_bytes, void *stream)
{
    return mlp_stream_grad<MlpBigBf16Host>(X, W1, b1, W2, b2, W3, b3, g, n, B, L, F, H1, H2, grads, workspace,
                                           workspace_bytes, stream);
}

}  // extern "C"
