// ltr_mlp_bf16.inc -- the stand-alone ReLU-MLP scorer (F -> H1 -> H2 -> 1) on a bf16 feature batch: the bf16 front of
// the row-streaming score and parameter-gradient kernels, with the first layer and the dW1 product on
// v_mfma_f32_16x16x32_bf16 (include/ltr_mlp_bf16.h).  Included by ltr_mlp.hip behind ltr_mlp_stream.inc, which has the
// kernel body (mlp_stream_body) and the host glue; everything behind layer 1 and in front of dW1 is f32 there.
//
// What this front supplies:
//   X is bf16 in HBM, F % 8 == 0 (a row starts on 16 bytes), and stays bf16 in the LDS image [32][32 KS + 8] (pitch
//   64 KS + 16 bytes: an odd number of 16-byte units); KS = ceil(F / 32) K-steps, the columns F .. 32 KS - 1 are zeros
//   written once.
//   Layer 1: A = W1 rows (lane l: W1[16w + (l & 15)][32 s + 8 (l >> 4) + j], j = 0 .. 7), rounded to bf16 ONCE, round
//   to nearest even (v_cvt_pk_bf16_f32), when the wave loads its fragments -- the one place where this network is not
//   the fp32 one; B = one 16-byte row read of the image; f32 accumulation, C/D as v_mfma_f32_16x16x4_f32, so H1 (never
//   rounded) meets the f32 chains in the orientation they have.
//   dW1[j1][f] += sum over the tile's 32 rows of dH1[r][j1] * X[r][f] is ONE K = 32 step per 16 x 16 output tile.  X is
//   exact in bf16; dH1 is fed as hi = bf16(d), lo = bf16(d - hi), two MFMAs into the same accumulator (error 2^-17
//   relative, against 2^-9 for a single rounding).  B is a column read of the same image by ds_read_b64_tr_b16 (two
//   blocks of 4 rows x 16 columns per fragment): no second, transposed image -- it would cost 2 KS KB of LDS and a
//   second set of stores per fill, the transposed reads cost nothing but their address register.
// A subtile of 16 rows without a real row is skipped by the forward chains; the dW1 step always spans the 32 rows, with
// zeros for that subtile's dH1 (its image rows are zeros as well).
// Instantiations by K-steps, KS = 1 .. 7; all run two workgroups per CU.  DESIGN.md section 20.
#pragma once

#include "ltr_mlp_bf16.h"

typedef __attribute__((ext_vector_type(8))) __bf16 mb_bf8;
typedef __attribute__((ext_vector_type(4))) __bf16 mb_bf4;
typedef __attribute__((ext_vector_type(4))) short mb_s4;

constexpr int kMbMaxKS = 7;          // 224 features

template <int KS>
struct MlpFrontBf16 {
    typedef uint16_t elem;
    typedef mb_bf8 w1frag;                          // bf16(W1[j1A][32s + 8g .. +7])
    static constexpr int EU = 8;                    // bf16 per 16 bytes
    static constexpr int IP = 32 * KS + 8;          // image pitch (bf16 elements)
    static constexpr int FU = 4 * KS;
    static constexpr int NC = 2 * KS;               // dW1 chunks of 16 features
    static constexpr int SP = 32 * KS + 4;          // pitch (floats) of the dW1 staging at the end
    static constexpr int NW1 = KS;
    static constexpr size_t lds_bytes(bool grad) { return mlp_stream_lds_bytes(IP * sizeof(uint16_t), SP, grad); }

    // W1 rounded to bf16 here, once
    static __device__ __forceinline__ void load_w1(w1frag (&w1r)[KS], const MlpStreamParams &p, const MlpLane &ln)
    {
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int f0 = 32 * s + 8 * ln.g;
            const bool ok = ln.j1A < p.H1 && f0 < p.F;          // (F % 8 == 0: all eight or none)
            const float *src = p.W1 + (ok ? (size_t)ln.j1A * p.F + f0 : 0);
            const mlp_f4 v0 = *reinterpret_cast<const mlp_f4 *>(src);
            const mlp_f4 v1 = *reinterpret_cast<const mlp_f4 *>(src + 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                w1r[s][i] = (__bf16)(ok ? v0[i] : 0.f);
                w1r[s][4 + i] = (__bf16)(ok ? v1[i] : 0.f);
            }
        }
    }
    template <int NS>
    static __device__ __forceinline__ void layer1(mlp_f4 (&h1)[2], const w1frag (&w1r)[KS], const uint16_t *img, int u0,
                                                  const MlpLane &ln)
    {
        const uint16_t *bsrc = img + (16 * u0 + ln.c16) * IP + 8 * ln.g;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
#pragma unroll
            for (int u = 0; u < NS; ++u) {
                const mb_bf8 xb = *reinterpret_cast<const mb_bf8 *>(bsrc + 16 * u * IP + 32 * s);
                h1[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1r[s], xb, h1[u], 0, 0, 0);
            }
        }
    }
    template <int NS>
    static __device__ __forceinline__ void dw1(mlp_f4 (&acc)[NC], const uint16_t *img, const float *scr, int u0,
                                               const MlpLane &ln)
    {
        const int c16 = ln.c16, g = ln.g;
        // ---- A of the dW1 step: dH1[row 8g + j of the tile][j1 = c16] as hi + lo in bf16; the rows of a skipped
        //      subtile (NS == 1: lanes whose g >> 1 is not u0) are zeros ----
        const bool mine = NS == 2 || (g >> 1) == u0;
        const float *asrc = scr + (NS == 2 ? 8 * g : 8 * (g & 1)) * kMsPS + c16;
        mb_bf8 ahi, alo;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = asrc[j * kMsPS];
            const float d = mine ? v : 0.f;
            const __bf16 h = (__bf16)d;
            ahi[j] = h;
            alo[j] = (__bf16)(d - (float)h);
        }
        // ---- dW1[tile] += dH1^T . X: B = image columns 16c .. 16c+15 of the rows 8g .. 8g+7, two transposed blocks:
        //      lane 4q + p of a 16-lane group addresses row q of the block, columns 4p .. 4p+3 ----
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
        }
    }
};
static_assert(MlpFrontBf16<kMbMaxKS>::lds_bytes(true) <= kLdsBudget / kMsWgs, "two workgroups per CU");

template <int KS, bool GRAD>
__global__ void __launch_bounds__(kMsThreads, kMsWgs)
mlp_bf16_kernel(MlpStreamParams p)
{
    mlp_stream_body<MlpFrontBf16<KS>, GRAD>(p);
}

// ---- host side ----
struct MlpBf16Host {
    static constexpr int kAlign = 8, kMaxF = 32 * kMbMaxKS;
    static int grid(long long rows, int, bool) { return mlp_stream_grid(rows, kMsWgs); }
    template <int KS, bool GRAD>
    static int launch_ks(const MlpStreamParams &p, int grid, hipStream_t stream)
    {
        const size_t lds = MlpFrontBf16<KS>::lds_bytes(GRAD);
        LTR_ENSURE_LDS((mlp_bf16_kernel<KS, GRAD>), lds);
        hipLaunchKernelGGL((mlp_bf16_kernel<KS, GRAD>), dim3((unsigned)grid), dim3(kMsThreads), lds, stream, p);
        return (int)hipGetLastError();
    }
    template <bool GRAD>
    static int launch(const MlpStreamParams &p, int grid, hipStream_t stream)
    {
        switch ((p.F + 31) / 32) {
        case 1: return launch_ks<1, GRAD>(p, grid, stream);
        case 2: return launch_ks<2, GRAD>(p, grid, stream);
        case 3: return launch_ks<3, GRAD>(p, grid, stream);
        case 4: return launch_ks<4, GRAD>(p, grid, stream);
        case 5: return launch_ks<5, GRAD>(p, grid, stream);
        case 6: return launch_ks<6, GRAD>(p, grid, stream);
        default: return launch_ks<7, GRAD>(p, grid, stream);
        }
    }
};

extern "C" {

int ltr_mlp_bf16_scores(const uint16_t *X, const float *W1, const float *b1, const float *W2, const float *b2,
                        const float *W3, const float *b3, const int64_t *n, int B, int L, int F, int H1, int H2,
                        float *scores_out, void *stream)
{
    return mlp_stream_scores<MlpBf16Host>(X, W1, b1, W2, b2, W3, b3, n, B, L, F, H1, H2, scores_out, stream);
}

size_t ltr_mlp_bf16_grad_workspace_bytes(int B, int L, int F, int H1, int H2)
{
    return mlp_stream_grad_workspace_bytes<MlpBf16Host>(B, L, F, H1, H2);
}

int ltr_mlp_bf16_grad(const uint16_t *X, const float *W1, const float *b1, const float *W2, const float *b2,
                      const float *W3, const float *b3, const float *g, const int64_t *n, int B, int L, int F,
                      int H1, int H2, float *grads, void *workspace, size_t workspace_bytes, void *stream)
{
    return mlp_stream_grad<MlpBf16Host>(X, W1, b1, W2, b2, W3, b3, g, n, B, L, F, H1, H2, grads, workspace,
                                        workspace_bytes, stream);
}

}  // extern "C"
