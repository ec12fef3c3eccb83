// ltr_mlp_rows.inc -- the ReLU-MLP scorer (F -> H1 -> H2 -> 1) on its own, f32 features: the f32 front of the
// row-streaming score and parameter-gradient kernels, on v_mfma_f32_16x16x4_f32, for lists of ANY length
// (include/ltr_mlp_rows.h).  Included by ltr_mlp.hip behind ltr_mlp_stream.inc, which has the kernel body
// (mlp_stream_body: the tile, the ring, barriers A - D, the owner waves, the epilogue) and the host glue.
//
// The fused per-query steps (ltr_mlp.inc, ltr_mlp2.inc) keep a whole query in a workgroup and stop at 256 / 128
// documents.  A document's score and its share of the parameter gradients depend on its own row and on the upstream
// d loss / d score only, so here the unit of work is a tile of 32 flat rows; a tile may hold several queries and a query
// may span many tiles; neither kernel has a list-length limit.  This is what the Linear scorer has in ltr_scorer.inc.
//
// What this front supplies: the fill in an LDS image [32][16*NT + 4] of floats, the wave's W1 fragments (NT float4),
// layer 1 as 8 NT MFMAs per wave and 32 rows, and the dW1 step as the shared f32 chain (8 NT MFMAs, B = image columns).
// All four feature buckets (NT = 3, 5, 9, 14) run this layout: without parked tiles and a loss row, the widest one
// needs 59 KB of LDS per workgroup (the staging of the dW1 tiles at the end); its gradient kernel runs one workgroup per
// CU (mlp_rows_wgs), every other instantiation two.
// DESIGN.md section 18 has the bytes, the FLOPs and the measurements.
#pragma once

#include "ltr_mlp_rows.h"

// Workgroups per CU: two, but ONE for the gradient kernel of the widest bucket: its W1 fragments (56 registers), dW1 tile
// (56) and fill in flight (28 + 7) leave too little of 256 registers for the chains (81 spilled); alone on its SIMD a
// wave has 512
constexpr int mlp_rows_wgs(int NT, bool grad) { return (grad && NT > 9) ? 1 : kMsWgs; }

template <int NT>
struct MlpFrontF32 {
    typedef float elem;
    typedef mlp_f4 w1frag;                          // W1[j1A][16c + 4g .. +3]
    static constexpr int EU = 4;                    // floats per 16 bytes
    static constexpr int IP = 16 * NT + 4;          // image pitch (floats): odd number of 16-byte units
    static constexpr int FU = 4 * NT, NC = NT, SP = IP, NW1 = NT;
    static constexpr size_t lds_bytes(bool grad) { return mlp_stream_lds_bytes(IP * sizeof(float), SP, grad); }

    static __device__ __forceinline__ void load_w1(w1frag (&w1r)[NT], const MlpStreamParams &p, const MlpLane &ln)
    {
        mlp_load_w1_f32<NT>(w1r, p, ln, 0);
    }
    template <int NS>
    static __device__ __forceinline__ void layer1(mlp_f4 (&h1)[2], const w1frag (&w1r)[NT], const float *img, int u0,
                                                  const MlpLane &ln)
    {
        const float *bsrc = img + (16 * u0 + ln.c16) * IP + 4 * ln.g;
#pragma unroll
        for (int c = 0; c < NT; ++c) {
            mlp_f4 xb[NS];
#pragma unroll
            for (int u = 0; u < NS; ++u) xb[u] = *reinterpret_cast<const mlp_f4 *>(bsrc + 16 * u * IP + 16 * c);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int u = 0; u < NS; ++u) h1[u] = mfma16(w1r[c][i], xb[u][i], h1[u]);
            }
        }
    }
    // dW1[tile] += dH1^T . X: A = the dH1 tile in the wave's scratch, read transposed ([4s + g][c16])
    template <int NS>
    static __device__ __forceinline__ void dw1(mlp_f4 (&acc)[NT], const float *img, const float *scr, int u0,
                                               const MlpLane &ln)
    {
        const float *tsrc = scr + ln.g * kMsPS + ln.c16;
        float a1[4 * NS];
#pragma unroll
        for (int s = 0; s < 4 * NS; ++s) a1[s] = tsrc[4 * s * kMsPS];
        mlp_dw1_chain_f32<NT, IP>(acc, a1, img + (16 * u0 + ln.g) * IP + ln.c16);
    }
};
// (the widest instantiations that share a CU: <14, false> and <9, true>; <14, true> is alone on its CU, mlp_rows_wgs)
static_assert(MlpFrontF32<14>::lds_bytes(false) <= kLdsBudget / kMsWgs && MlpFrontF32<9>::lds_bytes(true) <= kLdsBudget / kMsWgs,
              "two workgroups per CU");
static_assert(MlpFrontF32<14>::lds_bytes(true) <= kLdsBudget, "one workgroup per CU");

template <int NT, bool GRAD>
__global__ void __launch_bounds__(kMsThreads, mlp_rows_wgs(NT, GRAD))
mlp_rows_kernel(MlpStreamParams p)
{
    mlp_stream_body<MlpFrontF32<NT>, GRAD>(p);
}

// ---- host side ----
struct MlpRowsHost {
    static constexpr int kAlign = 4, kMaxF = 16 * 14;
    static int grid(long long rows, int F, bool grad) { return mlp_stream_grid(rows, mlp_rows_wgs(mlp_bucket(F), grad)); }
    template <int NT, bool GRAD>
    static int launch_nt(const MlpStreamParams &p, int grid, hipStream_t stream)
    {
        const size_t lds = MlpFrontF32<NT>::lds_bytes(GRAD);
        LTR_ENSURE_LDS((mlp_rows_kernel<NT, GRAD>), lds);
        hipLaunchKernelGGL((mlp_rows_kernel<NT, GRAD>), dim3((unsigned)grid), dim3(kMsThreads), lds, stream, p);
        return (int)hipGetLastError();
    }
    template <bool GRAD>
    static int launch(const MlpStreamParams &p, int grid, hipStream_t stream)
    {
        switch (mlp_bucket(p.F)) {
        case 3: return launch_nt<3, GRAD>(p, grid, stream);
        case 5: return launch_nt<5, GRAD>(p, grid, stream);
        case 9: return launch_nt<9, GRAD>(p, grid, stream);
        default: return launch_nt<14, GRAD>(p, grid, stream);
        }
    }
};

extern "C" {

int ltr_mlp_rows_scores_f32(const float *X, const float *W1, const float *b1, const float *W2, const float *b2,
                            const float *W3, const float *b3, const int64_t *n, int B, int L, int F, int H1, int H2,
                            float *scores_out, void *stream)
{
    return mlp_stream_scores<MlpRowsHost>(X, W1, b1, W2, b2, W3, b3, n, B, L, F, H1, H2, scores_out, stream);
}

size_t ltr_mlp_rows_grad_workspace_bytes(int B, int L, int F, int H1, int H2)
{
    return mlp_stream_grad_workspace_bytes<MlpRowsHost>(B, L, F, H1, H2);
}

int ltr_mlp_rows_grad_f32(const float *X, const float *W1, const float *b1, const float *W2, const float *b2,
                          const float *W3, const float *b3, const float *g, const int64_t *n, int B, int L, int F,
                          int H1, int H2, float *grads, void *workspace, size_t workspace_bytes, void *stream)
{
    return mlp_stream_grad<MlpRowsHost>(X, W1, b1, W2, b2, W3, b3, g, n, B, L, F, H1, H2, grads, workspace,
                                        workspace_bytes, stream);
}

}  // extern "C"
