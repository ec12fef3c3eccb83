// ltr_mlp_bigwidebf16.inc -- the stand-alone ReLU-MLP scorer (F -> H1 -> H2 -> 1) with WIDE HIDDEN LAYERS on WIDE BF16
// ROWS: H1 <= 256, H2 <= 64, bf16 rows of at most 704 features, lists of any length (include/ltr_mlp_bigwidebf16.h).
// Included by ltr_mlp.hip behind ltr_mlp_bigwide.inc (mlp_bigwide_body: the eight-wave workgroup, the groups of tiles,
// the chunk loop outside and the tile loop inside, everything from the store of the H1 tile to the dH1 rows in the
// workspace; the plan and the host glue of the two-kernel gradient) and ltr_mlp_bf16.inc (the bf16 vector types; the
// numerics are that file's: X bf16 from HBM to the MFMA, the fp32 master W1 rounded nearest-even as its fragments are
// loaded, fp32 accumulation, fp32 behind layer 1, dH1 into dW1 as hi + lo).
//
// Forward (mlp_bigwidebf16_fwd_kernel<NW, GRAD>): the bf16 front of mlp_bigwide_body.
//   Chunk.  32 NW features = NW K-steps of v_mfma_f32_16x16x32_bf16; NW = 4: a step's piece of X is 32 x 128 bf16 = 512
//     units of 16 bytes, one global load and one LDS store per thread, as in the f32 front -- for twice the features.
//   Image.  [2][32][32 NW + 8] bf16 (NW = 4: pitch 272 bytes = 17 units, an odd number), double buffered by step parity.
//     The body's fill writes EVERY unit of the piece: zeros on padded rows and past F, so a partial K-step (F % 32 = 8,
//     16, 24) multiplies zeros and never an earlier step's values.
//   W1.  A chunk's fragments of the wave's two blocks: lane l holds bf16(W1[j0 + (l & 15)][32 s + 8 (l >> 4) + j]),
//     j = 0 .. 7 -- 2 x NW x 4 registers, fetched as fp32 from the L2 once per chunk and group and rounded on arrival.
//   Layer 1.  One MFMA per K-step, subtile and block; one 16-byte B row read feeds both blocks.  C/D is laid out as
//     v_mfma_f32_16x16x4_f32's, so the H1 tile and everything behind it is the body's f32 code.
//
// Gradient, second kernel (mlp_bigwidebf16_dw1_kernel<NTS>): dW1 = dH1^T . X over (row range) x (column slice of 16 NTS
// features), the slices of a range adjacent in the grid.  A 32-row tile is exactly ONE K = 32 step per 16 x 16 output:
// wave w owns the dW1 rows of blocks w and w + 8; A = dH1^T from the workspace (the body's f32 rows), split once per
// tile and block into hi = bf16(d), lo = bf16(d - hi); B = columns of the bf16 image by ds_read_b64_tr_b16 (the read of
// MlpBigFrontBf16::dw1), one B fragment for both blocks' two MFMAs.  2 x NTS x 4 accumulator registers; slices of 8 or
// 15 steps: one slice up to 240 features, two up to 480, three up to 704 (Istella's 224: one; Yahoo's 704: three, where
// the f32 kernel takes four).  Partials and
// the two mlp_reduce_launch(loss = NULL) calls are those of ltr_mlp_bigwide.inc.  No atomics.
// DESIGN.md section 35 has the phase table, the register / LDS table, the bytes and the measurements.
#pragma once

#include "ltr_mlp_bigwidebf16.h"

// (compiled without the packed fp32 instructions, as ltr_mlp_bigwide.inc is)
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

constexpr int kBxMaxF = 704;
constexpr int kBxNW = 4;             // K = 32 steps per chunk of the shipped forward kernels: 128 features
constexpr int kBxMaxNTS = 15;        // 16-feature steps of the widest dW1 slice: 240 features, 120 accumulator registers
                                     // (22 steps -- 704 features in two slices -- compile to 256 VGPRs with 18 spilled)

template <int NW_>
struct MlpBigWideFrontBf16 {
    typedef uint16_t elem;
    typedef mlp_i4 unit;                 // 16 bytes = 8 values of X on their way into the image
    typedef mb_bf8 w1frag;               // bf16(W1[16 (w + 8 hb) + c16][KC ch + 32s + 8g .. +7]), zeros past H1 / F
    static constexpr int EU = 8, NW = NW_, KC = 32 * NW, IP = KC + 8;
    static constexpr size_t lds_bytes(bool grad)
    {
        return mlp_bigwide_lds_bytes_of((size_t)2 * kMsRows * IP * sizeof(uint16_t), grad);
    }
    static __device__ __forceinline__ int steps(int left)          // the chunk's K = 32 steps (uniform)
    {
        const int rem = (left + 31) >> 5;
        return rem < NW ? rem : NW;
    }
    // (F % 8 == 0: all eight values of a fragment or none)
    static __device__ __forceinline__ void load_w1_chunk(w1frag (&wf)[2][NW], const MlpStreamParams &p, int, int, int w,
                                                         int c16, int g, int ch)
    {
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
            const int j1A = 16 * (w + 8 * hb) + c16;
#pragma unroll
            for (int s = 0; s < NW; ++s) {
                const int f0 = ch * KC + 32 * s + 8 * g;
                const bool ok = j1A < p.H1 && f0 < p.F;
                const float *src = p.W1 + (ok ? (size_t)j1A * p.F + f0 : 0);
                const mlp_f4 v0 = *reinterpret_cast<const mlp_f4 *>(src);
                const mlp_f4 v1 = *reinterpret_cast<const mlp_f4 *>(src + 4);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    wf[hb][s][i] = (__bf16)(ok ? v0[i] : 0.f);
                    wf[hb][s][4 + i] = (__bf16)(ok ? v1[i] : 0.f);
                }
                // (four K-steps' fp32 words in flight at a time: 32 registers next to the group's accumulators)
                if ((s & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    // h[hb][U0 + u] += W1 block hb . X^T over NS subtiles of the image, NB blocks; nc: the chunk's K-steps that exist
    template <int NB, int NS, int U0>
    static __device__ __forceinline__ void l1_step(mlp_f4 (&h)[2][2], const w1frag (&wf)[2][NW], const uint16_t *im,
                                                   int nc, int c16, int g)
    {
        const uint16_t *bsrc = im + (16 * U0 + c16) * IP + 8 * g;
#pragma unroll
        for (int s = 0; s < NW; ++s) {
            if (s < nc) {
                mb_bf8 xb[NS];
#pragma unroll
                for (int u = 0; u < NS; ++u) xb[u] = *reinterpret_cast<const mb_bf8 *>(bsrc + 16 * u * IP + 32 * s);
#pragma unroll
                for (int u = 0; u < NS; ++u) {
#pragma unroll
                    for (int hb = 0; hb < NB; ++hb)
                        h[hb][U0 + u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[hb][s], xb[u], h[hb][U0 + u], 0, 0, 0);
                }
            }
        }
    }
    template <int NB>
    static __device__ __forceinline__ void layer1(mlp_f4 (&h)[2][2], const w1frag (&wf)[2][NW], const uint16_t *im, int nc,
                                                  unsigned m, int c16, int g)
    {
        const bool act0 = (m & 0xFFFFu) != 0, act1 = (m >> 16) != 0;   // subtiles with a real row (uniform)
        if (act0 && act1) l1_step<NB, 2, 0>(h, wf, im, nc, c16, g);
        else if (act0) l1_step<NB, 1, 0>(h, wf, im, nc, c16, g);
        else l1_step<NB, 1, 1>(h, wf, im, nc, c16, g);
    }
};
static_assert(MlpBigWideFrontBf16<kBxNW>::lds_bytes(true) <= kLdsBudget, "one workgroup per CU");

template <int NW, bool GRAD>
__global__ void __launch_bounds__(kBgThreads, 1)
mlp_bigwidebf16_fwd_kernel(MlpStreamParams p)
{
    mlp_bigwide_body<MlpBigWideFrontBf16<NW>, GRAD>(p);
}

// LDS of the dW1 kernel: two images [32][16 NTS + 8] bf16 and the ring's masks
constexpr size_t mlp_bigwidebf16_dw1_lds_bytes(int NTS)
{
    return (size_t)2 * kMsRows * (16 * NTS + 8) * sizeof(uint16_t) + 8 * sizeof(unsigned);
}

// dW1[:, slice] of the row range: workgroup blockIdx = range * nsl + slice (the workgroups that read the same dH1 rows
// start next to each other), features 16 NTS * slice .. + 16 NTS - 1, tiles range, range + GR, range + 2 GR, ...
template <int NTS>
__global__ void __launch_bounds__(kBgThreads, 1)
mlp_bigwidebf16_dw1_kernel(MlpStreamParams p, int nsl)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int T = kBgThreads;
    constexpr int IP = 16 * NTS + 8;                // image pitch (bf16): 2 NTS + 1 units of 16 bytes, an odd number
    constexpr int RU = 2 * NTS;                     // 16-byte units per image row
    constexpr int KP = (kMsRows * RU + T - 1) / T;  // units of a fill per thread
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, g = lane >> 4;
    const int F = p.F, H1 = p.H1;
    const uint16_t *X = static_cast<const uint16_t *>(p.X);
    const int nb1 = (H1 + 15) >> 4;
    const int nh = (w < nb1 ? 1 : 0) + (w + 8 < nb1 ? 1 : 0);      // hidden-1 blocks of this wave: w, w + 8
    const int DH = mlp_bigwide_dh(H1);
    const int slice = (int)blockIdx.x % nsl, range = (int)blockIdx.x / nsl;
    const int GR = (int)gridDim.x / nsl;
    const int f0s = slice * 16 * NTS;
    const int rem = (F - f0s + 15) >> 4;
    const int nc = rem < NTS ? rem : NTS;           // the slice's 16-feature steps (uniform)

    uint16_t *img = reinterpret_cast<uint16_t *>(smem);            // [2][32][IP]
    unsigned *vmask = reinterpret_cast<unsigned *>(img + (size_t)2 * kMsRows * IP);        // [3]
    const mlp_f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const mlp_i4 zero4i = {0, 0, 0, 0};

    mlp_f4 acc[2][NTS];                             // dW1[16 (w + 8 hb) + 4g + i][f0s + 16c + c16]
#pragma unroll
    for (int c = 0; c < NTS; ++c) { acc[0][c] = zero4; acc[1][c] = zero4; }

    int ur[KP], uc[KP];                             // unit tid + 512 k of a fill: image row, unit of the row
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        ur[k] = (tid + k * T) / RU;
        uc[k] = (tid + k * T) - ur[k] * RU;
    }
    mlp_i4 P[KP];                                   // the fill in flight ...
    float A[2][8];                                  // ... and its dH1^T operands: [j1 = 16 (w + 8 hb) + c16][row 8g + j]
#pragma unroll
    for (int j = 0; j < 8; ++j) { A[0][j] = 0.f; A[1][j] = 0.f; }
    auto issue_fill = [&](int tile, unsigned m) {
        const uint16_t *Xt = X + (size_t)tile * kMsRows * (size_t)F + f0s;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const bool ok = ur[k] < kMsRows && ((m >> (ur[k] & 31)) & 1u) && f0s + 8 * uc[k] < F;
            // (a padded row is never read: its lanes fetch the first 16 bytes of W1 and drop them)
            const void *src = ok ? (const void *)(Xt + (size_t)ur[k] * F + 8 * uc[k]) : (const void *)p.W1;
            P[k] = *reinterpret_cast<const mlp_i4 *>(src);
        }
        // (every row of a tile with a real row was written by the forward kernel: zeros on its padded rows)
        const float *Dt = p.dH1 + ((size_t)tile * kMsRows + 8 * g) * DH + 16 * w + c16;
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
            if (hb < nh) {
#pragma unroll
                for (int j = 0; j < 8; ++j) A[hb][j] = Dt[(size_t)j * DH + 128 * hb];
            }
        }
    };
    // (every unit of the slice's image rows is written, zeros on padded rows and past F)
    auto fill_image = [&](uint16_t *im, unsigned m) {
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const bool ok = ((m >> (ur[k] & 31)) & 1u) && f0s + 8 * uc[k] < F;
            if (ur[k] < kMsRows) *reinterpret_cast<mlp_i4 *>(im + ur[k] * IP + 8 * uc[k]) = ok ? P[k] : zero4i;
        }
    };

    int tile = range;
    mlp_ring_write<false>(p, tid, tile, 0, vmask, nullptr);
    mlp_ring_write<false>(p, tid, tile + GR, 1, vmask, nullptr);
    __syncthreads();
    {
        const unsigned m0 = __builtin_amdgcn_readfirstlane(vmask[0]);
        if (m0) issue_fill(tile, m0);
    }
    int slot = 0, par = 0;
    for (; tile < p.tiles; tile += GR, par ^= 1) {
        const int slot1 = mlp_ring_next(slot), slot2 = mlp_ring_next(slot1);
        // (both masks were written in front of a barrier every wave has passed; the slot rewritten below was last
        // read in front of the barrier of the iteration before)
        const unsigned m = __builtin_amdgcn_readfirstlane(vmask[slot]);
        const unsigned mnext = __builtin_amdgcn_readfirstlane(vmask[slot1]);
        uint16_t *im = img + (size_t)par * kMsRows * IP;
        // ---- A of this tile, once per tile and block: hi = bf16(d), lo = bf16(d - hi) ----
        mb_bf8 ahi[2], alo[2];
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float d = A[hb][j];
                const __bf16 hv = (__bf16)d;
                ahi[hb][j] = hv;
                alo[hb][j] = (__bf16)(d - (float)hv);
            }
        }
        if (m) fill_image(im, m);
        if (mnext) issue_fill(tile + GR, mnext);   // (past the last tile: mask 0)
        mlp_ring_write<false>(p, tid, tile + 2 * GR, slot2, vmask, nullptr);
        lds_barrier();                             // image filled (one barrier a tile: the images alternate)
        slot = slot1;
        if (m == 0) continue;
        // ---- dW1[slice] += dH1^T . X, ONE K = 32 step per output tile.  B = image columns 16c .. 16c + 15 of the rows
        //      8g .. 8g + 7, two transposed blocks of 4 rows: lane 4q + r of a 16-lane group addresses row q of the
        //      block, columns 4r .. 4r + 3 ----
        const uint16_t *xsrc = im + (8 * g + (c16 >> 2)) * IP + 4 * (c16 & 3);
        typedef mb_s4 __attribute__((address_space(3))) *lds_s4;
#pragma unroll
        for (int c = 0; c < NTS; ++c) {
            if (c < nc) {
                const mb_s4 lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(xsrc + 16 * c));
                const mb_s4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(xsrc + 16 * c + 4 * IP));
                const mb_bf4 l4 = __builtin_bit_cast(mb_bf4, lo4), h4 = __builtin_bit_cast(mb_bf4, hi4);
                const mb_bf8 xb = {l4[0], l4[1], l4[2], l4[3], h4[0], h4[1], h4[2], h4[3]};
#pragma unroll
                for (int hb = 0; hb < 2; ++hb) {
                    if (hb < nh) {
                        acc[hb][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahi[hb], xb, acc[hb][c], 0, 0, 0);
                        acc[hb][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(alo[hb], xb, acc[hb][c], 0, 0, 0);
                    }
                }
            }
        }
    }

    // ---- this row range's partial dW1, columns of the slice ----
    float *dst = p.part + (size_t)range * p.pitch;
#pragma unroll
    for (int hb = 0; hb < 2; ++hb) {
        if (hb < nh) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int j1 = 16 * (w + 8 * hb) + 4 * g + i;
#pragma unroll
                for (int c = 0; c < NTS; ++c) {
                    const int f = f0s + 16 * c + c16;
                    if (j1 < H1 && f < F) dst[(size_t)j1 * F + f] = acc[hb][c][i];
                }
            }
        }
    }
}

// ---- host side ----
struct MlpBigWideBf16Host {
    static constexpr int kAlign = 8, kMaxF = kBxMaxF, kMaxH1 = kBgH1, kMaxH2 = kBgH2;
    static int grid(long long rows, int, bool) { return mlp_stream_grid(rows, 1); }
    // dW1 slices: as few as the widest instantiation allows, then the narrowest instantiation that holds one
    static MlpBigWidePlan plan(long long rows, int F, int H1, int H2)
    {
        const int NT = (F + 15) >> 4;
        const int nsl = (NT + kBxMaxNTS - 1) / kBxMaxNTS;
        const int per = (NT + nsl - 1) / nsl;
        return mlp_bigwide_plan_of(rows, F, H1, H2, nsl, per <= 8 ? 8 : kBxMaxNTS);
    }
    template <bool GRAD>
    static int launch(const MlpStreamParams &p, int grid, hipStream_t stream)
    {
        const size_t lds = MlpBigWideFrontBf16<kBxNW>::lds_bytes(GRAD);
        LTR_ENSURE_LDS((mlp_bigwidebf16_fwd_kernel<kBxNW, GRAD>), lds);
        hipLaunchKernelGGL((mlp_bigwidebf16_fwd_kernel<kBxNW, GRAD>), dim3((unsigned)grid), dim3(kBgThreads), lds, stream, p);
        return (int)hipGetLastError();
    }
    template <int NTS>
    static int launch_dw1_nts(const MlpStreamParams &p, const MlpBigWidePlan &s, hipStream_t stream)
    {
        const size_t lds = mlp_bigwidebf16_dw1_lds_bytes(NTS);
        LTR_ENSURE_LDS((mlp_bigwidebf16_dw1_kernel<NTS>), lds);
        hipLaunchKernelGGL((mlp_bigwidebf16_dw1_kernel<NTS>), dim3((unsigned)(s.gr * s.nsl)), dim3(kBgThreads), lds, stream,
                           p, s.nsl);
        return (int)hipGetLastError();
    }
    static int launch_dw1(const MlpStreamParams &p, const MlpBigWidePlan &s, hipStream_t stream)
    {
        return s.nts == 8 ? launch_dw1_nts<8>(p, s, stream) : launch_dw1_nts<kBxMaxNTS>(p, s, stream);
    }
};

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

extern "C" {

int ltr_mlp_bigwidebf16_scores(const uint16_t *X, const float *W1, const float *b1, const float *W2, const float *b2,
                               const float *W3, const float *b3, const int64_t *n, int B, int L, int F, int H1, int H2,
                               float *scores_out, void *stream)
{
    return mlp_stream_scores<MlpBigWideBf16Host>(X, W1, b1, W2, b2, W3, b3, n, B, L, F, H1, H2, scores_out, stream);
}

size_t ltr_mlp_bigwidebf16_grad_workspace_bytes(int B, int L, int F, int H1, int H2)
{
    return mlp_bigwide_grad_workspace_bytes<MlpBigWideBf16Host>(B, L, F, H1, H2);
}

int ltr_mlp_bigwidebf16_grad(const uint16_t *X, const float *W1, const float *b1, const float *W2, const float *b2,
                             const float *W3, const float *b3, const float *g, const int64_t *n, int B, int L, int F,
                             int H1, int H2, float *grads, void *workspace, size_t workspace_bytes, void *stream)
{
    return mlp_bigwide_grad<MlpBigWideBf16Host>(X, W1, b1, W2, b2, W3, b3, g, n, B, L, F, H1, H2, grads, workspace,
                                                workspace_bytes, stream);
}

}  // extern "C"
