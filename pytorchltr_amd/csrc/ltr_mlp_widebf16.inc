// ltr_mlp_widebf16.inc -- the ReLU-MLP scorer (F -> H1 -> H2 -> 1) on WIDE bf16 feature rows, up to 704 features:
// K-streamed score and parameter-gradient kernels on v_mfma_f32_16x16x32_bf16 for lists of any length
// (include/ltr_mlp_widebf16.h).  Included by ltr_mlp.hip behind ltr_mlp_bf16.inc (whose vector types and MFMA it uses)
// and ltr_mlp_wide.inc; the row test, the ring, the owner waves, the f32 chains behind layer 1, the epilogues and the
// host glue are those of ltr_mlp_stream.inc.
//
// This is not ltr_mlp_wide.inc with another load.  A wave's bf16 W1 fragments cost 4 registers per K = 32 step: 88 for
// a row of 704 features, against 176 in fp32.  So W1 -- rounded to bf16 ONCE -- stays in registers for the workgroup's
// whole life, as in the row kernels, and only X streams through the LDS.
// The unit of work, the mask (`row % L < n[row / L]`), the persistent grid and the tile order (workgroup w takes the
// tiles w, w + G, w + 2G, ...) are those of ltr_mlp_stream.inc; so is the wave layout (four waves, wave w owns hidden-1
// rows 16w .. 16w + 15).
//
// Forward (mlp_widebf16_fwd_kernel<NCH, GRAD>, NCH = ceil(F / 256) chunks): TILE loop outside, chunk loop inside -- the
// opposite nest of ltr_mlp_wide.inc, whose groups of tiles exist to amortise a pass over W1 that is not made here.
//     for tile:  for chunk:  image[parity] <- the tile's 32 x 256 piece of X, bf16, pitch 528 bytes (33 x 16: odd);
//                            the next piece (of this tile or of the next one) requested                   one barrier
//                            8 K-steps (the third chunk: 6) x 2 subtiles of MFMAs per wave into the tile's 8 accumulators
//                layers 2 and 3 and the score store as in mlp_stream_body; GRAD: dH2 rows, the dW2 tile, the small sums,
//                and the tile's d loss / d hidden-1 (zeros on padded rows) -> workspace, 256 B a row
// The image is double buffered by step parity, which is what lets one barrier a step do; a tile of padding costs one
// barrier.  Which rows are real is worked out two tiles ahead (the ring of ltr_mlp_stream.inc), padded rows of X are
// never requested (their lanes fetch the head of W1 and write zeros).
//
// Gradient, second kernel (mlp_widebf16_dw1_kernel<KSS>): dW1 = dH1^T . X over (column slice of 32 KSS = 256 or 352
// features) x (row range).  A tile of 32 rows is exactly ONE K = 32 step per 16 x 16 output: A = dH1^T from the
// workspace as hi = bf16(d), lo = bf16(d - hi), two MFMAs into one accumulator; B = columns of the X image by
// ds_read_b64_tr_b16 (the read of MlpFrontBf16::dw1).  A slice of 352 features is 88 accumulator registers -- twice the
// f32 kernel's widest -- so 704 features are two slices and dH1 is read twice, not four times.  One partial dW1 per row
// range, one partial vector of the small sums per workgroup of the first kernel, two launches of
// mlp_reduce_launch(loss = NULL) add them in a fixed order.  No atomics.  DESIGN.md section 31.
#pragma once

#include "ltr_mlp_widebf16.h"

constexpr int kMxMaxF = 704;
constexpr int kMxKC = 8;                        // K = 32 steps per image chunk of the forward kernel
constexpr int kMxCF = 32 * kMxKC;               // features per chunk
constexpr int kMxMaxCH = (kMxMaxF + kMxCF - 1) / kMxCF;
constexpr int kMxIP = kMxCF + 8;                // image pitch (bf16): 33 units of 16 bytes, an odd number
constexpr int kMxDH = 64;                       // floats per flat row of the d loss / d hidden-1 tile in the workspace
constexpr int kMxSliceKS = 11;                  // K-steps of the widest dW1 slice: 352 features, 88 accumulators

constexpr size_t mlp_widebf16_fwd_lds_bytes()
{
    return (size_t)2 * kMsRows * kMxIP * sizeof(uint16_t) +
           ((size_t)kMsWaves * kMsRows * kMsPS + (size_t)kMsRows * kMsPS + (size_t)kMsRing * kMsRows + 4) * sizeof(float);
}
constexpr size_t mlp_widebf16_dw1_lds_bytes(int KSS)
{
    // two images [32][32 KSS + 8] bf16; the dW1 tiles of HALF a slice (64 rows of 16 KSS + 4 floats: the same bytes)
    // are staged there at the end, one half after the other; the ring's masks behind them
    return (size_t)2 * kMsRows * (32 * KSS + 8) * sizeof(uint16_t) + 4 * sizeof(unsigned);
}
static_assert(mlp_widebf16_fwd_lds_bytes() <= kLdsBudget / kMsWgs &&
              mlp_widebf16_dw1_lds_bytes(kMxSliceKS) <= kLdsBudget / kMsWgs, "two workgroups per CU");
static_assert((size_t)64 * (16 * kMxSliceKS + 4) * sizeof(float) <= mlp_widebf16_dw1_lds_bytes(kMxSliceKS) &&
              (size_t)kMsWaves * kMsFold * sizeof(float) <= mlp_widebf16_fwd_lds_bytes(), "the epilogues' staging");

// The device code of this file is compiled without the packed fp32 instructions, as ltr_mlp2_bf16.inc is: the helpers
// inlined into the kernels below are selected as plain fp32 operations here and keep their code everywhere else.
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// K = 32 steps of W1 a wave keeps for NCH chunks: whole chunks, but the third ends at 704 features (22, not 24)
__host__ __device__ constexpr int mlp_widebf16_ksteps(int nch)
{
    return nch * kMxKC < (kMxMaxF + 31) / 32 ? nch * kMxKC : (kMxMaxF + 31) / 32;
}

// layer 1 of one chunk: NK K-steps over both subtiles of the image (MlpFrontBf16::layer1 at the chunk's pitch) --
// A = the wave's W1 fragments, B = one 16-byte row read, f32 accumulation
template <int NK>
__device__ __forceinline__ void mlp_widebf16_layer1(mlp_f4 (&h1)[2], const mb_bf8 *w1c, const uint16_t *im, const MlpLane &ln)
{
    const uint16_t *bsrc = im + ln.c16 * kMxIP + 8 * ln.g;
#pragma unroll
    for (int s = 0; s < NK; ++s) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const mb_bf8 xb = *reinterpret_cast<const mb_bf8 *>(bsrc + 16 * u * kMxIP + 32 * s);
            h1[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1c[s], xb, h1[u], 0, 0, 0);
        }
    }
}

template <int NCH, bool GRAD>
__global__ void __launch_bounds__(kMsThreads, kMsWgs)
mlp_widebf16_fwd_kernel(MlpStreamParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const MlpLane ln = mlp_lane();
    const int tid = ln.tid, w = ln.w, c16 = ln.c16, g = ln.g;
    const int F = p.F;
    const uint16_t *X = static_cast<const uint16_t *>(p.X);
    constexpr int IP = kMxIP;

    uint16_t *img = reinterpret_cast<uint16_t *>(smem);            // [2][32][IP]  the piece of X of a step
    float *part = reinterpret_cast<float *>(img + (size_t)2 * kMsRows * IP);   // [4][32][20] layer-2 partials, later
    float *scr = part + (size_t)w * kMsRows * kMsPS;               //              this wave's transposition scratch
    float *dH2s = part + (size_t)kMsWaves * kMsRows * kMsPS;       // [32][20]
    float *gs = dH2s + (size_t)kMsRows * kMsPS;                    // [3][32]      d loss / d score of the tile's rows
    unsigned *vmask = reinterpret_cast<unsigned *>(gs + kMsRing * kMsRows);    // [3] bit r: row r of the tile is real

    const mlp_f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const mlp_i4 zero4i = {0, 0, 0, 0};

    // ---- this wave's W1 fragments of the WHOLE row, rounded to bf16 here, once: bf16(W1[j1A][256 ch + 32 s + 8g .. +7]),
    //      zeros past H1 / F (F % 8 == 0: all eight or none) ----
    mb_bf8 w1r[mlp_widebf16_ksteps(NCH)];
#pragma unroll
    for (int s = 0; s < mlp_widebf16_ksteps(NCH); ++s) {
        const int f0 = 32 * s + 8 * g;
        const bool ok = ln.j1A < p.H1 && f0 < F;
        const float *src = p.W1 + (ok ? (size_t)ln.j1A * F + f0 : 0);
        const mlp_f4 v0 = *reinterpret_cast<const mlp_f4 *>(src);
        const mlp_f4 v1 = *reinterpret_cast<const mlp_f4 *>(src + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            w1r[s][i] = (__bf16)(ok ? v0[i] : 0.f);
            w1r[s][4 + i] = (__bf16)(ok ? v1[i] : 0.f);
        }
        // (four K-steps' fp32 values at a time: all of them in flight at once would be 8 registers a step, twice what
        // the fragments themselves take)
        if ((s & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
    const MlpSmallFrags sf = mlp_small_frags(p, ln);
    MlpSmallSums sums = mlp_small_sums_zero();

    // A step moves a 32 x 256 piece of X: 1024 units of 16 bytes, four per thread -- rows fr, fr + 8, fr + 16, fr + 24
    // of the tile, 8 values at feature 8 fc of the chunk
    const int fr = tid >> 5, fc = tid & 31;
    mlp_i4 P[4];                                    // the piece in flight
    auto issue_fill = [&](int tile, int ch, unsigned m) {
        const int f = ch * kMxCF + 8 * fc;
        const uint16_t *Xt = X + ((size_t)tile * kMsRows + fr) * (size_t)F + f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool ok = ((m >> (fr + 8 * k)) & 1u) && f < F;
            // (a padded row is never read: its lanes fetch the first 16 bytes of W1 and drop them)
            const void *src = ok ? (const void *)(Xt + (size_t)(8 * k) * F) : (const void *)p.W1;
            P[k] = *reinterpret_cast<const mlp_i4 *>(src);
        }
    };
    auto fill_image = [&](uint16_t *im, int ch, unsigned m) {
        const int f = ch * kMxCF + 8 * fc;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool ok = ((m >> (fr + 8 * k)) & 1u) && f < F;
            *reinterpret_cast<mlp_i4 *>(im + (fr + 8 * k) * IP + 8 * fc) = ok ? P[k] : zero4i;
        }
    };

    // ---- prologue: masks of the first two tiles, the first piece ----
    const int G = (int)gridDim.x;
    int tile = (int)blockIdx.x;
    mlp_ring_write<GRAD>(p, tid, tile, 0, vmask, gs);
    mlp_ring_write<GRAD>(p, tid, tile + G, 1, vmask, gs);
    __syncthreads();
    {
        const unsigned m0 = __builtin_amdgcn_readfirstlane(vmask[0]);
        if (m0) issue_fill(tile, 0, m0);
    }
    int slot = 0, par = 0;
    for (; tile < p.tiles; tile += G) {
        const int slot1 = mlp_ring_next(slot), slot2 = mlp_ring_next(slot1);
        // (both masks were written in front of a barrier every wave has passed; the slot rewritten below is the tile
        // before's: its mask was read in front of, and its g in front of barrier C of, that tile -- and every tile has
        // a barrier behind those)
        const unsigned m = __builtin_amdgcn_readfirstlane(vmask[slot]);
        const unsigned mnext = __builtin_amdgcn_readfirstlane(vmask[slot1]);
        mlp_ring_write<GRAD>(p, tid, tile + 2 * G, slot2, vmask, gs);
        const int doc = 16 * w + c16;              // owner waves 0, 1: the row of the tile this lane finishes
        const long long orow = (long long)tile * kMsRows + doc;
        const int cur = slot;                      // (this tile's g)
        slot = slot1;
        if (m == 0) {                              // padding only: nothing of X was requested for it
            if (!GRAD && w < 2 && g == 0 && orow < (long long)p.rows) p.scores_out[orow] = 0.f;
            if (mnext) issue_fill(tile + G, 0, mnext);
            lds_barrier();                         // (the ring: see above)
            continue;
        }

        // ---- layer 1: the tile's 8 accumulators over the chunks; W1 never moves ----
        mlp_f4 h1[2] = {sf.b1v, sf.b1v};           // pre-activations [j1 = 16w+4g+i][doc c16] of the two subtiles
        auto step = [&](auto ch_c) {
            constexpr int ch = decltype(ch_c)::value;
            uint16_t *im = img + (size_t)par * kMsRows * IP;
            fill_image(im, ch, m);                 // (waits for the piece in P)
            if (ch + 1 < NCH) issue_fill(tile, ch + 1, m);
            else if (mnext) issue_fill(tile + G, 0, mnext);        // (past the last tile: mask 0)
            // one barrier a step: the image written two steps on is this one again, and a wave gets there only
            // through the barrier of the step between, which every wave reaches behind its reads of this step
            lds_barrier();
            mlp_widebf16_layer1<mlp_widebf16_ksteps(ch + 1) - kMxKC * ch>(h1, w1r + kMxKC * ch, im, ln);
            par ^= 1;
        };
        step(m2_ns<0>{});
        if constexpr (NCH > 1) step(m2_ns<1>{});
        if constexpr (NCH > 2) step(m2_ns<2>{});

        // ---- layers 2 and 3 (as in mlp_stream_body), GRAD: and back down to dH1 ----
#pragma unroll
        for (int u = 0; u < 2; ++u) mlp_layer2_partial(sf, h1[u], scr + (16 * u + c16) * kMsPS + 4 * g);
        lds_barrier();                             // B: layer-2 partials (rewritten behind a step barrier of the next tile)
        const bool own = w < 2;
        mlp_f4 h2 = zero4;
        float s = 0.f;
        if (own) s = mlp_owner_fwd(sf, part, doc, g, h2);
        if constexpr (!GRAD) {
            if (own && g == 0 && orow < (long long)p.rows) p.scores_out[orow] = ((m >> doc) & 1u) ? s : 0.f;
        } else {
            if (own) mlp_owner_bwd(sf, sums, h2, gs[cur * kMsRows + doc], dH2s, doc, g);
            lds_barrier();                         // C: dH2 rows (rewritten behind barrier B of the next tile)
            mlp_dw2_tile<2>(sums, h1, scr, dH2s, 0, ln);
            // the dH1^T tile -> workspace: row (tile, 16u + c16), floats 16w + 4g .. +3
            mlp_dh1_tile<2>(sf, sums, h1, dH2s, 0, ln, [&](int u, const mlp_f4 &d1) {
                *reinterpret_cast<mlp_f4 *>(p.dH1 + ((size_t)tile * kMsRows + 16 * u + c16) * kMxDH + 16 * w + 4 * g) = d1;
            });
        }
    }
    if constexpr (GRAD) {
        // ---- this workgroup's partial vector of the small sums [db1 | dW2 | db2 | dW3 | db3] ----
        float *dst = p.part + (size_t)blockIdx.x * p.pitch;
        __syncthreads();
        mlp_store_small_sums(sums, dst, 0, reinterpret_cast<float *>(smem), p, ln);
    }
}

// dW1[:, slice] of the row range: workgroup blockIdx = range * nsl + slice (the workgroups that read the same dH1 rows
// start next to each other), features 32 KSS * slice .. + 32 KSS - 1, tiles range, range + GR, range + 2 GR, ...
template <int KSS>
__global__ void __launch_bounds__(kMsThreads, kMsWgs)
mlp_widebf16_dw1_kernel(MlpStreamParams p, int nsl)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const MlpLane ln = mlp_lane();
    const int tid = ln.tid, w = ln.w, c16 = ln.c16, g = ln.g;
    constexpr int T = kMsThreads;
    const int F = p.F;
    const uint16_t *X = static_cast<const uint16_t *>(p.X);
    constexpr int IP = 32 * KSS + 8;                // image pitch (bf16): odd number of 16-byte units
    constexpr int CU = 4 * KSS;                     // 16-byte units per image row
    constexpr int KP = (kMsRows * CU + T - 1) / T;  // units of a fill per thread
    constexpr int NH = KSS;                         // 16-feature output tiles per HALF of the slice
    constexpr int SP = 16 * NH + 4;                 // staging pitch (floats) of a half at the end
    const int slice = (int)blockIdx.x % nsl, range = (int)blockIdx.x / nsl;
    const int GR = (int)gridDim.x / nsl;
    const int f0s = slice * 32 * KSS;

    uint16_t *img = reinterpret_cast<uint16_t *>(smem);            // [2][32][IP]
    unsigned *vmask = reinterpret_cast<unsigned *>(img + (size_t)2 * kMsRows * IP);        // [3]
    const mlp_f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const mlp_i4 zero4i = {0, 0, 0, 0};

    mlp_f4 acc[2][NH];                              // dW1[j1 = 16w+4g+i][f = f0s + 16 (NH h + c) + c16]
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int c = 0; c < NH; ++c) acc[h][c] = zero4;

    int ur[KP], uc[KP];                             // unit tid + 256 k of a fill: image row, unit of the row
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        ur[k] = (tid + k * T) / CU;
        uc[k] = (tid + k * T) - ur[k] * CU;
    }
    mlp_i4 P[KP];                                   // the fill in flight ...
    float A[8];                                     // ... and its dH1^T operand: [j1 = 16w + c16][row 8g + j]
    auto issue_fill = [&](int tile, unsigned m) {
        const uint16_t *Xt = X + (size_t)tile * kMsRows * (size_t)F + f0s;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const bool ok = ur[k] < kMsRows && ((m >> (ur[k] & 31)) & 1u) && f0s + 8 * uc[k] < F;
            const void *src = ok ? (const void *)(Xt + (size_t)ur[k] * F + 8 * uc[k]) : (const void *)p.W1;
            P[k] = *reinterpret_cast<const mlp_i4 *>(src);
        }
        // (every row of a tile with a real row was written by the forward kernel: zeros on its padded rows)
        const float *Dt = p.dH1 + ((size_t)tile * kMsRows + 8 * g) * kMxDH + 16 * w + c16;
#pragma unroll
        for (int j = 0; j < 8; ++j) A[j] = Dt[(size_t)j * kMxDH];
    };
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
        float a1[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) a1[j] = 0.f;
        if (m) {
            fill_image(im, m);
#pragma unroll
            for (int j = 0; j < 8; ++j) a1[j] = A[j];
        }
        if (mnext) issue_fill(tile + GR, mnext);   // (past the last tile: mask 0)
        mlp_ring_write<false>(p, tid, tile + 2 * GR, slot2, vmask, nullptr);
        lds_barrier();                             // image filled (one barrier a tile: the images alternate)
        slot = slot1;
        if (m == 0) continue;
        // ---- dW1[slice] += dH1^T . X, ONE K = 32 step per output tile: A as hi + lo in bf16 ----
        mb_bf8 ahi, alo;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const __bf16 hv = (__bf16)a1[j];
            ahi[j] = hv;
            alo[j] = (__bf16)(a1[j] - (float)hv);
        }
        // B = image columns 16c .. 16c+15 of the rows 8g .. 8g+7, two transposed blocks: lane 4q + p of a 16-lane group
        // addresses row q of the block, columns 4p .. 4p+3
        const uint16_t *xsrc = im + (8 * g + (c16 >> 2)) * IP + 4 * (c16 & 3);
        typedef mb_s4 __attribute__((address_space(3))) *lds_s4;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int c = 0; c < NH; ++c) {
                const uint16_t *col = xsrc + 16 * (NH * h + c);
                const mb_s4 lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)col);
                const mb_s4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(col + 4 * IP));
                const mb_bf4 l4 = __builtin_bit_cast(mb_bf4, lo4), h4 = __builtin_bit_cast(mb_bf4, hi4);
                const mb_bf8 xb = {l4[0], l4[1], l4[2], l4[3], h4[0], h4[1], h4[2], h4[3]};
                acc[h][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahi, xb, acc[h][c], 0, 0, 0);
                acc[h][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(alo, xb, acc[h][c], 0, 0, 0);
            }
        }
    }

    // ---- this row range's partial dW1, columns of the slice: one half after the other through the wave's staging ----
    __syncthreads();
    float *dst = p.part + (size_t)range * p.pitch;
#pragma unroll
    for (int h = 0; h < 2; ++h)
        mlp_store_dw1<NH, SP>(acc[h], reinterpret_cast<float *>(smem), dst, p, f0s + 16 * NH * h, 4 * NH, ln);
}

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

// ---- host side ----
struct MlpWideBf16Plan {
    int tiles;
    int g1;                          // workgroups of the forward kernel = partial vectors of the small sums
    int nch;                         // forward kernel: image chunks of 256 features
    int nsl, kss;                    // dW1 kernel: column slices, K = 32 steps per slice (8 or 11)
    int gr;                          // dW1 kernel: row ranges = partial dW1 matrices
    int pitchA, psmall, pitchB;      // floats: a partial dW1; the small sums and their pitch
    size_t offB, offH, bytes;        // workspace: [gr partial dW1 | g1 small vectors | dH1 rows]
};

inline MlpWideBf16Plan mlp_widebf16_plan(long long rows, int F, int H1, int H2)
{
    MlpWideBf16Plan s;
    s.tiles = (int)((rows + kMsRows - 1) / kMsRows);
    const long long wgs = (long long)kMsWgs * device_cu_count();
    s.g1 = (int)(s.tiles < wgs ? s.tiles : wgs);
    const int KS = (F + 31) >> 5;
    s.nch = (KS + kMxKC - 1) / kMxKC;
    s.nsl = KS > kMxSliceKS ? 2 : 1;
    s.kss = (KS + s.nsl - 1) / s.nsl <= 8 ? 8 : kMxSliceKS;
    const long long per = wgs / s.nsl > 0 ? wgs / s.nsl : 1;
    s.gr = (int)(s.tiles < per ? s.tiles : per);
    s.pitchA = H1 * F;               // (F % 8 == 0: rows of 16 bytes)
    s.psmall = H1 + H2 * H1 + 2 * H2 + 1;
    s.pitchB = mlp_pitch(s.psmall);
    s.offB = (size_t)s.gr * s.pitchA * sizeof(float);
    s.offH = s.offB + (size_t)s.g1 * s.pitchB * sizeof(float);
    s.bytes = s.offH + (size_t)s.tiles * kMsRows * kMxDH * sizeof(float);
    return s;
}

template <int NCH, bool GRAD>
int launch_mlp_widebf16_fwd_nch(const MlpStreamParams &p, int grid, hipStream_t stream)
{
    const size_t lds = mlp_widebf16_fwd_lds_bytes();
    LTR_ENSURE_LDS((mlp_widebf16_fwd_kernel<NCH, GRAD>), lds);
    hipLaunchKernelGGL((mlp_widebf16_fwd_kernel<NCH, GRAD>), dim3((unsigned)grid), dim3(kMsThreads), lds, stream, p);
    return (int)hipGetLastError();
}
template <bool GRAD>
int launch_mlp_widebf16_fwd(const MlpStreamParams &p, const MlpWideBf16Plan &s, hipStream_t stream)
{
    static_assert(kMxMaxCH == 3, "one instantiation per chunk count");
    switch (s.nch) {
    case 1: return launch_mlp_widebf16_fwd_nch<1, GRAD>(p, s.g1, stream);
    case 2: return launch_mlp_widebf16_fwd_nch<2, GRAD>(p, s.g1, stream);
    default: return launch_mlp_widebf16_fwd_nch<3, GRAD>(p, s.g1, stream);
    }
}

template <int KSS>
int launch_mlp_widebf16_dw1(const MlpStreamParams &p, const MlpWideBf16Plan &s, hipStream_t stream)
{
    const size_t lds = mlp_widebf16_dw1_lds_bytes(KSS);
    LTR_ENSURE_LDS((mlp_widebf16_dw1_kernel<KSS>), lds);
    hipLaunchKernelGGL((mlp_widebf16_dw1_kernel<KSS>), dim3((unsigned)(s.gr * s.nsl)), dim3(kMsThreads), lds, stream, p,
                       s.nsl);
    return (int)hipGetLastError();
}

extern "C" {

int ltr_mlp_widebf16_scores(const uint16_t *X, const float *W1, const float *b1, const float *W2, const float *b2,
                            const float *W3, const float *b3, const int64_t *n, int B, int L, int F, int H1, int H2,
                            float *scores_out, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (mlp_stream_bad_shape(B, L, F, H1, H2, 8, kMxMaxF, kMlpH1, kMlpH2)) return LTR_ERR_SHAPE;
    if (!W1 || !b1 || !W2 || !b2 || !W3 || !b3) return LTR_ERR_NULL;
    if (B == 0) return LTR_OK;
    if (!X || !scores_out) return LTR_ERR_NULL;
    const MlpWideBf16Plan s = mlp_widebf16_plan((long long)B * L, F, H1, H2);
    MlpStreamParams p = mlp_stream_params(X, W1, b1, W2, b2, W3, b3, nullptr, n, B, L, F, H1, H2);
    p.scores_out = scores_out;
    return launch_mlp_widebf16_fwd<false>(p, s, (hipStream_t)stream);
}

size_t ltr_mlp_widebf16_grad_workspace_bytes(int B, int L, int F, int H1, int H2)
{
    if (B <= 0 || mlp_stream_bad_shape(B, L, F, H1, H2, 8, kMxMaxF, kMlpH1, kMlpH2)) return 0;
    return mlp_widebf16_plan((long long)B * L, F, H1, H2).bytes;
}

int ltr_mlp_widebf16_grad(const uint16_t *X, const float *W1, const float *b1, const float *W2, const float *b2,
                          const float *W3, const float *b3, const float *g, const int64_t *n, int B, int L, int F,
                          int H1, int H2, float *grads, void *workspace, size_t workspace_bytes, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (mlp_stream_bad_shape(B, L, F, H1, H2, 8, kMxMaxF, kMlpH1, kMlpH2)) return LTR_ERR_SHAPE;
    if (!W1 || !b1 || !W2 || !b2 || !W3 || !b3 || !grads) return LTR_ERR_NULL;
    const int P = mlp_param_count(F, H1, H2);
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) return mlp_reduce_launch(nullptr, 0, P, grads, nullptr, 0, nullptr, st);     // zero gradients
    if (!X || !g) return LTR_ERR_NULL;
    const MlpWideBf16Plan s = mlp_widebf16_plan((long long)B * L, F, H1, H2);
    if (!workspace || workspace_bytes < s.bytes) return LTR_ERR_WORKSPACE;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    MlpStreamParams p = mlp_stream_params(X, W1, b1, W2, b2, W3, b3, g, n, B, L, F, H1, H2);
    p.dH1 = reinterpret_cast<float *>(ws + s.offH);
    // forward and back down to dH1; the small sums, one partial vector per workgroup
    p.part = reinterpret_cast<float *>(ws + s.offB); p.pitch = s.pitchB;
    int rc = launch_mlp_widebf16_fwd<true>(p, s, st);
    if (rc != 0) return rc;
    // dW1, one partial matrix per row range
    p.part = reinterpret_cast<float *>(ws); p.pitch = s.pitchA;
    rc = s.kss == 8 ? launch_mlp_widebf16_dw1<8>(p, s, st) : launch_mlp_widebf16_dw1<kMxSliceKS>(p, s, st);
    if (rc != 0) return rc;
    // grads = [dW1 | the small sums]: both sums in a fixed order (H1 * F floats are whole 16-byte units)
    rc = mlp_reduce_launch(ws, s.gr, s.pitchA, grads, nullptr, 0, nullptr, st);
    if (rc != 0) return rc;
    return mlp_reduce_launch(ws + s.offB, s.g1, s.psmall, grads + s.pitchA, nullptr, 0, nullptr, st);
}

}  // extern "C"
