// ltr_mlp_bigwide.inc -- the stand-alone ReLU-MLP scorer (F -> H1 -> H2 -> 1) with WIDE HIDDEN LAYERS on WIDE ROWS:
// H1 <= 256, H2 <= 64, f32 rows of at most 704 features, lists of any length (include/ltr_mlp_bigwide.h).  K-streamed
// score and parameter-gradient kernels on v_mfma_f32_16x16x4_f32.  Included by ltr_mlp.hip behind ltr_mlp_big.inc (the
// eight-wave workgroup, its LDS pitches and the layout of layers 2 and 3 and of the backward) and ltr_mlp_wide.inc (the
// chunk loop over a group of tiles, dW1 as a second kernel over column slices); the loop nest and the register / LDS
// plan are this file's own: ltr_mlp_big.inc keeps a wave's W1 fragments and dW1 tile in registers (72 + 72 at F = 144,
// 352 + 352 at 704), ltr_mlp_wide.inc keeps one hidden-1 block per wave and one hidden-2 fragment.
//
// Forward (mlp_bigwide_body behind a front; mlp_bigwide_fwd_kernel is its f32 front, described here, and
// ltr_mlp_bigwidebf16.inc holds the bf16 one): one workgroup of EIGHT waves per CU, wave w owns the hidden-1 blocks w and w + 8.
// A workgroup takes its 32-row tiles in GROUPS (eight for the scores, four in front of the backward half) and keeps the
// layer-1 accumulators of the whole group in registers, 16 per tile (two blocks x two subtiles).  Chunk loop outside,
// tile loop inside:
//     for chunk of 64 features:  W1 fragments of the wave's two blocks <- global (32 registers; L2: W1, 704 KiB at
//                 256 x 704, is read once per GROUP, i.e. per 720 / 360 KB of X)
//         for tile of the group:  image[parity] <- the tile's 32 x 64 piece of X, 16 bytes a thread, requested one step
//                 ahead (a padded row's lanes fetch the head of W1 and store zeros)                     one barrier
//                 up to 64 MFMAs per wave into the tile's accumulators
//     for tile of the group:  ReLU'd H1 -> LDS [32][272]                                               barrier B
//                 layers 2 and 3 as in ltr_mlp_big.inc: 4 hidden-2 blocks x 2 row subtiles, one K = H1 chain each over
//                 the W2 image [64][272]; scores: the fixed-order fold; GRAD: dH2 rows, db2 / dW3 / db3     barrier C
//                 GRAD: the hidden-1 owners add dW2[:, own rows] (registers) and db1, and write the tile's
//                 dH1 = W2^T . dH2 . [H1 > 0] to the workspace (16 ceil(H1 / 16) floats a row, zeros on padded rows)
// The image is double buffered by step parity, which is what lets one barrier a step do (ltr_mlp_wide.inc); the H1
// tile's columns are written and, in the backward, read by their owner wave only, so no barrier D is needed.
// Skipped, uniformly: blocks past H1 / H2, the 16-feature steps past the row's end in the last chunk (700 pays for 704),
// subtiles and tiles of padding only, the missing tiles of a partly filled last group (their steps cost a barrier).
//
// Gradient, second kernel (mlp_bigwide_dw1_kernel): dW1 = dH1^T . X over (row range) x (column slice of 128 or 176
// features).  Wave w owns the dW1 rows of blocks w and w + 8 for the slice (2 x 11 float4); X goes through a double-
// buffered LDS image, the A operands (dH1^T, 16 scalars a tile) come from the workspace, mostly L2: the slices of a range
// sit next to each other in the grid.  One B fragment feeds both blocks' MFMAs, which is why the chain is restated here
// and not mlp_dw1_chain_f32 called twice.  One partial dW1 per row range, one partial vector of the small sums per
// workgroup of the first kernel, two launches of mlp_reduce_launch(loss = NULL) add them in a fixed order.  No atomics.
// DESIGN.md section 34 has the phase table, the register / LDS table, the bytes and the measurements.
#pragma once

#include "ltr_mlp_bigwide.h"

// (compiled without the packed fp32 instructions, as ltr_mlp_big.inc is)
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

constexpr int kBwMaxF = 704;
constexpr int kBwNTC = 4;             // 16-feature steps per chunk
constexpr int kBwKC = 16 * kBwNTC;    // features per chunk: a step's piece of X is 512 float4, one per thread
constexpr int kBwIP = kBwKC + 4;      // image pitch (floats): odd number of 16-byte units
constexpr int kBwTG = 8;              // most tiles per group: 128 accumulator registers
// tiles per group: eight for the scores; four in front of the backward half, which holds dW2 (32 registers) as well
constexpr int mlp_bigwide_group(bool grad) { return grad ? 4 : kBwTG; }

// LDS of the forward kernel: [2][32][68] X images | [32][272] H1 tile | [64][272] W2 | [32][68] dH2 rows | [4][32] layer-3
// shares | [256] b1 [64] b2 [64] W3 | [8][32] g | [8] masks | GRAD: [516] small sums -- 135 728 bytes
// (images_bytes: both images of the front -- f32 here, bf16 in ltr_mlp_bigwidebf16.inc)
constexpr size_t mlp_bigwide_lds_bytes_of(size_t images_bytes, bool grad)
{
    return images_bytes + ((size_t)kMsRows * kBgHP + (size_t)kBgH2 * kBgHP + (size_t)kMsRows * kBgDP +
                           4 * kMsRows + kBgH1 + 2 * kBgH2 + kBwTG * kMsRows + 8 + (grad ? kBgSums : 0)) * sizeof(float);
}
constexpr size_t mlp_bigwide_fwd_lds_bytes(bool grad)
{
    return mlp_bigwide_lds_bytes_of((size_t)2 * kMsRows * kBwIP * sizeof(float), grad);
}
// LDS of the dW1 kernel: two images [32][16 NTS + 4] and the ring's masks
constexpr size_t mlp_bigwide_dw1_lds_bytes(int NTS)
{
    return ((size_t)2 * kMsRows * (16 * NTS + 4) + 8) * sizeof(float);
}
static_assert(mlp_bigwide_fwd_lds_bytes(true) <= kLdsBudget && mlp_bigwide_dw1_lds_bytes(11) <= kLdsBudget,
              "one workgroup per CU");

// floats per flat row of the d loss / d hidden-1 tile in the workspace: H1 padded to whole blocks
__host__ __device__ inline int mlp_bigwide_dh(int H1) { return 16 * ((H1 + 15) >> 4); }

// layer 1 of one step: h[hb][U0 + u] += W1 block hb (chunk fragments wf) . X^T over NS subtiles of the image, NB blocks;
// one B fragment feeds both blocks; nc: the chunk's 16-feature steps that exist
template <int NB, int NS, int U0>
__device__ __forceinline__ void mlp_bigwide_l1_step(mlp_f4 (&h)[2][2], const mlp_f4 (&wf)[2][kBwNTC], const float *im,
                                                    int nc, int c16, int g)
{
    const float *bsrc = im + (16 * U0 + c16) * kBwIP + 4 * g;
#pragma unroll
    for (int c = 0; c < kBwNTC; ++c) {
        if (c < nc) {
            mlp_f4 xb[NS];
#pragma unroll
            for (int u = 0; u < NS; ++u) xb[u] = *reinterpret_cast<const mlp_f4 *>(bsrc + 16 * u * kBwIP + 16 * c);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int u = 0; u < NS; ++u) {
#pragma unroll
                    for (int hb = 0; hb < NB; ++hb) h[hb][U0 + u] = mfma16(wf[hb][c][i], xb[u][i], h[hb][U0 + u]);
                }
            }
        }
    }
}
template <int NB>
__device__ __forceinline__ void mlp_bigwide_l1(mlp_f4 (&h)[2][2], const mlp_f4 (&wf)[2][kBwNTC], const float *im, int nc,
                                               unsigned m, int c16, int g)
{
    const bool act0 = (m & 0xFFFFu) != 0, act1 = (m >> 16) != 0;   // subtiles with a real row (uniform)
    if (act0 && act1) mlp_bigwide_l1_step<NB, 2, 0>(h, wf, im, nc, c16, g);
    else if (act0) mlp_bigwide_l1_step<NB, 1, 0>(h, wf, im, nc, c16, g);
    else mlp_bigwide_l1_step<NB, 1, 1>(h, wf, im, nc, c16, g);
}

// The f32 front of mlp_bigwide_body.  A front supplies what differs between the element types of X in front of the
// layer-1 accumulators: the image (element, 16-byte unit, pitch IP, chunk width KC), a chunk's W1 fragments of the wave's
// two blocks (NW per block), how many of a chunk's MFMA steps exist, and the layer-1 step itself.  The bf16 front is
// MlpBigWideFrontBf16 (ltr_mlp_bigwidebf16.inc).
struct MlpBigWideFrontF32 {
    typedef float elem;
    typedef mlp_f4 unit;                 // 16 bytes of X on their way into the image
    typedef mlp_f4 w1frag;               // W1[16 (w + 8 hb) + c16][64 ch + 16c + 4g .. +3], zeros past H1 / F
    static constexpr int EU = 4, KC = kBwKC, IP = kBwIP, NW = kBwNTC;
    static __device__ __forceinline__ int steps(int left)          // the chunk's 16-feature steps (uniform)
    {
        const int rem = (left + 15) >> 4;
        return rem < NW ? rem : NW;
    }
    static __device__ __forceinline__ void load_w1_chunk(w1frag (&wf)[2][NW], const MlpStreamParams &p, int tid, int lane,
                                                         int w, int c16, int g, int ch)
    {
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
            MlpLane ln;
            ln.tid = tid; ln.lane = lane; ln.w = w + 8 * hb; ln.c16 = c16; ln.g = g; ln.j1A = 16 * (w + 8 * hb) + c16;
            mlp_load_w1_f32<NW>(wf[hb], p, ln, ch * KC);
        }
    }
    template <int NB>
    static __device__ __forceinline__ void layer1(mlp_f4 (&h)[2][2], const w1frag (&wf)[2][NW], const float *im, int nc,
                                                  unsigned m, int c16, int g)
    {
        mlp_bigwide_l1<NB>(h, wf, im, nc, m, c16, g);
    }
};

// the forward kernel (GRAD: and the backward down to dH1) behind a front: everything in the header comment
template <class Front, bool GRAD>
__device__ __forceinline__ void mlp_bigwide_body(const MlpStreamParams &p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    typedef typename Front::elem elem;
    typedef typename Front::unit unit;
    constexpr int IP = Front::IP, HP = kBgHP, DP = kBgDP, TG = mlp_bigwide_group(GRAD);
    constexpr int RU = Front::KC / Front::EU;       // 16-byte units per image row
    constexpr int NP = kMsRows * RU / kBgThreads;   // units of a step per thread: rows fr + (32 / NP) k
    static_assert(NP >= 1 && NP * kBgThreads == kMsRows * RU, "whole units per thread");
    static_assert(TG % 2 == 0 && TG <= kBwTG && 32 * kBwTG <= kBgThreads, "image parity; one thread per row of a group");
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    int c16 = lane & 15, g = lane >> 4;             // (not const: see the top of the chunk loop)
    const int F = p.F, H1 = p.H1, H2 = p.H2;
    const elem *X = static_cast<const elem *>(p.X);
    const int NCH = (F + Front::KC - 1) / Front::KC;               // feature chunks
    const int nb1 = (H1 + 15) >> 4, nb2 = (H2 + 15) >> 4;          // 16-row blocks of the two hidden layers
    const int nh = (w < nb1 ? 1 : 0) + (w + 8 < nb1 ? 1 : 0);      // hidden-1 blocks of this wave: w, w + 8
    const int jb = w & 3, ju = w >> 2;              // layers 2 / 3: hidden-2 block and row subtile of this wave
    const int DH = mlp_bigwide_dh(H1);

    elem *img = reinterpret_cast<elem *>(smem);                    // [2][32][IP] the piece of X of a step
    float *h1s = reinterpret_cast<float *>(img + (size_t)2 * kMsRows * IP);    // [32][HP] H1 tile, document-major
    float *w2s = h1s + (size_t)kMsRows * HP;                       // [64][HP]    W2, zeros past (H2, H1)
    float *dH2s = w2s + (size_t)kBgH2 * HP;                        // [32][DP]
    float *sp = dH2s + (size_t)kMsRows * DP;                       // [4][32]     layer-3 partial dots per hidden-2 block
    float *b1s = sp + 4 * kMsRows;                                 // [256] b1 | [64] b2 | [64] W3, zeros past H1 / H2
    float *b2s = b1s + kBgH1, *w3s = b2s + kBgH2;
    float *gs = w3s + kBgH2;                                       // [8][32]     d loss / d score of the group's rows
    unsigned *vmask = reinterpret_cast<unsigned *>(gs + kBwTG * kMsRows);      // [8] bit r: row r of tile j is real
    // the small sums of the gradient kernel, one owner wave per entry (ltr_mlp_big.inc)
    float *db1s = gs + kBwTG * kMsRows + 8;                        // [256]
    float *db2s = db1s + kBgH1, *dw3s = db2s + 2 * kBgH2, *db3s = dw3s + 2 * kBgH2;     // [2][64], [2][64], [2]

    const mlp_f4 zero4 = {0.f, 0.f, 0.f, 0.f};

    // ---- prologue: the weights' LDS images (ltr_mlp_big.inc) ----
    for (int i = tid; i < kBgH2 * kBgH1; i += kBgThreads) {       // W2 over the blocks in use, zeros past (H2, H1)
        const int j2 = i >> 8, j1 = i & (kBgH1 - 1);
        if (j2 < 16 * nb2 && j1 < 16 * nb1) {
            const bool ok = j2 < H2 && j1 < H1;
            const float v = p.W2[ok ? (size_t)j2 * H1 + j1 : 0];
            w2s[j2 * HP + j1] = ok ? v : 0.f;
        }
    }
    if (tid < kBgH1) {
        const float v = p.b1[tid < H1 ? tid : 0];
        b1s[tid] = tid < H1 ? v : 0.f;
    } else if (tid < kBgH1 + kBgH2) {
        const int j = tid - kBgH1;
        const float v = p.b2[j < H2 ? j : 0];
        b2s[j] = j < H2 ? v : 0.f;
    } else if (tid < kBgH1 + 2 * kBgH2) {
        const int j = tid - kBgH1 - kBgH2;
        const float v = p.W3[j < H2 ? j : 0];
        w3s[j] = j < H2 ? v : 0.f;
    }
    if constexpr (GRAD)
        for (int i = tid; i < kBgSums; i += kBgThreads) db1s[i] = 0.f;
    const float b3 = p.b3[0];

    mlp_f4 accW2[4][2];              // dW2[16 b + 4g + i][16 (w + 8 hb) + c16]
#pragma unroll
    for (int b = 0; b < 4; ++b) { accW2[b][0] = zero4; accW2[b][1] = zero4; }

    // ---- a step moves a 32 x KC piece of X: 512 NP units of 16 bytes, NP per thread -- rows fr + (32 / NP) k of the
    //      tile, unit fc of the chunk (f32: 32 x 64, one float4 per thread) ----
    const int fr = tid / RU, fc = tid % RU;
    const unit zerou = {};
    unit P[NP];                                     // the piece in flight
#pragma unroll
    for (int k = 0; k < NP; ++k) P[k] = zerou;
    auto issue_fill = [&](int tile, int ch, unsigned m) {
        const int f = ch * Front::KC + Front::EU * fc;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int r = fr + (kMsRows / NP) * k;
            const bool ok = ((m >> r) & 1u) && f < F;
            // (a padded row is never read: its lanes fetch the first 16 bytes of W1 and drop them)
            const void *src = ok ? (const void *)(X + ((size_t)tile * kMsRows + r) * (size_t)F + f) : (const void *)p.W1;
            P[k] = *reinterpret_cast<const unit *>(src);
        }
    };
    // (every unit of the piece is written, zeros on padded rows and past F: no step multiplies stale LDS contents)
    auto fill_image = [&](elem *im, int ch, unsigned m) {
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int r = fr + (kMsRows / NP) * k;
            const bool ok = ((m >> r) & 1u) && ch * Front::KC + Front::EU * fc < F;
            *reinterpret_cast<unit *>(im + r * IP + Front::EU * fc) = ok ? P[k] : zerou;
        }
    };

    // ---- layers 2 and 3 of hidden-2 block jb on the 16 documents of subtile ju of tile j (ltr_mlp_big.inc's layer23:
    //      one K = H1 chain, A = W2 rows, B = H1 rows, 16 bytes each) ----
    auto layer23 = [&](int j) {
        const int doc = 16 * ju + c16;
        mlp_f4 h2 = *reinterpret_cast<const mlp_f4 *>(b2s + 16 * jb + 4 * g);
        const float *asrc = w2s + (16 * jb + c16) * HP + 4 * g;
        const float *bsrc = h1s + doc * HP + 4 * g;
        for (int s = 0; s < nb1; ++s) {
            const mlp_f4 a = *reinterpret_cast<const mlp_f4 *>(asrc + 16 * s);
            const mlp_f4 b = *reinterpret_cast<const mlp_f4 *>(bsrc + 16 * s);
#pragma unroll
            for (int i = 0; i < 4; ++i) h2 = mfma16(a[i], b[i], h2);
        }
        const mlp_f4 w3v = *reinterpret_cast<const mlp_f4 *>(w3s + 16 * jb + 4 * g);
#pragma unroll
        for (int i = 0; i < 4; ++i) h2[i] = fmaxf(h2[i], 0.f);
        if constexpr (!GRAD) {
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) s = __builtin_fmaf(w3v[i], h2[i], s);
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 32);
            if (g == 0) sp[jb * kMsRows + doc] = s;
        } else {
            const float ds = gs[j * kMsRows + doc];                // (0 on a padded row)
            mlp_f4 dh2, s2, s3;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                dh2[i] = (h2[i] > 0.f) ? ds * w3v[i] : 0.f;
                s2[i] = row16_sum(dh2[i]);
                s3[i] = row16_sum(ds * h2[i]);
            }
            *reinterpret_cast<mlp_f4 *>(dH2s + doc * DP + 16 * jb + 4 * g) = dh2;
            if (c16 == 0) {
                mlp_f4 *c2 = reinterpret_cast<mlp_f4 *>(db2s + ju * kBgH2 + 16 * jb + 4 * g);
                mlp_f4 *c3 = reinterpret_cast<mlp_f4 *>(dw3s + ju * kBgH2 + 16 * jb + 4 * g);
                *c2 += s2;
                *c3 += s3;
            }
            if (jb == 0) {
                const float s = row16_sum(ds);
                if (lane == 0) db3s[ju] += s;                      // (lanes 0 .. 15 hold the subtile's 16 documents)
            }
        }
    };
    // ---- hidden-1 owner, backward over subtiles u0 .. u0 + NS - 1 of `tile` (ltr_mlp_big.inc's chains; the dH1 tile
    //      leaves for the workspace instead of replacing H1, and a subtile of padding only gets zeros there) ----
    auto bwd = [&](auto ns_c, int u0, int tile) {
        constexpr int NS = decltype(ns_c)::value;
        const int d0 = 16 * u0;
        float *drow = p.dH1 + (size_t)tile * kMsRows * DH;
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
            if (hb < nh) {
                const int j0 = 16 * (w + 8 * hb);
                const float *own = h1s + j0;                       // this block's columns of the H1 tile
                // dW2[:, block] += dH2^T . H1: A = dH2 columns (document 4t + g), B = H1 columns
                {
                    float bb[4 * NS];
#pragma unroll
                    for (int t = 0; t < 4 * NS; ++t) bb[t] = own[(d0 + 4 * t + g) * HP + c16];
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        if (b < nb2) {
#pragma unroll
                            for (int t = 0; t < 4 * NS; ++t)
                                accW2[b][hb] = mfma16(dH2s[(d0 + 4 * t + g) * DP + 16 * b + c16], bb[t], accW2[b][hb]);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                // dH1^T block = (W2^T . dH2^T) . [H1 > 0]: A = W2 read transposed (hidden-2 row 4t + g), B = dH2 rows
                mlp_f4 d1[NS];
#pragma unroll
                for (int u = 0; u < NS; ++u) d1[u] = zero4;
                const float *asrc = w2s + g * HP + j0 + c16;
                const float *bsrc = dH2s + (d0 + c16) * DP + g;
                for (int t = 0; t < 4 * nb2; ++t) {
                    const float a = asrc[4 * t * HP];
#pragma unroll
                    for (int u = 0; u < NS; ++u) d1[u] = mfma16(a, bsrc[16 * u * DP + 4 * t], d1[u]);
                }
#pragma unroll
                for (int u = 0; u < NS; ++u) {
                    const mlp_f4 hv = *reinterpret_cast<const mlp_f4 *>(own + (d0 + 16 * u + c16) * HP + 4 * g);
#pragma unroll
                    for (int i = 0; i < 4; ++i) d1[u][i] = (hv[i] > 0.f) ? d1[u][i] : 0.f;
                    *reinterpret_cast<mlp_f4 *>(drow + (size_t)(d0 + 16 * u + c16) * DH + j0 + 4 * g) = d1[u];
                }
                if (NS == 1) *reinterpret_cast<mlp_f4 *>(drow + (size_t)(16 - d0 + c16) * DH + j0 + 4 * g) = zero4;
                mlp_f4 s1;
#pragma unroll
                for (int i = 0; i < 4; ++i) s1[i] = row16_sum(NS == 2 ? d1[0][i] + d1[NS - 1][i] : d1[0][i]);
                if (c16 == 0) *reinterpret_cast<mlp_f4 *>(db1s + j0 + 4 * g) += s1;
            }
        }
    };

    const int G = (int)gridDim.x;
    for (int t0 = (int)blockIdx.x; t0 < p.tiles; t0 += TG * G) {
        // ---- tile j of this group is t0 + j G; which of its rows are real, and their g (thread = row) ----
        __syncthreads();                           // (the prologue's images; the masks and g of the group before)
        if ((tid >> 5) < TG) {                     // (wave-uniform: a wave holds the rows of two tiles)
            const int tile = t0 + (tid >> 5) * G;
            const long long row = (long long)tile * kMsRows + (tid & 31);
            float gv;
            const bool ok = mlp_row_real<GRAD>(p, tile < p.tiles && row < (long long)p.rows, row, gv);
            const unsigned long long m = __ballot(ok);          // lanes 0 .. 31: tile 2w, lanes 32 .. 63: tile 2w + 1
            if (GRAD) gs[tid] = gv;
            if (lane == 0) {
                vmask[2 * w] = (unsigned)m;
                vmask[2 * w + 1] = (unsigned)(m >> 32);
            }
        }
        __syncthreads();

        mlp_f4 h1a[TG][2][2];                   // layer-1 pre-activations: [tile][block hb][subtile], rows 4g + i, doc c16
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
            const mlp_f4 b1v = *reinterpret_cast<const mlp_f4 *>(b1s + 16 * (w + 8 * hb) + 4 * g);
#pragma unroll
            for (int j = 0; j < TG; ++j) { h1a[j][hb][0] = b1v; h1a[j][hb][1] = b1v; }
        }

        // ---- layer 1: chunk loop outside, tile loop inside ----
        unsigned mcur = __builtin_amdgcn_readfirstlane(vmask[0]);
        if (mcur) issue_fill(t0, 0, mcur);
        for (int ch = 0; ch < NCH; ++ch) {
            // (opaque lane indices keep the address arithmetic of the steps inside the loop: ltr_mlp_big.inc)
            asm volatile("" : "+v"(c16), "+v"(g));
            typename Front::w1frag w1r[2][Front::NW];           // the chunk's W1 fragments of the wave's two blocks
            Front::load_w1_chunk(w1r, p, tid, lane, w, c16, g, ch);
            const int nc = Front::steps(F - ch * Front::KC);    // the chunk's MFMA steps that exist (uniform)
#pragma unroll
            for (int j = 0; j < TG; ++j) {
                elem *im = img + (size_t)(j & 1) * kMsRows * IP;
                if (mcur) fill_image(im, ch, mcur);             // (waits for the piece in P)
                const int jn = j + 1 < TG ? j + 1 : 0;
                const int chn = j + 1 < TG ? ch : ch + 1;
                const unsigned mn = chn < NCH ? __builtin_amdgcn_readfirstlane(vmask[jn]) : 0u;
                if (mn) issue_fill(t0 + jn * G, chn, mn);
                // one barrier a step: the image written two steps on is this one again, and a wave gets there only
                // through the barrier of the step between, which every wave reaches behind its reads of this step
                lds_barrier();
                if (mcur) {
                    if (nh == 2) Front::template layer1<2>(h1a[j], w1r, im, nc, mcur, c16, g);
                    else if (nh == 1) Front::template layer1<1>(h1a[j], w1r, im, nc, mcur, c16, g);
                }
                mcur = mn;
            }
        }

        // ---- the tiles of the group, one after the other: H1 tile, layers 2 and 3, GRAD: back down to dH1 ----
#pragma unroll
        for (int j = 0; j < TG; ++j) {
            const unsigned m = __builtin_amdgcn_readfirstlane(vmask[j]);
            const int tile = t0 + j * G;
            const long long orow = (long long)tile * kMsRows + tid;
            if (m == 0) {                          // padding only, or past the last tile (uniform: no barrier is owed)
                if (!GRAD && tid < kMsRows && orow < (long long)p.rows) p.scores_out[orow] = 0.f;
                continue;
            }
            const bool act0 = (m & 0xFFFFu) != 0, act1 = (m >> 16) != 0;
            // (the own columns of the H1 tile: last read by this wave's backward of the tile before, and by the layer-2
            // waves in front of its barrier C)
#pragma unroll
            for (int hb = 0; hb < 2; ++hb) {
                if (hb < nh) {
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        if (u == 0 ? act0 : act1) {
                            mlp_f4 h = h1a[j][hb][u];
#pragma unroll
                            for (int i = 0; i < 4; ++i) h[i] = fmaxf(h[i], 0.f);
                            *reinterpret_cast<mlp_f4 *>(h1s + (16 * u + c16) * HP + 16 * (w + 8 * hb) + 4 * g) = h;
                        }
                    }
                }
            }
            lds_barrier();                         // B: H1 tile
            if (jb < nb2 && (ju == 0 ? act0 : act1)) layer23(j);
            lds_barrier();                         // C: score shares / dH2 rows
            if constexpr (!GRAD) {
                // (the shares are rewritten behind barrier B of the next tile, which this wave has to reach)
                if (tid < kMsRows && orow < (long long)p.rows) {
                    float s = 0.f;
                    if ((m >> tid) & 1u) {
                        s = b3;
                        for (int b = 0; b < nb2; ++b) s += sp[b * kMsRows + tid];
                    }
                    p.scores_out[orow] = s;
                }
            } else {
                // (the dH2 rows are rewritten behind barrier B of the next tile: no barrier D)
                if (act0 && act1) bwd(m2_ns<2>{}, 0, tile);
                else bwd(m2_ns<1>{}, act0 ? 0 : 1, tile);
            }
        }
    }
    if constexpr (GRAD) {
        // ---- this workgroup's partial vector of the small sums [db1 | dW2 | db2 | dW3 | db3] ----
        float *dst = p.part + (size_t)blockIdx.x * p.pitch;
        const int oW2 = H1, oB2 = oW2 + H2 * H1, oW3 = oB2 + H2, oB3 = oW3 + H2;
        __syncthreads();                           // (the sums of the last tile)
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
            if (hb < nh) {
                const int j1 = 16 * (w + 8 * hb) + c16;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int j2 = 16 * b + 4 * g + i;
                        if (j2 < H2 && j1 < H1) dst[oW2 + j2 * H1 + j1] = accW2[b][hb][i];
                    }
                }
            }
        }
        if (tid < H1) dst[tid] = db1s[tid];
        if (tid < H2) {                            // the two subtiles' copies in a fixed order
            dst[oB2 + tid] = db2s[tid] + db2s[kBgH2 + tid];
            dst[oW3 + tid] = dw3s[tid] + dw3s[kBgH2 + tid];
        }
        if (tid == 0) dst[oB3] = db3s[0] + db3s[1];
    }
}

template <bool GRAD>
__global__ void __launch_bounds__(kBgThreads, 1)
mlp_bigwide_fwd_kernel(MlpStreamParams p)
{
    mlp_bigwide_body<MlpBigWideFrontF32, GRAD>(p);
}

// dW1[block hb][slice] += dH1^T . X over the 32 documents of a tile, 16-feature steps c0 .. c0 + CN - 1: A = a[hb][s]
// (dH1^T[16 (w + 8 hb) + c16][doc 4s + g]), B = image columns from xsrc (row g, column c16); one B fragment feeds the NB
// blocks, CN feature steps are in flight
template <int NB, int CN, int C0, int NTS, int IP>
__device__ __forceinline__ void mlp_bigwide_dw1_steps(mlp_f4 (&acc)[2][NTS], const float (&a)[2][8], const float *xsrc)
{
#pragma unroll
    for (int s = 0; s < 8; ++s) {
#pragma unroll
        for (int cc = 0; cc < CN; ++cc) {
            const float b = xsrc[4 * s * IP + 16 * (C0 + cc)];
#pragma unroll
            for (int hb = 0; hb < NB; ++hb) acc[hb][C0 + cc] = mfma16(a[hb][s], b, acc[hb][C0 + cc]);
        }
    }
}
// the steps C0, C0 + 2, ... in pairs; nc: the slice's 16-feature steps that exist (uniform)
template <int NB, int NTS, int IP, int C0 = 0>
__device__ __forceinline__ void mlp_bigwide_dw1_chain(mlp_f4 (&acc)[2][NTS], const float (&a)[2][8], const float *xsrc,
                                                      int nc)
{
    if constexpr (C0 + 1 < NTS) {
        if (C0 + 1 < nc) mlp_bigwide_dw1_steps<NB, 2, C0, NTS, IP>(acc, a, xsrc);
        else if (C0 < nc) mlp_bigwide_dw1_steps<NB, 1, C0, NTS, IP>(acc, a, xsrc);
        mlp_bigwide_dw1_chain<NB, NTS, IP, C0 + 2>(acc, a, xsrc, nc);
    } else if constexpr (C0 < NTS) {
        if (C0 < nc) mlp_bigwide_dw1_steps<NB, 1, C0, NTS, IP>(acc, a, xsrc);
    }
}

// dW1[:, slice] of the row range: workgroup blockIdx = range * nsl + slice (the workgroups that read the same dH1 rows
// start next to each other), features 16 NTS * slice .. + 16 NTS - 1, tiles range, range + GR, range + 2 GR, ...
template <int NTS>
__global__ void __launch_bounds__(kBgThreads, 1)
mlp_bigwide_dw1_kernel(MlpStreamParams p, int nsl)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int T = kBgThreads;
    constexpr int IP = 16 * NTS + 4;                // image pitch (floats): odd number of 16-byte units
    constexpr int C4 = 4 * NTS;                     // float4 units per image row
    constexpr int KP = (kMsRows * C4 + T - 1) / T;  // float4 units of a fill per thread
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, g = lane >> 4;
    const int F = p.F, H1 = p.H1;
    const float *X = static_cast<const float *>(p.X);
    const int nb1 = (H1 + 15) >> 4;
    const int nh = (w < nb1 ? 1 : 0) + (w + 8 < nb1 ? 1 : 0);      // hidden-1 blocks of this wave: w, w + 8
    const int DH = mlp_bigwide_dh(H1);
    const int slice = (int)blockIdx.x % nsl, range = (int)blockIdx.x / nsl;
    const int GR = (int)gridDim.x / nsl;
    const int f0s = slice * 16 * NTS;
    const int rem = (F - f0s + 15) >> 4;
    const int nc = rem < NTS ? rem : NTS;           // the slice's 16-feature steps (uniform)

    float *img = reinterpret_cast<float *>(smem);                  // [2][32][IP]
    unsigned *vmask = reinterpret_cast<unsigned *>(img + (size_t)2 * kMsRows * IP);        // [3]
    const mlp_f4 zero4 = {0.f, 0.f, 0.f, 0.f};

    mlp_f4 acc[2][NTS];                             // dW1[16 (w + 8 hb) + 4g + i][f0s + 16c + c16]
#pragma unroll
    for (int c = 0; c < NTS; ++c) { acc[0][c] = zero4; acc[1][c] = zero4; }

    int ur[KP], uc[KP];                             // float4 unit tid + 512 k of a fill: image row, float4 of the row
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        ur[k] = (tid + k * T) / C4;
        uc[k] = (tid + k * T) - ur[k] * C4;
    }
    mlp_f4 P[KP];                                   // the fill in flight ...
    float A[2][8];                                  // ... and its dH1^T operands
#pragma unroll
    for (int s = 0; s < 8; ++s) { A[0][s] = 0.f; A[1][s] = 0.f; }
    auto issue_fill = [&](int tile, unsigned m) {
        const float *Xt = X + (size_t)tile * kMsRows * (size_t)F + f0s;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const bool ok = ur[k] < kMsRows && ((m >> (ur[k] & 31)) & 1u) && f0s + 4 * uc[k] < F;
            // (a padded row is never read: its lanes fetch the first 16 bytes of W1 and drop them)
            const float *src = ok ? Xt + (size_t)ur[k] * F + 4 * uc[k] : p.W1;
            P[k] = *reinterpret_cast<const mlp_f4 *>(src);
        }
        // (every row of a tile with a real row was written by the forward kernel: zeros on its padded rows)
        const float *Dt = p.dH1 + ((size_t)tile * kMsRows + g) * DH + 16 * w + c16;
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
            if (hb < nh) {
#pragma unroll
                for (int s = 0; s < 8; ++s) A[hb][s] = Dt[(size_t)4 * s * DH + 128 * hb];
            }
        }
    };
    auto fill_image = [&](float *im, unsigned m) {
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const bool ok = ((m >> (ur[k] & 31)) & 1u) && f0s + 4 * uc[k] < F;
            mlp_f4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = ok ? P[k][i] : 0.f;
            if (ur[k] < kMsRows) *reinterpret_cast<mlp_f4 *>(im + ur[k] * IP + 4 * uc[k]) = v;
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
        float *im = img + (size_t)par * kMsRows * IP;
        float a1[2][8];
#pragma unroll
        for (int s = 0; s < 8; ++s) { a1[0][s] = A[0][s]; a1[1][s] = A[1][s]; }
        if (m) fill_image(im, m);
        if (mnext) issue_fill(tile + GR, mnext);   // (past the last tile: mask 0)
        mlp_ring_write<false>(p, tid, tile + 2 * GR, slot2, vmask, nullptr);
        lds_barrier();                             // image filled (one barrier a tile: the images alternate)
        slot = slot1;
        if (m == 0) continue;
        const float *xsrc = im + g * IP + c16;     // dW1[slice] += dH1^T . X: B = image columns
        if (nh == 2) mlp_bigwide_dw1_chain<2, NTS, IP>(acc, a1, xsrc, nc);
        else if (nh == 1) mlp_bigwide_dw1_chain<1, NTS, IP>(acc, a1, xsrc, nc);
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
struct MlpBigWidePlan {
    int tiles;
    int g1;                          // workgroups of the forward kernel = partial vectors of the small sums
    int nsl, nts;                    // dW1 kernel: column slices, 16-feature steps per slice (8 or 11)
    int gr;                          // dW1 kernel: row ranges = partial dW1 matrices
    int pitchA, psmall, pitchB;      // floats: a partial dW1; the small sums and their pitch
    size_t offB, offH, bytes;        // workspace: [gr partial dW1 | g1 small vectors | dH1 rows]
};

// nsl column slices of nts 16-feature steps each (the front's choice)
inline MlpBigWidePlan mlp_bigwide_plan_of(long long rows, int F, int H1, int H2, int nsl, int nts)
{
    MlpBigWidePlan s;
    s.tiles = (int)((rows + kMsRows - 1) / kMsRows);
    const long long wgs = device_cu_count();        // one workgroup per CU
    s.g1 = (int)(s.tiles < wgs ? s.tiles : wgs);
    s.nsl = nsl;
    s.nts = nts;
    const long long per = wgs / s.nsl > 0 ? wgs / s.nsl : 1;
    s.gr = (int)(s.tiles < per ? s.tiles : per);
    s.pitchA = H1 * F;               // (F % 4 == 0: rows of 16 bytes)
    s.psmall = H1 + H2 * H1 + 2 * H2 + 1;
    s.pitchB = mlp_pitch(s.psmall);
    s.offB = (size_t)s.gr * s.pitchA * sizeof(float);
    s.offH = s.offB + (size_t)s.g1 * s.pitchB * sizeof(float);
    s.bytes = s.offH + (size_t)s.tiles * kMsRows * mlp_bigwide_dh(H1) * sizeof(float);
    return s;
}

struct MlpBigWideHost {
    static constexpr int kAlign = 4, kMaxF = kBwMaxF, kMaxH1 = kBgH1, kMaxH2 = kBgH2;
    static int grid(long long rows, int, bool) { return mlp_stream_grid(rows, 1); }
    static MlpBigWidePlan plan(long long rows, int F, int H1, int H2)
    {
        const int NT = (F + 15) >> 4;
        const int nsl = (NT + 10) / 11;
        return mlp_bigwide_plan_of(rows, F, H1, H2, nsl, (NT + nsl - 1) / nsl <= 8 ? 8 : 11);
    }
    template <bool GRAD>
    static int launch(const MlpStreamParams &p, int grid, hipStream_t stream)
    {
        const size_t lds = mlp_bigwide_fwd_lds_bytes(GRAD);
        LTR_ENSURE_LDS((mlp_bigwide_fwd_kernel<GRAD>), lds);
        hipLaunchKernelGGL((mlp_bigwide_fwd_kernel<GRAD>), dim3((unsigned)grid), dim3(kBgThreads), lds, stream, p);
        return (int)hipGetLastError();
    }
    template <int NTS>
    static int launch_dw1_nts(const MlpStreamParams &p, const MlpBigWidePlan &s, hipStream_t stream)
    {
        const size_t lds = mlp_bigwide_dw1_lds_bytes(NTS);
        LTR_ENSURE_LDS((mlp_bigwide_dw1_kernel<NTS>), lds);
        hipLaunchKernelGGL((mlp_bigwide_dw1_kernel<NTS>), dim3((unsigned)(s.gr * s.nsl)), dim3(kBgThreads), lds, stream, p,
                           s.nsl);
        return (int)hipGetLastError();
    }
    static int launch_dw1(const MlpStreamParams &p, const MlpBigWidePlan &s, hipStream_t stream)
    {
        return s.nts == 8 ? launch_dw1_nts<8>(p, s, stream) : launch_dw1_nts<11>(p, s, stream);
    }
};

// The gradient entry points of a front.  Host: kAlign, kMaxF, kMaxH1, kMaxH2, plan(rows, F, H1, H2), launch<true>(p, grid,
// stream), launch_dw1(p, plan, stream)
template <class Host>
size_t mlp_bigwide_grad_workspace_bytes(int B, int L, int F, int H1, int H2)
{
    if (B <= 0 || mlp_stream_bad_shape(B, L, F, H1, H2, Host::kAlign, Host::kMaxF, Host::kMaxH1, Host::kMaxH2)) return 0;
    return Host::plan((long long)B * L, F, H1, H2).bytes;
}

template <class Host>
int mlp_bigwide_grad(const void *X, const float *W1, const float *b1, const float *W2, const float *b2, const float *W3,
                     const float *b3, const float *g, const int64_t *n, int B, int L, int F, int H1, int H2,
                     float *grads, void *workspace, size_t workspace_bytes, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (mlp_stream_bad_shape(B, L, F, H1, H2, Host::kAlign, Host::kMaxF, Host::kMaxH1, Host::kMaxH2)) return LTR_ERR_SHAPE;
    if (!W1 || !b1 || !W2 || !b2 || !W3 || !b3 || !grads) return LTR_ERR_NULL;
    const int P = mlp_param_count(F, H1, H2);
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) return mlp_reduce_launch(nullptr, 0, P, grads, nullptr, 0, nullptr, st);     // zero gradients
    if (!X || !g) return LTR_ERR_NULL;
    const MlpBigWidePlan s = Host::plan((long long)B * L, F, H1, H2);
    if (!workspace || workspace_bytes < s.bytes) return LTR_ERR_WORKSPACE;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    MlpStreamParams p = mlp_stream_params(X, W1, b1, W2, b2, W3, b3, g, n, B, L, F, H1, H2);
    p.dH1 = reinterpret_cast<float *>(ws + s.offH);
    // forward and back down to dH1; the small sums, one partial vector per workgroup
    p.part = reinterpret_cast<float *>(ws + s.offB); p.pitch = s.pitchB;
    int rc = Host::template launch<true>(p, s.g1, st);
    if (rc != 0) return rc;
    // dW1, one partial matrix per row range
    p.part = reinterpret_cast<float *>(ws); p.pitch = s.pitchA;
    rc = Host::launch_dw1(p, s, st);
    if (rc != 0) return rc;
    // grads = [dW1 | the small sums]: both sums in a fixed order (H1 * F floats are whole 16-byte units)
    rc = mlp_reduce_launch(ws, s.gr, s.pitchA, grads, nullptr, 0, nullptr, st);
    if (rc != 0) return rc;
    return mlp_reduce_launch(ws + s.offB, s.g1, s.psmall, grads + s.pitchA, nullptr, 0, nullptr, st);
}

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

extern "C" {

int ltr_mlp_bigwide_scores_f32(const float *X, const float *W1, const float *b1, const float *W2, const float *b2,
                               const float *W3, const float *b3, const int64_t *n, int B, int L, int F, int H1, int H2,
                               float *scores_out, void *stream)
{
    return mlp_stream_scores<MlpBigWideHost>(X, W1, b1, W2, b2, W3, b3, n, B, L, F, H1, H2, scores_out, stream);
}

size_t ltr_mlp_bigwide_grad_workspace_bytes(int B, int L, int F, int H1, int H2)
{
    return mlp_bigwide_grad_workspace_bytes<MlpBigWideHost>(B, L, F, H1, H2);
}

int ltr_mlp_bigwide_grad_f32(const float *X, const float *W1, const float *b1, const float *W2, const float *b2,
                             const float *W3, const float *b3, const float *g, const int64_t *n, int B, int L, int F,
                             int H1, int H2, float *grads, void *workspace, size_t workspace_bytes, void *stream)
{
    return mlp_bigwide_grad<MlpBigWideHost>(X, W1, b1, W2, b2, W3, b3, g, n, B, L, F, H1, H2, grads, workspace,
                                            workspace_bytes, stream);
}

}  // extern "C"
