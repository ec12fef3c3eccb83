// ltr_mlp_big.inc -- the stand-alone ReLU-MLP scorer (F -> H1 -> H2 -> 1) with WIDE HIDDEN LAYERS: H1 <= 256, H2 <= 64,
// f32 rows of at most 144 features, lists of any length (include/ltr_mlp_big.h).  Score and parameter-gradient kernels
// on v_mfma_f32_16x16x4_f32.  Included by ltr_mlp.hip behind ltr_mlp_stream.inc, whose ring, row test, dW1 chain and host
// glue it uses; the kernel body is its own: the four-wave tile of mlp_stream_body keeps one 16-row hidden-1 block per wave
// and one hidden-2 fragment, which cannot be stretched to 16 + 4 blocks.
//
// One workgroup of EIGHT waves per CU (two per SIMD, 256 registers a wave), a tile of 32 flat rows, a persistent grid.
//   Hidden 1.  Wave w owns the 16-row blocks w and w + 8 (so a 128-wide layer gives every wave one block, not half of the
//     waves two): their W1 fragments (2 NT float4) and, in the gradient kernel, their dW1 tiles (2 NT float4) and the
//     dW2 columns of those rows (4 x 2 float4) live in registers for the workgroup's whole life: 72 + 72 + 32 at F = 144.
//   W2 lives in LDS once, [64][272]: layer 2 reads its rows as 16-byte A fragments, the backward reads the same image
//     transposed (4-byte reads, lane groups 16 banks apart) as the A operand of dH1 = W2^T . dH2 -- no second copy.
//   Layer 2 without a cross-wave sum.  The ReLU'd hidden-1 tile goes to LDS once, [32][272]; behind one barrier the waves
//     are re-dealt as 4 hidden-2 blocks x 2 row subtiles (block w & 3, subtile w >> 2), each running ONE K = H1 chain
//     with both operands read as 16 bytes.  Layer 3 is the 64-long dot: a wave folds its 16 rows by two lane exchanges,
//     the four blocks meet in LDS and 32 lanes add them in a fixed order.
//   Backward.  g is known up front, so the layer-2 wave turns its H2 fragment straight into dH2 rows (LDS [32][68]) and
//     its db2 / dW3 / db3 sums; behind the next barrier the hidden-1 owners run, from the same LDS images,
//         dW2[:, own rows] += dH2^T . H1            (K = the tile's documents)
//         dH1 = W2^T . dH2 . [H1 > 0]               written IN PLACE over the wave's own columns of the H1 tile
//         dW1[own rows]   += dH1^T . X              (mlp_dw1_chain_f32, B = image columns)
//     -- the own columns of the H1 tile are read and written by their owner WAVE only, so no barrier separates the
//     three.  The dependence is cross-lane inside that wave: the dH1 cells one lane writes (16 bytes, document-major)
//     are read back transposed by other lanes as the A operand of dW1, and dW2 reads the H1 values before dH1 replaces
//     them.  That rests on the DS instructions of one wave executing in order, and on the compiler keeping every store
//     in front of the loads behind it -- all of them go through the one pointer `own`, so it has to assume they alias.
//     An edit that splits `own` into provably distinct pointers (or marks them __restrict__) loses that order.
//   Work that is not there is skipped, uniformly: 16-row blocks past H1 (in layer 1, in the K loops and in the
//     backward) and past H2, subtiles of padding only, tiles of padding only (barrier A alone).
// The feed is mlp_stream_body's, restated for 512 threads: 16-byte unconditional loads one tile ahead, a padded row's
// lanes redirected to the head of W1 and zeroed on the way into the image, row masks and g two tiles ahead in the
// three-slot ring (mlp_ring_write).  One partial vector per workgroup, mlp_reduce_launch adds them: no atomics.
// The kernel body is mlp_big_body<Front, GRAD>: what depends on the element type of X (the image, the W1 fragments,
// layer 1, the dW1 step) comes from a front -- MlpBigFrontF32<NT> below, under the kernel names mlp_big_kernel<NT, GRAD>;
// MlpBigFrontBf16<KS> in ltr_mlp_bigbf16.inc -- and everything from the store of the H1 tile to the dH1 write exists once.
// DESIGN.md section 32 has the design answers, the resource table and the measurements.
#pragma once

#include "ltr_mlp_big.h"

// The device code of this file is compiled without the packed fp32 instructions, as ltr_mlp2_bf16.inc is: the helpers
// inlined into the kernels below are selected as plain fp32 operations here and keep their code everywhere else.
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

constexpr int kBgThreads = 512;
constexpr int kBgWaves = 8;
constexpr int kBgH1 = 256;           // hidden-1 rows: 16 blocks, two per wave
constexpr int kBgH2 = 64;            // hidden-2 rows: 4 blocks, one per layer-2 wave of a subtile
constexpr int kBgMaxNT = 9;          // feature buckets (F <= 144): the gradient kernel's W1 + dW1 + dW2 fill 176 registers
constexpr int kBgMaxF = 16 * kBgMaxNT;
constexpr int kBgHP = kBgH1 + 16;    // row pitch (floats) of the H1 tile and of W2: 16-byte rows, 16 banks between lane groups
constexpr int kBgDP = kBgH2 + 4;     // row pitch of the dH2 rows
constexpr int kBgSums = kBgH1 + 4 * kBgH2 + 4;   // LDS sums across the tiles: [256] db1 | [2][64] db2 | [2][64] dW3 | [2] db3

// LDS floats behind the image [32][16 NT + 4].  One carve for both kernels: the score kernel never touches the dH2 rows
// (8.7 KB) nor the sums at the end (2 KB, the last region: its request leaves them out); at one workgroup per CU
// neither costs it anything.
constexpr size_t kBgFixedFloats = (size_t)kMsRows * kBgHP + (size_t)kBgH2 * kBgHP + (size_t)kMsRows * kBgDP +
                                  4 * kMsRows + kBgH1 + 2 * kBgH2 + kMsRing * kMsRows + 4;
__host__ __device__ constexpr size_t mlp_big_lds_bytes_of(size_t image_bytes, bool grad)
{
    return image_bytes + (kBgFixedFloats + (grad ? kBgSums : 0)) * sizeof(float);
}
__host__ __device__ constexpr size_t mlp_big_lds_bytes(int NT, bool grad)
{
    return mlp_big_lds_bytes_of((size_t)kMsRows * (16 * NT + 4) * sizeof(float), grad);
}
static_assert(mlp_big_lds_bytes(kBgMaxNT, true) <= kLdsBudget, "one workgroup per CU");

// whether the W1 fragments stay in registers: not in the gradient kernel of the widest bucket
constexpr bool mlp_big_w1_regs(int NT, bool grad) { return !(grad && NT > 5); }

// ---- the f32 FRONT of mlp_big_body: what depends on the element type of X -- the image, the W1 fragments, layer 1 and
//      the dW1 step of one hidden-1 block (the bf16 one: MlpBigFrontBf16, ltr_mlp_bigbf16.inc) ----
template <int NT>
struct MlpBigFrontF32 {
    typedef float elem;
    typedef mlp_f4 w1frag;                          // W1[j1A][16c + 4g .. +3]
    static constexpr int EU = 4;                    // elements per 16 bytes
    static constexpr int IP = 16 * NT + 4;          // image pitch (elements)
    static constexpr int FU = 4 * NT;               // 16-byte units of the widest row
    static constexpr int NW1 = NT;                  // W1 fragments of a block
    static constexpr int NC = NT;                   // dW1 chunks of 16 features
    static constexpr bool w1_regs(bool grad) { return mlp_big_w1_regs(NT, grad); }
    static constexpr size_t lds_bytes(bool grad) { return mlp_big_lds_bytes(NT, grad); }

    // W1 fragments of the block whose A-operand row of this lane is j1A: zeros past H1 / F
    static __device__ __forceinline__ void load_w1(w1frag (&wf)[NT], const MlpStreamParams &p, int j1A, int g)
    {
#pragma unroll
        for (int c = 0; c < NT; ++c) {
            const int f0 = 16 * c + 4 * g;
            const bool ok = j1A < p.H1 && f0 < p.F;
            const mlp_f4 v = *reinterpret_cast<const mlp_f4 *>(p.W1 + (ok ? (size_t)j1A * p.F + f0 : 0));
#pragma unroll
            for (int i = 0; i < 4; ++i) wf[c][i] = ok ? v[i] : 0.f;
        }
    }
    // h[u] += W1 block . X^T over subtiles u0 .. u0 + NS - 1 of the image
    template <int NS>
    static __device__ __forceinline__ void layer1(mlp_f4 (&h)[NS], const w1frag (&wf)[NT], const float *img, int u0,
                                                  int c16, int g)
    {
        const float *bsrc = img + (16 * u0 + c16) * IP + 4 * g;
        // (one chunk of B fragments ahead, and a scheduling fence per chunk: left alone, the scheduler requests the
        // fragments of all NT chunks in front of the first MFMA -- 8 NT registers the gradient kernel does not have)
        mlp_f4 xb[NS], xn[NS];
#pragma unroll
        for (int u = 0; u < NS; ++u) xb[u] = *reinterpret_cast<const mlp_f4 *>(bsrc + 16 * u * IP);
#pragma unroll
        for (int c = 0; c < NT; ++c) {
#pragma unroll
            for (int u = 0; u < NS; ++u)
                if (c + 1 < NT) xn[u] = *reinterpret_cast<const mlp_f4 *>(bsrc + 16 * u * IP + 16 * (c + 1));
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int u = 0; u < NS; ++u) h[u] = mfma16(wf[c][i], xb[u][i], h[u]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < NS; ++u) xb[u] = xn[u];
        }
    }
    // layer 1 where the fragments do not stay in registers: the block's are fetched again, then the chain above
    template <int NS>
    static __device__ __forceinline__ void layer1_refetch(mlp_f4 (&h)[NS], const MlpStreamParams &p, int j1A,
                                                          const float *img, int u0, int c16, int g)
    {
        w1frag wt[NT];
        load_w1(wt, p, j1A, g);
        layer1<NS>(h, wt, img, u0, c16, g);
    }
    // dW1[block] += dH1^T . X over the documents of subtiles u0 .. u0 + NS - 1: A = the dH1 columns the wave has just
    // written through `own` (document 4s + g), B = image columns
    template <int NS>
    static __device__ __forceinline__ void dw1(mlp_f4 (&acc)[NT], const float *img, const float *own, int u0, int c16,
                                               int g)
    {
        const int d0 = 16 * u0;
        float a1[4 * NS];
#pragma unroll
        for (int s = 0; s < 4 * NS; ++s) a1[s] = own[(d0 + 4 * s + g) * kBgHP + c16];
        const float *xsrc = img + (d0 + g) * IP + c16;
#pragma unroll
        for (int c = 0; c < NT; ++c) {                 // (a fence per chunk, as in layer 1)
#pragma unroll
            for (int s = 0; s < 4 * NS; ++s) acc[c] = mfma16(a1[s], xsrc[4 * s * IP + 16 * c], acc[c]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
};

// ---- the kernel body under both fronts.  Front: elem (type of X), EU (elements per 16 bytes), IP (image pitch,
//      elements), FU (16-byte units of the widest row), NW1 / w1frag / load_w1 / w1_regs, layer1<NS>, NC / dw1<NS>,
//      lds_bytes.  Everything between the store of the H1 tile and the dH1 write is here, once ----
template <class Front, bool GRAD>
__device__ __forceinline__ void mlp_big_body(const MlpStreamParams &p)
{
    typedef typename Front::elem elem;
    typedef typename Front::w1frag w1frag;
    constexpr bool W1R = Front::w1_regs(GRAD);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int T = kBgThreads, EU = Front::EU, IP = Front::IP, NW1 = Front::NW1, NC = Front::NC, HP = kBgHP, DP = kBgDP;
    constexpr int KP = (kMsRows * Front::FU + T - 1) / T;           // 16-byte units of a fill per thread
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    int c16 = lane & 15, g = lane >> 4;             // (not const: see the top of the tile loop)
    const int F = p.F, H1 = p.H1, H2 = p.H2;
    const int C = F >> (EU == 8 ? 3 : 2);           // 16-byte units per feature row
    const int nb1 = (H1 + 15) >> 4, nb2 = (H2 + 15) >> 4;          // 16-row blocks of the two hidden layers
    const int nh = (w < nb1 ? 1 : 0) + (w + 8 < nb1 ? 1 : 0);      // hidden-1 blocks of this wave: w, w + 8
    const int jb = w & 3, ju = w >> 2;              // layers 2 / 3: hidden-2 block and row subtile of this wave

    elem *img = reinterpret_cast<elem *>(smem);                    // [32][IP]   feature rows of the fill
    float *h1s = reinterpret_cast<float *>(img + (size_t)kMsRows * IP);        // [32][HP]   H1 tile, document-major; later dH1
    float *w2s = h1s + (size_t)kMsRows * HP;                       // [64][HP]   W2, zeros past (H2, H1)
    float *dH2s = w2s + (size_t)kBgH2 * HP;                        // [32][DP]
    float *sp = dH2s + (size_t)kMsRows * DP;                       // [4][32]    layer-3 partial dots per hidden-2 block
    float *b1s = sp + 4 * kMsRows;                                 // [256] b1 | [64] b2 | [64] W3, zeros past H1 / H2
    float *b2s = b1s + kBgH1, *w3s = b2s + kBgH2;
    float *gs = w3s + kBgH2;                                       // [3][32]    d loss / d score of the tile's rows
    unsigned *vmask = reinterpret_cast<unsigned *>(gs + kMsRing * kMsRows);    // [3] bit r: row r of the tile is real
    // the small sums of the gradient kernel, added to once per tile by the one wave that owns an entry (db2 / dW3 / db3:
    // one copy per row subtile, i.e. per layer-2 wave) -- in LDS, not in 17 registers the widest bucket does not have
    float *db1s = gs + kMsRing * kMsRows + 4;                      // [256]
    float *db2s = db1s + kBgH1, *dw3s = db2s + 2 * kBgH2, *db3s = dw3s + 2 * kBgH2;     // [2][64], [2][64], [2]

    const mlp_f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const mlp_i4 zero4i = {0, 0, 0, 0};

    // ---- W1 fragments of block w + 8 hb (Front::load_w1, A-operand row 16 (w + 8 hb) + c16), zeros past H1 / F.  W1R:
    //      both blocks' stay in registers; else (the widest gradient buckets: registers they do not have next to dW1 and
    //      dW2) layer 1 fetches a block's fragments again for every tile -- f32: 147 KB per tile at (256, 144) -- from
    //      the L2 ----
    w1frag w1r[W1R ? 2 : 1][NW1];
    if constexpr (W1R) {
        Front::load_w1(w1r[0], p, 16 * w + c16, g);
        Front::load_w1(w1r[1], p, 16 * (w + 8) + c16, g);
    }
    const float b3 = p.b3[0];

    // ---- accumulators that live across the tiles ----
    mlp_f4 acc[2][GRAD ? NC : 1];    // dW1[16 (w + 8 hb) + 4g + i][16c + c16]
    mlp_f4 accW2[4][2];              // dW2[16 jb + 4g + i][16 (w + 8 hb) + c16]
#pragma unroll
    for (int hb = 0; hb < 2; ++hb) {
#pragma unroll
        for (int c = 0; c < (GRAD ? NC : 1); ++c) acc[hb][c] = zero4;
#pragma unroll
        for (int b = 0; b < 4; ++b) accW2[b][hb] = zero4;
    }

    // ---- the fill (mlp_stream_body's, 512 threads): unit k of this thread is 16-byte unit u = tid + 512 k of the tile's
    //      rows in memory, row ur[k] = u / C of the tile (>= 32: past the tile), image element EU u + ur[k] (IP - EU C) ----
    int ur[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) ur[k] = (tid + k * T) / C;
    mlp_i4 P[KP];
    auto issue_fill = [&](int tile, unsigned m) {
        const elem *Xt = static_cast<const elem *>(p.X) + (size_t)tile * kMsRows * (size_t)F;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const bool ok = ur[k] < kMsRows && ((m >> (ur[k] & 31)) & 1u);
            // (a padded row is never read: its lanes fetch the first 16 bytes of W1 and drop them)
            const void *src = ok ? (const void *)(Xt + EU * (size_t)(tid + k * T)) : (const void *)p.W1;
            P[k] = *reinterpret_cast<const mlp_i4 *>(src);
        }
    };
    auto fill_image = [&](unsigned m) {
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const bool ok = (m >> (ur[k] & 31)) & 1u;
            const mlp_i4 v = ok ? P[k] : zero4i;
            if (ur[k] < kMsRows) *reinterpret_cast<mlp_i4 *>(img + EU * (tid + k * T) + ur[k] * (IP - EU * C)) = v;
        }
    };

    // ---- layer 1 over subtiles u0 .. u0 + NS - 1: ReLU'd rows of the wave's blocks -> H1 tile ----
    auto layer1 = [&](auto ns_c, int u0) {
        constexpr int NS = decltype(ns_c)::value;
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
            if (hb < nh) {
                const int j0 = 16 * (w + 8 * hb);
                const mlp_f4 b1v = *reinterpret_cast<const mlp_f4 *>(b1s + j0 + 4 * g);
                mlp_f4 h[NS];
#pragma unroll
                for (int u = 0; u < NS; ++u) h[u] = b1v;
                if constexpr (W1R) Front::template layer1<NS>(h, w1r[hb], img, u0, c16, g);
                else Front::template layer1_refetch<NS>(h, p, j0 + c16, img, u0, c16, g);
#pragma unroll
                for (int u = 0; u < NS; ++u) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) h[u][i] = fmaxf(h[u][i], 0.f);
                    *reinterpret_cast<mlp_f4 *>(h1s + (16 * (u0 + u) + c16) * HP + j0 + 4 * g) = h[u];
                }
            }
        }
    };
    // ---- layers 2 and 3 of hidden-2 block jb on the 16 documents of subtile ju: one K = H1 chain, A = W2 rows, B = H1
    //      rows, 16 bytes each; score kernel: the block's share of the dot -> sp; gradient kernel: dH2 rows -> LDS ----
    auto layer23 = [&](int slot) {
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
            const float ds = gs[slot * kMsRows + doc];             // (0 on a padded row)
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
    // ---- hidden-1 owner, backward over subtiles u0 .. u0 + NS - 1 (documents d0 .. d0 + 16 NS - 1) ----
    auto bwd = [&](auto ns_c, int u0) {
        constexpr int NS = decltype(ns_c)::value;
        const int d0 = 16 * u0;
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
            if (hb < nh) {
                const int j0 = 16 * (w + 8 * hb);
                float *own = h1s + j0;                             // this block's columns of the H1 tile
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
                // dH1^T block = (W2^T . dH2^T) . [H1 > 0], over the H1 values it masks with: A = W2 read transposed
                // (hidden-2 row 4t + g), B = dH2 rows
                {
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
                        mlp_f4 *cell = reinterpret_cast<mlp_f4 *>(own + (d0 + 16 * u + c16) * HP + 4 * g);
                        const mlp_f4 hv = *cell;
#pragma unroll
                        for (int i = 0; i < 4; ++i) d1[u][i] = (hv[i] > 0.f) ? d1[u][i] : 0.f;
                        *cell = d1[u];
                    }
                    mlp_f4 s1;
#pragma unroll
                    for (int i = 0; i < 4; ++i) s1[i] = row16_sum(NS == 2 ? d1[0][i] + d1[NS - 1][i] : d1[0][i]);
                    if (c16 == 0) *reinterpret_cast<mlp_f4 *>(db1s + j0 + 4 * g) += s1;
                }
                // dW1[block] += dH1^T . X: A = the dH1 columns just written, B = image columns (Front::dw1)
                // (cells written by OTHER lanes of this wave: in-order DS, and stores and loads through `own` alike)
                if constexpr (GRAD) Front::template dw1<NS>(acc[hb], img, own, u0, c16, g);
            }
        }
    };

    // ---- prologue: masks of the first two tiles, the weights' LDS images, the first fill ----
    const int G = (int)gridDim.x;
    int tile = (int)blockIdx.x;
    mlp_ring_write<GRAD>(p, tid, tile, 0, vmask, gs);
    mlp_ring_write<GRAD>(p, tid, tile + G, 1, vmask, gs);
    // the feature columns F .. IP - 1 of the image are never written by a fill: zero them once
    for (int i = tid; i < kMsRows * (IP - EU * C); i += T) {
        const int r = i / (IP - EU * C), cc = i - r * (IP - EU * C);
        img[r * IP + EU * C + cc] = 0;
    }
    for (int i = tid; i < kBgH2 * kBgH1; i += T) {                 // W2 over the blocks in use, zeros past (H2, H1)
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
        for (int i = tid; i < kBgSums; i += T) db1s[i] = 0.f;
    __syncthreads();
    issue_fill(tile, __builtin_amdgcn_readfirstlane(vmask[0]));

    int slot = 0;
    for (; tile < p.tiles; tile += G) {
        // Opaque lane indices keep the address arithmetic of the chains inside the loop: hoisted in front of it, the LDS
        // addresses of every phase live across all the others, next to 176 registers of W1, dW1 and dW2 (ltr_mlp2.inc)
        asm volatile("" : "+v"(c16), "+v"(g));
        const int slot1 = mlp_ring_next(slot), slot2 = mlp_ring_next(slot1);
        // (both masks were written in front of a barrier every wave has passed; the slot rewritten below was last read in
        // front of the last barrier of the iteration before: mlp_stream_body)
        const unsigned m = __builtin_amdgcn_readfirstlane(vmask[slot]);
        const unsigned mnext = __builtin_amdgcn_readfirstlane(vmask[slot1]);
        fill_image(m);                             // (waits for the fill in P; every wave is past the image's readers)
        issue_fill(tile + G, mnext);               // (past the last tile: mask 0, nothing of X is requested)
        mlp_ring_write<GRAD>(p, tid, tile + 2 * G, slot2, vmask, gs);
        lds_barrier();                             // A: image filled
        const bool act0 = (m & 0xFFFFu) != 0, act1 = (m >> 16) != 0;        // subtiles with a real row (uniform)
        const int u0 = act0 ? 0 : 1;
        if (m != 0) {
            if (act0 && act1) layer1(m2_ns<2>{}, 0);
            else layer1(m2_ns<1>{}, u0);
            lds_barrier();                         // B: H1 tile
            if (jb < nb2 && (ju == 0 ? act0 : act1)) layer23(slot);
            lds_barrier();                         // C: score shares / dH2 rows
            if constexpr (GRAD) {
                if (act0 && act1) bwd(m2_ns<2>{}, 0);
                else bwd(m2_ns<1>{}, u0);
                lds_barrier();                     // D: image, H1 tile and dH2 rows free
            }
        }
        if constexpr (!GRAD) {
            // (the shares are rewritten behind barrier B of the next tile, which this wave has to reach)
            const long long orow = (long long)tile * kMsRows + tid;
            if (tid < kMsRows && orow < (long long)p.rows) {
                float s = 0.f;
                if ((m >> tid) & 1u) {
                    s = b3;
                    for (int b = 0; b < nb2; ++b) s += sp[b * kMsRows + tid];
                }
                p.scores_out[orow] = s;
            }
        }
        slot = slot1;
    }
    if constexpr (GRAD) {
        // ---- this workgroup's partial vector [dW1 | db1 | dW2 | db2 | dW3 | db3] ----
        float *dst = p.part + (size_t)blockIdx.x * p.pitch;
        const int oB1 = H1 * F, oW2 = oB1 + H1, oB2 = oW2 + H2 * H1, oW3 = oB2 + H2, oB3 = oW3 + H2;
        __syncthreads();                           // (the image of the last tile is behind every wave)
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
            if (hb < nh) {
                const int j0 = 16 * (w + 8 * hb);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int j1 = j0 + 4 * g + i;
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        const int f = 16 * c + c16;
                        if (j1 < H1 && f < F) dst[(size_t)j1 * F + f] = acc[hb][c][i];
                    }
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int j2 = 16 * b + 4 * g + i;
                        if (j2 < H2 && j0 + c16 < H1) dst[oW2 + j2 * H1 + j0 + c16] = accW2[b][hb][i];
                    }
                }
            }
        }
        // the small sums: the two subtiles' copies in a fixed order (the last barrier of the loop is behind every wave)
        if (tid < H1) dst[oB1 + tid] = db1s[tid];
        if (tid < H2) {
            dst[oB2 + tid] = db2s[tid] + db2s[kBgH2 + tid];
            dst[oW3 + tid] = dw3s[tid] + dw3s[kBgH2 + tid];
        }
        if (tid == 0) dst[oB3] = db3s[0] + db3s[1];
    }
}

template <int NT, bool GRAD>
__global__ void __launch_bounds__(kBgThreads, 1)
mlp_big_kernel(MlpStreamParams p)
{
    mlp_big_body<MlpBigFrontF32<NT>, GRAD>(p);
}

// ---- host side ----
struct MlpBigHost {
    static constexpr int kAlign = 4, kMaxF = kBgMaxF, kMaxH1 = kBgH1, kMaxH2 = kBgH2;
    static int grid(long long rows, int, bool) { return mlp_stream_grid(rows, 1); }
    template <int NT, bool GRAD>
    static int launch_nt(const MlpStreamParams &p, int grid, hipStream_t stream)
    {
        const size_t lds = mlp_big_lds_bytes(NT, GRAD);
        LTR_ENSURE_LDS((mlp_big_kernel<NT, GRAD>), lds);
        hipLaunchKernelGGL((mlp_big_kernel<NT, GRAD>), dim3((unsigned)grid), dim3(kBgThreads), lds, stream, p);
        return (int)hipGetLastError();
    }
    template <bool GRAD>
    static int launch(const MlpStreamParams &p, int grid, hipStream_t stream)
    {
        switch (mlp_bucket(p.F)) {
        case 3: return launch_nt<3, GRAD>(p, grid, stream);
        case 5: return launch_nt<5, GRAD>(p, grid, stream);
        default: return launch_nt<9, GRAD>(p, grid, stream);
        }
    }
};

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

extern "C" {

int ltr_mlp_big_scores_f32(const float *X, const float *W1, const float *b1, const float *W2, const float *b2,
                           const float *W3, const float *b3, const int64_t *n, int B, int L, int F, int H1, int H2,
                           float *scores_out, void *stream)
{
    return mlp_stream_scores<MlpBigHost>(X, W1, b1, W2, b2, W3, b3, n, B, L, F, H1, H2, scores_out, stream);
}

size_t ltr_mlp_big_grad_workspace_bytes(int B, int L, int F, int H1, int H2)
{
    return mlp_stream_grad_workspace_bytes<MlpBigHost>(B, L, F, H1, H2);
}

int ltr_mlp_big_grad_f32(const float *X, const float *W1, const float *b1, const float *W2, const float *b2,
                         const float *W3, const float *b3, const float *g, const int64_t *n, int B, int L, int F,
                         int H1, int H2, float *grads, void *workspace, size_t workspace_bytes, void *stream)
{
    return mlp_stream_grad<MlpBigHost>(X, W1, b1, W2, b2, W3, b3, g, n, B, L, F, H1, H2, grads, workspace,
                                       workspace_bytes, stream);
}

}  // extern "C"
