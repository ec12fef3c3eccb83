// ltr_mlp_bf16.inc -- the stand-alone ReLU-MLP scorer (F -> H1 -> H2 -> 1) on a bf16 feature batch: the row-streaming
// score and parameter-gradient kernels of ltr_mlp_rows.inc with the first layer, and the dW1 product, on
// v_mfma_f32_16x16x32_bf16 (include/ltr_mlp_bf16.h).  Included by ltr_mlp.hip behind ltr_mlp_rows.inc, whose tile, ring,
// owner waves, partial vectors and reduction it shares.
//
// What is the same as in ltr_mlp_rows.inc: a tile is 32 consecutive flat rows of the (B * L, F) matrix, a row is real
// iff row % L < n[row / L]; four waves, wave w owns hidden-1 rows 16w .. 16w+15; barriers A - D; a persistent grid whose
// workgroup w takes the tiles w, w + G, ... and writes one partial vector that mlp_reduce_launch(loss = NULL) adds in a
// fixed order; unconditional 16-byte loads whose padded rows fetch the head of W1 and become zeros in the image.
// Layers 2 and 3, the biases, the ReLUs, dW2, dH1, db* and dW3 are the f32 code of that file, unchanged.
//
// What differs:
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
typedef __attribute__((ext_vector_type(4))) int mb_i4;

constexpr int kMbMaxKS = 7;          // 224 features

struct MlpBf16Params {
    const uint16_t *X;
    const float *W1, *b1, *W2, *b2, *W3, *b3, *g;
    const int64_t *n;
    float *scores_out, *part;
    int B, L, F, H1, H2;
    int rows;                        // B * L
    int tiles;                       // ceil(rows / 32)
    int pitch;                       // floats between consecutive partial vectors
};

__host__ __device__ constexpr size_t mlp_bf16_lds_bytes(int KS, bool grad)
{
    const size_t IPH = (size_t)32 * KS + 8;              // image pitch, bf16 elements
    const size_t loop = kMrRows * IPH * 2 + ((size_t)kMrWaves * kMrRows * kMrPS + (size_t)kMrRows * kMrPS +
                                             (size_t)kMrRing * kMrRows + 4) * sizeof(float);
    // the gradient kernel stages its four dW1 tiles (64 rows of 32 KS + 4 floats) and the fold of the small sums
    const size_t tail = grad ? (64 * ((size_t)32 * KS + 4) + (size_t)kMrWaves * 40) * sizeof(float) : 0;
    return loop > tail ? loop : tail;
}
static_assert(mlp_bf16_lds_bytes(kMbMaxKS, true) <= kLdsBudget / kMrWgs, "two workgroups per CU");

template <int KS, bool GRAD>
__global__ void __launch_bounds__(kMrThreads, kMrWgs)
mlp_bf16_kernel(MlpBf16Params p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    constexpr int T = kMrThreads;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15;
    const int g = lane >> 4;
    const int L = p.L, F = p.F, H1 = p.H1, H2 = p.H2;
    const int C = F >> 3;                           // 16-byte units (8 bf16) per feature row
    constexpr int IPH = 32 * KS + 8;                // image pitch (bf16 elements)
    constexpr int IPF = 32 * KS + 4;                // pitch (floats) of the dW1 staging at the end
    constexpr int NC = 2 * KS;                      // dW1 chunks of 16 features
    constexpr int KP = (kMrRows * 4 * KS + T - 1) / T;      // 16-byte units of a fill per thread

    uint16_t *img = reinterpret_cast<uint16_t *>(smem);            // [32][IPH]  feature rows of the fill, bf16
    float *part = reinterpret_cast<float *>(img + (size_t)kMrRows * IPH);      // [4][32][20] layer-2 partials, later
    float *scr = part + (size_t)w * kMrRows * kMrPS;               //            this wave's transposition scratch
    float *dH2s = part + (size_t)kMrWaves * kMrRows * kMrPS;       // [32][20]
    float *gs = dH2s + (size_t)kMrRows * kMrPS;                    // [3][32]    d loss / d score of the tile's rows
    unsigned *vmask = reinterpret_cast<unsigned *>(gs + kMrRing * kMrRows);    // [3] bit r: row r of the tile is real

    const mlp_f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const mb_i4 zero4i = {0, 0, 0, 0};

    // ---- this wave's weight fragments: W1 rounded to bf16 here, once; the rest as in ltr_mlp_rows.inc ----
    const int j1A = 16 * w + c16;                   // hidden-1 row as an A-operand row (lane & 15)
    mb_bf8 w1r[KS];                                 // bf16(W1[j1A][32s + 8g .. +7])
    mlp_f4 b1v, w2a, w2t, b2v, w3v;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int f0 = 32 * s + 8 * g;
        const bool ok = j1A < H1 && f0 < F;         // (F % 8 == 0: all eight or none)
        const float *src = p.W1 + (ok ? (size_t)j1A * F + f0 : 0);
        const mlp_f4 v0 = *reinterpret_cast<const mlp_f4 *>(src);
        const mlp_f4 v1 = *reinterpret_cast<const mlp_f4 *>(src + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            w1r[s][i] = (__bf16)(ok ? v0[i] : 0.f);
            w1r[s][4 + i] = (__bf16)(ok ? v1[i] : 0.f);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j1D = 16 * w + 4 * g + i;         // hidden-1 row as a D-fragment row
        const int j2D = 4 * g + i;                  // hidden-2 row as a D-fragment row
        const bool ok1 = j1D < H1, ok2 = j2D < H2;
        const float vb1 = p.b1[ok1 ? j1D : 0];
        b1v[i] = ok1 ? vb1 : 0.f;
        const bool oka = c16 < H2 && ok1;           // layer 2:  A[row j2 = c16][k <-> j1D]
        const float va = p.W2[oka ? (size_t)c16 * H1 + j1D : 0];
        w2a[i] = oka ? va : 0.f;
        const bool okt = ok2 && j1A < H1;           // dH1:      A[row j1A][k <-> j2D]
        const float vt = p.W2[okt ? (size_t)j2D * H1 + j1A : 0];
        w2t[i] = okt ? vt : 0.f;
        const float vb2 = p.b2[ok2 ? j2D : 0], v3 = p.W3[ok2 ? j2D : 0];
        b2v[i] = ok2 ? vb2 : 0.f;
        w3v[i] = ok2 ? v3 : 0.f;
    }
    const float b3 = p.b3[0];

    // ---- accumulators that live across the tiles (disjoint between the waves) ----
    mlp_f4 acc[GRAD ? NC : 1];       // dW1[j1 = 16w+4g+i][f = 16c + c16]
#pragma unroll
    for (int c = 0; c < (GRAD ? NC : 1); ++c) acc[c] = zero4;
    mlp_f4 accW2 = zero4;            // dW2[j2 = 4g+i][j1 = 16w + c16]
    mlp_f4 accB1 = zero4;            // db1[j1 = 16w+4g+i], partial over this lane's documents
    mlp_f4 accB2 = zero4, accW3 = zero4;     // db2 / dW3 [j2 = 4g+i], documents this wave finished
    float accB3 = 0.f;

    // 16-byte unit k of this thread is unit u = tid + 256 k of the tile: 16 bytes at byte 16 u of the tile's rows in
    // memory (flat rows are consecutive), row ur[k] = u / C of the tile (>= 32: past the tile), image element
    // 8 u + ur[k] * (IPH - 8 C)
    int ur[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) ur[k] = (tid + k * T) / C;

    // ---- which rows of a tile are real, and their g: lanes 0 .. 31 of wave 0, into slot `slot` of the ring ----
    auto tile_meta = [&](int tile, int slot) {
        if (tid < kMrRows) {
            const long long row = (long long)tile * kMrRows + tid;
            bool ok = row < (long long)p.rows;
            float gv = 0.f;
            if (ok) {
                const int q = (int)row / L, j = (int)row - q * L;
                ok = p.n ? j < clamp_n(p.n[q], L) : true;
                if (GRAD && ok) gv = p.g[row];
            }
            const unsigned long long m = __ballot(ok);
            if (GRAD) gs[slot * kMrRows + tid] = gv;
            if (tid == 0) vmask[slot] = (unsigned)m;
        }
    };
    mb_i4 P[KP];                                    // the fill in flight
    auto issue_fill = [&](int tile, unsigned m) {
        const uint16_t *Xt = p.X + (size_t)tile * kMrRows * (size_t)F;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const bool ok = ur[k] < kMrRows && ((m >> (ur[k] & 31)) & 1u);
            // (a padded row is never read: its lanes fetch the first 16 bytes of W1 and drop them)
            const void *src = ok ? (const void *)(Xt + 8 * (size_t)(tid + k * T)) : (const void *)p.W1;
            P[k] = *reinterpret_cast<const mb_i4 *>(src);
        }
    };
    auto fill_image = [&](unsigned m) {
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const bool ok = (m >> (ur[k] & 31)) & 1u;
            const mb_i4 v = ok ? P[k] : zero4i;
            if (ur[k] < kMrRows)
                *reinterpret_cast<mb_i4 *>(img + 8 * (tid + k * T) + ur[k] * (IPH - 8 * C)) = v;
        }
    };

    // ---- forward over subtiles u0 .. u0 + NS - 1 of the image: layer-1 tile -> h1 (kept), layer-2 partial -> LDS ----
    auto fwd_tile = [&](auto ns_c, int u0, mlp_f4 (&h1)[2]) {
        constexpr int NS = decltype(ns_c)::value;
#pragma unroll
        for (int u = 0; u < NS; ++u) h1[u] = b1v;
        const uint16_t *bsrc = img + (16 * u0 + c16) * IPH + 8 * g;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
#pragma unroll
            for (int u = 0; u < NS; ++u) {
                const mb_bf8 xb = *reinterpret_cast<const mb_bf8 *>(bsrc + 16 * u * IPH + 32 * s);
                h1[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1r[s], xb, h1[u], 0, 0, 0);
            }
        }
#pragma unroll
        for (int u = 0; u < NS; ++u) {
#pragma unroll
            for (int i = 0; i < 4; ++i) h1[u][i] = fmaxf(h1[u][i], 0.f);
            mlp_f4 hp = zero4;
#pragma unroll
            for (int i = 0; i < 4; ++i) hp = mfma16(w2a[i], h1[u][i], hp);
            *reinterpret_cast<mlp_f4 *>(scr + (16 * (u0 + u) + c16) * kMrPS + 4 * g) = hp;
        }
        if (NS == 1) h1[1] = zero4;
    };
    // tile wave, backward over the same subtiles: dW2, dH1 and dW1 contributions
    auto bwd_tile = [&](auto ns_c, int u0, const mlp_f4 (&h1)[2]) {
        constexpr int NS = decltype(ns_c)::value;
        const float *tsrc = scr + g * kMrPS + c16;              // transposed reads: [4s + g][c16]
        const float *dsrc = dH2s + (16 * u0 + g) * kMrPS + c16;
        // ---- dW2[:, tile] += dH2^T . H1: H1 through the scratch (document-major -> k-major) ----
#pragma unroll
        for (int u = 0; u < NS; ++u)
            *reinterpret_cast<mlp_f4 *>(scr + (16 * u + c16) * kMrPS + 4 * g) = h1[u];
        {
            mlp_f4 o = zero4;
#pragma unroll
            for (int s = 0; s < 4 * NS; ++s) {
                const float a = dsrc[4 * s * kMrPS], bb = tsrc[4 * s * kMrPS];
                if (s & 1) o = mfma16(a, bb, o); else accW2 = mfma16(a, bb, accW2);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) accW2[i] += o[i];
        }
        // ---- dH1^T tile = (W2^T . dH2^T) . [H1 > 0] -> scratch ----
#pragma unroll
        for (int u = 0; u < NS; ++u) {
            const mlp_f4 d2 = *reinterpret_cast<const mlp_f4 *>(dH2s + (16 * (u0 + u) + c16) * kMrPS + 4 * g);
            mlp_f4 d1 = zero4;
#pragma unroll
            for (int i = 0; i < 4; ++i) d1 = mfma16(w2t[i], d2[i], d1);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                d1[i] = (h1[u][i] > 0.f) ? d1[i] : 0.f;
                accB1[i] += d1[i];
            }
            *reinterpret_cast<mlp_f4 *>(scr + (16 * u + c16) * kMrPS + 4 * g) = d1;
        }
        // ---- A of the dW1 step: dH1[row 8g + j of the tile][j1 = c16] as hi + lo in bf16; the rows of a skipped
        //      subtile (NS == 1: lanes whose g >> 1 is not u0) are zeros ----
        const bool mine = NS == 2 || (g >> 1) == u0;
        const float *asrc = scr + (NS == 2 ? 8 * g : 8 * (g & 1)) * kMrPS + c16;
        mb_bf8 ahi, alo;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = asrc[j * kMrPS];
            const float d = mine ? v : 0.f;
            const __bf16 h = (__bf16)d;
            ahi[j] = h;
            alo[j] = (__bf16)(d - (float)h);
        }
        // ---- dW1[tile] += dH1^T . X: B = image columns 16c .. 16c+15 of the rows 8g .. 8g+7, two transposed blocks:
        //      lane 4q + p of a 16-lane group addresses row q of the block, columns 4p .. 4p+3 ----
        const uint16_t *xsrc = img + (8 * g + (c16 >> 2)) * IPH + 4 * (c16 & 3);
        typedef mb_s4 __attribute__((address_space(3))) *lds_s4;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const mb_s4 lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(xsrc + 16 * c));
            const mb_s4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(xsrc + 16 * c + 4 * IPH));
            const mb_bf4 l4 = __builtin_bit_cast(mb_bf4, lo4), h4 = __builtin_bit_cast(mb_bf4, hi4);
            const mb_bf8 xb = {l4[0], l4[1], l4[2], l4[3], h4[0], h4[1], h4[2], h4[3]};
            acc[GRAD ? c : 0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahi, xb, acc[GRAD ? c : 0], 0, 0, 0);
            acc[GRAD ? c : 0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(alo, xb, acc[GRAD ? c : 0], 0, 0, 0);
        }
    };

    // ---- prologue: masks of the first two tiles, the first fill ----
    const int G = (int)gridDim.x;
    int tile = (int)blockIdx.x;
    tile_meta(tile, 0);
    tile_meta(tile + G, 1);
    // the feature columns F .. 32 KS + 7 of the image are never written by a fill: zero them once
    // (layer 1 multiplies them by zero weights, the dW1 columns they produce are not stored)
    for (int i = tid; i < kMrRows * (IPH - 8 * C); i += T) {
        const int r = i / (IPH - 8 * C), cc = i - r * (IPH - 8 * C);
        img[r * IPH + 8 * C + cc] = 0;
    }
    __syncthreads();
    issue_fill(tile, __builtin_amdgcn_readfirstlane(vmask[0]));

    int slot = 0;
    for (; tile < p.tiles; tile += G) {
        const int slot1 = slot == kMrRing - 1 ? 0 : slot + 1;
        const int slot2 = slot1 == kMrRing - 1 ? 0 : slot1 + 1;
        // (both masks were written in front of a barrier every wave has passed: the prologue's, or barrier A of the
        // iteration before; the slot rewritten below was last read in front of barrier A of the iteration before)
        const unsigned m = __builtin_amdgcn_readfirstlane(vmask[slot]);
        const unsigned mnext = __builtin_amdgcn_readfirstlane(vmask[slot1]);
        fill_image(m);                             // (waits for the fill in P; every wave is past the image's readers)
        issue_fill(tile + G, mnext);               // (past the last tile: mask 0, nothing of X is requested)
        tile_meta(tile + 2 * G, slot2);
        lds_barrier();                             // A: image filled
        const bool act0 = (m & 0xFFFFu) != 0, act1 = (m >> 16) != 0;        // subtiles with a real row (uniform)
        const int doc = 16 * w + c16;              // owner waves 0, 1: the row of the tile this lane finishes
        const long long orow = (long long)tile * kMrRows + doc;
        if (m == 0) {                              // padding only
            if (!GRAD && w < 2 && g == 0 && orow < (long long)p.rows) p.scores_out[orow] = 0.f;
            slot = slot1;
            continue;
        }
        const int u0 = act0 ? 0 : 1;
        mlp_f4 h1[2];
        if (act0 && act1) fwd_tile(m2_ns<2>{}, 0, h1);
        else fwd_tile(m2_ns<1>{}, u0, h1);
        lds_barrier();                             // B: layer-2 partials
        // ---- owner wave: the four partial tiles of its documents, layers 2 (bias, relu) and 3 ----
        const bool own = w < 2 && (w == 0 ? act0 : act1);
        mlp_f4 h2 = zero4;
        float s = 0.f;
        if (own) {
            h2 = b2v;
#pragma unroll
            for (int t = 0; t < kMrWaves; ++t) {
                const mlp_f4 v = *reinterpret_cast<const mlp_f4 *>(part + ((size_t)t * kMrRows + doc) * kMrPS + 4 * g);
#pragma unroll
                for (int i = 0; i < 4; ++i) h2[i] += v[i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                h2[i] = fmaxf(h2[i], 0.f);
                s = __builtin_fmaf(w3v[i], h2[i], s);
            }
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 32);
            s += b3;
        }
        if (!GRAD) {
            if (w < 2 && g == 0 && orow < (long long)p.rows) p.scores_out[orow] = ((m >> doc) & 1u) ? s : 0.f;
            slot = slot1;
            continue;                              // (the partials are rewritten behind the next barrier A)
        }
        // ---- owner wave, backward through layers 3 and 2: dH2 rows -> LDS (g is 0 on padded rows) ----
        if (own) {
            const float ds = gs[slot * kMrRows + doc];
            mlp_f4 dh2;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                accW3[i] = __builtin_fmaf(ds, h2[i], accW3[i]);
                dh2[i] = (h2[i] > 0.f) ? ds * w3v[i] : 0.f;
                accB2[i] += dh2[i];
            }
            if (g == 0) accB3 += ds;
            *reinterpret_cast<mlp_f4 *>(dH2s + doc * kMrPS + 4 * g) = dh2;
        }
        lds_barrier();                             // C: dH2 rows
        if (act0 && act1) bwd_tile(m2_ns<2>{}, 0, h1);
        else bwd_tile(m2_ns<1>{}, u0, h1);
        lds_barrier();                             // D: image, scratch and dH2 rows free
        slot = slot1;
    }
    if (!GRAD) return;

    // ---- this workgroup's partial vector [dW1 | db1 | dW2 | db2 | dW3 | db3] (ltr_mlp_rows.inc) ----
    float *dst = p.part + (size_t)blockIdx.x * p.pitch;
    const int oB1 = H1 * F, oW2 = oB1 + H1, oB2 = oW2 + H2 * H1, oW3 = oB2 + H2, oB3 = oW3 + H2;
    const int C4 = F >> 2;                         // float4 units of a dW1 row
    __syncthreads();                               // (the ring words of the last iterations are behind every wave)
    {
        // dW1 tile: rows 16w .. 16w+15 of [H1][F] are one contiguous piece of the partial vector; the D fragments go
        // through a wave-private LDS tile and leave as 16-byte stores of consecutive addresses
        float *tile_s = reinterpret_cast<float *>(smem) + (size_t)w * 16 * IPF;
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) tile_s[(4 * g + i) * IPF + 16 * c + c16] = acc[GRAD ? c : 0][i];
        float *drow = dst + (size_t)16 * w * F;
        for (int idx = lane; idx < 16 * C4; idx += 64) {
            const int r = idx / C4, f4 = idx - r * C4;
            if (16 * w + r < H1)
                *reinterpret_cast<mlp_f4 *>(drow + 4 * idx) = *reinterpret_cast<const mlp_f4 *>(tile_s + r * IPF + 4 * f4);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j2 = 4 * g + i;
        if (j2 < H2 && j1A < H1) dst[oW2 + j2 * H1 + j1A] = accW2[i];
        const float s1 = row16_sum(accB1[i]);
        const int j1 = 16 * w + 4 * g + i;
        if (c16 == 0 && j1 < H1) dst[oB1 + j1] = s1;
        accB2[i] = row16_sum(accB2[i]);
        accW3[i] = row16_sum(accW3[i]);
    }
    accB3 = wave_sum(accB3);
    // the per-document-owner sums (db2, dW3, db3) fold over the waves in a fixed order
    // (behind the dW1 tiles of the store above: 64 staging rows from the start of the segment)
    float *fold = reinterpret_cast<float *>(smem) + (size_t)64 * IPF;
    float *slv = fold + (size_t)w * 40;            // [16] db2 | [16] dW3 | [1] db3
    if (c16 == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            slv[4 * g + i] = accB2[i];
            slv[16 + 4 * g + i] = accW3[i];
        }
    }
    if (lane == 0) slv[32] = accB3;
    __syncthreads();
    if (tid < 33) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < kMrWaves; ++k) t += fold[k * 40 + tid];
        if (tid < 16) { if (tid < H2) dst[oB2 + tid] = t; }
        else if (tid < 32) { if (tid - 16 < H2) dst[oW3 + tid - 16] = t; }
        else dst[oB3] = t;
    }
}

// ---- host side ----
inline int mlp_bf16_grid(long long rows)
{
    const long long tiles = (rows + kMrRows - 1) / kMrRows;
    const long long wgs = (long long)kMrWgs * device_cu_count();
    return (int)(tiles < wgs ? tiles : wgs);
}

inline bool mlp_bf16_bad_shape(int B, int L, int F, int H1, int H2)
{
    if (B < 0 || L <= 0 || F <= 0 || H1 <= 0 || H2 <= 0) return true;
    if ((F & 7) || F > 32 * kMbMaxKS || H1 > kMlpH1 || H2 > kMlpH2) return true;
    return (long long)B * L > 0x7fffffffLL;
}

template <int KS, bool GRAD>
int launch_mlp_bf16_ks(const MlpBf16Params &p, int grid, hipStream_t stream)
{
    const size_t lds = mlp_bf16_lds_bytes(KS, GRAD);
    LTR_ENSURE_LDS((mlp_bf16_kernel<KS, GRAD>), lds);
    hipLaunchKernelGGL((mlp_bf16_kernel<KS, GRAD>), dim3((unsigned)grid), dim3(kMrThreads), lds, stream, p);
    return (int)hipGetLastError();
}

template <bool GRAD>
int launch_mlp_bf16(const MlpBf16Params &p, int grid, hipStream_t stream)
{
    switch ((p.F + 31) / 32) {
    case 1: return launch_mlp_bf16_ks<1, GRAD>(p, grid, stream);
    case 2: return launch_mlp_bf16_ks<2, GRAD>(p, grid, stream);
    case 3: return launch_mlp_bf16_ks<3, GRAD>(p, grid, stream);
    case 4: return launch_mlp_bf16_ks<4, GRAD>(p, grid, stream);
    case 5: return launch_mlp_bf16_ks<5, GRAD>(p, grid, stream);
    case 6: return launch_mlp_bf16_ks<6, GRAD>(p, grid, stream);
    default: return launch_mlp_bf16_ks<7, GRAD>(p, grid, stream);
    }
}

extern "C" {

int ltr_mlp_bf16_scores(const uint16_t *X, const float *W1, const float *b1, const float *W2, const float *b2,
                        const float *W3, const float *b3, const int64_t *n, int B, int L, int F, int H1, int H2,
                        float *scores_out, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (mlp_bf16_bad_shape(B, L, F, H1, H2)) return LTR_ERR_SHAPE;
    if (!W1 || !b1 || !W2 || !b2 || !W3 || !b3) return LTR_ERR_NULL;
    if (B == 0) return LTR_OK;
    if (!X || !scores_out) return LTR_ERR_NULL;
    MlpBf16Params p;
    p.X = X; p.W1 = W1; p.b1 = b1; p.W2 = W2; p.b2 = b2; p.W3 = W3; p.b3 = b3; p.g = nullptr;
    p.n = n; p.scores_out = scores_out; p.part = nullptr;
    p.B = B; p.L = L; p.F = F; p.H1 = H1; p.H2 = H2;
    p.rows = B * L; p.tiles = (int)(((long long)p.rows + kMrRows - 1) / kMrRows); p.pitch = 0;
    return launch_mlp_bf16<false>(p, mlp_bf16_grid(p.rows), (hipStream_t)stream);
}

size_t ltr_mlp_bf16_grad_workspace_bytes(int B, int L, int F, int H1, int H2)
{
    if (B <= 0 || mlp_bf16_bad_shape(B, L, F, H1, H2)) return 0;
    return (size_t)mlp_bf16_grid((long long)B * L) * (size_t)mlp_pitch(mlp_param_count(F, H1, H2)) * sizeof(float);
}

int ltr_mlp_bf16_grad(const uint16_t *X, const float *W1, const float *b1, const float *W2, const float *b2,
                      const float *W3, const float *b3, const float *g, const int64_t *n, int B, int L, int F,
                      int H1, int H2, float *grads, void *workspace, size_t workspace_bytes, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (mlp_bf16_bad_shape(B, L, F, H1, H2)) return LTR_ERR_SHAPE;
    if (!W1 || !b1 || !W2 || !b2 || !W3 || !b3 || !grads) return LTR_ERR_NULL;
    const int P = mlp_param_count(F, H1, H2);
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) return mlp_reduce_launch(nullptr, 0, P, grads, nullptr, 0, nullptr, s);      // zero gradients
    if (!X || !g) return LTR_ERR_NULL;
    const int grid = mlp_bf16_grid((long long)B * L);
    if (!workspace || workspace_bytes < (size_t)grid * mlp_pitch(P) * sizeof(float)) return LTR_ERR_WORKSPACE;
    MlpBf16Params p;
    p.X = X; p.W1 = W1; p.b1 = b1; p.W2 = W2; p.b2 = b2; p.W3 = W3; p.b3 = b3; p.g = g;
    p.n = n; p.scores_out = nullptr; p.part = (float *)workspace;
    p.B = B; p.L = L; p.F = F; p.H1 = H1; p.H2 = H2;
    p.rows = B * L; p.tiles = (int)(((long long)p.rows + kMrRows - 1) / kMrRows); p.pitch = mlp_pitch(P);
    const int rc = launch_mlp_bf16<true>(p, grid, s);
    if (rc != 0) return rc;
    return mlp_reduce_launch(workspace, grid, P, grads, nullptr, 0, nullptr, s);
}

}  // extern "C"
