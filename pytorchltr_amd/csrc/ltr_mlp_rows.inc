// ltr_mlp_rows.inc -- the ReLU-MLP scorer (F -> H1 -> H2 -> 1) on its own: a row-streaming score kernel and a
// row-streaming parameter-gradient kernel on v_mfma_f32_16x16x4_f32, for lists of ANY length (include/ltr_mlp_rows.h).
// Included by ltr_mlp.hip behind ltr_mlp.inc, whose fragments, reduction kernel and padding rules it shares.
//
// The fused per-query steps (ltr_mlp.inc, ltr_mlp2.inc) keep a whole query in a workgroup and stop at 256 / 128
// documents.  A document's score and its share of the parameter gradients depend on its own row and on the upstream
// d loss / d score only, so here the unit of work is a TILE of 32 consecutive FLAT rows of the (B * L, F) matrix; a row
// is real iff row % L < n[row / L].  A tile may hold several queries and a query may span many tiles; neither kernel
// has a list-length limit.  This is what the Linear scorer has in ltr_scorer.inc.
//
// Mapping: the 4-wave layout of ltr_mlp2.inc (two workgroups per CU, every wave owns one 16-row tile of the first
// hidden layer, W1 / W2 fragments in registers, the fill in an LDS image [32][16*NT + 4], transposed activations so
// that a D fragment is the next B operand) with everything a query needed taken out: g is known up front, so a fill
// goes forward and straight back -- no pair pass, no parking, no loss slot, no scheduling pass.
//     (fill n+1 requested)  image <- fill n                                              barrier A
//     layer 1 tile, layer-2 partial tile -> LDS      (per wave: 8 NT + 8 MFMAs per 32 rows)   barrier B
//     owner waves 0, 1: layers 2 + 3 of 16 documents each -> score; GRAD: dH2 rows -> LDS    barrier C   (GRAD only)
//     GRAD: dW2 tile, dH1 tile, dW1 tile += ... (8 + 8 + 8 NT MFMAs)                           barrier D   (GRAD only)
// A subtile of 16 rows that is all padding is skipped by every chain; a tile of padding only costs its barrier A.
// Loads stay unconditional: a float4 of a padded row is requested from the first 16 bytes of W1 instead and replaced
// by zeros on its way into the image, so padded rows of X are never read; g is read for real rows only.
// Which rows of a tile are real is worked out two tiles ahead by 32 lanes (one division each; a 32-bit mask and the
// 32 values of g per tile in a three-deep LDS ring), so the address select of the next fill has its mask in time.
// Persistent grid: workgroup w takes the tiles w, w + G, w + 2G, ... (fixed order); the dW1 / dW2 tiles live in
// registers for the workgroup's whole life, one partial vector per workgroup, mlp_reduce_launch(loss = NULL) adds them
// in a fixed order.  No atomics: bit-identical run to run.
// All four feature buckets (NT = 3, 5, 9, 14) run this layout: without parked tiles and a loss row, the widest one
// needs 59 KB of LDS per workgroup (the staging of the dW1 tiles at the end); its gradient kernel runs one workgroup per
// CU (mlp_rows_wgs), every other instantiation two.
// DESIGN.md section 18 has the bytes, the FLOPs and the measurements.
#pragma once

#include "ltr_mlp_rows.h"

constexpr int kMrThreads = 256;
constexpr int kMrWaves = 4;
constexpr int kMrRows = 32;          // flat rows per tile (two 16-row subtiles)
constexpr int kMrWgs = 2;            // workgroups per CU the launch bounds and the grid are sized for ...
// ... but ONE for the gradient kernel of the widest bucket: its W1 fragments (56 registers), dW1 tile (56) and fill in
// flight (28 + 7) leave too little of 256 registers for the chains (81 spilled); alone on its SIMD a wave has 512
constexpr int mlp_rows_wgs(int NT, bool grad) { return (grad && NT > 9) ? 1 : kMrWgs; }
constexpr int kMrPS = 20;            // row pitch (floats) of the partial / scratch / dH2 images
constexpr int kMrRing = 3;           // tiles whose row mask / g values are kept in LDS

struct MlpRowsParams {
    const float *X, *W1, *b1, *W2, *b2, *W3, *b3, *g;
    const int64_t *n;
    float *scores_out, *part;
    int B, L, F, H1, H2;
    int rows;                        // B * L
    int tiles;                       // ceil(rows / 32)
    int pitch;                       // floats between consecutive partial vectors
};

__host__ __device__ constexpr size_t mlp_rows_lds_bytes(int NT, bool grad)
{
    const size_t IP = (size_t)16 * NT + 4;
    const size_t loop = kMrRows * IP + (size_t)kMrWaves * kMrRows * kMrPS + (size_t)kMrRows * kMrPS +
                        (size_t)kMrRing * kMrRows + 4;
    // the gradient kernel stages its four dW1 tiles (64 image rows) and the fold of the small sums at the end
    const size_t tail = grad ? 64 * IP + (size_t)kMrWaves * 40 : 0;
    return (loop > tail ? loop : tail) * sizeof(float);
}
// (the widest instantiations that share a CU: <14, false> and <9, true>; <14, true> is alone on its CU, mlp_rows_wgs)
static_assert(mlp_rows_lds_bytes(14, false) <= kLdsBudget / kMrWgs && mlp_rows_lds_bytes(9, true) <= kLdsBudget / kMrWgs,
              "two workgroups per CU");
static_assert(mlp_rows_lds_bytes(14, true) <= kLdsBudget, "one workgroup per CU");

template <int NT, bool GRAD>
__global__ void __launch_bounds__(kMrThreads, mlp_rows_wgs(NT, GRAD))
mlp_rows_kernel(MlpRowsParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    constexpr int T = kMrThreads;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15;
    const int g = lane >> 4;
    const int L = p.L, F = p.F, H1 = p.H1, H2 = p.H2;
    const int C = F >> 2;                           // float4 units per feature row
    constexpr int IP = 16 * NT + 4;                 // image pitch (floats): odd number of 16-byte units
    constexpr int KP = (kMrRows * 4 * NT + T - 1) / T;      // float4 units of a fill per thread

    float *img = reinterpret_cast<float *>(smem);                  // [32][IP]   feature rows of the fill
    float *part = img + (size_t)kMrRows * IP;                      // [4][32][20] layer-2 partials, later
    float *scr = part + (size_t)w * kMrRows * kMrPS;               //            this wave's transposition scratch
    float *dH2s = part + (size_t)kMrWaves * kMrRows * kMrPS;       // [32][20]
    float *gs = dH2s + (size_t)kMrRows * kMrPS;                    // [3][32]    d loss / d score of the tile's rows
    unsigned *vmask = reinterpret_cast<unsigned *>(gs + kMrRing * kMrRows);    // [3] bit r: row r of the tile is real

    const mlp_f4 zero4 = {0.f, 0.f, 0.f, 0.f};

    // ---- this wave's weight fragments, straight from global memory into registers (ltr_mlp2.inc) ----
    const int j1A = 16 * w + c16;                   // hidden-1 row as an A-operand row (lane & 15)
    mlp_f4 w1r[NT];                                 // W1[j1A][16c + 4g .. +3]
    mlp_f4 b1v, w2a, w2t, b2v, w3v;
#pragma unroll
    for (int c = 0; c < NT; ++c) {
        const int f0 = 16 * c + 4 * g;
        const bool ok = j1A < H1 && f0 < F;
        const mlp_f4 v = *reinterpret_cast<const mlp_f4 *>(p.W1 + (ok ? (size_t)j1A * F + f0 : 0));
#pragma unroll
        for (int i = 0; i < 4; ++i) w1r[c][i] = ok ? v[i] : 0.f;
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
    mlp_f4 acc[GRAD ? NT : 1];       // dW1[j1 = 16w+4g+i][f = 16c + c16]
#pragma unroll
    for (int c = 0; c < (GRAD ? NT : 1); ++c) acc[c] = zero4;
    mlp_f4 accW2 = zero4;            // dW2[j2 = 4g+i][j1 = 16w + c16]
    mlp_f4 accB1 = zero4;            // db1[j1 = 16w+4g+i], partial over this lane's documents
    mlp_f4 accB2 = zero4, accW3 = zero4;     // db2 / dW3 [j2 = 4g+i], documents this wave finished
    float accB3 = 0.f;

    // float4 unit k of this thread is unit u = tid + 256 k of the tile: 16 bytes at byte 16 u of the tile's rows in
    // memory (flat rows are consecutive), row ur[k] = u / C of the tile (>= 32: past the tile), image float
    // 4 u + ur[k] * (IP - 4 C)
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
    mlp_f4 P[KP];                                   // the fill in flight
    auto issue_fill = [&](int tile, unsigned m) {
        const float *Xt = p.X + (size_t)tile * kMrRows * (size_t)F;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const bool ok = ur[k] < kMrRows && ((m >> (ur[k] & 31)) & 1u);
            // (a padded row is never read: its lanes fetch the first 16 bytes of W1 and drop them)
            const float *src = ok ? Xt + 4 * (size_t)(tid + k * T) : p.W1;
            P[k] = *reinterpret_cast<const mlp_f4 *>(src);
        }
    };
    auto fill_image = [&](unsigned m) {
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const bool ok = (m >> (ur[k] & 31)) & 1u;
            mlp_f4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = ok ? P[k][i] : 0.f;
            if (ur[k] < kMrRows)
                *reinterpret_cast<mlp_f4 *>(img + 4 * (tid + k * T) + ur[k] * (IP - 4 * C)) = v;
        }
    };

    // ---- forward over subtiles u0 .. u0 + NS - 1 of the image: layer-1 tile -> h1 (kept), layer-2 partial -> LDS ----
    auto fwd_tile = [&](auto ns_c, int u0, mlp_f4 (&h1)[2]) {
        constexpr int NS = decltype(ns_c)::value;
#pragma unroll
        for (int u = 0; u < NS; ++u) h1[u] = b1v;
        const float *bsrc = img + (16 * u0 + c16) * IP + 4 * g;
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
        float a1[4 * NS];
#pragma unroll
        for (int s = 0; s < 4 * NS; ++s) a1[s] = tsrc[4 * s * kMrPS];
        // ---- dW1[tile] += dH1^T . X: B = image columns; three feature chunks in flight ----
        const float *xsrc = img + (16 * u0 + g) * IP + c16;
        constexpr int CG = 3;
#pragma unroll
        for (int c0 = 0; c0 < NT; c0 += CG) {
#pragma unroll
            for (int s = 0; s < 4 * NS; ++s) {
#pragma unroll
                for (int cc = 0; cc < CG; ++cc) {
                    if (c0 + cc < NT)
                        acc[GRAD ? c0 + cc : 0] =
                            mfma16(a1[s], xsrc[4 * s * IP + 16 * (c0 + cc)], acc[GRAD ? c0 + cc : 0]);
                }
            }
        }
    };

    // ---- prologue: masks of the first two tiles, the first fill ----
    const int G = (int)gridDim.x;
    int tile = (int)blockIdx.x;
    tile_meta(tile, 0);
    tile_meta(tile + G, 1);
    // the feature columns F .. 16*NT+3 of the image are never written by a fill: zero them once
    // (layer 1 multiplies them by zero weights, the dW1 columns they produce are not stored)
    for (int i = tid; i < kMrRows * (IP - 4 * C); i += T) {
        const int r = i / (IP - 4 * C), cc = i - r * (IP - 4 * C);
        img[r * IP + 4 * C + cc] = 0.f;
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

    // ---- this workgroup's partial vector [dW1 | db1 | dW2 | db2 | dW3 | db3] (ltr_mlp2.inc) ----
    float *dst = p.part + (size_t)blockIdx.x * p.pitch;
    const int oB1 = H1 * F, oW2 = oB1 + H1, oB2 = oW2 + H2 * H1, oW3 = oB2 + H2, oB3 = oW3 + H2;
    __syncthreads();                               // (the ring words of the last iterations are behind every wave)
    {
        // dW1 tile: rows 16w .. 16w+15 of [H1][F] are one contiguous piece of the partial vector; the D fragments go
        // through a wave-private LDS tile and leave as 16-byte stores of consecutive addresses
        float *tile_s = reinterpret_cast<float *>(smem) + (size_t)w * 16 * IP;
#pragma unroll
        for (int c = 0; c < NT; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) tile_s[(4 * g + i) * IP + 16 * c + c16] = acc[GRAD ? c : 0][i];
        float *drow = dst + (size_t)16 * w * F;
        for (int idx = lane; idx < 16 * C; idx += 64) {
            const int r = idx / C, f4 = idx - r * C;
            if (16 * w + r < H1)
                *reinterpret_cast<mlp_f4 *>(drow + 4 * idx) = *reinterpret_cast<const mlp_f4 *>(tile_s + r * IP + 4 * f4);
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
    // (behind the dW1 tiles of the store above: 64 image rows from the start of the segment)
    float *fold = reinterpret_cast<float *>(smem) + (size_t)64 * IP;
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
inline int mlp_rows_grid(long long rows, int F, bool grad)
{
    const long long tiles = (rows + kMrRows - 1) / kMrRows;
    const long long wgs = (long long)mlp_rows_wgs(mlp_bucket(F), grad) * device_cu_count();
    return (int)(tiles < wgs ? tiles : wgs);
}

inline bool mlp_rows_bad_shape(int B, int L, int F, int H1, int H2)
{
    if (B < 0 || L <= 0 || F <= 0 || H1 <= 0 || H2 <= 0) return true;
    if ((F & 3) || F > 16 * 14 || H1 > kMlpH1 || H2 > kMlpH2) return true;
    return (long long)B * L > 0x7fffffffLL;
}

template <int NT, bool GRAD>
int launch_mlp_rows_nt(const MlpRowsParams &p, int grid, hipStream_t stream)
{
    const size_t lds = mlp_rows_lds_bytes(NT, GRAD);
    LTR_ENSURE_LDS((mlp_rows_kernel<NT, GRAD>), lds);
    hipLaunchKernelGGL((mlp_rows_kernel<NT, GRAD>), dim3((unsigned)grid), dim3(kMrThreads), lds, stream, p);
    return (int)hipGetLastError();
}

template <bool GRAD>
int launch_mlp_rows(const MlpRowsParams &p, int grid, hipStream_t stream)
{
    switch (mlp_bucket(p.F)) {
    case 3: return launch_mlp_rows_nt<3, GRAD>(p, grid, stream);
    case 5: return launch_mlp_rows_nt<5, GRAD>(p, grid, stream);
    case 9: return launch_mlp_rows_nt<9, GRAD>(p, grid, stream);
    default: return launch_mlp_rows_nt<14, GRAD>(p, grid, stream);
    }
}

extern "C" {

int ltr_mlp_rows_scores_f32(const float *X, const float *W1, const float *b1, const float *W2, const float *b2,
                            const float *W3, const float *b3, const int64_t *n, int B, int L, int F, int H1, int H2,
                            float *scores_out, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (mlp_rows_bad_shape(B, L, F, H1, H2)) return LTR_ERR_SHAPE;
    if (!W1 || !b1 || !W2 || !b2 || !W3 || !b3) return LTR_ERR_NULL;
    if (B == 0) return LTR_OK;
    if (!X || !scores_out) return LTR_ERR_NULL;
    MlpRowsParams p;
    p.X = X; p.W1 = W1; p.b1 = b1; p.W2 = W2; p.b2 = b2; p.W3 = W3; p.b3 = b3; p.g = nullptr;
    p.n = n; p.scores_out = scores_out; p.part = nullptr;
    p.B = B; p.L = L; p.F = F; p.H1 = H1; p.H2 = H2;
    p.rows = B * L; p.tiles = (int)(((long long)p.rows + kMrRows - 1) / kMrRows); p.pitch = 0;
    return launch_mlp_rows<false>(p, mlp_rows_grid(p.rows, F, false), (hipStream_t)stream);
}

size_t ltr_mlp_rows_grad_workspace_bytes(int B, int L, int F, int H1, int H2)
{
    if (B <= 0 || mlp_rows_bad_shape(B, L, F, H1, H2)) return 0;
    return (size_t)mlp_rows_grid((long long)B * L, F, true) * (size_t)mlp_pitch(mlp_param_count(F, H1, H2)) * sizeof(float);
}

int ltr_mlp_rows_grad_f32(const float *X, const float *W1, const float *b1, const float *W2, const float *b2,
                          const float *W3, const float *b3, const float *g, const int64_t *n, int B, int L, int F,
                          int H1, int H2, float *grads, void *workspace, size_t workspace_bytes, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (mlp_rows_bad_shape(B, L, F, H1, H2)) return LTR_ERR_SHAPE;
    if (!W1 || !b1 || !W2 || !b2 || !W3 || !b3 || !grads) return LTR_ERR_NULL;
    const int P = mlp_param_count(F, H1, H2);
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) return mlp_reduce_launch(nullptr, 0, P, grads, nullptr, 0, nullptr, s);      // zero gradients
    if (!X || !g) return LTR_ERR_NULL;
    const int grid = mlp_rows_grid((long long)B * L, F, true);
    if (!workspace || workspace_bytes < (size_t)grid * mlp_pitch(P) * sizeof(float)) return LTR_ERR_WORKSPACE;
    MlpRowsParams p;
    p.X = X; p.W1 = W1; p.b1 = b1; p.W2 = W2; p.b2 = b2; p.W3 = W3; p.b3 = b3; p.g = g;
    p.n = n; p.scores_out = nullptr; p.part = (float *)workspace;
    p.B = B; p.L = L; p.F = F; p.H1 = H1; p.H2 = H2;
    p.rows = B * L; p.tiles = (int)(((long long)p.rows + kMrRows - 1) / kMrRows); p.pitch = mlp_pitch(P);
    const int rc = launch_mlp_rows<true>(p, grid, s);
    if (rc != 0) return rc;
    return mlp_reduce_launch(workspace, grid, P, grads, nullptr, 0, nullptr, s);
}

}  // extern "C"
