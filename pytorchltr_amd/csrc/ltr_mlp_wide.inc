// ltr_mlp_wide.inc -- the ReLU-MLP scorer (F -> H1 -> H2 -> 1) on WIDE feature rows, up to 704 features: K-streamed
// score and parameter-gradient kernels on v_mfma_f32_16x16x4_f32 for lists of any length (include/ltr_mlp_wide.h).
// Included by ltr_mlp.hip behind ltr_mlp_rows.inc, whose fragments, reduction kernel and padding rules it shares.
//
// The row kernels (ltr_mlp_rows.inc) keep a wave's W1 fragments, and the gradient kernel its dW1 tile, in registers for
// the workgroup's whole life: 56 + 56 registers at 224 features, 176 + 176 at 704, where W1 itself (176 KiB) is more
// than the LDS.  Here the feature dimension is walked in CHUNKS of 128 features instead.  The unit of work, the mask
// (`row % L < n[row / L]`), the persistent grid and the tile order (workgroup w takes the tiles w, w + G, w + 2G, ...)
// are those of ltr_mlp_rows.inc; so is the wave layout (four waves, wave w owns hidden-1 rows 16w .. 16w + 15).
//
// Forward (mlp_wide_fwd_kernel): a workgroup takes its tiles in GROUPS of eight (scores; four in front of the backward
// half, mlp_wide_group) and keeps the layer-1 accumulators of the whole group in registers (8 per tile).  Chunk loop
// outside, tile loop inside:
//     for chunk:  W1 fragments of the chunk <- global (32 registers, L2-resident: one 176 KiB pass over W1 per GROUP,
//                 i.e. per 720 / 360 KB of X at F = 704)
//         for tile of the group:  image[parity] <- the tile's 32 x 128 piece of X (requested one step ahead; the address
//                 select of the row kernels keeps padded rows unread)                                 one barrier
//                 64 MFMAs per wave into the tile's accumulators
//     for tile of the group:  layers 2 and 3 and the score store as in mlp_rows_kernel; GRAD: dH2 rows, the dW2 tile,
//                 the small sums, and the tile's d loss / d hidden-1 (zeros on padded rows) -> workspace, 256 B a row
// The image and the layer-2 partials are double buffered by step / tile parity, which is what lets one barrier a step do.
// Which rows of a group are real is worked out once per group: 256 threads, one row each, two tiles per ballot.
//
// Gradient, second kernel (mlp_wide_dw1_kernel): dW1 = dH1^T . X over (column slice of 128 or 176 features) x (row
// range): exactly the dW1 chain of mlp_rows_kernel with the A operand read from the workspace and a dW1 slice of 32 / 44
// registers per lane; X is read a second time.  One partial dW1 per row range, one partial vector of the small sums per
// workgroup of the first kernel, two launches of mlp_reduce_launch(loss = NULL) add them in a fixed order.  No atomics.
// DESIGN.md section 19 has the choice between this and a one-kernel gradient, the register / LDS table and the bytes.
#pragma once

#include "ltr_mlp_wide.h"

constexpr int kMwThreads = 256;
constexpr int kMwWaves = 4;
constexpr int kMwRows = 32;           // flat rows per tile (two 16-row subtiles)
constexpr int kMwWgs = 2;             // workgroups per CU the launch bounds and the grids are sized for
constexpr int kMwMaxF = 704;
constexpr int kMwNTC = 8;             // 16-feature steps per chunk
constexpr int kMwKC = 16 * kMwNTC;    // features per chunk
constexpr int kMwIP = kMwKC + 4;      // image pitch (floats): odd number of 16-byte units
constexpr int kMwTG = kMwThreads / kMwRows;      // most tiles per group: one thread per row works out the masks
// tiles per group: eight for the scores; four for the gradient's forward kernel, whose backward fragments and sums
// (37 registers) next to eight tiles' accumulators spilled 30 registers under the 256 of two workgroups per CU
constexpr int mlp_wide_group(bool grad) { return grad ? 4 : kMwTG; }
constexpr int kMwPS = 20;             // row pitch (floats) of the partial / scratch / dH2 images
constexpr int kMwRing = 3;            // dW1 kernel: tiles whose row mask is kept in LDS
constexpr int kMwDH = 64;             // floats per flat row of the d loss / d hidden-1 tile in the workspace

struct MlpWideParams {
    const float *X, *W1, *b1, *W2, *b2, *W3, *b3, *g;
    const int64_t *n;
    float *scores_out;
    float *part;                     // fwd: partial vectors of the small sums; dw1: partial dW1 matrices
    float *dH1;                      // [tiles * 32][64]
    int B, L, F, H1, H2;
    int rows;                        // B * L
    int tiles;                       // ceil(rows / 32)
    int pitch;                       // floats between consecutive partial vectors of `part`
};

constexpr size_t mlp_wide_fwd_lds_bytes()
{
    return ((size_t)2 * kMwRows * kMwIP + (size_t)2 * kMwWaves * kMwRows * kMwPS + (size_t)kMwRows * kMwPS +
            (size_t)kMwTG * kMwRows + kMwTG + 8) * sizeof(float);
}
constexpr size_t mlp_wide_dw1_lds_bytes(int NTS)
{
    // two images [32][16 NTS + 4]; the four dW1 tiles (64 image rows) are staged in the same floats at the end
    return ((size_t)2 * kMwRows * (16 * NTS + 4) + 8) * sizeof(float);
}
static_assert(mlp_wide_fwd_lds_bytes() <= kLdsBudget / kMwWgs && mlp_wide_dw1_lds_bytes(11) <= kLdsBudget / kMwWgs,
              "two workgroups per CU");

template <bool GRAD>
__global__ void __launch_bounds__(kMwThreads, kMwWgs)
mlp_wide_fwd_kernel(MlpWideParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15;
    const int g = lane >> 4;
    const int L = p.L, F = p.F, H1 = p.H1, H2 = p.H2;
    const int NC = (F + kMwKC - 1) / kMwKC;         // feature chunks
    constexpr int IP = kMwIP;
    constexpr int TG = mlp_wide_group(GRAD);        // tiles per group
    static_assert(TG % 2 == 0 && TG <= kMwTG, "buffers alternate by tile parity across the chunks");

    float *img = reinterpret_cast<float *>(smem);                  // [2][32][IP]    the piece of X of a step
    float *part = img + (size_t)2 * kMwRows * IP;                  // [2][4][32][20] layer-2 partials / wave scratch
    float *dH2s = part + (size_t)2 * kMwWaves * kMwRows * kMwPS;   // [32][20]
    float *gs = dH2s + (size_t)kMwRows * kMwPS;                    // [8][32]        d loss / d score of the group's rows
    unsigned *vmask = reinterpret_cast<unsigned *>(gs + kMwTG * kMwRows);      // [8] bit r: row r of tile j is real

    const mlp_f4 zero4 = {0.f, 0.f, 0.f, 0.f};

    // ---- the small weight fragments (ltr_mlp_rows.inc); the W1 fragments exist per chunk ----
    const int j1A = 16 * w + c16;                   // hidden-1 row as an A-operand row (lane & 15)
    mlp_f4 b1v, w2a, w2t, b2v, w3v;
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
    mlp_f4 accW2 = zero4;            // dW2[j2 = 4g+i][j1 = 16w + c16]
    mlp_f4 accB1 = zero4;            // db1[j1 = 16w+4g+i], partial over this lane's documents
    mlp_f4 accB2 = zero4, accW3 = zero4;     // db2 / dW3 [j2 = 4g+i], documents this wave finished
    float accB3 = 0.f;

    // A step moves a 32 x 128 piece of X: 1024 float4 units, four per thread -- rows fr, fr + 8, fr + 16, fr + 24 of
    // the tile, 16 bytes at float 4 fc of the chunk
    const int fr = tid >> 5, fc = tid & 31;
    mlp_f4 P[4];                                    // the piece in flight
    auto issue_fill = [&](int tile, int ch, unsigned m) {
        const int f = ch * kMwKC + 4 * fc;
        const float *Xt = p.X + ((size_t)tile * kMwRows + fr) * (size_t)F + f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool ok = ((m >> (fr + 8 * k)) & 1u) && f < F;
            // (a padded row is never read: its lanes fetch the first 16 bytes of W1 and drop them)
            const float *src = ok ? Xt + (size_t)(8 * k) * F : p.W1;
            P[k] = *reinterpret_cast<const mlp_f4 *>(src);
        }
    };
    auto fill_image = [&](float *im, int ch, unsigned m) {
        const int f = ch * kMwKC + 4 * fc;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool ok = ((m >> (fr + 8 * k)) & 1u) && f < F;
            mlp_f4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = ok ? P[k][i] : 0.f;
            *reinterpret_cast<mlp_f4 *>(im + (fr + 8 * k) * IP + 4 * fc) = v;
        }
    };

    const int G = (int)gridDim.x;
    for (int t0 = (int)blockIdx.x; t0 < p.tiles; t0 += TG * G) {
        // ---- tile j of this group is t0 + j G; which of its rows are real, and their g (thread = row) ----
        __syncthreads();                           // (the masks and g of the group before are behind every wave)
        if (fr < TG) {                             // (wave-uniform: a wave holds the rows of two tiles)
            const int tile = t0 + fr * G;
            const long long row = (long long)tile * kMwRows + fc;
            bool ok = tile < p.tiles && row < (long long)p.rows;
            float gv = 0.f;
            if (ok) {
                const int q = (int)row / L, j = (int)row - q * L;
                ok = p.n ? j < clamp_n(p.n[q], L) : true;
                if (GRAD && ok) gv = p.g[row];
            }
            const unsigned long long m = __ballot(ok);          // lanes 0 .. 31: tile 2w, lanes 32 .. 63: tile 2w + 1
            if (GRAD) gs[tid] = gv;
            if (lane == 0) {
                vmask[2 * w] = (unsigned)m;
                vmask[2 * w + 1] = (unsigned)(m >> 32);
            }
        }
        __syncthreads();

        mlp_f4 h1a[TG][2];                      // layer-1 pre-activations of the group: [j1 = 16w+4g+i][doc c16]
#pragma unroll
        for (int j = 0; j < TG; ++j) { h1a[j][0] = b1v; h1a[j][1] = b1v; }

        // ---- layer 1: chunk loop outside, tile loop inside ----
        unsigned mcur = __builtin_amdgcn_readfirstlane(vmask[0]);
        if (mcur) issue_fill(t0, 0, mcur);
        for (int ch = 0; ch < NC; ++ch) {
            mlp_f4 w1r[kMwNTC];                     // W1[j1A][128 ch + 16c + 4g .. +3]
#pragma unroll
            for (int c = 0; c < kMwNTC; ++c) {
                const int f0 = ch * kMwKC + 16 * c + 4 * g;
                const bool ok = j1A < H1 && f0 < F;
                const mlp_f4 v = *reinterpret_cast<const mlp_f4 *>(p.W1 + (ok ? (size_t)j1A * F + f0 : 0));
#pragma unroll
                for (int i = 0; i < 4; ++i) w1r[c][i] = ok ? v[i] : 0.f;
            }
            const bool hi = F - ch * kMwKC > kMwKC / 2;         // the chunk's upper 64 features exist (uniform)
#pragma unroll
            for (int j = 0; j < TG; ++j) {
                float *im = img + (size_t)(j & 1) * kMwRows * IP;
                if (mcur) fill_image(im, ch, mcur);             // (waits for the piece in P)
                const int jn = j + 1 < TG ? j + 1 : 0;
                const int chn = j + 1 < TG ? ch : ch + 1;
                const unsigned mn = chn < NC ? __builtin_amdgcn_readfirstlane(vmask[jn]) : 0u;
                if (mn) issue_fill(t0 + jn * G, chn, mn);
                // one barrier a step: the image written two steps on is this one again, and a wave gets there only
                // through the barrier of the step between, which every wave reaches behind its reads of this step
                lds_barrier();
                if (mcur) {
                    const float *bsrc = im + c16 * IP + 4 * g;
#pragma unroll
                    for (int half = 0; half < 2; ++half) {
                        if (half == 0 || hi) {
#pragma unroll
                            for (int c = 4 * half; c < 4 * half + 4; ++c) {
                                mlp_f4 xb[2];
#pragma unroll
                                for (int u = 0; u < 2; ++u)
                                    xb[u] = *reinterpret_cast<const mlp_f4 *>(bsrc + 16 * u * IP + 16 * c);
#pragma unroll
                                for (int i = 0; i < 4; ++i) {
#pragma unroll
                                    for (int u = 0; u < 2; ++u) h1a[j][u] = mfma16(w1r[c][i], xb[u][i], h1a[j][u]);
                                }
                            }
                        }
                    }
                }
                mcur = mn;
            }
        }

        // ---- layers 2 and 3 of every tile of the group (mlp_rows_kernel), GRAD: and back down to dH1 ----
#pragma unroll
        for (int j = 0; j < TG; ++j) {
            const unsigned m = __builtin_amdgcn_readfirstlane(vmask[j]);
            const int tile = t0 + j * G;
            const int doc = 16 * w + c16;          // owner waves 0, 1: the row of the tile this lane finishes
            const long long orow = (long long)tile * kMwRows + doc;
            if (m == 0) {                          // padding only, or past the last tile
                if (!GRAD && w < 2 && g == 0 && orow < (long long)p.rows) p.scores_out[orow] = 0.f;
                lds_barrier();                     // (keeps the tiles on either side, of one parity, a barrier apart)
                continue;
            }
            float *pj = part + (size_t)(j & 1) * kMwWaves * kMwRows * kMwPS;
            float *scr = pj + (size_t)w * kMwRows * kMwPS;
            mlp_f4 h1[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
#pragma unroll
                for (int i = 0; i < 4; ++i) h1[u][i] = fmaxf(h1a[j][u][i], 0.f);
                mlp_f4 hp = zero4;
#pragma unroll
                for (int i = 0; i < 4; ++i) hp = mfma16(w2a[i], h1[u][i], hp);
                *reinterpret_cast<mlp_f4 *>(scr + (16 * u + c16) * kMwPS + 4 * g) = hp;
            }
            lds_barrier();                         // B: layer-2 partials (of parity j: rewritten two tiles on)
            const bool own = w < 2;
            mlp_f4 h2 = zero4;
            float s = 0.f;
            if (own) {
                h2 = b2v;
#pragma unroll
                for (int t = 0; t < kMwWaves; ++t) {
                    const mlp_f4 v = *reinterpret_cast<const mlp_f4 *>(pj + ((size_t)t * kMwRows + doc) * kMwPS + 4 * g);
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
                if (own && g == 0 && orow < (long long)p.rows) p.scores_out[orow] = ((m >> doc) & 1u) ? s : 0.f;
                continue;
            }
            // ---- owner wave, backward through layers 3 and 2: dH2 rows -> LDS (g is 0 on padded rows) ----
            if (own) {
                const float ds = gs[j * kMwRows + doc];
                mlp_f4 dh2;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    accW3[i] = __builtin_fmaf(ds, h2[i], accW3[i]);
                    dh2[i] = (h2[i] > 0.f) ? ds * w3v[i] : 0.f;
                    accB2[i] += dh2[i];
                }
                if (g == 0) accB3 += ds;
                *reinterpret_cast<mlp_f4 *>(dH2s + doc * kMwPS + 4 * g) = dh2;
            }
            lds_barrier();                         // C: dH2 rows (rewritten behind barrier B of the next tile)
            // ---- dW2[:, tile] += dH2^T . H1: H1 through the scratch (document-major -> k-major) ----
            {
                const float *tsrc = scr + g * kMwPS + c16;      // transposed reads: [4s + g][c16]
                const float *dsrc = dH2s + g * kMwPS + c16;
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    *reinterpret_cast<mlp_f4 *>(scr + (16 * u + c16) * kMwPS + 4 * g) = h1[u];
                mlp_f4 o = zero4;
#pragma unroll
                for (int sx = 0; sx < 8; ++sx) {
                    const float a = dsrc[4 * sx * kMwPS], bb = tsrc[4 * sx * kMwPS];
                    if (sx & 1) o = mfma16(a, bb, o); else accW2 = mfma16(a, bb, accW2);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) accW2[i] += o[i];
            }
            // ---- dH1^T tile = (W2^T . dH2^T) . [H1 > 0] -> workspace: row (tile, 16u + c16), floats 16w + 4g .. +3 ----
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const mlp_f4 d2 = *reinterpret_cast<const mlp_f4 *>(dH2s + (16 * u + c16) * kMwPS + 4 * g);
                mlp_f4 d1 = zero4;
#pragma unroll
                for (int i = 0; i < 4; ++i) d1 = mfma16(w2t[i], d2[i], d1);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    d1[i] = (h1[u][i] > 0.f) ? d1[i] : 0.f;
                    accB1[i] += d1[i];
                }
                *reinterpret_cast<mlp_f4 *>(p.dH1 + ((size_t)tile * kMwRows + 16 * u + c16) * kMwDH + 16 * w + 4 * g) = d1;
            }
        }
    }
    if (!GRAD) return;

    // ---- this workgroup's partial vector of the small sums [db1 | dW2 | db2 | dW3 | db3] ----
    float *dst = p.part + (size_t)blockIdx.x * p.pitch;
    const int oW2 = H1, oB2 = oW2 + H2 * H1, oW3 = oB2 + H2, oB3 = oW3 + H2;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j2 = 4 * g + i;
        if (j2 < H2 && j1A < H1) dst[oW2 + j2 * H1 + j1A] = accW2[i];
        const float s1 = row16_sum(accB1[i]);
        const int j1 = 16 * w + 4 * g + i;
        if (c16 == 0 && j1 < H1) dst[j1] = s1;
        accB2[i] = row16_sum(accB2[i]);
        accW3[i] = row16_sum(accW3[i]);
    }
    accB3 = wave_sum(accB3);
    // the per-document-owner sums (db2, dW3, db3) fold over the waves in a fixed order
    float *fold = reinterpret_cast<float *>(smem);
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
        for (int k = 0; k < kMwWaves; ++k) t += fold[k * 40 + tid];
        if (tid < 16) { if (tid < H2) dst[oB2 + tid] = t; }
        else if (tid < 32) { if (tid - 16 < H2) dst[oW3 + tid - 16] = t; }
        else dst[oB3] = t;
    }
}

// dW1[:, slice] of the row range: workgroup blockIdx = range * nsl + slice (the workgroups that read the same dH1 rows
// start next to each other), features 16 NTS * slice .. + 16 NTS - 1, tiles range, range + GR, range + 2 GR, ...
template <int NTS>
__global__ void __launch_bounds__(kMwThreads, kMwWgs)
mlp_wide_dw1_kernel(MlpWideParams p, int nsl)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    constexpr int T = kMwThreads;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15;
    const int g = lane >> 4;
    const int L = p.L, F = p.F, H1 = p.H1;
    constexpr int IP = 16 * NTS + 4;                // image pitch (floats): odd number of 16-byte units
    constexpr int C4 = 4 * NTS;                     // float4 units per image row
    constexpr int KP = (kMwRows * C4 + T - 1) / T;  // float4 units of a fill per thread
    const int slice = (int)blockIdx.x % nsl, range = (int)blockIdx.x / nsl;
    const int GR = (int)gridDim.x / nsl;
    const int f0s = slice * 16 * NTS;

    float *img = reinterpret_cast<float *>(smem);                  // [2][32][IP]
    unsigned *vmask = reinterpret_cast<unsigned *>(img + (size_t)2 * kMwRows * IP);        // [3]
    const mlp_f4 zero4 = {0.f, 0.f, 0.f, 0.f};

    mlp_f4 acc[NTS];                                // dW1[j1 = 16w+4g+i][f = f0s + 16c + c16]
#pragma unroll
    for (int c = 0; c < NTS; ++c) acc[c] = zero4;

    int ur[KP], uc[KP];                             // float4 unit tid + 256 k of a fill: image row, float4 of the row
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        ur[k] = (tid + k * T) / C4;
        uc[k] = (tid + k * T) - ur[k] * C4;
    }
    auto tile_meta = [&](int tile, int slot) {
        if (tid < kMwRows) {
            const long long row = (long long)tile * kMwRows + tid;
            bool ok = row < (long long)p.rows;
            if (ok) {
                const int q = (int)row / L, j = (int)row - q * L;
                ok = p.n ? j < clamp_n(p.n[q], L) : true;
            }
            const unsigned long long m = __ballot(ok);
            if (tid == 0) vmask[slot] = (unsigned)m;
        }
    };
    mlp_f4 P[KP];                                   // the fill in flight ...
    float A[8];                                     // ... and its dH1^T operand: [j1 = 16w + c16][doc 4s + g]
    auto issue_fill = [&](int tile, unsigned m) {
        const float *Xt = p.X + (size_t)tile * kMwRows * (size_t)F + f0s;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const bool ok = ur[k] < kMwRows && ((m >> (ur[k] & 31)) & 1u) && f0s + 4 * uc[k] < F;
            const float *src = ok ? Xt + (size_t)ur[k] * F + 4 * uc[k] : p.W1;
            P[k] = *reinterpret_cast<const mlp_f4 *>(src);
        }
        // (every row of a tile with a real row was written by the forward kernel: zeros on its padded rows)
        const float *Dt = p.dH1 + ((size_t)tile * kMwRows + g) * kMwDH + 16 * w + c16;
#pragma unroll
        for (int s = 0; s < 8; ++s) A[s] = Dt[(size_t)4 * s * kMwDH];
    };
    auto fill_image = [&](float *im, unsigned m) {
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const bool ok = ((m >> (ur[k] & 31)) & 1u) && f0s + 4 * uc[k] < F;
            mlp_f4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = ok ? P[k][i] : 0.f;
            if (ur[k] < kMwRows) *reinterpret_cast<mlp_f4 *>(im + ur[k] * IP + 4 * uc[k]) = v;
        }
    };

    int tile = range;
    tile_meta(tile, 0);
    tile_meta(tile + GR, 1);
    __syncthreads();
    {
        const unsigned m0 = __builtin_amdgcn_readfirstlane(vmask[0]);
        if (m0) issue_fill(tile, m0);
    }
    int slot = 0, par = 0;
    for (; tile < p.tiles; tile += GR, par ^= 1) {
        const int slot1 = slot == kMwRing - 1 ? 0 : slot + 1;
        const int slot2 = slot1 == kMwRing - 1 ? 0 : slot1 + 1;
        // (both masks were written in front of a barrier every wave has passed; the slot rewritten below was last
        // read in front of the barrier of the iteration before)
        const unsigned m = __builtin_amdgcn_readfirstlane(vmask[slot]);
        const unsigned mnext = __builtin_amdgcn_readfirstlane(vmask[slot1]);
        float *im = img + (size_t)par * kMwRows * IP;
        float a1[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) a1[s] = 0.f;
        if (m) {
            fill_image(im, m);
#pragma unroll
            for (int s = 0; s < 8; ++s) a1[s] = A[s];
        }
        if (mnext) issue_fill(tile + GR, mnext);   // (past the last tile: mask 0)
        tile_meta(tile + 2 * GR, slot2);
        lds_barrier();                             // image filled (one barrier a tile: the images alternate)
        slot = slot1;
        if (m == 0) continue;
        // ---- dW1[slice] += dH1^T . X: B = image columns; three feature steps in flight (mlp_rows_kernel) ----
        const float *xsrc = im + g * IP + c16;
        constexpr int CG = 3;
#pragma unroll
        for (int c0 = 0; c0 < NTS; c0 += CG) {
#pragma unroll
            for (int s = 0; s < 8; ++s) {
#pragma unroll
                for (int cc = 0; cc < CG; ++cc) {
                    if (c0 + cc < NTS) acc[c0 + cc] = mfma16(a1[s], xsrc[4 * s * IP + 16 * (c0 + cc)], acc[c0 + cc]);
                }
            }
        }
    }

    // ---- this row range's partial dW1, columns of the slice: the D fragments go through a wave-private LDS tile and
    // leave as 16-byte stores of consecutive addresses ----
    __syncthreads();
    float *dst = p.part + (size_t)range * p.pitch;
    float *tile_s = reinterpret_cast<float *>(smem) + (size_t)w * 16 * IP;
#pragma unroll
    for (int c = 0; c < NTS; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) tile_s[(4 * g + i) * IP + 16 * c + c16] = acc[c][i];
    for (int idx = lane; idx < 16 * C4; idx += 64) {
        const int r = idx / C4, f = f0s + 4 * (idx - r * C4);
        if (16 * w + r < H1 && f < F)
            *reinterpret_cast<mlp_f4 *>(dst + (size_t)(16 * w + r) * F + f) =
                *reinterpret_cast<const mlp_f4 *>(tile_s + r * IP + (f - f0s));
    }
}

// ---- host side ----
inline bool mlp_wide_bad_shape(int B, int L, int F, int H1, int H2)
{
    if (B < 0 || L <= 0 || F <= 0 || H1 <= 0 || H2 <= 0) return true;
    if ((F & 3) || F > kMwMaxF || H1 > kMlpH1 || H2 > kMlpH2) return true;
    return (long long)B * L > 0x7fffffffLL;
}

struct MlpWidePlan {
    int tiles;
    int g1;                          // workgroups of the forward kernel = partial vectors of the small sums
    int nsl, nts;                    // dW1 kernel: column slices, 16-feature steps per slice (8 or 11)
    int gr;                          // dW1 kernel: row ranges = partial dW1 matrices
    int pitchA, psmall, pitchB;      // floats: a partial dW1; the small sums and their pitch
    size_t offB, offH, bytes;        // workspace: [gr partial dW1 | g1 small vectors | dH1 rows]
};

inline MlpWidePlan mlp_wide_plan(long long rows, int F, int H1, int H2)
{
    MlpWidePlan s;
    s.tiles = (int)((rows + kMwRows - 1) / kMwRows);
    const long long wgs = (long long)kMwWgs * device_cu_count();
    s.g1 = (int)(s.tiles < wgs ? s.tiles : wgs);
    const int NT = (F + 15) >> 4;
    s.nsl = (NT + 10) / 11;
    s.nts = (NT + s.nsl - 1) / s.nsl <= 8 ? 8 : 11;
    const long long per = wgs / s.nsl > 0 ? wgs / s.nsl : 1;
    s.gr = (int)(s.tiles < per ? s.tiles : per);
    s.pitchA = H1 * F;               // (F % 4 == 0: rows of 16 bytes)
    s.psmall = H1 + H2 * H1 + 2 * H2 + 1;
    s.pitchB = mlp_pitch(s.psmall);
    s.offB = (size_t)s.gr * s.pitchA * sizeof(float);
    s.offH = s.offB + (size_t)s.g1 * s.pitchB * sizeof(float);
    s.bytes = s.offH + (size_t)s.tiles * kMwRows * kMwDH * sizeof(float);
    return s;
}

template <bool GRAD>
int launch_mlp_wide_fwd(const MlpWideParams &p, int grid, hipStream_t stream)
{
    const size_t lds = mlp_wide_fwd_lds_bytes();
    LTR_ENSURE_LDS((mlp_wide_fwd_kernel<GRAD>), lds);
    hipLaunchKernelGGL((mlp_wide_fwd_kernel<GRAD>), dim3((unsigned)grid), dim3(kMwThreads), lds, stream, p);
    return (int)hipGetLastError();
}

template <int NTS>
int launch_mlp_wide_dw1(const MlpWideParams &p, const MlpWidePlan &s, hipStream_t stream)
{
    const size_t lds = mlp_wide_dw1_lds_bytes(NTS);
    LTR_ENSURE_LDS((mlp_wide_dw1_kernel<NTS>), lds);
    hipLaunchKernelGGL((mlp_wide_dw1_kernel<NTS>), dim3((unsigned)(s.gr * s.nsl)), dim3(kMwThreads), lds, stream, p, s.nsl);
    return (int)hipGetLastError();
}

extern "C" {

int ltr_mlp_wide_scores_f32(const float *X, const float *W1, const float *b1, const float *W2, const float *b2,
                            const float *W3, const float *b3, const int64_t *n, int B, int L, int F, int H1, int H2,
                            float *scores_out, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (mlp_wide_bad_shape(B, L, F, H1, H2)) return LTR_ERR_SHAPE;
    if (!W1 || !b1 || !W2 || !b2 || !W3 || !b3) return LTR_ERR_NULL;
    if (B == 0) return LTR_OK;
    if (!X || !scores_out) return LTR_ERR_NULL;
    const MlpWidePlan s = mlp_wide_plan((long long)B * L, F, H1, H2);
    MlpWideParams p;
    p.X = X; p.W1 = W1; p.b1 = b1; p.W2 = W2; p.b2 = b2; p.W3 = W3; p.b3 = b3; p.g = nullptr;
    p.n = n; p.scores_out = scores_out; p.part = nullptr; p.dH1 = nullptr;
    p.B = B; p.L = L; p.F = F; p.H1 = H1; p.H2 = H2;
    p.rows = B * L; p.tiles = s.tiles; p.pitch = 0;
    return launch_mlp_wide_fwd<false>(p, s.g1, (hipStream_t)stream);
}

size_t ltr_mlp_wide_grad_workspace_bytes(int B, int L, int F, int H1, int H2)
{
    if (B <= 0 || mlp_wide_bad_shape(B, L, F, H1, H2)) return 0;
    return mlp_wide_plan((long long)B * L, F, H1, H2).bytes;
}

int ltr_mlp_wide_grad_f32(const float *X, const float *W1, const float *b1, const float *W2, const float *b2,
                          const float *W3, const float *b3, const float *g, const int64_t *n, int B, int L, int F,
                          int H1, int H2, float *grads, void *workspace, size_t workspace_bytes, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (mlp_wide_bad_shape(B, L, F, H1, H2)) return LTR_ERR_SHAPE;
    if (!W1 || !b1 || !W2 || !b2 || !W3 || !b3 || !grads) return LTR_ERR_NULL;
    const int P = mlp_param_count(F, H1, H2);
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) return mlp_reduce_launch(nullptr, 0, P, grads, nullptr, 0, nullptr, st);     // zero gradients
    if (!X || !g) return LTR_ERR_NULL;
    const MlpWidePlan s = mlp_wide_plan((long long)B * L, F, H1, H2);
    if (!workspace || workspace_bytes < s.bytes) return LTR_ERR_WORKSPACE;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    MlpWideParams p;
    p.X = X; p.W1 = W1; p.b1 = b1; p.W2 = W2; p.b2 = b2; p.W3 = W3; p.b3 = b3; p.g = g;
    p.n = n; p.scores_out = nullptr;
    p.dH1 = reinterpret_cast<float *>(ws + s.offH);
    p.B = B; p.L = L; p.F = F; p.H1 = H1; p.H2 = H2;
    p.rows = B * L; p.tiles = s.tiles;
    // forward and back down to dH1; the small sums, one partial vector per workgroup
    p.part = reinterpret_cast<float *>(ws + s.offB); p.pitch = s.pitchB;
    int rc = launch_mlp_wide_fwd<true>(p, s.g1, st);
    if (rc != 0) return rc;
    // dW1, one partial matrix per row range
    p.part = reinterpret_cast<float *>(ws); p.pitch = s.pitchA;
    rc = s.nts == 8 ? launch_mlp_wide_dw1<8>(p, s, st) : launch_mlp_wide_dw1<11>(p, s, st);
    if (rc != 0) return rc;
    // grads = [dW1 | the small sums]: both sums in a fixed order (H1 * F floats are whole 16-byte units)
    rc = mlp_reduce_launch(ws, s.gr, s.pitchA, grads, nullptr, 0, nullptr, st);
    if (rc != 0) return rc;
    return mlp_reduce_launch(ws + s.offB, s.g1, s.psmall, grads + s.pitchA, nullptr, 0, nullptr, st);
}

}  // extern "C"
