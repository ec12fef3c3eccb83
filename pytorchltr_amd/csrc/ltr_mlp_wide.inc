// ltr_mlp_wide.inc -- the ReLU-MLP scorer (F -> H1 -> H2 -> 1) on WIDE feature rows, up to 704 features: K-streamed
// score and parameter-gradient kernels on v_mfma_f32_16x16x4_f32 for lists of any length (include/ltr_mlp_wide.h).
// Included by ltr_mlp.hip behind ltr_mlp_stream.inc, whose fragments, row test, owner waves, f32 backward chains and
// epilogue it calls, and whose host glue it shares.
//
// The row kernels (ltr_mlp_rows.inc) keep a wave's W1 fragments, and the gradient kernel its dW1 tile, in registers for
// the workgroup's whole life: 56 + 56 registers at 224 features, 176 + 176 at 704, where W1 itself (176 KiB) is more
// than the LDS.  Here the feature dimension is walked in CHUNKS of 128 features instead.  The unit of work, the mask
// (`row % L < n[row / L]`), the persistent grid and the tile order (workgroup w takes the tiles w, w + G, w + 2G, ...)
// are those of ltr_mlp_stream.inc; so is the wave layout (four waves, wave w owns hidden-1 rows 16w .. 16w + 15).
//
// Forward (mlp_wide_fwd_kernel): a workgroup takes its tiles in GROUPS of eight (scores; four in front of the backward
// half, mlp_wide_group) and keeps the layer-1 accumulators of the whole group in registers (8 per tile).  Chunk loop
// outside, tile loop inside:
//     for chunk:  W1 fragments of the chunk <- global (32 registers, L2-resident: one 176 KiB pass over W1 per GROUP,
//                 i.e. per 720 / 360 KB of X at F = 704)
//         for tile of the group:  image[parity] <- the tile's 32 x 128 piece of X (requested one step ahead; the address
//                 select of the row kernels keeps padded rows unread)                                 one barrier
//                 64 MFMAs per wave into the tile's accumulators
//     for tile of the group:  layers 2 and 3 and the score store as in mlp_stream_body; GRAD: dH2 rows, the dW2 tile,
//                 the small sums, and the tile's d loss / d hidden-1 (zeros on padded rows) -> workspace, 256 B a row
// The image and the layer-2 partials are double buffered by step / tile parity, which is what lets one barrier a step do.
// Which rows of a group are real is worked out once per group: 256 threads, one row each, two tiles per ballot.
//
// Gradient, second kernel (mlp_wide_dw1_kernel): dW1 = dH1^T . X over (column slice of 128 or 176 features) x (row
// range): the f32 dW1 chain of the row kernel (mlp_dw1_chain_f32) with the A operand read from the workspace and a dW1 slice of 32 / 44
// registers per lane; X is read a second time.  One partial dW1 per row range, one partial vector of the small sums per
// workgroup of the first kernel, two launches of mlp_reduce_launch(loss = NULL) add them in a fixed order.  No atomics.
// DESIGN.md section 19 has the choice between this and a one-kernel gradient, the register / LDS table and the bytes.
#pragma once

#include "ltr_mlp_wide.h"

constexpr int kMwMaxF = 704;
constexpr int kMwNTC = 8;             // 16-feature steps per chunk
constexpr int kMwKC = 16 * kMwNTC;    // features per chunk
constexpr int kMwIP = kMwKC + 4;      // image pitch (floats): odd number of 16-byte units
constexpr int kMwTG = kMsThreads / kMsRows;      // most tiles per group: one thread per row works out the masks
// tiles per group: eight for the scores; four for the gradient's forward kernel, whose backward fragments and sums
// (37 registers) next to eight tiles' accumulators spilled 30 registers under the 256 of two workgroups per CU
constexpr int mlp_wide_group(bool grad) { return grad ? 4 : kMwTG; }
constexpr int kMwDH = 64;             // floats per flat row of the d loss / d hidden-1 tile in the workspace

constexpr size_t mlp_wide_fwd_lds_bytes()
{
    return ((size_t)2 * kMsRows * kMwIP + (size_t)2 * kMsWaves * kMsRows * kMsPS + (size_t)kMsRows * kMsPS +
            (size_t)kMwTG * kMsRows + kMwTG + 8) * sizeof(float);
}
constexpr size_t mlp_wide_dw1_lds_bytes(int NTS)
{
    // two images [32][16 NTS + 4]; the four dW1 tiles (64 image rows) are staged in the same floats at the end
    return ((size_t)2 * kMsRows * (16 * NTS + 4) + 8) * sizeof(float);
}
static_assert(mlp_wide_fwd_lds_bytes() <= kLdsBudget / kMsWgs && mlp_wide_dw1_lds_bytes(11) <= kLdsBudget / kMsWgs,
              "two workgroups per CU");

template <bool GRAD>
__global__ void __launch_bounds__(kMsThreads, kMsWgs)
mlp_wide_fwd_kernel(MlpStreamParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const MlpLane ln = mlp_lane();
    const int tid = ln.tid, lane = ln.lane, w = ln.w, c16 = ln.c16, g = ln.g;
    const int F = p.F;
    const float *X = static_cast<const float *>(p.X);
    const int NC = (F + kMwKC - 1) / kMwKC;         // feature chunks
    constexpr int IP = kMwIP;
    constexpr int TG = mlp_wide_group(GRAD);        // tiles per group
    static_assert(TG % 2 == 0 && TG <= kMwTG, "buffers alternate by tile parity across the chunks");

    float *img = reinterpret_cast<float *>(smem);                  // [2][32][IP]    the piece of X of a step
    float *part = img + (size_t)2 * kMsRows * IP;                  // [2][4][32][20] layer-2 partials / wave scratch
    float *dH2s = part + (size_t)2 * kMsWaves * kMsRows * kMsPS;   // [32][20]
    float *gs = dH2s + (size_t)kMsRows * kMsPS;                    // [8][32]        d loss / d score of the group's rows
    unsigned *vmask = reinterpret_cast<unsigned *>(gs + kMwTG * kMsRows);      // [8] bit r: row r of tile j is real

    const mlp_f4 zero4 = {0.f, 0.f, 0.f, 0.f};

    const MlpSmallFrags sf = mlp_small_frags(p, ln);            // (the W1 fragments exist per chunk)
    MlpSmallSums sums = mlp_small_sums_zero();

    // A step moves a 32 x 128 piece of X: 1024 float4 units, four per thread -- rows fr, fr + 8, fr + 16, fr + 24 of
    // the tile, 16 bytes at float 4 fc of the chunk
    const int fr = tid >> 5, fc = tid & 31;
    mlp_f4 P[4];                                    // the piece in flight
    auto issue_fill = [&](int tile, int ch, unsigned m) {
        const int f = ch * kMwKC + 4 * fc;
        const float *Xt = X + ((size_t)tile * kMsRows + fr) * (size_t)F + f;
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
            const long long row = (long long)tile * kMsRows + fc;
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

        mlp_f4 h1a[TG][2];                      // layer-1 pre-activations of the group: [j1 = 16w+4g+i][doc c16]
#pragma unroll
        for (int j = 0; j < TG; ++j) { h1a[j][0] = sf.b1v; h1a[j][1] = sf.b1v; }

        // ---- layer 1: chunk loop outside, tile loop inside ----
        unsigned mcur = __builtin_amdgcn_readfirstlane(vmask[0]);
        if (mcur) issue_fill(t0, 0, mcur);
        for (int ch = 0; ch < NC; ++ch) {
            mlp_f4 w1r[kMwNTC];                     // W1[j1A][128 ch + 16c + 4g .. +3]
            mlp_load_w1_f32<kMwNTC>(w1r, p, ln, ch * kMwKC);
            const bool hi = F - ch * kMwKC > kMwKC / 2;         // the chunk's upper 64 features exist (uniform)
#pragma unroll
            for (int j = 0; j < TG; ++j) {
                float *im = img + (size_t)(j & 1) * kMsRows * IP;
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

        // ---- layers 2 and 3 of every tile of the group (as in mlp_stream_body), GRAD: and back down to dH1 ----
#pragma unroll
        for (int j = 0; j < TG; ++j) {
            const unsigned m = __builtin_amdgcn_readfirstlane(vmask[j]);
            const int tile = t0 + j * G;
            const int doc = 16 * w + c16;          // owner waves 0, 1: the row of the tile this lane finishes
            const long long orow = (long long)tile * kMsRows + doc;
            if (m == 0) {                          // padding only, or past the last tile
                if (!GRAD && w < 2 && g == 0 && orow < (long long)p.rows) p.scores_out[orow] = 0.f;
                lds_barrier();                     // (keeps the tiles on either side, of one parity, a barrier apart)
                continue;
            }
            float *pj = part + (size_t)(j & 1) * kMsWaves * kMsRows * kMsPS;
            float *scr = pj + (size_t)w * kMsRows * kMsPS;
            mlp_f4 h1[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                h1[u] = h1a[j][u];
                mlp_layer2_partial(sf, h1[u], scr + (16 * u + c16) * kMsPS + 4 * g);
            }
            lds_barrier();                         // B: layer-2 partials (of parity j: rewritten two tiles on)
            const bool own = w < 2;
            mlp_f4 h2 = zero4;
            float s = 0.f;
            if (own) s = mlp_owner_fwd(sf, pj, doc, g, h2);
            if (!GRAD) {
                if (own && g == 0 && orow < (long long)p.rows) p.scores_out[orow] = ((m >> doc) & 1u) ? s : 0.f;
                continue;
            }
            if (own) mlp_owner_bwd(sf, sums, h2, gs[j * kMsRows + doc], dH2s, doc, g);
            lds_barrier();                         // C: dH2 rows (rewritten behind barrier B of the next tile)
            mlp_dw2_tile<2>(sums, h1, scr, dH2s, 0, ln);
            // the dH1^T tile -> workspace: row (tile, 16u + c16), floats 16w + 4g .. +3
            mlp_dh1_tile<2>(sf, sums, h1, dH2s, 0, ln, [&](int u, const mlp_f4 &d1) {
                *reinterpret_cast<mlp_f4 *>(p.dH1 + ((size_t)tile * kMsRows + 16 * u + c16) * kMwDH + 16 * w + 4 * g) = d1;
            });
        }
    }
    if (!GRAD) return;

    // ---- this workgroup's partial vector of the small sums [db1 | dW2 | db2 | dW3 | db3] ----
    float *dst = p.part + (size_t)blockIdx.x * p.pitch;
    __syncthreads();
    mlp_store_small_sums(sums, dst, 0, reinterpret_cast<float *>(smem), p, ln);
}

// dW1[:, slice] of the row range: workgroup blockIdx = range * nsl + slice (the workgroups that read the same dH1 rows
// start next to each other), features 16 NTS * slice .. + 16 NTS - 1, tiles range, range + GR, range + 2 GR, ...
template <int NTS>
__global__ void __launch_bounds__(kMsThreads, kMsWgs)
mlp_wide_dw1_kernel(MlpStreamParams p, int nsl)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const MlpLane ln = mlp_lane();
    const int tid = ln.tid, w = ln.w, c16 = ln.c16, g = ln.g;
    constexpr int T = kMsThreads;
    const int F = p.F;
    const float *X = static_cast<const float *>(p.X);
    constexpr int IP = 16 * NTS + 4;                // image pitch (floats): odd number of 16-byte units
    constexpr int C4 = 4 * NTS;                     // float4 units per image row
    constexpr int KP = (kMsRows * C4 + T - 1) / T;  // float4 units of a fill per thread
    const int slice = (int)blockIdx.x % nsl, range = (int)blockIdx.x / nsl;
    const int GR = (int)gridDim.x / nsl;
    const int f0s = slice * 16 * NTS;

    float *img = reinterpret_cast<float *>(smem);                  // [2][32][IP]
    unsigned *vmask = reinterpret_cast<unsigned *>(img + (size_t)2 * kMsRows * IP);        // [3]
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
    mlp_f4 P[KP];                                   // the fill in flight ...
    float A[8];                                     // ... and its dH1^T operand: [j1 = 16w + c16][doc 4s + g]
    auto issue_fill = [&](int tile, unsigned m) {
        const float *Xt = X + (size_t)tile * kMsRows * (size_t)F + f0s;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const bool ok = ur[k] < kMsRows && ((m >> (ur[k] & 31)) & 1u) && f0s + 4 * uc[k] < F;
            const float *src = ok ? Xt + (size_t)ur[k] * F + 4 * uc[k] : p.W1;
            P[k] = *reinterpret_cast<const mlp_f4 *>(src);
        }
        // (every row of a tile with a real row was written by the forward kernel: zeros on its padded rows)
        const float *Dt = p.dH1 + ((size_t)tile * kMsRows + g) * kMwDH + 16 * w + c16;
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
        float a1[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) a1[s] = 0.f;
        if (m) {
            fill_image(im, m);
#pragma unroll
            for (int s = 0; s < 8; ++s) a1[s] = A[s];
        }
        if (mnext) issue_fill(tile + GR, mnext);   // (past the last tile: mask 0)
        mlp_ring_write<false>(p, tid, tile + 2 * GR, slot2, vmask, nullptr);
        lds_barrier();                             // image filled (one barrier a tile: the images alternate)
        slot = slot1;
        if (m == 0) continue;
        mlp_dw1_chain_f32<NTS, IP>(acc, a1, im + g * IP + c16);     // dW1[slice] += dH1^T . X: B = image columns
    }

    // ---- this row range's partial dW1, columns of the slice ----
    __syncthreads();
    mlp_store_dw1<NTS, IP>(acc, reinterpret_cast<float *>(smem), p.part + (size_t)range * p.pitch, p, f0s, C4, ln);
}

// ---- host side ----
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
    s.tiles = (int)((rows + kMsRows - 1) / kMsRows);
    const long long wgs = (long long)kMsWgs * device_cu_count();
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
    s.bytes = s.offH + (size_t)s.tiles * kMsRows * kMwDH * sizeof(float);
    return s;
}

template <bool GRAD>
int launch_mlp_wide_fwd(const MlpStreamParams &p, int grid, hipStream_t stream)
{
    const size_t lds = mlp_wide_fwd_lds_bytes();
    LTR_ENSURE_LDS((mlp_wide_fwd_kernel<GRAD>), lds);
    hipLaunchKernelGGL((mlp_wide_fwd_kernel<GRAD>), dim3((unsigned)grid), dim3(kMsThreads), lds, stream, p);
    return (int)hipGetLastError();
}

template <int NTS>
int launch_mlp_wide_dw1(const MlpStreamParams &p, const MlpWidePlan &s, hipStream_t stream)
{
    const size_t lds = mlp_wide_dw1_lds_bytes(NTS);
    LTR_ENSURE_LDS((mlp_wide_dw1_kernel<NTS>), lds);
    hipLaunchKernelGGL((mlp_wide_dw1_kernel<NTS>), dim3((unsigned)(s.gr * s.nsl)), dim3(kMsThreads), lds, stream, p, s.nsl);
    return (int)hipGetLastError();
}

extern "C" {

int ltr_mlp_wide_scores_f32(const float *X, const float *W1, const float *b1, const float *W2, const float *b2,
                            const float *W3, const float *b3, const int64_t *n, int B, int L, int F, int H1, int H2,
                            float *scores_out, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (mlp_stream_bad_shape(B, L, F, H1, H2, 4, kMwMaxF)) return LTR_ERR_SHAPE;
    if (!W1 || !b1 || !W2 || !b2 || !W3 || !b3) return LTR_ERR_NULL;
    if (B == 0) return LTR_OK;
    if (!X || !scores_out) return LTR_ERR_NULL;
    const MlpWidePlan s = mlp_wide_plan((long long)B * L, F, H1, H2);
    MlpStreamParams p = mlp_stream_params(X, W1, b1, W2, b2, W3, b3, nullptr, n, B, L, F, H1, H2);
    p.scores_out = scores_out;
    return launch_mlp_wide_fwd<false>(p, s.g1, (hipStream_t)stream);
}

size_t ltr_mlp_wide_grad_workspace_bytes(int B, int L, int F, int H1, int H2)
{
    if (B <= 0 || mlp_stream_bad_shape(B, L, F, H1, H2, 4, kMwMaxF)) return 0;
    return mlp_wide_plan((long long)B * L, F, H1, H2).bytes;
}

int ltr_mlp_wide_grad_f32(const float *X, const float *W1, const float *b1, const float *W2, const float *b2,
                          const float *W3, const float *b3, const float *g, const int64_t *n, int B, int L, int F,
                          int H1, int H2, float *grads, void *workspace, size_t workspace_bytes, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (mlp_stream_bad_shape(B, L, F, H1, H2, 4, kMwMaxF)) return LTR_ERR_SHAPE;
    if (!W1 || !b1 || !W2 || !b2 || !W3 || !b3 || !grads) return LTR_ERR_NULL;
    const int P = mlp_param_count(F, H1, H2);
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) return mlp_reduce_launch(nullptr, 0, P, grads, nullptr, 0, nullptr, st);     // zero gradients
    if (!X || !g) return LTR_ERR_NULL;
    const MlpWidePlan s = mlp_wide_plan((long long)B * L, F, H1, H2);
    if (!workspace || workspace_bytes < s.bytes) return LTR_ERR_WORKSPACE;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    MlpStreamParams p = mlp_stream_params(X, W1, b1, W2, b2, W3, b3, g, n, B, L, F, H1, H2);
    p.dH1 = reinterpret_cast<float *>(ws + s.offH);
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
