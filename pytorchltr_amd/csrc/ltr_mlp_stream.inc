// ltr_mlp_stream.inc -- what the stand-alone ReLU-MLP scorer kernels (F -> H1 -> H2 -> 1) share: the device layer under
// ltr_mlp_rows.inc (f32 rows), ltr_mlp_bf16.inc (bf16 rows) and ltr_mlp_wide.inc (K-streamed wide rows), the one
// streaming kernel body of the first two, and the host glue of all three.  Included by ltr_mlp.hip behind ltr_mlp.inc,
// whose mfma16 and padding rules it uses (the reduction: ltr_mlp_reduce.inc), and in front of those three files.
//
// The unit of work is a TILE of 32 consecutive FLAT rows of the (B * L, F) matrix; a row is real iff
// row % L < n[row / L].  Four waves; wave w owns hidden-1 rows 16w .. 16w+15 (W1 / W2 fragments in registers, transposed
// activations so that a D fragment is the next B operand: the layout of ltr_mlp2.inc); waves 0 and 1 also OWN the 16
// documents of one subtile each: they add the four layer-2 partial tiles and finish layers 2 and 3.
// mlp_stream_body is the row-streaming kernel.  g is known up front, so a fill goes forward and straight back:
//     (fill n+1 requested)  image <- fill n                                              barrier A
//     layer 1 tile, layer-2 partial tile -> LDS      (Front::layer1)                           barrier B
//     owner waves 0, 1: layers 2 + 3 of 16 documents each -> score; GRAD: dH2 rows -> LDS    barrier C   (GRAD only)
//     GRAD: dW2 tile, dH1 tile, dW1 tile += ...      (Front::dw1)                              barrier D   (GRAD only)
// A subtile of 16 rows that is all padding is skipped by the forward chains; a tile of padding only costs its barrier A.
// Loads stay unconditional: the 16 bytes of a padded row are requested from the head of W1 instead and replaced by zeros
// on their way into the image, so padded rows of X are never read; g is read for real rows only.
// Which rows of a tile are real is worked out two tiles ahead by 32 lanes (one division each; a 32-bit mask and the
// 32 values of g per tile in a three-deep LDS ring), so the address select of the next fill has its mask in time.
// Persistent grid: workgroup w takes the tiles w, w + G, w + 2G, ... (fixed order); the dW1 / dW2 tiles live in
// registers for the workgroup's whole life, one partial vector per workgroup, mlp_reduce_launch(loss = NULL) adds them
// in a fixed order.  No atomics: bit-identical run to run.
// A FRONT (MlpFrontF32<NT>, MlpFrontBf16<KS>) supplies what depends on the element type of X: the image, the W1
// fragments, layer 1 and the dW1 step.  The wide kernels keep their own loop nests and call the pieces.
// ltr_mlp2.inc (mlp_tile_kernel, the timed MLP step) holds its own copy of the small fragments and of the epilogue and
// has NOT adopted these helpers: its widest instantiations sit at exactly 256 VGPRs.  DESIGN.md sections 18 - 20.
#pragma once

constexpr int kMsThreads = 256;
constexpr int kMsWaves = 4;
constexpr int kMsRows = 32;          // flat rows per tile (two 16-row subtiles)
constexpr int kMsWgs = 2;            // workgroups per CU the launch bounds and the grids are sized for
constexpr int kMsPS = 20;            // row pitch (floats) of the partial / scratch / dH2 images
constexpr int kMsRing = 3;           // tiles whose row mask / g values are kept in LDS
constexpr int kMsFold = 40;          // floats per wave of the fold of the small sums: [16] db2 | [16] dW3 | [1] db3

typedef __attribute__((ext_vector_type(4))) int mlp_i4;      // 16 bytes of X on their way into the image

struct MlpStreamParams {
    const void *X;                   // float or bf16 rows (the front knows)
    const float *W1, *b1, *W2, *b2, *W3, *b3, *g;
    const int64_t *n;
    float *scores_out;
    float *part;                     // partial vectors (wide: of the small sums, then the partial dW1 matrices)
    float *dH1;                      // wide only: [tiles * 32][64]; NULL elsewhere
    int B, L, F, H1, H2;
    int rows;                        // B * L
    int tiles;                       // ceil(rows / 32)
    int pitch;                       // floats between consecutive partial vectors of `part`
};

struct MlpLane {
    int tid, lane, w, c16, g;        // thread, lane of the wave, wave (uniform), lane & 15, lane >> 4
    int j1A;                         // hidden-1 row as an A-operand row: 16 w + c16
};
__device__ __forceinline__ MlpLane mlp_lane()
{
    MlpLane ln;
    ln.tid = threadIdx.x;
    ln.lane = ln.tid & 63;
    ln.w = __builtin_amdgcn_readfirstlane(ln.tid >> 6);
    ln.c16 = ln.lane & 15;
    ln.g = ln.lane >> 4;
    ln.j1A = 16 * ln.w + ln.c16;
    return ln;
}

// ---- this wave's small weight fragments, straight from global memory into registers (ltr_mlp2.inc) ----
struct MlpSmallFrags {
    mlp_f4 b1v, w2a, w2t, b2v, w3v;
    float b3;
};
__device__ __forceinline__ MlpSmallFrags mlp_small_frags(const MlpStreamParams &p, const MlpLane &ln)
{
    MlpSmallFrags fr;
    const int H1 = p.H1, H2 = p.H2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j1D = 16 * ln.w + 4 * ln.g + i;   // hidden-1 row as a D-fragment row
        const int j2D = 4 * ln.g + i;               // hidden-2 row as a D-fragment row
        const bool ok1 = j1D < H1, ok2 = j2D < H2;
        const float vb1 = p.b1[ok1 ? j1D : 0];
        fr.b1v[i] = ok1 ? vb1 : 0.f;
        const bool oka = ln.c16 < H2 && ok1;        // layer 2:  A[row j2 = c16][k <-> j1D]
        const float va = p.W2[oka ? (size_t)ln.c16 * H1 + j1D : 0];
        fr.w2a[i] = oka ? va : 0.f;
        const bool okt = ok2 && ln.j1A < H1;        // dH1:      A[row j1A][k <-> j2D]
        const float vt = p.W2[okt ? (size_t)j2D * H1 + ln.j1A : 0];
        fr.w2t[i] = okt ? vt : 0.f;
        const float vb2 = p.b2[ok2 ? j2D : 0], v3 = p.W3[ok2 ? j2D : 0];
        fr.b2v[i] = ok2 ? vb2 : 0.f;
        fr.w3v[i] = ok2 ? v3 : 0.f;
    }
    fr.b3 = p.b3[0];
    return fr;
}
// N f32 W1 fragments of 16 features each: W1[j1A][fbase + 16c + 4g .. +3], zeros past H1 / F
template <int N>
__device__ __forceinline__ void mlp_load_w1_f32(mlp_f4 (&w1r)[N], const MlpStreamParams &p, const MlpLane &ln, int fbase)
{
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const int f0 = fbase + 16 * c + 4 * ln.g;
        const bool ok = ln.j1A < p.H1 && f0 < p.F;
        const mlp_f4 v = *reinterpret_cast<const mlp_f4 *>(p.W1 + (ok ? (size_t)ln.j1A * p.F + f0 : 0));
#pragma unroll
        for (int i = 0; i < 4; ++i) w1r[c][i] = ok ? v[i] : 0.f;
    }
}

// ---- the small accumulators that live across the tiles (disjoint between the waves) ----
struct MlpSmallSums {
    mlp_f4 accW2;                    // dW2[j2 = 4g+i][j1 = 16w + c16]
    mlp_f4 accB1;                    // db1[j1 = 16w+4g+i], partial over this lane's documents
    mlp_f4 accB2, accW3;             // db2 / dW3 [j2 = 4g+i], documents this wave finished
    float accB3;
};
__device__ __forceinline__ MlpSmallSums mlp_small_sums_zero()
{
    const mlp_f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    return MlpSmallSums{zero4, zero4, zero4, zero4, 0.f};
}

// ---- the row test: flat row `row` (inside: it exists at all) is real iff row % L < clamp_n(n[row / L], L), n == NULL:
//      every row; gv = its d loss / d score (GRAD, real rows only -- g of a padded row is never read), else 0 ----
template <bool GRAD>
__device__ __forceinline__ bool mlp_row_real(const MlpStreamParams &p, bool inside, long long row, float &gv)
{
    bool ok = inside;
    gv = 0.f;
    if (ok) {
        const int q = (int)row / p.L, j = (int)row - q * p.L;
        ok = p.n ? j < clamp_n(p.n[q], p.L) : true;
        if (GRAD && ok) gv = p.g[row];
    }
    return ok;
}
// ---- the ring: which rows of a tile are real, and their g: lanes 0 .. 31 of wave 0, into slot `slot` ----
template <bool GRAD>
__device__ __forceinline__ void mlp_ring_write(const MlpStreamParams &p, int tid, int tile, int slot, unsigned *vmask,
                                               float *gs)
{
    if (tid < kMsRows) {
        const long long row = (long long)tile * kMsRows + tid;
        float gv;
        const bool ok = mlp_row_real<GRAD>(p, row < (long long)p.rows, row, gv);
        const unsigned long long m = __ballot(ok);
        if (GRAD) gs[slot * kMsRows + tid] = gv;
        if (tid == 0) vmask[slot] = (unsigned)m;
    }
}
__device__ __forceinline__ int mlp_ring_next(int slot) { return slot == kMsRing - 1 ? 0 : slot + 1; }

// ---- tile wave: ReLU of a layer-1 subtile (kept in h1), its layer-2 partial tile -> dst[doc c16][4g ..] ----
__device__ __forceinline__ void mlp_layer2_partial(const MlpSmallFrags &fr, mlp_f4 &h1, float *dst)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) h1[i] = fmaxf(h1[i], 0.f);
    mlp_f4 hp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) hp = mfma16(fr.w2a[i], h1[i], hp);
    *reinterpret_cast<mlp_f4 *>(dst) = hp;
}
// ---- owner wave: the four partial tiles [4][32][20] of its document, layers 2 (bias, relu) and 3 -> score ----
__device__ __forceinline__ float mlp_owner_fwd(const MlpSmallFrags &fr, const float *part, int doc, int g, mlp_f4 &h2)
{
    float s = 0.f;
    h2 = fr.b2v;
#pragma unroll
    for (int t = 0; t < kMsWaves; ++t) {
        const mlp_f4 v = *reinterpret_cast<const mlp_f4 *>(part + ((size_t)t * kMsRows + doc) * kMsPS + 4 * g);
#pragma unroll
        for (int i = 0; i < 4; ++i) h2[i] += v[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        h2[i] = fmaxf(h2[i], 0.f);
        s = __builtin_fmaf(fr.w3v[i], h2[i], s);
    }
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    return s + fr.b3;
}
// ---- owner wave, backward through layers 3 and 2: dH2 row of its document -> LDS (ds is 0 on padded rows) ----
__device__ __forceinline__ void mlp_owner_bwd(const MlpSmallFrags &fr, MlpSmallSums &a, const mlp_f4 &h2, float ds,
                                              float *dH2s, int doc, int g)
{
    mlp_f4 dh2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        a.accW3[i] = __builtin_fmaf(ds, h2[i], a.accW3[i]);
        dh2[i] = (h2[i] > 0.f) ? ds * fr.w3v[i] : 0.f;
        a.accB2[i] += dh2[i];
    }
    if (g == 0) a.accB3 += ds;
    *reinterpret_cast<mlp_f4 *>(dH2s + doc * kMsPS + 4 * g) = dh2;
}

// ---- tile wave, backward over subtiles u0 .. u0 + NS - 1: dW2[:, tile] += dH2^T . H1, H1 through the wave's scratch
//      (document-major -> k-major) ----
template <int NS>
__device__ __forceinline__ void mlp_dw2_tile(MlpSmallSums &a, const mlp_f4 (&h1)[2], float *scr, const float *dH2s,
                                             int u0, const MlpLane &ln)
{
    const float *tsrc = scr + ln.g * kMsPS + ln.c16;            // transposed reads: [4s + g][c16]
    const float *dsrc = dH2s + (16 * u0 + ln.g) * kMsPS + ln.c16;
#pragma unroll
    for (int u = 0; u < NS; ++u) *reinterpret_cast<mlp_f4 *>(scr + (16 * u + ln.c16) * kMsPS + 4 * ln.g) = h1[u];
    mlp_f4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 4 * NS; ++s) {
        const float av = dsrc[4 * s * kMsPS], bb = tsrc[4 * s * kMsPS];
        if (s & 1) o = mfma16(av, bb, o); else a.accW2 = mfma16(av, bb, a.accW2);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) a.accW2[i] += o[i];
}
// ---- dH1^T tile = (W2^T . dH2^T) . [H1 > 0] -> sink(u, d1): subtile u of the chain, rows j1 = 16w+4g+i of doc c16 ----
template <int NS, class Sink>
__device__ __forceinline__ void mlp_dh1_tile(const MlpSmallFrags &fr, MlpSmallSums &a, const mlp_f4 (&h1)[2],
                                             const float *dH2s, int u0, const MlpLane &ln, Sink sink)
{
#pragma unroll
    for (int u = 0; u < NS; ++u) {
        const mlp_f4 d2 = *reinterpret_cast<const mlp_f4 *>(dH2s + (16 * (u0 + u) + ln.c16) * kMsPS + 4 * ln.g);
        mlp_f4 d1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) d1 = mfma16(fr.w2t[i], d2[i], d1);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            d1[i] = (h1[u][i] > 0.f) ? d1[i] : 0.f;
            a.accB1[i] += d1[i];
        }
        sink(u, d1);
    }
}
// ---- dW1 += dH1^T . X in f32: A = a1[s] (dH1^T[j1 = 16w + c16][doc 4s + g]), B = image columns from xsrc (row g, column
//      c16 of the first subtile; pitch IP); three feature steps in flight ----
template <int NT, int IP, int NK>
__device__ __forceinline__ void mlp_dw1_chain_f32(mlp_f4 (&acc)[NT], const float (&a1)[NK], const float *xsrc)
{
    constexpr int CG = 3;
#pragma unroll
    for (int c0 = 0; c0 < NT; c0 += CG) {
#pragma unroll
        for (int s = 0; s < NK; ++s) {
#pragma unroll
            for (int cc = 0; cc < CG; ++cc) {
                if (c0 + cc < NT) acc[c0 + cc] = mfma16(a1[s], xsrc[4 * s * IP + 16 * (c0 + cc)], acc[c0 + cc]);
            }
        }
    }
}

// ---- epilogue, dW1: rows 16w .. 16w+15 of dst[H1][F], columns f0s .. f0s + 4 CW - 1 (and < F); the D fragments go
//      through a wave-private LDS tile (pitch SP floats, from the start of the segment) and leave as 16-byte stores of
//      consecutive addresses ----
template <int NC, int SP>
__device__ __forceinline__ void mlp_store_dw1(const mlp_f4 (&acc)[NC], float *lds, float *dst, const MlpStreamParams &p,
                                              int f0s, int CW, const MlpLane &ln)
{
    float *tile_s = lds + (size_t)ln.w * 16 * SP;
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) tile_s[(4 * ln.g + i) * SP + 16 * c + ln.c16] = acc[c][i];
    for (int idx = ln.lane; idx < 16 * CW; idx += 64) {
        const int r = idx / CW, f4 = idx - r * CW, f = f0s + 4 * f4;
        if (16 * ln.w + r < p.H1 && f < p.F)
            *reinterpret_cast<mlp_f4 *>(dst + (size_t)(16 * ln.w + r) * p.F + f) =
                *reinterpret_cast<const mlp_f4 *>(tile_s + r * SP + 4 * f4);
    }
}
// ---- epilogue, the small sums [db1 | dW2 | db2 | dW3 | db3] at dst + oB1; the per-document-owner sums (db2, dW3, db3)
//      fold over the waves in a fixed order through `fold` ([4][40] floats of LDS no wave still reads) ----
__device__ __forceinline__ void mlp_store_small_sums(MlpSmallSums &a, float *dst, int oB1, float *fold,
                                                     const MlpStreamParams &p, const MlpLane &ln)
{
    const int H1 = p.H1, H2 = p.H2;
    const int oW2 = oB1 + H1, oB2 = oW2 + H2 * H1, oW3 = oB2 + H2, oB3 = oW3 + H2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j2 = 4 * ln.g + i;
        if (j2 < H2 && ln.j1A < H1) dst[oW2 + j2 * H1 + ln.j1A] = a.accW2[i];
        const float s1 = row16_sum(a.accB1[i]);
        const int j1 = 16 * ln.w + 4 * ln.g + i;
        if (ln.c16 == 0 && j1 < H1) dst[oB1 + j1] = s1;
        a.accB2[i] = row16_sum(a.accB2[i]);
        a.accW3[i] = row16_sum(a.accW3[i]);
    }
    a.accB3 = wave_sum(a.accB3);
    float *slv = fold + (size_t)ln.w * kMsFold;    // [16] db2 | [16] dW3 | [1] db3
    if (ln.c16 == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            slv[4 * ln.g + i] = a.accB2[i];
            slv[16 + 4 * ln.g + i] = a.accW3[i];
        }
    }
    if (ln.lane == 0) slv[32] = a.accB3;
    __syncthreads();
    if (ln.tid < 33) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < kMsWaves; ++k) t += fold[k * kMsFold + ln.tid];
        if (ln.tid < 16) { if (ln.tid < H2) dst[oB2 + ln.tid] = t; }
        else if (ln.tid < 32) { if (ln.tid - 16 < H2) dst[oW3 + ln.tid - 16] = t; }
        else dst[oB3] = t;
    }
}

// LDS bytes of mlp_stream_body: an image of 32 rows of `row_bytes`; the gradient kernel stages its four dW1 tiles
// (64 rows of `sp` floats) and the fold of the small sums in the same bytes at the end
__host__ __device__ constexpr size_t mlp_stream_lds_bytes(size_t row_bytes, size_t sp, bool grad)
{
    const size_t loop = kMsRows * row_bytes + ((size_t)kMsWaves * kMsRows * kMsPS + (size_t)kMsRows * kMsPS +
                                               (size_t)kMsRing * kMsRows + 4) * sizeof(float);
    const size_t tail = grad ? (64 * sp + (size_t)kMsWaves * kMsFold) * sizeof(float) : 0;
    return loop > tail ? loop : tail;
}

// ---- the row-streaming kernel.  Front: elem (type of X), EU (elements per 16 bytes), IP (image pitch, elements: an odd
//      number of 16-byte units), FU (16-byte units of the widest row), NC (16-feature dW1 chunks), SP (staging pitch,
//      floats), NW1 / w1frag / load_w1, layer1<NS>, dw1<NS> ----
template <class Front, bool GRAD>
__device__ __forceinline__ void mlp_stream_body(const MlpStreamParams &p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    typedef typename Front::elem elem;
    const MlpLane ln = mlp_lane();
    const int tid = ln.tid, w = ln.w, c16 = ln.c16, g = ln.g;
    constexpr int T = kMsThreads;
    constexpr int EU = Front::EU, IP = Front::IP, NC = Front::NC;
    const int F = p.F;
    const int C = F >> (EU == 8 ? 3 : 2);           // 16-byte units per feature row
    constexpr int KP = (kMsRows * Front::FU + T - 1) / T;           // 16-byte units of a fill per thread

    elem *img = reinterpret_cast<elem *>(smem);                    // [32][IP]   feature rows of the fill
    float *part = reinterpret_cast<float *>(img + (size_t)kMsRows * IP);       // [4][32][20] layer-2 partials, later
    float *scr = part + (size_t)w * kMsRows * kMsPS;               //            this wave's transposition scratch
    float *dH2s = part + (size_t)kMsWaves * kMsRows * kMsPS;       // [32][20]
    float *gs = dH2s + (size_t)kMsRows * kMsPS;                    // [3][32]    d loss / d score of the tile's rows
    unsigned *vmask = reinterpret_cast<unsigned *>(gs + kMsRing * kMsRows);    // [3] bit r: row r of the tile is real

    const mlp_f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const mlp_i4 zero4i = {0, 0, 0, 0};

    typename Front::w1frag w1r[Front::NW1];
    Front::load_w1(w1r, p, ln);
    const MlpSmallFrags fr = mlp_small_frags(p, ln);

    mlp_f4 acc[GRAD ? NC : 1];       // dW1[j1 = 16w+4g+i][f = 16c + c16]
#pragma unroll
    for (int c = 0; c < (GRAD ? NC : 1); ++c) acc[c] = zero4;
    MlpSmallSums sums = mlp_small_sums_zero();

    // 16-byte unit k of this thread is unit u = tid + 256 k of the tile: 16 bytes at byte 16 u of the tile's rows in
    // memory (flat rows are consecutive), row ur[k] = u / C of the tile (>= 32: past the tile), image element
    // EU u + ur[k] * (IP - EU C)
    int ur[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) ur[k] = (tid + k * T) / C;

    mlp_i4 P[KP];                                   // the fill in flight
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
    // forward over subtiles u0 .. u0 + NS - 1 of the image: layer-1 tile -> h1 (kept), layer-2 partial -> LDS
    auto fwd_tile = [&](auto ns_c, int u0, mlp_f4 (&h1)[2]) {
        constexpr int NS = decltype(ns_c)::value;
#pragma unroll
        for (int u = 0; u < NS; ++u) h1[u] = fr.b1v;
        Front::template layer1<NS>(h1, w1r, img, u0, ln);
#pragma unroll
        for (int u = 0; u < NS; ++u) mlp_layer2_partial(fr, h1[u], scr + (16 * (u0 + u) + c16) * kMsPS + 4 * g);
        if (NS == 1) h1[1] = zero4;
    };
    // tile wave, backward over the same subtiles: dW2, dH1 (-> scratch) and dW1 contributions
    auto bwd_tile = [&](auto ns_c, int u0, const mlp_f4 (&h1)[2]) {
        constexpr int NS = decltype(ns_c)::value;
        mlp_dw2_tile<NS>(sums, h1, scr, dH2s, u0, ln);
        mlp_dh1_tile<NS>(fr, sums, h1, dH2s, u0, ln, [&](int u, const mlp_f4 &d1) {
            *reinterpret_cast<mlp_f4 *>(scr + (16 * u + c16) * kMsPS + 4 * g) = d1;
        });
        Front::template dw1<NS>(acc, img, scr, u0, ln);
    };

    // ---- prologue: masks of the first two tiles, the first fill ----
    const int G = (int)gridDim.x;
    int tile = (int)blockIdx.x;
    mlp_ring_write<GRAD>(p, tid, tile, 0, vmask, gs);
    mlp_ring_write<GRAD>(p, tid, tile + G, 1, vmask, gs);
    // the feature columns F .. IP - 1 of the image are never written by a fill: zero them once
    // (layer 1 multiplies them by zero weights, the dW1 columns they produce are not stored)
    for (int i = tid; i < kMsRows * (IP - EU * C); i += T) {
        const int r = i / (IP - EU * C), cc = i - r * (IP - EU * C);
        img[r * IP + EU * C + cc] = 0;
    }
    __syncthreads();
    issue_fill(tile, __builtin_amdgcn_readfirstlane(vmask[0]));

    int slot = 0;
    for (; tile < p.tiles; tile += G) {
        const int slot1 = mlp_ring_next(slot), slot2 = mlp_ring_next(slot1);
        // (both masks were written in front of a barrier every wave has passed: the prologue's, or barrier A of the
        // iteration before; the slot rewritten below was last read in front of barrier A of the iteration before)
        const unsigned m = __builtin_amdgcn_readfirstlane(vmask[slot]);
        const unsigned mnext = __builtin_amdgcn_readfirstlane(vmask[slot1]);
        fill_image(m);                             // (waits for the fill in P; every wave is past the image's readers)
        issue_fill(tile + G, mnext);               // (past the last tile: mask 0, nothing of X is requested)
        mlp_ring_write<GRAD>(p, tid, tile + 2 * G, slot2, vmask, gs);
        lds_barrier();                             // A: image filled
        const bool act0 = (m & 0xFFFFu) != 0, act1 = (m >> 16) != 0;        // subtiles with a real row (uniform)
        const int doc = 16 * w + c16;              // owner waves 0, 1: the row of the tile this lane finishes
        const long long orow = (long long)tile * kMsRows + doc;
        // a tile of padding only (m == 0) costs its barrier A and, in the score kernel, the store of its zeros: ONE score
        // store for both cases (a second one on the padding path gets merged into this one behind exec-mask moves at the
        // end of every tile, 3-4 % of the score kernels; DESIGN.md 18)
        mlp_f4 h1[2], h2 = zero4;
        float s = 0.f;
        bool own = false;
        const int u0 = act0 ? 0 : 1;
        if (m != 0) {
            if (act0 && act1) fwd_tile(m2_ns<2>{}, 0, h1);
            else fwd_tile(m2_ns<1>{}, u0, h1);
            lds_barrier();                         // B: layer-2 partials
            own = w < 2 && (w == 0 ? act0 : act1);
            if (own) s = mlp_owner_fwd(fr, part, doc, g, h2);
        }
        if constexpr (!GRAD) {                     // (the partials are rewritten behind the next barrier A)
            if (w < 2 && g == 0 && orow < (long long)p.rows) p.scores_out[orow] = ((m >> doc) & 1u) ? s : 0.f;
        } else if (m != 0) {
            if (own) mlp_owner_bwd(fr, sums, h2, gs[slot * kMsRows + doc], dH2s, doc, g);
            lds_barrier();                         // C: dH2 rows
            if (act0 && act1) bwd_tile(m2_ns<2>{}, 0, h1);
            else bwd_tile(m2_ns<1>{}, u0, h1);
            lds_barrier();                         // D: image, scratch and dH2 rows free
        }
        slot = slot1;
    }
    if constexpr (GRAD) {
        // ---- this workgroup's partial vector [dW1 | db1 | dW2 | db2 | dW3 | db3] (ltr_mlp2.inc) ----
        float *dst = p.part + (size_t)blockIdx.x * p.pitch;
        float *lds = reinterpret_cast<float *>(smem);
        __syncthreads();                           // (the ring words of the last iterations are behind every wave)
        mlp_store_dw1<NC, Front::SP>(acc, lds, dst, p, 0, F >> 2, ln);
        // (the fold: behind the dW1 tiles of the store above, 64 staging rows from the start of the segment)
        mlp_store_small_sums(sums, dst, p.H1 * F, lds + (size_t)64 * Front::SP, p, ln);
    }
}

// ---- host side ----
// align: features per 16 bytes of a row of X; maxF: the widest row of the family
inline bool mlp_stream_bad_shape(int B, int L, int F, int H1, int H2, int align, int maxF)
{
    if (B < 0 || L <= 0 || F <= 0 || H1 <= 0 || H2 <= 0) return true;
    if ((F & (align - 1)) || F > maxF || H1 > kMlpH1 || H2 > kMlpH2) return true;
    return (long long)B * L > 0x7fffffffLL;
}

// the params of a launch; scores_out / part / pitch / dH1 are the caller's to set
inline MlpStreamParams mlp_stream_params(const void *X, const float *W1, const float *b1, const float *W2,
                                         const float *b2, const float *W3, const float *b3, const float *g,
                                         const int64_t *n, int B, int L, int F, int H1, int H2)
{
    MlpStreamParams p;
    p.X = X; p.W1 = W1; p.b1 = b1; p.W2 = W2; p.b2 = b2; p.W3 = W3; p.b3 = b3; p.g = g;
    p.n = n; p.scores_out = nullptr; p.part = nullptr; p.dH1 = nullptr;
    p.B = B; p.L = L; p.F = F; p.H1 = H1; p.H2 = H2;
    p.rows = B * L; p.tiles = (int)(((long long)p.rows + kMsRows - 1) / kMsRows); p.pitch = 0;
    return p;
}

// persistent grid: one workgroup per tile up to wgs_per_cu workgroups on every CU
inline int mlp_stream_grid(long long rows, int wgs_per_cu)
{
    const long long tiles = (rows + kMsRows - 1) / kMsRows;
    const long long wgs = (long long)wgs_per_cu * device_cu_count();
    return (int)(tiles < wgs ? tiles : wgs);
}

// The entry points of a row-streaming family.  Host: kAlign, kMaxF, grid(rows, F, grad), launch<GRAD>(p, grid, stream)
template <class Host>
int mlp_stream_scores(const void *X, const float *W1, const float *b1, const float *W2, const float *b2,
                      const float *W3, const float *b3, const int64_t *n, int B, int L, int F, int H1, int H2,
                      float *scores_out, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (mlp_stream_bad_shape(B, L, F, H1, H2, Host::kAlign, Host::kMaxF)) return LTR_ERR_SHAPE;
    if (!W1 || !b1 || !W2 || !b2 || !W3 || !b3) return LTR_ERR_NULL;
    if (B == 0) return LTR_OK;
    if (!X || !scores_out) return LTR_ERR_NULL;
    MlpStreamParams p = mlp_stream_params(X, W1, b1, W2, b2, W3, b3, nullptr, n, B, L, F, H1, H2);
    p.scores_out = scores_out;
    return Host::template launch<false>(p, Host::grid(p.rows, F, false), (hipStream_t)stream);
}

template <class Host>
size_t mlp_stream_grad_workspace_bytes(int B, int L, int F, int H1, int H2)
{
    if (B <= 0 || mlp_stream_bad_shape(B, L, F, H1, H2, Host::kAlign, Host::kMaxF)) return 0;
    return (size_t)Host::grid((long long)B * L, F, true) * (size_t)mlp_pitch(mlp_param_count(F, H1, H2)) * sizeof(float);
}

template <class Host>
int mlp_stream_grad(const void *X, const float *W1, const float *b1, const float *W2, const float *b2, const float *W3,
                    const float *b3, const float *g, const int64_t *n, int B, int L, int F, int H1, int H2,
                    float *grads, void *workspace, size_t workspace_bytes, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (mlp_stream_bad_shape(B, L, F, H1, H2, Host::kAlign, Host::kMaxF)) return LTR_ERR_SHAPE;
    if (!W1 || !b1 || !W2 || !b2 || !W3 || !b3 || !grads) return LTR_ERR_NULL;
    const int P = mlp_param_count(F, H1, H2);
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) return mlp_reduce_launch(nullptr, 0, P, grads, nullptr, 0, nullptr, s);      // zero gradients
    if (!X || !g) return LTR_ERR_NULL;
    const int grid = Host::grid((long long)B * L, F, true);
    if (!workspace || workspace_bytes < (size_t)grid * mlp_pitch(P) * sizeof(float)) return LTR_ERR_WORKSPACE;
    MlpStreamParams p = mlp_stream_params(X, W1, b1, W2, b2, W3, b3, g, n, B, L, F, H1, H2);
    p.part = (float *)workspace; p.pitch = mlp_pitch(P);
    const int rc = Host::template launch<true>(p, grid, s);
    if (rc != 0) return rc;
    return mlp_reduce_launch(workspace, grid, P, grads, nullptr, 0, nullptr, s);
}
