// ltr_scorer.inc -- the Linear(F, 1) candidate scorer on its own: scores = X.W + b and its weight
// gradient, as two HBM-streaming kernels, on rows of f32 (include/ltr_hip.h) or of bf16 (include/ltr_linear_bf16.h).
// Included by ltr_mlp.hip behind ltr_mlp_reduce.inc, whose reduction kernel adds the gradient's partial vectors.
// One scores body and one gradient body; a FRONT (LinFrontF32<4>: rows of float4, LinFrontF32<1>: rows of float for
// F % 4 != 0, LinFrontBf16: rows of eight bf16) supplies what depends on the element type, and the six entry points
// at the end differ in their shape predicate and in the kernel they name.  The bf16 fused step is ltr_linear_bf16.inc.
//
// The reference's users score with torch.nn.Linear(F, 1) (examples/01-basic-usage.py:45,
// tests/test_integration.py:30); on ROCm that is a rocBLAS GEMM with one output column, which runs
// the C2 batch (131 072 x 136) at ~280 GB/s.  The fused scorer+loss kernels (ltr_linear.inc) avoid
// it altogether; these two are for the UNFUSED drop-in composition `loss_fn(model(xs), ys, n)` --
// `model = pytorchltr_amd.fused.LinearScorer(F)` -- and for composing long-list steps out of
// balanced pieces.  Both skip padded documents when `n` is given (score 0, no gradient).
//
//   scores: a workgroup takes kScRows consecutive rows of one query: one wave per row, kScUnr rows in flight, W in
//           registers as fp32.
//   grad:   dW = sum_r g[r] X[r,:], db = sum_r g[r]: a workgroup takes kSgRows consecutive rows of one query,
//           thread (column vector, row group) accumulates in fp32, row groups fold in LDS, one partial
//           vector [dW | db] per workgroup; mlp_reduce_kernel adds the partials in a fixed order.
// Numerics on bf16 rows: widening is exact, W and every product and sum are fp32 (ltr_common.inc, LbW8).
#pragma once

#include "ltr_linear_bf16.h"

constexpr int kScUnr = 4;                  // rows in flight per wave, scores kernel (swept 2..16 with branch-free loads: 4)
constexpr int kSgUnr = 4;                  // rows in flight per thread, gradient kernel
constexpr int kScThreads = 256;
constexpr int kScRows = 128;  // documents per job (query, chunk), scores kernel
constexpr int kSgRows = 256;  // same, gradient kernel (swept: 256)
constexpr int kScMaxVec = 16;         // column vectors per lane: F <= 64 * 16 * VEC

struct ScorerParams {
    const void *X;                     // float or bf16 rows (the front knows)
    const float *W, *bias, *g;
    const int64_t *n;
    float *out;                        // scores (scores kernel) or partials (grad kernel)
    int B, L, F;
    int chunks;                        // row chunks per query (jobs = B * chunks)
};

// ---- the fronts: what depends on the element type of X ----
// X: what a lane loads of a row, one COLUMN VECTOR of kCols features (a row is C = F / kCols of them, back to back);
// A: the fp32 weights of a column vector, or its dW accumulator; P, kPieces: A as the pieces the fold of the gradient
// kernel adds and stores one per thread.  dot and fma are the type's own arithmetic, in the type's own order.
template <int VEC>
struct LinFrontF32 {
    using X = typename VecT<VEC>::type;
    using A = X;
    using P = X;
    static constexpr int kCols = VEC, kPieces = 1;
    static __device__ __forceinline__ A load_w(const float *W, int c, int C)
    {
        return c < C ? reinterpret_cast<const A *>(W)[c] : vzero<A>();
    }
    // `in`: the column vector is one of the row's C (the others were loaded from the clamped address): zeroed here as
    // well as in w.  In this form -- the select on the operand, by reference -- the compiler forms the four products
    // packed and unfused and adds them in order; given the zero weights alone, or the select in a function of its own, it
    // contracts the same expression into an fma chain and the last bits of every score change.
    static __device__ __forceinline__ float dot(const X &x, bool in, const A &w) { return vdot(in ? x : vzero<X>(), w); }
    static __device__ __forceinline__ void fma(A &acc, float g, X x) { vfma(acc, g, x); }
    static __device__ __forceinline__ A zero() { return vzero<A>(); }
    static __device__ __forceinline__ P piece(const A &acc, int) { return acc; }
};

struct LinFrontBf16 {
    using X = ltr_u32x4;                   // eight bf16
    using A = LbW8;
    using P = float4;
    static constexpr int kCols = 8, kPieces = 2;
    static __device__ __forceinline__ A load_w(const float *W, int c, int C)
    {
        if (c >= C) return lb_zero();
        A w;
        w.a = reinterpret_cast<const float4 *>(W)[2 * c];
        w.b = reinterpret_cast<const float4 *>(W)[2 * c + 1];
        return w;
    }
    // (no select: the zero weights do it, the two fmaf chains of lb_dot are fixed, and at 17 of 64 lanes busy this
    // kernel is short of VALU issue slots, not of bytes)
    static __device__ __forceinline__ float dot(X x, bool, const A &w) { return lb_dot(x, w); }
    static __device__ __forceinline__ void fma(A &acc, float g, X x) { lb_fma(acc, g, x); }
    static __device__ __forceinline__ A zero() { return lb_zero(); }
    static __device__ __forceinline__ P piece(const A &acc, int h) { return h ? acc.b : acc.a; }
};

// A job is (query b, chunk of kScRows documents): no per-row division, and the documents past
// n[b] are never touched (their scores are written as 0).  NV >= ceil(C / 64) column vectors per lane.
template <class Fr, int NV>
__device__ __forceinline__ void linear_scores_body(const ScorerParams &p)
{
    using XV = typename Fr::X;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    constexpr int NW = kScThreads / 64;
    const int C = p.F / Fr::kCols;
    const int b = blockIdx.x / p.chunks;
    const int l0 = (blockIdx.x - b * p.chunks) * kScRows;
    const int l1 = min(p.L, l0 + kScRows);
    const int nb = p.n ? clamp_n(p.n[b], p.L) : p.L;
    const int lv = min(l1, nb);                                 // documents [l0, lv) are real
    const size_t row0 = (size_t)b * p.L;
    for (int l = max(l0, lv) + threadIdx.x; l < l1; l += kScThreads) p.out[row0 + l] = 0.f;
    if (l0 >= lv) return;
    typename Fr::A w[NV];                                      // zero past C
#pragma unroll
    for (int i = 0; i < NV; ++i) w[i] = Fr::load_w(p.W, lane + 64 * i, C);
    const float bias = p.bias ? p.bias[0] : 0.f;
    const XV *Xq = reinterpret_cast<const XV *>(p.X) + row0 * (size_t)C;
    constexpr int UNR = kScUnr;
    for (int la = l0 + wave; la < lv; la += NW * UNR) {
        float acc[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) acc[u] = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {                          // unrolled: w[] stays in registers
            // unconditional loads from clamped addresses (a per-lane condition around a load becomes a branch and a
            // full wait, and serialises the rows in flight): rows past lv re-read row lv - 1 and their result is
            // dropped, columns past C re-read column C - 1 against zero weights
            const int c = lane + 64 * i;
            const int cc = min(c, C - 1);
            XV x[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int l = min(la + u * NW, lv - 1);
                x[u] = Xq[(size_t)l * C + cc];
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) acc[u] += Fr::dot(x[u], c < C, w[i]);
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int l = la + u * NW;
            const float s = wave_sum(acc[u]);
            if (lane == 0 && l < lv) p.out[row0 + l] = s + bias;
        }
    }
}

// One partial vector [dW | db] per job (query, chunk of kSgRows documents): thread (column vector, row group)
// accumulates its rows, the row groups fold in LDS: [piece][row group][column vector], one piece per thread of the fold.
// More than kScThreads column vectors (scalar rows only) go tile by tile.
template <class Fr>
__device__ __forceinline__ void linear_grad_body(const ScorerParams &p)
{
    using XV = typename Fr::X;
    using PV = typename Fr::P;
    constexpr int T = kScThreads;
    constexpr int NP = Fr::kPieces;
    __shared__ PV dred[NP * T];
    __shared__ float gred[T / 64];
    const int tid = threadIdx.x;
    const int C = p.F / Fr::kCols;
    const int b = blockIdx.x / p.chunks;
    const int l0 = (blockIdx.x - b * p.chunks) * kSgRows;
    const int nb = p.n ? clamp_n(p.n[b], p.L) : p.L;
    const int lv = min(min(p.L, l0 + kSgRows), nb);             // documents [l0, lv) are real
    const size_t row0 = (size_t)b * p.L;
    float *part = p.out + (size_t)blockIdx.x * partial_pitch(p.F);   // partial rows start 16-byte aligned
    if (l0 >= lv) {                                            // nothing real here: a zero partial
        for (int i = tid; i <= p.F; i += T) part[i] = 0.f;
        return;
    }
    const XV *Xq = reinterpret_cast<const XV *>(p.X) + row0 * (size_t)C;
    const float *gq = p.g + row0;
    const int CT = C < T ? C : T;                              // column vectors per tile
    const int RG = T / CT;                                     // row groups
    const int rg = tid / CT, cl = tid - rg * CT;
    float gb = 0.f;
    for (int l = l0 + tid; l < lv; l += T) gb += gq[l];
    gb = wave_sum(gb);
    if ((tid & 63) == 0) gred[tid >> 6] = gb;
    for (int c0 = 0; c0 < C; c0 += CT) {
        const int c = c0 + cl;
        const bool mine = rg < RG && c < C;
        typename Fr::A acc = Fr::zero();
        if (mine) {
            constexpr int UNR = kSgUnr;
            for (int la = l0 + rg; la < lv; la += RG * UNR) {
                XV x[UNR];
                float g[UNR];
#pragma unroll
                for (int u = 0; u < UNR; ++u) {                // rows past lv: row lv - 1 again, with g = 0
                    const int l = la + u * RG;
                    const int lc = min(l, lv - 1);
                    const float gv = gq[lc];
                    g[u] = (l < lv) ? gv : 0.f;
                    x[u] = Xq[(size_t)lc * C + c];
                }
#pragma unroll
                for (int u = 0; u < UNR; ++u) Fr::fma(acc, g[u], x[u]);
            }
        }
        __syncthreads();                                       // previous tile's readers are done
        if (mine) {
#pragma unroll
            for (int h = 0; h < NP; ++h) dred[h * T + rg * CT + cl] = Fr::piece(acc, h);
        }
        __syncthreads();
        if (tid < NP * CT && c0 * NP + tid < NP * C) {         // piece tid % NP of column vector c0 + tid / NP
            const PV *src = dred + (tid % NP) * T + tid / NP;
            PV s = vzero<PV>();
            for (int q = 0; q < RG; ++q) vadd(s, src[q * CT]);
            reinterpret_cast<PV *>(part)[c0 * NP + tid] = s;
        }
    }
    if (tid == 0) {
        float s = 0.f;
        for (int q = 0; q < T / 64; ++q) s += gred[q];
        part[p.F] = s;
    }
}

// The kernels, under the names profiles and tests know.  Occupancy they are sized for (waves per SIMD): the bf16 ones
// eight (<= 64 VGPRs) with one column vector per lane (F <= 512) and in the gradient kernel, six (<= 80) with two;
// tests/test_linear_bf16_host.py and tests/test_codeobj.py hold the compiler to them.
template <int VEC, int NV>
__global__ void __launch_bounds__(kScThreads)
linear_scores_kernel(ScorerParams p) { linear_scores_body<LinFrontF32<VEC>, NV>(p); }

template <int VEC>
__global__ void __launch_bounds__(kScThreads)
linear_grad_kernel(ScorerParams p) { linear_grad_body<LinFrontF32<VEC>>(p); }

template <int NV>
__global__ void __launch_bounds__(kScThreads)
linear_bf16_scores_kernel(ScorerParams p) { linear_scores_body<LinFrontBf16, NV>(p); }

__global__ void __launch_bounds__(kScThreads)
linear_bf16_grad_kernel(ScorerParams p) { linear_grad_body<LinFrontBf16>(p); }

// ---- host side: the checks in one order; an entry point brings its type's shape predicate and its kernel ----
typedef void (*ScorerKernel)(ScorerParams);

inline bool linear_f32_shape_bad(int B, int L, int F) { return B < 0 || L <= 0 || F <= 0; }

inline int linear_scores_launch(bool shape_bad, ScorerKernel kernel, const void *X, const float *W, const float *bias,
                                const int64_t *n, int B, int L, int F, float *scores, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (shape_bad) return LTR_ERR_SHAPE;
    if (B == 0) return LTR_OK;
    if (!X || !W || !scores) return LTR_ERR_NULL;
    const int chunks = (L + kScRows - 1) / kScRows;
    const ScorerParams p = {X, W, bias, nullptr, n, scores, B, L, F, chunks};
    hipLaunchKernelGGL(kernel, dim3((unsigned)((long long)B * chunks)), dim3(kScThreads), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

// one partial vector [dW | db | pad] per (query, chunk of kSgRows documents)
inline size_t linear_grad_workspace(bool shape_bad, int B, int L, int F)
{
    if (shape_bad || B <= 0) return 0;
    const long long blocks = (long long)B * ((L + kSgRows - 1) / kSgRows);
    return (size_t)blocks * (size_t)partial_pitch(F) * sizeof(float);
}

inline int linear_grad_launch(bool shape_bad, ScorerKernel kernel, const void *X, const float *g, const int64_t *n, int B,
                              int L, int F, float *dW_db, void *workspace, size_t workspace_bytes, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (shape_bad) return LTR_ERR_SHAPE;
    if (!dW_db) return LTR_ERR_NULL;
    if (B > 0 && (!X || !g)) return LTR_ERR_NULL;
    if (B > 0 && (!workspace || workspace_bytes < linear_grad_workspace(false, B, L, F))) return LTR_ERR_WORKSPACE;
    const int chunks = (L + kSgRows - 1) / kSgRows;
    const int blocks = B * chunks;
    hipStream_t st = (hipStream_t)stream;
    if (B > 0) {
        const ScorerParams p = {X, nullptr, nullptr, g, n, (float *)workspace, B, L, F, chunks};
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kScThreads), 0, st, p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(mlp_reduce_kernel, dim3((unsigned)((F + 1 + kMlpRedCols - 1) / kMlpRedCols)),
                       dim3(kMlpRedCols * kMlpRedSlices), 0, st,
                       (const float *)workspace, blocks, F + 1, partial_pitch(F), dW_db, (const float *)nullptr, 0,
                       (float *)nullptr);
    return (int)hipGetLastError();
}

extern "C" {

int ltr_linear_scores_f32(const float *X, const float *W, const float *bias, const int64_t *n, int B,
                          int L, int F, float *scores, void *stream)
{
    // rows of float4 where F allows; NV of 1, 4 or 16 column vectors per lane (the vector path never needs more than 4)
    const int nv = (F / (F % 4 == 0 ? 4 : 1) + 63) / 64;
    const ScorerKernel kernel = F % 4 == 0 ? (nv <= 1 ? linear_scores_kernel<4, 1> : linear_scores_kernel<4, 4>)
                                : nv <= 1  ? linear_scores_kernel<1, 1>
                                : nv <= 4  ? linear_scores_kernel<1, 4>
                                           : linear_scores_kernel<1, kScMaxVec>;
    return linear_scores_launch(linear_f32_shape_bad(B, L, F) || F > 64 * kScMaxVec, kernel, X, W, bias, n, B, L, F,
                                scores, stream);
}

size_t ltr_linear_grad_workspace_bytes(int B, int L, int F)
{
    return linear_grad_workspace(linear_f32_shape_bad(B, L, F), B, L, F);
}

int ltr_linear_grad_f32(const float *X, const float *g, const int64_t *n, int B, int L, int F,
                        float *dW_db, void *workspace, size_t workspace_bytes, void *stream)
{
    return linear_grad_launch(linear_f32_shape_bad(B, L, F), F % 4 == 0 ? linear_grad_kernel<4> : linear_grad_kernel<1>,
                              X, g, n, B, L, F, dW_db, workspace, workspace_bytes, stream);
}

int ltr_linear_scores_bf16(const uint16_t *X, const float *W, const float *bias, const int64_t *n, int B, int L,
                           int F, float *scores, void *stream)
{
    return linear_scores_launch(lb_shape_bad(B, L, F), F / 8 <= 64 ? linear_bf16_scores_kernel<1> : linear_bf16_scores_kernel<2>,
                                X, W, bias, n, B, L, F, scores, stream);
}

size_t ltr_linear_grad_workspace_bytes_bf16(int B, int L, int F)
{
    return linear_grad_workspace(lb_shape_bad(B, L, F), B, L, F);
}

int ltr_linear_grad_bf16(const uint16_t *X, const float *g, const int64_t *n, int B, int L, int F, float *dW_db,
                         void *workspace, size_t workspace_bytes, void *stream)
{
    return linear_grad_launch(lb_shape_bad(B, L, F), linear_bf16_grad_kernel, X, g, n, B, L, F, dW_db, workspace,
                              workspace_bytes, stream);
}

}  // extern "C"
