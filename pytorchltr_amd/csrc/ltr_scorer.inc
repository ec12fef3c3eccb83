// ltr_scorer.inc -- the Linear(F, 1) candidate scorer on its own: scores = X.W + b and its weight
// gradient, as two HBM-streaming kernels.  Included by ltr_kernels.hip.
//
// The reference's users score with torch.nn.Linear(F, 1) (examples/01-basic-usage.py:45,
// tests/test_integration.py:30); on ROCm that is a rocBLAS GEMM with one output column, which runs
// the C2 batch (131 072 x 136) at ~280 GB/s.  The fused scorer+loss kernels (ltr_linear.inc) avoid
// it altogether; these two are for the UNFUSED drop-in composition `loss_fn(model(xs), ys, n)` --
// `model = pytorchltr_amd.fused.LinearScorer(F)` -- and for composing long-list steps out of
// balanced pieces.  Both skip padded documents when `n` is given (score 0, no gradient).
//
//   scores: one wave per row, kScUnr rows in flight, W in registers; grid-stride over rows.
//   grad:   dW = sum_r g[r] X[r,:], db = sum_r g[r]: a workgroup takes kScRows consecutive rows,
//           thread (column vector, row group) accumulates, row groups fold in LDS, one partial
//           vector [dW | db] per workgroup; mlp_reduce_kernel adds the partials in a fixed order.
#pragma once

constexpr int kScUnr = 4;                  // rows in flight per wave, scores kernel (swept 2..16 with branch-free loads: 4)
constexpr int kSgUnr = 4;                  // rows in flight per thread, gradient kernel
constexpr int kScThreads = 256;
constexpr int kScRows = 128;  // documents per job (query, chunk), scores kernel
constexpr int kSgRows = 256;  // same, gradient kernel (swept: 256)
constexpr int kScMaxVec = 16;         // column vectors per lane: F <= 64 * 16 * VEC

struct ScorerParams {
    const float *X, *W, *bias, *g;
    const int64_t *n;
    float *out;                        // scores (scores kernel) or partials (grad kernel)
    int B, L, F;
    int chunks;                        // row chunks per query (jobs = B * chunks)
};

// A job is (query b, chunk of kScRows documents): no per-row division, and the documents past
// n[b] are never touched (their scores are written as 0).
template <int VEC, int NV>
__global__ void __launch_bounds__(kScThreads)
linear_scores_kernel(ScorerParams p)
{
    using V = typename VecT<VEC>::type;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    constexpr int NW = kScThreads / 64;
    const int C = p.F / VEC;
    const int b = blockIdx.x / p.chunks;
    const int l0 = (blockIdx.x - b * p.chunks) * kScRows;
    const int l1 = min(p.L, l0 + kScRows);
    const int nb = p.n ? clamp_n(p.n[b], p.L) : p.L;
    const int lv = min(l1, nb);                                 // documents [l0, lv) are real
    const size_t row0 = (size_t)b * p.L;
    for (int l = max(l0, lv) + threadIdx.x; l < l1; l += kScThreads) p.out[row0 + l] = 0.f;
    if (l0 >= lv) return;
    V w[NV];                                                   // NV >= ceil(C / 64) vectors per lane
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        w[i] = (c < C) ? reinterpret_cast<const V *>(p.W)[c] : vzero<V>();
    }
    const float bias = p.bias ? p.bias[0] : 0.f;
    const float *Xq = p.X + row0 * (size_t)p.F;
    constexpr int UNR = kScUnr;
    for (int la = l0 + wave; la < lv; la += NW * UNR) {
        float acc[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) acc[u] = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {                          // unrolled: w[] stays in registers
            {
                const int c = lane + 64 * i;
                // unconditional loads from clamped addresses (a per-lane condition around a load
                // becomes a branch + s_waitcnt vmcnt(0) and serialises the rows in flight): rows
                // past lv re-read row lv-1 and their result is dropped, columns past C are zeroed
                const int cc = min(c, C - 1);
                V x[UNR];
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    const int l = min(la + u * NW, lv - 1);
                    x[u] = reinterpret_cast<const V *>(Xq + (size_t)l * p.F)[cc];
                }
#pragma unroll
                for (int u = 0; u < UNR; ++u) acc[u] += vdot(c < C ? x[u] : vzero<V>(), w[i]);
            }
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int l = la + u * NW;
            const float s = wave_sum(acc[u]);
            if (lane == 0 && l < lv) p.out[row0 + l] = s + bias;
        }
    }
}

// One partial vector [dW | db] per job (query, chunk): thread (column vector, row group)
// accumulates its rows, row groups fold in LDS.  LDS: RG x CT vectors.
template <int VEC>
__global__ void __launch_bounds__(kScThreads)
linear_grad_kernel(ScorerParams p)
{
    using V = typename VecT<VEC>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    V *dred = reinterpret_cast<V *>(smem);
    __shared__ float gred[kScThreads / 64];
    const int tid = threadIdx.x;
    constexpr int T = kScThreads;
    const int C = p.F / VEC;
    const int b = blockIdx.x / p.chunks;
    const int l0 = (blockIdx.x - b * p.chunks) * kSgRows;
    const int nb = p.n ? clamp_n(p.n[b], p.L) : p.L;
    const int lv = min(min(p.L, l0 + kSgRows), nb);             // documents [l0, lv) are real
    const size_t row0 = (size_t)b * p.L;
    const int pitch = (p.F + 1 + 3) & ~3;                      // partial rows start 16-byte aligned
    float *part = p.out + (size_t)blockIdx.x * pitch;
    if (l0 >= lv) {                                            // nothing real here: a zero partial
        for (int i = tid; i <= p.F; i += T) part[i] = 0.f;
        return;
    }
    const float *Xq = p.X + row0 * (size_t)p.F;
    const float *gq = p.g + row0;
    const int CT = C < T ? C : T;                              // column vectors per tile
    const int RG = T / CT;                                     // row groups
    const int cl = tid % CT, rg = tid / CT;
    float gb = 0.f;
    for (int l = l0 + tid; l < lv; l += T) gb += gq[l];
    gb = wave_sum(gb);
    if ((tid & 63) == 0) gred[tid >> 6] = gb;
    for (int c0 = 0; c0 < C; c0 += CT) {
        const int c = c0 + cl;
        V acc = vzero<V>();
        if (rg < RG && c < C) {
            constexpr int UNR = kSgUnr;
            for (int la = l0 + rg; la < lv; la += RG * UNR) {
                V x[UNR];
                float g[UNR];
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    const int l = la + u * RG;
                    const bool live = l < lv;
                    g[u] = live ? gq[l] : 0.f;
                    x[u] = live ? reinterpret_cast<const V *>(Xq + (size_t)l * p.F)[c] : vzero<V>();
                }
#pragma unroll
                for (int u = 0; u < UNR; ++u) vfma(acc, g[u], x[u]);
            }
        }
        __syncthreads();                                       // previous tile's readers are done
        if (rg < RG && c < C) dred[(size_t)rg * CT + cl] = acc;
        __syncthreads();
        if (tid < CT && c0 + tid < C) {
            V s = vzero<V>();
            for (int q = 0; q < RG; ++q) vadd(s, dred[(size_t)q * CT + tid]);
            reinterpret_cast<V *>(part)[c0 + tid] = s;
        }
    }
    if (tid == 0) {
        float s = 0.f;
        for (int q = 0; q < T / 64; ++q) s += gred[q];
        part[p.F] = s;
    }
}

// The fixed-order sum of a workspace of partial vectors for the translation units that do not have mlp_reduce_kernel
// (ltr_linear_bf16.inc): out[i] = sum over the nPart vectors, `pitch` floats apart, i < P.  Not part of the C ABI.
extern "C" __attribute__((visibility("hidden"))) int ltr_internal_reduce_partials(const float *part, int nPart, int P, int pitch,
                                                                                  float *out, void *stream)
{
    hipLaunchKernelGGL(mlp_reduce_kernel, dim3((unsigned)((P + kMlpRedCols - 1) / kMlpRedCols)),
                       dim3(kMlpRedCols * kMlpRedSlices), 0, (hipStream_t)stream, part, nPart, P, pitch, out,
                       (const float *)nullptr, 0, (float *)nullptr);
    return (int)hipGetLastError();
}

extern "C" {

int ltr_linear_scores_f32(const float *X, const float *W, const float *bias, const int64_t *n, int B,
                          int L, int F, float *scores, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (B < 0 || L <= 0 || F <= 0) return LTR_ERR_SHAPE;
    if (F > 64 * kScMaxVec) return LTR_ERR_SHAPE;              // scalar path holds F / 64 values per lane
    if (B == 0) return LTR_OK;
    if (!X || !W || !scores) return LTR_ERR_NULL;
    ScorerParams p;
    p.X = X; p.W = W; p.bias = bias; p.g = nullptr; p.n = n; p.out = scores;
    p.B = B; p.L = L; p.F = F; p.chunks = (L + kScRows - 1) / kScRows;
    const long long blocks = (long long)B * p.chunks;
    const int vec = (F % 4 == 0) ? 4 : 1;
    const int nv = (F / vec + 63) / 64;
    const dim3 grid((unsigned)blocks), block(kScThreads);
    hipStream_t st = (hipStream_t)stream;
#define LTR_SC_LAUNCH(V, N) hipLaunchKernelGGL((linear_scores_kernel<V, N>), grid, block, 0, st, p)
    if (vec == 4) {
        if (nv <= 1) LTR_SC_LAUNCH(4, 1);
        else if (nv <= 4) LTR_SC_LAUNCH(4, 4);
        else LTR_SC_LAUNCH(4, kScMaxVec);
    } else {
        if (nv <= 1) LTR_SC_LAUNCH(1, 1);
        else if (nv <= 4) LTR_SC_LAUNCH(1, 4);
        else LTR_SC_LAUNCH(1, kScMaxVec);
    }
#undef LTR_SC_LAUNCH
    return (int)hipGetLastError();
}

size_t ltr_linear_grad_workspace_bytes(int B, int L, int F)
{
    if (B <= 0 || L <= 0 || F <= 0) return 0;
    const long long blocks = (long long)B * ((L + kSgRows - 1) / kSgRows);
    // partial rows are padded to a multiple of 4 floats so that the vector stores stay aligned
    return (size_t)blocks * (size_t)((F + 1 + 3) & ~3) * sizeof(float);
}

int ltr_linear_grad_f32(const float *X, const float *g, const int64_t *n, int B, int L, int F,
                        float *dW_db, void *workspace, size_t workspace_bytes, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (B < 0 || L <= 0 || F <= 0) return LTR_ERR_SHAPE;
    if (!dW_db) return LTR_ERR_NULL;
    if (B > 0 && (!X || !g)) return LTR_ERR_NULL;
    if (B > 0 && (!workspace || workspace_bytes < ltr_linear_grad_workspace_bytes(B, L, F)))
        return LTR_ERR_WORKSPACE;
    const int chunks = (L + kSgRows - 1) / kSgRows;
    const int blocks = B * chunks;
    const int pitch = (F + 1 + 3) & ~3;
    hipStream_t st = (hipStream_t)stream;
    if (B > 0) {
        ScorerParams p;
        p.X = X; p.W = nullptr; p.bias = nullptr; p.g = g; p.n = n; p.out = (float *)workspace;
        p.B = B; p.L = L; p.F = F; p.chunks = chunks;
        const int vec = (F % 4 == 0) ? 4 : 1;
        const int C = F / vec;
        const int CT = C < kScThreads ? C : kScThreads;
        const size_t lds = (size_t)(kScThreads / CT) * CT * vec * sizeof(float);
        if (vec == 4)
            hipLaunchKernelGGL((linear_grad_kernel<4>), dim3((unsigned)blocks), dim3(kScThreads), lds, st, p);
        else
            hipLaunchKernelGGL((linear_grad_kernel<1>), dim3((unsigned)blocks), dim3(kScThreads), lds, st, p);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(mlp_reduce_kernel, dim3((unsigned)((F + 1 + kMlpRedCols - 1) / kMlpRedCols)),
                       dim3(kMlpRedCols * kMlpRedSlices), 0, st,
                       (const float *)workspace, blocks, F + 1, pitch, dW_db, (const float *)nullptr, 0,
                       (float *)nullptr);
    return (int)hipGetLastError();
}

}  // extern "C"
