// ltr_mlp_reduce.inc -- the cross-workgroup sum behind every kernel of this translation unit that leaves one partial
// vector per workgroup: the fused MLP step (ltr_mlp.inc, ltr_mlp2.inc), the stand-alone MLP scorer's gradient
// (ltr_mlp_stream.inc, ltr_mlp_wide.inc) and the Linear scorer's (ltr_scorer.inc).
//     grads[i] = sum over the workgroups' partial vectors, fixed order;  loss_sum[0] = sum_b loss[b].
// The column sum is written once per load width (mlp_reduce_core: 4-byte loads; mlp_reduce4_core: 16-byte loads) as a
// __device__ template over an epilogue type, which owns what a kernel does with the sums:
//     fetch(i)      float4 core: the thread that will hold the final sums of the 4 columns from flat index i, ahead of
//                   the first LDS write and the two folds
//     between()     float4 core: every thread, between the two barriers of the fold (one idle thread may work there)
//     finish(i, g)  the owning thread, with the N final sums (N = 1: the 4-byte core, its one fold and one barrier)
// MlpReduceStore below stores them (mlp_reduce_kernel, mlp_reduce4_kernel); ltr_mlp_train.inc puts the optimizer update
// there.  The order of every addition is the cores', so every kernel built on them sums alike, bit for bit.
// Needs block_sum and vadd (ltr_common.inc).
#pragma once

// floats between the partial vectors of consecutive workgroups (16-byte aligned rows)
__host__ __device__ inline int mlp_pitch(int P) { return (P + 3) & ~3; }

__host__ __device__ inline bool mlp_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Block = 64 parameters x 16 slices of the partial rows (1024 threads): every thread adds its rows
// with four independent chains, the 16 slices meet in LDS.
constexpr int kMlpRedSlices = 32;
constexpr int kMlpRedCols = 32;      // 32 parameters x 32 row slices per block: P / 32 blocks (232 at the
                                     // guide's network) cover the chip; 64 x 16 left half of the CUs idle
                                     // (reduce kernel 6.5 -> measured below)
// The same sum with 16-byte loads: a block takes COLS4 float4 columns x 1024 / COLS4 row slices (every
// load instruction of a wave moves COLS4 * 16 contiguous bytes of 64 / COLS4 rows -- four times fewer, wider
// requests than the 4-byte version for the same 15 MB), the slices meet in LDS in two levels.  Fixed order.
constexpr int kMlpRedCols4 = 16;
constexpr int kMlpRedThreads = 1024;  // the block of all four reduction kernels
static_assert(kMlpRedCols * kMlpRedSlices == kMlpRedThreads, "one block size under both widths");

// the plain epilogue: the N sums go to grads[i ..], cut at P (the float4 of the last column may reach into the pitch)
template <int N>
struct MlpReduceStore {
    float *__restrict__ grads;
    int P;
    __device__ __forceinline__ void fetch(int) {}
    __device__ __forceinline__ void between() {}
    __device__ __forceinline__ void finish(int i, const float *g)
    {
        if constexpr (N == 1) {
            grads[i] = g[0];
        } else if (i + 3 < P) {
            *reinterpret_cast<float4 *>(grads + i) = make_float4(g[0], g[1], g[2], g[3]);
        } else {
            if (i < P) grads[i] = g[0];
            if (i + 1 < P) grads[i + 1] = g[1];
            if (i + 2 < P) grads[i + 2] = g[2];
        }
    }
};

// loss_sum[0] = sum_b loss[b], by ONE workgroup: the tail of every reduction kernel, behind its column sums, under
// `if (loss_sum && blockIdx.x == 0)`.  The guard stands in the kernels: with the workgroup index known to be 0
// inside this function, the compiler no longer folds block_sum's blockDim.x into one read of the dispatch's group size.
__device__ __forceinline__ void mlp_reduce_loss_sum(const float *__restrict__ loss, int B, float *__restrict__ loss_sum)
{
    __shared__ float lred[16];
    const int tid = threadIdx.x;
    float s = 0.f;
    for (int b = tid; b < B; b += kMlpRedThreads) s += loss[b];
    s = block_sum(s, lred);
    if (tid == 0) loss_sum[0] = s;
}

// `pitch` = floats between consecutive partial vectors (>= P)
template <class Epilogue>
__device__ __forceinline__ void mlp_reduce_core(const float *__restrict__ part, int nPart, int P, int pitch, Epilogue &epi)
{
    __shared__ float red[kMlpRedSlices][kMlpRedCols];
    const int tid = threadIdx.x;
    const int col = tid % kMlpRedCols, slice = tid / kMlpRedCols;
    const int i = blockIdx.x * kMlpRedCols + col;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (i < P) {
        // 16 rows per round, all 16 loads in flight before the first add (the kernel is bound by the
        // round trips of its strided 4-byte loads: 6.3 -> measured below with 4 loads in flight)
        const float *src = part + i;
        for (int r0 = slice; r0 < nPart; r0 += 16 * kMlpRedSlices) {
            float v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int r = r0 + k * kMlpRedSlices;
                v[k] = src[(size_t)(r < nPart ? r : r0) * pitch];
            }
#pragma unroll
            for (int k = 0; k < 16; k += 4) {
                a0 += (r0 + k * kMlpRedSlices < nPart) ? v[k] : 0.f;
                a1 += (r0 + (k + 1) * kMlpRedSlices < nPart) ? v[k + 1] : 0.f;
                a2 += (r0 + (k + 2) * kMlpRedSlices < nPart) ? v[k + 2] : 0.f;
                a3 += (r0 + (k + 3) * kMlpRedSlices < nPart) ? v[k + 3] : 0.f;
            }
        }
    }
    red[slice][col] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (slice == 0 && i < P) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < kMlpRedSlices; ++k) t += red[k][col];
        epi.finish(i, &t);
    }
}

template <int COLS4, class Epilogue>
__device__ __forceinline__ void mlp_reduce4_core(const float *__restrict__ part, int nPart, int pitch, Epilogue &epi)
{
    constexpr int SL = 1024 / COLS4;
    static_assert(SL % 16 == 0, "two-level fold: 16 groups of slices");
    __shared__ float4 red[SL][COLS4];
    __shared__ float4 red2[16][COLS4];
    const int tid = threadIdx.x;
    const int col = tid % COLS4, slice = tid / COLS4;
    const int c4 = blockIdx.x * COLS4 + col;
    const int P4 = pitch >> 2;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c4 < P4) {
        const float4 *src = reinterpret_cast<const float4 *>(part) + c4;
        for (int r0 = slice; r0 < nPart; r0 += 8 * SL) {
            float4 v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int r = r0 + k * SL;
                v[k] = src[(size_t)(r < nPart ? r : r0) * P4];
            }
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (r0 + k * SL < nPart) vadd(a, v[k]);
        }
    }
    // the owners of the block's columns fetch what their epilogue needs ahead of the two folds (and of the first LDS write)
    const bool owner = tid < COLS4 && c4 < P4;
    if (owner) epi.fetch(4 * c4);
    red[slice][col] = a;
    __syncthreads();
    epi.between();                                                 // (what it writes to LDS is published by the barrier below)
    if (tid < 16 * COLS4) {
        const int g = tid / COLS4;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < SL / 16; ++j) vadd(t, red[g + 16 * j][col]);
        red2[g][col] = t;
    }
    __syncthreads();
    if (owner) {
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int g = 0; g < 16; ++g) vadd(t, red2[g][col]);
        const float g4[4] = {t.x, t.y, t.z, t.w};
        epi.finish(4 * c4, g4);
    }
}

__global__ void __launch_bounds__(kMlpRedCols * kMlpRedSlices)
mlp_reduce_kernel(const float *__restrict__ part, int nPart, int P, int pitch, float *__restrict__ grads,
                  const float *__restrict__ loss, int B, float *__restrict__ loss_sum)
{
    MlpReduceStore<1> store{grads, P};
    mlp_reduce_core(part, nPart, P, pitch, store);
    if (loss_sum && blockIdx.x == 0) mlp_reduce_loss_sum(loss, B, loss_sum);
}

template <int COLS4>
__global__ void __launch_bounds__(1024)
mlp_reduce4_kernel(const float *__restrict__ part, int nPart, int P, int pitch, float *__restrict__ grads,
                   const float *__restrict__ loss, int B, float *__restrict__ loss_sum)
{
    MlpReduceStore<4> store{grads, P};
    mlp_reduce4_core<COLS4>(part, nPart, pitch, store);
    if (loss_sum && blockIdx.x == 0) mlp_reduce_loss_sum(loss, B, loss_sum);
}

// ---- host side ----
// The launch shape of a sum over P columns: blocks of kMlpRedThreads threads, kMlpRedCols4 float4 columns each for the
// float4 kernel -- taken wherever everything the launch moves as 16 bytes is aligned: the workspace, and the plain
// launch's grads -- else kMlpRedCols columns each for the 4-byte version.
inline dim3 mlp_reduce_blocks(int P, bool vec4)
{
    return dim3((unsigned)(vec4 ? ((mlp_pitch(P) >> 2) + kMlpRedCols4 - 1) / kMlpRedCols4 : (P + kMlpRedCols - 1) / kMlpRedCols));
}

// the cross-workgroup sum of the partial vectors (and loss_sum) behind a training step of any entry point
inline int mlp_reduce_launch(void *workspace, int grid, int P, float *grads, const float *loss, int B, float *loss_sum,
                             hipStream_t s)
{
    // (grads as float4 needs a 16-byte aligned output; otherwise the 4-byte version)
    const bool vec4 = mlp_aligned16(grads) && mlp_aligned16(workspace);
    const auto kernel = vec4 ? mlp_reduce4_kernel<kMlpRedCols4> : mlp_reduce_kernel;
    hipLaunchKernelGGL(kernel, mlp_reduce_blocks(P, vec4), dim3(kMlpRedThreads), 0, s, (const float *)workspace, grid, P,
                       mlp_pitch(P), grads, loss, B, loss_sum);
    return (int)hipGetLastError();
}
