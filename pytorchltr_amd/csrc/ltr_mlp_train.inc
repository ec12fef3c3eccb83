// ltr_mlp_train.inc -- the fused MLP training step with the optimizer update inside the reduction launch
// (include/ltr_mlp_train.h; DESIGN.md 28, 29).  Included behind ltr_mlp_step.inc, whose launch path and guards it uses
// as they are; the two reduce-and-update kernels are the reduction cores of ltr_mlp_reduce.inc -- the geometry and the
// summation order of mlp_reduce4_kernel and mlp_reduce_kernel -- with the update rule as their epilogue, behind the
// final sum, in the thread that holds it.
#include "ltr_mlp_train.h"

// What the update kernels get: the six parameter tensors, the flat layout's segment starts, the state and the rule's
// scalars.  fp32 scalars are rounded from the caller's doubles once, on the host; what depends on t stays double.
struct MlpTrainArgs {
    float *par[6];                 // W1 (rows of w1_pitch floats), b1, W2, b2, W3, b3
    int seg[6];                    // first flat index of each tensor ([0] = 0); P behind the last
    int P, F, w1_pitch;
    float *state;                  // nbuf x P floats, then the header; may be nullptr (SGD without momentum)
    unsigned *hdr;                 // {t, ticket, 0, 0}; nullptr with state
    float *grads_out;              // may be nullptr
    int algo, nesterov;
    float lr, wd, mu, omd, eps, b1, omb1, b2, omb2;        // omd = 1 - dampening, omb = 1 - beta
    double lr_d, lr_decay_d, b1_d, b2_d;
};

// per-workgroup scalars of a step, written by one thread (LDS): t, and the rule's t-dependent factors
struct MlpTrainStep {
    unsigned t;
    float s0;                      // Adagrad: clr; Adam: lr / (1 - beta1^(t+1)); SGD: lr
    float s1;                      // Adam: sqrt(1 - beta2^(t+1))
};

// One thread of every workgroup reads t (mlp_train_read_t), THEN takes the workgroup's ticket (mlp_train_ticket).  The
// load has returned (vmcnt(0)) before the atomic is issued, so no workgroup can read the t + 1 that the holder of the
// last ticket stores.  t and the ticket are written by agent-scope atomics (write-through, never left in one XCD's L2);
// the next launch in stream order reads them behind the kernel boundary.  The two halves are apart so that a reduction
// can issue the load ahead of its sums and take the ticket in a wave that idles behind them.
__device__ inline unsigned mlp_train_read_t(const MlpTrainArgs &a)
{
    return a.hdr ? __hip_atomic_load(a.hdr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
}

__device__ inline void mlp_train_ticket(const MlpTrainArgs &a, unsigned t, MlpTrainStep *st)
{
    if (a.hdr) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned ticket = __hip_atomic_fetch_add(a.hdr + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (ticket == gridDim.x - 1) {
            __hip_atomic_store(a.hdr, t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(a.hdr + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    st->t = t;
    st->s0 = a.lr;
    st->s1 = 1.0f;
    if (a.algo == LTR_OPT_ADAGRAD) {
        st->s0 = (float)(a.lr_d / (1.0 + (double)t * a.lr_decay_d));
    } else if (a.algo == LTR_OPT_ADAM) {
        const double step = (double)t + 1.0;
        st->s0 = (float)(a.lr_d / (1.0 - pow(a.b1_d, step)));
        st->s1 = (float)sqrt(1.0 - pow(a.b2_d, step));
    }
}

__device__ inline void mlp_train_begin(const MlpTrainArgs &a, MlpTrainStep *st) { mlp_train_ticket(a, mlp_train_read_t(a), st); }

// the address of parameter `i` of the flat layout, or nullptr for a gradient column of W1's zero padding
__device__ inline float *mlp_train_addr(const MlpTrainArgs &a, int i)
{
    const int s = (i >= a.seg[1]) + (i >= a.seg[2]) + (i >= a.seg[3]) + (i >= a.seg[4]) + (i >= a.seg[5]);
    if (s == 0) {
        const int row = i / a.F, col = i - row * a.F;
        return col < a.w1_pitch ? a.par[0] + (size_t)row * a.w1_pitch + col : nullptr;
    }
    return a.par[s] + (i - a.seg[s]);
}

// one parameter: p, its state x0 (momentum buffer / sum / exp_avg) and x1 (exp_avg_sq), its gradient g
__device__ inline void mlp_train_rule(const MlpTrainArgs &a, const MlpTrainStep &st, float g, float &p, float &x0, float &x1)
{
    if (a.wd != 0.f) g = g + a.wd * p;
    if (a.algo == LTR_OPT_SGD) {
        if (a.mu != 0.f) {
            x0 = st.t == 0 ? g : a.mu * x0 + a.omd * g;
            g = a.nesterov ? g + a.mu * x0 : x0;
        }
        p = p - a.lr * g;
    } else if (a.algo == LTR_OPT_ADAGRAD) {
        x0 = x0 + g * g;
        p = p - st.s0 * (g / (sqrtf(x0) + a.eps));
    } else {
        x0 = a.b1 * x0 + a.omb1 * g;
        x1 = a.b2 * x1 + a.omb2 * (g * g);
        p = p - st.s0 * (x0 / (sqrtf(x1) / st.s1 + a.eps));
    }
}

// The epilogue of a thread that holds N consecutive gradients from flat index `i` (N = 1 or 4), in two halves: the loads
// of the parameters and their state (mlp_train_load: they depend on nothing the launch computes, so a reduction issues
// them ahead of its last fold), then the rule and the stores (mlp_train_finish).  The segment starts are no multiples of
// 4: every element is mapped on its own, and parameters or state move as one float4 only where the four addresses are
// consecutive and 16-byte aligned.
template <int N>
struct MlpTrainElems {
    float *pp[N];                  // the parameters' addresses; nullptr: past P, or a column of W1's zero padding
    float p[N], x0[N], x1[N];
    bool vec, vec0, vec1;          // parameters / first / second state buffer as one float4
};

template <int N>
__device__ inline void mlp_train_load(const MlpTrainArgs &a, int i, MlpTrainElems<N> &e)
{
#pragma unroll
    for (int k = 0; k < N; ++k) e.pp[k] = i + k < a.P ? mlp_train_addr(a, i + k) : nullptr;
    const bool need0 = a.algo != LTR_OPT_SGD || a.mu != 0.f, need1 = a.algo == LTR_OPT_ADAM;
    const float *s0 = a.state + i, *s1 = a.state + (size_t)a.P + i;
    e.vec = false;
    if (N == 4) {
        e.vec = e.pp[0] && e.pp[N > 1 ? 1 : 0] == e.pp[0] + 1 && e.pp[N > 2 ? 2 : 0] == e.pp[0] + 2 &&
                e.pp[N > 3 ? 3 : 0] == e.pp[0] + 3 && mlp_aligned16(e.pp[0]);
    }
    e.vec0 = N == 4 && need0 && e.vec && mlp_aligned16(s0);
    e.vec1 = N == 4 && need1 && e.vec && mlp_aligned16(s1);
    if (e.vec) {
        const float4 v = *reinterpret_cast<const float4 *>(e.pp[0]);
        e.p[0] = v.x; e.p[N > 1 ? 1 : 0] = v.y; e.p[N > 2 ? 2 : 0] = v.z; e.p[N > 3 ? 3 : 0] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) e.p[k] = e.pp[k] ? *e.pp[k] : 0.f;
    }
    if (e.vec0) {
        const float4 v = *reinterpret_cast<const float4 *>(s0);
        e.x0[0] = v.x; e.x0[N > 1 ? 1 : 0] = v.y; e.x0[N > 2 ? 2 : 0] = v.z; e.x0[N > 3 ? 3 : 0] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) e.x0[k] = need0 && e.pp[k] ? s0[k] : 0.f;
    }
    if (e.vec1) {
        const float4 v = *reinterpret_cast<const float4 *>(s1);
        e.x1[0] = v.x; e.x1[N > 1 ? 1 : 0] = v.y; e.x1[N > 2 ? 2 : 0] = v.z; e.x1[N > 3 ? 3 : 0] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) e.x1[k] = need1 && e.pp[k] ? s1[k] : 0.f;
    }
}

template <int N>
__device__ inline void mlp_train_finish(const MlpTrainArgs &a, const MlpTrainStep &st, int i, const float *g,
                                        MlpTrainElems<N> &e)
{
    if (a.grads_out) {
        if (N == 4 && i + 3 < a.P && mlp_aligned16(a.grads_out + i)) {
            *reinterpret_cast<float4 *>(a.grads_out + i) = make_float4(g[0], g[N > 1 ? 1 : 0], g[N > 2 ? 2 : 0], g[N > 3 ? 3 : 0]);
        } else {
#pragma unroll
            for (int k = 0; k < N; ++k)
                if (i + k < a.P) a.grads_out[i + k] = g[k];
        }
    }
    const bool need0 = a.algo != LTR_OPT_SGD || a.mu != 0.f, need1 = a.algo == LTR_OPT_ADAM;
    float *s0 = a.state + i, *s1 = a.state + (size_t)a.P + i;
#pragma unroll
    for (int k = 0; k < N; ++k) mlp_train_rule(a, st, g[k], e.p[k], e.x0[k], e.x1[k]);
    if (e.vec) {
        *reinterpret_cast<float4 *>(e.pp[0]) = make_float4(e.p[0], e.p[N > 1 ? 1 : 0], e.p[N > 2 ? 2 : 0], e.p[N > 3 ? 3 : 0]);
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (e.pp[k]) *e.pp[k] = e.p[k];
    }
    if (e.vec0) {
        *reinterpret_cast<float4 *>(s0) = make_float4(e.x0[0], e.x0[N > 1 ? 1 : 0], e.x0[N > 2 ? 2 : 0], e.x0[N > 3 ? 3 : 0]);
    } else if (need0) {
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (e.pp[k]) s0[k] = e.x0[k];
    }
    if (e.vec1) {
        *reinterpret_cast<float4 *>(s1) = make_float4(e.x1[0], e.x1[N > 1 ? 1 : 0], e.x1[N > 2 ? 2 : 0], e.x1[N > 3 ? 3 : 0]);
    } else if (need1) {
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (e.pp[k]) s1[k] = e.x1[k];
    }
}

template <int N>
__device__ inline void mlp_train_update(const MlpTrainArgs &a, const MlpTrainStep &st, int i, const float *g)
{
    MlpTrainElems<N> e;
    mlp_train_load<N>(a, i, e);
    mlp_train_finish<N>(a, st, i, g, e);
}

// The update as the epilogue of a reduction core (ltr_mlp_reduce.inc): the gradient it consumes is the core's sum, the
// very additions of mlp_reduce_kernel / mlp_reduce4_kernel.  In the float4 core the owners of the block's columns fetch
// their parameters and state ahead of the two folds, and thread 1023 takes the ticket between the barriers with the t
// it read at kernel entry; the 4-byte core (one barrier, the fallback of an unaligned workspace) begins in its kernel
// and loads behind its fold.
template <int N>
struct MlpTrainEpilogue {
    const MlpTrainArgs &a;
    MlpTrainStep *step;            // LDS; written by between() (N = 4) or by the kernel ahead of the core (N = 1)
    unsigned t_read;               // N = 4, thread 1023: mlp_train_read_t at kernel entry
    MlpTrainElems<N> el;           // (left as it is until fetch: only the owners' are ever read)
    __device__ __forceinline__ MlpTrainEpilogue(const MlpTrainArgs &a, MlpTrainStep *step, unsigned t_read)
        : a(a), step(step), t_read(t_read) {}
    __device__ __forceinline__ void fetch(int i) { mlp_train_load<N>(a, i, el); }
    __device__ __forceinline__ void between()
    {
        if (threadIdx.x == 1023) mlp_train_ticket(a, t_read, step);
    }
    __device__ __forceinline__ void finish(int i, const float *g)
    {
        if (N == 1) mlp_train_load<N>(a, i, el);
        mlp_train_finish<N>(a, *step, i, g, el);
    }
};

// mlp_reduce_kernel (mlp_reduce_core) with the update behind the sum of column i
__global__ void __launch_bounds__(kMlpRedCols * kMlpRedSlices)
mlp_reduce_update_kernel(const float *__restrict__ part, int nPart, int pitch, const float *__restrict__ loss, int B,
                         float *__restrict__ loss_sum, MlpTrainArgs a)
{
    __shared__ MlpTrainStep step;
    if (threadIdx.x == 0) mlp_train_begin(a, &step);
    MlpTrainEpilogue<1> update(a, &step, 0);
    mlp_reduce_core(part, nPart, a.P, pitch, update);
    if (loss_sum && blockIdx.x == 0) mlp_reduce_loss_sum(loss, B, loss_sum);
}

// mlp_reduce4_kernel (mlp_reduce4_core) with the update behind the float4 at 4 * c4
template <int COLS4>
__global__ void __launch_bounds__(1024)
mlp_reduce_update4_kernel(const float *__restrict__ part, int nPart, int pitch, const float *__restrict__ loss, int B,
                          float *__restrict__ loss_sum, MlpTrainArgs a)
{
    __shared__ MlpTrainStep step;
    // the last thread (a wave with nothing to do behind the first barrier) reads t now and takes the ticket there
    unsigned t_read = 0;
    if (threadIdx.x == 1023) t_read = mlp_train_read_t(a);
    MlpTrainEpilogue<4> update(a, &step, t_read);
    mlp_reduce4_core<COLS4>(part, nPart, pitch, update);
    if (loss_sum && blockIdx.x == 0) mlp_reduce_loss_sum(loss, B, loss_sum);
}

// the update alone, on a flat gradient already summed: 256 threads x 4 parameters a block
constexpr int kMlpApplyThreads = 256;
__global__ void __launch_bounds__(kMlpApplyThreads)
mlp_apply_update_kernel(const float *__restrict__ grads, MlpTrainArgs a)
{
    __shared__ MlpTrainStep step;
    if (threadIdx.x == 0) mlp_train_begin(a, &step);
    __syncthreads();
    const int i = 4 * (blockIdx.x * kMlpApplyThreads + threadIdx.x);
    if (i >= a.P) return;
    float g[4];
    if (i + 3 < a.P && mlp_aligned16(grads + i)) {
        const float4 v = *reinterpret_cast<const float4 *>(grads + i);
        g[0] = v.x; g[1] = v.y; g[2] = v.z; g[3] = v.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) g[e] = i + e < a.P ? grads[i + e] : 0.f;
    }
    mlp_train_update<4>(a, step, i, g);
}

// ---- host side ----
inline int mlp_train_nbuf(int algo) { return algo == LTR_OPT_ADAM ? 2 : 1; }

inline bool mlp_train_bad_scalar(double v) { return !std::isfinite(v) || v < 0.0; }

// the hyper-parameter guard of both entry points (after the algo's): what torch.optim refuses
inline bool mlp_train_bad_optim(const ltr_mlp_optim &o)
{
    if (mlp_train_bad_scalar(o.lr) || mlp_train_bad_scalar(o.weight_decay)) return true;
    if (o.algo == LTR_OPT_SGD) {
        if (mlp_train_bad_scalar(o.momentum) || !std::isfinite(o.dampening)) return true;
        return o.nesterov && (o.momentum <= 0.0 || o.dampening != 0.0);
    }
    if (mlp_train_bad_scalar(o.eps)) return true;
    if (o.algo == LTR_OPT_ADAGRAD) return mlp_train_bad_scalar(o.lr_decay);
    return !(o.beta1 >= 0.0 && o.beta1 < 1.0) || !(o.beta2 >= 0.0 && o.beta2 < 1.0);
}

inline bool mlp_train_needs_state(const ltr_mlp_optim &o) { return o.algo != LTR_OPT_SGD || o.momentum != 0.0; }

inline MlpTrainArgs mlp_train_args(float *W1, float *b1, float *W2, float *b2, float *W3, float *b3, int w1_pitch,
                                   float *state, const ltr_mlp_optim &o, float *grads_out, int F, int H1, int H2)
{
    MlpTrainArgs a;
    a.par[0] = W1; a.par[1] = b1; a.par[2] = W2; a.par[3] = b2; a.par[4] = W3; a.par[5] = b3;
    a.seg[0] = 0; a.seg[1] = H1 * F; a.seg[2] = a.seg[1] + H1; a.seg[3] = a.seg[2] + H2 * H1;
    a.seg[4] = a.seg[3] + H2; a.seg[5] = a.seg[4] + H2;
    a.P = mlp_param_count(F, H1, H2); a.F = F; a.w1_pitch = w1_pitch;
    a.state = state;
    a.hdr = state ? reinterpret_cast<unsigned *>(state + LTR_MLP_TRAIN_HEADER_AT((size_t)mlp_train_nbuf(o.algo) * a.P))
                  : nullptr;
    a.grads_out = grads_out;
    a.algo = o.algo; a.nesterov = o.nesterov ? 1 : 0;
    a.lr = (float)o.lr; a.wd = (float)o.weight_decay; a.mu = (float)o.momentum; a.omd = (float)(1.0 - o.dampening);
    a.eps = (float)o.eps; a.b1 = (float)o.beta1; a.omb1 = (float)(1.0 - o.beta1); a.b2 = (float)o.beta2;
    a.omb2 = (float)(1.0 - o.beta2);
    a.lr_d = o.lr; a.lr_decay_d = o.lr_decay; a.b1_d = o.beta1; a.b2_d = o.beta2;
    if (o.algo != LTR_OPT_SGD) a.mu = 0.f;
    return a;
}

// the reduce-and-update launch in the place of mlp_reduce_launch: the float4 kernel under its alignment rule
inline int mlp_reduce_update_launch(void *workspace, int grid, const MlpTrainArgs &a, const float *loss, int B,
                                    float *loss_sum, hipStream_t s)
{
    // (no flat output that must be a float4: the epilogue moves 16 bytes only where its own addresses allow it)
    const bool vec4 = mlp_aligned16(workspace);
    const auto kernel = vec4 ? mlp_reduce_update4_kernel<kMlpRedCols4> : mlp_reduce_update_kernel;
    hipLaunchKernelGGL(kernel, mlp_reduce_blocks(a.P, vec4), dim3(kMlpRedThreads), 0, s, (const float *)workspace, grid,
                       mlp_pitch(a.P), loss, B, loss_sum, a);
    return (int)hipGetLastError();
}

extern "C" {

size_t ltr_mlp_train_state_floats(int algo, int F, int H1, int H2)
{
    if (algo < LTR_OPT_SGD || algo > LTR_OPT_ADAM || F <= 0 || H1 <= 0 || H2 <= 0) return 0;
    return LTR_MLP_TRAIN_HEADER_AT((size_t)mlp_train_nbuf(algo) * (size_t)mlp_param_count(F, H1, H2)) + 4;
}

int ltr_mlp_train_step_f32(int family, int code, int k, float sigma, const float *X, float *W1, float *b1, float *W2,
                           float *b2, float *W3, float *b3, int w1_pitch, const float *W1_rows, const void *rel,
                           int rel_dtype, const int64_t *n, const int32_t *tie, int use_seed, uint64_t seed,
                           const int64_t *seed_dev, const float *grad_out, int B, int L, int F, int H1, int H2,
                           float *loss, float *scores_out, float *loss_sum, float *state,
                           const struct ltr_mlp_optim *optim, float *grads_out, void *workspace,
                           size_t workspace_bytes, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (!optim) return LTR_ERR_NULL;
    if (family < LTR_MLP_TRAIN_PAIRWISE || family > LTR_MLP_TRAIN_LAMBDARANK || bad_label_dtype(rel_dtype)) return LTR_ERR_KIND;
    if (family == LTR_MLP_TRAIN_PAIRWISE && (code < LTR_HINGE || code > LTR_NDCG2)) return LTR_ERR_KIND;
    if (family == LTR_MLP_TRAIN_LISTWISE && bad_mlp_listwise_loss(code)) return LTR_ERR_KIND;
    if (optim->algo < LTR_OPT_SGD || optim->algo > LTR_OPT_ADAM) return LTR_ERR_KIND;
    if (mlp_step_bad_network(B, L, F, H1, H2)) return LTR_ERR_SHAPE;
    if (family == LTR_MLP_TRAIN_LAMBDARANK && !std::isfinite(sigma)) return LTR_ERR_SHAPE;
    if (w1_pitch < 1 || w1_pitch > F || mlp_train_bad_optim(*optim)) return LTR_ERR_SHAPE;
    if (L > mlp_step_max_len(F)) return LTR_ERR_LIST_TOO_LONG;
    if (B == 0) return LTR_OK;
    if (!X || !W1 || !b1 || !W2 || !b2 || !W3 || !b3 || !rel || !n || !loss) return LTR_ERR_NULL;
    if ((!state && mlp_train_needs_state(*optim)) || (w1_pitch < F && !W1_rows)) return LTR_ERR_NULL;
    // the MFMA launch of the family's entry point: the same call description through the same launch path
    const int slot = family == LTR_MLP_TRAIN_PAIRWISE ? code
                     : family == LTR_MLP_TRAIN_LAMBDARANK ? LTR_MLP_LAMBDARANK : mlp_listwise_slot_of(code);
    const MlpStepCall call{slot, sigma, k, tie, use_seed, seed, seed_dev, X, W1_rows ? W1_rows : W1, b1, W2, b2, W3, b3,
                           rel, rel_dtype, n, grad_out, B, L, F, H1, H2, loss, scores_out, workspace, workspace_bytes};
    hipStream_t s = (hipStream_t)stream;
    int grid;
    const int rc = mlp_step_launch(call, grid, s);
    if (rc != 0) return rc;
    return mlp_reduce_update_launch(workspace, grid, mlp_train_args(W1, b1, W2, b2, W3, b3, w1_pitch, state, *optim,
                                                                    grads_out, F, H1, H2), loss, B, loss_sum, s);
}

int ltr_mlp_apply_update_f32(const float *grads, float *W1, float *b1, float *W2, float *b2, float *W3, float *b3,
                             int w1_pitch, float *state, const struct ltr_mlp_optim *optim, int F, int H1, int H2,
                             void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (!optim) return LTR_ERR_NULL;
    if (optim->algo < LTR_OPT_SGD || optim->algo > LTR_OPT_ADAM) return LTR_ERR_KIND;
    if (F <= 0 || H1 <= 0 || H2 <= 0 || w1_pitch < 1 || w1_pitch > F || mlp_train_bad_optim(*optim)) return LTR_ERR_SHAPE;
    if (!grads || !W1 || !b1 || !W2 || !b2 || !W3 || !b3) return LTR_ERR_NULL;
    if (!state && mlp_train_needs_state(*optim)) return LTR_ERR_NULL;
    const MlpTrainArgs a = mlp_train_args(W1, b1, W2, b2, W3, b3, w1_pitch, state, *optim, nullptr, F, H1, H2);
    const int per = 4 * kMlpApplyThreads;
    hipLaunchKernelGGL(mlp_apply_update_kernel, dim3((unsigned)((a.P + per - 1) / per)), dim3(kMlpApplyThreads), 0,
                       (hipStream_t)stream, grads, a);
    return (int)hipGetLastError();
}

}  // extern "C"
