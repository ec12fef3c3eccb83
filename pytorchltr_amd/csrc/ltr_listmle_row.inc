// ltr_listmle_row.inc -- the ListMLE row of one staged query on the ranked-row core's LDS layout (ltr_ranked.inc), and
// the two scan operators under it.  Included by ltr_listmle.inc (listmle_kernel, the long path's epilogues; with it
// ltr_linear_listwise.inc) and by ltr_mlp.hip (the listwise slot of the fused MLP step, ltr_mlp_listwise.inc).  The
// scans and their orders are described at the top of ltr_listmle.inc.
#pragma once

namespace {

// ---- the two scan operators ----
// (max, sum) pairs: (m, s) stands for s exp(m).  Commutative; no exp of a positive argument; (-inf, 0) is the identity.
__device__ __forceinline__ void ms_add(float &m, float &s, float m2, float s2)
{
    const float hi = fmaxf(m, m2), lo = fminf(m, m2);
    const float e = lo == -INFINITY ? 0.f : expf(lo - hi);
    s = m >= m2 ? s + s2 * e : s * e + s2;
    m = hi;
}

// affine maps D -> a D + b: (a, b) = (a1, b1) then (a2, b2).  Identity (1, 0).
__device__ __forceinline__ void aff_then(float &a, float &b, float a2, float b2)
{
    b = __builtin_fmaf(a2, b, b2);
    a = a * a2;
}

// The two as operators of block_pair_scan.  ms_add's rounding depends on which argument is the larger, so each
// states the order it has always been called in: a lane's own pair first in the wave ladder of (max, sum), the
// predecessor's map first in that of the affine maps.
struct MaxSum {
    static constexpr float idx = -INFINITY, idy = 0.f;
    static __device__ __forceinline__ void then(float &m, float &s, float m2, float s2) { ms_add(m, s, m2, s2); }
    static __device__ __forceinline__ void after(float &m, float &s, float pm, float ps) { ms_add(m, s, pm, ps); }
};
struct Affine {
    static constexpr float idx = 1.f, idy = 0.f;
    static __device__ __forceinline__ void then(float &a, float &b, float a2, float b2) { aff_then(a, b, a2, b2); }
    static __device__ __forceinline__ void after(float &a, float &b, float pa, float pb) { aff_then(pa, pb, a, b); a = pa; b = pb; }
};

// a_i = exp(LSE_i - LSE_{i-1}) from the (M, log S) pairs of ranks i and i - 1 (<= 1; clamped against rounding)
__device__ __forceinline__ float lse_step(float m, float ls, float mp, float lsp)
{
    return expf(fminf((m - mp) + (ls - lsp), 0.f));
}

// exp(x - LSE) <= 1
__device__ __forceinline__ float lse_prob(float x, float m, float ls) { return expf(fminf((x - m) - ls, 0.f)); }

// The ListMLE row of one staged query: q.sy holds the (label, score) pairs of the first nb documents (metric_ranks ranks
// the x slot).  Ranks by label, scans, stores the loss of the first K factors to *loss and, `grad`, leaves the gradient
// BY RANK in q.curve, published: document j's is q.curve[q.rank_s[j]].  What listmle_kernel and linear_listwise_kernel
// (ltr_linear_listwise.inc) share.  Contains barriers: call from uniform code, behind the barrier that publishes q.sy.
template <int DPT>
__device__ __forceinline__ void listmle_row(const MetricParams &m, const RankedRowLds &q, int nb, int K, float *loss, bool grad)
{
    const int L4 = (m.L + 3) & ~3;
    const int tid = row_tid();
    const int T = blockDim.x;
    float2 *sy = q.sy;
    int *rank_s = q.rank_s;
    float *xs = reinterpret_cast<float *>(q.rank_y);                   // ranked scores (rank_y's slot)
    float *curve = q.curve;                                            // the gradient by rank
    float *red = q.red, *pair = q.scan;
    float *mx = reinterpret_cast<float *>(q.sy), *ls = mx + L4;        // (M_i, log S_i), over sy once it is read

    for (int j = tid; j < L4; j += T) rank_s[j] = 0;
    __syncthreads();
    metric_ranks<DPT>(m, q, nb, false);
    __syncthreads();
    for (int j = tid; j < nb; j += T) xs[rank_s[j]] = sy[j].y;
    __syncthreads();

    // 1. suffix (max, sum) scan: thread t owns ranks nb - 1 - [t ch, (t + 1) ch), walked downwards
    const int ch = (nb + T - 1) / T;
    const int lo = min(nb, tid * ch), hi = min(nb, lo + ch);
    float cm = -INFINITY, cs = 0.f, tm, ts;
    for (int u = lo; u < hi; ++u) ms_add(cm, cs, xs[nb - 1 - u], 1.f);
    block_pair_scan<MaxSum>(cm, cs, tm, ts, pair);
    for (int u = lo; u < hi; ++u) {
        const int i = nb - 1 - u;
        ms_add(cm, cs, xs[i], 1.f);
        mx[i] = cm;
        ls[i] = logf(cs);
    }
    __syncthreads();
    float acc = 0.f;
    for (int i = tid; i < K; i += T) acc += (mx[i] - xs[i]) + ls[i];
    acc = block_sum(acc, red);
    if (tid == 0) *loss = acc;
    if (!grad) return;

    // 2. gradient scan: thread t owns ranks [t ch, (t + 1) ch), walked upwards
    float ca = 1.f, cb = 0.f, ta, tb;
    for (int i = lo; i < hi; ++i)
        aff_then(ca, cb, i > 0 ? lse_step(mx[i], ls[i], mx[i - 1], ls[i - 1]) : 0.f, i < K ? 1.f : 0.f);
    block_pair_scan<Affine>(ca, cb, ta, tb, pair);
    float d = cb;                                                      // D before the chunk (D_{-1} = 0)
    for (int i = lo; i < hi; ++i) {
        const float bi = i < K ? 1.f : 0.f;
        d = __builtin_fmaf(i > 0 ? lse_step(mx[i], ls[i], mx[i - 1], ls[i - 1]) : 0.f, d, bi);
        curve[i] = lse_prob(xs[i], mx[i], ls[i]) * d - bi;
    }
    __syncthreads();
}

}  // namespace
