// ltr_linear_listwise.inc -- the Linear(F, 1) scorer fused with the listwise losses, ListNet (the listwise softmax of
// ltr_listwise_softmax_f32) and ListMLE (included by ltr_kernels.hip after ltr_listmle.inc; C ABI:
// include/ltr_listwise.h; DESIGN.md 15), and with LambdaRank (kLossLambdaRank below, an internal loss code: its entry
// points are in ltr_lambdarank.inc, C ABI include/ltr_lambdarank.h; DESIGN.md 25).
//
// linear_listwise_kernel, one workgroup per query on the ranked-row core's launch shapes (metric_shape, launch_ranked):
//   1. scores  s_j = X[b, j, :] . W + bias of the real documents j < n_b, one wave per row, straight into the slot the
//      row function reads (sy[j].y); scores_out, when asked for, gets them too (0 for padded documents);
//   2. the loss row: ListMLE -- listmle_row, the row function of listmle_kernel --, LambdaRank -- lambdarank_row, that
//      of lambdarank_kernel -- or ListNet, workgroup-wide max / sum of the scores and the labels; the gradient by
//      document g_j ends in the icurve slot of the core's layout, which no loss uses once its row is done;
//   3. the weight-gradient row  dW_b = sum_{j < n_b} g_j X[b, j, :], db_b = sum_j g_j: threads as (row r, column
//      vector c), R rows per iteration, the R partial rows added in order through LDS, stored as row b of the
//      (B, partial_pitch(F)) matrix that ltr_linear_reduce_* consume.
// Rows j >= n_b are never read (0 * NaN is NaN).  Rows are whole, 16-byte aligned float4 (F % 4 == 0).  No atomics, every
// sum in a fixed order: bit-identical run to run.  Behind the core's layout the dynamic LDS holds W float[F] and the
// cross-row buffer float4[R * min(F / 4, T)].

#include "ltr_lambdarank_row.inc"

namespace {

constexpr int kLossLambdaRank = 2;       // the third LOSS value of linear_listwise_kernel; not a code of ltr_listwise.h

struct LinearListwiseParams {
    MetricParams m;          // the batch and the tie words (m.scores, m.out unused)
    const float *X, *W, *bias;
    float *loss, *scores_out, *part;
    int F;
    int k;                   // ListMLE: <= 0 every factor; LambdaRank: <= 0 no cutoff
    int R;                   // rows per workgroup iteration of phase 3
    float sigma;             // LambdaRank
};

struct OpMax { static constexpr float id = -INFINITY; static __device__ __forceinline__ float f(float a, float b) { return fmaxf(a, b); } };

// The bytes of the core's layout a loss uses, where W starts.  ListNet ranks nothing: it keeps sy, the gradient
// (icurve) and the reduction scratch of the counting-rank layout.
__host__ __device__ inline size_t linear_listwise_core_bytes(int loss, int L, bool sort)
{
    if (loss == LTR_LISTWISE_LISTNET) return ranked_row_layout(L, false).red + (32 + 64) * 4;
    return ranked_row_layout(L, sort).end;
}

constexpr int kListwiseUnr = 4;          // rows in flight per wave (phase 1) / per thread (phase 3)
constexpr int kListwiseMaxR = 64;        // the R partial rows are added by one thread per column vector

// The query of workgroup blockIdx.x, start to end: the body of linear_listwise_kernel and linear_lambdarank_kernel below.
template <int LOSS, int DPT>
__device__ __forceinline__ void linear_listwise_query(const LinearListwiseParams &p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool kSort = LOSS != LTR_LISTWISE_LISTNET && DPT <= 0;
    constexpr bool kScoreFirst = LOSS == kLossLambdaRank;              // its row takes (score, label) pairs
    const MetricParams &m = p.m;
    const int b = blockIdx.x;
    const int L = m.L, F = p.F;
    const int C = F >> 2;                                              // column vectors per row
    const int tid = threadIdx.x, T = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, nwaves = T >> 6;
    const int nb = clamp_n(m.n[b], L);

    const RankedRowLds q = ranked_row_lds(smem, L, kSort);
    float *wl = reinterpret_cast<float *>(smem + linear_listwise_core_bytes(LOSS, L, kSort));
    float4 *dred = reinterpret_cast<float4 *>(wl + F);
    float *g = q.icurve;                                               // the gradient by document
    const size_t row = (size_t)b * L;
    const float *Xq = p.X + row * (size_t)F;

    // (label, score) pairs, as listmle_kernel stages them; LambdaRank: (score, label), as lambdarank_kernel does
    for (int f = tid; f < F; f += T) wl[f] = p.W[f];
    for (int j = tid; j < nb; j += T) (kScoreFirst ? q.sy[j].y : q.sy[j].x) = load_label(m.rel, m.rel_dtype, row + j);
    const float bias = p.bias ? p.bias[0] : 0.f;
    __syncthreads();

    // ---- phase 1: the scores of the real documents, one wave per row ----
    {
        const float4 *wv = reinterpret_cast<const float4 *>(wl);
        constexpr int UNR = kListwiseUnr;
        for (int l0 = wave; l0 < nb; l0 += nwaves * UNR) {
            float acc[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) acc[u] = 0.f;
            for (int c = lane; c < C; c += 64) {
                float4 x[UNR];
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    const int l = l0 + u * nwaves;
                    x[u] = (l < nb) ? reinterpret_cast<const float4 *>(Xq + (size_t)l * F)[c] : vzero<float4>();
                }
                const float4 w = wv[c];
#pragma unroll
                for (int u = 0; u < UNR; ++u) acc[u] += vdot(x[u], w);
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int l = l0 + u * nwaves;
                const float s = wave_sum(acc[u]) + bias;
                if (lane == 0 && l < nb) {
                    (kScoreFirst ? q.sy[l].x : q.sy[l].y) = s;
                    if (p.scores_out) p.scores_out[row + l] = s;
                }
            }
        }
        if (p.scores_out)
            for (int j = nb + tid; j < L; j += T) p.scores_out[row + j] = 0.f;
    }
    __syncthreads();

    // ---- phase 2: the loss row; g[j] = d loss[b] / d s_j ----
    float gs = 0.f;
    if constexpr (LOSS == LTR_LISTWISE_LISTMLE) {
        listmle_row<DPT>(m, q, nb, p.k > 0 ? min(p.k, nb) : nb, p.loss + b, true);
        for (int j = tid; j < nb; j += T) {
            const float v = q.curve[q.rank_s[j]];
            g[j] = v;
            gs += v;
        }
    } else if constexpr (LOSS == kLossLambdaRank) {
        lambdarank_row<DPT>(m, q, nb, p.k > 0 ? min(p.k, nb) : nb, p.sigma, p.loss + b, true);
        const float *gr = reinterpret_cast<const float *>(q.rank_y);
        for (int j = tid; j < nb; j += T) {
            const float v = gr[q.rank_s[j]];
            g[j] = v;
            gs += v;
        }
    } else {
        float ms = -INFINITY, my = -INFINITY;
        for (int j = tid; j < nb; j += T) {
            const float2 v = q.sy[j];
            my = fmaxf(my, v.x);
            ms = fmaxf(ms, v.y);
        }
        ms = block_reduce<OpMax>(ms, q.red);
        my = block_reduce<OpMax>(my, q.red);
        float zs = 0.f, zy = 0.f, dot = 0.f;
        for (int j = tid; j < nb; j += T) {
            const float2 v = q.sy[j];
            const float ds = v.y - ms;
            const float ey = expf(v.x - my);
            zs += expf(ds);
            zy += ey;
            dot += ey * ds;
        }
        block_sum2(zs, zy, q.red);
        dot = block_sum(dot, q.red);
        const float inv_zs = nb > 0 ? 1.0f / zs : 0.f;
        const float inv_zy = nb > 0 ? 1.0f / zy : 0.f;
        for (int j = tid; j < nb; j += T) {
            const float2 v = q.sy[j];
            const float gj = expf(v.y - ms) * inv_zs - expf(v.x - my) * inv_zy;
            g[j] = gj;
            gs += gj;
        }
        if (tid == 0) p.loss[b] = nb > 0 ? (logf(zs) - dot * inv_zy) : 0.f;
    }
    const float gsum = block_sum(gs, q.red);                           // d / d bias
    __syncthreads();                                                   // g is published (one wave: block_sum has no barrier)

    // ---- phase 3: dW_b[f] = sum_j g[j] X[b, j, f], columns in tiles of CT = min(C, T) vectors, R row groups per tile ----
    float *part = p.part + (size_t)b * partial_pitch(F);
    const int R = p.R;
    const int CT = C < T ? C : T;
    const int cl = tid % CT;
    const int r = tid / CT;
    for (int c0 = 0; c0 < C; c0 += CT) {
        const int c = c0 + cl;
        if (r < R && c < C) {
            float4 acc = vzero<float4>();
            constexpr int UNR = kListwiseUnr;
            for (int l0 = r; l0 < nb; l0 += R * UNR) {
                float4 x[UNR];
                float gv[UNR];
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    const int lf = l0 + u * R;
                    const bool ok = lf < nb;
                    // rows in reverse: the rows phase 1 read last are the likeliest to be in L2 still
                    const int l = ok ? nb - 1 - lf : 0;
                    gv[u] = ok ? g[l] : 0.f;
                    x[u] = ok ? reinterpret_cast<const float4 *>(Xq + (size_t)l * F)[c] : vzero<float4>();
                }
#pragma unroll
                for (int u = 0; u < UNR; ++u) vfma(acc, gv[u], x[u]);
            }
            dred[(size_t)r * CT + cl] = acc;
        }
        __syncthreads();
        if (tid < CT && c0 + tid < C) {
            float4 s = vzero<float4>();
            for (int rr = 0; rr < R; ++rr) vadd(s, dred[(size_t)rr * CT + tid]);
            reinterpret_cast<float4 *>(part)[c0 + tid] = s;            // coalesced: consecutive threads, consecutive columns
        }
        lds_barrier();                                                 // (dred is rewritten by the next tile)
    }
    if (tid == 0) {
        part[F] = gsum;
        for (int f = F + 1; f < partial_pitch(F); ++f) part[f] = 0.f;
    }
}

// (the launch bounds of the ranked-row core's kernels; ListNet has one instantiation, DPT = 0, for every shape)
template <int LOSS, int DPT>
__global__ void __launch_bounds__(1024, (DPT <= 0 ? 8 : 4))
linear_listwise_kernel(LinearListwiseParams p)
{
    linear_listwise_query<LOSS, DPT>(p);
}

// LambdaRank in the loss slot: the six launch shapes of the core, under a name of their own
template <int DPT>
__global__ void __launch_bounds__(1024, (DPT <= 0 ? 8 : 4))
linear_lambdarank_kernel(LinearListwiseParams p)
{
    linear_listwise_query<kLossLambdaRank, DPT>(p);
}

// The launch of (loss, B, L, F): the ranked-row core's shape -- ListNet, which ranks nothing, in the counting-rank
// shapes' geometry at every length --, the LDS behind the core's layout and R.  False: the LDS does not fit.
struct LinearListwiseShape { MetricShape sh; size_t extra; int R; };
inline bool linear_listwise_shape(int loss, MetricParams &m, int F, LinearListwiseShape &o)
{
    if (loss == LTR_LISTWISE_LISTNET && m.L > kSortRankMinLen) {
        const LaunchShape s = choose_shape(m.B, m.L);
        m.msplit = s.msplit;
        o.sh.threads = s.owners * s.msplit;
    } else {
        o.sh = metric_shape(m);
    }
    if (loss == LTR_LISTWISE_LISTNET) { o.sh.dpt = 0; o.sh.lds = linear_listwise_core_bytes(loss, m.L, false); }
    const int C = F / 4, T = o.sh.threads;
    const int CT = C < T ? C : T;
    int R = T / CT < kListwiseMaxR ? T / CT : kListwiseMaxR;
    const size_t fixed = o.sh.lds + 4 * (size_t)F;
    while (R > 1 && fixed + 16 * (size_t)R * CT > kLdsBudget) --R;
    o.R = R;
    o.extra = 4 * (size_t)F + 16 * (size_t)R * CT;
    return o.sh.lds + o.extra <= kLdsBudget;
}

inline bool bad_listwise_loss(int loss) { return loss != LTR_LISTWISE_LISTNET && loss != LTR_LISTWISE_LISTMLE; }

template <int LOSS>
int launch_linear_listwise(LinearListwiseParams &p, hipStream_t stream)
{
    LinearListwiseShape s;
    if (!linear_listwise_shape(LOSS, p.m, p.F, s)) return LTR_ERR_CONFIG;
    p.R = s.R;
    return launch_ranked(s.sh, p.m.B, s.extra, stream, p, [](auto D) {
        if constexpr (LOSS == kLossLambdaRank) return &linear_lambdarank_kernel<decltype(D)::value>;
        else return &linear_listwise_kernel<LOSS, (LOSS == LTR_LISTWISE_LISTNET ? 0 : decltype(D)::value)>;
    });
}

}  // namespace

extern "C" {

int ltr_linear_listwise_plan(int loss, int B, int L, int F)
{
    if (bad_listwise_loss(loss) || B <= 0 || L <= 0 || F <= 0 || L > kMaxListLen || F % 4 != 0) return 0;
    MetricParams m{};
    m.B = B; m.L = L;
    LinearListwiseShape s;
    return linear_listwise_shape(loss, m, F, s) ? 1 : 0;
}

int ltr_linear_listwise_partials_f32(int loss, int k, const float *X, const float *W, const float *bias,
                                     const void *rel, int rel_dtype, const int64_t *n, const int32_t *tie, int use_seed,
                                     uint64_t seed, const int64_t *seed_dev, int B, int L, int F, float *loss_out,
                                     float *scores_out, float *partials, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (bad_listwise_loss(loss) || bad_label_dtype(rel_dtype)) return LTR_ERR_KIND;
    if (B < 0 || L <= 0 || F <= 0) return LTR_ERR_SHAPE;
    if (L > kMaxListLen) return LTR_ERR_LIST_TOO_LONG;
    if (B == 0) return LTR_OK;
    if (!X || !W || !rel || !n || !loss_out || !partials) return LTR_ERR_NULL;
    if (!ltr_linear_listwise_plan(loss, B, L, F) || (uintptr_t)X % 16 != 0 || (uintptr_t)partials % 16 != 0)
        return LTR_ERR_CONFIG;
    if (const int st = status_peek()) return st;           // a kernel of an earlier call gave up
    LinearListwiseParams p{};
    p.m.rel = rel; p.m.n = n; p.m.B = B; p.m.L = L; p.m.rel_dtype = rel_dtype;
    p.X = X; p.W = W; p.bias = bias; p.loss = loss_out; p.scores_out = scores_out; p.part = partials;
    p.F = F; p.k = k;
    if (loss == LTR_LISTWISE_LISTNET) return launch_linear_listwise<LTR_LISTWISE_LISTNET>(p, (hipStream_t)stream);
    set_tie(p.m, tie, use_seed, seed, seed_dev);
    return launch_linear_listwise<LTR_LISTWISE_LISTMLE>(p, (hipStream_t)stream);
}

}  // extern "C"
