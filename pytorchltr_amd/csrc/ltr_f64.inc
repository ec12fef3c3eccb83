// ltr_f64.inc -- double-precision instantiation of the seven losses (included by
// ltr_kernels.hip).  The reference computes in the dtype of `scores`: fp64 in -> fp64 out
// (measured, SURVEY.md 8 a-5), which is what `torch.autograd.gradcheck` users rely on.  This is
// the straightforward both-ends pass in double -- correctness first: gfx950 runs fp64 VALU at
// half rate and v_exp/v_log have no f64 form, so it is several times slower than the fp32
// kernels and is not on the benchmarked path.

namespace {

__device__ __forceinline__ double block_sum_f64(double v, double *red)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    const int nw = blockDim.x >> 6;
    if (nw == 1) return v;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < nw; ++i) t += red[i];
    return t;
}

struct LossParams64 {
    const double *scores;
    const void *rel;
    const int64_t *n;
    double *loss;
    double *dscores;
    int B, L;
    double sigma;
    int rel_dtype;
};

// LDS: s, y, aux (a_k or G_k), gout double[L] each; delta double[L+2]; red double[32]; rank int[L]
__host__ __device__ inline size_t loss64_lds_bytes(int L)
{
    const size_t Lp = (size_t)((L + 1) & ~1);
    return 8 * Lp * 4 + 4 * Lp + 8 * (Lp + 2) + 8 * 32;
}

template <int KIND>
__global__ void __launch_bounds__(256)
pairwise_loss_f64_kernel(LossParams64 p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = blockIdx.x;
    const int L = p.L;
    const int Lp = (L + 1) & ~1;
    const int tid = threadIdx.x;
    const int T = blockDim.x;
    const int nb = clamp_n(p.n[b], L);
    double *s = reinterpret_cast<double *>(smem);
    double *y = s + Lp;
    double *aux = y + Lp;
    double *gout = aux + Lp;
    double *delta = gout + Lp;
    double *red = delta + Lp + 2;
    int *rank = reinterpret_cast<int *>(red + 32);
    const size_t row = (size_t)b * L;
    for (int m = tid; m < nb; m += T) {
        s[m] = p.scores[row + m];
        y[m] = (p.rel_dtype == LTR_LABEL_I64) ? (double)((const int64_t *)p.rel)[row + m]
             : (p.rel_dtype == LTR_LABEL_F32) ? (double)((const float *)p.rel)[row + m]
                                              : (double)((const int32_t *)p.rel)[row + m];
    }
    __syncthreads();
    constexpr double kLn2d = 0.6931471805599453094;

    if (KIND == LTR_NDCG1 || KIND == LTR_NDCG2) {
        // ranks by score and by label (counting), maxDCG, gains -- loss/pairwise_lambda.py:221-241
        double part = 0.0;
        for (int k = tid; k < nb; k += T) {
            int rs = 0, ry = 0;
            const double sk = s[k], yk = y[k];
            for (int m = 0; m < nb; ++m) {
                rs += (s[m] > sk) | ((s[m] == sk) & (m < k));
                ry += (y[m] > yk) | ((y[m] == yk) & (m < k));
            }
            rank[k] = rs;
            part += (exp2(yk) - 1.0) / log2(2.0 + (double)ry);
        }
        double maxdcg = block_sum_f64(part, red);
        if (maxdcg == 0.0) maxdcg = 1.0;
        for (int k = tid; k < nb; k += T) {
            const double G = (exp2(y[k]) - 1.0) / maxdcg;
            aux[k] = (KIND == LTR_NDCG1) ? G / log2(2.0 + (double)rank[k]) : G;
        }
        if (KIND == LTR_NDCG2)
            for (int d = tid; d < nb; d += T)
                delta[d] = fabs(1.0 / log2(2.0 + (double)d) - 1.0 / log2(3.0 + (double)d));
        __syncthreads();
    } else if (KIND == LTR_ARP1) {
        for (int k = tid; k < nb; k += T) aux[k] = y[k];
        __syncthreads();
    }

    // both-ends pass: thread owns document k, streams every m < nb
    double lacc = 0.0;
    const double sig = p.sigma;
    for (int k = tid; k < nb; k += T) {
        const double sk = s[k], yk = y[k];
        double g = 0.0;
        for (int m = 0; m < nb; ++m) {
            const double d = sk - s[m];
            if (KIND == LTR_HINGE || KIND == LTR_DCG_HINGE) {
                if (yk > y[m]) { const double u = 1.0 - d; if (u >= 0.0) { lacc += u; g -= 1.0; } }
                else if (yk < y[m]) { const double u = 1.0 + d; if (u >= 0.0) g += 1.0; }
            } else if (KIND == LTR_ARP1 || KIND == LTR_NDCG1) {
                const double x = sig * d;
                const double e = exp(-fabs(x));
                const double sneg = (x >= 0.0) ? e / (1.0 + e) : 1.0 / (1.0 + e);
                lacc += aux[k] * (log1p(e) + fmax(-x, 0.0)) / kLn2d;
                g += aux[m] - (aux[k] + aux[m]) * sneg;
            } else {
                const bool gt = yk > y[m], lt = yk < y[m];
                if (!(gt | lt)) continue;
                double W = 1.0;
                if (KIND == LTR_ARP2) W = fabs(yk - y[m]);
                if (KIND == LTR_NDCG2) W = delta[abs(rank[k] - rank[m])] * fabs(aux[k] - aux[m]);
                const double z = gt ? sig * d : -sig * d;
                const double e = exp(-fabs(z));
                const double psi = (z >= 0.0) ? e / (1.0 + e) : 1.0 / (1.0 + e);
                if (gt) lacc += W * (log1p(e) + fmax(-z, 0.0)) / kLn2d;
                g += (gt ? -W : W) * psi;
            }
        }
        gout[k] = g;
    }
    __syncthreads();
    double total = block_sum_f64(lacc, red);
    double gscale = 1.0;
    if (KIND == LTR_DCG_HINGE) {
        const double lg = log(2.0 + total);
        gscale = 1.0 / ((2.0 + total) * lg * lg);
        total = -1.0 / lg;
    } else if (KIND != LTR_HINGE) {
        gscale = sig / kLn2d;
    }
    if (tid == 0) p.loss[b] = total;
    if (p.dscores != nullptr)
        for (int k = tid; k < L; k += T) p.dscores[row + k] = (k < nb) ? gout[k] * gscale : 0.0;
}

__global__ void scale_rows_f64_kernel(const double *__restrict__ ds, const double *__restrict__ go,
                                      size_t total, int L, double *__restrict__ out)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride)
        out[i] = ds[i] * go[i / (size_t)L];
}

template <int KIND>
int launch_loss64(const LossParams64 &p, hipStream_t stream)
{
    const size_t lds = loss64_lds_bytes(p.L);
    LTR_ENSURE_LDS((pairwise_loss_f64_kernel<KIND>), lds);
    hipLaunchKernelGGL((pairwise_loss_f64_kernel<KIND>), dim3((unsigned)p.B), dim3(256), lds, stream, p);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int ltr_max_list_len_f64(void)
{
    LTR_CLEAR_STALE_ERROR();
    int L = kMaxListLen;
    while (L > 1 && loss64_lds_bytes(L) > kLdsBudget) --L;
    return L;
}

int ltr_pairwise_loss_f64(int kind, double sigma, const double *scores, const void *rel,
                          int rel_dtype, const int64_t *n, int B, int L, double *loss,
                          double *dscores, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (const int rc = check_kind(kind, rel_dtype)) return rc;
    if (B < 0 || L <= 0) return LTR_ERR_SHAPE;
    if (L > kMaxListLen || loss64_lds_bytes(L) > kLdsBudget) return LTR_ERR_LIST_TOO_LONG;
    if (B == 0) return LTR_OK;
    if (!scores || !rel || !n || !loss) return LTR_ERR_NULL;
    LossParams64 p;
    p.scores = scores; p.rel = rel; p.n = n; p.loss = loss; p.dscores = dscores;
    p.B = B; p.L = L; p.sigma = sigma; p.rel_dtype = rel_dtype;
    return with_kind(kind, [&](auto K) { return launch_loss64<K>(p, (hipStream_t)stream); });
}

int ltr_scale_rows_f64(const double *dscores, const double *grad_out, int B, int L, double *out,
                       void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (B < 0 || L <= 0) return LTR_ERR_SHAPE;
    if (B == 0) return LTR_OK;
    if (!dscores || !grad_out || !out) return LTR_ERR_NULL;
    const size_t total = (size_t)B * L;
    hipLaunchKernelGGL(scale_rows_f64_kernel, dim3(grid_for(total, 256)), dim3(256), 0,
                       (hipStream_t)stream, dscores, grad_out, total, L, out);
    return (int)hipGetLastError();
}

}  // extern "C"
