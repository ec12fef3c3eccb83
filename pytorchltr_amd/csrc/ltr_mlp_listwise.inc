// ltr_mlp_listwise.inc -- the listwise loss slot of the fused MLP training step (included by ltr_mlp.hip, in front of
// both kernels; C ABI: ltr_mlp_listwise_f32, include/ltr_listwise.h; DESIGN.md 17).
//
// Both MLP kernels (mlp_tile_kernel, ltr_mlp2.inc; mlp_pairwise_kernel, ltr_mlp.inc) have one loss slot between the
// forward and the backward chain: the whole query's scores and labels sit in LDS, and the slot leaves
// d loss[b] / d s_j * weight per document in gfin[] (0 for the padded slots up to the list-length class) and writes
// loss[b].  For KIND = LTR_MLP_LISTNET / LTR_MLP_LISTMLE the slot is mlp_listwise_slot below instead of the pair pass:
//   ListMLE  listmle_row (ltr_listmle_row.inc), the row function of listmle_kernel and of the fused Linear step, on the
//            ranked-row layout (ranked_row_lds) carved where the pairwise kinds keep their QueryLds; the ranking is the
//            counting rank (DPT = 1) with the workgroup cut into owners x slices by the query's own length;
//   ListNet  workgroup-wide max / sum of the scores and the labels (phase 2 of linear_listwise_kernel).
// KIND = LTR_MLP_LAMBDARANK (C ABI: ltr_mlp_lambdarank_f32, include/ltr_mlp_lambdarank.h; DESIGN.md 27) takes
// mlp_lambdarank_slot: lambdarank_row (ltr_lambdarank_row.inc) on the same layout and workgroup cut as ListMLE.
// The forward chain stages (label, score) pairs -- sy[j].x the label, sy[j].y the score -- where the pairwise kinds
// and LambdaRank stage (score, label): that is the order the row functions read.  The row functions synchronise with __syncthreads();
// the slot's own last barrier is the caller's lds_barrier().  No atomics on floats, every sum in a fixed order.
#pragma once

// the tie mode and ListMLE's k of a call, next to MlpParams (ltr_mlp.inc)
struct MlpListwiseArgs {
    const int32_t *tie;
    const int64_t *tie_seed_dev;
    unsigned long long tie_seed;
    int use_seed;
    int k;                           // ListMLE: <= 0 every factor; LambdaRank: <= 0 no cutoff
};

// the slot carves ranked_row_lds where loss_lds_bytes reserved room for it
static_assert(ranked_row_layout(128, false).end == loss_lds_bytes(LTR_MLP_LISTMLE, 128, 4) &&
              ranked_row_layout(256, false).end == loss_lds_bytes(LTR_MLP_LISTMLE, 256, 4),
              "loss_lds_bytes(LTR_MLP_LISTMLE) is the ranked-row layout of the counting rank");
static_assert(ranked_row_layout(128, false).end == loss_lds_bytes(LTR_MLP_LAMBDARANK, 128, 4) &&
              ranked_row_layout(256, false).end == loss_lds_bytes(LTR_MLP_LAMBDARANK, 256, 4),
              "loss_lds_bytes(LTR_MLP_LAMBDARANK) is the ranked-row layout of the counting rank");

struct MlpOpMax { static constexpr float id = -INFINITY; static __device__ __forceinline__ float f(float a, float b) { return fmaxf(a, b); } };

// T: threads of the workgroup (= blockDim.x); LT: list-length class (gfin[0 .. LT) is written); qbase: the query's LDS
// block (sy first); nb <= LT documents staged as (label, score); weight = grad_out[b] or 1 / B.
// Contains barriers: call from uniform code, behind the barrier that publishes sy; the caller's barrier publishes gfin.
template <int KIND, int T, int LT>
__device__ __forceinline__ void mlp_listwise_slot(unsigned char *qbase, const MlpListwiseArgs &a, int nb, float weight,
                                                  float *loss, float *gfin)
{
    const int tid = row_tid();
    if constexpr (KIND == LTR_MLP_LISTMLE) {
        const RankedRowLds r = ranked_row_lds(qbase, LT, false);
        MetricParams m{};
        m.L = LT;                                   // the layout's length: the tie words depend on the position only
        m.tie = a.tie; m.use_seed = a.use_seed; m.tie_seed = a.tie_seed; m.tie_seed_dev = a.tie_seed_dev;
        // counting rank: `owners` threads take one document each against 1 / msplit of the list
        const int owners = nb <= 64 ? 64 : (nb <= 128 ? 128 : 256);
        m.msplit = T / (owners < T ? owners : T);
        const int K = a.k > 0 ? min(a.k, nb) : nb;
        listmle_row<1>(m, r, nb, K, loss, true);
        for (int j = tid; j < LT; j += T) gfin[j] = j < nb ? r.curve[r.rank_s[j]] * weight : 0.f;
    } else {
        const float2 *sy = reinterpret_cast<const float2 *>(qbase);
        float *red = reinterpret_cast<float *>(qbase + 8 * (size_t)((LT + 3) & ~3));
        float ms = -INFINITY, my = -INFINITY;
        for (int j = tid; j < nb; j += T) {
            const float2 v = sy[j];
            my = fmaxf(my, v.x);
            ms = fmaxf(ms, v.y);
        }
        ms = block_reduce<MlpOpMax>(ms, red);
        my = block_reduce<MlpOpMax>(my, red);
        float zs = 0.f, zy = 0.f, dot = 0.f;
        for (int j = tid; j < nb; j += T) {
            const float2 v = sy[j];
            const float ds = v.y - ms;
            const float ey = expf(v.x - my);
            zs += expf(ds);
            zy += ey;
            dot += ey * ds;
        }
        block_sum2(zs, zy, red);
        dot = block_sum(dot, red);
        const float inv_zs = nb > 0 ? 1.0f / zs : 0.f;
        const float inv_zy = nb > 0 ? 1.0f / zy : 0.f;
        for (int j = tid; j < LT; j += T) {
            float gj = 0.f;
            if (j < nb) {
                const float2 v = sy[j];
                gj = (expf(v.y - ms) * inv_zs - expf(v.x - my) * inv_zy) * weight;
            }
            gfin[j] = gj;
        }
        if (tid == 0) *loss = nb > 0 ? (logf(zs) - dot * inv_zy) : 0.f;
    }
}

// The slot of KIND = LTR_MLP_LAMBDARANK (ltr_mlp_lambdarank_f32; DESIGN.md 27): lambdarank_row, the row function of
// lambdarank_kernel and of the fused Linear step, on the same ranked-row layout and with the same owners x slices cut
// as ListMLE above.  nb <= LT documents staged as (score, label); ties in document-index order (no tie words); k <= 0:
// no cutoff.  The row leaves the gradient by rank, in units of the loss, in the rank_y slot.  Same barrier contract.
template <int T, int LT>
__device__ __forceinline__ void mlp_lambdarank_slot(unsigned char *qbase, int k, float sigma, int nb, float weight,
                                                    float *loss, float *gfin)
{
    const int tid = row_tid();
    const RankedRowLds r = ranked_row_lds(qbase, LT, false);
    MetricParams m{};
    m.L = LT;
    const int owners = nb <= 64 ? 64 : (nb <= 128 ? 128 : 256);
    m.msplit = T / (owners < T ? owners : T);
    const int K = k > 0 ? min(k, nb) : nb;
    lambdarank_row<1>(m, r, nb, K, sigma, loss, true);
    const float *gr = reinterpret_cast<const float *>(r.rank_y);
    for (int j = tid; j < LT; j += T) gfin[j] = j < nb ? gr[r.rank_s[j]] * weight : 0.f;
}
