// ltr_lambdarank_row.inc -- the LambdaRank (NDCG@k swap weights) row of one staged query on the ranked-row core's LDS
// layout (ltr_ranked.inc), which is all it needs in front of it.  Included by ltr_linear_listwise.inc (the loss slot of
// the fused Linear step) and, through it, by ltr_lambdarank.inc (lambdarank_kernel); and by ltr_mlp.hip (the loss slot
// of the fused MLP step, mlp_lambdarank_slot in ltr_mlp_listwise.inc).  The loss, the passes and their orders are
// described at the top of ltr_lambdarank.inc.
#pragma once

namespace {

// One pair seen from its `own` document against a `vis`iting one, both as (score, label, G, d): the gradient of the own
// document in units of sigma / ln 2 into g, and, `count`, the pair's loss into l.  The weight is
// |G_own - G_vis| |d_own - d_vis|; the labels orient the pair (equal labels: no pair -- selects, no 0 * x).  Stable
// softplus: e = exp2(-|z|) <= 1 with z = sigma log2(e) (s_win - s_lose).
__device__ __forceinline__ void lambdarank_pair(float2 own, float2 own_gd, float2 vis, float2 vis_gd, float c1, bool count,
                                                float &g, float &l)
{
    const bool gt = own.y > vis.y, lt = own.y < vis.y;
    const float t = (own.x - vis.x) * c1;
    const float z = gt ? t : -t;
    const float e = __builtin_amdgcn_exp2f(-fabsf(z));
    const float u = 1.0f + e;
    const float r = __builtin_amdgcn_rcpf(u);
    const float psi = (z >= 0.0f) ? e * r : r;                         // sigmoid(-sigma (s_win - s_lose))
    const float lg = log2_1p_comp(e, u, r) + fmaxf(-z, 0.0f);          // log2(1 + exp(-sigma (s_win - s_lose)))
    const float W = fabsf(own_gd.x - vis_gd.x) * fabsf(own_gd.y - vis_gd.y);
    const bool on = gt | lt;
    l += (count & on) ? W * lg : 0.0f;
    g += on ? (gt ? -W : W) * psi : 0.0f;
}

// The LambdaRank row of one staged query: q.sy holds the (score, label) pairs of the first nb documents.  Ranks by
// score and by label (ties by the tie words of m: lambdarank_kernel and the fused step leave them at document-index
// order), stores the loss at the cutoff K to *loss and, `grad`, leaves d loss / d score BY RANK in the rank_y slot,
// published: document j's is reinterpret_cast<float *>(q.rank_y)[q.rank_s[j]].  No LDS beyond the core's layout: once
// the ranks are taken the work region holds (score, label) by rank, sy is overwritten by (G, d) by rank and rank_y by
// the gradient.  Contains barriers: call from uniform code.
template <int DPT>
__device__ __forceinline__ void lambdarank_row(const MetricParams &m, const RankedRowLds &q, int nb, int K, float sigma,
                                               float *loss, bool grad)
{
    const int L4 = (m.L + 3) & ~3;
    const int tid = row_tid();
    const int T = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, nwaves = T >> 6;
    int *rank_s = q.rank_s;
    float2 *sr = reinterpret_cast<float2 *>(q.curve);                  // (score, label) by rank (curve | icurve)
    float2 *gd = q.sy;                                                 // (G, d) by rank, over sy once it is read
    float *gr = reinterpret_cast<float *>(q.rank_y);                   // the gradient by rank (rank_y's slot)

    for (int j = tid; j < 2 * L4; j += T) rank_s[j] = 0;               // (rank_s | rank_y)
    __syncthreads();
    metric_ranks<DPT>(m, q, nb, true);
    __syncthreads();

    // maxDCG at K over the ideal ranking; 0 -> 1
    float part = 0.f;
    for (int j = tid; j < nb; j += T) {
        const int ry = q.rank_y[j];
        if (ry < K) part = __builtin_fmaf(ndcg_gain(q.sy[j].y), inv_discount((float)ry), part);
    }
    float maxdcg = block_sum(part, q.red);
    if (maxdcg == 0.0f) maxdcg = 1.0f;
    const float inv_maxdcg = 1.0f / maxdcg;

    for (int j = tid; j < nb; j += T) sr[rank_s[j]] = q.sy[j];
    __syncthreads();
    for (int r = tid; r < nb; r += T)
        gd[r] = make_float2(ndcg_gain(sr[r].y) * inv_maxdcg, r < K ? inv_discount((float)r) : 0.f);
    __syncthreads();

    // pass A: rank r against the anchors a < K -- all of a document's pairs below the cutoff, the pairs within the top K
    // of one above it; a pair's loss is counted by its lower member (a < r)
    const float c1 = sigma * kLog2e;                                   // sigma / ln 2: the gradient's unit as well
    const bool tail = K < nb;
    float lacc = 0.f;
    for (int r = tid; r < nb; r += T) {
        const float2 own = sr[r], own_gd = gd[r];
        float g = 0.f;
        for (int a = 0; a < K; ++a) lambdarank_pair(own, own_gd, sr[a], gd[a], c1, a < r, g, lacc);
        if (grad) gr[r] = (tail && r < K) ? g : g * c1;
    }
    lacc = block_sum(lacc, q.red);
    if (tid == 0) *loss = lacc;
    if (!grad) return;
    __syncthreads();

    // pass B: the anchors' pairs with the ranks below the cutoff, one wave per anchor (evaluated a second time: no
    // scatter across threads, a fixed order)
    if (tail) {
        for (int a = wave; a < K; a += nwaves) {
            const float2 own = sr[a], own_gd = gd[a];
            float g = 0.f, unused = 0.f;
            for (int r = K + lane; r < nb; r += 64) lambdarank_pair(own, own_gd, sr[r], gd[r], c1, false, g, unused);
            g = wave_sum(g);
            if (lane == 0) gr[a] = (gr[a] + g) * c1;
        }
        __syncthreads();
    }
}

}  // namespace
