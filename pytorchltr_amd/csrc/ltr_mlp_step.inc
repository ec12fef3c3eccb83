// ltr_mlp_step.inc -- host side of the fused MLP training step: the layout choice, the slot dispatch, the slot-fit rule,
// ONE launch path (mlp_step_launch) and the C ABI entry points on it -- ltr_mlp_pairwise_f32 (include/ltr_hip.h),
// ltr_mlp_listwise_f32 (include/ltr_listwise.h), ltr_mlp_lambdarank_f32 (include/ltr_mlp_lambdarank.h); the fourth,
// ltr_mlp_train_step_f32, is in ltr_mlp_train.inc.  An entry point is its own guards in its documented order, the
// launch path, and its reduction (mlp_reduce_launch, ltr_mlp_reduce.inc; the trainer: mlp_reduce_update_launch).
// Needs the launchers of both kernels (ltr_mlp.inc, ltr_mlp2.inc).  No GPU code.  DESIGN.md 29.
#pragma once

// ltr_debug_mlp_layout(1) keeps the training step on the 8-wave kernel of ltr_mlp.inc (A/B measurements,
// tests of both kernels; the 4-wave tile kernel of ltr_mlp2.inc is the default where it applies)
inline int &mlp_layout_choice() { static int choice = 0; return choice; }

// auto (0): the tile kernel where the batch gives every CU its two workgroups (B >= 2 x CUs) or the
// lists are longer than the 8-wave kernel takes; below that the 8-wave kernel is 1.5-2 us faster
// (B = 64 .. 384 at the guide's network: 27.5 / 29.1 / 32.9 / 42.3 against 29.7 / 30.9 / 34.6 / 44.3 us;
// 512: 47.4 / 46.6, 768: 58.0 / 49.5).  1: 8-wave kernel wherever it applies, 2: tile kernel likewise.
inline bool mlp_use_tile_layout(int F, int B, int L)
{
    if (!mlp2_takes(F)) return false;
    if (L > kMlpMaxLen) return true;
    const int choice = mlp_layout_choice();
    if (choice == 1) return false;
    if (choice == 2) return true;
    return B >= 2 * device_cu_count();
}

// the feature widths the kernels take (16-byte rows, at most 14 tiles of 16 features), and the longest list at one
inline bool mlp_step_bad_width(int F) { return F <= 0 || (F & 3) || F > 16 * 14; }
inline int mlp_step_max_len(int F) { return mlp2_takes(F) ? kM2MaxLen : kMlpMaxLen; }

// B, L, the network and its limits as every launching entry point of this file checks them
inline bool mlp_step_bad_network(int B, int L, int F, int H1, int H2)
{
    return B < 0 || L <= 0 || H1 <= 0 || H2 <= 0 || mlp_step_bad_width(F) || H1 > kMlpH1 || H2 > kMlpH2;
}

inline bool bad_mlp_listwise_loss(int loss) { return loss != LTR_LISTWISE_LISTNET && loss != LTR_LISTWISE_LISTMLE; }
inline int mlp_listwise_slot_of(int loss) { return loss == LTR_LISTWISE_LISTNET ? LTR_MLP_LISTNET : LTR_MLP_LISTMLE; }

// The plan rule behind the shape checks: the list fits the layouts that take F, and the LDS of every layout the call
// may be steered to (ltr_debug_mlp_layout) -- the static part and the loss slot's row -- fits the workgroup.
// (`kind`: LTR_MLP_LISTNET, LTR_MLP_LISTMLE or LTR_MLP_LAMBDARANK)
inline bool mlp_slot_fits(int kind, int L, int F)
{
    if (L > mlp_step_max_len(F)) return false;
    if (mlp2_takes(F) &&
        mlp2_lds_bytes(kind, mlp_bucket(F), L <= kM2ParkLen ? kM2ParkLen : kM2MaxLen) > kLdsBudget / kM2Wgs)
        return false;
    if (L <= kMlpMaxLen && mlp_lds_bytes(kind, F) > kLdsBudget) return false;
    return true;
}

// the params of a launch without a loss: float labels at X (not used; any readable address for the prefetch); the rest is the caller's
inline MlpParams mlp_step_params(const float *X, const float *W1, const float *b1, const float *W2, const float *b2,
                                 const float *W3, const float *b3, const int64_t *n, int B, int L, int F, int H1, int H2)
{
    MlpParams p;
    p.X = X; p.W1 = W1; p.b1 = b1; p.W2 = W2; p.b2 = b2; p.W3 = W3; p.b3 = b3;
    p.rel = X; p.n = n; p.grad_out = nullptr;
    p.loss = nullptr; p.scores_out = nullptr; p.part = nullptr;
    p.B = B; p.L = L; p.F = F; p.H1 = H1; p.H2 = H2;
    p.sigma = 1.0f; p.rel_dtype = LTR_LABEL_F32; p.P = mlp_param_count(F, H1, H2); p.pitch = mlp_pitch(p.P); p.fwd_only = 0;
    return p;
}

// The loss slot of a step as a template argument, with_kind (ltr_common.inc) over the kernels' whole KIND range: the
// seven pairwise kinds and the three row slots.
template <class Fn>
int with_mlp_slot(int slot, Fn &&f)
{
    switch (slot) {
    case LTR_MLP_LISTNET: return f(std::integral_constant<int, LTR_MLP_LISTNET>{});
    case LTR_MLP_LISTMLE: return f(std::integral_constant<int, LTR_MLP_LISTMLE>{});
    case LTR_MLP_LAMBDARANK: return f(std::integral_constant<int, LTR_MLP_LAMBDARANK>{});
    default: return with_kind(slot, f);
    }
}

// One step call, as every entry point describes it once its own guards have passed (B > 0, pointers checked).
struct MlpStepCall {
    int slot;                      // the kernels' KIND: LTR_HINGE .. LTR_NDCG2, LTR_MLP_LISTNET / LISTMLE / LAMBDARANK
    float sigma;                   // the pairwise kinds and LambdaRank (the listwise slots run at 1)
    int k;                         // ListMLE, LambdaRank
    const int32_t *tie;            // ListMLE: the tie arguments of include/ltr_listwise.h (ListNet ranks nothing)
    int use_seed;
    uint64_t seed;
    const int64_t *seed_dev;
    const float *X, *W1, *b1, *W2, *b2, *W3, *b3;
    const void *rel;
    int rel_dtype;
    const int64_t *n;
    const float *grad_out;
    int B, L, F, H1, H2;
    float *loss, *scores_out;
    void *workspace;               // one partial vector per workgroup of the launch
    size_t workspace_bytes;
};

// From the validated arguments to the MFMA launch: the layout and its grid (returned in `grid` for the caller's
// reduction), LTR_ERR_WORKSPACE, LTR_ERR_CONFIG for a row slot that does not fit, MlpParams, the kernel of the slot.
inline int mlp_step_launch(const MlpStepCall &c, int &grid, hipStream_t s)
{
    const bool row_slot = c.slot > LTR_NDCG2;
    const bool tile = mlp_use_tile_layout(c.F, c.B, c.L);
    grid = tile ? mlp2_grid(c.B) : mlp_grid(c.B);
    const int P = mlp_param_count(c.F, c.H1, c.H2);
    if (!c.workspace || c.workspace_bytes < (size_t)grid * mlp_pitch(P) * sizeof(float)) return LTR_ERR_WORKSPACE;
    if (row_slot && !mlp_slot_fits(c.slot, c.L, c.F)) return LTR_ERR_CONFIG;
    MlpParams p = mlp_step_params(c.X, c.W1, c.b1, c.W2, c.b2, c.W3, c.b3, c.n, c.B, c.L, c.F, c.H1, c.H2);
    p.rel = c.rel; p.rel_dtype = c.rel_dtype; p.grad_out = c.grad_out;
    p.loss = c.loss; p.scores_out = c.scores_out; p.part = (float *)c.workspace;
    if (c.slot != LTR_MLP_LISTNET && c.slot != LTR_MLP_LISTMLE) p.sigma = c.sigma;
    if (row_slot) p.lw.k = c.k;
    if (c.slot == LTR_MLP_LISTMLE) {              // (ListNet ranks nothing: the tie arguments are ignored)
        if (c.use_seed) { p.lw.use_seed = 1; p.lw.tie_seed = c.seed; p.lw.tie_seed_dev = c.seed_dev; }
        else p.lw.tie = c.tie;
    }
    return with_mlp_slot(c.slot, [&](auto K) {
        return tile ? launch_mlp2_kind<K>(p, grid, s) : launch_mlp_kind<K>(p, grid, s);
    });
}

extern "C" {

LTR_DEBUG_HOOK void ltr_debug_mlp_layout(int layout) { mlp_layout_choice() = layout; }

int ltr_mlp_max_list_len(int F)
{
    return mlp_step_bad_width(F) ? 0 : mlp_step_max_len(F);
}

size_t ltr_mlp_param_count(int F, int H1, int H2)
{
    if (F <= 0 || H1 <= 0 || H2 <= 0) return 0;
    return (size_t)mlp_param_count(F, H1, H2);
}

size_t ltr_mlp_workspace_bytes(int B, int F, int H1, int H2)
{
    if (B <= 0 || F <= 0 || H1 <= 0 || H2 <= 0) return 0;
    // (the larger of the two layouts' grids)
    return (size_t)mlp2_grid(B) * (size_t)mlp_pitch(mlp_param_count(F, H1, H2)) * sizeof(float);
}

// (SHAPE and LIST_TOO_LONG ahead of KIND; the parameter pointers even at B == 0, where the reduction still runs:
// grads is zeroed and loss_sum written)
int ltr_mlp_pairwise_f32(int kind, float sigma, const float *X, const float *W1, const float *b1,
                         const float *W2, const float *b2, const float *W3, const float *b3,
                         const void *rel, int rel_dtype, const int64_t *n, const float *grad_out,
                         int B, int L, int F, int H1, int H2, float *loss, float *scores_out,
                         float *grads, float *loss_sum, void *workspace, size_t workspace_bytes,
                         void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (mlp_step_bad_network(B, L, F, H1, H2)) return LTR_ERR_SHAPE;
    if (L > mlp_step_max_len(F)) return LTR_ERR_LIST_TOO_LONG;
    if (kind < LTR_HINGE || kind > LTR_NDCG2) return LTR_ERR_KIND;
    if (rel_dtype < LTR_LABEL_I64 || rel_dtype > LTR_LABEL_I32) return LTR_ERR_KIND;
    if (!W1 || !b1 || !W2 || !b2 || !W3 || !b3 || !grads) return LTR_ERR_NULL;
    if (B > 0 && (!X || !rel || !n || !loss)) return LTR_ERR_NULL;
    hipStream_t s = (hipStream_t)stream;
    int grid = 0;
    if (B > 0) {
        const MlpStepCall call{kind, sigma, 0, nullptr, 0, 0, nullptr, X, W1, b1, W2, b2, W3, b3, rel, rel_dtype, n,
                               grad_out, B, L, F, H1, H2, loss, scores_out, workspace, workspace_bytes};
        const int rc = mlp_step_launch(call, grid, s);
        if (rc != 0) return rc;
    }
    return mlp_reduce_launch(workspace, grid, mlp_param_count(F, H1, H2), grads, loss, B, loss_sum, s);
}

// ---- the listwise step (include/ltr_listwise.h; DESIGN.md 17) ----
int ltr_mlp_listwise_plan(int loss, int B, int L, int F, int H1, int H2)
{
    if (bad_mlp_listwise_loss(loss) || B == 0 || mlp_step_bad_network(B, L, F, H1, H2)) return 0;
    return mlp_slot_fits(mlp_listwise_slot_of(loss), L, F) ? 1 : 0;
}

int ltr_mlp_listwise_f32(int loss, int k, const float *X, const float *W1, const float *b1, const float *W2,
                         const float *b2, const float *W3, const float *b3, const void *rel, int rel_dtype,
                         const int64_t *n, const int32_t *tie, int use_seed, uint64_t seed, const int64_t *seed_dev,
                         const float *grad_out, int B, int L, int F, int H1, int H2, float *loss_out, float *scores_out,
                         float *grads, float *loss_sum, void *workspace, size_t workspace_bytes, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (bad_mlp_listwise_loss(loss) || bad_label_dtype(rel_dtype)) return LTR_ERR_KIND;
    if (mlp_step_bad_network(B, L, F, H1, H2)) return LTR_ERR_SHAPE;
    if (L > mlp_step_max_len(F)) return LTR_ERR_LIST_TOO_LONG;
    if (B == 0) return LTR_OK;
    if (!X || !W1 || !b1 || !W2 || !b2 || !W3 || !b3 || !rel || !n || !loss_out || !grads) return LTR_ERR_NULL;
    const MlpStepCall call{mlp_listwise_slot_of(loss), 1.0f, k, tie, use_seed, seed, seed_dev, X, W1, b1, W2, b2, W3, b3,
                           rel, rel_dtype, n, grad_out, B, L, F, H1, H2, loss_out, scores_out, workspace, workspace_bytes};
    hipStream_t s = (hipStream_t)stream;
    int grid;
    const int rc = mlp_step_launch(call, grid, s);
    if (rc != 0) return rc;
    return mlp_reduce_launch(workspace, grid, mlp_param_count(F, H1, H2), grads, loss_out, B, loss_sum, s);
}

// ---- the LambdaRank step (include/ltr_mlp_lambdarank.h; DESIGN.md 27) ----
int ltr_mlp_lambdarank_plan(int B, int L, int F, int H1, int H2)
{
    if (B == 0 || mlp_step_bad_network(B, L, F, H1, H2)) return 0;
    return mlp_slot_fits(LTR_MLP_LAMBDARANK, L, F) ? 1 : 0;
}

int ltr_mlp_lambdarank_f32(int k, float sigma, const float *X, const float *W1, const float *b1, const float *W2,
                           const float *b2, const float *W3, const float *b3, const void *rel, int rel_dtype,
                           const int64_t *n, const float *grad_out, int B, int L, int F, int H1, int H2, float *loss_out,
                           float *scores_out, float *grads, float *loss_sum, void *workspace, size_t workspace_bytes,
                           void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (bad_label_dtype(rel_dtype)) return LTR_ERR_KIND;
    // (sigma: the guard of ltr_lambdarank_f32, check_lambdarank in ltr_lambdarank.inc)
    if (mlp_step_bad_network(B, L, F, H1, H2) || !std::isfinite(sigma)) return LTR_ERR_SHAPE;
    if (L > mlp_step_max_len(F)) return LTR_ERR_LIST_TOO_LONG;
    if (B == 0) return LTR_OK;
    if (!X || !W1 || !b1 || !W2 || !b2 || !W3 || !b3 || !rel || !n || !loss_out || !grads) return LTR_ERR_NULL;
    const MlpStepCall call{LTR_MLP_LAMBDARANK, sigma, k, nullptr, 0, 0, nullptr, X, W1, b1, W2, b2, W3, b3,
                           rel, rel_dtype, n, grad_out, B, L, F, H1, H2, loss_out, scores_out, workspace, workspace_bytes};
    hipStream_t s = (hipStream_t)stream;
    int grid;
    const int rc = mlp_step_launch(call, grid, s);
    if (rc != 0) return rc;
    return mlp_reduce_launch(workspace, grid, mlp_param_count(F, H1, H2), grads, loss_out, B, loss_sum, s);
}

// bench.py `extra.mlp_scorer_fused.launch_ceiling` (include/ltr_hip.h): the launch geometry of the fused MLP training
// step on the tile layout -- fills, image, barriers, MFMA streams -- with nothing else (mlp_tile_kernel<..., PROBE>)
LTR_DEBUG_HOOK int ltr_debug_mlp_probe_f32(const float *X, const float *W1, const float *b1, const float *W2, const float *b2,
                            const float *W3, const float *b3, const int64_t *n, int B, int L, int F, int H1, int H2,
                            float *out, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (B <= 0 || L <= 0 || L > kM2ParkLen || F != 136 || H1 <= 0 || H2 <= 0 || H1 > kMlpH1 || H2 > kMlpH2) return LTR_ERR_SHAPE;
    if (!X || !W1 || !b1 || !W2 || !b2 || !W3 || !b3 || !n || !out) return LTR_ERR_NULL;
    MlpParams p = mlp_step_params(X, W1, b1, W2, b2, W3, b3, n, B, L, F, H1, H2);
    p.loss = out;
    const size_t lds = mlp2_lds_bytes(LTR_HINGE, 9, kM2ParkLen);
    LTR_ENSURE_LDS((mlp_tile_kernel<LTR_HINGE, 9, 34, kM2ParkLen, false, true>), lds);
    hipLaunchKernelGGL((mlp_tile_kernel<LTR_HINGE, 9, 34, kM2ParkLen, false, true>), dim3((unsigned)mlp2_grid(B)), dim3(kM2Threads), lds,
                       (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

int ltr_mlp_scores_f32(const float *X, const float *W1, const float *b1, const float *W2,
                       const float *b2, const float *W3, const float *b3, const int64_t *n, int B,
                       int L, int F, int H1, int H2, float *scores_out, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (mlp_step_bad_network(B, L, F, H1, H2)) return LTR_ERR_SHAPE;
    const bool tile_scores = L > kMlpMaxLen && mlp2_takes(F);       // 129 .. 256 documents: the tile kernel
    if (L > (tile_scores ? kM2MaxLen : kMlpMaxLen)) return LTR_ERR_LIST_TOO_LONG;
    if (!W1 || !b1 || !W2 || !b2 || !W3 || !b3) return LTR_ERR_NULL;
    if (B == 0) return LTR_OK;
    if (!X || !n || !scores_out) return LTR_ERR_NULL;
    MlpParams p = mlp_step_params(X, W1, b1, W2, b2, W3, b3, n, B, L, F, H1, H2);
    p.scores_out = scores_out; p.fwd_only = 1;
    if (tile_scores) return launch_mlp2_scores(p, mlp2_grid(B), (hipStream_t)stream);
    return launch_mlp_scores(p, mlp_grid(B), (hipStream_t)stream);
}

}  // extern "C"
