// ltr_linear_step.inc -- the host side of the fused Linear step: the planner (which kernel family runs a shape), the launch of
// the per-query partials, the reduce entry points and the steps in one call (ltr_linear_pairwise_f32, ltr_linear_step_f32,
// ltr_linear_sgd_step_f32), with the debug hooks that belong to them.  No kernels.  Needs the launchers and shape choosers of
// ltr_linear.inc, ltr_cluster.inc and ltr_parts.inc, LtrOverlap and the bucket (ltr_overlap.inc), mailbox_launch
// (ltr_mailbox.inc).  LazyRequest and set_pending_update stand here, not in ltr_linear_lazy.inc: linear_partials_launch reads them.
namespace {
inline size_t linear_partials_bytes(int B, int F)
{
    // (B, partial_pitch(F)) partials, rounded up, plus -- batches the split reduction takes: launch_linear_reduce -- its scratch
    // rows, plus a reserved 256-byte tail
    const size_t PF = (size_t)partial_pitch(F);
    const size_t split = (B >= kReduceSplitMin && PF / 4 <= 256) ? (size_t)kReduceMaxSplit * (size_t)reduce_scratch_pitch((int)PF) * sizeof(float) : 0;
    return ((((size_t)B * PF * sizeof(float)) + 255) & ~(size_t)255) + split + 256;
}

// The argument checks every step entry point makes: a shape no step runs (LTR_ERR_SHAPE), a workspace that cannot hold a
// batch of B queries (LTR_ERR_WORKSPACE; an empty batch needs none)
inline bool step_shape_bad(int B, int L, int F) { return B < 0 || L <= 0 || F <= 0; }
inline bool step_workspace_short(int B, int L, int F, const void *ws, size_t bytes) { return B > 0 && (!ws || bytes < ltr_linear_workspace_bytes(B, L, F)); }

// The cluster kernel takes the shapes it covers first (small batches of lists the symmetric pass takes: measured
// faster than the parts kernel there, round 4)
inline bool prefer_cluster()
{
    return !parts_debug_all();          // (tests of the parts kernel: ltr_debug_parts_all puts it first)
}

// Which kernel family runs a fused Linear step of (kind, B, L, F), and its shape: the ONE copy of the fallback chain register
// tile -> cluster (when prefer_cluster()) -> parts -> cluster -> general.  What the launch knows and the plan ABI does not is
// an argument: vec = 4 when X's rows are whole, 16-byte aligned float4; fast = LTR_TRACE_ALLOW_FAST (no score matrix asked
// for); labels = the cluster kernel's label kind (1 integer, 0 float, -1 unknown).  The general kernel's shape stays with its
// launch (choose_linear_shape).
struct LinearPlan { int family; RegtileShape rs; ClusterShape cs; PartsShape ps; };

LinearPlan plan_linear(int kind, int B, int L, int F, int vec, bool fast, int labels)
{
    LinearPlan pl;
    pl.family = LTR_PLAN_GENERAL;
    if (vec != 4 || !fast) return pl;
    const bool cluster_first = prefer_cluster();
    if (choose_regtile_shape(kind, L, F, pl.rs)) pl.family = LTR_PLAN_REGISTER_TILE;
    else if (cluster_first && choose_cluster_shape(kind, B, L, F, pl.cs, labels)) pl.family = LTR_PLAN_CLUSTER;
    else if (choose_parts_shape(kind, B, L, F, pl.ps)) pl.family = LTR_PLAN_PARTS;
    else if (!cluster_first && choose_cluster_shape(kind, B, L, F, pl.cs, labels)) pl.family = LTR_PLAN_CLUSTER;
    return pl;
}

// hold-backs of a lazy launch's query workgroups in units of 512 cycles (LinearParams::pend_sleep): without quiet workgroups,
// and with them -- everybody else's and the quiet ones' own (profiles/r07_lazy_quiet.txt)
constexpr int kLazyHoldPlain = 2, kLazyHold = 0, kLazyHoldQuiet = 8;
inline int &lazy_holdback() { static int v = -1; return v; }       // ltr_debug_lazy_holdback: >= 0 replaces the packed word
// Where the quiet rule was measured to pay (profiles/r07_lazy_quiet.txt): the hinge kinds -- their launch is bound by the memory
// system all CUs share, the others by their most loaded CU, which the reducers' CUs taking the shortest lists unbalances (C3,
// LambdaNDCG2: 17.3 -> 18.2 us; logistic 14.4 -> 15.2) --, a grid that fills the CUs (a fourth workgroup on some: at 600 queries
// the quiet ones' wait is the launch's tail, 10.4 -> 11.0) and rows of at least 64 features (8 features: 19.8 -> 20.1)
inline bool lazy_quiet_pays(int kind, int B, int F)
{
    return (kind == LTR_HINGE || kind == LTR_DCG_HINGE) && B > 3 * device_cu_count() && F >= 64;
}
}  // namespace

extern "C" {
LTR_DEBUG_HOOK void ltr_debug_force_timeout(int on) { cluster_force_timeout() = on ? 1 : 0; }
LTR_DEBUG_HOOK void ltr_debug_cluster_mode(int bits) { cluster_debug_mode() = bits; }
LTR_DEBUG_HOOK int ltr_debug_parts_all(int on) { const int old = parts_debug_all(); parts_debug_all() = on ? 1 : 0; return old; }

size_t ltr_linear_workspace_bytes(int B, int L, int F)
{
    if (B <= 0 || F <= 0) return 0;
    size_t bytes = linear_partials_bytes(B, F);
    // long lists on small batches, NDCG kinds: scratch of the cluster kernel behind the partials (the parts
    // kernel keeps its exchange buffers in memory the library owns: exchange_area_get)
    size_t scratch = 0;
    ClusterShape cs;
    // (the largest over the kinds: their batch limits differ, and the NDCG kinds carry the rank exchange -- round 4's
    // fuzz found LambdaNDCG1 at a batch size LambdaNDCG2 and the logistic loss both decline, sized from those two)
    // (and over the label dtypes: the hinge kinds' members are lighter -- more of them per query -- on integer labels)
    for (int kind = LTR_HINGE; kind <= LTR_NDCG2 && L > 0; ++kind)
        for (int labels = 0; labels <= 1; ++labels)
            if (choose_cluster_shape(kind, B, L, F, cs, labels) && cs.scratch_floats * sizeof(float) > scratch)
                scratch = cs.scratch_floats * sizeof(float);
    return bytes + scratch;
}

int ltr_linear_fused_plan(int kind, int B, int L, int F)
{
    LTR_CLEAR_STALE_ERROR();
    if (kind < LTR_HINGE || kind > LTR_NDCG2 || B <= 0 || L <= 0 || F <= 0) return LTR_PLAN_NONE;
    if (L > kMaxListLen) return LTR_PLAN_NONE;
    // (the plan of a launch on 16-byte aligned rows, no score matrix asked for, the label dtype not known)
    return plan_linear(kind, B, L, F, 4, true, -1).family;
}

namespace {
// the pending update a lazy step hands to the register-tile launch (ltr_linear_sgd_lazy_step_f32), or the flush to its reducers
struct LazyRequest {
    int pend_B; float lr; float *W, *bias, *out; unsigned long long *gran; unsigned tag; int part_g, pend_g;
    float scale;                        // weight of a pending query's gradient row (<= 0: 1 / pend_B)
    const float *scale_dev;             // ... or the weights on the device (or null): query b's is scale_dev[b * scale_stride]
    int scale_stride;
    const MailboxDev *mb;               // data parallel: the mailbox (gran / tag are then ITS granules and the tag of its lazy half)
};

// the uniform weight of a pending query's gradient row
inline float pending_weight(float scale, int pend_B) { return scale > 0.f ? scale : 1.0f / (float)pend_B; }

// The pending update's fields of a launch that carries reducers (linear_lazy_reduce): the ONE copy of the layout they read the
// rows in, for the lazy step's launch and for the flush alike.  queries: the lazy step -- its queries' workgroups hold their
// bursts back and poll the reducers' granules, so the status word and the spin limit are always set; false: the flush, the
// reducers alone, which only wait on the all-reduce of a mailbox.
void set_pending_update(LinearParams &p, const LazyRequest &r, int F, bool queries, hipStream_t stream, bool quiet_pays = false)
{
    p.pend_B = r.pend_B; p.pend_g = r.pend_g; p.pend_lr = r.lr; p.pend_w = pending_weight(r.scale, r.pend_B);
    p.pend_mb = r.mb; p.pend_wptr = r.scale_dev; p.pend_wstride = r.scale_stride;
    p.pend_W = r.W; p.pend_bias = r.bias; p.pend_out = r.out;
    p.pend_gran = r.gran; p.pend_tag = r.tag; p.pend_gstride = (F + 2 + 15) & ~15;
    // four columns per reducer + the losses' one
    p.pend_nred = (F + 1 + 3) / 4 + 1;
    p.pend_general = (p.pend_mb || p.pend_wptr || !p.pend_W) ? 1 : 0;
    // (a reducer sums ~1024 rows at most, whatever the batch size.  Low byte: every query workgroup's hold-back; next byte: the
    // quiet ones' -- under the list-length order with fewer reducers than CUs, sched_quiet, on the kinds where it pays; 0: nobody
    // is quiet)
    const bool quiet = quiet_pays && p.sched != 0 && p.pend_nred < (p.sched >> 16);
    p.pend_sleep = !queries ? 0 : lazy_holdback() >= 0 ? lazy_holdback() : quiet ? kLazyHoldQuiet << 8 | kLazyHold : kLazyHoldPlain;
    if (queries || r.mb) {
        p.status = status_device_ptr(stream);
        p.spin_limit = cluster_force_timeout() ? -1 : (r.mb ? 0x7fffffff : (1 << 22));
    }
}

int linear_partials_launch(int kind, float sigma, const float *X, const float *W, const float *bias, const void *rel, int rel_dtype,
                           const int64_t *n, int B, int L, int F, float *loss, float *scores_out, float *partials, void *stream,
                           const LazyRequest *lazy)
{
    LTR_CLEAR_STALE_ERROR();
    if (const int rc = check_kind(kind, rel_dtype)) return rc;
    if (step_shape_bad(B, L, F)) return LTR_ERR_SHAPE;
    if (L > kMaxListLen) return LTR_ERR_LIST_TOO_LONG;
    if (B == 0) return LTR_OK;
    if (!X || !W || !rel || !n || !loss || !partials) return LTR_ERR_NULL;
    if (const int st = status_peek()) return st;           // a kernel of an earlier call gave up
    const int vec = (F % 4 == 0 && ((uintptr_t)X % 16 == 0)) ? 4 : 1;
    LinearParams p;
    p.X = X; p.W = W; p.bias = bias; p.rel = rel; p.n = n;
    p.loss = loss; p.scores_out = scores_out; p.part = partials;
    p.B = B; p.L = L; p.F = F; p.sigma = sigma; p.rel_dtype = rel_dtype;
    p.sched = 0; p.rows_r = 0;
    const LinearPlan pl = plan_linear(kind, B, L, F, vec, LTR_TRACE_ALLOW_FAST(scores_out), rel_dtype != LTR_LABEL_F32 ? 1 : 0);
    if (lazy && pl.family != LTR_PLAN_REGISTER_TILE) return LTR_ERR_CONFIG;        // (the caller checked: lazy_layout_g)
    switch (pl.family) {
    case LTR_PLAN_REGISTER_TILE:
        p.msplit = kRegtileThreads / 64;         // (the body takes its slices from TT; the argument is eight on every tile)
        // (lists of 64 and fewer do not win the pass back: 512 x 64 x 136 6.7 -> 7.0 us; 1024 x 96: 11.3 -> 10.4)
        p.sched = (L > 64) ? sched_groups(B, kSchedMaxPerCu) : 0;
        // (snake dealing of the rounds, sched_query_sampled: measured round 6 on 1024 x 128 x 136 with four workgroups per CU resident --
        // LambdaNDCG2 16.6 -> 16.1 us, logistic 14.0 -> 13.5, hinge 11.84 -> 11.82: the kinds with compute behind their loads are
        // bound by their most loaded CU.  EXPERIMENTS.md round 6)
        // (on grids of whole rounds -- B = 2, 3 or 4 x #CUs, a multiple of 64 -- the kernel deals by the CU slot that hosts the block
        // id instead, sched_slot_cu, for every kind, quiet rule on or off: same box, same call, both orders of lazy_ab.py, lazy step
        // 1024 x 128 x 136: hinge 12.54-12.59 -> 12.05-12.06 us, DCG-hinge 12.87-12.91 -> 12.32-12.36, LambdaNDCG2 17.55 -> 17.33-17.35,
        // logistic 14.52-14.75 -> 14.33-14.59 (below in three pairs of four, by less than the order bias: no win, no loss); hinge
        // 768 x 128 x 136 11.73-11.79 -> 11.12-11.14, 512 x 128 x 136 9.95-9.98 -> 9.91-9.94 (inside the spread).  No kind or shape
        // lost, so there is no rule function in front of it.  profiles/sched_balance_ab.txt)
        if (p.sched) p.sched |= device_cu_count() << 16;
        if (lazy) p.part_g = lazy->part_g;
        p.scores_out = LTR_TRACE_BUFFER(p.scores_out);      // (trace builds: the lazy step's launches have no score matrix to stamp)
        if (lazy && lazy->pend_B > 0) set_pending_update(p, *lazy, F, true, (hipStream_t)stream, lazy_quiet_pays(kind, B, F));
        return launch_regtile(kind, p, pl.rs, (hipStream_t)stream);
    case LTR_PLAN_PARTS:
        p.msplit = 0;
        return launch_parts(kind, p, pl.ps, (hipStream_t)stream);
    case LTR_PLAN_CLUSTER: {
        p.msplit = pl.cs.threads / 64;
        p.sched = (B >= 16) ? (B + 63) / 64 : 0;
        float *scratch = partials + linear_partials_bytes(B, F) / sizeof(float);
        return launch_cluster(kind, p, pl.cs, scratch, (hipStream_t)stream);
    }
    default: break;
    }
    LinearShape s;
    if (!choose_linear_shape(kind, B, L, F, vec, s)) return LTR_ERR_SHAPE;
    p.msplit = s.msplit; p.rows_r = s.R;
    p.sched = sched_groups_for_lists(B, L);
    return (vec == 4) ? launch_linear<4>(kind, p, s, (hipStream_t)stream)
                      : launch_linear<1>(kind, p, s, (hipStream_t)stream);
}
}  // namespace

int ltr_linear_partials_f32(int kind, float sigma, const float *X, const float *W,
                            const float *bias, const void *rel, int rel_dtype,
                            const int64_t *n, int B, int L, int F, float *loss,
                            float *scores_out, float *partials, void *stream)
{
    return linear_partials_launch(kind, sigma, X, W, bias, rel, rel_dtype, n, B, L, F, loss, scores_out, partials, stream, nullptr);
}

LTR_DEBUG_HOOK int ltr_debug_sched_slots(int B, int G, int cus, int nred, int *group, int *rank)
{
    if (B <= 0 || G <= 0 || cus < 0 || nred < 0) return LTR_ERR_SHAPE;
    if (nred > 0 && nred < cus && (long long)B + nred >= 8ll * cus) return LTR_ERR_SHAPE;        // (sched_round)
    if (!group || !rank) return LTR_ERR_NULL;
    for (int i = 0; i < B; ++i) {
        const SchedSlot s = sched_slot(nred + i, B, G, cus, nred);
        group[i] = s.group;
        rank[i] = s.rank;
    }
    return LTR_OK;
}

LTR_DEBUG_HOOK int ltr_debug_sched_slots_cu(int B, int G, int cus, int nred, int quiet, int *group, int *rank)
{
    if (B <= 0 || G != (B + 63) / 64 || !sched_cu_deal_applies(B, cus, nred, quiet != 0)) return LTR_ERR_SHAPE;
    if (!group || !rank) return LTR_ERR_NULL;
    for (int i = 0; i < B; ++i) {
        const SchedSlot s = sched_slot_cu(nred + i, B, G, cus, nred, quiet != 0);
        group[i] = s.group;
        rank[i] = s.rank;
    }
    return LTR_OK;
}

#ifdef LTR_TRACE
// Trace builds only: the stamp buffer of the launches that are given no score matrix (the lazy step's), or null.
int ltr_debug_trace_buffer(void *buf) { trace_buffer() = (float *)buf; return LTR_OK; }
#endif

// Measurement aid (bench.py `roofline`): the next launch of the 512-thread register tile on this thread records `start` right
// before and `stop` right behind the kernel (hipExtLaunchKernelGGL) -- the kernel's own duration, as a profiler sees it.
LTR_DEBUG_HOOK int ltr_debug_kernel_events(void *start, void *stop)
{
    KernelEvents &ke = kernel_events();
    ke.start = (hipEvent_t)start; ke.stop = (hipEvent_t)stop;
    ke.armed = start != nullptr && stop != nullptr;
    return LTR_OK;
}

LTR_DEBUG_HOOK int ltr_debug_stream_probe_f32(const float *X, const int64_t *n, int B, int L, int F, float *out, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (B <= 0 || L <= 0 || F <= 0 || F % 4 != 0) return LTR_ERR_SHAPE;
    if (!X || !n || !out) return LTR_ERR_NULL;
    const long long vecs = (long long)L * (F / 4);
    const dim3 grid((unsigned)B);
    hipStream_t st = (hipStream_t)stream;
#define LTR_PROBE(NI_, TT_) hipLaunchKernelGGL((stream_probe_kernel<NI_, TT_>), grid, dim3(TT_), 0, st, X, n, L, F, out)
    if (vecs <= 3 * 512) LTR_PROBE(3, 512);
    else if (vecs <= 5 * 512) LTR_PROBE(5, 512);
    else if (vecs <= 9 * 512) LTR_PROBE(9, 512);
    else if (vecs <= 12 * 512) LTR_PROBE(12, 512);
    else if (vecs <= 19 * 512) LTR_PROBE(19, 512);
    else return LTR_ERR_SHAPE;
#undef LTR_PROBE
    return (int)hipGetLastError();
}

int ltr_linear_reduce_accum_f32(const float *partials, const float *grad_out, const float *loss,
                                int B, int F, float *dW, float *db, float *loss_sum, int accumulate,
                                void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (B < 0 || F <= 0) return LTR_ERR_SHAPE;
    if (!dW || !db) return LTR_ERR_NULL;
    if (B > 0 && !partials) return LTR_ERR_NULL;
    if ((loss_sum != nullptr) && B > 0 && !loss) return LTR_ERR_NULL;
    if (const int st = status_peek()) return st;           // a kernel of an earlier call gave up
    return launch_linear_reduce((hipStream_t)stream, partials, grad_out, B > 0 ? 1.0f / (float)B : 0.f, 1, B, F, dW, db, loss, loss_sum,
                                accumulate ? 1 : 0, nullptr, nullptr, 0.f);
}

// include/ltr_hip.h: dW = scale[0] * sum_b partials[b, :], the upstream gradient a DEVICE scalar (what autograd hands a
// `.mean().backward()` / `.sum().backward()`: an expanded scalar of stride 0 -- no (B,) copy of it is made)
int ltr_linear_reduce_bcast_f32(const float *partials, const float *scale, int B, int F, float *dW, float *db, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (B < 0 || F <= 0) return LTR_ERR_SHAPE;
    if (!dW || !db || !scale) return LTR_ERR_NULL;
    if (B > 0 && !partials) return LTR_ERR_NULL;
    if (const int st = status_peek()) return st;
    return launch_linear_reduce((hipStream_t)stream, partials, scale, 0.f, 0, B, F, dW, db, nullptr, nullptr, 0, nullptr, nullptr, 0.f);
}

int ltr_linear_reduce_loss_f32(const float *partials, const float *grad_out, const float *loss,
                               int B, int F, float *dW, float *db, float *loss_sum, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    return ltr_linear_reduce_accum_f32(partials, grad_out, loss, B, F, dW, db, loss_sum, 0, stream);
}

int ltr_linear_reduce_f32(const float *partials, const float *grad_out, int B, int F, float *dW,
                          float *db, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    return ltr_linear_reduce_loss_f32(partials, grad_out, nullptr, B, F, dW, db, nullptr, stream);
}

int ltr_linear_step_f32(int kind, float sigma, const float *X, const float *W, const float *bias,
                        const void *rel, int rel_dtype, const int64_t *n, const float *grad_out,
                        int B, int L, int F, float *loss, float *bucket, int accumulate,
                        void *workspace, size_t workspace_bytes, void *overlap, int slot, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (step_shape_bad(B, L, F)) return LTR_ERR_SHAPE;
    if (!bucket) return LTR_ERR_NULL;
    if (step_workspace_short(B, L, F, workspace, workspace_bytes)) return LTR_ERR_WORKSPACE;
    LtrOverlap *o = reinterpret_cast<LtrOverlap *>(overlap);
    if (o && o->depth > 0 && (slot < 0 || slot >= o->depth)) return LTR_ERR_CONFIG;
    // the bucket of this slot may still be in its last all-reduce: the kernels queue up behind it
    if (o) { const int rc = ltr_overlap_wait(o, slot, stream); if (rc != 0) return rc; }
    int rc = ltr_linear_partials_f32(kind, sigma, X, W, bias, rel, rel_dtype, n, B, L, F, loss, nullptr,
                                     (float *)workspace, stream);
    if (rc != 0) return rc;
    rc = ltr_linear_reduce_accum_f32((const float *)workspace, grad_out, loss, B, F, bucket, bucket_db(bucket, F),
                                     bucket_loss_sum(bucket, F), accumulate, stream);
    if (rc != 0 || !o) return rc;
    // in-stream: one ncclAllReduce behind the kernels, nothing else
    if (o->depth == 0) return overlap_allreduce(o, bucket, bucket_count(F), stream);
    const hipError_t e = hipEventRecord(o->ready[slot], (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    o->bucket[slot] = bucket;
    o->count[slot] = bucket_count(F);
    o->pending[slot] = true;
    o->submitted[slot].fetch_add(1, std::memory_order_relaxed);
    { std::lock_guard<std::mutex> lock(o->m); o->jobs.push_back(slot); }
    o->cv.notify_one();
    return LTR_OK;
}

// One synchronous-SGD step of the reference's training loop (examples/01-basic-usage.py:66-75:
// loss_fn(model(xs), ys, n).mean().backward(); optimizer.step() with torch.optim.SGD) in ONE call: partials +
// reduction into the bucket [dW | db | loss_sum] with the upstream gradient grad_out (NULL = 1 / B), the
// step's gradient all-reduce when an in-stream overlap handle is given (data parallel: grad_out = 1 / (B * N)
// makes the summed bucket the gradient of the global mean), then W -= lr * dW, bias -= lr * db.  The next step's
// scores depend on this step's all-reduced gradient: the collective sits on the critical path by construction.
// At one rank the update rides in the reduction kernel (two launches in all); behind an all-reduce it is one
// small launch more.
int ltr_linear_sgd_step_f32(int kind, float sigma, const float *X, float *W, float *bias, const void *rel,
                            int rel_dtype, const int64_t *n, const float *grad_out, int B, int L, int F,
                            float lr, float *loss, float *bucket, void *workspace, size_t workspace_bytes,
                            void *overlap, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (step_shape_bad(B, L, F)) return LTR_ERR_SHAPE;
    if (!bucket || !W) return LTR_ERR_NULL;
    if (step_workspace_short(B, L, F, workspace, workspace_bytes)) return LTR_ERR_WORKSPACE;
    LtrOverlap *o = reinterpret_cast<LtrOverlap *>(overlap);
    if (o && o->depth != 0) return LTR_ERR_CONFIG;              // (a deferred all-reduce cannot feed this step's update)
    int rc = ltr_linear_partials_f32(kind, sigma, X, W, bias, rel, rel_dtype, n, B, L, F, loss, nullptr,
                                     (float *)workspace, stream);
    if (rc != 0) return rc;
    if (const int st = status_peek()) return st;
    rc = launch_linear_reduce((hipStream_t)stream, (const float *)workspace, grad_out, B > 0 ? 1.0f / (float)B : 0.f, 1, B, F, bucket,
                              bucket_db(bucket, F), loss, bucket_loss_sum(bucket, F), 0, o ? nullptr : W, o ? nullptr : bias, lr);
    if (rc != 0 || !o) return rc;
    if (o->fn == &ltr_mailbox_allreduce)          // (the mailbox kernel sums AND applies the update: one launch)
        return mailbox_launch(reinterpret_cast<LtrMailbox *>(o->comm), bucket, bucket, bucket_count(F), W, bias, lr, F,
                              (hipStream_t)stream);
    rc = overlap_allreduce(o, bucket, bucket_count(F), stream);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(sgd_update_kernel, dim3((unsigned)((F + 1 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       W, bias, (const float *)bucket, lr, F);
    return (int)hipGetLastError();
}

int ltr_linear_pairwise_f32(int kind, float sigma, const float *X, const float *W,
                            const float *bias, const void *rel, int rel_dtype,
                            const int64_t *n, const float *grad_out, int B, int L, int F,
                            float *loss, float *scores_out, float *dW, float *db,
                            void *workspace, size_t workspace_bytes, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (step_shape_bad(B, L, F)) return LTR_ERR_SHAPE;
    if (!dW || !db) return LTR_ERR_NULL;
    if (step_workspace_short(B, L, F, workspace, workspace_bytes)) return LTR_ERR_WORKSPACE;
    int rc = ltr_linear_partials_f32(kind, sigma, X, W, bias, rel, rel_dtype, n, B, L, F, loss,
                                     scores_out, (float *)workspace, stream);
    if (rc != 0) return rc;
    return ltr_linear_reduce_f32((const float *)workspace, grad_out, B, F, dW, db, stream);
}
}  // extern "C"
