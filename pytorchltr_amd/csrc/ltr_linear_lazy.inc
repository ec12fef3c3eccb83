// ltr_linear_lazy.inc -- the host side of the lazy SGD step: which batches write their rows column-group major (lazy_layout_g),
// the next in-launch all-reduce of a mailbox's lazy half, the flush and the lazy step entry points.  No kernels.  Needs
// LazyRequest, set_pending_update and linear_partials_launch (ltr_linear_step.inc), lazy_area_next and mailbox_next_tag
// (ltr_areas.inc), the mailbox (ltr_mailbox.inc), the bucket (ltr_overlap.inc) and linear_lazy_flush_kernel (ltr_linear.inc).
// ---------------------------------------------------------------------------------------------
// LAZY synchronous SGD (include/ltr_hip.h).  ltr_linear_sgd_step_f32 is two launches -- the fused kernel, then the reduction of
// its (B, F + 1) partial rows with the update -- and two kernel boundaries per step (1.5-1.9 us each on this stack).  The update of
// step k only has to be applied before step k + 1 takes its dot products, and those come BEHIND the tile burst: so step k + 1's
// launch applies it itself (the first workgroups reduce a column each in front of their burst and publish the new weights as
// tagged granules, every workgroup picks its weights up behind its burst: linear_regtile2_kernel), and the reduction launch and
// one boundary are gone from every step but the last, whose update ltr_linear_sgd_flush_f32 applies.  The same arithmetic in
// the same order as the two launches: W, bias, dW, db and the losses are bit-identical (tests/test_gpu_step.py).
// Granules and their tags live in a lazy area per (device, stream): library-owned, zeroed when allocated, the tag a host-side
// counter -- eager launches only (a captured launch would replay a frozen tag): under capture, and on shapes the register tile
// does not take, the pending update is flushed first and the step runs as the plain launch.
// ---------------------------------------------------------------------------------------------
extern "C" {
namespace {
bool stream_is_capturing(hipStream_t stream)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) != hipSuccess) return true;      // (cannot tell: the safe path)
    return cs != hipStreamCaptureStatusNone;
}
}  // namespace

// Does a lazy step write the partial rows of a (B, L, F) batch column-group major?  A matter of the SHAPE only -- the step that
// wrote them, the step that reads them and the flush must agree: the register-tile kernel's shapes.  (X must be 16-byte aligned
// for the lazy entry points when F % 4 == 0.)
// ONE ROUND of workgroups at most (B <= 4 x CUs): a larger batch's update never rides in the next launch (see below), so
// its step is the plain launch behind a reduction launch either way -- and row-major rows have the better of both: a query's row
// is ONE contiguous store (the column-group layout scatters it in 16-byte pieces: 65 536 full lists 894 against 779 us per step)
// and launch_linear_reduce's split kernels sum them at the chip's bandwidth whatever B (round 6; the first version of this
// round split the lazy reducers instead -- several workgroups per column group, tagged scratch rows: dropped, EXPERIMENTS.md).
static bool lazy_one_round(int B) { return B <= 4 * device_cu_count(); }
static bool lazy_layout_g(int kind, int B, int L, int F)
{
    if (B <= 0 || F % 4 != 0 || !lazy_one_round(B)) return false;
    RegtileShape rs;
    return choose_regtile_shape(kind, L, F, rs);         // (plan_linear's first choice)
}
// (May a launch of MORE than one round take a pending update along?  No: every workgroup of every later round still pays the
// hold-back and the hand-over in front of its dot products -- its poll sits behind its tile burst in the in-order return queue --
// and the launch loses more than the reduction launch costs.  4096 x 128 x 136, round 5: 40.6 -> 44.4 us per step; round 6 with
// split reducers: 36.8 -> 45.6, and with their combine stripped of its fences and load chain, hold-back 0 / 1 / 2:
// 35.0 -> 36.3 .. 36.9 at 4096 queries, 68.1 -> 71.6 .. 74.4 at 8192.)

// The next in-launch all-reduce of the mailbox's lazy half: ONE host-side tag (eager launches only; every rank makes the same
// calls) for the peers' granules AND the launch's own weight granules, which belong to the mailbox for these launches; the time
// budget travels in device memory (updated in stream order when it changed: ltr_mailbox_set_timeout_ms, the tests' forced give-up).
static int lazy_mailbox_next(LtrMailbox *m, hipStream_t stream, int F, const MailboxDev **mb, unsigned long long **gran, unsigned *tag)
{
    if (lazy_area_words(F) > m->lazy_gran_count) return LTR_ERR_CONFIG;
    const long long ticks = mailbox_timeout_ticks();
    if (ticks != m->dev_ticks) {
        long long *src = &m->stage[m->stage_i++ & 15];
        *src = ticks;
        if (hipMemcpyAsync(&m->dev->ticks, src, sizeof(long long), hipMemcpyHostToDevice, stream) != hipSuccess) return LTR_ERR_CONFIG;
        m->dev_ticks = ticks;
    }
    const unsigned next = mailbox_next_tag(m->lazy_tag);
    if (next < m->lazy_tag) {
        // the tags start over (2^32 all-reduces): the weight granules go back to zero first, in stream order
        if (hipMemsetAsync(m->lazy_gran, 0, m->lazy_gran_count * 8, stream) != hipSuccess) return LTR_ERR_CONFIG;
    }
    m->lazy_tag = next;
    *mb = m->dev; *gran = m->lazy_gran; *tag = next;
    return LTR_OK;
}

namespace {
// The pending batch's rows summed into the bucket.  update: W -= lr * dW and bias -= lr * db with it (W is required; data
// parallel: behind the mailbox's all-reduce); else the reduction alone, W and bias null.  has_bias: whether the step that wrote
// the rows had a bias -- with the shape, what decides their layout (lazy_layout_g(...) && bias in the lazy step).
int lazy_flush_impl(int kind, bool update, float *W, float *bias, bool has_bias, int pending_B, int L, int F, float lr, float pending_scale,
                    const float *pending_scale_dev, int pending_scale_stride, const float *loss, float *bucket, const void *workspace, void *mailbox,
                    void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (step_shape_bad(pending_B, L, F)) return LTR_ERR_SHAPE;
    LtrMailbox *m = mailbox_or_none(mailbox);
    if (pending_B == 0) return m ? LTR_ERR_SHAPE : LTR_OK;       // (data parallel: every rank brings at least one query to every step)
    if ((update && !W) || !bucket || !workspace || !loss) return LTR_ERR_NULL;
    if (!update && m) return LTR_ERR_CONFIG;
    if (mailbox_unfit(m, F, bias)) return LTR_ERR_CONFIG;
    if (const int st = status_peek()) return st;
    if (lazy_layout_g(kind, pending_B, L, F) && has_bias) {
        // rows in the lazy step's layout: the reducers of the lazy launch, on their own (data parallel: with their all-reduce)
        LazyRequest req{pending_B, lr, W, bias, bucket, nullptr, 0u, 0, 1, pending_scale, pending_scale_dev, pending_scale_stride, nullptr};
        if (m) {
            if (stream_is_capturing((hipStream_t)stream)) return LTR_ERR_CONFIG;      // (host-side tags: eager launches only)
            if (const int rc = lazy_mailbox_next(m, (hipStream_t)stream, F, &req.mb, &req.gran, &req.tag)) return rc;
        }
        LinearParams p{};
        p.part = const_cast<float *>(reinterpret_cast<const float *>(workspace));
        p.loss = const_cast<float *>(loss);
        p.F = F; p.B = pending_B;
        set_pending_update(p, req, F, false, (hipStream_t)stream);
        hipLaunchKernelGGL(linear_lazy_flush_kernel, dim3((unsigned)p.pend_nred), dim3(256), 0, (hipStream_t)stream, p);
        return (int)hipGetLastError();
    }
    // (the upstream gradient: a device scalar read with stride 0, or the uniform weight)
    const float *go = pending_scale_dev;
    const float scale = pending_weight(pending_scale, pending_B);
    if (!m)
        return launch_linear_reduce((hipStream_t)stream, (const float *)workspace, go, scale, pending_scale_stride, pending_B, F, bucket,
                                    bucket_db(bucket, F), loss, bucket_loss_sum(bucket, F), 0, W, bias, lr);
    // data parallel, rows by query (shapes off the register tile): the reduction launch, then the plain mailbox all-reduce with
    // the update riding in it
    if (const int rc = launch_linear_reduce((hipStream_t)stream, (const float *)workspace, go, scale, pending_scale_stride, pending_B, F,
                                            bucket, bucket_db(bucket, F), loss, bucket_loss_sum(bucket, F), 0, nullptr, nullptr, lr)) return rc;
    return mailbox_launch(m, bucket, bucket, bucket_count(F), W, bias, lr, F, (hipStream_t)stream);
}
}  // namespace

int ltr_linear_sgd_flush_dp_f32(int kind, float *W, float *bias, int pending_B, int L, int F, float lr, float pending_scale,
                                const float *pending_scale_dev, int pending_scale_stride, const float *loss, float *bucket,
                                const void *workspace, void *mailbox, void *stream)
{
    return lazy_flush_impl(kind, true, W, bias, bias != nullptr, pending_B, L, F, lr, pending_scale, pending_scale_dev, pending_scale_stride,
                           loss, bucket, workspace, mailbox, stream);
}

int ltr_linear_lazy_rows_reduce_f32(int kind, int pending_B, int L, int F, float pending_scale, const float *pending_scale_dev,
                                    int pending_scale_stride, const float *loss, float *bucket, const void *workspace, int has_bias, void *stream)
{
    return lazy_flush_impl(kind, false, nullptr, nullptr, has_bias != 0, pending_B, L, F, 0.f, pending_scale, pending_scale_dev,
                           pending_scale_stride, loss, bucket, workspace, nullptr, stream);
}

int ltr_linear_sgd_flush_f32(int kind, float *W, float *bias, int pending_B, int L, int F, float lr, const float *loss,
                             float *bucket, const void *workspace, void *stream)
{
    return ltr_linear_sgd_flush_dp_f32(kind, W, bias, pending_B, L, F, lr, 0.f, nullptr, 0, loss, bucket, workspace, nullptr, stream);
}

int ltr_linear_sgd_lazy_step_dp_f32(int kind, float sigma, const float *X, float *W, float *bias, const void *rel,
                                    int rel_dtype, const int64_t *n, int B, int L, int F, float lr, float *loss, float *bucket,
                                    void *workspace, size_t workspace_bytes, int pending_B, float pending_scale,
                                    const float *pending_scale_dev, int pending_scale_stride, void *mailbox, void *stream)
{
    LTR_CLEAR_STALE_ERROR();
    if (step_shape_bad(B, L, F) || pending_B < 0) return LTR_ERR_SHAPE;
    if (!bucket || !W || !loss) return LTR_ERR_NULL;
    LtrMailbox *m = mailbox_or_none(mailbox);
    if (mailbox_unfit(m, F, bias)) return LTR_ERR_CONFIG;
    if (step_workspace_short(B, L, F, workspace, workspace_bytes)) return LTR_ERR_WORKSPACE;
    if (step_workspace_short(pending_B, L, F, workspace, workspace_bytes)) return LTR_ERR_WORKSPACE;
    if (F % 4 == 0 && (uintptr_t)X % 16 != 0) return LTR_ERR_CONFIG;          // (the layout of the rows must follow from the shape alone)
    if (B == 0) return ltr_linear_sgd_flush_dp_f32(kind, W, bias, pending_B, L, F, lr, pending_scale, pending_scale_dev, pending_scale_stride, loss, bucket, workspace, mailbox, stream);
    const bool part_g = lazy_layout_g(kind, B, L, F) && bias != nullptr;
    const bool pend_g = pending_B > 0 && lazy_layout_g(kind, pending_B, L, F) && bias != nullptr;
    // does this launch take the pending update along?  (both batches on the register-tile kernel, an eager launch)
    const bool along = pending_B > 0 && part_g && pend_g && lazy_one_round(B) && !stream_is_capturing((hipStream_t)stream);
    if (pending_B > 0 && !along) {
        const int rc = ltr_linear_sgd_flush_dp_f32(kind, W, bias, pending_B, L, F, lr, pending_scale, pending_scale_dev, pending_scale_stride, loss, bucket, workspace, mailbox, stream);
        if (rc != 0) return rc;
    }
    LazyRequest req{along ? pending_B : 0, lr, W, bias, bucket, nullptr, 0u, part_g ? 1 : 0, pend_g ? 1 : 0, pending_scale, pending_scale_dev, pending_scale_stride, nullptr};
    if (along) {
        if (m) {
            if (const int rc = lazy_mailbox_next(m, (hipStream_t)stream, F, &req.mb, &req.gran, &req.tag)) return rc;
        } else if (const int rc = lazy_area_next((hipStream_t)stream, lazy_area_words(F), &req.gran, &req.tag)) return rc;
    }
    return linear_partials_launch(kind, sigma, X, W, bias, rel, rel_dtype, n, B, L, F, loss, nullptr, (float *)workspace, stream,
                                  part_g ? &req : nullptr);
}

int ltr_linear_sgd_lazy_step_f32(int kind, float sigma, const float *X, float *W, float *bias, const void *rel,
                                 int rel_dtype, const int64_t *n, int B, int L, int F, float lr, float *loss, float *bucket,
                                 void *workspace, size_t workspace_bytes, int pending_B, void *stream)
{
    return ltr_linear_sgd_lazy_step_dp_f32(kind, sigma, X, W, bias, rel, rel_dtype, n, B, L, F, lr, loss, bucket, workspace,
                                           workspace_bytes, pending_B, 0.f, nullptr, 0, nullptr, stream);
}

LTR_DEBUG_HOOK int ltr_debug_lazy_holdback(int packed)
{
    const int old = lazy_holdback();
    lazy_holdback() = packed < 0 ? -1 : (packed & 0xffff);
    return old;
}
}  // extern "C"
