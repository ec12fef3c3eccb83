// ltr_overlap.inc -- the gradient bucket of a Linear step and its all-reduce: the bucket's layout, the ONE call of the caller's
// collective, and LtrOverlap, the handle whose helper thread keeps that call off the launching thread (ltr_overlap_*,
// include/ltr_hip.h).  Host code only; needs <atomic>, <condition_variable>, <deque>, <mutex>, <thread> from the translation
// unit and, for the tests' fake collective at the end, fake_allreduce_kernel (ltr_linear.inc).
// ---- the step in one call, with its gradient all-reduce overlapped (include/ltr_hip.h) ----
// Measured on MI355X / ROCm 7.2 (by a host-cost script that is no longer in the tree): hipEventRecord 0.9 us and hipStreamWaitEvent on
// a COMPLETED event 0.4 us of host time, but a wait on an event that has just been recorded (a real
// cross-stream dependency) 6.5 us -- two of those per step make the thread that launches the 15 us step
// host-bound at 33 us.  So the dependency-creating calls live on a helper thread of the handle: the
// launching thread only records `ready` behind its kernels and hands the slot over; the helper makes the
// side stream wait for it, enqueues the all-reduce and records `done`.  When the launching thread comes
// back to the slot (depth steps later) `done` has long completed and its wait costs 0.4 us.
extern "C" {
namespace {
constexpr int kOverlapMaxDepth = 8;
struct LtrOverlap {
    ltr_allreduce_fn fn;
    void *comm;
    int depth, device;
    hipStream_t side;
    hipEvent_t ready[kOverlapMaxDepth], done[kOverlapMaxDepth];
    float *bucket[kOverlapMaxDepth];
    size_t count[kOverlapMaxDepth];
    std::atomic<unsigned> submitted[kOverlapMaxDepth], completed[kOverlapMaxDepth];
    bool pending[kOverlapMaxDepth];
    std::atomic<int> error;
    std::thread worker;
    std::mutex m;
    std::condition_variable cv;
    std::deque<int> jobs;
    bool stop;
};

// The bucket a step leaves its gradient in, and what is all-reduced: [dW (F) | db | loss_sum], F + 2 floats.
inline float *bucket_db(float *bucket, int F) { return bucket + F; }
inline float *bucket_loss_sum(float *bucket, int F) { return bucket + F + 1; }
inline size_t bucket_count(int F) { return (size_t)F + 2; }

// The caller's collective, in place on `count` floats; 0, or 1000 + the ncclResult_t it returned
inline int overlap_allreduce(const LtrOverlap *o, float *bucket, size_t count, void *stream)
{
    const int nrc = o->fn(bucket, bucket, count, 7 /* ncclFloat32 */, 0 /* ncclSum */, o->comm, stream);
    return nrc != 0 ? 1000 + nrc : LTR_OK;
}

void overlap_worker(LtrOverlap *o)
{
    (void)hipSetDevice(o->device);
    for (;;) {
        int slot;
        {
            std::unique_lock<std::mutex> lock(o->m);
            o->cv.wait(lock, [o] { return o->stop || !o->jobs.empty(); });
            if (o->jobs.empty()) return;                   // stop requested and nothing left to do
            slot = o->jobs.front();
            o->jobs.pop_front();
        }
        hipError_t e = hipStreamWaitEvent(o->side, o->ready[slot], 0);
        int rc = (e == hipSuccess) ? 0 : (int)e;
        if (rc == 0) rc = overlap_allreduce(o, o->bucket[slot], o->count[slot], o->side);
        if (rc == 0) { e = hipEventRecord(o->done[slot], o->side); if (e != hipSuccess) rc = (int)e; }
        if (rc != 0) { int zero = 0; o->error.compare_exchange_strong(zero, rc); }
        o->completed[slot].fetch_add(1, std::memory_order_release);
    }
}

// the helper has taken every job handed to this slot (its `done` event is recorded)
inline void overlap_settle(LtrOverlap *o, int slot)
{
    const unsigned want = o->submitted[slot].load(std::memory_order_relaxed);
    while (o->completed[slot].load(std::memory_order_acquire) != want) std::this_thread::yield();
}
}  // namespace

int ltr_overlap_create(ltr_allreduce_fn allreduce_fn, void *comm, int depth, void **handle)
{
    LTR_CLEAR_STALE_ERROR();
    if (!allreduce_fn || !handle) return LTR_ERR_NULL;
    if (depth < 0 || depth > kOverlapMaxDepth) return LTR_ERR_CONFIG;
    LtrOverlap *o = new LtrOverlap();
    o->fn = allreduce_fn; o->comm = comm; o->depth = depth; o->side = nullptr; o->stop = false;
    o->error.store(0);
    o->device = 0;
    (void)hipGetDevice(&o->device);
    for (int i = 0; i < kOverlapMaxDepth; ++i) {
        o->ready[i] = nullptr; o->done[i] = nullptr; o->pending[i] = false; o->bucket[i] = nullptr; o->count[i] = 0;
        o->submitted[i].store(0); o->completed[i].store(0);
    }
    if (depth == 0) {            // in-stream mode: the all-reduce is enqueued on the step's own stream, no helper
        *handle = o;
        return LTR_OK;
    }
    hipError_t e = hipStreamCreateWithFlags(&o->side, hipStreamNonBlocking);
    for (int i = 0; i < depth && e == hipSuccess; ++i) {
        e = hipEventCreateWithFlags(&o->ready[i], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&o->done[i], hipEventDisableTiming);
    }
    if (e != hipSuccess) { (void)ltr_overlap_destroy(o); return (int)e; }
    o->worker = std::thread(overlap_worker, o);
    *handle = o;
    return LTR_OK;
}

int ltr_overlap_destroy(void *handle)
{
    LtrOverlap *o = reinterpret_cast<LtrOverlap *>(handle);
    if (!o) return LTR_OK;
    if (o->worker.joinable()) {
        { std::lock_guard<std::mutex> lock(o->m); o->stop = true; }
        o->cv.notify_all();
        o->worker.join();
    }
    if (o->side) { (void)hipStreamSynchronize(o->side); (void)hipStreamDestroy(o->side); }
    for (int i = 0; i < kOverlapMaxDepth; ++i) {
        if (o->ready[i]) (void)hipEventDestroy(o->ready[i]);
        if (o->done[i]) (void)hipEventDestroy(o->done[i]);
    }
    delete o;
    return LTR_OK;
}

int ltr_overlap_wait(void *handle, int slot, void *stream)
{
    LtrOverlap *o = reinterpret_cast<LtrOverlap *>(handle);
    if (!o) return LTR_ERR_NULL;
    if (o->depth == 0) return LTR_OK;
    if (slot < 0 || slot >= o->depth) return LTR_ERR_CONFIG;
    if (!o->pending[slot]) return o->error.load();
    overlap_settle(o, slot);
    o->pending[slot] = false;
    if (const int err = o->error.load()) return err;
    return (int)hipStreamWaitEvent((hipStream_t)stream, o->done[slot], 0);
}

int ltr_overlap_flush(void *handle)
{
    LtrOverlap *o = reinterpret_cast<LtrOverlap *>(handle);
    if (!o) return LTR_ERR_NULL;
    if (o->depth == 0) return LTR_OK;
    for (int i = 0; i < o->depth; ++i) { overlap_settle(o, i); o->pending[i] = false; }
    const hipError_t e = hipStreamSynchronize(o->side);
    if (const int err = o->error.load()) return err;
    return (int)e;
}

// Tests only: an `ltr_allreduce_fn` that adds a second, known bucket -- `comm` is a device pointer to `count`
// floats, "the other rank's contribution" -- on the given stream.
LTR_DEBUG_HOOK int ltr_debug_fake_allreduce(const void *sendbuf, void *recvbuf, size_t count, int dtype, int op, void *comm, void *stream)
{
    if (dtype != 7 || op != 0 || !comm) return 1;
    hipLaunchKernelGGL(fake_allreduce_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float *)sendbuf, (float *)recvbuf, (const float *)comm, count);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
}  // extern "C"
