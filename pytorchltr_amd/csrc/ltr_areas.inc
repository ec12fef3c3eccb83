// ltr_areas.inc -- the device memory the LIBRARY owns: one pool of zeroed areas for the kernels that hand data to each other
// through memory (ltr_cluster.inc, ltr_parts.inc: exchange_area_get; the lazy SGD step: lazy_area_next).  Host code only.
// Needs LTR_OK / LTR_ERR_* (ltr_hip.h) and <deque>, <mutex> from the translation unit.
// ---------------------------------------------------------------------------------------------
// Exchange areas.  The kernels whose workgroups hand data to each other inside a launch
// (ltr_parts.inc) keep their control words and tagged granules in device memory that the LIBRARY owns:
// zeroed when it is allocated and never handed to anybody else, so no kernel ever trusts
// uninitialised memory (round 3 kept them in the caller's workspace behind a magic word; a recycled
// allocation could leave the magic intact over dirty counters -- ADVICE r3).  One area per (device,
// stream) for eager launches -- launches on a stream are ordered, so they can share it; a PRIVATE
// area for every call made under stream capture -- a captured launch may be replayed on any stream,
// next to anything.  An area is two allocations: `gran` holds nothing but granules ({tag, value}
// words and zeros: memory that has carried other data can never look like a granule of the current
// tag), `misc` the control block (fixed size, in front) and the parked shares.
// Lazy areas.  The weight granules of the lazy SGD step (ltr_linear_lazy.inc), one area per (device, stream): the tag is a
// host-side counter, so eager launches only.
// Both kinds live in ONE pool: one mutex, one allocator (exchange_alloc_zeroed), one list of retired blocks.  Areas grow, and a
// block that is outgrown stays allocated (work queued on the stream, or a graph, may still refer to it); ltr_exchange_release()
// frees every block of the pool when the caller knows nothing is in flight.
// ---------------------------------------------------------------------------------------------
namespace {
// control region in front of `misc`: the parts kernel's control block (tag, tickets, arrival counters of up to 8192
// queries), then the cluster kernel's counters (256 bytes per query); both zero between launches
constexpr size_t kExPartsCtrlBytes = 64 * 1024;
constexpr size_t kExClusterCtrlBytes = 128 * 1024;
constexpr size_t kExCtrlBytes = kExPartsCtrlBytes + kExClusterCtrlBytes;
struct ExchangeArea {
    int device;
    hipStream_t stream;
    bool captured;                  // belongs to one stream capture (capture_id): shared by the calls of that capture, never
                                    // looked up by anybody else
    unsigned long long capture_id;
    bool dirty;                     // a launch gave up: zero before the next use
    unsigned char *gran, *misc;
    size_t gran_bytes, misc_bytes;
};
struct LazyArea { int device; hipStream_t stream; unsigned tag; unsigned long long *gran; size_t cap; };
struct AreaPool { std::mutex m; std::deque<ExchangeArea> exchange; std::deque<LazyArea> lazy; std::deque<void *> retired; };
inline AreaPool &area_pool() { static AreaPool *a = new AreaPool(); return *a; }

// device memory, zeroed; legal under stream capture (the allocation is not part of the captured work:
// the thread's capture mode is relaxed around it, the zeroing runs on a stream of its own)
inline hipError_t exchange_alloc_zeroed(void **out, size_t bytes)
{
    hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
    (void)hipThreadExchangeStreamCaptureMode(&mode);
    void *ptr = nullptr;
    hipError_t e = hipMalloc(&ptr, bytes);
    if (e == hipSuccess) {
        hipStream_t zs = nullptr;
        e = hipStreamCreateWithFlags(&zs, hipStreamNonBlocking);
        if (e == hipSuccess) {
            e = hipMemsetAsync(ptr, 0, bytes, zs);
            const hipError_t e2 = hipStreamSynchronize(zs);
            if (e == hipSuccess) e = e2;
            (void)hipStreamDestroy(zs);
        }
        if (e != hipSuccess) { (void)hipFree(ptr); ptr = nullptr; }
    }
    (void)hipThreadExchangeStreamCaptureMode(&mode);
    *out = ptr;
    return e;
}

// A fresh zeroed block of `bytes` in place of `ptr`, under the pool's mutex.  The old block is retired, not freed: work queued on
// the stream may still use it.
template <class T>
hipError_t area_replace(AreaPool &P, T *&ptr, size_t bytes)
{
    void *np = nullptr;
    const hipError_t e = exchange_alloc_zeroed(&np, bytes);
    if (e != hipSuccess) return e;
    if (ptr) P.retired.push_back(ptr);
    ptr = reinterpret_cast<T *>(np);
    return hipSuccess;
}

int exchange_area_get(hipStream_t stream, size_t gran_bytes, size_t misc_bytes, unsigned char **gran, unsigned char **misc,
                      size_t *gran_have = nullptr)
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    // Under stream capture the area belongs to the CAPTURE (its id): every call captured into one graph shares it -- the
    // graph's kernel nodes run one after the other like the launches of a stream -- and a later capture gets its own (round 4
    // gave every captured CALL an area: a graph of K steps held K of them; ADVICE r4).
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    unsigned long long cid = 0;
    if (hipStreamGetCaptureInfo(stream, &cs, &cid) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; cid = 0; }
    const bool capturing = cs != hipStreamCaptureStatusNone;
    AreaPool &P = area_pool();
    std::lock_guard<std::mutex> lock(P.m);
    ExchangeArea *a = nullptr;
    for (auto &x : P.exchange)
        if (x.device == dev && x.stream == stream && x.captured == capturing && (!capturing || x.capture_id == cid)) { a = &x; break; }
    if (!a) {
        P.exchange.push_back(ExchangeArea{dev, stream, capturing, capturing ? cid : 0ull, false, nullptr, nullptr, 0, 0});
        a = &P.exchange.back();
    }
    auto grow = [&](unsigned char *&ptr, size_t &have, size_t need) -> hipError_t {
        if (have >= need) return hipSuccess;
        size_t bytes = (need + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
        if (!capturing && have > 0 && bytes < have + have / 2) bytes = have + have / 2;      // (geometric: few retired blocks)
        const hipError_t e = area_replace(P, ptr, bytes);
        if (e == hipSuccess) have = bytes;
        return e;
    };
    // (a new control block behind a grown `misc` starts at tag 1 again: `gran` must not keep granules of
    // the old block's tags -- the two grow together)
    const bool regrow = (a->gran_bytes < gran_bytes) || (a->misc_bytes < misc_bytes);
    if (regrow && (a->gran || a->misc)) {
        if (a->gran) P.retired.push_back(a->gran);
        if (a->misc) P.retired.push_back(a->misc);
        const size_t g = a->gran_bytes + a->gran_bytes / 2, m = a->misc_bytes + a->misc_bytes / 2;
        gran_bytes = gran_bytes > g ? gran_bytes : g;
        misc_bytes = misc_bytes > m ? misc_bytes : m;
        a->gran = a->misc = nullptr;
        a->gran_bytes = a->misc_bytes = 0;
    }
    hipError_t e = grow(a->gran, a->gran_bytes, gran_bytes);
    if (e == hipSuccess) e = grow(a->misc, a->misc_bytes, misc_bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); return (int)e; }
    if (a->dirty) {
        // a launch on this area gave up and the caller has cleared the status: start from zero
        e = hipMemsetAsync(a->gran, 0, a->gran_bytes, stream);
        if (e == hipSuccess) e = hipMemsetAsync(a->misc, 0, a->misc_bytes, stream);
        if (e != hipSuccess) return (int)e;
        a->dirty = false;
    }
    *gran = a->gran;
    *misc = a->misc;
    if (gran_have) *gran_have = a->gran_bytes;          // (the whole area: what a tag wrap has to zero)
    return LTR_OK;
}

// The two tag sequences that count on the host, and their wrap rules -- NOT the same rule, on purpose:
//   a lazy area's tag (below):     1, 2, ..., 0xFFFFFFFF, 1, 2, ...  The wrap skips 0 -- "never written" -- and zeroes the
//                                  granules in stream order first: one buffer, any tag that differs from the last will do.
//   a mailbox's (ltr_mailbox.inc): 1, 2, ..., 0xFFFFFFFF, 2, 3, ...  The wrap skips 0 AND 1, so that consecutive all-reduces
//                                  always alternate between the two halves (the tag's parity picks the half); round 4 wrapped
//                                  to 1 and used one half twice in a row.
__host__ __device__ inline unsigned mailbox_next_tag(unsigned prev) { const unsigned t = prev + 1u; return t ? t : 2u; }

// the next tag of the stream's lazy area and its granules (at least `count` of them)
int lazy_area_next(hipStream_t stream, size_t count, unsigned long long **gran, unsigned *tag)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return LTR_ERR_CONFIG;
    AreaPool &P = area_pool();
    std::lock_guard<std::mutex> lock(P.m);
    LazyArea *a = nullptr;
    for (auto &x : P.lazy) if (x.device == dev && x.stream == stream) { a = &x; break; }
    if (!a) { P.lazy.push_back(LazyArea{dev, stream, 0u, nullptr, 0}); a = &P.lazy.back(); }
    if (a->cap < count) {
        // (a larger buffer starts a new tag sequence on zeroed memory)
        const size_t cap = count < 4096 ? 4096 : count;
        if (area_replace(P, a->gran, cap * 8) != hipSuccess) return LTR_ERR_CONFIG;
        a->cap = cap;
        a->tag = 0u;
    }
    if (++a->tag == 0u) {
        // 2^32 launches on this area: the granules go back to zero (in stream order) before the tags start over
        if (hipMemsetAsync(a->gran, 0, a->cap * 8, stream) != hipSuccess) return LTR_ERR_CONFIG;
        a->tag = 1u;
    }
    *gran = a->gran;
    *tag = a->tag;
    return LTR_OK;
}
}  // namespace

// (called by ltr_device_status(clear) in ltr_kernels.hip once a timeout has been acknowledged)
extern "C" __attribute__((visibility("hidden"))) void ltr_internal_exchange_mark_dirty(void)
{
    AreaPool &P = area_pool();
    std::lock_guard<std::mutex> lock(P.m);
    for (auto &x : P.exchange) x.dirty = true;
}

extern "C" {
// Frees every area of the process (ltr_hip.h), the lazy steps' weight granules included: only when no launch that used one is
// in flight and no captured graph that contains one will be replayed again.
int ltr_exchange_release(void)
{
    AreaPool &P = area_pool();
    std::lock_guard<std::mutex> lock(P.m);
    for (auto &x : P.lazy) P.retired.push_back(x.gran);
    for (auto &x : P.exchange) { P.retired.push_back(x.gran); P.retired.push_back(x.misc); }
    hipError_t e = hipSuccess;
    for (void *r : P.retired)
        if (r) { const hipError_t q = hipFree(r); if (q != hipSuccess) e = q; }
    P.lazy.clear();
    P.exchange.clear();
    P.retired.clear();
    return (int)e;
}

// The tag the NEXT launch on `stream`'s exchange area will use (tests: the wrap from 2^32 - 1 to 1).
LTR_DEBUG_HOOK int ltr_debug_set_exchange_tag(void *stream, unsigned tag)
{
    unsigned char *gran = nullptr, *misc = nullptr;
    if (const int rc = exchange_area_get((hipStream_t)stream, 16, kExCtrlBytes, &gran, &misc)) return rc;
    static unsigned staged[8];
    static int slot = 0;
    unsigned *src = &staged[slot++ & 7];
    *src = tag;
    return (int)hipMemcpyAsync(misc, src, sizeof(unsigned), hipMemcpyHostToDevice, (hipStream_t)stream);
}
}  // extern "C"
