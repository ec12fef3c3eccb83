// ltr_mailbox.inc -- the mailbox all-reduce (ltr_mailbox_*, include/ltr_hip.h): its kernel, the handle, the create / connect /
// destroy calls.  Needs MailboxDev, kMbMaxRanks and lazy_area_words (ltr_linear.inc: LinearParams carries the mailbox of a
// data-parallel lazy step), mailbox_next_tag (ltr_areas.inc, next to the other tag rule), cluster_force_timeout
// (ltr_cluster.inc) and bucket_count (ltr_overlap.inc).
// ---------------------------------------------------------------------------------------------
// Mailbox all-reduce: the step's gradient bucket (F + 2 floats, < 3 KB) summed over the ranks of one node
// WITHOUT a collective library in the step -- the parts kernel's exchange, across GPUs.  Every rank owns a
// MAILBOX in fine-grained device memory, [2 parities][world][count_max] 8-byte granules, mapped into every other
// rank's address space with hipIpcGetMemHandle / hipIpcOpenMemHandle (one process per GPU).  One small kernel
// per all-reduce (one 256-thread workgroup):
//   1. thread i stores {tag, send[i]} into slot [parity][my rank][i] of EVERY peer's mailbox (system-scope 8-byte
//      stores: over xGMI for the other GPUs) -- the data is the flag;
//   2. it then takes the ranks 0 .. world-1 IN RANK ORDER, its own value from the register, the others' from its
//      own mailbox (system-scope loads until the tag is this all-reduce's), and adds them: every rank adds the
//      same numbers in the same order, so all ranks end with bit-identical sums, run after run;
//   3. recv[i] = sum; with an update target, W[i] -= lr * sum too (the optimiser step of a synchronous-SGD step:
//      ltr_linear_sgd_step_f32 saves a launch).
// The tag counts the all-reduces of this mailbox (device state: a captured launch replays with fresh tags).  Two
// parities because a peer may run ONE all-reduce ahead: it cannot finish all-reduce k + 1 before it has my k + 1
// granule, which I send only after I have read its granule of all-reduce k -- so while I still poll for k, a fast
// peer's k + 1 lands in the other half and nothing I have not read is overwritten.  Latency-bound by design: no
// rings, no protocol negotiation, one hop.  RCCL stays the fallback (and the cross-check at set-up).
// ---------------------------------------------------------------------------------------------
extern "C" {
namespace {
// how long one all-reduce waits for its peers before it gives up (a collective library's watchdog waits minutes: a
// rank may be late by a checkpoint, an evaluation pass, a stalled data loader).  LTR_MAILBOX_TIMEOUT_MS in the
// environment (read once) or ltr_mailbox_set_timeout_ms() override the default of 120 s.
inline long long *mailbox_timeout_ms()
{
    static long long v = [] { const char *e = getenv("LTR_MAILBOX_TIMEOUT_MS"); const long long x = e ? atoll(e) : 0; return x > 0 ? x : 120000ll; }();
    return &v;
}
// ... in the 100 MHz ticks the kernels count; 0 -- give up at once -- under the tests' forced time-out
inline long long mailbox_timeout_ticks() { return cluster_force_timeout() ? 0 : *mailbox_timeout_ms() * 100000ll; }
struct LtrMailbox {
    int rank, world, count_max, device;
    unsigned long long *mine;                       // [2][world][count_max]
    unsigned long long *peer[kMbMaxRanks];          // peer[r]: rank r's mailbox in MY address space (peer[rank] == mine)
    bool opened[kMbMaxRanks];
    unsigned *tag;                                  // device word: all-reduces done on this mailbox
    int *status;                                    // device status word (pinned host page) or null
    // the data-parallel LAZY steps' half of the mailbox (halves 2 and 3 of `mine`: [2][world][count_max] more granules): its
    // all-reduces happen inside the fused launch (linear_lazy_reduce), their tag is a host-side counter -- eager launches only
    unsigned lazy_tag;
    MailboxDev *dev;                                // the peers' addresses etc. in (ordinary) device memory, for those launches
    unsigned long long *lazy_gran;                  // the weight granules of those launches (kLazyCopies copies of count_max, padded)
    size_t lazy_gran_count;
    long long dev_ticks;                            // what dev->ticks holds (in stream order)
    long long stage[16];                            // host staging of ticks updates (a ring: an update is rare)
    int stage_i;
};
struct MailboxArgs {
    unsigned long long *peer[kMbMaxRanks];
    unsigned long long *mine;
    unsigned *tag;
    int *status;
    int rank, world, count_max;
    long long timeout_ticks;                        // 100 MHz ticks one all-reduce may wait for its peers; <= 0: give up at once (tests)
};

// The mailbox argument of a lazy entry point: a mailbox of one rank has nothing to exchange and counts as none ...
inline LtrMailbox *mailbox_or_none(void *mailbox) { LtrMailbox *m = reinterpret_cast<LtrMailbox *>(mailbox); return (m && m->world == 1) ? nullptr : m; }
// ... and one of several ranks must be connected, hold a step's bucket, and the step must have a bias
inline bool mailbox_unfit(const LtrMailbox *m, int F, const float *bias) { return m && (!m->dev || (size_t)m->count_max < bucket_count(F) || !bias); }

// (the tag sequence 1, 2, ..., 0xFFFFFFFF, 2, 3, ...: mailbox_next_tag, ltr_areas.inc)
__global__ void __launch_bounds__(256)
mailbox_allreduce_kernel(MailboxArgs a, const float *__restrict__ send, float *__restrict__ recv, int count,
                         float *__restrict__ w_upd, float *__restrict__ b_upd, float lr, int F)
{
    const int tid = threadIdx.x;
    const unsigned t = mailbox_next_tag((unsigned)__builtin_amdgcn_readfirstlane((int)a.tag[0]));
    const size_t half = (size_t)(t & 1u) * (size_t)a.world * (size_t)a.count_max;
    // ONE time budget for the whole all-reduce (100 MHz wall clock), shared by every peer and element: a peer that
    // never shows up costs timeout_ticks once, not once per peer and element; polls back off to ~1 us
    const long long deadline = (long long)__builtin_amdgcn_s_memrealtime() + a.timeout_ticks;
    __shared__ int s_failed;
    if (tid == 0) s_failed = 0;
    __syncthreads();
    // 1. my granules to every peer (all of them before the first poll: nobody waits for a slow sender's later elements)
    for (int i = tid; i < count; i += 256) {
        const unsigned long long g = ((unsigned long long)t << 32) | (unsigned long long)__float_as_uint(send[i]);
        for (int r = 0; r < a.world; ++r)
            if (r != a.rank)
                __hip_atomic_store(a.peer[r] + half + (size_t)a.rank * a.count_max + i, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    // 2. the sums, in rank order
    float acc[4] = {0.f, 0.f, 0.f, 0.f};                   // count <= 1024 in practice; more elements loop below
    bool ok = a.timeout_ticks > 0;                         // (tests: a zero budget fails on every rank, arrived or not)
    if (!ok) __hip_atomic_store(&s_failed, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    for (int i = tid, u = 0; i < count && ok; i += 256, ++u) {
        const float v = send[i];
        float sum = 0.f;
        for (int r = 0; r < a.world && ok; ++r) {
            float x = v;
            if (r != a.rank) {
                const unsigned long long *src = a.mine + half + (size_t)r * a.count_max + i;
                unsigned long long gv = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                int spins = 0;
                while ((unsigned)(gv >> 32) != t) {
                    if ((++spins & 15) == 0 &&
                        ((long long)__builtin_amdgcn_s_memrealtime() > deadline || __hip_atomic_load(&s_failed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))) {
                        ok = false;
                        break;
                    }
                    if (spins < 64) __builtin_amdgcn_s_sleep(2); else __builtin_amdgcn_s_sleep(32);
                    gv = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
                x = __uint_as_float((unsigned)gv);
            }
            sum += x;
        }
        if (!ok) { __hip_atomic_store(&s_failed, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); break; }
        if (u < 4) acc[u] = sum; else recv[i] = sum;        // (elements beyond 1024: stored at once, see below)
    }
    __syncthreads();
    const bool failed = s_failed != 0;
    // 3. results.  A peer that never arrived: the bucket is poisoned, the WEIGHTS ARE LEFT ALONE (round 4 wrote NaN into
    // them -- unrecoverable) and the sticky status says LTR_ERR_TIMEOUT: callers of ltr_linear_sgd_step_f32 must look
    // at ltr_device_status before they trust W after a step that may have timed out.
    for (int i = tid, u = 0; i < count; i += 256, ++u) {
        const float sum = failed ? __builtin_nanf("") : (u < 4 ? acc[u] : recv[i]);
        recv[i] = sum;
        if (w_upd && !failed) {
            if (i < F) w_upd[i] -= lr * sum;
            else if (i == F && b_upd) b_upd[0] -= lr * sum;
        }
    }
    if (failed && tid == 0 && a.status) __hip_atomic_store(a.status, (int)LTR_ERR_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (tid == 0) a.tag[0] = t;
}

int mailbox_launch(LtrMailbox *m, const float *send, float *recv, size_t count, float *w_upd, float *b_upd, float lr,
                   int F, hipStream_t stream)
{
    if (!m) return LTR_ERR_NULL;
    if (count > (size_t)m->count_max) return LTR_ERR_SHAPE;
    MailboxArgs a;
    for (int r = 0; r < kMbMaxRanks; ++r) a.peer[r] = (r < m->world) ? m->peer[r] : nullptr;
    a.mine = m->mine; a.tag = m->tag; a.status = status_device_ptr(stream);
    a.rank = m->rank; a.world = m->world; a.count_max = m->count_max;
    a.timeout_ticks = mailbox_timeout_ticks();
    hipLaunchKernelGGL(mailbox_allreduce_kernel, dim3(1), dim3(256), 0, stream, a, send, recv, (int)count, w_upd, b_upd, lr, F);
    return (int)hipGetLastError();
}
}  // namespace

// include/ltr_hip.h: the mailbox all-reduce (no counterpart in the reference: it is single-process)
int ltr_mailbox_create(int rank, int world, int count_max, void **handle, void *ipc_handle_out /* 64 bytes */)
{
    LTR_CLEAR_STALE_ERROR();
    if (!handle || !ipc_handle_out) return LTR_ERR_NULL;
    if (world < 1 || world > kMbMaxRanks || rank < 0 || rank >= world || count_max < 1) return LTR_ERR_CONFIG;
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "the IPC handle travels as 64 bytes");
    LtrMailbox *m = new LtrMailbox();
    m->rank = rank; m->world = world; m->count_max = count_max; m->device = 0;
    (void)hipGetDevice(&m->device);
    for (int r = 0; r < kMbMaxRanks; ++r) { m->peer[r] = nullptr; m->opened[r] = false; }
    const size_t bytes = 4 * (size_t)world * (size_t)count_max * 8 + 256;      // (two halves per kind of all-reduce: plain, lazy)
    m->lazy_tag = 0u; m->dev = nullptr; m->lazy_gran = nullptr; m->lazy_gran_count = 0; m->dev_ticks = -1; m->stage_i = 0;
    void *p = nullptr;
    // fine-grained: the peers' stores land without a kernel boundary, my polling loads see them
    // (no silent fall-back to coarse-grained memory: a peer's stores would not be guaranteed visible before a kernel
    // boundary -- the caller sees the error and takes the collective library instead; one rank needs no peers)
    hipError_t e = hipExtMallocWithFlags(&p, bytes, hipDeviceMallocFinegrained);
    if (e != hipSuccess && world == 1) { (void)hipGetLastError(); e = hipMalloc(&p, bytes); }
    if (e != hipSuccess) { (void)hipGetLastError(); delete m; return LTR_ERR_CONFIG; }
    if (e == hipSuccess) e = hipMemset(p, 0, bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { if (p) (void)hipFree(p); delete m; return (int)e; }
    m->mine = reinterpret_cast<unsigned long long *>(p);
    m->tag = reinterpret_cast<unsigned *>(reinterpret_cast<unsigned char *>(p) + 4 * (size_t)world * (size_t)count_max * 8);
    m->peer[rank] = m->mine;
    hipIpcMemHandle_t h;
    memset(&h, 0, sizeof(h));
    if (world > 1) {
        e = hipIpcGetMemHandle(&h, p);
        if (e != hipSuccess) { (void)hipFree(p); delete m; return (int)e; }
    }
    memcpy(ipc_handle_out, &h, 64);
    *handle = m;
    return LTR_OK;
}

int ltr_mailbox_connect(void *handle, const void *all_ipc_handles /* world x 64 bytes, rank order */)
{
    LTR_CLEAR_STALE_ERROR();
    LtrMailbox *m = reinterpret_cast<LtrMailbox *>(handle);
    if (!m || !all_ipc_handles) return LTR_ERR_NULL;
    for (int r = 0; r < m->world; ++r) {
        if (r == m->rank || m->opened[r]) continue;
        hipIpcMemHandle_t h;
        memcpy(&h, reinterpret_cast<const unsigned char *>(all_ipc_handles) + 64 * (size_t)r, 64);
        void *p = nullptr;
        const hipError_t e = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) { (void)hipGetLastError(); return (int)e; }
        m->peer[r] = reinterpret_cast<unsigned long long *>(p);
        m->opened[r] = true;
    }
    // what the lazy steps' launches read: the same addresses, in device memory
    MailboxDev h;
    memset(&h, 0, sizeof(h));
    for (int r = 0; r < m->world; ++r) h.peer[r] = m->peer[r];
    h.rank = m->rank; h.world = m->world; h.count_max = m->count_max;
    h.ticks = mailbox_timeout_ticks();         // (lazy_mailbox_next brings it up to date in front of every launch that reads it)
    if (!m->dev) { void *d = nullptr; if (hipMalloc(&d, sizeof(MailboxDev)) != hipSuccess) { (void)hipGetLastError(); return LTR_ERR_CONFIG; } m->dev = reinterpret_cast<MailboxDev *>(d); }
    if (!m->lazy_gran) {
        m->lazy_gran_count = lazy_area_words(m->count_max - 2 > 0 ? m->count_max - 2 : 1);
        void *d = nullptr;
        if (hipMalloc(&d, m->lazy_gran_count * 8) != hipSuccess) { (void)hipGetLastError(); return LTR_ERR_CONFIG; }
        if (hipMemset(d, 0, m->lazy_gran_count * 8) != hipSuccess) { (void)hipFree(d); return LTR_ERR_CONFIG; }
        m->lazy_gran = reinterpret_cast<unsigned long long *>(d);
    }
    const hipError_t ec = hipMemcpy(m->dev, &h, sizeof(h), hipMemcpyHostToDevice);
    m->dev_ticks = h.ticks;
    return ec == hipSuccess ? LTR_OK : (int)ec;
}

int ltr_mailbox_destroy(void *handle)
{
    LtrMailbox *m = reinterpret_cast<LtrMailbox *>(handle);
    if (!m) return LTR_OK;
    (void)hipDeviceSynchronize();
    for (int r = 0; r < m->world; ++r)
        if (m->opened[r] && m->peer[r]) (void)hipIpcCloseMemHandle(m->peer[r]);
    if (m->mine) (void)hipFree(m->mine);
    if (m->dev) (void)hipFree(m->dev);
    if (m->lazy_gran) (void)hipFree(m->lazy_gran);
    delete m;
    return LTR_OK;
}

long long ltr_mailbox_set_timeout_ms(long long timeout_ms)
{
    const long long old = *mailbox_timeout_ms();
    if (timeout_ms > 0) *mailbox_timeout_ms() = timeout_ms;
    return old;
}

// tests (include/ltr_hip.h)
LTR_DEBUG_HOOK int ltr_debug_mailbox_state(void *handle, long long timeout_ms, long long tag)
{
    LtrMailbox *m = reinterpret_cast<LtrMailbox *>(handle);
    if (timeout_ms > 0) *mailbox_timeout_ms() = timeout_ms;
    if (tag >= 0) {
        if (!m) return LTR_ERR_NULL;
        const unsigned t = (unsigned)tag;
        (void)hipDeviceSynchronize();
        m->lazy_tag = t;                                 // (the lazy steps' half counts on the host)
        return (int)hipMemcpy(m->tag, &t, sizeof(t), hipMemcpyHostToDevice);
    }
    return LTR_OK;
}

// an ltr_allreduce_fn (ncclFloat32 / ncclSum): comm = the mailbox handle
int ltr_mailbox_allreduce(const void *sendbuf, void *recvbuf, size_t count, int dtype, int op, void *comm, void *stream)
{
    if (dtype != 7 || op != 0) return 1;
    return mailbox_launch(reinterpret_cast<LtrMailbox *>(comm), (const float *)sendbuf, (float *)recvbuf, count, nullptr, nullptr,
                          0.f, 0, (hipStream_t)stream) == 0 ? 0 : 1;
}
}  // extern "C"
