// ltr_linear.inc -- Linear(F,1) scorer fused with the pairwise loss: LinearParams, the kernels, their shape choosers and
// launchers (included by ltr_linear.hip; the host side of the step is in ltr_linear_step.inc and the files listed there).
// One workgroup per query runs the whole training-step slice
//     scores = X[b] . W + bias  ->  loss[b], d loss/d scores  ->  dW_b = (go_b * g)^T X[b]
// (examples/01-basic-usage.py:70-75 in the reference: loss_fn(model(xs), ys, n).mean().backward()
// with model = torch.nn.Linear(F, 1)).
//
// Two kernels share the pipeline.  linear_regtile2_kernel (below) is the fast path: the whole
// tile lives in VGPRs and crosses HBM once.  linear_pairwise_kernel is the general one:
//   phase 1  GEMV, one wave per document row: lanes stride the row in 16-byte vectors, the
//            wave reduces with DPP.  Only rows l < n[b] are read (padded documents can never
//            contribute: their d loss/d score is 0), unless the caller asks for the full
//            score matrix.
//   phase 2  the same pair pass as the stand-alone loss kernel.
//   phase 3  dW_b: threads laid out (row r, column-vector c) over the flat tile, so a
//            workgroup-iteration reads R consecutive rows as one contiguous span; the rows
//            are re-read (L2 / Infinity Cache / HBM).  Parking the tile in LDS, with or
//            without an LDS-DMA copy and a persistent work queue, was measured slower at
//            every shape (DESIGN.md section 4) and removed.
//   then     per-query partials (B x (F+1)) are summed by a second small kernel --
//            deterministic, no float atomics.
// This is HBM-bound work (arithmetic intensity ~0.5 flop/byte): no MFMA, the N=1 output
// column makes it a bandwidth problem.

namespace {

constexpr int kP1Unr = 4;
constexpr int kP3Unr = 4;
constexpr int kLinearThreads = 512;

// (the per-query partial rows: partial_pitch, ltr_common.inc)

// The mailbox of a data-parallel lazy step as the device sees it (ltr_mailbox_*, ltr_mailbox.inc; here because LinearParams carries it): a small struct in this rank's
// own device memory -- every rank's mailbox mapped into THIS address space, who I am, the granules per (parity, rank) slot.
constexpr int kMbMaxRanks = 16;
struct MailboxDev {
    unsigned long long *peer[kMbMaxRanks];          // peer[r]: rank r's mailbox here (peer[rank] == mine)
    int rank, world, count_max, pad;
    long long ticks;                                // 100 MHz ticks an in-launch all-reduce waits for its peers; <= 0: give up at once
};
// what a reducer publishes instead of a weight when its all-reduce gave up: a quiet NaN no arithmetic produces
constexpr unsigned kLazyPoison = 0x7fc0deadu;

#define LTR_KARG __attribute__((address_space(4)))       // the kernarg segment's address space (constant)
struct LinearParams {
    const float *X;
    const float *W;
    const float *bias;
    const void *rel;
    const int64_t *n;
    float *loss;
    float *scores_out;
    float *part;        // (B, partial_pitch(F)) per-query partials, see partial_pitch
    int B, L, F;
    float sigma;
    int rel_dtype;
    int msplit;
    int rows_r;         // R: rows handled per workgroup-iteration in phase 3
    int sched;          // > 0: number of 64-query sample groups of the list-length scheduling (low 16 bits); bits 16 and up, register
                        // tile: the CUs of the device when the rounds of workgroups are dealt in snake order, else 0
    // LAZY synchronous SGD (ltr_linear_sgd_lazy_step_f32; register-tile kernel only): pend_B > 0 -- `part` / `loss` still hold
    // the partial rows / losses of the PREVIOUS batch (pend_B queries) whose update has not been applied: the first workgroups
    // reduce them (one column each: the arithmetic of linear_reduce_kernel, bit for bit), apply W -= lr * dW in place and
    // publish the new weights as {tag, value} granules; every workgroup takes its weights from the granules, behind its tile burst
    int part_g = 0;                     // != 0: `part` is written column-group major (the lazy step's private layout, below)
    int pend_B = 0;
    int pend_g = 0;                     // the pending batch's rows are column-group major
    int pend_nred = 0;                  // reducer workgroups in front of the grid: ceil((F + 1) / 4) of four columns + 1 (losses)
    float pend_lr = 0.f, pend_w = 0.f;  // learning rate, uniform weight 1 / pend_B of the pending batch's queries
    const float *pend_wptr = nullptr;   // != null: query b's weight is pend_wptr[b * pend_wstride] instead of pend_w (the upstream
    int pend_wstride = 0;               // gradient as autograd hands it over: `.sum()`'s expanded scalar, `.mean()`'s vector of 1 / B)
    int pend_general = 0;               // != 0: the reducers' general form (a weight pointer, a mailbox, no weights); 0: the
                                        // single-process step's lean one
    float *pend_W = nullptr, *pend_bias = nullptr;      // the weights, writable
    float *pend_out = nullptr;          // dW (F) | db | sum of the losses of the pending batch
    unsigned long long *pend_gran = nullptr;            // (F + 2) granules: tag << 32 | weight bits (the last one: the losses are read) (library-owned, zero when allocated)
    int pend_sleep = 0;                 // the queries' workgroups hold their tile burst back for pend_sleep x 512 cycles
    int pend_gstride = 0;               // granules per copy (kLazyCopies copies: one per XCD)
    unsigned pend_tag = 0;              // this launch's tag (host-side counter of the lazy area: eager launches only)
    int *status = nullptr;              // process status word or null
    int spin_limit = 0;
    // DATA-PARALLEL lazy step (ltr_linear_sgd_lazy_step_dp_f32): the reducers all-reduce their column sums over the ranks through
    // the mailbox's lazy half before they publish the weights; the losses' reducer is then the ONE writer of W / bias
    // (pend_gran / pend_tag are then the MAILBOX's granules and the tag of its lazy half: one host-side counter for both)
    const MailboxDev *pend_mb = nullptr;
};

#include "ltr_trace.inc"          // tuning hooks: every macro of it is empty in the product build
// LDS layout of the general fused kernel (bytes), after the query block of loss_lds_bytes():
//   wl    float[F4]           W
//   gfin  float[L4]           d loss[b] / d s_l
//   dred  float[R * F4]       phase-3 cross-row reduction
// (Ls = LDS row stride: L rounded to 4, or to 64-wide tiles for the symmetric pass; slices =
// gradient slices: msplit, or waves per workgroup for the symmetric pass)
__host__ __device__ inline size_t linear_lds_bytes(int kind, int Ls, int F, int slices, int R)
{
    const size_t L4 = (size_t)Ls;
    const size_t F4 = (size_t)((F + 3) & ~3);
    size_t bytes = loss_lds_bytes(kind, Ls, slices);
    bytes = (bytes + 15) & ~(size_t)15;
    bytes += 4 * F4 + 4 * L4 + 4 * (size_t)R * F4;
    return (bytes + 15) & ~(size_t)15;
}

// DPT == 0: symmetric pair pass (L <= kSymMaxLen), LDS rows padded to 64-wide tiles and one
// gradient slice per wave; DPT in {1, 4}: both-ends pass.  Block size is a launch parameter
// (512, or 1024 when the batch is too small to fill the CUs with 512-thread workgroups).
template <int KIND, int DPT, int VEC>
__device__ __forceinline__ void linear_pairwise_body(const LinearParams &p);

// (The symmetric and one-row passes under 64 VGPRs -- eight waves per SIMD, four 512-thread workgroups per CU instead of three, two
// of 1024 threads instead of one: left alone the 16-byte-row instantiations take 70 and run seven.  One to three spilled VGPRs
// each; hinge 4096 x 300 x 64 114.6 -> 100.6 us, 8192 x 400 x 48 308 -> 277, 16 384 x 300 x 32 439 -> 392, logistic / LambdaARP2
// 4096 x 300 x 64 146 -> 133.  Round 6.)
template <int KIND, int DPT, int VEC>
__global__ void __launch_bounds__(1024, (DPT <= 1 ? 8 : 4))
linear_pairwise_kernel(LinearParams p)
{
    linear_pairwise_body<KIND, DPT, VEC>(p);
}

// The instantiations that need <= 64 VGPRs but 84-105 SGPRs left to themselves (the LambdaNDCG kinds' symmetric and one-row passes,
// the hinge kinds' one-row pass on 4-byte rows): more than 80 SGPRs hold SEVEN waves per SIMD (4.6 of DESIGN.md) -- ONE 1024-thread
// workgroup per CU instead of two.  Capped: LambdaNDCG2 1024 x 128 x 45 23.3 -> 19.4 us, 8192 queries 140 -> 128, LambdaNDCG1
// 8192 x 100 x 45 130 -> 113 (round 6).  (The attribute wants a literal: an entry point of its own around the same body.)
template <int KIND, int DPT, int VEC>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_num_sgpr(80)))
linear_pairwise_kernel80(LinearParams p)
{
    linear_pairwise_body<KIND, DPT, VEC>(p);
}
template <int KIND, int DPT, int VEC>
constexpr auto linear_pairwise_entry()
{
    if constexpr (((KIND == LTR_NDCG1 || KIND == LTR_NDCG2) && DPT <= 1) || ((KIND == LTR_HINGE || KIND == LTR_DCG_HINGE) && DPT == 1 && VEC == 1))
        return &linear_pairwise_kernel80<KIND, DPT, VEC>;
    else return &linear_pairwise_kernel<KIND, DPT, VEC>;
}

template <int KIND, int DPT, int VEC>
__device__ __forceinline__ void linear_pairwise_body(const LinearParams &p)
{
    using V = typename VecT<VEC>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int L = p.L, F = p.F;
    int b, nb;
    if (p.sched) {
        b = sched_query_sampled(p.n, p.B, L, p.sched & 0xffff, (int)threadIdx.x, nb, (int)blockIdx.x, p.sched >> 16);
    } else {
        b = (int)blockIdx.x;
        nb = clamp_n(p.n[b], L);
    }
    constexpr bool kSym = (DPT == 0);
    const int L4 = kSym ? ((L + 63) & ~63) : ((L + 3) & ~3);     // LDS row stride of the query block
    const int F4 = (F + 3) & ~3;
    const int C = F / VEC;                        // column vectors per row
    const int tid = threadIdx.x;
    const int T = blockDim.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int nwaves = T >> 6;
    const int msplit = kSym ? (T >> 6) : p.msplit;
    const int R = p.rows_r;

    const QueryLds q = carve_query_lds<KIND>(smem, L4, msplit);
    size_t off = (loss_lds_bytes(KIND, L4, msplit) + 15) & ~(size_t)15;
    float *wl = reinterpret_cast<float *>(smem + off);
    float *gfin = wl + F4;
    float *dred = gfin + L4;

    const size_t row = (size_t)b * L;
    const float *Xq = p.X + row * (size_t)F;

    for (int f = tid; f < F; f += T) wl[f] = p.W[f];
    stage_labels(q.sy, p.rel, p.rel_dtype, row, L, nb, tid, T);
    if (KIND == LTR_NDCG1 || KIND == LTR_NDCG2)
        for (int m = tid; m < 2 * L4; m += T) q.rank_s[m] = 0;
    const float bias = p.bias ? p.bias[0] : 0.f;
    __syncthreads();

    // ---- phase 1: scores = X.W + bias, one wave per row, 4 rows in flight per wave ----
    {
        const int nrows = p.scores_out ? L : nb;
        const V *wv = reinterpret_cast<const V *>(wl);
        constexpr int UNR = kP1Unr;
        for (int l0 = wave; l0 < nrows; l0 += nwaves * UNR) {
            float acc[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) acc[u] = 0.f;
            for (int c = lane; c < C; c += 64) {
                V x[UNR];
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    const int l = l0 + u * nwaves;
                    x[u] = (l < nrows) ? reinterpret_cast<const V *>(Xq + (size_t)l * F)[c] : vzero<V>();
                }
                const V w = wv[c];
#pragma unroll
                for (int u = 0; u < UNR; ++u) acc[u] += vdot(x[u], w);
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int l = l0 + u * nwaves;
                const float s = wave_sum(acc[u]) + bias;
                if (lane == 0 && l < nrows) {
                    if (l < nb) q.sy[l].x = s;
                    if (p.scores_out) p.scores_out[row + l] = s;
                }
            }
        }
    }
    __syncthreads();

    // ---- phase 2: pair pass ----
    float gscale, gsum = 0.f;
    float total;
    if constexpr (kSym) {
        if (KIND == LTR_NDCG1 || KIND == LTR_NDCG2) {
            int owners = 64;
            while (owners < L4 && owners < T) owners *= 2;
            const int ms = T / owners;
            const int mlen = (nb + ms - 1) / ms;
            const int m0 = __builtin_amdgcn_readfirstlane(min(nb, (tid / owners) * mlen));
            const int m1 = __builtin_amdgcn_readfirstlane(min(nb, m0 + mlen));
            prepare_ndcg<KIND, 1>(q, nb, owners, tid % owners, m0, m1, ms > 1);
        }
        total = pairwise_core_sym<KIND>(q, nb, L4, p.sigma, gscale);
    } else {
        total = pairwise_core<KIND, (DPT > 0 ? DPT : 1)>(q, nb, L4, msplit, p.sigma, gscale, gsum);
    }
    // (the loss is stored at the end of the kernel: a store in front of a __syncthreads() makes its wave wait for the
    // acknowledgement, and the other waves for that wave)
    float gs = 0.f;
    for (int k = tid; k < nb; k += T) {
        float g = 0.f;
        for (int s = 0; s < msplit; ++s) g += q.gpart[(size_t)s * L4 + k];
        g *= gscale;
        gfin[k] = g;
        gs += g;
    }
    if (kSym) gsum = block_sum(gs, q.red);        // d/d bias; its barriers also publish gfin
    else __syncthreads();

    // ---- phase 3: dW_b[f] = sum_l gfin[l] * X[b,l,f] ----
    float *part = p.part + (size_t)b * partial_pitch(F);    // this query's row of the partials
    {
        // columns are processed in tiles of CT = min(C, T) column vectors (one tile unless the
        // row is wider than the workgroup), R row groups per tile
        const int CT = C < T ? C : T;
        const int cl = tid % CT;
        const int r = tid / CT;
        for (int c0 = 0; c0 < C; c0 += CT) {
            const int c = c0 + cl;
            if (r < R && c < C) {
                V acc = vzero<V>();
                constexpr int UNR = kP3Unr;
                for (int l0 = r; l0 < nb; l0 += R * UNR) {
                    V x[UNR];
                    float g[UNR];
#pragma unroll
                    for (int u = 0; u < UNR; ++u) {
                        const int lf = l0 + u * R;
                        const bool ok = lf < nb;
                        // rows in REVERSE: the rows phase 1 streamed last are the likeliest to be
                        // still in L2 / Infinity Cache (C5 full lists 264 -> 249 us)
                        const int l = ok ? nb - 1 - lf : 0;
                        g[u] = ok ? gfin[l] : 0.f;
                        x[u] = ok ? reinterpret_cast<const V *>(Xq + (size_t)l * F)[c] : vzero<V>();
                    }
#pragma unroll
                    for (int u = 0; u < UNR; ++u) vfma(acc, g[u], x[u]);
                }
                reinterpret_cast<V *>(dred)[(size_t)r * CT + cl] = acc;
            }
            __syncthreads();
            if (tid < CT && c0 + tid < C) {
                V s = vzero<V>();
                for (int rr = 0; rr < R; ++rr) vadd(s, reinterpret_cast<const V *>(dred)[(size_t)rr * CT + tid]);
                const int cc = c0 + tid;
                reinterpret_cast<V *>(part)[cc] = s;          // coalesced: consecutive threads, consecutive columns
            }
            lds_barrier();          // (dred is rewritten by the next tile; nobody waits for the row's store)
        }
        if (tid == 0) {
            part[F] = gsum;
            for (int f = F + 1; f < partial_pitch(F); ++f) part[f] = 0.f;
            p.loss[b] = total;
        }
    }
}


// ---------------------------------------------------------------------------------
// Register-resident single-pass variant -- the fast path for MSLR-class shapes.
// Chosen when one 512-thread workgroup can hold a whole query tile in VGPRs.
//   * FLAT mapping: the n[b] real rows of a query are one contiguous span of n[b]*F floats;
//     thread t owns the 16-byte vectors t, t + R*C, t + 2*R*C, ... of that span (C = F/4 column
//     vectors per row, R = 512 / C rows per sweep).  Every wave-load is 1 KiB of contiguous
//     memory, the thread's column c = t % C never changes, and the WHOLE tile is requested in
//     one burst -- one HBM round trip per query instead of a batched row loop;
//   * scores: per-thread partial dots (the thread's W vector lives in registers) go through a
//     padded LDS matrix, a quad of lanes per row folds them with two DPP adds;
//   * the features STAY in registers through the pair pass; dW is then NI FMAs per thread
//     (same column, NI rows) and one LDS fold over the R row groups.
// Features cross HBM exactly once and never touch LDS.  Four workgroups (32 waves) per CU:
// some compute while the others' loads are in flight.
// ---------------------------------------------------------------------------------
constexpr int kRegtileMinW = 6;       // waves/SIMD the register allocator must allow (<= 80 VGPRs)
constexpr int kRegtileThreads = 512;       // measured sweet spot on MI355X (256..1024 swept)

// the lists the register tile takes: the symmetric pair pass's (LDS rows padded to 64-wide tiles, one slice per wave)
__host__ __device__ inline bool regtile_sym(int L) { return L <= 256; }

__device__ __forceinline__ float4 f4_scale(float4 v, float g) { return make_float4(v.x * g, v.y * g, v.z * g, v.w * g); }

// ---------------------------------------------------------------------------------
// Register tile (lists up to 256 documents: the symmetric pair pass).  The round-1 version of this kernel
// (linear_regtile_kernel, retired in round 4) had the same mapping and arithmetic; what changed is everything
// around it, from the instruction trace of the first version (profiles/r02_regtile_trace.txt: the
// launch was as much VALU-issue- as HBM-bound -- ~3.5 k VALU wave-instructions per query of which
// the pair pass needs < 1 k -- and two dependent HBM round trips sat in front of the first feature
// load):
//   * the feature loads are BUFFER loads through a descriptor whose size is the query's n[b] real
//     rows: rows past the end return 0 in hardware -- no per-load predicate, no branch, no 64-bit
//     address arithmetic (one 32-bit offset add per load);
//   * load order W -> features -> labels: the label fetch no longer sits (with its own wait) in
//     front of the features, it comes back behind them and is needed only by the pair pass;
//   * CT = F / 4 as a template parameter for the common feature counts: rows per sweep, LDS
//     pitches and every loop bound of the score fold / dW fold are compile-time, the folds are
//     unrolled LDS reads behind ONE wait instead of a wait per element;
//   * the partial-dot matrix has a pitch = 4 (mod 8) words, conflict-free for the quad-per-row fold;
//   * the gradient vector is zero-filled past n[b], so the dW pass needs no predicates either.
// ---------------------------------------------------------------------------------
__host__ __device__ inline int regtile2_cp(int C) { return ((C + 3) & ~7) + 4; }

__host__ __device__ inline size_t regtile2_lds_bytes(int kind, int L, int F, int NI, int T)
{
    const size_t L4 = (size_t)((L + 63) & ~63);
    const size_t C = (size_t)F / 4;
    const size_t R = (size_t)T / C;
    size_t bytes = (loss_lds_bytes(kind, (int)L4, T / 64) + 15) & ~(size_t)15;
    const size_t Lg = ((size_t)NI * R + 3) & ~(size_t)3;
    const size_t pd = 4 * (size_t)L * (size_t)regtile2_cp((int)C);
    const size_t dr = 16 * (size_t)T + 4 * R;
    // (behind them: the weights of a lazy step as they arrive, F + 2 floats)
    return bytes + 4 * Lg + (((pd > dr ? pd : dr) + 15) & ~(size_t)15) + 4 * (((size_t)F + 2 + 3) & ~(size_t)3);
}

constexpr int kLazyCopies = 8;          // copies of a lazy step's weight granules: one per XCD (readers spread over the channels)
// A lazy area, in 8-byte words, every one of them a (launch tag << 32 | float) pair written with one store: the weight granules,
// kLazyCopies copies of F + 2.  A word counts only under the tag of the launch that reads it, so the shapes that share a stream's
// area may lay it out differently: what another launch left is stale by its tag, wherever it lies.
__host__ __device__ inline size_t lazy_area_words(int F)
{
    return (size_t)kLazyCopies * (size_t)((F + 2 + 15) & ~15) + 8;
}


// TT threads per workgroup: 512 (eight waves, <= 80 VGPRs: four workgroups per CU), or 256 with
// twice the sweeps per thread for the kinds whose per-wave fixed cost is high (the NDCG kinds:
// two rankings + gains per query -- C3 fused kernel 19.5 -> 17.4 us; hinge 11.2 -> 11.4, so the
// rank-free kinds keep 512)
// NI = 19 at TT = 512 (round 4): the lists the 9- / 12-sweep tiles cannot hold, at <= 128 VGPRs (two workgroups per
// CU) -- see choose_regtile_shape.  (A 1024-thread tile of nine sweeps was built for the same lists first: 8-9 % slower
// than 19 sweeps, EXPERIMENTS.md.)
// a * b rounded to fp32 on its own: the product is opaque to the compiler, which may not contract it with the sum behind it
// (__fmul_rn is a plain multiplication in HIP)
__device__ __forceinline__ float mul_rounded(float a, float b)
{
    float t = a * b;
    asm volatile("" : "+v"(t));
    return t;
}

// LAZY step, a reducer workgroup (no query of its own): block j sums the columns 4j .. 4j + 3 of the pending batch's partial
// rows (16-byte loads; column F is the bias column, the row pitch pads with zeros), the last reducer the per-query losses --
// every column exactly as linear_reduce_kernel sums it (256 threads: rows t, t + 256, ... four at a time, products rounded on
// their own, DPP wave sums, (w0 + w1) + (w2 + w3)) --, applies the update in place and publishes the new weights as granules.
// (The eight 16-byte groups of a 128-byte line on ONE XCD -- linear_reduce_kernel's trick -- LOSES here: 14.26 -> 14.95 us per
// step at C2; the reducers then sit on five of the eight XCDs, eight to an XCD, in front of those XCDs' queries.)
// DATA PARALLEL: one column's sum over the ranks, through the mailbox's lazy half (mailbox_allreduce_kernel's protocol, one column
// per thread): my {tag, sum} into slot [parity][my rank][f] of EVERY peer -- the data is the flag --, then the ranks IN RANK ORDER,
// mine from the register, the others' polled out of my own mailbox: every rank adds the same numbers in the same order, so all
// ranks publish bit-identical weights.  Returns the sum, or the poison pattern when a peer did not arrive within `ticks` (the
// status word is raised).  Only a reducer's four threads ever get here.  (As a real call -- `noinline` -- it made things worse: the
// callee-saved convention put stack frames into 70 kernels; EXPERIMENTS.md round 6.)
__device__ __forceinline__ float lazy_dp_allreduce(const MailboxDev *mbp, unsigned tag, int f, float sres, int *status)
{
    const MailboxDev &mb = *mbp;
    const long long ticks = mb.ticks;
    const int world = mb.world, me = mb.rank, cm = mb.count_max;
    const size_t half = (size_t)(2u + (tag & 1u)) * (size_t)world * (size_t)cm;      // (halves 2, 3: the lazy steps')
    const unsigned long long g = ((unsigned long long)tag << 32) | (unsigned long long)__float_as_uint(sres);
    for (int r = 0; r < world; ++r)
        if (r != me) __hip_atomic_store(mb.peer[r] + half + (size_t)me * cm + f, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const long long deadline = (long long)__builtin_amdgcn_s_memrealtime() + ticks;
    bool ok = ticks > 0;                                 // (tests: a zero budget fails on every rank, arrived or not)
    float sum = 0.f;
    for (int r = 0; r < world && ok; ++r) {
        float x = sres;
        if (r != me) {
            const unsigned long long *src = mb.peer[me] + half + (size_t)r * cm + f;
            unsigned long long gv = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            int spins = 0;
            while ((unsigned)(gv >> 32) != tag) {
                if ((++spins & 15) == 0 && (long long)__builtin_amdgcn_s_memrealtime() > deadline) { ok = false; break; }
                if (spins < 64) __builtin_amdgcn_s_sleep(2); else __builtin_amdgcn_s_sleep(32);
                gv = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            x = __uint_as_float((unsigned)gv);
        }
        sum += x;
    }
    if (!ok && status) __hip_atomic_store(status, (int)LTR_ERR_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return ok ? sum : __uint_as_float(kLazyPoison);
}

// GENERAL = false: the single-process step with the uniform weight 1 / B -- the headline's reducers, nothing else on their path (the
// weights' hand-over is on the critical path of every workgroup of the launch: the selects and skipped branches of the general form
// cost the C2 step 0.3 us); true: an upstream gradient read from the device and / or the all-reduce over the ranks.
template <bool GENERAL>
__device__ __forceinline__ void linear_lazy_reduce_t(const LinearParams &p, float *red, const int nt /* threads of the workgroup */)
{
    const int tid = threadIdx.x;
    const int F = p.F;
    const int bx = (int)blockIdx.x;
    const bool losses = bx == p.pend_nred - 1;
    const int r0 = 0, r1 = p.pend_B;                 // (one round of workgroups at most: lazy_layout_g)
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tid < 256) {
        if (!losses) {
            // (the pending rows in the layout their step wrote: column-group major -- contiguous per reducer -- or by query)
            const float4 *col = reinterpret_cast<const float4 *>(p.part) + (p.pend_g ? (size_t)bx * (size_t)p.pend_B : (size_t)bx);
            const size_t pitch4 = p.pend_g ? 1 : ((size_t)partial_pitch(F) >> 2);
            for (int b0 = r0 + tid; b0 < r1; b0 += 1024) {
                float4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { const int bb = b0 + 256 * u; v[u] = (bb < r1) ? col[(size_t)bb * pitch4] : make_float4(0.f, 0.f, 0.f, 0.f); }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int bq = b0 + 256 * u;
                    float wq = (bq < r1) ? p.pend_w : 0.f;
                    if constexpr (GENERAL) { if (p.pend_wptr && bq < r1) wq = p.pend_wptr[(size_t)bq * (size_t)p.pend_wstride]; }
                    acc.x += mul_rounded(v[u].x, wq); acc.y += mul_rounded(v[u].y, wq);
                    acc.z += mul_rounded(v[u].z, wq); acc.w += mul_rounded(v[u].w, wq);
                }
            }
        } else {
            for (int i = r0 + tid; i < r1; i += 256) acc.x += p.loss[i];
        }
        acc.x = wave_sum(acc.x); acc.y = wave_sum(acc.y); acc.z = wave_sum(acc.z); acc.w = wave_sum(acc.w);
        if ((tid & 63) == 0) reinterpret_cast<float4 *>(red)[tid >> 6] = acc;
    }
    lds_barrier();
    if (GENERAL && p.pend_mb) {
        // DATA PARALLEL: the four column sums all-reduced over the ranks (LDS in, LDS out: red[20 .. 23])
        if (tid < 4) {
            const int f = losses ? F + 1 : 4 * bx + tid;
            if ((!losses && f <= F) || (losses && tid == 0))
                red[20 + tid] = lazy_dp_allreduce(p.pend_mb, p.pend_tag, f,
                                                  (red[tid] + red[4 + tid]) + (red[8 + tid] + red[12 + tid]), p.status);
        }
        lds_barrier();
    }
    const bool dp = GENERAL && p.pend_mb != nullptr;
    if (tid < 4) {
        const int f = losses ? F + 1 : 4 * bx + tid;
        if ((!losses && f <= F) || (losses && tid == 0)) {
            float sres = dp ? red[20 + tid] : (red[tid] + red[4 + tid]) + (red[8 + tid] + red[12 + tid]);
            const bool ok = !dp || __float_as_uint(sres) != kLazyPoison;
            if (!ok) sres = __builtin_nanf("");
            p.pend_out[f] = sres;                                      // dW[f] | db | loss sum
            float wnew = sres;
            if (f <= F && (!GENERAL || p.pend_W)) {                    // (no weights: the reduction alone)
                float *wp = (f < F) ? p.pend_W + f : p.pend_bias;
                wnew = __builtin_fmaf(-p.pend_lr, sres, wp[0]);
                // (data parallel: the weights have ONE writer, the losses' reducer below, once it has seen every column arrive --
                // a peer that never came leaves W / bias untouched as a whole)
                if (!dp) wp[0] = wnew;
            }
            red[16 + tid] = ok ? wnew : __uint_as_float(kLazyPoison);
        }
    }
    lds_barrier();
    // (the losses' column too: a query's workgroup overwrites loss[b] and its partial row at its end -- it waits for EVERY
    // column's granule in front of its dot products, so nothing of the pending batch is read after it is rewritten)
    // (Measured and dropped, round 6, same box: the stores straight from the four threads that computed the weights -- a barrier
    // less -- and the old weight's load issued at the reducer's start: each costs the C2 step 0.25 us, 12.97 -> 13.2 .. 13.3.)
    if (p.pend_gran && tid < 4 * kLazyCopies) {
        const int u = tid & 3, copy = tid >> 2;
        const int f = losses ? F + 1 : 4 * bx + u;
        if ((!losses && f <= F) || (losses && u == 0))
            __hip_atomic_store(p.pend_gran + (size_t)copy * p.pend_gstride + f, ((unsigned long long)p.pend_tag << 32) | __float_as_uint(red[16 + u]),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (dp && losses && p.pend_gran) {
        // DATA PARALLEL: the weights have ONE writer -- this workgroup, the losses' reducer -- once EVERY column's granule of this
        // launch is there and none of them is poison (a reducer whose all-reduce gave up): a peer that never came leaves W / bias
        // untouched as a whole.  (The reducers are the first workgroups of the grid, all resident: nothing to wait for but them.)
        lds_barrier();
        if (tid == 0) red[24] = 0.f;
        lds_barrier();
        const unsigned long long *g0 = p.pend_gran;              // (copy 0)
        bool bad = false;
        for (int g = tid; g < F + 2; g += nt) {
            int spins = 0;
            for (;;) {
                const unsigned long long gv = __hip_atomic_load(g0 + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((unsigned)(gv >> 32) == p.pend_tag) { bad = bad || (unsigned)gv == kLazyPoison || p.spin_limit < 0; break; }
                if (++spins > p.spin_limit) { bad = true; break; }
                __builtin_amdgcn_s_sleep(2);
            }
        }
        if (bad) red[24] = 1.f;
        lds_barrier();
        if (red[24] == 0.f)
            for (int g = tid; g <= F; g += nt) {
                const unsigned long long gv = __hip_atomic_load(g0 + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                float *wp = (g < F) ? p.pend_W + g : p.pend_bias;
                wp[0] = __uint_as_float((unsigned)gv);
            }
    }
}

__device__ __forceinline__ void linear_lazy_reduce(const LinearParams &p, float *red, const int nt)
{
    if (p.pend_general) linear_lazy_reduce_t<true>(p, red, nt);
    else linear_lazy_reduce_t<false>(p, red, nt);
}

// ltr_linear_sgd_flush_f32 on rows in the lazy step's layout: the reducers on their own (no granules)
// the weights of this launch from XCD copy `copy` of the granules, one granule per thread, into wst (LDS)
template <int T>
__device__ __forceinline__ void linear_lazy_poll_weights(const LinearParams &p, float *wst, unsigned copy, int tid)
{
    const int F = p.F;
    const unsigned long long *g0 = p.pend_gran + (size_t)(copy & (kLazyCopies - 1)) * p.pend_gstride;
    bool bad = false;
    for (int g = tid; g < F + 2; g += T) {
        unsigned long long gv = 0ull;
        int spins = 0;
        for (;;) {
            gv = __hip_atomic_load(g0 + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((unsigned)(gv >> 32) == p.pend_tag && p.spin_limit >= 0) break;      // (< 0, tests: give up whatever arrives)
            // (data parallel: spin_limit = INT_MAX -- the reducers may wait for a late peer as long as the mailbox's budget says
            // and ALWAYS publish, weights or poison, so the readers do not give up on their own)
            if (++spins > p.spin_limit) { bad = true; gv = 0x7fc000007fc00000ull; break; }       // (NaN: the step is invalid)
            __builtin_amdgcn_s_sleep(2);
        }
        wst[g] = __uint_as_float((unsigned)gv);
    }
    if (bad && p.status) __hip_atomic_store(p.status, (int)LTR_ERR_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ void __launch_bounds__(256)
linear_lazy_flush_kernel(LinearParams p)
{
    __shared__ float red[32];
    linear_lazy_reduce(p, red, 256);
}

// (the SGPR cliff, round 6: a wave's SGPRs are allocated in sixteens and the trap handler takes sixteen more, so with more than 80
// the 800 SGPRs of a SIMD hold SEVEN waves, not eight -- three 512-thread workgroups per CU instead of four, a quarter of C2's
// queries waits for a slot: 11.7 -> 13.3 us with 82 SGPRs and not one instruction changed on the hot path)
// Two entry points share the body: linear_regtile2_kernel -- the shapes that run EIGHT waves per SIMD (the rank-free kinds on 3 / 5 / 9
// sweeps of 512 threads: four workgroups per CU), compiled under caps of 64 VGPRs and 80 SGPRs -- and
// linear_regtile2w_kernel, everything else
// (fewer waves per SIMD by their VGPRs: no cap).  regtile2_entry picks.
template <int KIND, int NI, int CT, int TT>
__device__ __forceinline__ void linear_regtile2_body(const LinearParams &p);

template <int KIND, int NI, int CT, int TT>
__global__ void __launch_bounds__(TT, 8) __attribute__((amdgpu_num_sgpr(80)))          // eight waves per SIMD: <= 64 VGPRs, <= 80 SGPRs
linear_regtile2_kernel(LinearParams p)
{
    linear_regtile2_body<KIND, NI, CT, TT>(p);
}

template <int KIND, int NI, int CT, int TT>
__global__ void __launch_bounds__(TT, (TT == 512 && NI < 19 ? kRegtileMinW : 4))
linear_regtile2w_kernel(LinearParams p)
{
    linear_regtile2_body<KIND, NI, CT, TT>(p);
}

template <int KIND, int NI, int CT, int TT>
constexpr auto regtile2_entry()
{
    // (The generic-width tiles too -- every feature count but 136: left alone they take 68-69 VGPRs, seven waves per SIMD, three
    // workgroups per CU; under the cap they need 44 (three / five sweeps) or 64 (nine) and nothing spills but five VGPRs of the
    // DCG-hinge ones.  Round 6, same box, us: hinge 1024 x 64 x 220 12.9 -> 11.2, 1024 x 80 x 220 15.5 -> 13.1, 1024 x 128 x 64
    // 13.3 -> 11.1, 1024 x 128 x 128 14.8 -> 12.7, 4096 x 80 x 220 40.0 -> 36.1, logistic 1024 x 80 x 220 16.3 -> 13.6, DCG-hinge
    // 15.6 -> 13.1, LambdaARP2 4096 x 128 x 64 39.6 -> 37.4.  The first version of the cap excluded them as "seven waves either way".)
    if constexpr (KIND != LTR_NDCG1 && KIND != LTR_NDCG2 && TT == 512 && NI <= 9) return &linear_regtile2_kernel<KIND, NI, CT, TT>;
    else return &linear_regtile2w_kernel<KIND, NI, CT, TT>;
}

template <int KIND, int NI, int CT, int TT>
__device__ __forceinline__ void linear_regtile2_body(const LinearParams &p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int T = TT;
    const int L = p.L;
    LTR_TRACE_ENTRY();
    // LAZY step (p.pend_B > 0): the first pend_nred workgroups of the grid carry no query -- they reduce the pending batch's
    // partial rows, one column each, and leave (linear_lazy_reduce); the queries follow behind them
    const bool lazy = p.pend_B > 0;
    const int qblock = (int)blockIdx.x - (lazy ? p.pend_nred : 0);
    if (lazy && qblock < 0) {
        // The reducers read THEIR kernel arguments here, from the kernarg segment, behind a pointer the compiler cannot see through:
        // left to itself it loads every argument any path uses in the entry block, and the two dozen words only the reducers need
        // push the entry over the 80 SGPRs of eight waves per SIMD (spilled SGPRs take a VGPR for the whole kernel -- the 65th).
        const LTR_KARG unsigned char *ka = (const LTR_KARG unsigned char *)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ka));
        LinearParams pr;
#define LTR_KA(field) pr.field = *reinterpret_cast<const LTR_KARG decltype(pr.field) *>(ka + offsetof(LinearParams, field))
        LTR_KA(part); LTR_KA(loss); LTR_KA(F); LTR_KA(pend_B); LTR_KA(pend_g); LTR_KA(pend_nred); LTR_KA(pend_lr); LTR_KA(pend_w);
        LTR_KA(pend_wptr); LTR_KA(pend_wstride); LTR_KA(pend_general); LTR_KA(pend_W); LTR_KA(pend_bias); LTR_KA(pend_out);
        LTR_KA(pend_gran); LTR_KA(pend_gstride); LTR_KA(pend_tag); LTR_KA(status); LTR_KA(spin_limit); LTR_KA(pend_mb);
#undef LTR_KA
        LTR_TRACE_REDUCER(0);
        linear_lazy_reduce(pr, reinterpret_cast<float *>(smem), TT);
        LTR_TRACE_REDUCER(1);
        return;
    }
    // (a head start for the reducers: their scattered 4-byte loads take microseconds once a thousand tile bursts are in the
    // queues in front of them, and every workgroup then waits for the weights -- C2 14.9 -> 15.9 us; on an idle memory
    // system they are done in about one, which is what the queries' bursts are held back for)
    // (two hold-backs in one word: the low byte for everybody, the next one -- != 0: the quiet rule is on -- for the QUIET
    // workgroups, the ones on the reducers' own CUs, sched_quiet, whose bursts would sit in the very memory queue the reducer's
    // loads and granule stores go through; they carry the batch's shortest lists, sched_slot, and can afford to start last)
    const int qhold = lazy ? p.pend_sleep >> 8 : 0;
    if (lazy) {
        const int hold = (qhold && sched_quiet((int)blockIdx.x, p.sched >> 16, p.pend_nred)) ? qhold : (p.pend_sleep & 0xff);
        for (int i = 0; i < hold; ++i) __builtin_amdgcn_s_sleep(8);
    }
    int b, nb;
    if (p.sched) {
        // (the block id and the reducers in front of it: the dealing goes by the CU slot that hosts the id, sched_slot_cu)
        b = sched_query_sampled(p.n, p.B, L, p.sched & 0xffff, (int)threadIdx.x, nb, (int)blockIdx.x, p.sched >> 16,
                                lazy ? p.pend_nred : 0, qhold != 0);
    } else {
        b = qblock;
        nb = clamp_n(p.n[b], L);
    }
    const int C = CT > 0 ? CT : (p.F >> 2);         // column vectors per row
    const int F = C << 2;
    const int R = T / C;                            // rows per sweep
    const int CP = regtile2_cp(C);                  // pitch of the partial-dot matrix (words)
    const int L4 = (L + 63) & ~63;                  // LDS row stride of the query block
    const int tid = threadIdx.x;
    constexpr int msplit = T >> 6;
    const bool active = tid < R * C;
    const int rq = tid / C;
    const int c = tid - rq * C;                     // (inactive threads: a valid column, r below never matches)
    const int r = active ? rq : (1 << 20);

    const QueryLds q = carve_query_lds<KIND>(smem, L4, msplit);
    size_t off = (loss_lds_bytes(KIND, L4, msplit) + 15) & ~(size_t)15;
    const int Lg = (NI * R + 3) & ~3;
    float *gfin = reinterpret_cast<float *>(smem + off);      // [Lg] d loss / d s, 0 past n[b]
    float *pd = gfin + Lg;                                    // [L][CP] partial dots ...
    float4 *dred = reinterpret_cast<float4 *>(pd);            // ... later [T] dW partials
    float *bred = reinterpret_cast<float *>(dred + T);        // [R] d/d bias partials
    const size_t row = (size_t)b * L;
    LTR_STAMP2(0);
    LTR_TRACE_PLACEMENT();

    // ---- W, then the whole tile in one burst, then the labels (needed last) ----
    // (a LAZY step takes them from the granules, behind the burst)
    float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
    float bias = 0.f;
    if (!lazy) {
        w = reinterpret_cast<const float4 *>(p.W)[c];
        bias = p.bias ? p.bias[0] : 0.f;
    }
    // (descriptor inputs through readfirstlane: the compiler must be able to PROVE them wave-uniform,
    // or it wraps every buffer load in a waterfall loop)
    const uintptr_t xaddr = reinterpret_cast<uintptr_t>(p.X + row * (size_t)F);
    const unsigned xlo = __builtin_amdgcn_readfirstlane((unsigned)xaddr);
    const unsigned xhi = __builtin_amdgcn_readfirstlane((unsigned)(xaddr >> 32));
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<void *>(((uintptr_t)xhi << 32) | xlo), 0,
        __builtin_amdgcn_readfirstlane(nb * F * 4), 0x00020000);
    const int voff = active ? tid * 16 : 0x7ffffff0;           // out of range -> 0
    const int sweep = R * C * 16;                              // bytes per sweep
    float4 x[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const ltr_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff + i * sweep, 0, 0);
        x[i] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
    }
    // L <= T: one label per thread, fetched raw as two 32-bit words by two unconditional loads (for
    // the 4-byte dtypes the second one repeats the first) -- no dtype-dependent control flow, hence
    // no copy or conversion that would make the compiler wait for the label right here; the
    // conversion happens after the dot products (below)
    int ylo = 0, yhi = 0;
    {
        const int wide = (p.rel_dtype == LTR_LABEL_I64) ? 1 : 0;
        const int *rp = reinterpret_cast<const int *>(p.rel) + ((row + (size_t)min(tid, L - 1)) << wide);
        ylo = rp[0];
        yhi = rp[wide];
    }
    if (KIND == LTR_NDCG1 || KIND == LTR_NDCG2)
        for (int m = tid; m < 2 * L4; m += T) q.rank_s[m] = 0;
    LTR_STAMP2(7);

    if (lazy) {
        // the weights: F + 2 granules (columns, bias, the losses' column -- read, so that nothing of the pending batch is
        // rewritten before it has been summed), one per thread, from this XCD's copy, until they carry this launch's tag;
        // then through LDS to everybody.  (Every thread polling its own four columns was 2.6 M coherent loads on nine lines
        // per launch: C2 14.8 -> 21.4 us.)
        {
            const size_t pdb = (size_t)4 * L * CP, drb = (size_t)16 * T + 4 * R;           // (regtile2_lds_bytes)
            float *wst = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(pd) + (((pdb > drb ? pdb : drb) + 15) & ~(size_t)15));
            unsigned xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            linear_lazy_poll_weights<T>(p, wst, xcc, tid);
            lds_barrier();
            LTR_STAMP2(11);
            w = reinterpret_cast<const float4 *>(wst)[c];
            bias = wst[F];
        }
    }

    // ---- scores: partial dots -> LDS, quad per row folds them ----
    {
        float *pdw = pd + (active ? rq : 0) * CP + c;        // row r, column c; sweeps are R * CP words apart
#pragma unroll
        for (int i = 0; i < NI; ++i)
            if (r < nb - i * R) pdw[i * R * CP] = vdot_pk(x[i], w);
    }
    // (opaque to the scheduler: the conversion -- and with it the wait for the label, the LAST load
    // of the burst -- stays behind the dot products, which consume the tile as it arrives)
    asm volatile("" : "+v"(ylo), "+v"(yhi));
    if (tid < nb) {
        if (p.rel_dtype != LTR_LABEL_I64) yhi = ylo >> 31;
        const long long y64 = ((long long)yhi << 32) | (unsigned)ylo;
        q.sy[tid].y = (p.rel_dtype == LTR_LABEL_F32) ? __int_as_float(ylo) : (float)y64;
    }
    __syncthreads();
    LTR_STAMP2(1);
    {
        const int h = tid & 3;
        for (int l = tid >> 2; l < nb; l += T >> 2) {
            const float *pr = pd + l * CP + h;
            float acc = 0.f;
            if (CT > 0) {
                float v[(CT + 3) / 4 > 0 ? (CT + 3) / 4 : 1];
#pragma unroll
                for (int k = 0; k < (CT + 3) / 4; ++k) v[k] = (4 * k + 3 < CT || h + 4 * k < CT) ? pr[4 * k] : 0.f;
#pragma unroll
                for (int k = 0; k < (CT + 3) / 4; ++k) acc += v[k];
            } else {
                for (int cc = h; cc < C; cc += 4) acc += pr[cc - h];
            }
            acc = quad_sum(acc);
            if (h == 0) q.sy[l].x = acc + bias;
        }
    }
    __syncthreads();
    LTR_STAMP2(2);

    // ---- pair pass ----
    float gscale;
    if constexpr (KIND == LTR_NDCG1 || KIND == LTR_NDCG2) {
        int owners = 64;
        while (owners < L4 && owners < T) owners *= 2;
        const int ms = T / owners;
        const int mlen = (nb + ms - 1) / ms;
        const int m0 = __builtin_amdgcn_readfirstlane(min(nb, (tid / owners) * mlen));
        const int m1 = __builtin_amdgcn_readfirstlane(min(nb, m0 + mlen));
        prepare_ndcg<KIND, 1, msplit, true>(q, nb, owners, tid % owners, m0, m1, ms > 1);
    }
    LTR_STAMP2(3);
    // (integer label dtypes: the hinge kinds take the sign of a label difference from one v_med3)
    const bool intlab = (KIND == LTR_HINGE || KIND == LTR_DCG_HINGE) && p.rel_dtype != LTR_LABEL_F32;
    const float total = intlab ? pairwise_core_sym<KIND, msplit, true, true>(q, nb, L4, p.sigma, gscale LTR_SYM_TRACE_ARGS)
                               : pairwise_core_sym<KIND, msplit, true, false>(q, nb, L4, p.sigma, gscale LTR_SYM_TRACE_ARGS);
    LTR_STAMP2(4);
    // (the loss is stored at the very end: a store in front of a __syncthreads() -- which carries a fence -- makes its wave wait
    // for the acknowledgement, and the other waves for that wave)
    for (int k = tid; k < Lg; k += T) {
        float g = 0.f;
        if (k < nb) {
#pragma unroll
            for (int s = 0; s < msplit; ++s) g += q.gpart[s * L4 + k];
            g *= gscale;
        }
        gfin[k] = g;
    }
    __syncthreads();
    LTR_STAMP2(5);

    // ---- dW_b: same column, NI rows per thread, straight from the registers; the bias is the
    // feature column of ones (threads of column 0 also sum their rows' gradients) ----
    {
        const int rr = active ? rq : 0;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        float gb = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const float g = gfin[rr + i * R];
            vfma(acc, g, x[i]);
            gb += g;
        }
        dred[tid] = acc;                           // (inactive threads hold zeros)
        if (active && c == 0) bred[rr] = gb;
    }
    __syncthreads();
    {
        // column vector j of the query's row: the R row groups' float4 partials, in order; thread C
        // adds the bias column.  One coalesced 16-byte store per thread, C + 1 threads.
        // (part_g, the lazy step's rows: column GROUP major -- float4 [C + 1][B], group g of query b at g * B + b -- so that the
        // reducers of the next launch read whole lines instead of a 16-byte piece out of every row; else the query's row)
        float4 *part4 = p.part_g ? reinterpret_cast<float4 *>(p.part) + b
                                 : reinterpret_cast<float4 *>(p.part + (size_t)b * partial_pitch(F));
        const size_t gpitch = p.part_g ? (size_t)p.B : 1;
        if (tid < C) {
            float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;
            if (CT > 0) {
                constexpr int RS = T / (CT > 0 ? CT : 1);
#pragma unroll
                for (int rr = 0; rr < RS; ++rr) { if (rr & 1) vadd(s1, dred[rr * CT + tid]); else vadd(s0, dred[rr * CT + tid]); }
            } else {
                int rr = 0;
                for (; rr + 1 < R; rr += 2) { vadd(s0, dred[rr * C + tid]); vadd(s1, dred[(rr + 1) * C + tid]); }
                if (rr < R) vadd(s0, dred[rr * C + tid]);
            }
            vadd(s0, s1);
            part4[(size_t)tid * gpitch] = s0;
        }
        // (the bias column from a thread that always exists: C == T when a row has as many column
        // vectors as the workgroup has threads)
        if (tid == (C < T ? C : T - 1)) {
            float sb = 0.f;
            for (int rr = 0; rr < R; ++rr) sb += bred[rr];
            part4[(size_t)C * gpitch] = make_float4(sb, 0.f, 0.f, 0.f);
        }
    }
    if (tid == 0) p.loss[b] = total;
    LTR_STAMP2(6);
}

// Launch-geometry ceiling of the register-tile kernel (bench.py `roofline.launch_ceiling`): the SAME grid
// (one workgroup per query), the same workgroup size and the same ragged spans -- thread t buffer-loads
// the 16-byte vectors t, t + T, ... of the query's n[b] * F real floats, NI in flight -- and nothing else:
// the vectors are summed (so that the loads stay) and every wave stores one dword.  What this takes is what
// ONE ROUND of workgroups can stream at all at this batch size; the fused kernel is judged against it.
template <int NI, int TT>
__global__ void __launch_bounds__(TT)
stream_probe_kernel(const float *__restrict__ X, const int64_t *__restrict__ n, int L, int F, float *__restrict__ out)
{
    const int b = (int)blockIdx.x;
    const int tid = threadIdx.x;
    const int nb = clamp_n(n[b], L);
    const uintptr_t xaddr = reinterpret_cast<uintptr_t>(X + (size_t)b * L * (size_t)F);
    const unsigned xlo = __builtin_amdgcn_readfirstlane((unsigned)xaddr);
    const unsigned xhi = __builtin_amdgcn_readfirstlane((unsigned)(xaddr >> 32));
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<void *>(((uintptr_t)xhi << 32) | xlo), 0,
        __builtin_amdgcn_readfirstlane(nb * F * 4), 0x00020000);
    ltr_u32x4 v[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) v[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, tid * 16, i * TT * 16, 0);
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < NI; ++i)
        acc += (__uint_as_float(v[i].x) + __uint_as_float(v[i].y)) + (__uint_as_float(v[i].z) + __uint_as_float(v[i].w));
    acc = wave_sum(acc);
    if ((tid & 63) == 0) out[(size_t)b * (TT / 64) + (tid >> 6)] = acc;
}

// out[f] = sum_b go[b] * part[b, f] for f in [0, F] (column F is d/d bias); go == NULL means the
// uniform weight `uniform` (1/B for `.mean().backward()`).  One 256-thread workgroup per column:
// thread t takes rows t, t + 256, ... (4-byte loads a row pitch apart -- the 16 columns of a 64-byte
// line are read by 16 different workgroups, the line comes from L2 / Infinity Cache once it has
// been touched; a column-tiled variant with 16-byte loads and 18 workgroups took 4.5 us instead of
// 2.3: too few CUs for a latency-bound kernel).  Fixed order: deterministic.  The extra last
// workgroup totals the per-query losses.
__global__ void __launch_bounds__(256)
linear_reduce_kernel(const float *__restrict__ part, const float *__restrict__ go, float uniform,
                     int B, int F, int PF, float *__restrict__ dW, float *__restrict__ db,
                     const float *__restrict__ loss, float *__restrict__ loss_sum, int accumulate,
                     float *__restrict__ w_upd = nullptr, float *__restrict__ b_upd = nullptr, float lr = 0.f,
                     int go_stride = 1)
{
    __shared__ float red[4];
    const int tid = threadIdx.x;
    // Which column: the 16 columns of one 64-byte line go to workgroups of ONE XCD (block ids are
    // dealt round-robin over the 8 XCDs, each with its own L2), so a line is fetched into one L2
    // instead of eight -- placement only decides speed (4.3 -> 2.6 us), never the result.
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int f = 16 * (xcd + 8 * (slot >> 4)) + (slot & 15);
    const bool is_loss = ((int)blockIdx.x == (int)gridDim.x - 1) && loss_sum != nullptr;
    if (!is_loss && f > F) return;
    float acc = 0.f;
    if (is_loss) {
        for (int i = tid; i < B; i += 256) acc += loss[i];
    } else {
        const float *col = part + f;
        for (int b = tid; b < B; b += 1024) {              // four independent loads in flight
            float v[4], w[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int bb = b + 256 * u;
                v[u] = (bb < B) ? col[(size_t)bb * PF] : 0.f;
                w[u] = (bb < B) ? (go ? go[(size_t)bb * go_stride] : uniform) : 0.f;      // (stride 0: one device scalar for all)
            }
            // (product and sum rounded separately: linear_lazy_reduce takes the same sums inside the next step's launch and
            // must arrive at the same bits whatever the compiler would contract -- mul_rounded)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc += mul_rounded(v[u], w[u]);
        }
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        const float s = (red[0] + red[1]) + (red[2] + red[3]);
        if (is_loss) loss_sum[0] = accumulate ? loss_sum[0] + s : s;
        else if (f < F) {
            const float g = accumulate ? dW[f] + s : s;
            dW[f] = g;
            // (single-GPU SGD step: the optimiser's W -= lr * dW rides in the reduction -- the thread that owns
            // the column owns its weight; examples/01-basic-usage.py:74-75)
            if (w_upd) w_upd[f] = __builtin_fmaf(-lr, g, w_upd[f]);
        } else {
            const float g = accumulate ? db[0] + s : s;
            db[0] = g;
            if (b_upd) b_upd[0] = __builtin_fmaf(-lr, g, b_upd[0]);
        }
    }
}


// The same reduction for batches beyond kReduceSplitMin queries, where linear_reduce_kernel's one workgroup per column walks
// B / 256 rows per thread in a chain of load latencies (65 536 queries: 125 us for 36 MB of rows -- 0.3 TB/s).  Two launches:
//   linear_reduce_rows_kernel     workgroup s of S sums ITS rows [s * chunk, (s + 1) * chunk), whole rows, coalesced: thread t owns
//                                 the 16-byte column group t % CG (CG = PF / 4) of the rows t / CG, t / CG + RPS, ...
//                                 (RPS = 256 / CG rows per sweep, four sweeps in flight), then the RPS row lanes of a column group
//                                 are added in lane order out of LDS -> scratch[s][0 .. PF) and the chunk's losses -> scratch[s][PF]
//   linear_reduce_combine_kernel  one workgroup per column group (and one for the losses): the S scratch rows, one per thread
//                                 (S <= kReduceMaxSplit = 1024: four per thread), butterfly over the wave, the four waves in order;
//                                 then linear_reduce_kernel's ending (accumulate, the SGD update riding along)
// Fixed mapping, fixed order: deterministic, run to run and whatever the grid's placement.  The sums differ from
// linear_reduce_kernel's in the last bits (another association), like any two batch sizes' do.
constexpr int kReduceSplitMin = 4096;
constexpr int kReduceMaxSplit = 1024;
__host__ __device__ inline int reduce_scratch_pitch(int PF) { return PF + 4; }

__global__ void __launch_bounds__(256)
linear_reduce_rows_kernel(const float *__restrict__ part, const float *__restrict__ go, float uniform, int go_stride, int B, int PF,
                          int chunk, const float *__restrict__ loss, float *__restrict__ scratch)
{
    __shared__ float4 lanes[256];
    __shared__ float lred[4];
    const int tid = threadIdx.x;
    const int CG = PF >> 2, RPS = 256 / CG;
    const int r0 = (int)blockIdx.x * chunk, r1 = min(B, r0 + chunk);
    const int cg = tid % CG, lane = tid / CG;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane < RPS) {
        const float4 *base = reinterpret_cast<const float4 *>(part) + cg;
        for (int r = r0 + lane; r < r1; r += 4 * RPS) {
            float4 v[4];
            float w[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int rr = r + u * RPS;
                const bool ok = rr < r1;
                v[u] = ok ? base[(size_t)rr * (size_t)CG] : make_float4(0.f, 0.f, 0.f, 0.f);
                w[u] = ok ? (go ? go[(size_t)rr * (size_t)go_stride] : uniform) : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                acc.x += mul_rounded(v[u].x, w[u]); acc.y += mul_rounded(v[u].y, w[u]);
                acc.z += mul_rounded(v[u].z, w[u]); acc.w += mul_rounded(v[u].w, w[u]);
            }
        }
    }
    lanes[tid] = acc;
    float ls = 0.f;
    if (loss) for (int i = r0 + tid; i < r1; i += 256) ls += loss[i];
    ls = wave_sum(ls);
    if ((tid & 63) == 0) lred[tid >> 6] = ls;
    __syncthreads();
    float *out = scratch + (size_t)blockIdx.x * (size_t)reduce_scratch_pitch(PF);
    if (tid < CG) {
        float4 t = lanes[tid];
        for (int k = 1; k < RPS; ++k) { const float4 o = lanes[tid + k * CG]; t.x += o.x; t.y += o.y; t.z += o.z; t.w += o.w; }
        reinterpret_cast<float4 *>(out)[tid] = t;
    }
    if (tid == 0) out[PF] = (lred[0] + lred[1]) + (lred[2] + lred[3]);
}

__global__ void __launch_bounds__(256)
linear_reduce_combine_kernel(const float *__restrict__ scratch, int S, int F, int PF, float *__restrict__ dW, float *__restrict__ db,
                             float *__restrict__ loss_sum, int accumulate, float *__restrict__ w_upd, float *__restrict__ b_upd, float lr)
{
    __shared__ float4 red[4];
    const int tid = threadIdx.x;
    const int cg = (int)blockIdx.x;               // column group; PF / 4 = the losses (one float: the pitch keeps four)
    const int SP = reduce_scratch_pitch(PF);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = tid; k < S; k += 256) {
        const float4 v = *reinterpret_cast<const float4 *>(scratch + (size_t)k * SP + 4 * cg);
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    acc.x = wave_sum(acc.x); acc.y = wave_sum(acc.y); acc.z = wave_sum(acc.z); acc.w = wave_sum(acc.w);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid < 4) {
        const float *r = reinterpret_cast<const float *>(red);
        const float s = (r[tid] + r[4 + tid]) + (r[8 + tid] + r[12 + tid]);
        const int f = 4 * cg + tid;
        if (4 * cg == PF) {
            if (tid == 0 && loss_sum) loss_sum[0] = accumulate ? loss_sum[0] + s : s;
        } else if (f < F) {
            const float g = accumulate ? dW[f] + s : s;
            dW[f] = g;
            if (w_upd) w_upd[f] = __builtin_fmaf(-lr, g, w_upd[f]);
        } else if (f == F) {
            const float g = accumulate ? db[0] + s : s;
            db[0] = g;
            if (b_upd) b_upd[0] = __builtin_fmaf(-lr, g, b_upd[0]);
        }
    }
}

// the reduction of row-major partial rows, whichever kernel the batch size calls for (every entry point's launch site)
inline int launch_linear_reduce(hipStream_t stream, const float *part, const float *go, float uniform, int go_stride, int B, int F,
                                float *dW, float *db, const float *loss, float *loss_sum, int accumulate,
                                float *w_upd, float *b_upd, float lr)
{
    const int PF = partial_pitch(F);
    const int CG = PF >> 2;
    if (B >= kReduceSplitMin && CG <= 256) {
        const int RPS = 256 / CG;
        int S = (B + 4 * RPS - 1) / (4 * RPS);
        if (S > kReduceMaxSplit) S = kReduceMaxSplit;
        const int chunk = (B + S - 1) / S;
        S = (B + chunk - 1) / chunk;
        // (the scratch rows: in the caller's workspace, behind the rows -- linear_partials_bytes)
        float *scratch = const_cast<float *>(part) + ((((size_t)B * (size_t)PF * sizeof(float)) + 255) & ~(size_t)255) / sizeof(float);
        hipLaunchKernelGGL(linear_reduce_rows_kernel, dim3((unsigned)S), dim3(256), 0, stream, part, go, uniform, go_stride, B, PF, chunk,
                           loss_sum ? loss : (const float *)nullptr, scratch);
        hipLaunchKernelGGL(linear_reduce_combine_kernel, dim3((unsigned)(CG + (loss_sum ? 1 : 0))), dim3(256), 0, stream,
                           (const float *)scratch, S, F, PF, dW, db, loss_sum, accumulate, w_upd, b_upd, lr);
        return (int)hipGetLastError();
    }
    // column f -> block id 8 * (16 * (f / 128) + f % 16) + (f / 16) % 8: whole groups of 128 columns
    const int blocks = 128 * ((F + 1 + 127) / 128);
    hipLaunchKernelGGL(linear_reduce_kernel, dim3((unsigned)(blocks + (loss_sum ? 1 : 0))), dim3(256), 0, stream, part, go, uniform, B, F, PF,
                       dW, db, loss, loss_sum, accumulate, w_upd, b_upd, lr, go_stride);
    return (int)hipGetLastError();
}

// W -= lr * bucket[0 .. F), bias -= lr * bucket[F]: the optimiser step behind the gradient all-reduce of a
// data-parallel step (one small launch; at one rank the update rides in linear_reduce_kernel instead)
__global__ void __launch_bounds__(256)
sgd_update_kernel(float *__restrict__ W, float *__restrict__ bias, const float *__restrict__ bucket, float lr, int F)
{
    const int f = (int)(blockIdx.x * 256 + threadIdx.x);
    if (f < F) W[f] -= lr * bucket[f];
    else if (f == F && bias) bias[0] -= lr * bucket[F];
}

// tests: "the other rank's bucket" added in-stream (ltr_debug_fake_allreduce)
__global__ void __launch_bounds__(256)
fake_allreduce_kernel(const float *__restrict__ send, float *__restrict__ recv, const float *__restrict__ other, size_t count)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) recv[i] = send[i] + other[i];
}

struct LinearShape { int dpt, msplit, R, threads; size_t lds; };

bool choose_linear_shape(int kind, int B, int L, int F, int vec, LinearShape &s)
{
    // 512-thread workgroups; 1024 when the batch cannot even give every CU two of those; 256 once every CU has eight queries -- what
    // bounds the launch then is the number of queries a CU has in flight (ltr_kernels.hip: choose_loss_shape).  Round 6, 512 -> 256
    // threads, us: hinge 2048 x 300 x 64 51.6 -> 47.2, 4096 x 300 x 64 100.6 -> 88.1, 16 384 x 300 x 32 392 -> 316, 2048 x 128 x 45
    // 26.4 -> 20.2, 65 536 x 128 x 45 751 -> 496, LambdaNDCG2 16 384 x 128 x 45 259 -> 181; at 1024 queries 29.6 -> 41.9 and
    // 15.3 -> 16.0: not below eight per CU.  (128 threads: 65 536 x 128 x 45 439, but 4096 x 600 x 32 204 -> 259.)
    const int cus = device_cu_count();
    const int T = (B <= 2 * cus) ? 1024 : (B >= 8 * cus ? 256 : kLinearThreads);
    s.threads = T;
    const int C = F / vec;
    const int CT = C < T ? C : T;               // column vectors per phase-3 tile
    s.R = T / CT;
    if (s.R > 64) s.R = 64;
    int Ls, slices;
    if (L <= kSymMaxLen) {
        // symmetric pair pass: rows padded to 64-wide tiles, one gradient slice per wave
        s.dpt = 0;
        Ls = (L + 63) & ~63;
        slices = T / 64;
        s.msplit = slices;
    } else {
        // both-ends pass: owners = smallest power-of-two multiple of 64 covering L (capped at T)
        int owners = 64;
        while (owners < L && owners < T) owners *= 2;
        s.dpt = (L > owners) ? 4 : 1;
        s.msplit = T / owners;
        Ls = (L + 3) & ~3;
        slices = s.msplit;
    }
    s.lds = linear_lds_bytes(kind, Ls, F, slices, s.R);
    while (s.dpt != 0 && s.lds > kLdsBudget && s.msplit > 1) {
        s.msplit /= 2;
        s.lds = linear_lds_bytes(kind, Ls, F, s.msplit, s.R);
    }
    while (s.lds > kLdsBudget && s.R > 1) {         // very wide rows: shrink the phase-3 fan-out
        s.R /= 2;
        s.lds = linear_lds_bytes(kind, Ls, F, s.dpt == 0 ? slices : s.msplit, s.R);
    }
    return s.lds <= kLdsBudget;
}

template <int KIND, int VEC>
int launch_linear_kind(const LinearParams &p, const LinearShape &s, hipStream_t stream)
{
    const dim3 grid((unsigned)p.B), block((unsigned)s.threads);
#define LTR_LAUNCH(D)                                                                           \
    do {                                                                                        \
        constexpr auto entry = linear_pairwise_entry<KIND, D, VEC>();                           \
        LTR_ENSURE_LDS((*entry), s.lds);                                                        \
        hipLaunchKernelGGL(entry, grid, block, s.lds, stream, p);                               \
    } while (0)
    if (s.dpt == 0) LTR_LAUNCH(0);
    else if (s.dpt == 1) LTR_LAUNCH(1);
    else LTR_LAUNCH(4);
#undef LTR_LAUNCH
    return (int)hipGetLastError();
}

template <int VEC>
int launch_linear(int kind, const LinearParams &p, const LinearShape &s, hipStream_t stream)
{
    return with_kind(kind, [&](auto K) { return launch_linear_kind<K, VEC>(p, s, stream); });
}



// NI sweeps of `threads` threads (512, or the NDCG kinds' 256), `lds` bytes of dynamic LDS
struct RegtileShape { int ni, threads; size_t lds; };

bool choose_regtile_shape(int kind, int L, int F, RegtileShape &s)
{
    // (lists beyond the symmetric pass: cluster / parts / general kernel)
    if (F % 4 != 0 || !regtile_sym(L)) return false;
    const int C = F / 4;
    if (C > kRegtileThreads) return false;
    const bool ndcg = (kind == LTR_NDCG1 || kind == LTR_NDCG2);
    const int R = kRegtileThreads / C;
    const int ni = (L + R - 1) / R;
    s.threads = kRegtileThreads;
    if (ni <= 3) s.ni = 3;
    else if (ni <= 5) s.ni = 5;
    else if (ni <= 9) s.ni = 9;
    // 12 sweeps (F = 136: lists up to 180) for the rank-free kinds: 1024 x 160 x 136 hinge 26.2 -> 21.0 us,
    // logistic 28.6 -> 23.7 against the two-pass kernel; LambdaNDCG2 35.5 -> 39.0, and 19 sweeps
    // (lists up to 285) lose for every kind (1024 x 256 x 136 hinge 35 -> 52): occupancy
    else if (ni <= 12 && !ndcg) s.ni = 12;
    else {
        // Round 4: NINETEEN sweeps on the 512-thread workgroups -- lists of up to 256 documents at F = 136 (171 at
        // F = 220) -- at <= 128 VGPRs, i.e. two workgroups per CU instead of four: these shapes fell to the two-pass
        // general kernel (features read twice).  Cold, general -> 19 sweeps (hinge / logistic / LambdaNDCG2, us):
        //   1024 x 200 x 136 28.8 / 31.1 / 38.0 -> 20.3 / 24.6 / 29.8     1024 x 256 x 136 34.3 / 39.3 / 47.0 -> 22.4 / 28.7 / 34.9
        //   512 x 256 x 136 25.8 / 29.6 / 37.3 -> 14.1 / 19.0 / 22.8      1024 x 160 x 220 30.4 / 32.4 / 38.5 -> 22.5 / 26.0 / 31.5
        // (round 1 had measured 19 sweeps as a loss -- under the 80 VGPRs of four workgroups per CU they spill; a
        // 1024-thread tile of nine sweeps, two per CU, was built first this round and is 8-9 % slower than this one:
        // 24.4 us at 1024 x 256 x 136 -- and 45 % slower than the 512-thread tile on shapes that one holds, EXPERIMENTS.md;
        // the NDCG kinds on it are slower than the general kernel)
        // (24 sweeps: 216 documents at F = 220 -- Istella-S reaches 182 -- in 116-121 VGPRs for the rank-free kinds; the
        // NDCG kinds spill 4-12 registers under the 128 there and still beat the two-pass kernel: 1024 x 200 x 220
        // LambdaNDCG1 / 2 43.9 / 44.6 -> 37.5 / 39.5 us, 512 x 200 x 220 40.9 -> 24.9)
        const int nsw = (ni <= 19) ? 19 : ((ni <= 24) ? 24 : 0);
        if (nsw == 0) return false;
        s.ni = nsw;
        s.lds = regtile2_lds_bytes(kind, L, F, nsw, kRegtileThreads);
        return s.lds <= 78 * 1024;
    }
    if (ndcg && C <= 256) {
        // 256-thread workgroups, up to 19 sweeps in registers
        const int R2 = 256 / C;
        const int ni2 = (L + R2 - 1) / R2;
        const int n2 = ni2 <= 5 ? 5 : (ni2 <= 9 ? 9 : (ni2 <= 12 ? 12 : (ni2 <= 19 ? 19 : 0)));
        if (n2 > 0) {
            const size_t lds256 = regtile2_lds_bytes(kind, L, F, n2, 256);
            if (lds256 <= 40 * 1024) { s.threads = 256; s.ni = n2; s.lds = lds256; return true; }
        }
    }
    s.lds = regtile2_lds_bytes(kind, L, F, s.ni, kRegtileThreads);
    return s.lds <= 64 * 1024;
}

struct KernelEvents { bool armed; hipEvent_t start, stop; };
inline KernelEvents &kernel_events() { static thread_local KernelEvents e = {false, nullptr, nullptr}; return e; }

// One launch of the register tile, NI sweeps of TT threads.  `ke` (or null): the start / stop event pair ltr_debug_kernel_events
// armed -- recorded by the command processor right at the kernel's begin and end (bench.py's live duration of the lazy launch) --,
// for the 512-thread tiles of 3 / 5 / 9 sweeps only: any other tile is a plain launch and leaves the events unrecorded.
template <int KIND, int NI, int CT, int TT>
int launch_regtile2_tt(const LinearParams &p, size_t lds, const KernelEvents *ke, hipStream_t stream)
{
    constexpr auto entry = regtile2_entry<KIND, NI, CT, TT>();
    const dim3 grid((unsigned)(p.B + (p.pend_B > 0 ? p.pend_nred : 0)));        // (a lazy step: the reducer workgroups in front)
    if constexpr (TT == kRegtileThreads && NI >= 19) LTR_ENSURE_LDS((*entry), lds);       // (up to 78 KiB of LDS)
    if constexpr (TT == kRegtileThreads && NI <= 9) {
        if (ke) {
            hipExtLaunchKernelGGL(entry, grid, dim3(TT), (unsigned)lds, stream, ke->start, ke->stop, 0, p);
            return (int)hipGetLastError();
        }
    }
    hipLaunchKernelGGL(entry, grid, dim3(TT), lds, stream, p);
    return (int)hipGetLastError();
}

// The tiles there are: 512 threads on 3 / 5 / 9 / 19 / 24 sweeps, and on 12 for the rank-free kinds (choose_regtile_shape sends
// the NDCG kinds from nine sweeps straight to nineteen); 256 threads on 5 / 9 / 12 / 19 sweeps for the NDCG kinds only.
template <int KIND, int NI, int CT>
int launch_regtile2_ni(const LinearParams &p, const RegtileShape &s, const KernelEvents *ke, hipStream_t stream)
{
    constexpr bool ndcg = (KIND == LTR_NDCG1 || KIND == LTR_NDCG2);
    if (s.threads == 256) {
        if constexpr (ndcg && NI != 3 && NI != 24) return launch_regtile2_tt<KIND, NI, CT, 256>(p, s.lds, nullptr, stream);
        else return LTR_ERR_CONFIG;
    }
    if constexpr (ndcg && NI == 12) return LTR_ERR_CONFIG;
    else return launch_regtile2_tt<KIND, NI, CT, kRegtileThreads>(p, s.lds, ke, stream);
}

template <int KIND, int CT>
int launch_regtile2_ct(const LinearParams &p, const RegtileShape &s, hipStream_t stream)
{
    // (the measurement hook serves the next launch of the tile, whichever: every launch disarms it)
    KernelEvents &events = kernel_events();
    const KernelEvents *ke = events.armed ? &events : nullptr;
    events.armed = false;
    switch (s.ni) {
    case 3: return launch_regtile2_ni<KIND, 3, CT>(p, s, ke, stream);
    case 5: return launch_regtile2_ni<KIND, 5, CT>(p, s, ke, stream);
    case 9: return launch_regtile2_ni<KIND, 9, CT>(p, s, ke, stream);
    case 12: return launch_regtile2_ni<KIND, 12, CT>(p, s, ke, stream);
    case 19: return launch_regtile2_ni<KIND, 19, CT>(p, s, ke, stream);
    case 24: return launch_regtile2_ni<KIND, 24, CT>(p, s, ke, stream);
    default: return LTR_ERR_CONFIG;
    }
}

int launch_regtile(int kind, const LinearParams &p, const RegtileShape &s, hipStream_t stream)
{
    // feature counts with compile-time loop bounds: MSLR-WEB10K/30K (136); anything else runs the same kernel with
    // run-time bounds
    return with_kind(kind, [&](auto K) {
        return p.F == 136 ? launch_regtile2_ct<K, 34>(p, s, stream) : launch_regtile2_ct<K, 0>(p, s, stream);
    });
}

}  // namespace
