// ltr_parts.inc -- Linear(F,1) scorer fused with the pairwise loss for lists that do not fit one
// workgroup's registers: features read ONCE, one exchange per query, persistent workgroups
// (included by ltr_linear.hip after ltr_areas.inc and ltr_cluster.inc; the step it replaces is examples/01-basic-usage.py:66-75 of the
// reference, loss_fn(Linear(F,1)(xs), ys, n).mean().backward() with the losses of
// loss/pairwise_additive.py:51-163 and loss/pairwise_lambda.py:114-140).
//
// A query is cut into P = ceil(n[b] / rpw) PARTS of equal size; a part is the unit of work.  The
// workgroup that holds a part
//   1. loads the part's rows into registers in one burst (NI x CV float4 per thread; thread = (row of
//      the sweep, lane c of the row's RS lanes) owning the row's 16-byte column vectors c, c + RS, ...
//      so its W vectors and its dW accumulators never change) and takes their scores (16-lane DPP row
//      sums + a short LDS fold).  256-thread workgroups = one wave per SIMD: k of them per CU is
//      exactly k waves per SIMD (384-thread workgroups packed one per CU fewer than the occupancy
//      API said: 6 waves do not spread evenly over 4 SIMDs);
//   2. publishes them as 8-byte {tag, score} granules (one write-through store each) and collects the
//      scores of the query's other parts by polling THEIR granules until every tag is this launch's
//      -- the data is the flag: the only exchange of the step;
//   3. runs the pair pass for ITS rows against the whole query (a home window of 64 of my documents
//      in the lanes, every 64-wide tile of the query rotating past it: the visitor rotation of
//      pairwise_core_sym without the visitor's gradient) -- d pair-sum / d s of my rows and my share
//      of the pair sum need nothing from the other parts;
//   4. folds its rows into a dW share straight from the registers and, if the query has other
//      parts, parks the share; the LAST part to arrive (one atomic per part) adds the shares in part
//      order, applies the loss modifier / gradient scale of the whole query and writes the query's
//      row of the (B, PF) partials and loss[b].
// Against the cluster kernel (ltr_cluster.inc: three exchanges, one workgroup per part in block-id
// order, counters zeroed by a launch of their own) this has one exchange, no second launch, and
// its forward progress does not rest on the dispatch order:
//   * PERSISTENT workgroups, at most as many as are resident, take parts from a ticket counter.
//     Tickets run through the queries in a fixed order with a query's parts on consecutive tickets;
//     a workgroup draws its next ticket only once the part it holds no longer waits for anybody.
//     So every ticket below the counter is held by a running workgroup that publishes its scores
//     before it waits, and at most one query straddles the counter: with more running workgroups than
//     parts per query somebody can always draw the missing tickets.  (The first ticket of workgroup
//     g is g itself; block 0, which the dispatcher starts first, also brings up the control block.)
//   * queries are taken longest first (a counting sort on the part count, built by every workgroup
//     in LDS from n[]), so the launch ends on the shortest parts.
//   * control words and granule buffers live in an EXCHANGE AREA the library owns (ltr_areas.inc:
//     exchange_area_get -- one per (device, stream), a private one per captured call; zeroed when it is
//     allocated, never handed to anybody else: nothing in it is ever uninitialised memory).  The control
//     words are SELF-RESETTING: the last part of a query zeroes its arrival counter, the last workgroup
//     to leave zeroes the ticket counter and bumps the 32-bit tag of the granules -- nothing to zero
//     between launches, graph replay included (the tag is device state, not a frozen kernel argument).
//     Tags run 1, 2, ... 2^32 - 1; the workgroup that leaves last under the last tag zeroes the granule
//     buffers before it starts over at 1, so a granule in memory never carries the tag of a later launch.
//     A launch that gave up leaves the counters dirty: the host zeroes the area before its next use
//     (ltr_device_status(clear) marks the areas).
// Deterministic: fixed summation orders, no float atomics; results do not depend on which
// workgroup takes which part.  A wait that gives up poisons the query (NaN) and raises the sticky
// device status (LTR_ERR_TIMEOUT), as in the cluster kernel.
#pragma once

namespace {

constexpr int kPtThreads = 256;                 // 4 waves, one per SIMD: 3 workgroups per CU at <= 168 VGPRs, 4 at <= 128
constexpr int kPtWaves = kPtThreads / 64;
constexpr int kPtMaxCV = 3;                     // column vectors per thread and row: rows up to 3 * 64 float4
// Row sweeps in registers (NI x CV float4 of features per thread) -- the most that compiles without a
// single spill (a spilled feature vector puts an s_waitcnt vmcnt(0) into the load burst):
// (float4 per thread for CV = 1 / 2 / 3)
//   2 workgroups per CU, <= 256 VGPRs: 36 / 40 / 42
//   3 per CU, <= 168 VGPRs:            21 / 22 / 21
//   4 per CU, <= 128 VGPRs:            14 / 12 / 12
constexpr int kPtNIRanked = 24;        // registers the ranked hinge formulation's call needs of the tile's
__host__ __device__ constexpr int parts_ni_base(int wpc, int cv)
{
    return wpc == 2 ? (cv == 1 ? 46 : (cv == 2 ? 23 : 16))
         : wpc == 3 ? (cv == 1 ? 27 : (cv == 2 ? 13 : 9))
                    : (cv == 1 ? 17 : (cv == 2 ? 8 : 5));
}
// (ranked: the counting formulation of the hinge kinds is a real call under the register-resident tile -- the
// callee's registers come out of the tile's, or the caller spills them around the call)
// (kind: the NDCG kinds' rankings and pair step need a few registers more -- sweeps fewer in the tile)
constexpr int kPtNINdcg1 = 1;
constexpr int kPtNINdcg2 = 1;
__host__ __device__ constexpr int parts_ni(int wpc, int cv, bool ranked = false, int kind = -1)
{
    return parts_ni_base(wpc, cv) - (ranked ? (kPtNIRanked / 4 + cv - 1) / cv : 0)
           - (kind == LTR_NDCG1 ? kPtNINdcg1 : (kind == LTR_NDCG2 ? kPtNINdcg2 : 0))
           - (((kind == LTR_NDCG1 || kind == LTR_NDCG2) && cv == 1 && wpc == 3) ? 1 : 0);
}

constexpr int kPtMaxParts = 32;                 // parts per query (classes of the counting sort)
constexpr int kPtMaxB = 8192;
constexpr int kPtSpinLimit = 1 << 18;
// control block (in the library's exchange area: zero when allocated), ints:
// [0] tag of the NEXT launch (0 = 1) | [4] tickets drawn | [5] workgroups gone | [8 + b] arrivals of query b
constexpr int kPtCtrlHeader = 8;
constexpr size_t kPtCtrlBytes = kExCtrlBytes;   // the control region of the exchange area (ltr_areas.inc), fixed: the shares start behind it
constexpr int kPtSleep = 4;
constexpr int kPtCombineInflight = 8;      // shares per thread in flight when a query's shares are added up

// How a part gets d pair-sum / d s of its rows:
//   ONESIDED  its rows against the whole query, every unordered pair met from both ends (by the part of
//             either document): twice the symmetric pass's work, nothing to exchange but the scores;
//   RANKED    the hinge kinds on long lists by counting (parts_hinge_ranked), else as ONESIDED.
enum { PT_ONESIDED = 0, PT_RANKED = 1 };
// LDS LANDING BUFFER (round 5, session 5; verdict r4 item 6).  A part's registers are taken from the request of its tile to its
// dW fold, and nothing of the NEXT tile can be asked for in between: by Little's law the two tiles of a CU turn over at what
// their life time allows (4.0 TB/s at C5).  The LDS the kernel leaves free (~50 KB per workgroup at two per CU) takes the first
// sweeps of the next part's tile by LDS-DMA (buffer_load_dwordx4 ... lds: no registers) while this part is still in its
// gradient / dW phase; they move into the registers (ds_read_b128) at the top of the next part, in front of its
// dot products (ONE place where those registers are written: two -- landed or not -- made the allocator spill 40-140 VGPRs),
// the rest of the tile follows from memory as before.  The next ticket must be known for that: the kinds that poll in front of their pair pass
// (logistic, LambdaARP1 / 2) draw it there already.  The hinge kinds poll INSIDE the pass and draw behind it; drawing in front
// (safe once every ticket of the part's own query is out) was built and measured: the siblings of the early-drawn part start
// up to a pair pass apart and wait for each other -- C5 102 -> 175 us (EXPERIMENTS.md) -- so they stay as they are.
constexpr int kPtPf2 = 12;                 // float4 per thread landing in LDS at two workgroups per CU (0: off)
__host__ __device__ constexpr int parts_pf_sweeps(int wpc, int cv)
{
    return wpc == 2 ? kPtPf2 / cv : 0;
}

struct PartsParams {
    LinearParams lp;              // lp.part = the (B, PF) partials of the plain path
    unsigned long long *sbuf;     // (B, L) score granules: tag << 32 | score bits
    unsigned long long *slices;   // the NDCG kinds: (B, L) score-rank granules: tag << 32 | rank
    float *pvec;                  // (B * Pmax, pitch) shares: dW (F) | db | raw pair sum | padding
    int *ctrl;
    unsigned long long gran_words; // granules of the whole exchange area behind sbuf (sbuf and slices are one allocation): zeroed when the tag wraps
    int Pmax, rpw, pitch;
    int rtarget;                  // rows per part aimed at (<= rpw): a query has ceil(n / rtarget) parts
    int RS, R;                    // threads per row (F/4 rounded up to 16), rows per sweep
    int rank_lds;                 // != 0: the LDS carries the tables of the ranked hinge formulation
    int Lg;                       // (unused: the list rounded to 64)
    unsigned park_off;            // byte offset in the dynamic LDS where W's slots end (the landing buffer, or the end of the LDS)
    int sort_min;                 // (unused: -1)
    int direct;                   // != 0: one round -- workgroup t holds part t % Pmax of query t / Pmax (or nothing), no part table
    int *status;                  // process status word (pinned host page) or null
    int spin_limit;               // polls before a wait gives up; < 0: give up at once (tests)
    unsigned pf_off;              // byte offset of the landing buffer in the dynamic LDS (0: none -- no prefetch)
};

// One LDS-DMA instruction (buffer_load_dwordx4 ... lds): lane l's 16 bytes at buffer offset voff + soff land at lds + 16 l
// (lds: wave-uniform, the generic address of dynamic LDS).  Bytes past the descriptor's range arrive as zeros.
__device__ __forceinline__ void pt_load_lds16(__amdgpu_buffer_rsrc_t rsrc, unsigned char *lds, int voff, int soff)
{
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void *)(__attribute__((address_space(3))) unsigned char *)lds,
                                             16, voff, soff, 0, 0);
}
__device__ __forceinline__ bool direct_launch(const PartsParams &pp)
{
    return pp.direct != 0;
}
__device__ __forceinline__ unsigned long long pt_ld64(const void *ptr)
{
    return __hip_atomic_load(reinterpret_cast<const unsigned long long *>(ptr), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void pt_st64(void *ptr, unsigned long long v)
{
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(ptr), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void pt_st32(int *ptr, int v)
{
    __hip_atomic_store(ptr, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Pair pass of one part: home windows of 64 of MY documents (rows r0 .. r0 + rows) against every
// 64-wide tile of the query.  gwave[0 .. 64 * nh): this wave's slice of d pair-sum / d s of my rows.
// A part of at most 32 (16) rows sits 2 (4) times in its one window, the copies hw lanes apart: a
// visitor tile then passes every document in hw steps instead of 64, the copies' sums are added.
// Returns this wave's share of the pair sum: every unordered pair of an oriented kind is met from both
// ends (by the part of either document) with the same value, so the caller halves the total; the
// row-weight kind (LambdaARP1: all ordered pairs, loss/pairwise_lambda.py:114-117) counts (home,
// visitor) only, the i = j terms included (the visitor tiles contain the home documents).
// POLL: the scores of the other parts are not in LDS yet.  A wave fetches the granules of a visitor tile
// right before it works on it (its own rows are there already) and takes the segments of its unit range whose
// tiles have arrived first, so the wait for the slowest part of the query hides behind the work on the others.
// INTLAB: integer labels, the hinge kinds' sign of a label difference from one v_med3 (see pairwise_core_sym).
// LambdaNDCG1 / LambdaNDCG2 (round 4): the kernel has the score ranks of the whole query in LDS before the pass
// (every part ranks ITS rows, the ranks are exchanged: see the kernel); the gains come unnormalised, 1 / maxDCG is
// applied where the query's shares meet.  NDCG1 is the row-weight pass on a_k = g_k / D(rank_k) in the label slot;
// NDCG2 reads (score, label, gain, rank) from q4 and the discount differences from the delta table -- the
// signed-weight step of pairwise_core_sym without the visitor's gradient (an inert document carries the rank
// 2 nb - 1: its distance to any real rank, and to another inert one, lands on a zero of the table).
template <int KIND, bool POLL = false, bool INTLAB = false>
__device__ __forceinline__ float parts_pair_pass(float2 *sy, int nb, int r0, int rows, float sigma,
                                                 float *gwave, int wl, int lane,
                                                 const unsigned long long *gran = nullptr, unsigned tag = 0u,
                                                 int spin_limit = 0, bool *ok = nullptr,
                                                 const float4 *q4 = nullptr, const float *delta = nullptr)
{
    constexpr bool kRowWeight = (KIND == LTR_ARP1 || KIND == LTR_NDCG1);
    static_assert(!(POLL && (KIND == LTR_NDCG1 || KIND == LTR_NDCG2)), "the rankings need every score first");
    constexpr bool kIntHinge = INTLAB && (KIND == LTR_HINGE || KIND == LTR_DCG_HINGE);
    const float kNaN = __builtin_nanf("");
    const float c1 = sigma * kLog2e;
    const int nt = (nb + 63) >> 6;
    const int nh = (rows + 63) >> 6;
    // width of the (only) home window when the part is small: 16 / 32 lanes, else the full 64
    const int hwid = (rows <= 16) ? 16 : ((rows <= 32) ? 32 : 64);
    const int hsh = (rows <= 16) ? 4 : ((rows <= 32) ? 5 : 6);
    for (int i = lane; i < 64 * nh; i += 64) gwave[i] = 0.f;
    const int S = (nh * nt) << hsh;                            // steps in all: hwid per (window, tile) job
    // (everything that steers the loops through readfirstlane: the compiler cannot prove the divisions
    // wave-uniform and would run the step loop on a vector counter with exec masks -- 18 instead of 14
    // instructions per step)
    const int u0 = __builtin_amdgcn_readfirstlane((wl * S) / kPtWaves);
    const int u1 = __builtin_amdgcn_readfirstlane(((wl + 1) * S) / kPtWaves);
    float lacc = 0.f;
    // one segment of this wave's unit range: `steps` steps of job (hw, v) from rotation j0 on
    auto run = [&](int hw, int v, int j0, int steps) {
            const int hloc = 64 * hw + (lane & (hwid - 1));         // (copies: lanes hwid apart hold the same document)
            const bool hvalid = hloc < rows;
            const int vidx = 64 * v + ((lane + j0) & 63);
            const bool vvalid = vidx < nb;
            if constexpr (KIND == LTR_NDCG2) {
                const int zrank = 4 * (2 * nb - 1);
                const unsigned dbase = (unsigned)(size_t)(__attribute__((address_space(3))) const float *)delta;
                const float4 h4 = q4[hvalid ? r0 + hloc : 0];
                const float4 v4 = q4[vvalid ? vidx : 0];
                const float sh = h4.x, Gh = h4.z;
                const int rh = hvalid ? ((int)h4.w << 2) : zrank;
                float sv = v4.x, Gv = v4.z;
                int rv = vvalid ? ((int)v4.w << 2) : zrank;
                float gh = 0.f, g1 = 0.f, l1a = 0.f;
                // one evaluation: the signed weight Ws = delta * (G_home - G_vis) carries the orientation
                auto eval = [&](float sv_, float Gv_, float d_, float &g, float &l) {
                    const float t = (sh - sv_) * c1;
                    const float Ws = d_ * (Gh - Gv_);
                    const float e = __builtin_amdgcn_exp2f(-fabsf(t));
                    const float u = 1.0f + e;
                    const float rr = __builtin_amdgcn_rcpf(u);
                    const float l1 = log2_1p_comp(e, u, rr);
                    const bool ahead = t * Ws >= 0.0f;
                    const float psi = ahead ? e * rr : rr;
                    const float lg = l1 + (ahead ? 0.0f : fabsf(t));
                    l = __builtin_fmaf(fabsf(Ws), lg, l);
                    g = __builtin_fmaf(-Ws, psi, g);
                };
                // Two steps at a time on independent accumulators (the pass is bound by the latency of a step's
                // dependent chain, not by issue); the discounts of the NEXT two steps are requested before these
                // two are evaluated: the LDS round trip is off the dependency chain.
                int rv1 = wave_rol1i(rv);
                float d0 = lds_at_absdiff(dbase, rh, rv), d1 = lds_at_absdiff(dbase, rh, rv1);
                int s = 0;
                for (; s + 2 <= steps; s += 2) {
                    const float sv1 = wave_rol1(sv), Gv1 = wave_rol1(Gv);
                    const int rv2 = wave_rol1i(rv1), rv3 = wave_rol1i(rv2);
                    const float dn0 = lds_at_absdiff(dbase, rh, rv2), dn1 = lds_at_absdiff(dbase, rh, rv3);
                    eval(sv, Gv, d0, gh, lacc);
                    eval(sv1, Gv1, d1, g1, l1a);
                    sv = wave_rol1(sv1); Gv = wave_rol1(Gv1);
                    rv = rv2; rv1 = rv3; d0 = dn0; d1 = dn1;
                }
                if (s < steps) eval(sv, Gv, d0, gh, lacc);
                gh += g1;
                lacc += l1a;
                if (hwid <= 32) gh += __shfl_xor(gh, 32);
                if (hwid <= 16) gh += __shfl_xor(gh, 16);
                if (hvalid && lane < hwid) gwave[hloc] += gh;
                return;
            }
            const float2 hv = sy[hvalid ? r0 + hloc : 0];
            const float2 vv = sy[vvalid ? vidx : 0];
            float sh, yh, sv, yv;
            if (kRowWeight) { sh = hvalid ? hv.x : kNaN; yh = hv.y; sv = vvalid ? vv.x : kNaN; yv = vv.y; }
            else if (kIntHinge) {
                sh = hvalid ? hv.x : -__builtin_inff(); yh = hvalid ? hv.y : -3.0e38f;
                sv = vvalid ? vv.x : -__builtin_inff(); yv = vvalid ? vv.y : -3.0e38f;
            }
            else { sh = hv.x; yh = hvalid ? hv.y : kNaN; sv = vv.x; yv = vvalid ? vv.y : kNaN; }
            // One evaluation of (home, visitor): adds d term / d s_home to g and the pair value to l.
            auto visit = [&](float sv_, float yv_, float &g, float &l) {
                if (KIND == LTR_HINGE || KIND == LTR_DCG_HINGE) {
                    // the margin term of pairwise_core_sym: sgn = -1 / +1 when the home / the visitor carries
                    // the higher label, 0 for equal labels or a NaN sentinel; active iff u >= 0 (non-strict,
                    // loss/pairwise_additive.py:107-113)
                    float sgn;
                    if (kIntHinge) {
                        sgn = __builtin_amdgcn_fmed3f(yv_ - yh, -1.0f, 1.0f);
                    } else {
                        sgn = (yh < yv_) ? 1.0f : 0.0f;
                        sgn = (yh > yv_) ? -1.0f : sgn;
                    }
                    const float uu = __builtin_fmaf(sgn, sh - sv_, __builtin_fabsf(sgn));
                    l += __builtin_fmaxf(uu, 0.0f);
                    g += (uu >= 0.0f) ? sgn : 0.0f;
                } else if (!kRowWeight) {
                    const bool gt = yh > yv_, lt = yh < yv_;
                    float Wp = 1.0f;
                    if (KIND == LTR_ARP2) Wp = fabsf(yh - yv_);
                    const float t = (sh - sv_) * c1;
                    const float z = gt ? t : -t;
                    const float e = __builtin_amdgcn_exp2f(-fabsf(z));
                    const float r = __builtin_amdgcn_rcpf(1.0f + e);
                    const float psi = (z >= 0.0f) ? e * r : r;
                    const float lg = log2_1p(e) + fmaxf(-z, 0.0f);
                    const float Wm = (gt | lt) ? Wp : 0.0f;
                    l += Wm * lg;
                    g += (gt ? -Wm : Wm) * psi;
                } else {
                    const float x = (sh - sv_) * c1;
                    const bool ok = (x == x);                       // NaN score = inert document
                    const float e = __builtin_amdgcn_exp2f(-fabsf(x));
                    const float r = __builtin_amdgcn_rcpf(1.0f + e);
                    const float sneg = (x >= 0.0f) ? e * r : r;
                    const float l1 = log2_1p(e);
                    l += ok ? yh * (l1 + fmaxf(-x, 0.0f)) : 0.0f;
                    g += ok ? (yv_ - (yh + yv_) * sneg) : 0.0f;
                }
            };
            // Four steps at a time on independent accumulators: with two or three waves per SIMD the pass is
            // bound by the latency of one step's dependent chain (~100 cycles per step measured when stepping
            // one by one), not by issue; the four evaluations interleave.
            float gh = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f, l1a = 0.f, l2a = 0.f, l3a = 0.f;
            int s = 0;
            for (; s + 4 <= steps; s += 4) {
                const float sv1 = wave_rol1(sv), yv1 = wave_rol1(yv);
                const float sv2 = wave_rol1(sv1), yv2 = wave_rol1(yv1);
                const float sv3 = wave_rol1(sv2), yv3 = wave_rol1(yv2);
                visit(sv, yv, gh, lacc);
                visit(sv1, yv1, g1, l1a);
                visit(sv2, yv2, g2, l2a);
                visit(sv3, yv3, g3, l3a);
                sv = wave_rol1(sv3);
                yv = wave_rol1(yv3);
            }
            for (; s < steps; ++s) {
                visit(sv, yv, gh, lacc);
                sv = wave_rol1(sv);
                yv = wave_rol1(yv);
            }
            gh += (g1 + g2) + g3;
            lacc += (l1a + l2a) + l3a;
            // the copies of a document: row_bcast-free fold through the lanes hwid apart
            if (hwid <= 32) gh += __shfl_xor(gh, 32);
            if (hwid <= 16) gh += __shfl_xor(gh, 16);
            if (hvalid && lane < hwid) gwave[hloc] += gh;
    };
    if (!POLL) {
        int u = u0;
        while (u < u1) {
            const int job = u >> hsh, j0 = u & (hwid - 1);
            const int hw = __builtin_amdgcn_readfirstlane(job / nt);
            const int steps = __builtin_amdgcn_readfirstlane(min(hwid - j0, u1 - u));
            run(hw, job - hw * nt, j0, steps);
            u += steps;
        }
        return lacc;
    }
    // ---- POLL: the segments of [u0, u1) (the pieces inside one job) in order; the granules of a segment's
    // visitor tile are requested while the segment before it is being worked on ----
    if (u1 <= u0) return lacc;
    const int job_first = u0 >> hsh;
    const int nseg = ((u1 - 1) >> hsh) - job_first + 1;
    auto tile_of = [&](int i) { const int job = job_first + i; return job - (job / nt) * nt; };
    auto fetch = [&](int v) -> unsigned long long {          // this lane's granule of tile v (0 where none is needed)
        const int k = 64 * v + lane;
        const bool need = (k < nb) && (k < r0 || k >= r0 + rows);
        return need ? pt_ld64(gran + k) : 0ull;
    };
    int spins = 0;
    bool fine = true;
    unsigned long long gnext = fetch(tile_of(0));
    for (int i = 0; i < nseg; ++i) {
        const int job = job_first + i;
        const int us = (i == 0) ? u0 : (job << hsh);
        const int j0 = us & (hwid - 1);
        const int hw = __builtin_amdgcn_readfirstlane(job / nt);
        const int v = job - hw * nt;
        const int steps = __builtin_amdgcn_readfirstlane(min(hwid - j0, u1 - us));
        unsigned long long gv = gnext;
        if (i + 1 < nseg) gnext = fetch(tile_of(i + 1));          // in flight under this segment's steps
        const int k = 64 * v + lane;
        const bool need = (k < nb) && (k < r0 || k >= r0 + rows);
        while (__ballot(need && (unsigned)(gv >> 32) != tag) != 0ull) {
            if (++spins > spin_limit) { fine = false; break; }
            __builtin_amdgcn_s_sleep(kPtSleep);
            gv = fetch(v);
        }
        if (need) sy[k].x = __uint_as_float((unsigned)gv);
        run(hw, v, j0, steps);
    }
    if (!fine && ok) *ok = false;
    return lacc;
}

// ---------------------------------------------------------------------------------------------
// The two hinge kinds on long lists WITHOUT the O(n^2) pair pass (VERDICT r2 item 3).  For a document k
//   d pair-sum / d s_k = #{m : y_m > y_k, fl(s_m - s_k) <= 1}  -  #{m : y_m < y_k, fl(s_k - s_m) <= 1}
// and its share of the pair sum is the sum of 1 - (s_k - s_m) over the second set (loss/
// pairwise_additive.py:107-113: a pair counts iff 1 - (s_i - s_j) >= 0, i the higher label) -- COUNT and SUM
// queries over the documents of other grades inside a score window.  With the query's documents dealt
// into NB buckets by score (a counting sort: histogram, prefix, scatter) and, per bucket boundary, the
// number of documents of grade >= g below it (g = 1..4, four 16-bit fields of one 64-bit word) and the sum
// of the scores of grade < g above it (a float4), a document needs two table look-ups and an exact,
// element-wise visit of the three buckets around each window edge -- the fp32 predicate is the pair
// pass's own (the same fmaf), and it is monotone in s_m, so everything below the edge buckets passes it
// and everything above fails it: the counts, hence the gradients, are the pair pass's bit for bit.
// O(n + rows * bucket size) instead of O(rows * n).
// Labels must be the integers 0..4 and the scores finite with a spread of more than a few thousand ulps
// (else the buckets would be narrower than the rounding of the predicate); otherwise -- decided per
// query, uniformly -- the caller runs the pair pass.  Deterministic: fixed scan orders, buckets sorted
// by document index before anything is summed.
// ---------------------------------------------------------------------------------------------
constexpr int kPtRankMinN = 192;
constexpr long long kPtRankMinWork = 80000;
constexpr int kPtRankMaxN = 2048;
__host__ __device__ inline int parts_rank_buckets(int n)
{
    int nbk = 64;
    while ((n > 1024 ? 4 : 2) * nbk < n) nbk <<= 1;            // ~2 documents per bucket, ~4 on the longest lists (LDS)
    return nbk;
}
// LDS of the ranked formulation (sizes below; the layout is in parts_hinge_ranked)
__host__ __device__ inline size_t parts_rank_lds_bytes(int kind, int L)
{
    if (!(kind == LTR_HINGE || kind == LTR_DCG_HINGE) || L < kPtRankMinN) return 0;
    const size_t n = (size_t)(L < kPtRankMaxN ? L : kPtRankMaxN);
    const size_t NB = (size_t)parts_rank_buckets((int)n);
    // aggS u64[4][NB + 1] | aggC u64[NB + 1] | elems int2[n] | start int[NB + 2] | cur int[NB]
    return 40 * (NB + 1) + 8 * ((n + 1) & ~(size_t)1) + 4 * ((NB + 2 + 3) & ~(size_t)3) + 4 * (NB + 4);
}

template <int CTRL, int ROW_MASK, int BANK_MASK>
__device__ __forceinline__ unsigned pt_dpp0(unsigned v)
{
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, BANK_MASK, false);
}
__device__ __forceinline__ unsigned long long pt_scan_u64(unsigned long long v)
{
#define PT_STEP(SRC, CTRL, RM, BM)                                                                              \
    do {                                                                                                        \
        const unsigned lo_ = pt_dpp0<CTRL, RM, BM>((unsigned)(SRC)), hi_ = pt_dpp0<CTRL, RM, BM>((unsigned)((SRC) >> 32)); \
        acc += ((unsigned long long)hi_ << 32) | lo_;                                                           \
    } while (0)
    unsigned long long acc = v;
    PT_STEP(v, 0x111, 0xF, 0xF);          // row_shr:1
    PT_STEP(v, 0x112, 0xF, 0xF);          // row_shr:2
    PT_STEP(v, 0x113, 0xF, 0xF);          // row_shr:3
    { const unsigned long long a4 = acc; PT_STEP(a4, 0x114, 0xF, 0xE); }      // row_shr:4, banks 1-3
    { const unsigned long long a8 = acc; PT_STEP(a8, 0x118, 0xF, 0xC); }      // row_shr:8, banks 2-3
    { const unsigned long long ab = acc; PT_STEP(ab, 0x142, 0xA, 0xF); }      // row_bcast15 -> rows 1, 3
    { const unsigned long long ac = acc; PT_STEP(ac, 0x143, 0xC, 0xF); }      // row_bcast31 -> rows 2, 3
#undef PT_STEP
    return acc;
}
// min / max over the wave, every lane gets it (lanes without a source keep their own value)
template <bool MAX>
__device__ __forceinline__ float pt_wave_minmax(float v)
{
#define PT_MM(CTRL, RM)                                                                                          \
    do {                                                                                                        \
        const float o_ = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, RM, 0xF, false)); \
        v = MAX ? fmaxf(v, o_) : fminf(v, o_);                                                                  \
    } while (0)
    PT_MM(0xB1, 0xF); PT_MM(0x4E, 0xF); PT_MM(0x141, 0xF); PT_MM(0x140, 0xF); PT_MM(0x142, 0xA); PT_MM(0x143, 0xC);
#undef PT_MM
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}


// All 256 threads; contains barriers.  gloc[0 .. rpw) <- d pair-sum / d s of my rows (0 past `rows`);
// raw_out <- twice my share of the pair sum (the caller halves the sum of an oriented kind).
// scr: 64 words of LDS scratch.  Returns false (nothing written) when the query does not qualify.
// Everything that is summed in an order the hardware chooses (LDS atomics, the documents of a bucket in
// scatter order) is summed in FIXED POINT, so the result does not depend on that order: scores as
// 30-bit fractions of the query's score range (64-bit sums), the margins met in the edge buckets as 32-bit
// fractions of 3 bucket widths + 2, summed in 64 bits.  A visited document lies less than two bucket widths (and
// the rounding of the bucket index: under half a width, by `need`) above the window edge, or above the query's
// minimum where the edge is clamped to it: its margin is below 1 + 2.5 widths, so a term fits 32 bits and 2048 of
// them 43.  The quantum follows the margins that are summed, not the range: one far outlier puts every other
// document into bucket 0, and as 24-bit fractions of range + 2 each margin lost ~range / 2^24 (2e-3 of the loss at
// 1e5); and a 32-bit sum of those wrapped once some 600 lower-graded documents with margins near 1 shared the edge
// buckets -- a cluster of tied scores at the query's minimum, the loss 18-37 % low.
#ifdef LTR_TRACE
#define RK_STAMP(i) do { if (trace && threadIdx.x == 0) trace[i] = (long long)wall_clock64(); } while (0)
#else
#define RK_STAMP(i) do { } while (0)
#endif
// (not inlined: its ~120 registers would otherwise be live next to the feature tile of every instantiation;
// the LDS regions come as byte OFFSETS into the dynamic segment -- generic pointers through a real call make
// every LDS access a flat_* instruction, 3x slower here)
__device__ __attribute__((noinline)) bool parts_hinge_ranked(
int nb, int r0, int rows, int rpw, unsigned rk_off,
                                   unsigned gloc_off, unsigned scr_off, float &raw_out, long long *trace = nullptr)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const float2 *sy = reinterpret_cast<const float2 *>(smem);
    unsigned char *rk = smem + rk_off;
    float *gloc = reinterpret_cast<float *>(smem + gloc_off);
    float *scr = reinterpret_cast<float *>(smem + scr_off);
    constexpr int T = kPtThreads;
    const int tid = threadIdx.x, lane = tid & 63, wl = tid >> 6;
    const int NB = parts_rank_buckets(nb);
    // LDS: aggS u64[4][NB + 1] (threshold-major) | aggC u64[NB + 1] | elems int2[n] | start int[NB + 2] | cur int[NB]
    unsigned long long *aggS = reinterpret_cast<unsigned long long *>(rk);
    unsigned long long *aggC = aggS + 4 * (size_t)(NB + 1);
    int2 *elems = reinterpret_cast<int2 *>(aggC + NB + 1);
    int *start = reinterpret_cast<int *>(elems + ((nb + 1) & ~1));
    int *cur = start + ((NB + 2 + 3) & ~3);
    int *iscr = reinterpret_cast<int *>(scr);
    unsigned long long *lscr = reinterpret_cast<unsigned long long *>(scr);

    // ---- S1: the query qualifies?  min / max of the scores ----
    float lo = __builtin_inff(), hi = -__builtin_inff();
    int bad = 0;
    for (int k = tid; k < nb; k += T) {
        const float2 v = sy[k];
        lo = fminf(lo, v.x); hi = fmaxf(hi, v.x);
        bad |= (int)!(fabsf(v.x) < __builtin_inff()) | (int)!(v.y == floorf(v.y) && v.y >= 0.0f && v.y <= 4.0f);
    }
    lo = pt_wave_minmax<false>(lo);
    hi = pt_wave_minmax<true>(hi);
    bad = (__ballot(bad != 0) != 0ull) ? 1 : 0;
    if (lane == 0) { scr[wl] = lo; scr[4 + wl] = hi; iscr[8 + wl] = bad; }
    // (the tables are cleared while the verdict is on its way)
    for (int i = tid; i < 5 * (NB + 1); i += T) aggS[i] = 0ull;
    for (int i = tid; i < NB + 2 + NB + 4; i += T) start[i] = 0;          // start[] and cur[] are neighbours
    __syncthreads();
    lo = fminf(fminf(scr[0], scr[1]), fminf(scr[2], scr[3]));
    hi = fmaxf(fmaxf(scr[4], scr[5]), fmaxf(scr[6], scr[7]));
    bad = iscr[8] | iscr[9] | iscr[10] | iscr[11];
    // a bucket must be wider than the rounding of the window edges (8 ulps of the largest |s| + 1)
    const float span = hi - lo;
    const float need = (float)NB * 9.6e-7f * (fmaxf(fabsf(lo), fabsf(hi)) + 1.0f);
    if (bad || !(span > need)) { __syncthreads(); return false; }
    const float scale = (float)NB / span;
    auto bucket = [&](float x) {
        const float f = (x - lo) * scale;
        int bb = (int)f;                                      // (f >= 0 for x >= lo; below lo: clamped)
        bb = (f < 0.0f) ? 0 : bb;
        return bb > NB - 1 ? NB - 1 : bb;
    };
    const float qs = 1073741824.0f / span;                    // scores -> 30-bit fractions of the range
    const float qs_inv = span * (1.0f / 1073741824.0f);
    const float mmax = 3.0f * span / (float)NB + 2.0f;        // above every margin the visits of S5 meet
    const float qu = 4294967296.0f / mmax;                    // those margins -> 32-bit fractions of it
    const float qu_inv = mmax * (1.0f / 4294967296.0f);
    RK_STAMP(10);

    // ---- S2: histogram + per-bucket counts / sums in one pass over the documents ----
    for (int k = tid; k < nb; k += T) {
        const float2 v = sy[k];
        const int bb = bucket(v.x);
        const int g = (int)v.y;
        atomicAdd(&start[bb], 1);
        const unsigned long long cge = (g >= 1 ? 1ull : 0ull) | (g >= 2 ? 1ull << 16 : 0ull) | (g >= 3 ? 1ull << 32 : 0ull) |
                                       (g >= 4 ? 1ull << 48 : 0ull);
        if (cge) atomicAdd(&aggC[bb], cge);
        const unsigned long long q = (unsigned long long)(unsigned)((v.x - lo) * qs);
        for (int th = g + 1; th <= 4; ++th) atomicAdd(&aggS[(size_t)(th - 1) * (NB + 1) + bb], q);     // grade < th
    }
    __syncthreads();
    RK_STAMP(11);
    // ---- S3: scans over the buckets: exclusive prefix of the histogram and of the counts, inclusive SUFFIX of
    // the sums (small where few documents remain).  Thread t owns ipt consecutive buckets; for the suffix
    // the chunks are taken in reverse. ----
    const int ipt = NB >= T ? NB / T : 1;                      // buckets per thread (<= 4)
    const bool act = tid * ipt < NB;
    const int nch = NB >= T ? T : NB;
    const int rch = nch - 1 - tid;                             // my chunk in the reversed order
    {
        unsigned long long h[4], c[4], sfx[4][4];
        unsigned long long hr = 0ull, cr = 0ull, sr[4] = {0ull, 0ull, 0ull, 0ull};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool on = act && i < ipt;
            h[i] = on ? (unsigned long long)(unsigned)start[tid * ipt + i] : 0ull;
            c[i] = on ? aggC[tid * ipt + i] : 0ull;
            hr += h[i]; cr += c[i];
#pragma unroll
            for (int th = 0; th < 4; ++th) {
                sfx[th][i] = on ? aggS[(size_t)th * (NB + 1) + rch * ipt + (ipt - 1 - i)] : 0ull;
                sr[th] += sfx[th][i];
            }
        }
        // histogram and counts share one scan: the histogram rides in bits 48.. of a second word? no -- two scans
        const unsigned long long hi_ = pt_scan_u64(hr), ci_ = pt_scan_u64(cr);
        unsigned long long si_[4];
#pragma unroll
        for (int th = 0; th < 4; ++th) si_[th] = pt_scan_u64(sr[th]);
        if (lane == 63) {
            lscr[8 + wl] = hi_; lscr[12 + wl] = ci_;
#pragma unroll
            for (int th = 0; th < 4; ++th) lscr[16 + 4 * th + wl] = si_[th];
        }
        __syncthreads();
        unsigned long long hb = hi_ - hr, cb = ci_ - cr, sb[4];
#pragma unroll
        for (int th = 0; th < 4; ++th) sb[th] = si_[th] - sr[th];
        for (int w = 0; w < wl; ++w) {
            hb += lscr[8 + w]; cb += lscr[12 + w];
#pragma unroll
            for (int th = 0; th < 4; ++th) sb[th] += lscr[16 + 4 * th + w];
        }
        unsigned long long ctot = 0ull;
        for (int w = 0; w < kPtWaves; ++w) ctot += lscr[12 + w];
        if (act) {
#pragma unroll
            for (int i = 0; i < 4; ++i) if (i < ipt) {
                start[tid * ipt + i] = (int)hb; hb += h[i];
                aggC[tid * ipt + i] = cb; cb += c[i];
#pragma unroll
                for (int th = 0; th < 4; ++th) { sb[th] += sfx[th][i]; aggS[(size_t)th * (NB + 1) + rch * ipt + (ipt - 1 - i)] = sb[th]; }
            }
        }
        if (tid == 0) { start[NB] = nb; aggC[NB] = ctot; }
    }
    __syncthreads();
    RK_STAMP(12);
    // ---- S4: scatter the documents into their buckets (any order inside a bucket) ----
    for (int k = tid; k < nb; k += T) {
        const float2 v = sy[k];
        const int bb = bucket(v.x);
        const int slot = start[bb] + atomicAdd(&cur[bb], 1);
        elems[slot] = make_int2(__float_as_int(v.x), (int)v.y);
    }
    __syncthreads();
    RK_STAMP(13);
    RK_STAMP(14);
    // ---- S5: my rows ----
    const unsigned long long totc = aggC[NB];
    float lsum = 0.f;
    for (int lr = tid; lr < rpw; lr += T) {
        float g = 0.f;
        if (lr < rows) {
            const float2 hv = sy[r0 + lr];
            const float s = hv.x;
            const int y = (int)hv.y;
            int A = 0, Bc = 0;
            if (y < 4) {
                // higher labels m: the pair counts iff 1 + (s - s_m) >= 0, true for s_m up to ~ s + 1
                const int sh = 16 * y;                        // field of threshold y + 1
                const int bt = bucket(s + 1.0f);
                const int b0 = bt > 0 ? bt - 1 : 0, b1 = bt + 2 < NB ? bt + 2 : NB;
                A = (int)((aggC[b0] >> sh) & 0xffffull);
                const int e1 = start[b1];
                for (int e = start[b0]; e < e1; e += 4) {
                    int2 x[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) x[u] = elems[min(e + u, e1 - 1)];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const float uu = __builtin_fmaf(1.0f, s - __int_as_float(x[u].x), 1.0f);
                        A += (e + u < e1 && x[u].y > y && uu >= 0.0f) ? 1 : 0;
                    }
                }
            }
            if (y > 0) {
                // lower labels m: the pair counts iff 1 - (s - s_m) >= 0, true for s_m from ~ s - 1 on
                const int sh = 16 * (y - 1);                  // field of threshold y
                const int bt = bucket(s - 1.0f);
                const int b0 = bt > 0 ? bt - 1 : 0, b1 = bt + 2 < NB ? bt + 2 : NB;
                const int all_above = nb - start[b1];
                const int ge_above = (int)((totc >> sh) & 0xffffull) - (int)((aggC[b1] >> sh) & 0xffffull);
                Bc = all_above - ge_above;
                // sum of 1 - (s - s_m) over them = Bc * (1 - s + lo) + (sum of s_m - lo), the latter in fixed point
                float lk = (float)Bc * ((1.0f - s) + lo) + (float)(long long)aggS[(size_t)(y - 1) * (NB + 1) + b1] * qs_inv;
                unsigned long long uq = 0ull;
                const int e1 = start[b1];
                for (int e = start[b0]; e < e1; e += 4) {
                    int2 x[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) x[u] = elems[min(e + u, e1 - 1)];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const float uu = __builtin_fmaf(-1.0f, s - __int_as_float(x[u].x), 1.0f);
                        const bool on = e + u < e1 && x[u].y < y && uu >= 0.0f;
                        Bc += on ? 1 : 0;
                        uq += on ? (unsigned)(uu * qu) : 0u;
                    }
                }
                lsum += lk + (float)uq * qu_inv;
            }
            g = (float)(A - Bc);
        }
        gloc[lr] = g;
    }
    const float ws = wave_sum(lsum);
    if (lane == 0) scr[48 + wl] = ws;
    __syncthreads();
    raw_out = 2.0f * ((scr[48] + scr[49]) + (scr[50] + scr[51]));
    return true;
}

// The query's loss and the factor on its unscaled gradient from the raw pair sum (the modifier of
// loss/pairwise_additive.py:132-133 for the DCG hinge; sigma / ln 2 for the log2-sigmoid kinds).
template <int KIND>
__device__ __forceinline__ float parts_finish(float raw, float sigma, float &gscale)
{
    // (the one-sided pass meets every unordered pair of an oriented kind from both ends)
    float total = (KIND == LTR_ARP1 || KIND == LTR_NDCG1) ? raw : 0.5f * raw;
    gscale = 1.0f;
    if (KIND == LTR_DCG_HINGE) {
        const float lg = logf(2.0f + total);
        gscale = 1.0f / ((2.0f + total) * lg * lg);
        total = -1.0f / lg;
    } else if (KIND != LTR_HINGE) {
        gscale = sigma / kLn2;
    }
    return total;
}

// The NDCG kinds: q4 (score, label, gain, rank) and the discount-difference table of LambdaNDCG2, then the score
// ranks of the query [Ls], the label ranks of my rows [Ls] and the packed (score key, label key) pairs of the
// keyed counting rank [Ls x 16 bytes] -- behind the ranked formulation's tables.
__host__ __device__ inline size_t parts_ndcg_lds_bytes(int kind, int L)
{
    if (kind != LTR_NDCG1 && kind != LTR_NDCG2) return 0;
    const size_t Ls = (size_t)((L + 63) & ~63);
    size_t bytes = 24 * Ls;
    if (kind == LTR_NDCG2) bytes += 16 * Ls + ((4 * ndcg2_delta_floats(Ls) + 15) & ~(size_t)15);
    return bytes;
}
// LDS of one workgroup (bytes); the layout is carved in the kernel in the same order.  rank_kind: the kind when
// the kernel carries the tables of the ranked hinge formulation, else -1.
__host__ __device__ inline size_t parts_lds_bytes(int B, int L, int RS, int R, int CV, int rpw, int Pmax, int rank_kind, int kind)
{
    const size_t Ls = (size_t)((L + 63) & ~63);
    const size_t rpwp = (size_t)((rpw + 63) & ~63);
    const size_t SEGP = (size_t)(RS >> 4) + 1;
    const size_t Bp = (size_t)((B + 3) & ~3);
    const size_t chunks = ((size_t)B + kPtThreads - 1) / kPtThreads;
    size_t bytes = 8 * Ls;                                           // sy
    bytes += 4 * (((size_t)rpw * SEGP + 3) & ~(size_t)3);            // pd
    bytes += 4 * (size_t)kPtWaves * rpwp + 4 * rpwp;                 // gw: the waves' gradient slices of my rows; gloc
    bytes += 16 * (size_t)R * RS * CV;                               // dred
    bytes += 4 * (32 + 16 + 2 * (kPtMaxParts + 2));                  // red, misc, tend, qstart
    bytes += 4 * 3 * Bp;                                             // nl, order, doneq
    bytes += 2 * 4 * chunks * kPtWaves * (size_t)Pmax;               // counting-sort counts, the waves' offsets
    bytes = (bytes + 15) & ~(size_t)15;
    bytes += 4 * 64 + parts_rank_lds_bytes(rank_kind, L);            // scratch + tables of the ranked hinge formulation
    bytes = (bytes + 15) & ~(size_t)15;
    bytes += parts_ndcg_lds_bytes(kind, L);                          // the NDCG kinds' rankings, gains and discount table
    bytes += 16 * (size_t)RS * CV;                                   // W, one float4 per (lane of a row, column vector)
    return bytes;
}

#ifdef LTR_TRACE
// trace build: 16 stamps of the 100 MHz wall clock per part (ticket) in the score-output buffer
#define PT_STAMP(i) do { if (tid == 0) reinterpret_cast<long long *>(p.scores_out)[(size_t)t * 16 + (i)] = (long long)wall_clock64(); } while (0)
#else
#define PT_STAMP(i) do { } while (0)
#endif
// NI row sweeps x CV column vectors per thread in registers; MINW = workgroups per CU the register
// allocation must allow (= waves per SIMD: a workgroup is one wave per SIMD).
// MODE (PT_*): PT_RANKED compiles the ranked hinge formulation in (the hinge kinds on shapes where it can
// pay: the call costs the other shapes registers -- C5 108 -> 124 us with it compiled in and never taken).
template <int KIND, int NI, int CV, int MINW, int MODE = PT_ONESIDED, bool PF = false>
__global__ void __launch_bounds__(kPtThreads, MINW)
linear_parts_kernel(PartsParams pp)
{
    constexpr bool RK = (MODE == PT_RANKED);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const LinearParams &p = pp.lp;
#ifdef LTR_TRACE
    const long long t_entry = (long long)wall_clock64();
#endif
    constexpr int T = kPtThreads, NW = kPtWaves;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wl = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int B = p.B, L = p.L, F = p.F;
    const int C = F >> 2, RS = pp.RS, R = pp.R;
    const int SEG = RS >> 4, SEGP = SEG + 1;
    const int rpw = pp.rpw, Pmax = pp.Pmax, rtarget = pp.rtarget;
    const int Ls = (L + 63) & ~63;
    const int rpwp = (rpw + 63) & ~63;
    const int Bp = (B + 3) & ~3;
    const int G = (int)gridDim.x;
    const int RSC = RS * CV;                                          // float4 slots of a row in dred

    float2 *sy = reinterpret_cast<float2 *>(smem);                    // [Ls] (score, label) of the query
    float *pd = reinterpret_cast<float *>(sy + Ls);                   // [rpw][SEGP] 16-lane partial dots
    float *gw = pd + ((rpw * SEGP + 3) & ~3);                         // [NW][rpwp] gradient slices of the waves
    float *gloc = gw + NW * rpwp;                                     // [rpwp] d pair-sum / d s of my rows
    float4 *dred = reinterpret_cast<float4 *>(gloc + rpwp);           // [R][CV * RS] dW partials of the row groups
    float *red = reinterpret_cast<float *>(dred + R * RSC);           // [32]
    int *misc = reinterpret_cast<int *>(red + 32);                    // [16]
    int *tend = misc + 16;                                            // [kPtMaxParts + 2] last ticket + 1 of a class
    int *qstart = tend + kPtMaxParts + 2;                             // [kPtMaxParts + 2] first query of a class
    int *nl = qstart + kPtMaxParts + 2;                               // [Bp] clamped n
    int *order = nl + Bp;                                             // [Bp] queries, most parts first
    int *doneq = order + Bp;                                          // [Bp] queries whose last (deferred) arrival was mine: (P << 24) | b
    int *ccnt = doneq + Bp;                                           // [chunks][NW][Pmax] class counts | [NW][chunks][Pmax] the waves' offsets
    float *rscr = reinterpret_cast<float *>(smem + ((((size_t)(reinterpret_cast<unsigned char *>(ccnt + 2 * ((B + T - 1) / T) * NW * Pmax) - smem)) + 15) & ~(size_t)15));   // [64]
    unsigned char *rk = reinterpret_cast<unsigned char *>(rscr + 64);  // tables of the ranked hinge formulation
    // the NDCG kinds' region (parts_ndcg_lds_bytes; the kernels of these kinds carry no ranked-formulation tables)
    constexpr bool kNdcg = (KIND == LTR_NDCG1 || KIND == LTR_NDCG2);
    QueryLds nq;
    if constexpr (kNdcg) {
        unsigned char *cur = smem + (((size_t)(rk - smem) + 15) & ~(size_t)15);
        nq.sy = sy; nq.q4 = nullptr; nq.delta = nullptr;
        if (KIND == LTR_NDCG2) {
            nq.q4 = reinterpret_cast<float4 *>(cur);
            cur += 16 * (size_t)Ls;
            nq.delta = reinterpret_cast<float *>(cur);
            cur += (4 * ndcg2_delta_floats((size_t)Ls) + 15) & ~(size_t)15;
        }
        nq.rank_s = reinterpret_cast<int *>(cur);
        nq.rank_y = nq.rank_s + Ls;
        nq.gpart = reinterpret_cast<float *>(cur);
        nq.gbytes = 24u * (unsigned)Ls;
        nq.red = red;
    }
    // the landing buffer: sweeps 0 .. NPF - 1 of the next part, slot (i, j) of thread tid at [(i * CV + j) * T + tid] (a wave's
    // 64 lanes = the 1 KB an LDS-DMA instruction writes)
    constexpr int NPF = PF ? parts_pf_sweeps(MINW, CV) : 0;
    static_assert(!PF || (MODE == PT_ONESIDED && (KIND == LTR_LOGISTIC || KIND == LTR_ARP1 || KIND == LTR_ARP2) && NPF > 0),
                  "landing buffer: the one-sided kernels of the kinds that draw their next ticket in front of the pair pass");
    static_assert(NPF < NI, "the landing buffer holds a part of the tile");
    const bool pf_on = NPF > 0 && !direct_launch(pp);

    // ---- control block: read now, looked at behind the table build ----
    // (plain loads: what an earlier launch left is visible at the kernel boundary, and hundreds of
    // workgroups reading the same words coherently are served one by one -- 10 us of prologue)
    // (a plain load: what an earlier launch left is visible at the kernel boundary; a fresh area holds 0: the first tag is 1)
    const unsigned tag_word = (unsigned)__builtin_amdgcn_readfirstlane(pp.ctrl[0]);
    const unsigned tag = tag_word ? tag_word : 1u;
    const bool direct = pp.direct != 0;
    // (DIRECT: the length of this workgroup's query, requested before anything else -- the tile cannot be asked
    // for without it)
    const int nb_direct = direct ? __builtin_amdgcn_readfirstlane(clamp_n(p.n[(int)blockIdx.x / pp.Pmax], p.L)) : 0;
#ifdef LTR_TRACE
    long long t_pro[4] = {0, 0, 0, 0};
#define PT_PRO(i) t_pro[i] = (long long)wall_clock64()
#else
#define PT_PRO(i) do { } while (0)
#endif
    const int r = tid / RS;                                           // (R * RS == T: every thread has a row)
    const int c = tid - r * RS;
    // W waits in LDS (the registers it would occupy for the whole kernel are worth more to the tile): slot
    // c + j * RS = column vector j of lane c, zero beyond the row
    float4 *wlds = reinterpret_cast<float4 *>(smem + pp.park_off) - RSC;
    for (int i = tid; i < RSC; i += T)
        wlds[i] = (i < C) ? reinterpret_cast<const float4 *>(p.W)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float bias = p.bias ? p.bias[0] : 0.f;

    // ---- the part table: queries by part count, descending (counting sort; every workgroup builds the
    // same table: ballots and fixed prefix orders only).  Two barriers: the per-(chunk, wave) class counts
    // meet in LDS, then EVERY wave takes the prefixes it needs itself (lane c = class c + 1: the counts of
    // its class in registers, the class offsets by a scalar walk over the lanes) and scatters its own
    // queries; wave 0 also leaves the class table for decode(). ----
    // DIRECT launches (every part of the batch has a workgroup of its own: B * Pmax workgroups, one round) skip
    // the table: workgroup t looks at n[t / Pmax] and is part t % Pmax of that query, or has nothing to do.
    const int chunks = (B + T - 1) / T;
    int *cpre = ccnt + chunks * NW * Pmax;                     // [chunks][Pmax] this wave's offsets (wave-private rows)
    cpre += wl * chunks * Pmax;
    int total = B * Pmax;
    if (!direct) {
    for (int j = 0; j < chunks; ++j) {
        const int q = j * T + tid;
        int Pq = 0;
        if (q < B) {
            const int nq = clamp_n(p.n[q], L);
            nl[q] = nq;
            Pq = (nq + rtarget - 1) / rtarget;
            Pq = Pq < 1 ? 1 : Pq;
        }
        int mine = 0;
        for (int cls = 1; cls <= Pmax; ++cls) {
            const int cnt = __popcll(__ballot(Pq == cls));
            mine = (lane == cls - 1) ? cnt : mine;
        }
        if (lane < Pmax) ccnt[(j * NW + wl) * Pmax + lane] = mine;
    }
    __syncthreads();
    PT_PRO(0);
    {
        const int cc = lane < Pmax ? lane : 0;
        int run = 0;
        for (int j = 0; j < chunks; ++j) {
            int v[NW];
#pragma unroll
            for (int w2 = 0; w2 < NW; ++w2) v[w2] = ccnt[(j * NW + w2) * Pmax + cc];
            int before = run;
#pragma unroll
            for (int w2 = 0; w2 < NW; ++w2) { before += (w2 < wl) ? v[w2] : 0; run += v[w2]; }
            if (lane < Pmax) cpre[j * Pmax + lane] = before;   // queries of my class in earlier (chunk, wave) pieces
        }
        // class offsets, most parts first: a scalar walk over the lanes' totals
        int qs = 0, ts = 0, my_qstart = 0, my_tend = 0;
        for (int cls = Pmax; cls >= 1; --cls) {
            const int cnt = __builtin_amdgcn_readlane(run, cls - 1);
            my_qstart = (lane == cls - 1) ? qs : my_qstart;
            qs += cnt;
            ts += cnt * cls;
            my_tend = (lane == cls - 1) ? ts : my_tend;
        }
        total = ts;                                            // parts in all
        if (wl == 0 && lane < Pmax) { qstart[lane + 1] = my_qstart; tend[lane + 1] = my_tend; }
        for (int j = 0; j < chunks; ++j) {
            const int q = j * T + tid;
            int Pq = 0;
            if (q < B) {
                Pq = (nl[q] + rtarget - 1) / rtarget;
                Pq = Pq < 1 ? 1 : Pq;
            }
            const int off = my_qstart + ((lane < Pmax) ? cpre[j * Pmax + lane] : 0);     // lane c: where my (chunk, wave) piece of class c + 1 starts
            for (int cls = 1; cls <= Pmax; ++cls) {
                const unsigned long long mc = __ballot(Pq == cls);
                const int base = __builtin_amdgcn_readlane(off, cls - 1);
                if (Pq == cls) order[base + __popcll(mc & ((1ull << lane) - 1ull))] = q;
            }
        }
    }
    }       // !direct
    if (tid == 0) misc[6] = 0;
    __syncthreads();
    PT_PRO(1);
    bool ok_wg = true;

    const __amdgpu_buffer_rsrc_t prsrc = __builtin_amdgcn_make_buffer_rsrc(
        pp.pvec, 0, __builtin_amdgcn_readfirstlane((int)min((size_t)0x7fffffff, (size_t)B * Pmax * pp.pitch * 4)), 0x00020000);

    // A part, as every thread sees it (wave-uniform values).
    struct Part { int b, part, P, nb, r0, rows; };
    auto decode = [&](int t) {
        if (direct) {
            Part a;
            a.b = __builtin_amdgcn_readfirstlane(t / Pmax);
            a.part = __builtin_amdgcn_readfirstlane(t - a.b * Pmax);
            a.nb = nb_direct;              // (a DIRECT workgroup decodes one ticket: its block id)
            int Pq = (a.nb + rtarget - 1) / rtarget;
            a.P = Pq < 1 ? 1 : Pq;
            const int rp = (a.nb + a.P - 1) / a.P;
            a.r0 = a.part * rp;
            a.rows = (a.part < a.P) ? max(0, min(rp, a.nb - a.r0)) : -1;       // -1: no such part
            return a;
        }
        int cls = Pmax;
        while (cls > 1 && t >= tend[cls]) --cls;
        const int tfirst = (cls == Pmax) ? 0 : tend[cls + 1];
        const int rel_t = t - tfirst;
        const int qi = rel_t / cls;
        Part a;
        a.part = __builtin_amdgcn_readfirstlane(rel_t - qi * cls);
        a.P = __builtin_amdgcn_readfirstlane(cls);
        a.b = __builtin_amdgcn_readfirstlane(order[qstart[cls] + qi]);
        a.nb = __builtin_amdgcn_readfirstlane(nl[a.b]);
        const int rp = (a.nb + a.P - 1) / a.P;                 // rows per part, balanced
        a.r0 = a.part * rp;
        a.rows = max(0, min(rp, a.nb - a.r0));
        return a;
    };
    // The part's rows, one burst (buffer loads through a descriptor of exactly these rows: anything past
    // them, and the padding lanes, read 0).
    float4 x[NI][CV];
    const int sweep = __builtin_amdgcn_readfirstlane(R * C * 16);
    auto issue = [&](const Part &a, bool landed = false) {
        const uintptr_t xaddr = reinterpret_cast<uintptr_t>(p.X + ((size_t)a.b * L + (size_t)a.r0) * (size_t)F);
        const unsigned xlo = __builtin_amdgcn_readfirstlane((unsigned)xaddr);
        const unsigned xhi = __builtin_amdgcn_readfirstlane((unsigned)(xaddr >> 32));
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
            reinterpret_cast<void *>(((uintptr_t)xhi << 32) | xlo), 0,
            __builtin_amdgcn_readfirstlane(a.rows * F * 4), 0x00020000);
        // (per-thread offsets made opaque once per part: the compiler would otherwise keep NI addresses
        // per access pattern alive across the whole persistent loop -- ~3 * NI registers)
        int voff[CV];
#pragma unroll
        for (int j = 0; j < CV; ++j) {
            voff[j] = (c + j * RS < C) ? (r * C + c + j * RS) * 16 : 0x7ff00000;
            asm volatile("" : "+v"(voff[j]));
        }
        if constexpr (NPF > 0) {
            // (sweeps 0 .. NPF - 1 ALWAYS go through the landing buffer -- one place where those registers are written, at the
            // top of the part: they are free from the dW fold to the dot products; landed: the LDS-DMA is under way already)
            if (!landed) {
                unsigned char *lb = smem + pp.pf_off + wl * 1024;
#pragma unroll
                for (int i = 0; i < NPF; ++i) {
#pragma unroll
                    for (int j = 0; j < CV; ++j) pt_load_lds16(rsrc, lb + (i * CV + j) * (T * 16), voff[j], i * sweep);
                }
            }
        }
#pragma unroll
        for (int i = NPF; i < NI; ++i) {
#pragma unroll
            for (int j = 0; j < CV; ++j) {
                const ltr_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff[j], i * sweep, 0);
                x[i][j] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
            }
        }
    };
    // the first NPF sweeps of part a, straight into the landing buffer (LDS-DMA: rows past the part read 0 there too)
    auto issue_lds = [&](const Part &a) {
        if constexpr (NPF > 0) {
            const uintptr_t xaddr = reinterpret_cast<uintptr_t>(p.X + ((size_t)a.b * L + (size_t)a.r0) * (size_t)F);
            const unsigned xlo = __builtin_amdgcn_readfirstlane((unsigned)xaddr);
            const unsigned xhi = __builtin_amdgcn_readfirstlane((unsigned)(xaddr >> 32));
            const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
                reinterpret_cast<void *>(((uintptr_t)xhi << 32) | xlo), 0,
                __builtin_amdgcn_readfirstlane(a.rows * F * 4), 0x00020000);
            unsigned char *lb = smem + pp.pf_off + wl * 1024;
#pragma unroll
            for (int i = 0; i < NPF; ++i) {
#pragma unroll
                for (int j = 0; j < CV; ++j) {
                    const int vo = (c + j * RS < C) ? (r * C + c + j * RS) * 16 : 0x7ff00000;
                    pt_load_lds16(rsrc, lb + (i * CV + j) * (T * 16), vo, i * sweep);
                }
            }
        }
    };

    // The last part of a query to arrive adds the parked shares and writes the query's row of the (B, PF) partials
    // and its loss.  All threads: thread (column vector col, group grp) takes the shares grp, grp + NG, ... with
    // eight coherent loads in flight (no tile is in the registers where this runs), the groups' sums meet in LDS
    // in a fixed order; the raw pair sum rides in lane y of the last column vector.  Contains barriers.
    auto combine = [&](int qb, int qP) {
        const int CG = C + 1;
        const int NG = T / CG;                                     // (>= 1: C + 1 <= 193)
        const int grp = tid / CG, col = tid - grp * CG;
        if (grp < NG) {
            float4 s4 = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int q0 = grp; q0 < qP; q0 += kPtCombineInflight * NG) {
                ltr_u32x4 v[kPtCombineInflight];
#pragma unroll
                for (int u = 0; u < kPtCombineInflight; ++u) {
                    const int qq = min(q0 + u * NG, qP - 1);
                    v[u] = __builtin_amdgcn_raw_buffer_load_b128(prsrc, ((qb * Pmax + qq) * pp.pitch) * 4 + 16 * col, 0, 16);
                }
#pragma unroll
                for (int u = 0; u < kPtCombineInflight; ++u)
                    if (q0 + u * NG < qP)
                        vadd(s4, make_float4(__uint_as_float(v[u].x), __uint_as_float(v[u].y), __uint_as_float(v[u].z), __uint_as_float(v[u].w)));
            }
            dred[grp * CG + col] = s4;
        }
        __syncthreads();
        float4 tot = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tid < CG)
            for (int g = 0; g < NG; ++g) vadd(tot, dred[g * CG + tid]);
        if (tid == C) { red[30] = tot.y; red[31] = tot.z; }
        __syncthreads();
        if (tid < CG) {
            float gscale;
            const float inv_mx = kNdcg ? 1.0f / (red[31] == 0.0f ? 1.0f : red[31]) : 1.0f;       // the parts' terms of maxDCG, in part order
            const float total_l = parts_finish<KIND>(red[30] * inv_mx, p.sigma, gscale);
            gscale *= inv_mx;
            float4 *dst4 = reinterpret_cast<float4 *>(p.part + (size_t)qb * partial_pitch(F));
            if (tid < C) dst4[tid] = f4_scale(tot, gscale);
            else dst4[C] = make_float4(tot.x * gscale, 0.f, 0.f, 0.f);
            if (tid == 0) p.loss[qb] = total_l;
        }
        __syncthreads();
    };

    int t = (int)blockIdx.x;
#ifdef LTR_TRACE
    if (tid == 0 && t < total) {
        long long *tr = reinterpret_cast<long long *>(p.scores_out) + (size_t)t * 16;
        tr[15] = t_entry; tr[10] = t_pro[0]; tr[11] = t_pro[1];
    }
#endif
    Part cur = {0, 0, 1, 0, 0, 0};
    if (t < total) {
        PT_STAMP(0);
        cur = decode(t);
        if (cur.rows < 0) t = total;            // (DIRECT: this query has fewer parts)
        else issue(cur);
    }
    int pend_b = -1, pend_P = 0;
    while (t < total) {
        const int b = cur.b, part = cur.part, P = cur.P, nb = cur.nb, r0 = cur.r0, rows = cur.rows;
        const size_t row = (size_t)b * L;
        int pdoff = r * SEGP + (c >> 4);
        int goff = r;
        asm volatile("" : "+v"(pdoff), "+v"(goff));
        PT_STAMP(1);
        // labels of the whole query (needed by the pair pass only)
        for (int k = tid; k < nb; k += T) sy[k].y = load_label(p.rel, p.rel_dtype, row + k);
        if (tid == 0) misc[2] = 1;

        // ---- scores of my rows: dot per 16-byte vector, sum over the 16 lanes of a DPP row, fold ----
        float4 w[CV];
#pragma unroll
        for (int j = 0; j < CV; ++j) w[j] = wlds[c + j * RS];
        if constexpr (NPF > 0) {
            // what the landing buffer holds (this wave's own LDS-DMA, the oldest of its memory operations: no barrier)
            const float4 *pf = reinterpret_cast<const float4 *>(smem + pp.pf_off) + tid;
#pragma unroll
            for (int i = 0; i < NPF; ++i) {
#pragma unroll
                for (int j = 0; j < CV; ++j) x[i][j] = pf[(i * CV + j) * T];
            }
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            float d = vdot_pk(x[i][0], w[0]);
#pragma unroll
            for (int j = 1; j < CV; ++j) d += vdot_pk(x[i][j], w[j]);
            d = quad_sum(d);
            d += dpp_move<0x141, 0xF>(d);
            d += dpp_move<0x140, 0xF>(d);
            if ((c & 15) == 0) pd[pdoff + i * (R * SEGP)] = d;
            // (the tile arrives in order: keep the folds in order too, a few at a time, instead of NI dot
            // products in flight -- registers)
            if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        if (pend_b >= 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        PT_STAMP(2);
        // the previous part's arrival (see the finish below); its return is looked at behind the fold and the poll
        int pend_old = 0;
        if (pend_b >= 0 && tid == 0)
            pend_old = __hip_atomic_fetch_add(pp.ctrl + kPtCtrlHeader + pend_b, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int lr = tid; lr < rows; lr += T) {
            float s = bias;
            for (int g = 0; g < SEG; ++g) s += pd[lr * SEGP + g];
            sy[r0 + lr].x = s;
            if (P > 1) pt_st64(pp.sbuf + row + r0 + lr, ((unsigned long long)tag << 32) | __float_as_uint(s));
        }
        PT_STAMP(3);
        // ---- the scores of the other parts.  Kernels without the ranked formulation fetch them tile by tile
        // INSIDE the pair pass (POLL, below): the wait for the slowest part hides behind the tiles that have
        // arrived.  The ranked formulation needs every score first: poll here, up to four per thread in flight ----
        // (the hinge kinds only: the log-sigmoid kinds' pass is several times longer and their kernels have no
        // registers to spare for it)
        constexpr bool kPollInPass = !RK && (KIND == LTR_HINGE || KIND == LTR_DCG_HINGE);
        if (!kPollInPass && P > 1) {
            bool okw = true;
            for (int k0 = 0; k0 < nb; k0 += 4 * T) {
                unsigned need = 0;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int k = k0 + u * T + tid;
                    if (k < nb && (k < r0 || k >= r0 + rows)) need |= 1u << u;
                }
                int spins = 0;
                while (__ballot(need != 0) != 0ull) {
                    unsigned long long gv[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        gv[u] = (need >> u & 1u) ? pt_ld64(pp.sbuf + row + k0 + u * T + tid) : 0ull;
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        if ((need >> u & 1u) && (unsigned)(gv[u] >> 32) == tag) {
                            sy[k0 + u * T + tid].x = __uint_as_float((unsigned)gv[u]);
                            need &= ~(1u << u);
                        }
                    }
                    if (__ballot(need != 0) == 0ull) break;
                    if (++spins > pp.spin_limit) { okw = false; break; }
                    __builtin_amdgcn_s_sleep(kPtSleep);
                }
            }
            if (!okw && lane == 0) misc[2] = 0;
        }
        if (pend_b >= 0 && tid == 0 && pend_old == pend_P - 1) {
            // the last to arrive: the query's sum is this workgroup's, taken at the end of the kernel
            pt_st32(pp.ctrl + kPtCtrlHeader + pend_b, 0);
            const int cnt = misc[6];
            doneq[cnt] = pend_b | (pend_P << 24);
            misc[6] = cnt + 1;
        }
        pend_b = -1;
        // (LDS-only barriers in the loop where nothing in global memory is handed over inside the workgroup: __syncthreads()
        // would make the publishing wave wait for the acknowledgement of its granule stores, and the others for that wave)
        lds_barrier();                      // (my rows' scores, the labels -- and with the poll above every score -- are in sy)
        PT_STAMP(4);
        // a part draws its next ticket only once it no longer waits for anybody: here when every score is in,
        // behind the pair pass when the pass itself still polls
        int tnext = 0;
        if (!kPollInPass) {
            if (!misc[2]) ok_wg = false;
            if (!kNdcg && tid == 0) tnext = direct ? total : G + __hip_atomic_fetch_add(pp.ctrl + 4, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }

        // ---- the NDCG kinds (round 4): a part ranks ITS rows against the whole query (keyed counting rank on the
        // exchanged scores and on the labels: rows * n compares over the workgroup instead of two sorts of the
        // whole list per part), publishes the score ranks as a second set of tagged granules and collects the other
        // parts'; its rows' terms of maxDCG ride in its share and meet in the combine, where 1 / maxDCG scales the
        // query's loss and gradient once (every pair term of both kinds carries that factor) ----
        float mx_part = 0.f;
        if constexpr (kNdcg) {
            ulonglong2 *keys = reinterpret_cast<ulonglong2 *>(nq.rank_s + 2 * Ls);
            for (int k = tid; k < nb; k += T) {
                const float2 v = sy[k];
                keys[k] = make_ulonglong2(rank_key(v.x, k), rank_key(v.y, k));
            }
            for (int lr = tid; lr < rows; lr += T) { nq.rank_s[r0 + lr] = 0; nq.rank_y[lr] = 0; }
            if (KIND == LTR_NDCG2) fill_ndcg2_delta(nq.delta, nb, Ls, tid, T);
            __syncthreads();
            {
                // thread = (my row o, slice of the list): partial counts meet in LDS (integer adds: any order)
                const int owners = (rows <= 64) ? 64 : ((rows <= 128) ? 128 : 256);
                const int ms = T / owners;
                const int sl = __builtin_amdgcn_readfirstlane(tid / owners);
                const int mlen = (nb + ms - 1) / ms;
                const int m0 = __builtin_amdgcn_readfirstlane(min(nb, sl * mlen));
                const int m1 = __builtin_amdgcn_readfirstlane(min(nb, m0 + mlen));
                // (a part of more rows than the workgroup has threads -- very narrow feature rows -- takes them in blocks)
                for (int o = tid & (owners - 1); o < rows; o += owners) {
                    const ulonglong2 kk = keys[r0 + o];
                    int cs = 0, cy = 0;
#pragma unroll 4
                    for (int m = m0; m < m1; ++m) {
                        const ulonglong2 v = keys[m];
                        cs += (v.x < kk.x);
                        cy += (v.y < kk.y);
                    }
                    atomicAdd(&nq.rank_s[r0 + o], cs);
                    atomicAdd(&nq.rank_y[o], cy);
                }
            }
            __syncthreads();
            float mxp = 0.f;
            for (int lr = tid; lr < rows; lr += T) {
                const int rs = nq.rank_s[r0 + lr];
                if (P > 1) pt_st64(pp.slices + row + r0 + lr, ((unsigned long long)tag << 32) | (unsigned)rs);
                mxp = __builtin_fmaf(ndcg_gain(sy[r0 + lr].y), inv_discount((float)nq.rank_y[lr]), mxp);
            }
            {
                const float ws = wave_sum(mxp);
                if (lane == 0) red[8 + wl] = ws;
            }
            if (P > 1) {
                bool okw = true;
                for (int k0 = 0; k0 < nb; k0 += 4 * T) {
                    unsigned need = 0;
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int k = k0 + u * T + tid;
                        if (k < nb && (k < r0 || k >= r0 + rows)) need |= 1u << u;
                    }
                    int spins = 0;
                    while (__ballot(need != 0) != 0ull) {
                        unsigned long long gv[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            gv[u] = (need >> u & 1u) ? pt_ld64(pp.slices + row + k0 + u * T + tid) : 0ull;
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            if ((need >> u & 1u) && (unsigned)(gv[u] >> 32) == tag) {
                                nq.rank_s[k0 + u * T + tid] = (int)(unsigned)gv[u];
                                need &= ~(1u << u);
                            }
                        }
                        if (__ballot(need != 0) == 0ull) break;
                        if (++spins > pp.spin_limit) { okw = false; break; }
                        __builtin_amdgcn_s_sleep(kPtSleep);
                    }
                }
                if (!okw && lane == 0) misc[2] = 0;
            }
            __syncthreads();
            if (!misc[2]) ok_wg = false;
            // nobody is waited for any more: the next ticket
            if (tid == 0) tnext = direct ? total : G + __hip_atomic_fetch_add(pp.ctrl + 4, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (int k = tid; k < nb; k += T) {
                const float2 v = sy[k];
                const float g = ndcg_gain(v.y);
                const int rr = nq.rank_s[k];
                if (KIND == LTR_NDCG1) sy[k].y = g * inv_discount((float)rr);       // a_k * maxDCG
                else nq.q4[k] = make_float4(v.x, v.y, g, (float)rr);
            }
#pragma unroll
            for (int i = 0; i < NW; ++i) mx_part += red[8 + i];
            __syncthreads();
        }

        // ---- d pair-sum / d s of my rows and my share of the pair sum: the counting formulation for the hinge
        // kinds on long lists of integer grades, else the pair pass ----
        float raw = 0.f;
        bool ranked = false;
        if constexpr (RK && (KIND == LTR_HINGE || KIND == LTR_DCG_HINGE)) {
            // (measured, MI355X: the tables cost ~11-14 us per part whatever the list -- a dozen barriers of
            // latency-bound scans and scatters on four waves -- the pair pass rows * n / 64 steps over four waves:
            // 160 rows x 1000 documents 25 us, 56 x 512 5 us; the crossing is near rows * n = 80 000)
            // The choice is per QUERY (rows of a full part, not of this one): a ranked part reports the pairs its
            // rows WIN, a pair-pass part half of everything its rows take part in -- the two do not mix.
            if (pp.rank_lds && nb >= kPtRankMinN && nb <= kPtRankMaxN && (long long)((nb + P - 1) / P) * nb >= kPtRankMinWork)
#ifdef LTR_TRACE
                ranked = parts_hinge_ranked(nb, r0, rows, rpw, (unsigned)(rk - smem), (unsigned)(reinterpret_cast<unsigned char *>(gloc) - smem),
                                            (unsigned)(reinterpret_cast<unsigned char *>(rscr) - smem), raw,
                                            reinterpret_cast<long long *>(p.scores_out) + (size_t)t * 16);
#else
                ranked = parts_hinge_ranked(nb, r0, rows, rpw, (unsigned)(rk - smem), (unsigned)(reinterpret_cast<unsigned char *>(gloc) - smem),
                                            (unsigned)(reinterpret_cast<unsigned char *>(rscr) - smem), raw);
#endif
        }
        if (!ranked) {
            float lacc;
            const bool intlab = (KIND == LTR_HINGE || KIND == LTR_DCG_HINGE) && p.rel_dtype != LTR_LABEL_F32;
            if constexpr (kNdcg) {
                lacc = parts_pair_pass<KIND, false, false>(sy, nb, r0, rows, p.sigma, gw + wl * rpwp, wl, lane, nullptr, 0u, 0, nullptr,
                                                           nq.q4, nq.delta);
            } else if (kPollInPass && P > 1) {
                bool okw = true;
                lacc = intlab ? parts_pair_pass<KIND, true, true>(sy, nb, r0, rows, p.sigma, gw + wl * rpwp, wl, lane, pp.sbuf + row, tag,
                                                                  pp.spin_limit, &okw)
                              : parts_pair_pass<KIND, true, false>(sy, nb, r0, rows, p.sigma, gw + wl * rpwp, wl, lane, pp.sbuf + row, tag,
                                                                   pp.spin_limit, &okw);
                if (!okw && lane == 0) misc[2] = 0;
            } else {
                lacc = intlab ? parts_pair_pass<KIND, false, true>(sy, nb, r0, rows, p.sigma, gw + wl * rpwp, wl, lane)
                              : parts_pair_pass<KIND, false, false>(sy, nb, r0, rows, p.sigma, gw + wl * rpwp, wl, lane);
            }
            const float ws = wave_sum(lacc);
            if (lane == 0) red[wl] = ws;
        }
        if (!kPollInPass && tid == 0) misc[0] = tnext;
        lds_barrier();
        PT_STAMP(5);
        if (kPollInPass) {
            if (!misc[2]) ok_wg = false;
            if (tid == 0) tnext = direct ? total : G + __hip_atomic_fetch_add(pp.ctrl + 4, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // ---- the next part is known: the first sweeps of its tile start for the landing buffer, under the gradient / dW phase ----
        bool landed = false;
        if constexpr (NPF > 0) {
            if (pf_on) {
                const int tnb = __builtin_amdgcn_readfirstlane(misc[0]);
                if (tnb < total) {
                    const Part nxt = decode(tnb);
                    issue_lds(nxt);
                    landed = true;
                }
            }
        }
        if (!ranked) {
#pragma unroll
            for (int i = 0; i < NW; ++i) raw += red[i];
            for (int lr = tid; lr < rpw; lr += T) {
                float g = 0.f;
                if (lr < rows) {
#pragma unroll
                    for (int i = 0; i < NW; ++i) g += gw[i * rpwp + lr];
                }
                gloc[lr] = g;
            }
        }
        lds_barrier();              // (the ticket drawn behind the pair pass stays in flight under the dW fold)

        // ---- dW share straight from the registers; the bias is the feature column of ones ----
        {
            float4 acc[CV];
#pragma unroll
            for (int j = 0; j < CV; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            float gb = 0.f;
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const float g = gloc[goff + i * R];
#pragma unroll
                for (int j = 0; j < CV; ++j) {
                    const float4 xv = x[i][j];
                    vfma(acc[j], g, xv);
                }
                gb += g;
                if ((i & 7) == 7) __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int j = 0; j < CV; ++j) dred[r * RSC + j * RS + c] = acc[j];
            if (c == 0) pd[r] = gb;
        }
        if (kPollInPass && tid == 0) misc[0] = tnext;         // (the ticket drawn behind the pair pass)
        __syncthreads();
        // column vector tid of the query's row (C <= kPtMaxCV * 64 < T); thread C carries (d/d bias, raw pair sum)
        float4 share = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tid < C) {
            for (int rr = 0; rr < R; ++rr) vadd(share, dred[rr * RSC + tid]);
        } else if (tid == C) {
            float sb = 0.f;
            for (int rr = 0; rr < R; ++rr) sb += pd[rr];
            share = make_float4(sb, raw, kNdcg ? mx_part : 0.f, 0.f);
        }
        PT_STAMP(6);
        // ---- the registers are free: the NEXT part's rows are requested before this part is finished off ----
        const int tn = misc[0];
        float4 *part4 = reinterpret_cast<float4 *>(p.part + (size_t)b * partial_pitch(F));
        const float poison = ok_wg ? 1.0f : __builtin_nanf("");
        // (the burst is issued on EVERY path -- with no part left, through an empty descriptor: every load returns 0
        // without touching memory.  A path on which the tile registers keep their old contents makes them live
        // around the whole loop body for the register allocator: a dozen spilled vectors)
        const Part none = {0, 0, 1, 0, 0, 0};
        if (P == 1) {
            cur = (tn < total) ? decode(tn) : none;
            issue(cur, landed);
            float gscale;
            const float inv_mx = kNdcg ? 1.0f / (mx_part == 0.0f ? 1.0f : mx_part) : 1.0f;      // loss/pairwise_lambda.py:227
            const float total_l = parts_finish<KIND>(raw * inv_mx, p.sigma, gscale) * poison;
            gscale *= poison * inv_mx;
            if (tid < C) part4[tid] = f4_scale(share, gscale);
            else if (tid == C) part4[C] = make_float4(share.x * gscale, 0.f, 0.f, 0.f);
            if (tid == 0) p.loss[b] = total_l;
        } else {
            // park my share (write-through) and arrive; the last part of the query adds the shares in part
            // order.  Order of the memory operations: share stores, their acknowledgement, the arrival
            // atomic, THEN the next part's loads -- the atomic's return is older than the loads, so the
            // wave that needs it does not wait for the features.
            const int slot = b * Pmax + part;
            if (tid <= C) {
                const float4 sv = f4_scale(share, poison);
                ltr_u32x4 v;
                v.x = __float_as_uint(sv.x); v.y = __float_as_uint(sv.y); v.z = __float_as_uint(sv.z); v.w = __float_as_uint(sv.w);
                __builtin_amdgcn_raw_buffer_store_b128(v, prsrc, (slot * pp.pitch + 4 * tid) * 4, 0, 16);
            }
            const bool on_the_spot = tn >= total;
            if (!on_the_spot) {
                pend_b = b;
                pend_P = P;
                cur = decode(tn);
                issue(cur, landed);
            } else {
                cur = none;
                issue(cur);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                if (tid == 0) {
                    const int old = __hip_atomic_fetch_add(pp.ctrl + kPtCtrlHeader + b, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const int last = (old == P - 1) ? 1 : 0;
                    if (last) pt_st32(pp.ctrl + kPtCtrlHeader + b, 0);
                    misc[1] = last;
                }
                __syncthreads();
            }
            // (the sum itself is taken behind the loop -- this was the workgroup's last part --, where no tile
            // occupies the registers: eight shares per thread in flight)
            if (on_the_spot && misc[1] && tid == 0) {
                const int cnt = misc[6];
                doneq[cnt] = b | (P << 24);
                misc[6] = cnt + 1;
            }
        }
        PT_STAMP(7);
#ifdef LTR_TRACE
        if (tid == 0) reinterpret_cast<long long *>(p.scores_out)[(size_t)t * 16 + 8] = ((long long)b << 32) | (part << 16) | (P << 8) | (rows & 0xff);
        if (tid == 0) reinterpret_cast<long long *>(p.scores_out)[(size_t)t * 16 + 9] = (long long)blockIdx.x;
#endif
        lds_barrier();             // (misc / sy / pd are rewritten by the next part; the share stores are waited for where the
                                   // arrival needs them: in front of the barrier behind the next part's dot products)
        t = tn;
#ifdef LTR_TRACE
        if (t < total) PT_STAMP(0);
#endif
    }

    // ---- the sums of the queries whose last arrival was one of this workgroup's deferred ones ----
    __syncthreads();
    {
        const int ndone = misc[6];
        for (int i = 0; i < ndone; ++i) {
            const int e = doneq[i];
            combine(e & 0xffffff, e >> 24);
        }
    }

    // ---- leave: the last workgroup resets the ticket counter and opens the next tag ----
    if (tid == 0) {
        // a wait gave up: the step is invalid -- say so where the host sees it (the host zeroes the exchange
        // areas once the status has been cleared: ltr_device_status)
        if (!ok_wg && pp.status) __hip_atomic_store(pp.status, (int)LTR_ERR_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const int old = __hip_atomic_fetch_add(pp.ctrl + 5, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        misc[1] = (old == G - 1) ? 1 : 0;
    }
    __syncthreads();
    if (misc[1]) {
        unsigned next = tag + 1u;
        if (next == 0u) {
            // the last tag there is: every granule goes back to 0 before the tags start over at 1 (once per
            // 2^32 - 1 launches on this area; nobody else is left in this launch, the next one is behind the
            // kernel boundary)
            ulonglong2 *g2 = reinterpret_cast<ulonglong2 *>(pp.sbuf);
            const unsigned long long n2 = pp.gran_words >> 1;
            for (unsigned long long i = (unsigned long long)tid; i < n2; i += T) g2[i] = make_ulonglong2(0ull, 0ull);
            next = 1u;
            __syncthreads();
        }
        if (tid == 0) {
            pt_st32(pp.ctrl + 5, 0);
            pt_st32(pp.ctrl + 4, 0);
            pt_st32(pp.ctrl + 0, (int)next);
        }
    }
}

struct PartsShape { int ni, cv, wpc, RS, R, rpw, rtarget, Pmax, pitch, grid, mode, direct; size_t lds; size_t gran_words, misc_bytes; unsigned pf_off; };

constexpr int kPtMinL = 256;

// tests (ltr_debug_parts_all): every shape the kernel can take, whatever the measured rule says
inline int &parts_debug_all() { static int v = 0; return v; }

// Shapes the parts kernel takes: rank-free kinds, rows of whole float4 up to kPtMaxCV * 64 vectors, lists
// too long for the register tile.  A row's C = F/4 column vectors are dealt to RS lanes (a power of two,
// 16 .. 64) with CV = ceil(C / RS) vectors per lane; RS is the choice that wastes the fewest registers.
bool choose_parts_shape(int kind, int B, int L, int F, PartsShape &s)
{
    const bool ndcg = (kind == LTR_NDCG1 || kind == LTR_NDCG2);
    // (lists of 64 .. 256 documents: only where measured -- below)
    if (L > kMaxListLen || L < 64) return false;
    // (the NDCG kinds, round 4: lists up to the symmetric pass's length -- the rank arrays, keys and the discount
    // table live in the part's LDS)
    if (ndcg && L > kSymMaxLen) return false;
    if (F % 4 != 0 || B > kPtMaxB || B < 1) return false;
    const int C = F / 4;
    if (C > kPtMaxCV * 64) return false;
    const int cus = device_cu_count();
    // Where it pays against the one-workgroup-per-query kernels (measured, MI355X; profiles/README.md):
    //   * lists beyond the symmetric pass (L > 1024), where the general kernel visits both ends too and reads
    //     the features twice: 512 x 2000 x 64 678 -> 381 us, 256 x 4000 x 32 1030 -> 704;
    //   * wide rows (>= 112 float4): 512 x 512 x 700 121 -> 108, 1024 x 512 x 700 250 -> 222.
    // Lists the symmetric pass still takes (L <= 1024): against the general kernel (one workgroup per query, the
    // symmetric pair pass, features read twice) the one-sided parts win on WIDE rows only, and not on batches of
    // one workgroup per CU or fewer.  Measured cold (two batches in rotation, MI355X, round 4 session 3:
    // profiles/r04_parts_vs_general.txt), time parts / general:
    //   C = 112  (F 448): hinge 1.01 / 1.02 / 1.01 / 0.89 (512 x 300, 512 x 512, 1024 x 400, 2048 x 300), 768 x 1000: 1.22;
    //                     logistic 1.13-1.35, arp1 1.24-1.46
    //   C = 128  (F 512): hinge 0.99 / 0.97 / 0.90 (512 x 300, 512 x 512, 1024 x 512), 384 x 1000: 1.03; logistic 1.05-1.12; arp1 1.14-1.23
    //   C = 144  (F 576): hinge 0.90 / 0.91; logistic 0.97; arp1 1.04
    //   C = 160  (F 640): hinge 0.95 / 0.88 / 0.83; logistic 0.98 / 0.90 / 0.93; arp1 1.03 / 0.98 / 0.98
    //   C = 175  (F 700): 256 x 300: 1.47 / 1.29 / 1.32 (!), 320 x 400: 0.87 / 0.89 / 0.96, 320 x 768: 0.73 / 0.71 / 0.79,
    //                     512 x 512 (C5): 0.85 / 0.90 / 0.98, 1024 x 300: 0.79 / 0.85 / 0.90
    //   NDCG kinds (a second exchange, of ranks; wide rows): 128 x 512 x 700 0.62, 256 x 1000 x 700 0.79-0.84, 512 x 512 x 700 0.97,
    //                     512 x 400 x 700 0.95, 1024 x 512 x 700 1.04, 384 x 512 x 640 1.07, 256 x 768 x 512 1.14-1.22
    //   underfilled general kernel (B <= #CUs; F 700 unless noted): 256 x 300: 1.47 / 1.29 / 1.32, 192 x 400: 1.21 / 0.98 / 1.00,
    //                     256 x 400: 0.80 / 0.75 / 0.80, 192 x 512: 0.78 / 0.74 / 0.75, 256 x 512: 0.76 / 0.77 / 0.83,
    //                     256 x 768: 0.69 / 0.67 / 0.75, 256 x 1000: 0.64 / 0.63 / 0.69, 160 x 1000 x 512: 0.60 / 0.55 / 0.57
    if (!parts_debug_all() && L <= kPtMinL) {
        // Short lists (the general kernel reads the features twice and is bandwidth-bound on that at wide rows: Yahoo-
        // shaped batches, 700 features, lists of ~100-250 documents), cold, parts / general, hinge / logistic:
        //   2048 x 128 x 700 0.81 / 0.81    1024 x 256 x 700 0.80 / 0.86    1024 x 200 x 700 0.86 / 0.92    512 x 256 x 640 0.88 / 0.93
        //   1024 x 128 x 700 0.98 / 0.92    1024 x 128 x 512 0.95 / 1.04    1024 x 200 x 448 1.03 / 1.17 (!)
        //   512 x 128 x 700 1.48 / 1.43 (!)  256 x 256 x 700 1.55 / 1.39 (!)   LambdaNDCG2: 0.92 ... 1.25 -- never
        if (ndcg || C < 160 || B < 512 || (long long)B * L < 130000) return false;
    } else if (!parts_debug_all() && L <= kSymMaxLen) {
        if (ndcg) {
            // wide rows as above; or batches that leave the general kernel's one workgroup per query CUs empty, on
            // long lists (any row width; parts / general, NDCG1 / NDCG2: 128 x 1000 x 136 0.55 / 0.81, 192 x 1000 x 136
            // 0.66 / 0.94, 128 x 1000 x 220 0.61 / 0.72, 192 x 700 x 220 0.83 / 0.95, 160 x 1000 x 512 0.64 / 0.79,
            // 128 x 700 x 448 0.65 / 0.69; but 256 x 1000 x 136 1.04 / 1.22, 256 x 1000 x 220 1.15 / 1.27, 128 x 512 x 220 1.02;
            // the smallest batches go to the cluster kernel first)
            // (second sweep: 200 x 768 x 512 0.71 / 0.90, 200 x 600 x 448 0.74 / 0.76, 192 x 512 x 512 0.80 / 0.82, 256 x 1000 x 640 0.83 / 0.84,
            // but 256 x 768 x 512 1.13 / 1.16, 224 x 1000 x 512 1.00 / 1.03, 256 x 600 x 512 0.97 / 0.98)
            const bool wide = ((C >= 168 && L >= 400) || (C >= 160 && L >= 768)) && (long long)B * L <= 300000;
            const bool underfilled = 5 * B <= 4 * cus && (L >= 600 || (C >= 112 && L >= 512));
            if (!wide && !underfilled) return false;
        } else {
            if ((long long)B * L < 90000) return false;
            const bool hinge = (kind == LTR_HINGE || kind == LTR_DCG_HINGE);
            int cmin;
            if (B <= cus) cmin = (L >= 600) ? 112 : 128;       // (200 x 768 x 448 hinge / logistic 59.9 / 75.7 us; the cluster kernel 84.7 / 96.1)
            else cmin = hinge ? (B >= 4 * cus ? 128 : 144) : (kind == LTR_ARP1 ? 160 : 144);
            if (C < cmin) return false;
            if (kind == LTR_ARP1 && B > cus && L < 400) return false;
        }
    }
    s.RS = 0;
    for (int rs = 16; rs <= 64; rs *= 2) {
        const int cv = (C + rs - 1) / rs;
        if (cv > kPtMaxCV) continue;
        if (s.RS == 0 || cv * rs < s.cv * s.RS) { s.RS = rs; s.cv = cv; }
    }
    if (s.RS == 0) return false;
    s.R = kPtThreads / s.RS;
    // workgroups per CU (2 / 3 / 4, i.e. 256 / 168 / 128 VGPRs): the heaviest that still gives every CU-slot
    // a few parts
    s.wpc = 0;
    for (int wpc = 2; wpc <= 4 && s.wpc == 0; ++wpc) {
        const int rpw = parts_ni(wpc, s.cv, false, kind) * s.R;
        const long long parts = (long long)B * ((L / 2 + rpw - 1) / rpw);
        if (parts >= 2LL * wpc * cus || wpc == 4) s.wpc = wpc;
    }
    if (ndcg && s.wpc > 3) s.wpc = 3;
    for (;; --s.wpc) {              // (too many parts per query, or too much LDS for that many workgroups: heavier ones)
        // the counting formulation of the hinge kinds (lists beyond the symmetric pass): its call takes registers
        // from the tile, so its kernels hold fewer sweeps -- taken when a part of THAT size can reach the threshold
        bool rank = false;
        if (s.wpc == 2 && parts_rank_lds_bytes(kind, L) > 0) {          // (the heaviest workgroups only: six kernels)
            const int rpw_r = parts_ni(s.wpc, s.cv, true) * s.R;
            rank = (long long)rpw_r * L >= kPtRankMinWork;
        }
        for (int attempt = 0; attempt < 2; ++attempt, rank = false) {
            s.ni = parts_ni(s.wpc, s.cv, rank, kind);
            s.rpw = s.ni * s.R;
            // rows per part aimed at: a full tile (a one-sided part's work does not shrink with its rows)
            s.rtarget = s.rpw;
            s.Pmax = (L + s.rtarget - 1) / s.rtarget;
            s.pitch = (F + 2 + 3) & ~3;
            s.gran_words = (size_t)B * L + (ndcg ? (size_t)B * L : 0);     // (NDCG kinds: rank granules)
            s.mode = rank ? PT_RANKED : PT_ONESIDED;
            s.lds = parts_lds_bytes(B, L, s.RS, s.R, s.cv, s.rpw, s.Pmax, rank ? kind : -1, kind);
            // the landing buffer for the next part's first sweeps, where the LDS of a workgroup has room for it
            s.pf_off = 0;
            {
                const size_t pf_bytes = 16 * (size_t)kPtThreads * (size_t)(parts_pf_sweeps(s.wpc, s.cv) * s.cv);
                if (s.mode == PT_ONESIDED && (kind == LTR_LOGISTIC || kind == LTR_ARP1 || kind == LTR_ARP2) && pf_bytes > 0 && s.lds + pf_bytes <= kLdsBudget / s.wpc) {
                    s.pf_off = (unsigned)s.lds;
                    s.lds += pf_bytes;
                }
            }
            if (s.Pmax <= kPtMaxParts && s.lds <= kLdsBudget / s.wpc) break;
            if (!rank) break;                    // (second attempt: without the tables of the ranked formulation)
        }
        if (s.Pmax <= kPtMaxParts && s.lds <= kLdsBudget / s.wpc) break;
        if (s.wpc == 2) return false;
    }
    s.gran_words = (s.gran_words + 1) & ~(size_t)1;
    const long long items = (long long)B * s.Pmax;
    const long long slots = (long long)s.wpc * cus;
    // one round: every part gets a workgroup of its own and no table is built (DIRECT)
    s.direct = (items <= slots) ? 1 : 0;
    s.grid = (int)(items < slots ? items : slots);
    if (s.grid < s.Pmax) s.grid = s.Pmax;           // (forward progress: more running workgroups than parts per query)
    const size_t pv = (size_t)B * s.Pmax * s.pitch;
    if (pv * 4 > 0x7fffffffull) return false;
    s.misc_bytes = kPtCtrlBytes + pv * 4;
    return true;
}

template <int KIND, int CV, int WPC, int MODE, bool PF = false>
int launch_parts_mode(const PartsParams &pp, const PartsShape &s, hipStream_t stream)
{
    const dim3 grid((unsigned)s.grid), block((unsigned)kPtThreads);
    LTR_ENSURE_LDS((linear_parts_kernel<KIND, parts_ni(WPC, CV, MODE == PT_RANKED, KIND), CV, WPC, MODE, PF>), s.lds);
    hipLaunchKernelGGL((linear_parts_kernel<KIND, parts_ni(WPC, CV, MODE == PT_RANKED, KIND), CV, WPC, MODE, PF>), grid, block, s.lds, stream, pp);
    return (int)hipGetLastError();
}

template <int KIND, int CV, int WPC>
int launch_parts_wpc(const PartsParams &pp, const PartsShape &s, hipStream_t stream)
{
    if constexpr ((KIND == LTR_HINGE || KIND == LTR_DCG_HINGE) && WPC == 2) {
        if (s.mode == PT_RANKED) return launch_parts_mode<KIND, CV, WPC, PT_RANKED>(pp, s, stream);
    }
    if (s.mode == PT_RANKED) return LTR_ERR_CONFIG;
    if constexpr ((KIND == LTR_LOGISTIC || KIND == LTR_ARP1 || KIND == LTR_ARP2) && parts_pf_sweeps(WPC, CV) > 0) {
        if (pp.pf_off) return launch_parts_mode<KIND, CV, WPC, PT_ONESIDED, true>(pp, s, stream);
    }
    return launch_parts_mode<KIND, CV, WPC, PT_ONESIDED>(pp, s, stream);
}

template <int KIND, int CV>
int launch_parts_cv(const PartsParams &pp, const PartsShape &s, hipStream_t stream)
{
    if constexpr (KIND == LTR_NDCG1 || KIND == LTR_NDCG2) {      // (two or three workgroups per CU: choose_parts_shape)
        if (s.wpc == 2) return launch_parts_wpc<KIND, CV, 2>(pp, s, stream);
        if (s.wpc == 3) return launch_parts_wpc<KIND, CV, 3>(pp, s, stream);
        return LTR_ERR_CONFIG;
    } else {
    switch (s.wpc) {
    case 2: return launch_parts_wpc<KIND, CV, 2>(pp, s, stream);
    case 3: return launch_parts_wpc<KIND, CV, 3>(pp, s, stream);
    case 4: return launch_parts_wpc<KIND, CV, 4>(pp, s, stream);
    default: return LTR_ERR_CONFIG;
    }
    }
}

template <int KIND>
int launch_parts_kind(const PartsParams &pp, const PartsShape &s, hipStream_t stream)
{
    switch (s.cv) {
    case 1: return launch_parts_cv<KIND, 1>(pp, s, stream);
    case 2: return launch_parts_cv<KIND, 2>(pp, s, stream);
    case 3: return launch_parts_cv<KIND, 3>(pp, s, stream);
    default: return LTR_ERR_CONFIG;
    }
}

int launch_parts(int kind, const LinearParams &p, const PartsShape &s, hipStream_t stream)
{
    PartsParams pp;
    pp.pf_off = (s.mode == PT_ONESIDED) ? s.pf_off : 0;
    pp.lp = p;
    pp.status = status_device_ptr(stream);
    pp.spin_limit = cluster_force_timeout() ? -1 : kPtSpinLimit;
    pp.Pmax = s.Pmax; pp.rpw = s.rpw; pp.rtarget = s.rtarget; pp.pitch = s.pitch; pp.RS = s.RS; pp.R = s.R;
    pp.rank_lds = (s.mode == PT_RANKED) ? 1 : 0;
    pp.direct = s.direct;
    pp.Lg = (p.L + 63) & ~63;
    pp.sort_min = -1;
    pp.park_off = s.pf_off ? s.pf_off : (unsigned)s.lds;
    // the exchange area of this (device, stream): granule buffers | control block + shares
    unsigned char *gran = nullptr, *misc = nullptr;
    size_t gran_have = 0;
    if (const int rc = exchange_area_get(stream, s.gran_words * 8, s.misc_bytes, &gran, &misc, &gran_have)) return rc;
    const size_t B = (size_t)p.B, L = (size_t)p.L;
    pp.sbuf = reinterpret_cast<unsigned long long *>(gran);
    pp.slices = pp.sbuf + B * L;
    // (the WHOLE granule area, not this launch's share of it: a tag wrap must also clear what a larger shape of an earlier launch
    // left behind -- ADVICE r4)
    pp.gran_words = (unsigned long long)(gran_have / 8);
    pp.ctrl = reinterpret_cast<int *>(misc);
    pp.pvec = reinterpret_cast<float *>(misc + kPtCtrlBytes);
    return with_kind(kind, [&](auto K) { return launch_parts_kind<K>(pp, s, stream); });
}

}  // namespace
