// ltr_mlp2_bf16.inc -- the training step of the fused ReLU-MLP scorer (F -> H1 -> H2 -> 1) on a bf16 feature batch: the
// query loop of mlp_tile_kernel (ltr_mlp2.inc) on the data path of the bf16 front (ltr_mlp_bf16.inc), one MFMA launch
// for scores, loss, d loss / d score and the six parameter gradients (include/ltr_mlp_step_bf16.h).  Included by
// ltr_mlp.hip behind both; the host side of the step is ltr_mlp_step.inc (mlp_step_launch, x_bf16), which needs only the
// two functions at the end of this file.  DESIGN.md section 30.
//
// What is the tile kernel's: 256 threads = four waves, one per 16-row tile of hidden-1, two workgroups per CU; fills of
// 32 documents, the next one requested into registers (buffer loads sized to the rows the query has: rows past n[b]
// return 0 and are never requested from memory) while the current one is computed; mlp_schedule; a query of R > 1
// fills runs forward over fills 0 .. R-1 with the layer-1 tiles and layer-2 rows of all but the last parked in LDS,
// then the loss slot (carve_query_lds<KIND>, the ten KINDs), then backward over fill R-1 (still in the image) down to 0,
// each fetched a second time; dW1 / dW2 tiles in registers across the workgroup's queries; one partial vector per
// workgroup in the pitch mlp_reduce_launch and mlp_reduce_update_launch read.  Fixed assignment, fixed summation
// orders, no atomics: bit-identical run to run.
// What is the bf16 front's (MlpFrontBf16<KS>): X stays bf16 from HBM to the MFMA -- the image is [32][32 KS + 8] bf16
// (pitch: an odd number of 16-byte units), a fill is moved in 16-byte pieces of 8 values and never widened, the columns
// F .. 32 KS + 7 are zeros written once (K is padded in the image, not in HBM).  Layer 1 is v_mfma_f32_16x16x32_bf16: A =
// the wave's W1 rows, loaded from the fp32 master weights once per workgroup, rounded to bf16 (nearest even), KS x 4
// VGPRs; B = one ds_read_b128 of an image row; C/D as v_mfma_f32_16x16x4_f32, so layers 2 and 3, dH2, dH1 and dW2 are
// the fp32 chains of the stand-alone kernels (ltr_mlp_stream.inc, the layout of ltr_mlp2.inc).  dW1: a fill is ONE
// K = 32 step per 16 x 16 output tile, dH1 as hi = bf16(d), lo = bf16(d - hi), two MFMAs into one accumulator, X through
// ds_read_b64_tr_b16 straight from the image.  That step always spans the 32 rows: every fill writes all 32 image rows
// (zeros past the query's length), and the dH1 rows of a subtile without a document are zeros.
// NUMERICS: those of include/ltr_mlp_bf16.h.  The function is mlp(X; bf16(W1), b1, W2, b2, W3, b3); products of layer
// 1 are exact and accumulate in fp32, everything behind it is fp32; dW1 is the gradient with respect to the rounded
// W1 (straight-through), with d loss / d H1 as a sum of two bf16 terms (relative error 2^-17).
// Lists up to 128 documents (four fills, parked).  The 129 .. 256 class of the fp32 tile recomputes the forward pass in
// its backward pass -- a second body and ten more instantiations per bucket -- and is declined: the pieces run.
// Feature buckets by K-steps, KS = 2 / 5 (F <= 64 / 160): 20 instantiations, none spills, all run two workgroups per
// CU.  F = 168 .. 224 (KS = 7: 28 W1 + 56 dW1 registers) is declined by the plan: nine of the ten loss slots spill at
// the 256 registers two workgroups per CU leave a wave (DESIGN.md section 30 has the counts); the pieces run there.
#pragma once

#include "ltr_mlp_step_bf16.h"

constexpr int kM2Bf16MaxKS = 5;
constexpr int kM2Bf16MaxF = 32 * kM2Bf16MaxKS;       // 160 features

__host__ __device__ constexpr int mlp2_bf16_bucket(int F)
{
    return F <= 64 ? 2 : kM2Bf16MaxKS;
}

// bytes in front of the loss slot: the image, the layer-2 partials / scratches, the dH2 rows, d loss / d score, the
// query list, the parked layer-1 tiles and layer-2 rows of three fills
__host__ __device__ constexpr size_t mlp2_bf16_static_bytes(int KS)
{
    constexpr size_t slots = kM2ParkLen / kM2Docs - 1;
    return ((size_t)kM2Docs * (32 * KS + 8) * sizeof(uint16_t) +
            ((size_t)kM2Waves * kM2Docs * kM2PS + (size_t)kM2Docs * kM2PS + kM2ParkLen + kMlpListCap + 4 +
             slots * 2 * kM2Threads * 4 + slots * 128 * 4) * sizeof(float) + 15) & ~(size_t)15;
}

inline size_t mlp2_bf16_lds_bytes(int kind, int KS)
{
    const size_t loop = mlp2_bf16_static_bytes(KS) + loss_lds_bytes(kind, kM2ParkLen, kM2Waves);
    // the epilogue stages the four dW1 tiles (64 rows of the front's staging pitch) and the fold from the start
    const size_t tail = ((size_t)64 * (32 * KS + 4) + (size_t)kMsWaves * kMsFold) * sizeof(float);
    return loop > tail ? loop : tail;
}

// The device code of this file is compiled without the packed fp32 instructions (v_pk_add_f32 / v_pk_mul_f32 /
// v_pk_fma_f32): whatever is inlined into the kernel below, the helpers of the other files included, is selected as
// plain fp32 operations.  The other kernels of the translation unit keep their code.
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// The loss slot over the whole query, as mlp_tile_kernel runs it: the symmetric pair pass, or the listwise / LambdaRank
// row (ltr_mlp_listwise.inc); d loss / d score of the query's documents -> gfin, the query's loss -> p.loss[b].  Every
// thread of the workgroup; the caller's barrier follows.
template <int KIND, int T, int Lt>
__device__ __forceinline__ void mlp2_loss_slot(const MlpParams &p, const QueryLds &q, unsigned char *qbase, int b, int nb,
                                               float *gfin, int tid)
{
    const float wq = p.grad_out ? p.grad_out[b] : 1.0f / (float)p.B;
    if constexpr (KIND == LTR_MLP_LISTNET || KIND == LTR_MLP_LISTMLE) {
        mlp_listwise_slot<KIND, T, Lt>(qbase, p.lw, nb, wq, p.loss + b, gfin);
    } else if constexpr (KIND == LTR_MLP_LAMBDARANK) {
        mlp_lambdarank_slot<T, Lt>(qbase, p.lw.k, p.sigma, nb, wq, p.loss + b, gfin);
    } else {
        float gscale;
        if (KIND == LTR_NDCG1 || KIND == LTR_NDCG2) {
            constexpr int owners = 128;
            constexpr int ms = T / owners;
            const int mlen = (nb + ms - 1) / ms;
            const int m0 = __builtin_amdgcn_readfirstlane(min(nb, (tid / owners) * mlen));
            const int m1 = __builtin_amdgcn_readfirstlane(min(nb, m0 + mlen));
            prepare_ndcg<KIND, 1, kM2Waves, true>(q, nb, owners, tid % owners, m0, m1, ms > 1);
        }
        const float total = pairwise_core_sym<KIND, kM2Waves, true>(q, nb, Lt, p.sigma, gscale);
        if (tid == 0) p.loss[b] = total;
        const float weight = wq * gscale;
        if (tid < Lt) {
            float gk = 0.f;
            if (tid < nb) {
#pragma unroll
                for (int s = 0; s < kM2Waves; ++s) gk += q.gpart[(size_t)s * Lt + tid];
            }
            gfin[tid] = gk * weight;
        }
    }
}

// p.X holds bf16 values (MlpStepCall::x_bf16); everything else of MlpParams is as mlp_tile_kernel reads it.
template <int KIND, int KS>
__global__ void __launch_bounds__(kM2Threads, kM2Wgs)
mlp_tile_bf16_kernel(MlpParams p)
{
    typedef MlpFrontBf16<KS> Front;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int T = kM2Threads, Lt = kM2ParkLen;
    constexpr int IP = Front::IP, NC = Front::NC;
    constexpr bool kListwise = KIND == LTR_MLP_LISTNET || KIND == LTR_MLP_LISTMLE;   // sy holds (label, score)
    constexpr bool kLambdaRank = KIND == LTR_MLP_LAMBDARANK;                         // (score, label), its own slot
    constexpr int kSlots = kM2ParkLen / kM2Docs - 1;
    constexpr int KP = (kM2Docs * Front::FU + T - 1) / T;          // 16-byte units of a fill per thread

    MlpLane ln = mlp_lane();                       // (not const: see the top of the query loop)
    const int w = ln.w;
    const int L = p.L, F = p.F;
    const int C = F >> 3;                          // 16-byte units per feature row

    uint16_t *img = reinterpret_cast<uint16_t *>(smem);            // [32][IP]   feature rows of the fill, bf16
    float *part = reinterpret_cast<float *>(img + (size_t)kM2Docs * IP);       // [4][32][20] layer-2 partials, later
    float *scr = part + (size_t)w * kM2Docs * kM2PS;               //            this wave's transposition scratch
    float *dH2s = part + (size_t)kM2Waves * kM2Docs * kM2PS;       // [32][20]
    float *gfin = dH2s + (size_t)kM2Docs * kM2PS;                  // [128]
    int *qlist = reinterpret_cast<int *>(gfin + Lt);               // [kMlpListCap + 4]
    mlp_f4 *h1park = reinterpret_cast<mlp_f4 *>(qlist + kMlpListCap + 4);      // [3][2][256]
    mlp_f4 *h2park = h1park + kSlots * 2 * T;                                  // [3][128]
    unsigned char *qbase = smem + mlp2_bf16_static_bytes(KS);
    const QueryLds q = carve_query_lds<KIND>(qbase, Lt, kM2Waves);

    const mlp_f4 zero4 = {0.f, 0.f, 0.f, 0.f};

    // the network as the helpers of ltr_mlp_stream.inc read it
    MlpStreamParams sp;
    sp.W1 = p.W1; sp.b1 = p.b1; sp.W2 = p.W2; sp.b2 = p.b2; sp.W3 = p.W3; sp.b3 = p.b3;
    sp.F = F; sp.H1 = p.H1; sp.H2 = p.H2;

    // ---- accumulators that live across queries (tiles disjoint between the waves) ----
    mlp_f4 acc[NC];                  // dW1[j1 = 16w+4g+i][f = 16c + c16]
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = zero4;
    MlpSmallSums sums = mlp_small_sums_zero();

    // ---- which queries this workgroup takes (the scratch borrows the partials) ----
    const int G = (int)gridDim.x;
    const int nq = mlp_schedule<T, Lt>(p.n, p.B, L, qlist, reinterpret_cast<unsigned *>(part), false);
    const int nqueries = nq < 0 ? (p.B - (int)blockIdx.x + G - 1) / G : nq;
    auto query_at = [&](int qi) { return nq < 0 ? (int)blockIdx.x + qi * G : qlist[qi]; };
    // the feature columns F .. IP - 1 of the image are never written by a fill: zero them once
    // (layer 1 multiplies them by zero weights, the dW1 columns they produce are not stored)
    for (int i = ln.tid; i < kM2Docs * (IP - 8 * C); i += T) {
        const int r = i / (IP - 8 * C), cc = i - r * (IP - 8 * C);
        img[r * IP + 8 * C + cc] = 0;
    }

    // ---- the fill in flight: 32 feature rows = 32 C units of 16 bytes, unit tid + 256 k in P[k]; its place in the
    //      image: row u / C, 8 values from column 8 (u % C) (-1: past the 32 rows, nothing is stored) ----
    int ioff[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        const int u = ln.tid + k * T, r = u / C;
        ioff[k] = r < kM2Docs ? r * IP + 8 * (u - r * C) : -1;
    }
    ltr_u32x4 P[KP];
    auto issue_fill = [&](int bq, int fill, int nbq) {
        const int rows = min(max(nbq - kM2Docs * fill, 0), kM2Docs);
        const uintptr_t xaddr = reinterpret_cast<uintptr_t>(reinterpret_cast<const uint16_t *>(p.X) +
                                                            ((size_t)bq * L + kM2Docs * fill) * (size_t)F);
        const unsigned xlo = __builtin_amdgcn_readfirstlane((unsigned)xaddr);
        const unsigned xhi = __builtin_amdgcn_readfirstlane((unsigned)(xaddr >> 32));
        // (bytes of the rows the query has in this fill: a unit past them returns 0 and touches no memory)
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
            reinterpret_cast<void *>(((uintptr_t)xhi << 32) | xlo), 0,
            __builtin_amdgcn_readfirstlane(rows * F * 2), 0x00020000);
#pragma unroll
        for (int k = 0; k < KP; ++k) P[k] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (ln.tid + k * T) * 16, 0, 0);
    };
    // registers -> image, all 32 rows: the rows past n arrive as zeros, and the dW1 step reads every row
    auto fill_image = [&]() {
#pragma unroll
        for (int k = 0; k < KP; ++k)
            if (ioff[k] >= 0) *reinterpret_cast<ltr_u32x4 *>(img + ioff[k]) = P[k];
    };

    typename Front::w1frag w1r[KS];
    MlpSmallFrags fr;

    // ---- forward over the fill in the image: layer-1 tile -> h1 (kept), layer-2 partial -> LDS ----
    auto fwd_tile = [&](auto ns_c, mlp_f4 (&h1)[2]) {
        constexpr int NS = decltype(ns_c)::value;
#pragma unroll
        for (int u = 0; u < NS; ++u) h1[u] = fr.b1v;
        Front::template layer1<NS>(h1, w1r, img, 0, ln);
#pragma unroll
        for (int u = 0; u < NS; ++u) mlp_layer2_partial(fr, h1[u], scr + (16 * u + ln.c16) * kM2PS + 4 * ln.g);
        if (NS == 1) h1[1] = zero4;
    };
    // tile wave, backward: dW2, dH1 (-> scratch) and dW1 contributions of the fill in the image
    auto bwd_tile = [&](auto ns_c, const mlp_f4 (&h1)[2]) {
        constexpr int NS = decltype(ns_c)::value;
        mlp_dw2_tile<NS>(sums, h1, scr, dH2s, 0, ln);
        mlp_dh1_tile<NS>(fr, sums, h1, dH2s, 0, ln, [&](int u, const mlp_f4 &d1) {
            *reinterpret_cast<mlp_f4 *>(scr + (16 * u + ln.c16) * kM2PS + 4 * ln.g) = d1;
        });
        Front::template dw1<NS>(acc, img, scr, 0, ln);
    };

    float ynext = 0.f;                             // label of document `tid` of the next query
    int nb_next = 0;
    if (nqueries > 0) {
        const int b0 = query_at(0);
        nb_next = clamp_n(p.n[b0], L);
        if (ln.tid < L) ynext = load_label(p.rel, p.rel_dtype, (size_t)b0 * L + ln.tid);
        issue_fill(b0, 0, nb_next);
    }
    // this wave's weight fragments, straight from global memory into registers, behind the first fill (the scheduling
    // pass and its n[] loads are the critical path of the prologue); W1 is rounded to bf16 here, once
    Front::load_w1(w1r, sp, ln);
    fr = mlp_small_frags(sp, ln);

    for (int qi = 0; qi < nqueries; ++qi) {
        // (ltr_mlp2.inc: opaque lane indices keep the address arithmetic of the chains inside this loop, where the row
        // slots bring lane-derived addresses of their own)
        if constexpr (kListwise || kLambdaRank) asm volatile("" : "+v"(ln.c16), "+v"(ln.g), "+v"(ln.tid));
        const int tid = ln.tid;
        const int b = __builtin_amdgcn_readfirstlane(query_at(qi));
        const int nb = __builtin_amdgcn_readfirstlane(nb_next);
        const size_t row0 = (size_t)b * L;
        const int R = max((nb + kM2Docs - 1) / kM2Docs, 1);     // fills of this query (an empty one: 1, no rows)
        const bool more = qi + 1 < nqueries;
        const int bn = __builtin_amdgcn_readfirstlane(more ? query_at(qi + 1) : b);
        if (more) nb_next = __builtin_amdgcn_readfirstlane(clamp_n(p.n[bn], L));

        if (tid < nb) { if (kListwise) q.sy[tid].x = ynext; else q.sy[tid].y = ynext; }
        if (KIND == LTR_NDCG1 || KIND == LTR_NDCG2)
            for (int m = tid; m < 2 * Lt; m += T) q.rank_s[m] = 0;
        // the next query's label goes out ahead of the fills in the in-order vmcnt queue
        if (more && tid < L) ynext = load_label(p.rel, p.rel_dtype, (size_t)bn * L + tid);

        // ---- forward, fill by fill ----
        mlp_f4 h1[2], h2 = zero4;
        for (int h = 0; h < R; ++h) {
            const int nsub = min((nb - kM2Docs * h + 15) >> 4, 2);
            fill_image();                          // (waits for the fill in P)
            // next fill: the one after this, else the one before for its backward pass, else the next query's first
            // (a fill is requested on EVERY path -- with nothing left, through an empty descriptor -- or the registers
            // of P are live around the whole loop body on one path: ltr_mlp2.inc)
            if (h + 1 < R) issue_fill(b, h + 1, nb);
            else if (R > 1) issue_fill(b, R - 2, nb);
            else if (more) issue_fill(bn, 0, nb_next);
            else issue_fill(b, 0, 0);
            lds_barrier();                         // image filled
            h1[0] = zero4; h1[1] = zero4;
            if (nsub == 2) fwd_tile(m2_ns<2>{}, h1);
            else if (nsub == 1) fwd_tile(m2_ns<1>{}, h1);
            lds_barrier();                         // layer-2 partials
            if (w < nsub) {                        // owner wave: layers 2 and 3 of its 16 documents
                const int doc = 16 * w + ln.c16, k = kM2Docs * h + doc;
                const float s = mlp_owner_fwd(fr, part, doc, ln.g, h2);
                if (ln.g == 0 && k < nb) {
                    if (kListwise) q.sy[k].y = s; else q.sy[k].x = s;
                    if (p.scores_out) p.scores_out[row0 + k] = s;
                }
            }
            if (h + 1 < R) {                       // not the last fill: park (a fill before the last is full)
                h1park[(2 * h) * T + tid] = h1[0];
                h1park[(2 * h + 1) * T + tid] = h1[1];
                if (w < 2) h2park[h * 128 + tid] = h2;
            }
            // (the image is rewritten only after the barrier behind the layer-1 reads; the partials only after the next
            // one, which this wave reaches past its owner reads)
        }
        lds_barrier();

        mlp2_loss_slot<KIND, T, Lt>(p, q, qbase, b, nb, gfin, tid);
        lds_barrier();

        // ---- backward, last fill (still in the image) first ----
        for (int h = R - 1; h >= 0; --h) {
            const int nsub = min((nb - kM2Docs * h + 15) >> 4, 2);
            if (h < R - 1) {
                fill_image();                      // (every wave is past the barrier behind the last image read)
                if (h > 0) issue_fill(b, h - 1, nb);
                else if (more) issue_fill(bn, 0, nb_next);
                else issue_fill(b, 0, 0);
                h1[0] = h1park[(2 * h) * T + tid];
                h1[1] = h1park[(2 * h + 1) * T + tid];
                if (w < 2) h2 = h2park[h * 128 + tid];
            }
            if (w < nsub) {
                const int doc = 16 * w + ln.c16;
                mlp_owner_bwd(fr, sums, h2, gfin[kM2Docs * h + doc], dH2s, doc, ln.g);
            }
            lds_barrier();                         // refill, dH2 rows
            if (nsub == 2) bwd_tile(m2_ns<2>{}, h1);
            else if (nsub == 1) bwd_tile(m2_ns<1>{}, h1);
            lds_barrier();                         // image, dH2 rows (and, at the end, sy / gfin) free
        }
    }

    // ---- this workgroup's partial vector [dW1 | db1 | dW2 | db2 | dW3 | db3] (the epilogue of mlp_stream_body) ----
    float *dst = p.part + (size_t)blockIdx.x * p.pitch;
    float *lds = reinterpret_cast<float *>(smem);
    __syncthreads();                               // (a workgroup without a query: the zeroing above is behind every wave)
    mlp_store_dw1<NC, Front::SP>(acc, lds, dst, sp, 0, F >> 2, ln);
    mlp_store_small_sums(sums, dst, p.H1 * F, lds + (size_t)64 * Front::SP, sp, ln);
}

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

// ---- host side: what mlp_step_launch (ltr_mlp_step.inc) needs of this file ----
// the plan rule behind the width checks: rows of at most 160 features, lists up to 128 documents, the loss slot next to
// the network's LDS
inline bool mlp_step_bf16_fits(int kind, int L, int F)
{
    return F <= kM2Bf16MaxF && L <= kM2ParkLen && mlp2_bf16_lds_bytes(kind, mlp2_bf16_bucket(F)) <= kLdsBudget / kM2Wgs;
}

template <int KIND, int KS>
int launch_mlp2_bf16_ks(const MlpParams &p, int grid, hipStream_t stream)
{
    const size_t lds = mlp2_bf16_lds_bytes(KIND, KS);
    LTR_ENSURE_LDS((mlp_tile_bf16_kernel<KIND, KS>), lds);
    hipLaunchKernelGGL((mlp_tile_bf16_kernel<KIND, KS>), dim3((unsigned)grid), dim3(kM2Threads), lds, stream, p);
    return (int)hipGetLastError();
}

int launch_mlp2_bf16(int slot, const MlpParams &p, int grid, hipStream_t stream)
{
    return with_mlp_slot(slot, [&](auto K) {
        if (mlp2_bf16_bucket(p.F) == 2) return launch_mlp2_bf16_ks<K, 2>(p, grid, stream);
        return launch_mlp2_bf16_ks<K, kM2Bf16MaxKS>(p, grid, stream);
    });
}
