// ltr_mlp2.inc -- the training step of the fused ReLU-MLP scorer (F -> H1 -> H2 -> 1) + pairwise
// loss + backward, second layout: FOUR-wave workgroups, TWO per CU, every wave owns one 16-row
// tile of the first hidden layer.  Included behind ltr_mlp.inc (whose kernel keeps the evaluation half
// and the widest feature bucket).  Same contract: the reference guide's training step
//     loss_fn(model(xs), ys, n).mean().backward()          docs/source/getting-started.rst:40-101
// with `model` = Linear(F,50) / ReLU / Linear(50,10) / ReLU / Linear(10,1), losses of
// loss/pairwise_additive.py:51-163 and loss/pairwise_lambda.py:50-241 (SURVEY.md section 8 f-2).
//
// Why a second layout.  ltr_mlp.inc runs one 8-wave workgroup per CU with every phase of a query
// behind a workgroup barrier: 37 % of its time has no MFMA in flight (pair pass, staging, folds)
// and the dW1 GEMM crosses five barrier rounds per query (DESIGN.md section 10).  Here a query
// belongs to a 4-wave workgroup -- one wave per SIMD -- and a CU hosts two of them (LDS 40 KB,
// <= 256 registers per wave), out of phase: while one runs its pair pass (VALU, barriers), the
// other one's MFMA stream has the matrix pipes.
//
// Mapping.  Documents are processed in fills of 32 rows (a query of n <= 128 documents has up to
// four).  A fill's feature rows are written ONCE, in their natural layout, into an LDS image
// [32][16*NT + 4]; every GEMM operand that involves X is a read of that image:
//     layer 1    H1^T[tile w] = relu(W1[tile w] . X^T + b1)    A = W1 rows of tile w: REGISTERS, loaded
//                                                              once per workgroup (no LDS copy of W1)
//                                                              B = image rows (b128, document on lane&15)
//     layer 2    H2^T = relu(W2 . H1^T + b2)  contracts over the hidden-1 rows, i.e. over the waves:
//                every wave multiplies its tile (D fragment of layer 1 = B operand, no LDS), the
//                four partial tiles meet in LDS and wave u finishes documents 16u .. 16u+15
//     layer 3    s = w3 . H2^T + b3                            4 FMAs + two cross-row adds (owner wave)
//     (barrier)  symmetric pair pass over the query's scores -> d loss / d s        (barrier)
//     dH2^T      = w3 (x) ds . [H2 > 0]                        owner wave, registers -> LDS [32][20]
//     dH1^T[tile w] = W2^T[tile w] . dH2^T . [H1 > 0]          A = W2 columns of tile w: registers
//     dW2[:, tile w] += dH2^T . H1                             contracts over documents: both operands
//     dW1[tile w]    += dH1^T . X                              through transposed LDS reads -- dH1 / H1
//                                                              via a wave-private 32 x 20 scratch, X
//                                                              straight from the image (column reads)
// The dW1 / dW2 tiles of the four waves are disjoint and live in registers across all queries of the
// workgroup (36 + 4 registers per lane at F = 136); nothing is folded until the end of the kernel,
// and no barrier separates the GEMMs of the backward pass.  The next fill is fetched into registers
// (buffer loads sized to the rows the query really has: rows past n return 0) while the current one
// is computed.  A query of R > 1 fills runs forward over fills 0 .. R-1 (the layer-1 tiles and
// layer-2 rows of all but the last are parked in LDS, lane-linear: every lane reads back its own
// 16 bytes), then the pair pass, then backward over fill R-1 (still in the image, its tiles still
// in registers) down to 0, each of which is fetched a second time (L2 / Infinity Cache: the fetch
// is in flight during the GEMMs of the fill before).
// Deterministic: fixed assignment (mlp_schedule), fixed summation orders, no atomics.
#pragma once

constexpr int kM2Threads = 256;
constexpr int kM2Waves = 4;
constexpr int kM2Docs = 32;          // rows per fill (two 16-document subtiles)
constexpr int kM2Wgs = 2;                  // workgroups per CU the launch bounds and the grid are sized for
constexpr int kM2MaxLen = 256;       // longest list: 8 fills (lists over 128: no parking, see below)
constexpr int kM2ParkLen = 128;      // lists up to here park the tiles of their first fills in LDS
constexpr int kM2PS = 20;            // row pitch (floats) of the partial / scratch / dH2 images
constexpr int kM2MaxNT = 9;          // feature buckets this layout takes (F <= 144)

// LT = list-length class of the instantiation: 128 (tiles of the first fills parked) or 256
__host__ __device__ inline size_t mlp2_static_floats(int NT, int LT)
{
    const size_t slots = LT <= kM2ParkLen ? (size_t)(kM2ParkLen / kM2Docs - 1) : 0;
    return (size_t)kM2Docs * (16 * NT + 4) + (size_t)kM2Waves * kM2Docs * kM2PS + (size_t)kM2Docs * kM2PS +
           LT + kMlpListCap + 4 +
           slots * 2 * kM2Threads * 4 +                         // parked layer-1 tiles
           slots * 128 * 4 +                                    // parked layer-2 rows (owner waves 0, 1)
           (slots == 0 ? 2 * 128 : 0);                          // (room for the fold of the epilogue)
}

__host__ __device__ inline size_t mlp2_lds_bytes(int kind, int NT, int LT)
{
    size_t bytes = ((mlp2_static_floats(NT, LT) * 4 + 15) & ~(size_t)15) + loss_lds_bytes(kind, LT, kM2Waves);
    // the epilogue stages the four dW1 tiles (64 rows of the image pitch) from the start of the segment
    const size_t tiles = (size_t)64 * (16 * NT + 4) * 4 + 1024;
    return bytes > tiles ? bytes : tiles;
}

// -DLTR_MLP_TRACE: per-phase cycle sums, kept in (scalar) registers and written once at the end of
// the kernel -- a stamp that adds to global memory waits for every load in flight, i.e. for the
// prefetched fill, and would show a stall the production kernel does not have.
#ifdef LTR_MLP_TRACE
#define M2_STAMP(slot) do { const long long now_ = (long long)__builtin_readcyclecounter(); \
    tr_[slot] += now_ - last_; last_ = now_; } while (0)
#else
#define M2_STAMP(slot) do { } while (0)
#endif

template <int NS>
using m2_ns = std::integral_constant<int, NS>;

// LT: 128 or 256 (list-length class); FWD: scores only (evaluation) -- no labels, no pair pass, no
// backward, plain round-robin assignment.
// PROBE (bench.py `extra.mlp_scorer_fused.launch_ceiling`, ltr_debug_mlp_probe_f32): the launch geometry of the
// training step and nothing else -- the same grid and workgroups, the same fills requested, written to the image and
// read back, the same barriers and the same MFMA streams (80 forward + 88 backward per 32 rows and wave), the same
// assignment of queries to workgroups (the scheduling pass runs), with no labels, owner-wave work (layers 2-3 per document), parking, pair pass or partial vector: every
// wave stores one dword.  What this takes is what the fills + MFMA chains of ONE workgroup per two SIMD-slots can do
// at this batch size; the fused step is judged against it.  The numbers it computes mean nothing.
template <int KIND, int NT, int CT, int LT, bool FWD = false, bool PROBE = false>
__global__ void __launch_bounds__(kM2Threads, kM2Wgs)
mlp_tile_kernel(MlpParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int tid = threadIdx.x;                         // (not const, like c16 and g: see the top of the query loop)
    constexpr int T = kM2Threads;
#ifdef LTR_MLP_TRACE
    long long last_ = (long long)__builtin_readcyclecounter();
    long long tr_[15] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#endif
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    int c16 = lane & 15;
    int g = lane >> 4;
    const int L = p.L, F = p.F, H1 = p.H1, H2 = p.H2;
    const int C = CT > 0 ? CT : (F >> 2);           // float4 units per feature row
    constexpr int IP = 16 * NT + 4;                 // image pitch (floats): odd number of 16-byte units
    constexpr int Lt = LT;
    constexpr bool kListwise = KIND == LTR_MLP_LISTNET || KIND == LTR_MLP_LISTMLE;   // sy holds (label, score)
    constexpr bool kLambdaRank = KIND == LTR_MLP_LAMBDARANK;                         // (score, label), its own slot
    constexpr bool kPark = LT <= kM2ParkLen;        // else: forward again in the backward pass
    constexpr int kSlots = kPark ? kM2ParkLen / kM2Docs - 1 : 0;
    constexpr int KP = (kM2Docs * 4 * NT + T - 1) / T;     // float4 units of a fill per thread

    float *img = reinterpret_cast<float *>(smem);                  // [32][IP]   feature rows of the fill
    float *part = img + (size_t)kM2Docs * IP;                      // [4][32][20] layer-2 partials, later
    float *scr = part + (size_t)w * kM2Docs * kM2PS;               //            this wave's transposition scratch
    float *dH2s = part + (size_t)kM2Waves * kM2Docs * kM2PS;       // [32][20]
    float *gfin = dH2s + (size_t)kM2Docs * kM2PS;                  // [LT]
    int *qlist = reinterpret_cast<int *>(gfin + LT);               // [kMlpListCap + 4]
    mlp_f4 *h1park = reinterpret_cast<mlp_f4 *>(qlist + kMlpListCap + 4);      // [3][2][256]
    mlp_f4 *h2park = h1park + kSlots * 2 * kM2Threads;                         // [3][128]
    const size_t qoff = (mlp2_static_floats(NT, LT) * 4 + 15) & ~(size_t)15;
    const QueryLds q = carve_query_lds<KIND>(smem + qoff, Lt, kM2Waves);

    const mlp_f4 zero4 = {0.f, 0.f, 0.f, 0.f};

    // ---- this wave's weight fragments, straight from global memory into registers (requested
    // behind the first fill, below: the scheduling pass comes first, its n[] loads are the critical
    // path of the prologue) ----
    const int j1A = 16 * w + c16;                   // hidden-1 row as an A-operand row (lane & 15)
    mlp_f4 w1r[NT];                                 // W1[j1A][16c + 4g .. +3]
    mlp_f4 b1v, w2a, w2t, b2v, w3v;
    float b3 = 0.f;
    auto load_fragments = [&]() {
#pragma unroll
        for (int c = 0; c < NT; ++c) {
            const int f0 = 16 * c + 4 * g;
            const bool ok = j1A < H1 && f0 < F;
            const mlp_f4 v = *reinterpret_cast<const mlp_f4 *>(p.W1 + (ok ? (size_t)j1A * F + f0 : 0));
#pragma unroll
            for (int i = 0; i < 4; ++i) w1r[c][i] = ok ? v[i] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j1D = 16 * w + 4 * g + i;         // hidden-1 row as a D-fragment row
            const int j2D = 4 * g + i;                  // hidden-2 row as a D-fragment row
            const bool ok1 = j1D < H1, ok2 = j2D < H2;
            const float vb1 = p.b1[ok1 ? j1D : 0];
            b1v[i] = ok1 ? vb1 : 0.f;
            const bool oka = c16 < H2 && ok1;           // layer 2:  A[row j2 = c16][k <-> j1D]
            const float va = p.W2[oka ? (size_t)c16 * H1 + j1D : 0];
            w2a[i] = oka ? va : 0.f;
            const bool okt = ok2 && j1A < H1;           // dH1:      A[row j1A][k <-> j2D]
            const float vt = p.W2[okt ? (size_t)j2D * H1 + j1A : 0];
            w2t[i] = okt ? vt : 0.f;
            const float vb2 = p.b2[ok2 ? j2D : 0], v3 = p.W3[ok2 ? j2D : 0];
            b2v[i] = ok2 ? vb2 : 0.f;
            w3v[i] = ok2 ? v3 : 0.f;
        }
        b3 = p.b3[0];
    };

    // ---- accumulators that live across queries (tiles disjoint between the waves) ----
    mlp_f4 acc[NT];                  // dW1[j1 = 16w+4g+i][f = 16c + c16]
#pragma unroll
    for (int c = 0; c < NT; ++c) acc[c] = zero4;
    mlp_f4 accW2 = zero4;            // dW2[j2 = 4g+i][j1 = 16w + c16]
    mlp_f4 accB1 = zero4;            // db1[j1 = 16w+4g+i], partial over this lane's documents
    mlp_f4 accB2 = zero4, accW3 = zero4;     // db2 / dW3 [j2 = 4g+i], documents this wave finished
    float accB3 = 0.f;

    // ---- which queries this workgroup takes (the scratch borrows the image) ----
    const int G = (int)gridDim.x;
    const int nq = mlp_schedule<T, LT>(p.n, p.B, L, qlist, reinterpret_cast<unsigned *>(img), FWD);
    const int nqueries = nq < 0 ? (p.B - (int)blockIdx.x + G - 1) / G : nq;
    M2_STAMP(9);                                   // scheduling
    auto query_at = [&](int qi) { return nq < 0 ? (int)blockIdx.x + qi * G : qlist[qi]; };
    // the feature columns F .. 16*NT+3 of the image are never written by a fill: zero them once
    // (layer 1 multiplies them by zero weights, the dW1 columns they produce are not stored)
    for (int i = tid; i < kM2Docs * (IP - 4 * C); i += T) {
        const int r = i / (IP - 4 * C), cc = i - r * (IP - 4 * C);
        img[r * IP + 4 * C + cc] = 0.f;
    }
    M2_STAMP(0);                                  // fragments requested, scheduling done

    // ---- the fill in flight: 32 feature rows = 32*C float4 units, unit tid + 256k in P[k] ----
    mlp_f4 P[KP];
    auto issue_fill = [&](int bq, int fill, int nbq) {
        const int rows = min(max(nbq - kM2Docs * fill, 0), kM2Docs);
        const uintptr_t xaddr = reinterpret_cast<uintptr_t>(p.X + ((size_t)bq * L + kM2Docs * fill) * (size_t)F);
        const unsigned xlo = __builtin_amdgcn_readfirstlane((unsigned)xaddr);
        const unsigned xhi = __builtin_amdgcn_readfirstlane((unsigned)(xaddr >> 32));
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
            reinterpret_cast<void *>(((uintptr_t)xhi << 32) | xlo), 0,
            __builtin_amdgcn_readfirstlane(rows * F * 4), 0x00020000);
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const ltr_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (tid + k * T) * 16, 0, 0);
            P[k][0] = __uint_as_float(v.x); P[k][1] = __uint_as_float(v.y);
            P[k][2] = __uint_as_float(v.z); P[k][3] = __uint_as_float(v.w);
        }
    };
    // registers -> image; only the rows of the subtiles in use are written (rows of the last
    // subtile past n arrive as zeros)
    auto fill_image = [&](int nsub) {
        const int rlim = 16 * nsub;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const int u = tid + k * T;
            const int r = u / C, f4 = u - r * C;
            if (r < rlim) *reinterpret_cast<mlp_f4 *>(img + r * IP + 4 * f4) = P[k];
        }
    };

    // ---- forward over the fill in the image: layer-1 tile -> h1 (kept), layer-2 partial -> LDS ----
    auto fwd_tile = [&](auto ns_c, mlp_f4 (&h1)[2]) {
        constexpr int NS = decltype(ns_c)::value;
#pragma unroll
        for (int u = 0; u < NS; ++u) h1[u] = b1v;
        const float *bsrc = img + c16 * IP + 4 * g;
#pragma unroll
        for (int c = 0; c < NT; ++c) {
            mlp_f4 xb[NS];
#pragma unroll
            for (int u = 0; u < NS; ++u) xb[u] = *reinterpret_cast<const mlp_f4 *>(bsrc + 16 * u * IP + 16 * c);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int u = 0; u < NS; ++u) h1[u] = mfma16(w1r[c][i], xb[u][i], h1[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < NS; ++u) {
#pragma unroll
            for (int i = 0; i < 4; ++i) h1[u][i] = fmaxf(h1[u][i], 0.f);
            mlp_f4 hp = zero4;
#pragma unroll
            for (int i = 0; i < 4; ++i) hp = mfma16(w2a[i], h1[u][i], hp);
            *reinterpret_cast<mlp_f4 *>(scr + (16 * u + c16) * kM2PS + 4 * g) = hp;
        }
        if (NS == 1) h1[1] = zero4;
    };
    // owner wave: sum the four partial tiles of its documents, layers 2 (bias, relu) and 3
    auto fwd_owner = [&](int fill, int nb, size_t row0, mlp_f4 &h2, bool publish) {
        const int doc = 16 * w + c16;
        h2 = b2v;
#pragma unroll
        for (int t = 0; t < kM2Waves; ++t) {
            const mlp_f4 v = *reinterpret_cast<const mlp_f4 *>(part + ((size_t)t * kM2Docs + doc) * kM2PS + 4 * g);
#pragma unroll
            for (int i = 0; i < 4; ++i) h2[i] += v[i];
        }
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            h2[i] = fmaxf(h2[i], 0.f);
            s = __builtin_fmaf(w3v[i], h2[i], s);
        }
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        s += b3;
        const int k = kM2Docs * fill + doc;
        if (publish && g == 0 && k < nb) {
            if (!FWD) { if (kListwise) q.sy[k].y = s; else q.sy[k].x = s; }
#ifndef LTR_MLP_TRACE
            if (p.scores_out) p.scores_out[row0 + k] = s;
#endif
        }
    };
    // owner wave, backward through layers 3 and 2 for its documents: dH2 rows -> LDS
    auto bwd_owner = [&](int fill, const mlp_f4 &h2) {
        const int doc = 16 * w + c16;
        const float ds = gfin[kM2Docs * fill + doc];
        mlp_f4 dh2;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            accW3[i] = __builtin_fmaf(ds, h2[i], accW3[i]);
            dh2[i] = (h2[i] > 0.f) ? ds * w3v[i] : 0.f;
            accB2[i] += dh2[i];
        }
        if (g == 0) accB3 += ds;
        *reinterpret_cast<mlp_f4 *>(dH2s + doc * kM2PS + 4 * g) = dh2;
    };
    // tile wave, backward: dH1 tile, dW2 and dW1 contributions of the fill in the image
    auto bwd_tile = [&](auto ns_c, const mlp_f4 (&h1)[2]) {
        constexpr int NS = decltype(ns_c)::value;
        const float *tsrc = scr + g * kM2PS + c16;              // transposed reads: [4s + g][c16]
        const float *dsrc = dH2s + g * kM2PS + c16;
        // ---- dW2[:, tile] += dH2^T . H1: H1 through the scratch (document-major -> k-major) ----
#pragma unroll
        for (int u = 0; u < NS; ++u)
            *reinterpret_cast<mlp_f4 *>(scr + (16 * u + c16) * kM2PS + 4 * g) = h1[u];
        {
            mlp_f4 o = zero4;
#pragma unroll
            for (int s = 0; s < 4 * NS; ++s) {
                const float a = dsrc[4 * s * kM2PS], bb = tsrc[4 * s * kM2PS];
                if (s & 1) o = mfma16(a, bb, o); else accW2 = mfma16(a, bb, accW2);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) accW2[i] += o[i];
        }
        // ---- dH1^T tile = (W2^T . dH2^T) . [H1 > 0] -> scratch ----
#pragma unroll
        for (int u = 0; u < NS; ++u) {
            const mlp_f4 d2 = *reinterpret_cast<const mlp_f4 *>(dH2s + (16 * u + c16) * kM2PS + 4 * g);
            mlp_f4 d1 = zero4;
#pragma unroll
            for (int i = 0; i < 4; ++i) d1 = mfma16(w2t[i], d2[i], d1);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                d1[i] = (h1[u][i] > 0.f) ? d1[i] : 0.f;
                accB1[i] += d1[i];
            }
            *reinterpret_cast<mlp_f4 *>(scr + (16 * u + c16) * kM2PS + 4 * g) = d1;
        }
        float a1[4 * NS];
#pragma unroll
        for (int s = 0; s < 4 * NS; ++s) a1[s] = tsrc[4 * s * kM2PS];
        // ---- dW1[tile] += dH1^T . X: B = image columns; three feature chunks in flight ----
        const float *xsrc = img + g * IP + c16;
        constexpr int CG = 3;
#pragma unroll
        for (int c0 = 0; c0 < NT; c0 += CG) {
#pragma unroll
            for (int s = 0; s < 4 * NS; ++s) {
#pragma unroll
                for (int cc = 0; cc < CG; ++cc) {
                    if (c0 + cc < NT)
                        acc[c0 + cc] = mfma16(a1[s], xsrc[4 * s * IP + 16 * (c0 + cc)], acc[c0 + cc]);
                }
            }
        }
    };

    float ynext = 0.f;                             // label of document `tid` of the next query
    int nb_next = 0;
    if (nqueries > 0) {
        const int b0 = query_at(0);
        nb_next = clamp_n(p.n[b0], L);
        if (!FWD && !PROBE && tid < L) ynext = load_label(p.rel, p.rel_dtype, (size_t)b0 * L + tid);
        issue_fill(b0, 0, nb_next);
    }
    load_fragments();
    M2_STAMP(8);                                   // first fill and weight fragments requested

    for (int qi = 0; qi < nqueries; ++qi) {
        // The listwise rows bring their own lane-derived addresses; with those of the chains below hoisted out of this
        // loop as well, the register allocator spills (ListNet at F = 136: 6 VGPRs, ListMLE: 28).  Opaque lane indices
        // keep the address arithmetic inside the loop: a few VALU instructions per query, no spill (the row functions'
        // own reads of the thread index: ltr_mlp.hip).
        if constexpr (kListwise || kLambdaRank) asm volatile("" : "+v"(c16), "+v"(g), "+v"(tid));
        const int b = __builtin_amdgcn_readfirstlane(query_at(qi));
        const int nb = __builtin_amdgcn_readfirstlane(nb_next);
        const size_t row0 = (size_t)b * L;
        const int R = max((nb + kM2Docs - 1) / kM2Docs, 1);     // fills of this query (an empty one: 1, no rows)
        const bool more = qi + 1 < nqueries;
        const int bn = __builtin_amdgcn_readfirstlane(more ? query_at(qi + 1) : b);
        if (more) nb_next = __builtin_amdgcn_readfirstlane(clamp_n(p.n[bn], L));

        if (PROBE) {
        } else if (!FWD) {
            if (tid < nb) { if (kListwise) q.sy[tid].x = ynext; else q.sy[tid].y = ynext; }
            if (KIND == LTR_NDCG1 || KIND == LTR_NDCG2)
                for (int m = tid; m < 2 * Lt; m += T) q.rank_s[m] = 0;
            // the next query's label goes out ahead of the fills in the in-order vmcnt queue
            if (more && tid < L) ynext = load_label(p.rel, p.rel_dtype, (size_t)bn * L + tid);
        } else {
#ifndef LTR_MLP_TRACE
            for (int k = nb + tid; k < L; k += T) p.scores_out[row0 + k] = 0.f;     // padded documents
#endif
        }

        // ---- forward, fill by fill ----
        mlp_f4 h1[2], h2 = zero4;
        for (int h = 0; h < R; ++h) {
            const int nsub = min((nb - kM2Docs * h + 15) >> 4, 2);
            M2_STAMP(10);                          // (loop top: owner work of the fill before, parking)
            fill_image(nsub);                      // (waits for the fill in P)
            M2_STAMP(11);                          // P arrived, image written
            // next fill: the one after this, else (training) the one before for its backward pass,
            // else the next query's first
            // (a fill is requested on EVERY path -- with nothing left, through an empty descriptor: the loads
            // return 0 without touching memory -- or the registers of P keep their old contents on one path and
            // are live around the whole loop body for the register allocator: ltr_parts.inc, round 4)
            if (h + 1 < R) issue_fill(b, h + 1, nb);
            else if (!FWD && R > 1) issue_fill(b, R - 2, nb);
            else if (more) issue_fill(bn, 0, nb_next);
            else issue_fill(b, 0, 0);
            lds_barrier();
            M2_STAMP(1);                          // image filled
            h1[0] = zero4; h1[1] = zero4;
            if (nsub == 2) fwd_tile(m2_ns<2>{}, h1);
            else if (nsub == 1) fwd_tile(m2_ns<1>{}, h1);
            lds_barrier();
            M2_STAMP(2);                          // layer-1 tile, layer-2 partials
            if (!PROBE && w < nsub) fwd_owner(h, nb, row0, h2, true);
            M2_STAMP(13);                         // owner rows
            if (!FWD && !PROBE && kPark && h + 1 < R) {      // not the last fill: park (a fill before the last is full)
                h1park[(2 * h) * T + tid] = h1[0];
                h1park[(2 * h + 1) * T + tid] = h1[1];
                if (w < 2) h2park[h * 128 + tid] = h2;
            }
            M2_STAMP(14);                         // parking
            // (the image is rewritten only after the barrier behind the layer-1 reads; the
            // partials only after the next one, which this wave reaches past its owner reads)
        }
        lds_barrier();
        M2_STAMP(3);                              // layers 2, 3 (owner), parking
        if (FWD) continue;

        if (PROBE) {
            // (no pair pass: the backward chain below runs on whatever the regions hold)
            for (int h = R - 1; h >= 0; --h) {
                const int nsub = min((nb - kM2Docs * h + 15) >> 4, 2);
                if (h < R - 1) {
                    fill_image(nsub);
                    if (h > 0) issue_fill(b, h - 1, nb);
                    else if (more) issue_fill(bn, 0, nb_next);
                    else issue_fill(b, 0, 0);
                }
                lds_barrier();
                if (nsub == 2) bwd_tile(m2_ns<2>{}, h1);
                else if (nsub == 1) bwd_tile(m2_ns<1>{}, h1);
                lds_barrier();
            }
            continue;
        }
        // ---- the loss slot over the whole query: the pair pass, or the listwise row (ltr_mlp_listwise.inc) ----
        if constexpr (kListwise) {
            mlp_listwise_slot<KIND, T, Lt>(smem + qoff, p.lw, nb, p.grad_out ? p.grad_out[b] : 1.0f / (float)p.B,
                                           p.loss + b, gfin);
        } else if constexpr (kLambdaRank) {
            mlp_lambdarank_slot<T, Lt>(smem + qoff, p.lw.k, p.sigma, nb, p.grad_out ? p.grad_out[b] : 1.0f / (float)p.B,
                                       p.loss + b, gfin);
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
            const float weight = (p.grad_out ? p.grad_out[b] : 1.0f / (float)p.B) * gscale;
            if (tid < Lt) {
                float gk = 0.f;
                if (tid < nb) {
#pragma unroll
                    for (int s = 0; s < kM2Waves; ++s) gk += q.gpart[(size_t)s * Lt + tid];
                }
                gfin[tid] = gk * weight;
            }
        }
        lds_barrier();
        M2_STAMP(4);                              // pair pass

        // ---- backward, last fill (still in the image) first ----
        for (int h = R - 1; h >= 0; --h) {
            const int nsub = min((nb - kM2Docs * h + 15) >> 4, 2);
            if (h < R - 1) {
                fill_image(nsub);                  // (every wave is past the barrier behind the last image read)
                if (h > 0) issue_fill(b, h - 1, nb);
                else if (more) issue_fill(bn, 0, nb_next);
                else issue_fill(b, 0, 0);
                if (kPark) {
                    h1[0] = h1park[(2 * h) * T + tid];
                    h1[1] = h1park[(2 * h + 1) * T + tid];
                    if (w < 2) h2 = h2park[h * 128 + tid];
                } else {
                    // lists over 128 documents: nothing was parked -- the forward pass of the fill
                    // again (layer-1 tile, layer-2 partials, owner rows; a full fill: nsub == 2)
                    lds_barrier();
                    fwd_tile(m2_ns<2>{}, h1);
                    lds_barrier();
                    if (w < nsub) fwd_owner(h, nb, row0, h2, false);
                }
            }
            if (w < nsub) bwd_owner(h, h2);
            lds_barrier();
            M2_STAMP(5);                          // refill, dH2 rows
            if (nsub == 2) bwd_tile(m2_ns<2>{}, h1);
            else if (nsub == 1) bwd_tile(m2_ns<1>{}, h1);
            lds_barrier();                         // image, dH2 rows (and, at the end, sy / gfin) free
            M2_STAMP(6);                          // backward GEMMs
        }
    }
    if (FWD) return;
    if (PROBE) {
        // (the accumulators must stay: one dword per wave)
        float t = accW2[0] + accB1[0];
#pragma unroll
        for (int c = 0; c < NT; ++c) t += (acc[c][0] + acc[c][1]) + (acc[c][2] + acc[c][3]);
        t = wave_sum(t);
        if (lane == 0) p.loss[(size_t)blockIdx.x * kM2Waves + w] = t;
        return;
    }

    // ---- this workgroup's partial vector [dW1 | db1 | dW2 | db2 | dW3 | db3] ----
    float *dst = p.part + (size_t)blockIdx.x * p.pitch;
    const int oB1 = H1 * F, oW2 = oB1 + H1, oB2 = oW2 + H2 * H1, oW3 = oB2 + H2, oB3 = oW3 + H2;
    // dW1 tile: rows 16w .. 16w+15 of [H1][F] are one contiguous piece of the partial vector.  The D
    // fragments (4 rows x 16 columns per register quad) go through a wave-private LDS tile (all LDS
    // is dead by now; the last barrier of the query loop is behind every wave) and leave as 16-byte
    // stores of consecutive addresses (the row pitch of the partial vectors is a multiple of 4).
    {
        float *tile = reinterpret_cast<float *>(smem) + (size_t)w * 16 * IP;
#pragma unroll
        for (int c = 0; c < NT; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) tile[(4 * g + i) * IP + 16 * c + c16] = acc[c][i];
        float *drow = dst + (size_t)16 * w * F;
        for (int idx = lane; idx < 16 * C; idx += 64) {
            const int r = idx / C, f4 = idx - r * C;
            if (16 * w + r < H1)
                *reinterpret_cast<mlp_f4 *>(drow + 4 * idx) = *reinterpret_cast<const mlp_f4 *>(tile + r * IP + 4 * f4);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j2 = 4 * g + i;
        if (j2 < H2 && j1A < H1) dst[oW2 + j2 * H1 + j1A] = accW2[i];
        const float s1 = row16_sum(accB1[i]);
        const int j1 = 16 * w + 4 * g + i;
        if (c16 == 0 && j1 < H1) dst[oB1 + j1] = s1;
        accB2[i] = row16_sum(accB2[i]);
        accW3[i] = row16_sum(accW3[i]);
    }
    accB3 = wave_sum(accB3);
    // the per-document-owner sums (db2, dW3, db3) fold over the four waves in a fixed order
    // (behind the dW1 tiles of the store above: 64 image rows from the start of the segment)
    float *fold = reinterpret_cast<float *>(smem) + (size_t)64 * IP;
    float *slv = fold + (size_t)w * 40;            // [16] db2 | [16] dW3 | [1] db3
    if (c16 == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            slv[4 * g + i] = accB2[i];
            slv[16 + 4 * g + i] = accW3[i];
        }
    }
    if (lane == 0) slv[32] = accB3;
    __syncthreads();
    if (tid < 33) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < kM2Waves; ++k) t += fold[k * 40 + tid];
        if (tid < 16) { if (tid < H2) dst[oB2 + tid] = t; }
        else if (tid < 32) { if (tid - 16 < H2) dst[oW3 + tid - 16] = t; }
        else dst[oB3] = t;
    }
    M2_STAMP(7);                                  // partial vector written
#ifdef LTR_MLP_TRACE
    if (tid == 0)
        for (int i = 0; i < 15; ++i) reinterpret_cast<long long *>(p.scores_out)[16 * (size_t)blockIdx.x + i] = tr_[i];
#endif
}

// ---- host side ----
inline int mlp2_grid(int B)
{
    const int wgs = kM2Wgs * device_cu_count();
    return B < wgs ? B : wgs;
}

inline bool mlp2_takes(int F) { return mlp_bucket(F) <= kM2MaxNT; }

template <int KIND, int NT, int CT, int LT, bool FWD = false>
int launch_mlp2_ct(const MlpParams &p, int grid, hipStream_t stream)
{
    const size_t lds = mlp2_lds_bytes(KIND, NT, LT);
    LTR_ENSURE_LDS((mlp_tile_kernel<KIND, NT, CT, LT, FWD>), lds);
    hipLaunchKernelGGL((mlp_tile_kernel<KIND, NT, CT, LT, FWD>), dim3((unsigned)grid), dim3(kM2Threads), lds,
                       stream, p);
    return (int)hipGetLastError();
}

template <int KIND, int LT, bool FWD = false>
int launch_mlp2_len(const MlpParams &p, int grid, hipStream_t stream)
{
    switch (mlp_bucket(p.F)) {
    case 3: return launch_mlp2_ct<KIND, 3, 0, LT, FWD>(p, grid, stream);
    case 5: return launch_mlp2_ct<KIND, 5, 0, LT, FWD>(p, grid, stream);
    default:
        if (p.F == 136) return launch_mlp2_ct<KIND, 9, 34, LT, FWD>(p, grid, stream);
        return launch_mlp2_ct<KIND, 9, 0, LT, FWD>(p, grid, stream);
    }
}

// training step; lists up to 128 documents park their tiles, longer ones (<= 256) run the forward
// pass of a fill again in the backward pass
template <int KIND>
int launch_mlp2_kind(const MlpParams &p, int grid, hipStream_t stream)
{
    if (p.L <= kM2ParkLen) return launch_mlp2_len<KIND, kM2ParkLen>(p, grid, stream);
    return launch_mlp2_len<KIND, kM2MaxLen>(p, grid, stream);
}

// scores only, lists of 129 .. 256 documents (shorter ones: the 8-wave kernel of ltr_mlp.inc)
inline int launch_mlp2_scores(const MlpParams &p, int grid, hipStream_t stream)
{
    return launch_mlp2_len<LTR_HINGE, kM2MaxLen, true>(p, grid, stream);
}
