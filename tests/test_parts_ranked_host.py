"""CPU tier: the counting formulation of the hinge kinds in the parts kernel (csrc/ltr_parts.inc: parts_hinge_ranked,
parts_rank_buckets) restated in numpy, step for step, against the oracle's pair pass -- the companion of
tests/test_sorted_runs_host.py for the bucket path; tests/test_gpu_hinge_counting.py runs the same inputs on the device.

The device path replaces the O(n^2) pair pass (loss/pairwise_additive.py:107-113) on integer grades 0..4 by: S1 the
qualification test (finite scores, integer grades 0..4, a score span above `need`), S2 a histogram over NB score buckets
with per-bucket counts of "grade >= g" and fixed-point sums of the scores of "grade < g", S3 prefix / suffix scans, S4 the
documents dealt into their buckets, S5 per document two table look-ups and an exact visit of the three buckets around each
window edge with the pair pass's own fp32 predicate fl(1 -+ fl(s - s_m)) >= 0.

The restatement models the WIDTHS of the kernel's accumulators, so it states what the arithmetic gives and not what was
meant.  Two modes of S5's sum of the visited margins:
  "u64"  the kernel as it is: 64-bit sum of margins as 32-bit fractions of `3 bucket widths + 2` (a visited margin is
         below 1 + 2.5 bucket widths) -- cannot wrap (2048 x 2^32), quantum ~2e-10 of the margins visited;
  "u32"  the kernel as it was: 32-bit sum of margins as 24-bit fractions of `range + 2`.  It wraps when some 600
         lower-graded documents with margins near 1 sit in the visited buckets (a tie cluster at the query's minimum),
         and floors every margin to (range + 2) / 2^24 (one far outlier: all other documents in bucket 0).
test_the_old_widths_reproduce_both_defects keeps the reason for the change on record.

Claims tested: the per-document gradient counts are the fp32-predicate pair pass's integers, document for document, on
every distribution of scores the device test uses; the loss is within the long-list tolerance (rtol 5e-4, atol 1e-5) of
the fp64 oracle's; the hinge kinds see the labels only through their order (the device test reaches the parts kernel's pair
pass by adding 5 to every label)."""
import numpy as np
import pytest

from oracle import ltr_oracle as O

f32 = np.float32
T = 256                                    # kPtThreads
RANK_MIN_N, RANK_MAX_N = 192, 2048         # kPtRankMinN, kPtRankMaxN


def rank_buckets(n):
    """parts_rank_buckets: ~2 documents per bucket, ~4 on the longest lists."""
    nbk = 64
    while (4 if n > 1024 else 2) * nbk < n:
        nbk <<= 1
    return nbk


def rank_need(lo, hi, NB):
    """S1: the least score span the buckets accept (8 ulps of the largest |s| + 1 per bucket), in the kernel's fp32."""
    return f32(f32(f32(NB) * f32(9.6e-7)) * f32(max(abs(f32(lo)), abs(f32(hi))) + f32(1.0)))


def ranked_hinge(s, y, mode="u64"):
    """parts_hinge_ranked on one query held by one part (r0 = 0, rows = n).  Returns None where the kernel returns false
    (the caller runs the pair pass), else (g[n] integer gradients of the pair sum, pair sum)."""
    s = np.asarray(s, dtype=np.float32)
    yf = np.asarray(y, dtype=np.float32)
    n = len(s)
    NB = rank_buckets(n)
    # ---- S1 ----
    with np.errstate(invalid="ignore", over="ignore"):
        bad = bool(np.any(~(np.abs(s) < np.inf)) or np.any(~((yf == np.floor(yf)) & (yf >= 0) & (yf <= 4))))
        lo, hi = f32(np.min(s)), f32(np.max(s))               # (fminf / fmaxf: a NaN is `bad` anyway)
        span = f32(hi - lo)
    if bad or not (span > rank_need(lo, hi, NB)):
        return None
    yi = yf.astype(np.int64)
    scale = f32(f32(NB) / span)

    def bucket(x):
        f = ((np.asarray(x, dtype=np.float32) - lo).astype(np.float32) * scale).astype(np.float32)
        bb = np.where(f < 0, 0, np.trunc(f).astype(np.int64))
        return np.minimum(bb, NB - 1)

    qs = f32(f32(1073741824.0) / span)                        # scores -> 30-bit fractions of the range
    qs_inv = f32(span * f32(1.0 / 1073741824.0))
    if mode == "u32":
        qu = f32(f32(16777216.0) / f32(span + f32(2.0)))      # margins -> 24-bit fractions of range + 2
        qu_inv = f32(f32(span + f32(2.0)) * f32(1.0 / 16777216.0))
        wrap = 1 << 32
    else:
        mmax = f32(f32(f32(3.0) * span) / f32(NB) + f32(2.0))  # above 1 + 2 bucket widths, the largest margin a visit meets
        qu = f32(f32(4294967296.0) / mmax)                    # margins -> 32-bit fractions of it
        qu_inv = f32(mmax * f32(1.0 / 4294967296.0))
        wrap = 1 << 64
    # ---- S2: histogram, counts of grade >= g, sums of the quantised scores of grade < th ----
    bk = bucket(s)
    hist = np.bincount(bk, minlength=NB)
    q = np.trunc(((s - lo).astype(np.float32) * qs).astype(np.float32)).astype(np.int64)      # (unsigned)(float)
    cnt = np.zeros((5, NB), dtype=np.int64)                   # cnt[g][b]: grade >= g in bucket b (16-bit fields: n <= 2048)
    sums = np.zeros((5, NB), dtype=np.int64)                  # sums[th][b]: sum of q over grade < th in bucket b (u64)
    for g in range(1, 5):
        cnt[g] = np.bincount(bk[yi >= g], minlength=NB)
        sums[g] = np.bincount(bk[yi < g], weights=q[yi < g].astype(np.float64), minlength=NB).astype(np.int64)   # < 2^53: exact
    # ---- S3: exclusive prefixes of histogram and counts (entry NB = the totals), inclusive suffix of the sums ----
    start = np.concatenate([[0], np.cumsum(hist)])
    aggC = np.concatenate([np.zeros((5, 1), dtype=np.int64), np.cumsum(cnt, axis=1)], axis=1)
    aggS = np.concatenate([np.cumsum(sums[:, ::-1], axis=1)[:, ::-1], np.zeros((5, 1), dtype=np.int64)], axis=1)
    # ---- S4: the documents of a bucket, in any order ----
    order = np.argsort(bk, kind="stable")
    es, ey = s[order], yi[order]
    # ---- S5: every document's two windows; the rows of a chunk side by side, their visits padded to the longest ----
    g_out = np.zeros(n, dtype=np.int64)
    term = np.zeros(n, dtype=np.float32)                      # what the document's thread adds to its lsum
    bt_up, bt_dn = bucket((s + f32(1.0)).astype(np.float32)), bucket((s - f32(1.0)).astype(np.float32))

    def visit(rows, bt):
        b0, b1 = np.maximum(bt[rows] - 1, 0), np.minimum(bt[rows] + 2, NB)
        e0, e1 = start[b0], start[b1]
        idx = e0[:, None] + np.arange(max(int(np.max(e1 - e0)), 1))[None, :]
        valid = idx < e1[:, None]
        idx = np.minimum(idx, n - 1)
        return b0, b1, es[idx], ey[idx], valid

    for c0 in range(0, n, 128):
        rows = np.arange(c0, min(c0 + 128, n))
        sk, yk = s[rows], yi[rows]
        # higher labels m: the pair counts iff fmaf(1, s - s_m, 1) >= 0
        b0, b1, xs, xy, valid = visit(rows, bt_up)
        uu = ((sk[:, None] - xs).astype(np.float32) + f32(1.0)).astype(np.float32)
        A = aggC[np.minimum(yk + 1, 4), b0] + np.count_nonzero(valid & (xy > yk[:, None]) & (uu >= 0), axis=1)
        A = np.where(yk < 4, A, 0)
        # lower labels m: the pair counts iff fmaf(-1, s - s_m, 1) >= 0
        b0, b1, xs, xy, valid = visit(rows, bt_dn)
        yt = np.maximum(yk, 1)                                 # (threshold y: grade < y; rows of grade 0 are masked below)
        Bc = (n - start[b1]) - (aggC[yt, NB] - aggC[yt, b1])
        lk = ((Bc.astype(np.float32) * ((f32(1.0) - sk).astype(np.float32) + lo).astype(np.float32)).astype(np.float32)
              + (aggS[yt, b1].astype(np.float32) * qs_inv).astype(np.float32)).astype(np.float32)
        uu = (f32(1.0) - (sk[:, None] - xs).astype(np.float32)).astype(np.float32)
        on = valid & (xy < yk[:, None]) & (uu >= 0)
        Bc = Bc + np.count_nonzero(on, axis=1)
        fixed = np.where(on, np.trunc((uu * qu).astype(np.float32)), f32(0.0)).astype(np.uint64)     # (unsigned ...)(uu * qu)
        uq = np.sum(fixed, axis=1, dtype=np.uint64)            # wraps at 2^64 like the accumulator ...
        assert mode == "u32" or np.all(fixed < (1 << 32))       # (a term is converted to 32 bits in either mode)
        if wrap == 1 << 32:
            uq = uq & np.uint64(0xFFFFFFFF)                    # ... or at 2^32 like the old one
        tk = (lk + (uq.astype(np.float32) * qu_inv).astype(np.float32)).astype(np.float32)
        Bc = np.where(yk > 0, Bc, 0)
        term[rows] = np.where(yk > 0, tk, f32(0.0))
        g_out[rows] = A - Bc
    thread_sum = np.zeros(T, dtype=np.float32)                # lsum of thread k % T, rows in increasing order
    for c0 in range(0, n, T):
        m = min(T, n - c0)
        thread_sum[:m] = (thread_sum[:m] + term[c0:c0 + m]).astype(np.float32)
    return g_out, float(np.sum(thread_sum.astype(np.float64)))


def pair_pass_f32(s, y):
    """The pair pass with the kernels' fp32 predicate, by brute force: (integer gradients, pair sum with fp32 terms summed
    in fp64)."""
    s = np.asarray(s, dtype=np.float32)
    y = np.asarray(y)
    u = (f32(1.0) - (s[:, None] - s[None, :]).astype(np.float32)).astype(np.float32)     # [i, j]: i the higher label
    act = (y[:, None] > y[None, :]) & (u >= 0)
    g = act.sum(axis=0).astype(np.int64) - act.sum(axis=1).astype(np.int64)
    return g, float(np.sum(np.where(act, u, f32(0.0)).astype(np.float64)))


# ---------------------------------------------------------------------------------------------------------------------
# The score distributions (tests/test_gpu_hinge_counting.py draws the same ones)
# ---------------------------------------------------------------------------------------------------------------------
def flavour_scores(flavour, n, rng, y=None):
    """fp32 scores of one query of n documents (y: its grades, rewritten in place where the flavour places a grade)."""
    z = rng.standard_normal(n).astype(np.float32)
    u = rng.random(n).astype(np.float32)
    if flavour.startswith("cluster_"):                        # 75 % of the documents tie exactly; the rest over a range
        where, rng_w = flavour.split("_")[1], float(flavour.split("_")[2])
        s = (u * f32(rng_w)).astype(np.float32)
        tie = rng.random(n) < 0.75
        s[0], s[1] = f32(0.0), f32(rng_w)                     # (both ends of the range are there)
        tie[:2] = False
        s[tie] = {"min": f32(0.0), "max": f32(rng_w), "mid": f32(0.5 * rng_w)}[where]
        return (s + f32(0.25)).astype(np.float32)             # (the scored bias of all-zero feature rows)
    if flavour == "two_clusters":                             # two tie clusters exactly 1.0 apart
        s = (z * f32(0.7)).astype(np.float32)
        pick = rng.random(n)
        s[pick < 0.35] = f32(-0.375)
        s[(pick >= 0.35) & (pick < 0.7)] = f32(0.625)
        return s
    if flavour in ("margin", "margin_exact", "margin_1000"):  # neighbours at differences of exactly 1 and 1 -+ one ulp
        # "margin": around 0, where fl(s - s_m) ROUNDS (1 + half an ulp of 1 becomes 1: the fp32 predicate takes pairs the
        # fp64 oracle's leaves out -- gradients off by one on an eighth of the documents, so the device test, which holds
        # every case to the oracle, draws the next two); "margin_exact": scores in [2, 4) and their partners in [1, 3), whose
        # differences are exact in fp32, so both precisions decide every pair alike; "margin_1000": exact likewise
        s = {"margin": z, "margin_exact": f32(2.0) + f32(2.0) * u, "margin_1000": z + f32(1000.0)}[flavour].astype(np.float32)
        a = s[0::4]
        m1 = (a - f32(1.0)).astype(np.float32)
        s[1::4] = m1[:len(s[1::4])]
        s[2::4] = np.nextafter(m1, f32(np.inf))[:len(s[2::4])]
        s[3::4] = np.nextafter(m1, f32(-np.inf))[:len(s[3::4])]
        return s
    if flavour == "offset_1000":
        return (f32(1000.0) + u * f32(rng.uniform(2.0, 4.0))).astype(np.float32)
    if flavour == "offset_-5000":
        return (f32(-5000.0) + u * f32(rng.uniform(2.0, 4.0))).astype(np.float32)
    if flavour in ("need_above", "need_below"):               # offset 1000, the span just to either side of `need`
        NB = rank_buckets(n)
        span = f32(rank_need(1000.0, 1001.0, NB)) * (f32(1.02) if flavour == "need_above" else f32(0.98))
        s = (f32(1000.0) + u * span).astype(np.float32)
        s[0], s[1] = f32(1000.0), f32(f32(1000.0) + span)
        return s
    if flavour.startswith("outlier_"):                        # outlier_<top|bottom>_<exponent>_<grade>
        _, side, ex, gr = flavour.split("_")
        s = z.copy()
        at = 0 if int(ex) == 5 else n // 3                    # (document 0 is the cluster kernel's centre of the pair sum)
        s[at] = f32(10.0 ** int(ex)) * (f32(1.0) if side == "top" else f32(-1.0))
        if y is not None:
            y[at] = int(gr)
        return s
    if flavour == "lognormal":
        return np.exp(f32(3.0) * z).astype(np.float32)
    if flavour == "grid_8":
        return (np.round(z * f32(8.0)) / f32(8.0)).astype(np.float32)
    assert flavour == "gaussian", flavour
    return z


FLAVOURS = ["cluster_min_2", "cluster_min_0.5", "cluster_max_2", "cluster_mid_2", "two_clusters", "margin", "margin_exact", "margin_1000",
            "offset_1000", "offset_-5000", "need_above", "need_below", "outlier_top_3_4", "outlier_top_4_4", "outlier_top_5_4",
            "outlier_top_5_0", "outlier_top_4_0", "outlier_bottom_5_0", "outlier_bottom_5_4", "lognormal", "grid_8", "gaussian"]


def _query(flavour, n, seed):
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 5, n)
    s = flavour_scores(flavour, n, rng, y)
    return s, y


def _oracle(kind, s, y):
    l, g = O.pairwise_loss(kind, s.reshape(1, -1).astype(np.float64), y.reshape(1, -1), np.array([len(s)]))
    return float(l[0]), g[0]


@pytest.mark.parametrize("flavour,n", [(f, 2000) for f in FLAVOURS] + [
    (f, m) for m in (2048, 1500, 257) for f in ("cluster_min_2", "margin", "need_above", "outlier_top_5_4", "lognormal", "grid_8")])
def test_counting_gives_the_pair_pass(flavour, n):
    """Gradient counts equal to the fp32-predicate pair pass's, exactly; the pair sum within the long-list tolerance of
    the fp64 oracle's, and of the fp32 pair pass's far inside it."""
    s, y = _query(flavour, n, 1000 + n)
    got = ranked_hinge(s, y)
    if flavour == "need_below":
        assert got is None                                    # the buckets would be narrower than the predicate's rounding
        return
    assert got is not None, "the query must take the counting formulation"
    g, raw = got
    gb, lb = pair_pass_f32(s, y)
    assert np.array_equal(g, gb)
    assert raw == pytest.approx(lb, rel=2e-6, abs=1e-4)
    want, want_g = _oracle("hinge", s, y)
    assert np.isclose(raw, want, rtol=5e-4, atol=1e-5)
    # the fp32 pair terms alone are far inside the bound, so the oracle is a fair reference for these inputs -- for the
    # gradients too, but where fl(s - s_m) rounds across the margin ("margin")
    assert np.isclose(lb, want, rtol=2e-6, atol=1e-5)
    if flavour != "margin":
        assert np.array_equal(gb, np.rint(want_g).astype(np.int64)) and np.array_equal(np.rint(want_g), want_g)


def test_the_old_widths_reproduce_both_defects():
    """The 32-bit sum of 24-bit margin fractions of range + 2 (the kernel before this file existed): (1) it wraps under a tie
    cluster at the query's minimum -- the loss tens of per cent low, the integer gradients untouched; the same cluster at
    the maximum or in the middle is harmless; (2) under one far outlier every margin is floored to (range + 2) / 2^24:
    -2e-4, -2e-3, -2e-2 at 1e4, 1e5, 1e6.  The 64-bit mode passes all of them."""
    n = 2000
    for flavour, low, high in [("cluster_min_2", -0.6, -0.05), ("cluster_min_0.5", -0.6, -0.05)]:
        s, y = _query(flavour, n, 7)
        gb, lb = pair_pass_f32(s, y)
        g, raw = ranked_hinge(s, y, mode="u32")
        assert np.array_equal(g, gb)
        assert low < raw / lb - 1.0 < high, (flavour, raw / lb - 1.0)
        assert ranked_hinge(s, y)[1] == pytest.approx(lb, rel=2e-6)
    for flavour in ("cluster_max_2", "cluster_mid_2"):
        s, y = _query(flavour, n, 7)
        assert ranked_hinge(s, y, mode="u32")[1] == pytest.approx(pair_pass_f32(s, y)[1], rel=2e-6)
    for ex, low, high in [(4, -4e-4, -1e-4), (5, -4e-3, -1e-3), (6, -4e-2, -1e-2)]:
        s, y = _query("outlier_top_%d_4" % ex, n, 7)
        gb, lb = pair_pass_f32(s, y)
        g, raw = ranked_hinge(s, y, mode="u32")
        assert np.array_equal(g, gb)
        assert low < raw / lb - 1.0 < high, (ex, raw / lb - 1.0)
        assert ranked_hinge(s, y)[1] == pytest.approx(lb, rel=2e-6)


def test_qualification():
    """S1: lists the counting formulation declines (the kernel's caller also requires kPtRankMinN <= n <= kPtRankMaxN and
    rows * n >= kPtRankMinWork)."""
    rng = np.random.default_rng(3)
    n = 600
    s, y = rng.standard_normal(n).astype(np.float32), rng.integers(0, 5, n)
    assert ranked_hinge(s, y) is not None
    assert ranked_hinge(s, y + 5) is None                     # grades 5..9: how the device test reaches the pair pass
    assert ranked_hinge(s, y + 0.5) is None
    assert ranked_hinge(s, y - 1) is None
    for v in (np.inf, -np.inf, np.nan):
        t = s.copy()
        t[17] = v
        assert ranked_hinge(t, y) is None
    assert ranked_hinge(np.full(n, f32(0.3)), y) is None
    assert ranked_hinge((s * f32(1e-7)).astype(np.float32), y) is None
    assert [rank_buckets(m) for m in (192, 257, 1024, 1025, 2000, 2048)] == [128, 256, 512, 512, 512, 512]


@pytest.mark.parametrize("kind", ["hinge", "dcg_hinge"])
def test_the_hinge_kinds_see_only_the_order_of_the_labels(kind):
    """Adding 5 to every label leaves the oracle's loss and gradients of the hinge kinds unchanged, bit for bit: the device
    test uses it to send a query the counting formulation takes down the parts kernel's pair pass."""
    for flavour in ("gaussian", "cluster_min_2", "outlier_top_5_0"):
        s, y = _query(flavour, 300, 11)
        l0, g0 = _oracle(kind, s, y)
        l5, g5 = _oracle(kind, s, y + 5)
        assert l0 == l5 and np.array_equal(g0, g5)
