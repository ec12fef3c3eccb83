"""GPU tier: the two counting formulations of the hinge kinds -- score buckets in the parts kernel (csrc/ltr_parts.inc:
parts_hinge_ranked), sorted runs in the cluster kernel (csrc/ltr_cluster.inc: cluster_hinge_from_runs) -- on scores that
cluster and scores that spread wide, against the fp64 oracle AND against the same kernel's own pair pass.
tests/test_parts_ranked_host.py restates the bucket path in numpy and draws the same distributions.

Every batch holds one flavour of query, drawn again per query with another seed, lists ragged from 3/4 of the list
length up, one list of exactly L documents and one of 150 (below kPtRankMinN: the pair pass).  The scores are designed: W = e_0,
bias 0, X[:, :, 0] = the scores, the other columns random (dW still sums real rows) -- but for the two `cluster_min`
flavours, whose tied documents are ALL-ZERO feature rows under a general W and a non-zero bias (they score the bias: how
such a cluster arises in practice), the others laid along W.

Flavours: 75 % of the documents tied at the query's minimum with the rest over a range of 2 or 0.5, the same cluster at
the maximum and in the middle; two tie clusters exactly 1 apart; neighbours at differences of exactly 1 and 1 -+ one ulp,
in [1, 4) and around 1000 (differences that fp32 forms exactly, so the fp64 oracle decides every pair like the kernels;
the rounding case around 0 is tests/test_parts_ranked_host.py's `margin`); offsets 1000 and -5000 with a range of 2-4;
offset 1000 with the span 2 % above and 2 % below the bucket path's `need` threshold in alternate queries; one outlier
at +1e3 / 1e4 / 1e5 of grade 4 or 0 or at -1e5 (the outlier at +-1e5 is document 0); log-normal exp(3 N(0, 1)); a 1/8 grid;
plain Gaussian; int32 labels on two of them.

What the file found when it was written (MI355X, largest relative loss error over the rows of a batch; the full table is in
DESIGN.md section 4.3.1):
  * bucket path, margins summed in 32 bits as 24-bit fractions of range + 2: the sum WRAPPED under the tie cluster at the
    minimum -- hinge -18 % (range 2) and -37 % (range 0.5), dcg_hinge's loss -1.5 % / -3.3 % and its gradient scale with it;
    and every margin was floored to (range + 2) / 2^24 under an outlier: 1.6e-5 / 1.9e-4 / 1.9e-3 at 1e3 / 1e4 / 1e5,
    3.5e-5 on the log-normal scores.  Now 64-bit sums of 32-bit fractions of 3 bucket widths + 2: all below 3e-7.
  * sorted runs, #active + sum (s - c) g with c = the query's first score: 5e-4 .. 1.8e-3 with the outlier in that place.
    Now c = the median score of the first run: below 3e-7.
  * the pair-pass runs stay below 3e-7 of the oracle on every flavour (they vouch for the inputs), so bound (b) below is
    rtol 3e-6 everywhere.

Every case asserts (a) loss per row (rtol 5e-4, atol 1e-5), dW and db (2e-4 max(1, max |dW|)) against O.linear_pairwise: the
long-list bounds of tests/test_gpu_fullsize.py; (b) the counting path against the kernel's pair pass -- the parts kernel's by
running the batch again with 5 added to every label (grades 5..9 disqualify the query; the hinge kinds see only the order of the
labels: tests/test_parts_ranked_host.py), the cluster kernel's by ltr_debug_cluster_mode(2) -- per-row loss within the larger of
rtol 3e-6 / atol 2e-5 and twice the pair pass's own largest relative error against the oracle in that batch, never above 5e-4;
hinge's dW and db bit-identical between the two on BOTH kernels (the per-document gradients are the same integers, reduced
alike); dcg_hinge's within the rounding of two fp32 sums of the same terms; (c) a second run bit-identical, the device status
clean."""
import numpy as np
import pytest
import torch

from oracle import ltr_oracle as O
from tests.conftest import synth
from tests.test_parts_ranked_host import flavour_scores

pytestmark = pytest.mark.gpu

FLAVOURS = ["cluster_min_2", "cluster_min_0.5", "cluster_max_2", "cluster_mid_2", "two_clusters", "margin_exact", "margin_1000",
            "offset_1000", "offset_-5000", "need_both", "outlier_top_3_4", "outlier_top_4_4", "outlier_top_5_4",
            "outlier_top_3_0", "outlier_top_4_0", "outlier_top_5_0", "outlier_bottom_5_0", "lognormal", "grid_8", "gaussian",
            "gaussian_int32", "cluster_min_2_int32"]
# (path, kind, B, L, F).  The parts kernel carries the bucket tables only in its heaviest workgroups (two per CU) and where a
# part's rows x L reach kPtRankMinWork (choose_parts_shape): 6 x 2000 x 512 and 6 x 2048 x 512 are the smallest batches that
# get them at lists long enough for the wrap (some 600 lower-graded documents in the visited buckets) -- parts of 80 rows,
# counting from 1000 documents on.  40 x 2000 x 64 (the shape of test_parts_kernel_ranked_hinge_falls_back) and
# 60 x 2048 x 32 plan lighter workgroups WITHOUT the tables: every query of theirs takes the pair pass, (measured: their
# losses have the pair pass's bits) -- they stay as the control of the label shift.  The cluster kernel takes its sorted runs at both of
# its shapes.
PATHS = [("parts", "hinge", 6, 2000, 512), ("parts", "dcg_hinge", 6, 2048, 512),
         ("parts", "hinge", 40, 2000, 64), ("parts", "dcg_hinge", 60, 2048, 32),
         ("cluster", "hinge", 33, 1000, 220), ("cluster", "dcg_hinge", 33, 1000, 220),
         ("cluster", "hinge", 64, 300, 64), ("cluster", "dcg_hinge", 64, 300, 64)]
# shapes whose qualifying queries really count: their losses cannot all have the pair pass's bits (other summation
# orders, fixed point), so a batch of identical bits means the path under test did not run
COUNTS = {(6, 2000, 512), (6, 2048, 512), (33, 1000, 220), (64, 300, 64)}

_batches = {}


def _batch(flavour, B, L, F):
    """(X, W, b, y, n, int32 labels?) of one flavour: built once, shared by the cases of a shape, never written."""
    key = (flavour, B, L, F)
    if key in _batches:
        return _batches[key]
    int32 = flavour.endswith("_int32")
    fl = flavour[:-6] if int32 else flavour
    _, y, n, X, W, b = synth(B, L, 4242 + L, F=F)
    y = y.numpy().copy()
    n = torch.clamp(n, min=(3 * L) // 4)
    n[0], n[1] = L, 150
    X = X.clone()
    zero_rows = fl.startswith("cluster_min")
    if zero_rows:
        b = torch.tensor([0.25])
        along = (W / float(W.double().pow(2).sum())).float()             # x = t * along scores t
    else:
        W = torch.zeros(F)
        W[0] = 1.0
        b = torch.zeros(1)
    for q in range(B):
        nq = int(n[q])
        rng = np.random.default_rng(100000 + 97 * q + L)
        f = fl if fl != "need_both" else ("need_above" if q % 2 == 0 else "need_below")
        s = flavour_scores(f, nq, rng, y[q])
        if zero_rows:
            t = torch.from_numpy(s - np.float32(0.25))                   # >= 0: the tied documents are the zero rows
            X[q, :nq] = t[:, None] * along[None, :]
        else:
            X[q, :nq, 0] = torch.from_numpy(s)
    _batches[key] = (X, W, b, torch.from_numpy(y), n, int32)
    return _batches[key]


def _step(args, kind):
    from pytorchltr_amd.fused import linear_loss_step
    return tuple(t.cpu() for t in linear_loss_step(*args, loss=kind))


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("path", PATHS, ids=lambda p: "%s-%s-%dx%dx%d" % p)
def test_hinge_by_counting(path, flavour):
    from pytorchltr_amd import _C
    which, kind, B, L, F = path
    lib = _C.lib()
    dev = torch.device("cuda:0")
    assert lib.ltr_linear_fused_plan(getattr(_C, kind.upper()), B, L, F) == (_C.PLAN_PARTS if which == "parts" else _C.PLAN_CLUSTER)
    X, W, b, y, n, int32 = _batch(flavour, B, L, F)
    yd = y.to(dev).to(torch.int32) if int32 else y.to(dev)
    args = (X.to(dev), W.to(dev), b.to(dev), yd, n.to(dev))
    loss, dW, db = _step(args, kind)
    again = _step(args, kind)
    if which == "parts":
        loss_p, dW_p, db_p = _step(args[:3] + (yd + 5,) + args[4:], kind)
    else:
        lib.ltr_debug_cluster_mode(2)
        try:
            loss_p, dW_p, db_p = _step(args, kind)
        finally:
            lib.ltr_debug_cluster_mode(0)
    _C.device_status()
    want_l, want_s, want_dW, want_db = O.linear_pairwise(kind, X.numpy(), W.numpy(), float(b[0]), y.numpy(), n.numpy(),
                                                    np.full(B, 1.0 / B))
    tol = 2e-4 * max(1.0, float(np.max(np.abs(want_dW))))
    l, lp = loss.double().numpy(), loss_p.double().numpy()
    rel = lambda got: float(np.max(np.abs(got - want_l) / np.maximum(np.abs(want_l), 1e-30)))       # noqa: E731
    err_pair = rel(lp)
    rtol_b = min(5e-4, max(3e-6, 2.0 * err_pair))
    print("MEASURED %s %s %dx%dx%d %s: loss vs oracle counting %.3g pair %.3g | counting vs pair %.3g (allowed %.3g) | "
          "dW vs oracle counting %.3g pair %.3g of %.3g | hinge dW identical %s" % (
              (which, kind, B, L, F, flavour, rel(l), err_pair, float(np.max(np.abs(l - lp) / np.maximum(np.abs(lp), 1e-30))), rtol_b,
               float(np.max(np.abs(dW.numpy() - want_dW))), float(np.max(np.abs(dW_p.numpy() - want_dW))), tol,
               bool(torch.equal(dW, dW_p) and torch.equal(db, db_p)))))
    # (c) deterministic
    assert all(torch.equal(u, v) for u, v in zip((loss, dW, db), again)), "runs differ (the kernel must be deterministic)"
    # (a) the oracle: the pair pass first (it vouches for the inputs), then the counting path
    for name, (ll, ww, bb) in (("pair pass", (lp, dW_p, db_p)), ("counting", (l, dW, db))):
        assert np.all(np.isfinite(ll)), name
        assert np.isclose(ll, want_l, rtol=5e-4, atol=1e-5).all(), name          # every row
        assert np.max(np.abs(ww.numpy() - want_dW)) < tol, name
        assert abs(float(bb[0]) - want_db) < tol, name
    # (b) the same kernel's pair pass
    assert np.isclose(l, lp, rtol=rtol_b, atol=2e-5).all()
    if flavour == "gaussian" and kind == "hinge" and (B, L, F) in COUNTS:       # (dcg_hinge's -1 / log flattens the last bits)
        assert not torch.equal(loss, loss_p), "no query of this shape took the counting path"
    if kind == "hinge":
        assert torch.equal(dW, dW_p) and torch.equal(db, db_p)
    else:
        # The modifier's factor on the gradients comes from the summed loss and is applied at another place of the
        # reduction on either path: two fp32 sums of the same terms g_k x_kj / B in different association.  Each is within
        # depth * 2^-24 * sum |terms| of the exact sum, depth <= 32 (rows per thread, then trees), whatever cancels in the sum
        # itself (column 0 under an offset of -5000 cancels to 1e-7 of its terms).  A gradient scale from a wrapped
        # loss is 1e4 times beyond that.
        _, ds = O.pairwise_loss(kind, want_s, y.numpy(), n.numpy())
        live = np.arange(L)[None, :] < n.numpy()[:, None]
        ads = np.abs(ds) * live
        terms = np.concatenate([np.einsum("bk,bkj->j", ads, np.abs(X.numpy()).astype(np.float64)), [ads.sum()]]) / B
        bound = 64 * 2.0 ** -24 * terms + 1e-30
        diff = np.abs(np.concatenate([dW.numpy() - dW_p.numpy(), db.numpy() - db_p.numpy()]).astype(np.float64))
        print("MEASURED   dcg_hinge dW counting vs pair / bound: %.3g" % float(np.max(diff / bound)))
        assert np.all(diff <= bound)
