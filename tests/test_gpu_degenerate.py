"""GPU tier of the degenerate-query parity (run with `-m gpu` on an MI355X): the batches of tests/degenerate.py -- no
relevant document, one relevant document, all labels equal, lists of 0 / 1 / 2 documents, padded labels that must not
count, a grade above 4, a negative grade, next to one ordinary query -- through every kernel path, every row against
the fp64 oracle (pinned to the real reference on these very queries by tests/test_degenerate_host.py).

The rules these queries exercise are written once per kernel family: `maxDCG == 0 -> 1`, "labels of padded documents
do not enter a loss's maxDCG", "a query without a y_i > y_j pair has zero gradient".  Each copy sits behind another
exchange (waves' shares, parts' terms, tile partials), so each path gets the same batches.

Scores are exact (W = e_0, bias 0.25, column 0 on a dyadic grid -- or constant: every score tied, the index tie rule
decides every rank), so fp32 and fp64 rank alike: NO row is excused as a rank flip, the bounds are the neighbouring
tests' own, unwidened:
  loss            rtol 2e-5 up to 256 documents, 5e-4 beyond, atol 1e-5
  dscores         tests/test_gpu_parity.py::_check_grad (hinge: exact); the long-pair path:
                  tests/test_gpu_long_pairs.py::_check_grad_vs_oracle
  dW, db          tests/test_gpu_fused.py::_check
  MLP step        tests/test_gpu_mlp.py::_check itself, on the builder's X, y, n (the scores are not exact there)
  listwise        tests/test_listwise.py, tests/test_gpu_listmle.py::_check, tests/test_gpu_linear_listwise.py,
                  tests/test_gpu_mlp_listwise.py::_compare
  metrics         tests/test_gpu_eval.py::_check
Rows whose loss and gradient are 0 in exact arithmetic (degenerate.zero_rows) must come out of the loss-only kernels
as exactly +-0.0: every term there is gated by a false predicate or multiplied by a zero gain.

Each case asserts the path it means to hit (ltr_linear_fused_plan, the workspace size of the split launch, the debug
hooks -- restored in `finally`)."""
import functools

import numpy as np
import pytest
import torch

from oracle import ltr_oracle as O
from tests.degenerate import (DCG_HINGE_ZERO, NO_RELEVANT, degenerate_batch, exact_scores, rows_of, zero_rows)
from tests.test_gpu_long_pairs import _check_grad_vs_oracle
from tests.test_gpu_parity import _check_grad

pytestmark = pytest.mark.gpu

KINDS = list(O.KINDS)
HINGES = ("hinge", "dcg_hinge")
MODES = ("grid", "constant")
LABELS = {"int64": torch.int64, "int32": torch.int32, "float32": torch.float32}


def _dev():
    assert torch.cuda.is_available(), "GPU tier needs a ROCm device"
    return torch.device("cuda:0")


def _code(kind):
    from pytorchltr_amd import _C
    return _C.__dict__[kind.upper()]


@functools.lru_cache(maxsize=8)
def _batch(B, L, F, mode, labels="int64"):
    """The builder's batch of one shape (CPU tensors, shared between the tests: never written to)."""
    X, W, b, y, n, fl = degenerate_batch(B, L, F, 7000 + 13 * L + F + B, scores=mode, label_dtype=LABELS[labels])
    return X, W, b, y, n, tuple(fl)


@functools.lru_cache(maxsize=None)
def _want_loss(kind, B, L, mode):
    """fp64 loss and dscores of the loss-only batches (F = 1: the feature tensor IS the score column)."""
    X, W, b, y, n, fl = _batch(B, L, 1, mode)
    return O.pairwise_loss(kind, exact_scores(X), y.numpy(), n.numpy())


@functools.lru_cache(maxsize=None)
def _want_step(kind, B, L, F, mode):
    X, W, b, y, n, fl = _batch(B, L, F, mode)
    return O.linear_pairwise(kind, X.numpy(), W.numpy(), float(b[0]), y.numpy(), n.numpy(), np.full(B, 1.0 / B))


class _Errors(list):
    """Every kind of a case is run and measured before the case fails: one GPU visit shows all of them."""

    def expect(self, ok, what, *figures):
        if not ok:
            self.append("%s %s" % (what, " ".join(str(f) for f in figures)))

    def done(self):
        assert not self, "\n".join(self)


def _loss_bound(L):
    return (5e-4 if L > 256 else 2e-5), 1e-5


def _loss_excess(got, want, L):
    """Worst |got - want| - (atol + rtol |want|) over the rows (<= 0: inside the bound), and the row."""
    rtol, atol = _loss_bound(L)
    ex = np.abs(np.asarray(got, dtype=np.float64) - want) - (atol + rtol * np.abs(want))
    r = int(np.argmax(ex))
    return float(ex[r]), r


def _check_rows(errs, kind, loss, ds, want_l, want_g, y, n, fl, L, what, long_path=False):
    loss = np.asarray(loss, dtype=np.float64)
    errs.expect(np.all(np.isfinite(loss)) and np.all(np.isfinite(ds)), what, "not finite", loss)
    ex, r = _loss_excess(loss, want_l, L)
    print("%s: loss worst excess %.3e (row %d, %s: got %r want %r)" % (what, ex, r, fl[r], loss[r], want_l[r]))
    errs.expect(ex <= 0, what, "loss row %d (%s): got %r want %r" % (r, fl[r], loss[r], want_l[r]))
    try:
        if long_path:
            _check_grad_vs_oracle(ds, want_g, what)
        else:
            _check_grad(ds, want_g, what, exact=(kind == "hinge"))
    except AssertionError as e:
        bad = np.nonzero(np.any(np.abs(ds - want_g) > 1e-5 * np.max(np.abs(want_g), axis=1, keepdims=True) + 1e-6, axis=1))[0]
        errs.append("%s gradient: %s rows %s" % (what, str(e)[:200], [(int(i), fl[i]) for i in bad[:6]]))
    real = np.arange(L)[None, :] < np.clip(n, 0, L)[:, None]
    errs.expect(not ds[~real].any(), what, "gradient past n[b]")
    # rows without a pair: exactly +-0.0 (dcg_hinge: its constant, to the loss tolerance above)
    rows = zero_rows(kind, y, n)
    assert rows.size >= 3
    if kind != "dcg_hinge":
        errs.expect(not loss[rows].any(), what, "loss of pair-free rows not exactly 0:", loss[rows])
    else:
        assert np.all(want_l[rows] == DCG_HINGE_ZERO)
    errs.expect(not ds[rows].any(), what, "gradient of pair-free rows not exactly 0: max", np.abs(ds[rows]).max())


# ---------------------------------------------------------------------------------------------------------------------
# the loss-only kernels
# ---------------------------------------------------------------------------------------------------------------------
def _run_loss_only(kind, B, L, mode, labels="int64", cfg=None, long_lists=False):
    from pytorchltr_amd._autograd import pairwise_loss_and_grad
    X, W, b, y, n, fl = _batch(B, L, 1, mode, labels)
    dev = _dev()
    s = (X[:, :, 0] + b[0]).contiguous()
    loss, ds = pairwise_loss_and_grad(s.to(dev), y.to(dev), n.to(dev), _code(kind), 1.0, cfg=cfg, long_lists=long_lists)
    return loss.cpu().numpy(), ds.cpu().numpy().astype(np.float64)


def _loss_only_case(B, L, mode, labels="int64", cfg=None, long_lists=False, kinds=KINDS, tag=""):
    X, W, b, y, n, fl = _batch(B, L, 1, mode)
    errs = _Errors()
    for kind in kinds:
        loss, ds = _run_loss_only(kind, B, L, mode, labels, cfg, long_lists)
        want_l, want_g = _want_loss(kind, B, L, mode)
        _check_rows(errs, kind, loss, ds, want_l, want_g, y.numpy(), n.numpy(), fl, L,
                    "%s %s %dx%d %s %s" % (tag, kind, B, L, mode, labels), long_path=long_lists)
    errs.done()


def _plain_launch(B, L):
    """The shape takes ltr_pairwise_loss_f32 as it is: no split-query workspace for any kind."""
    from pytorchltr_amd import _C
    return all(_C.lib().ltr_pairwise_loss_workspace_bytes(_code(k), B, L) == 0 for k in KINDS)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", [37, 128, 300])
def test_loss_only_default_launch(L, mode):
    """One workgroup per query, the launch shape ltr_pairwise_loss_f32 picks: one wave tile, two, a long list."""
    _loss_only_case(24, L, mode, tag="default")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cfg", [(64, 1, 1), (128, 2, 4), (64, 0, 8)], ids=lambda c: "%d-%d-%d" % c)
def test_loss_only_explicit_launch_shapes(cfg, mode):
    """One document per thread on one wave, the widest split of the pair loop, and the symmetric pair pass (dpt 0)."""
    _loss_only_case(24, 300, mode, cfg=cfg, tag="cfg%s" % (cfg,))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,L", [(24, 1000), (12, 1025)])
def test_loss_only_split_query_launch(B, L, mode):
    """Several workgroups per query through the workspace entry point (the NDCG kinds behind their ranking pre-pass), and
    a list in the 1024 .. 2048 range, where the symmetric pass no longer applies; the same lists also as one plain
    launch."""
    from pytorchltr_amd import _C
    assert all(_C.lib().ltr_pairwise_loss_workspace_bytes(_code(k), B, L) > 0 for k in KINDS)
    _loss_only_case(B, L, mode, cfg="split", tag="split")
    if L == 1025:
        _loss_only_case(B, L, mode, tag="one workgroup")


@pytest.mark.parametrize("mode", MODES)
def test_loss_only_narrow_workgroups(mode):
    """4096 queries of 64 documents: several rounds of queries per CU, where choose_loss_shape gives a query one or two
    waves (tests/test_gpu_parity.py::test_many_queries_take_narrow_workgroups)."""
    assert _plain_launch(4096, 64)
    _loss_only_case(4096, 64, mode, tag="narrow")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sorted_preparation", [False, True], ids=["prepare_kernel", "sorted_preparation"])
def test_loss_only_forced_long_pair_path(sorted_preparation, mode):
    """ltr_pairwise_loss_long_f32 forced onto lists of 300 documents: the owner tiles against the streamed query behind
    the key sort and the label sort with ltr_longpair.inc's own maxDCG from the tile partials -- the long path's one
    preparation, so both ids run it, the second with ltr_debug_long_sort_all set as well."""
    from pytorchltr_amd import _C
    lib = _C.lib()
    prev = lib.ltr_debug_long_pairs_all(1)
    prev_sort = lib.ltr_debug_long_sort_all(1) if sorted_preparation else None
    try:
        assert lib.ltr_debug_long_pairs_all(1) == 1
        assert lib.ltr_pairwise_loss_long_workspace_bytes(_code("ndcg2"), 24, 300) > 0
        _loss_only_case(24, 300, mode, long_lists=True, tag="forced long")
    finally:
        if sorted_preparation:
            lib.ltr_debug_long_sort_all(prev_sort)
        lib.ltr_debug_long_pairs_all(prev)


@pytest.mark.parametrize("kind", KINDS)
def test_loss_only_long_pair_path_past_the_limit(kind):
    """... and for real: 4097 documents, one past ltr_max_list_len(), with long_lists=True.  Twelve queries, one of
    each flavour: the oracle's pair loop over them takes a second or two per kind."""
    from pytorchltr_amd import _C
    assert 4097 > _C.max_list_len()
    for mode in MODES:
        _loss_only_case(12, 4097, mode, long_lists=True, kinds=(kind,), tag="long")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", [37, 300])
def test_loss_only_fp64_scores(L, mode):
    """fp64 scores take the fp64 kernels (ltr_f64.inc, with a maxDCG guard of their own): bounds of
    tests/test_gpu_parity.py::test_fp64_scores_give_fp64_arithmetic."""
    from tests.test_gpu_parity import _loss_cls
    dev = _dev()
    X, W, b, y, n, fl = _batch(24, L, 1, mode)
    errs = _Errors()
    for kind in KINDS:
        what = "fp64 %s 24x%d %s" % (kind, L, mode)
        sc = torch.from_numpy(exact_scores(X)).to(dev).requires_grad_(True)
        out = _loss_cls(kind)()(sc, y.to(dev), n.to(dev))
        assert out.dtype == torch.float64
        out.sum().backward()
        loss, ds = out.detach().cpu().numpy(), sc.grad.cpu().numpy()
        want_l, want_g = _want_loss(kind, 24, L, mode)
        errs.expect(np.allclose(loss, want_l, rtol=1e-11, atol=1e-12), what, "loss err", np.abs(loss - want_l).max())
        scale = np.max(np.abs(want_g), axis=1, keepdims=True) + 1e-300
        errs.expect(np.all(np.abs(ds - want_g) <= 1e-11 * scale + 1e-13), what, "grad err", np.abs(ds - want_g).max())
        rows = zero_rows(kind, y.numpy(), n.numpy())
        if kind != "dcg_hinge":
            errs.expect(not loss[rows].any(), what, "loss of pair-free rows not exactly 0:", loss[rows])
        errs.expect(not ds[rows].any(), what, "gradient of pair-free rows not exactly 0")
    errs.done()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("labels", ["int32", "float32"])
def test_loss_only_label_dtypes(labels, mode):
    """The same values as int32 and float32 labels (float labels switch off the integer-label shortcuts)."""
    for L in (128, 300):
        _loss_only_case(24, L, mode, labels=labels, tag="default")


# ---------------------------------------------------------------------------------------------------------------------
# the fused Linear step
# ---------------------------------------------------------------------------------------------------------------------
class _Hooks:
    """ltr_debug_parts_all / ltr_debug_cluster_mode for one block, restored on the way out."""

    def __init__(self, parts_all=False, cluster_mode=0):
        self.parts_all, self.cluster_mode = parts_all, cluster_mode

    def __enter__(self):
        from pytorchltr_amd import _C
        lib = _C.lib()
        self.prev = lib.ltr_debug_parts_all(1) if self.parts_all else None
        if self.cluster_mode:
            lib.ltr_debug_cluster_mode(self.cluster_mode)
        return self

    def __exit__(self, *exc):
        from pytorchltr_amd import _C
        lib = _C.lib()
        if self.cluster_mode:
            lib.ltr_debug_cluster_mode(0)
        if self.parts_all:
            lib.ltr_debug_parts_all(self.prev)
        return False


def _step_case(B, L, F, mode, plan, labels="int64", kinds=KINDS, return_scores=False, parts_all=False, cluster_mode=0,
               tag=""):
    from pytorchltr_amd import _C
    from pytorchltr_amd.fused import linear_loss_step
    dev = _dev()
    lib = _C.lib()
    X, W, b, y, n, fl = _batch(B, L, F, mode, labels)
    Xd, Wd, bd, yd, nd = X.to(dev), W.to(dev), b.to(dev), y.to(dev), n.to(dev)
    # a batch made only of queries without a pair: the real labels all 0, list lengths and padded labels as they are
    real = torch.arange(L)[None, :] < n[:, None]
    y0d = torch.where(real, torch.zeros_like(y), y).to(dev)
    errs = _Errors()
    multi = plan in (_C.PLAN_CLUSTER, _C.PLAN_PARTS)
    with _Hooks(parts_all, cluster_mode):
        for kind in kinds:
            what = "%s %s %dx%dx%d %s %s" % (tag, kind, B, L, F, mode, labels)
            assert lib.ltr_linear_fused_plan(_code(kind), B, L, F) == plan, what
            out = linear_loss_step(Xd, Wd, bd, yd, nd, loss=kind, return_scores=return_scores)
            zero = linear_loss_step(Xd, Wd, bd, y0d, nd, loss=kind, return_scores=return_scores)
            torch.cuda.synchronize()
            if multi:
                _C.device_status()
            loss, dW, db = (t.cpu().numpy().astype(np.float64) for t in out[:3])
            want_l, want_s, want_dW, want_db = _want_step(kind, B, L, F, mode)
            errs.expect(np.all(np.isfinite(loss)) and np.all(np.isfinite(dW)), what, "not finite")
            ex, r = _loss_excess(loss, want_l, L)
            print("%s: loss worst excess %.3e (row %d, %s: got %r want %r)" % (what, ex, r, fl[r], loss[r], want_l[r]))
            errs.expect(ex <= 0, what, "loss row %d (%s): got %r want %r" % (r, fl[r], loss[r], want_l[r]))
            tol = 2e-5 * max(1.0, float(np.max(np.abs(want_dW)))) * (10 if L > 256 else 1)     # tests/test_gpu_fused.py::_check
            e_w, e_b = float(np.max(np.abs(dW - want_dW))), abs(float(db[0]) - want_db)
            print("%s: dW err %.3e db err %.3e tol %.3e" % (what, e_w, e_b, tol))
            errs.expect(e_w < tol and e_b < tol, what, "dW err %.3e db err %.3e tol %.3e" % (e_w, e_b, tol))
            if return_scores:
                sc = out[3].cpu().numpy()
                rl = real.numpy()
                errs.expect(np.array_equal(sc[rl].astype(np.float64), exact_scores(X)[rl]), what, "scores not exact")
            z_loss, z_dW, z_db = (t.cpu().numpy() for t in zero[:3])
            if kind == "dcg_hinge":
                errs.expect(np.allclose(z_loss, DCG_HINGE_ZERO, rtol=2e-5, atol=1e-5), what, "pair-free batch: loss", z_loss)
            else:
                errs.expect(not z_loss.any(), what, "pair-free batch: loss not exactly 0:", z_loss)
            errs.expect(not z_dW.any() and not z_db.any(), what, "pair-free batch: dW / db not exactly 0:",
                        np.abs(z_dW).max(), z_db)
    errs.done()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(24, 128, 136), (64, 129, 220), (64, 216, 220)], ids=lambda s: "%dx%dx%d" % s)
def test_step_register_tiles(shape, mode):
    """The 8-sweep register tile (lists up to 128 documents at MSLR's width), the 19-sweep and the 24-sweep tile."""
    from pytorchltr_amd import _C
    _step_case(*shape, mode, _C.PLAN_REGISTER_TILE, tag="tile")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(24, 128, 136, True), (24, 128, 6, False)], ids=["scores_out", "scalar_rows"])
def test_step_general_kernel(shape, mode):
    """The general (re-read) kernel: what a register-tile shape takes once the scores are asked for, and rows that are
    not whole float4 (F = 6, the scalar path)."""
    from pytorchltr_amd import _C
    B, L, F, scores_out = shape
    _step_case(B, L, F, mode, _C.PLAN_REGISTER_TILE if scores_out else _C.PLAN_GENERAL, return_scores=True, tag="general")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(33, 1000, 220), (64, 300, 64)], ids=lambda s: "%dx%dx%d" % s)
def test_step_cluster_kernel(shape, mode):
    """A query spread over a cluster of workgroups (ltr_cluster.inc's maxDCG from the members' shares); for the hinge
    kinds also the pair pass instead of the sorted runs (mode 2) and the write-through exchange (mode 1)."""
    from pytorchltr_amd import _C
    _step_case(*shape, mode, _C.PLAN_CLUSTER, tag="cluster")
    _step_case(*shape, mode, _C.PLAN_CLUSTER, kinds=HINGES, cluster_mode=2, tag="cluster pair pass")
    _step_case(*shape, mode, _C.PLAN_CLUSTER, kinds=HINGES, cluster_mode=1, tag="cluster write-through")


# the smallest lists the parts kernel takes at narrow rows under ltr_debug_parts_all (one part per query: the guard of the
# P == 1 branch), and lists of more rows than one part holds for any kind (16 rows per sweep, at most 25 sweeps: 400), so
# that the full lists are split and their maxDCG comes out of the combine of the parts' terms
PARTS_SHAPES = [(24, 257, 16), (24, 420, 16)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", PARTS_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_step_parts_kernel(shape, mode):
    """The parts kernel (ltr_parts.inc: maxDCG of a one-part query, and from the parts' terms) on the smallest shape it
    plans under ltr_debug_parts_all(1) -- one document shorter and the dispatcher picks another kernel whatever the hook
    says -- and on lists of two parts."""
    from pytorchltr_amd import _C
    lib = _C.lib()
    B, L, F = shape
    if shape == PARTS_SHAPES[0]:
        with _Hooks(parts_all=True):
            assert lib.ltr_linear_fused_plan(_C.HINGE, B, L - 1, F) != _C.PLAN_PARTS
    assert lib.ltr_linear_fused_plan(_C.HINGE, B, L, F) != _C.PLAN_PARTS          # (not without the hook)
    _step_case(B, L, F, mode, _C.PLAN_PARTS, parts_all=True, tag="parts")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("labels", ["int32", "float32"])
def test_step_label_dtypes(labels, mode):
    """The 8-sweep tile, the cluster kernel and the parts kernel on int32 and float32 labels of the same values: float
    labels switch off the integer-label shortcuts and the hinge kinds' sorted runs."""
    from pytorchltr_amd import _C
    _step_case(24, 128, 136, mode, _C.PLAN_REGISTER_TILE, labels=labels, tag="tile")
    _step_case(64, 300, 64, mode, _C.PLAN_CLUSTER, labels=labels, tag="cluster")
    _step_case(*PARTS_SHAPES[1], mode, _C.PLAN_PARTS, labels=labels, parts_all=True, tag="parts")


# ---------------------------------------------------------------------------------------------------------------------
# the fused MLP step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", [100, 200])
@pytest.mark.parametrize("layout", ["tile", "wide"])
def test_mlp_step(layout, L, mode):
    """mlp_loss_step on the guide's 136-50-10-1 network, both kernel layouts (ltr_debug_mlp_layout), one fill of the
    tile and the 129 .. 256 class; tests/test_gpu_mlp.py::_check on the builder's features, labels and lengths."""
    from pytorchltr_amd import _C
    from tests.test_gpu_mlp import _check, _mlp_params
    X, W, b, y, n, fl = _batch(24, L, 136, mode)
    params = _mlp_params(136, 50, 10, 31 + L)
    lib = _C.lib()
    lib.ltr_debug_mlp_layout(1 if layout == "wide" else 2)
    try:
        for kind in KINDS:
            _check(kind, X, y, n, params)
    finally:
        lib.ltr_debug_mlp_layout(0)


@pytest.mark.parametrize("mode", MODES)
def test_mlp_step_past_the_fused_limit(mode):
    """300 documents: no fused MLP kernel holds the list; the row score kernel, the loss kernel, the row gradient kernel."""
    from pytorchltr_amd import fused
    from tests.test_gpu_mlp import _check, _mlp_params
    assert not fused.mlp_supported(300, 24, 50, 10)
    X, W, b, y, n, fl = _batch(6, 300, 24, mode)
    params = _mlp_params(24, 50, 10, 331)
    for kind in KINDS:
        _check(kind, X, y, n, params)


# ---------------------------------------------------------------------------------------------------------------------
# the listwise losses
# ---------------------------------------------------------------------------------------------------------------------
def _listnet_uniform_rows(y, n, fl, want_g, s):
    """`zero` and `equal3`: P_y is uniform over the real documents, so d loss / d s = softmax(s) - 1 / n."""
    for r in rows_of(fl, ("zero", "equal3")):
        nb = int(n[r])
        p = np.exp(s[r, :nb] - s[r, :nb].max())
        assert np.allclose(want_g[r, :nb], p / p.sum() - 1.0 / nb, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", [37, 300, 1000])
def test_listwise_softmax_standalone(L, mode):
    from pytorchltr_amd._autograd import LISTWISE_SOFTMAX, pairwise_loss_and_grad
    dev = _dev()
    X, W, b, y, n, fl = _batch(24, L, 1, mode)
    s = exact_scores(X)
    want_l, want_g = O.listwise_softmax(s, y.numpy(), n.numpy())
    _listnet_uniform_rows(y.numpy(), n.numpy(), fl, want_g, s)
    for labels in LABELS:
        yd = _batch(24, L, 1, mode, labels)[3].to(dev)
        loss, ds = pairwise_loss_and_grad(torch.from_numpy(s).float().to(dev), yd, n.to(dev), LISTWISE_SOFTMAX)
        assert np.allclose(loss.cpu().numpy(), want_l, rtol=1e-5, atol=2e-6), labels       # tests/test_listwise.py
        assert np.allclose(ds.cpu().numpy(), want_g, rtol=1e-5, atol=1e-6), labels
        assert loss.cpu().numpy()[rows_of(fl, ("n0",))].tolist() == [0.0, 0.0]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [None, 10])
@pytest.mark.parametrize("L", [37, 300, 1000])
def test_listmle_standalone(L, k, mode):
    """One workgroup per query and, under ltr_debug_long_sort_all, the sort path.  `zero`, `equal3` (and every other
    run of equal labels) must fall back to the index order: the oracle's lexsort by (label, index)."""
    from tests.test_gpu_listmle import _LongSortAll, _call, _check
    from tests.test_listmle_host import oracle, oracle_order
    dev = _dev()
    X, W, b, y, n, fl = _batch(24, L, 1, mode)
    s = exact_scores(X).astype(np.float32)
    for r in rows_of(fl, ("zero", "equal3")):
        assert np.array_equal(oracle_order(y.numpy()[r], int(n[r])), np.arange(int(n[r])))
    want = oracle(s, y.numpy(), n.numpy(), k)
    ts, tn = torch.from_numpy(s).to(dev), n.to(dev)
    for labels in LABELS:
        ty = _batch(24, L, 1, mode, labels)[3].to(dev)
        _check(_call(ts, ty, tn, k=k), want, L)
        with _LongSortAll():
            _check(_call(ts, ty, tn, k=k), want, L)


def _listwise_reference(loss, k, X, y, n):
    """fp64 (loss (B), dW (F), db) of mean_b loss_b on the exact scores."""
    from tests.test_listmle_host import oracle
    s = exact_scores(X)
    want_l, ds = O.listwise_softmax(s, y.numpy(), n.numpy()) if loss == "listnet" else oracle(s, y.numpy(), n.numpy(), k)
    L = s.shape[1]
    real = np.arange(L)[None, :] < n.numpy()[:, None]
    up = np.where(real, ds, 0.0) / s.shape[0]
    return want_l, np.einsum("bl,blf->f", up, X.double().numpy()), float(up.sum())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(24, 100, 136), (6, 1000, 24)], ids=lambda s: "%dx%dx%d" % s)
def test_listwise_fused_linear_step(shape, mode):
    """FusedLinearLoss' one-launch step (ltr_linear_listwise_plan == 1 at both shapes) for ListNet, ListMLE and
    ListMLE(k = 10): bounds of tests/test_gpu_linear_listwise.py (_close_loss / the row checks)."""
    from pytorchltr_amd import _C
    from pytorchltr_amd.fused import FusedLinearLoss, linear_loss_step
    from pytorchltr_amd.loss import ListMLELoss, ListwiseSoftmaxLoss
    dev = _dev()
    B, L, F = shape
    X, W, b, y, n, fl = _batch(B, L, F, mode)
    Xd, Wd, bd, yd, nd = X.to(dev), W.to(dev), b.to(dev), y.to(dev), n.to(dev)
    for name, k, obj in (("listnet", None, ListwiseSoftmaxLoss()), ("listmle", None, ListMLELoss()),
                         ("listmle", 10, ListMLELoss(k=10))):
        assert _C.lib().ltr_linear_listwise_plan(0 if name == "listnet" else 1, B, L, F) == 1
        lossv, dW, db = linear_loss_step(Xd, Wd, bd, yd, nd, loss=obj)
        want_l, want_dW, want_db = _listwise_reference(name, k, X, y, n)
        got_l = lossv.cpu().numpy().astype(np.float64)
        if name == "listnet":
            np.testing.assert_allclose(got_l, want_l, rtol=1e-5, atol=2e-6)
        else:
            np.testing.assert_allclose(got_l, want_l, rtol=1e-4, atol=1e-4)
        tol = 1e-5 * max(1.0, float(np.abs(want_dW).max()))
        np.testing.assert_allclose(dW.cpu().numpy(), want_dW, rtol=1e-4, atol=tol)
        np.testing.assert_allclose(db.cpu().numpy(), [want_db], rtol=1e-4, atol=tol)
        assert not got_l[rows_of(fl, ("n0",))].any()
        # the module: the same launch under autograd, `.mean().backward()`
        m = FusedLinearLoss(F, loss=obj).to(dev)
        with torch.no_grad():
            m.weight.copy_(W.reshape(1, F))
            m.bias.copy_(b)
        out = m(Xd, yd, nd)
        out.mean().backward()
        assert torch.equal(out.detach(), lossv)
        np.testing.assert_allclose(m.weight.grad.cpu().numpy().reshape(-1), want_dW, rtol=1e-4, atol=tol)
        np.testing.assert_allclose(m.bias.grad.cpu().numpy().reshape(-1), [want_db], rtol=1e-4, atol=tol)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layout", ["tile", "wide"])
def test_listwise_fused_mlp_step(layout, mode):
    """mlp_loss_step with ListNet / ListMLE in the loss slot at 24 x 100 x 136, both layouts, against the fp64 reference
    of tests/test_gpu_mlp_listwise.py (network in float64, oracle loss and d loss / d s, autograd) and its _compare."""
    from pytorchltr_amd import fused
    from pytorchltr_amd.fused import _ListwiseKind
    from pytorchltr_amd.loss import ListMLELoss
    from pytorchltr_amd import _C
    from tests.test_gpu_mlp import _mlp_params
    from tests.test_gpu_mlp_listwise import _Layout, _compare, _loss64, _network64, _step
    from pytorchltr_amd.utils import tie_breaking
    B, L, F = 24, 100, 136
    X, W, b, y, n, fl = _batch(B, L, F, mode)
    params = [p.numpy() for p in _mlp_params(F, 50, 10, 77)]
    Xn, yn, nn_ = X.numpy(), y.numpy(), n.numpy()
    real = np.arange(L)[None, :] < nn_[:, None]
    for loss, k in (("listnet", None), ("listmle", None), ("listmle", 10)):
        code = _C.LISTWISE_LISTMLE if loss == "listmle" else _C.LISTWISE_LISTNET
        assert fused.mlp_listwise_supported(_ListwiseKind(code, k), B, L, F, 50, 10)
        s, leaves = _network64(Xn, params)
        want_l, ds = _loss64(loss, s.detach().numpy(), yn, nn_, k)
        up = np.where(real, ds, 0.0) / B
        s.backward(torch.from_numpy(up))
        want = (want_l, s.detach().numpy(), [t.grad.numpy() for t in leaves], float(np.abs(up).sum()))
        with _Layout(layout), tie_breaking("index"):
            got = _step(loss, Xn, yn, nn_, params, k=k)
            # FusedMLPListwiseLoss: the reduced loss and the six .grad of the same launch under autograd
            m = fused.FusedMLPListwiseLoss(F, loss=ListMLELoss(k) if k else loss, hidden=(50, 10)).to(_dev())
            with torch.no_grad():
                for prm, value in zip(m.parameters(), params):
                    prm.copy_(torch.from_numpy(value))
            out = m(X.to(_dev()), y.to(_dev()), n.to(_dev()))
            out.backward()
        _compare(loss, got, want, nn_, L)
        assert [tuple(t.shape) for t in m.parameters()] == [t.shape for t in params]
        assert torch.allclose(out.detach(), got[0].mean(), rtol=1e-6, atol=1e-7)
        for prm, g in zip(m.parameters(), got[1]):
            assert torch.allclose(prm.grad.reshape(-1), g.reshape(-1), rtol=1e-6, atol=1e-7 * max(1.0, float(g.abs().max())))


# ---------------------------------------------------------------------------------------------------------------------
# the metrics
# ---------------------------------------------------------------------------------------------------------------------
def _plain_metrics(ts, ty, tn, forced):
    """ndcg@10, dcg@10, arp and the last column of the ndcg / dcg curves from ndcg(), dcg() and arp().  Under the forced
    sort path: from their entry points, with the sort workspace the wrappers do not size for lists that the one-workgroup
    kernels take."""
    import pytorchltr_amd.evaluation as ev
    from pytorchltr_amd import _C
    if not forced:
        return {"ndcg@10": ev.ndcg(ts, ty, tn, k=10), "dcg@10": ev.dcg(ts, ty, tn, k=10), "arp": ev.arp(ts, ty, tn),
                "ndcg": ev.ndcg(ts, ty, tn)[:, -1], "dcg": ev.dcg(ts, ty, tn)[:, -1]}
    lib = _C.lib()
    B, L = ts.shape
    st = _C.stream_of(ts)

    def run(op, k=0, normalize=0):
        nbytes = int(lib.ltr_sort_workspace_bytes(op, B, L))
        assert nbytes > 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device=ts.device)
        out = torch.empty((B,) if (k or op == 2) else (B, L), dtype=torch.float32, device=ts.device)
        if op == 1:
            _C.check(lib.ltr_dcg_long_f32(_C.ptr(ts), _C.ptr(ty), _C.label_dtype(ty), _C.ptr(tn), None, 0, 0, None, B, L, k, 1,
                                          normalize, _C.ptr(out), _C.ptr(ws), nbytes, st))
        else:
            _C.check(lib.ltr_arp_long_f32(_C.ptr(ts), _C.ptr(ty), _C.label_dtype(ty), _C.ptr(tn), None, 0, 0, None, B, L,
                                          _C.ptr(out), _C.ptr(ws), nbytes, st))
        torch.cuda.synchronize()
        return out
    return {"ndcg@10": run(1, 10, 1), "dcg@10": run(1, 10, 0), "arp": run(2), "ndcg": run(1, 0, 1)[:, -1], "dcg": run(1, 0, 0)[:, -1]}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L,sort_path", [(37, False), (37, True), (1000, False), (1000, True), (5000, False)])
def test_metrics(L, sort_path, mode):
    """ndcg, dcg, arp and every metric of evaluate() on the degenerate labels against tests/test_eval_host.py's oracle:
    one workgroup per query, the forced sort path (ltr_debug_long_sort_all), and 5000 documents, where the sort path
    is the only one.  Rows without a relevant real document: MAP, MRR, P, recall and ERR exactly 0; `zero` rows: NDCG
    exactly 0 (maxDCG == 0 -> 1 under a zero DCG); dcg counts padded labels -- `zero_real_pad_nonzero` has a DCG."""
    import pytorchltr_amd.evaluation as ev
    from pytorchltr_amd import _C
    from pytorchltr_amd.utils import tie_breaking
    from tests.test_eval_host import oracle, oracle_ranking
    from tests.test_gpu_eval import ALL, NEW, _check
    dev = _dev()
    B = 24 if L <= 1000 else 12
    X, W, b, y, n, fl = _batch(B, L, 1, mode)
    s = exact_scores(X).astype(np.float32)
    yn, nn_ = y.numpy(), n.numpy()
    ranking = oracle_ranking(s, nn_)
    ts, tn = torch.from_numpy(s).to(dev), n.to(dev)
    lib = _C.lib()
    assert (L > _C.max_list_len()) == (L == 5000)
    prev = lib.ltr_debug_long_sort_all(1) if sort_path else None
    try:
        for labels in (("int64",) if sort_path else LABELS):
            ty = _batch(B, L, 1, mode, labels)[3].to(dev)
            with tie_breaking("index"):
                out = ev.evaluate(ts, ty, tn, metrics=ALL)
                plain = _plain_metrics(ts, ty, tn, sort_path)
            for name in ALL:
                want = oracle(name, ranking, yn, nn_)
                _check(out[name].cpu().numpy(), want, "L=%d %s %s %s" % (L, name, mode, labels))
                if name in plain:
                    _check(plain[name].cpu().numpy(), want, "L=%d %s() %s %s" % (L, name, mode, labels))
            got = {name: out[name].cpu().numpy() for name in ALL}
            none = rows_of(fl, NO_RELEVANT)
            for name in NEW:
                assert not got[name][none].any(), name
            zero = rows_of(fl, ("zero",))
            for name in ("ndcg@1", "ndcg@10", "ndcg"):
                assert not got[name][zero].any(), name
            assert not plain["ndcg@10"].cpu().numpy()[zero].any() and not plain["ndcg"].cpu().numpy()[zero].any()
            # (padded labels count in dcg: the real documents of this flavour, all 0, fill the first ten ranks)
            pad = rows_of(fl, ("zero_real_pad_nonzero",))
            assert np.all(got["dcg"][pad] > 1.0) and not got["dcg@10"][pad].any() and not got["arp"][pad].any()
    finally:
        if sort_path:
            lib.ltr_debug_long_sort_all(prev)
