"""GPU tier of the Linear(F, 1) scorer on bf16 feature batches (include/ltr_linear_bf16.h): the streaming score and
weight-gradient kernels, the fused register-tile step, the routes of the modules, capture and replay, the bf16 collate.

Reference for every value: the fp64 oracle (oracle.ltr_oracle.linear_pairwise; torch float64 on the CPU for the plain
scorer) on ``X.bfloat16().double()`` -- the exact input: bf16 -> fp32 is exact, W stays fp32, every product and sum is
fp32, so the kernels compute the fp32 network on those values up to summation order.  Tolerances are the project's own:
tests/test_gpu_scorer.py's for the scorer (scores rtol 1e-5, atol 2e-6 sqrt(F); dW rtol 1e-4, atol 1e-5 max(1, max|dW|);
db atol 1e-4 max(1, |db|)), tests/test_gpu_fused.py::_check's for the fused step (scores rtol 1e-5 / atol 1e-5 on real
documents; loss rtol 2e-5 -- 5e-4 past 256 documents --, atol 1e-5; |dW - want|, |db - want| < 2e-5 max(1, max|dW|),
x 10 past 256 documents).
Hinge kinds: `_oracle` asserts on the CPU, from the oracle's fp64 scores, that no real pair with y_i > y_j lies within
1e-5 of the margin (one flipped pair moves dW by go (x_i - x_j)).  LambdaNDCG kinds: losses through
tests.conftest.assert_rank_dependent_losses on X.bfloat16().float()."""
import functools

import numpy as np
import pytest
import torch

from oracle import ltr_oracle as O
from tests.conftest import assert_rank_dependent_losses

pytestmark = pytest.mark.gpu
KINDS = list(O.KINDS)


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _module(kind, sigma=1.0, **kw):
    from pytorchltr_amd import loss as L_
    mod = {"hinge": L_.PairwiseHingeLoss, "dcg_hinge": L_.PairwiseDCGHingeLoss, "logistic": L_.PairwiseLogisticLoss,
           "arp1": L_.LambdaARPLoss1, "arp2": L_.LambdaARPLoss2, "ndcg1": L_.LambdaNDCGLoss1, "ndcg2": L_.LambdaNDCGLoss2}[kind]
    return mod(**kw) if kind in ("hinge", "dcg_hinge") else mod(sigma, **kw)


@functools.lru_cache(maxsize=None)
def _batch(B, L, F, seed, lengths="ragged", wscale=1.0):
    """A synthetic batch whose features are bf16 values: (X16 bf16, X32 = the same values as fp32, W, b, y, n).  Cached
    and shared: never written to.  lengths: "ragged" (n ~ U[1, L]; n[0] = 0 from five queries on), "full", or a tuple.
    wscale: W is nn.Linear's initial range times this (the lists of thousands of documents: millions of pairs, of which
    some always lie within 1e-5 of the hinge margin at the initial range; far-spread scores thin them out)."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, 5, (B, L), generator=g)
    n = torch.randint(1, L + 1, (B,), generator=g)
    X16 = torch.randn(B, L, F, generator=g).bfloat16()
    bound = 1.0 / (F ** 0.5)
    W = (torch.rand(F, generator=g) * 2 - 1) * bound * wscale
    b = (torch.rand(1, generator=g) * 2 - 1) * bound
    if lengths == "full":
        n = torch.full_like(n, L)
    elif lengths != "ragged":
        n = torch.tensor(lengths, dtype=torch.int64)
    elif B >= 5:
        n[0] = 0
    return X16, X16.float(), W, b, y, n


def _margin_clear(want_s, y, n):
    """No real pair with y_i > y_j within 1e-5 of the hinge margin: min over those pairs of |1 - (s_i - s_j)|."""
    worst = np.inf
    yy = y.numpy()
    for r in range(want_s.shape[0]):
        nr = int(min(max(int(n[r]), 0), want_s.shape[1]))
        if nr < 2:
            continue
        s, lab = want_s[r, :nr], yy[r, :nr]
        d = np.abs(1.0 - (s[:, None] - s[None, :]))[lab[:, None] > lab[None, :]]
        if d.size:
            worst = min(worst, float(d.min()))
    return worst


@functools.lru_cache(maxsize=None)
def _oracle(kind, B, L, F, seed, lengths="ragged", sigma=1.0, go="mean", wscale=1.0):
    """(loss, scores, dW, db, grad_out) of the fp64 oracle on the bf16 values; hinge kinds: the margin condition."""
    X16, X32, W, b, y, n = _batch(B, L, F, seed, lengths, wscale)
    gout = np.full(B, 1.0 / max(B, 1)) if go == "mean" else (np.arange(B, dtype=np.float64) % 5 - 1.5) / 3.0
    want = O.linear_pairwise(kind, X16.double().numpy(), W.numpy(), float(b[0]), y.numpy(), n.numpy(), gout, sigma=sigma)
    if kind in ("hinge", "dcg_hinge"):
        clear = _margin_clear(want[1], y, n)
        assert clear > 1e-5, "seed %d puts a pair %.3g from the margin: pick another" % (seed, clear)
    return want + (gout,)


def _assert_step(kind, got, B, L, F, seed, lengths="ragged", sigma=1.0, go="mean", scores=None, what="", wscale=1.0):
    """loss, dW, db (and scores) of a step against the oracle at tests/test_gpu_fused.py::_check's tolerances."""
    X16, X32, W, b, y, n = _batch(B, L, F, seed, lengths, wscale)
    want_l, want_s, want_dW, want_db, _ = _oracle(kind, B, L, F, seed, lengths, sigma, go, wscale)
    loss, dW, db = (np.asarray(t.detach().cpu().numpy(), dtype=np.float64).reshape(-1) for t in got)
    assert dW.shape == (F,) and db.shape == (1,) and loss.shape == (B,)
    long = L > 256
    rtol = 5e-4 if long else 2e-5
    tol = 2e-5 * max(1.0, float(np.max(np.abs(want_dW)))) * (10 if long else 1)
    err_l = float(np.max(np.abs(loss - want_l) - rtol * np.abs(want_l))) if B else 0.0
    print("%s %s %dx%dx%d: loss excess %.3g (atol 1e-5), dW err %.3g, db err %.3g (tol %.3g)" % (
        what, kind, B, L, F, err_l, float(np.max(np.abs(dW - want_dW))), abs(db[0] - want_db), tol))
    if scores is not None:
        real = np.arange(L)[None, :] < np.clip(n.numpy(), 0, L)[:, None]
        sc = scores.detach().cpu().numpy().reshape(B, L)
        assert scores.dtype is torch.float32
        assert np.allclose(sc[real], want_s[real], rtol=1e-5, atol=1e-5), (what, kind)
        assert np.all(sc[~real] == 0.0), (what, kind)
    if kind in ("ndcg1", "ndcg2"):
        assert_rank_dependent_losses(kind, loss, X32, W, b, y, n, want_l, want_s, rtol=rtol, sigma=sigma)
    else:
        assert np.allclose(loss, want_l, rtol=rtol, atol=1e-5), (what, kind)
    assert np.max(np.abs(dW - want_dW)) < tol, (what, kind)
    assert abs(db[0] - want_db) < tol, (what, kind)


def _on_plan(kind, B, L, F):
    from pytorchltr_amd import _C
    return _C.lib().ltr_linear_bf16_plan(O.KINDS[kind], B, L, F) == 1


# ---------------------------------------------------------------------------------------------
# 1. the streaming kernels, through LinearScorer
# ---------------------------------------------------------------------------------------------
STREAM = [(1, 1, 8, "ragged"), (8, 16, 8, "ragged"), (5, 33, 136, (0, 1, 33, 38, 17)), (7, 33, 136, None),
          (3, 1000, 224, "ragged"), (5, 77, 704, "ragged"), (2, 9, 1024, "ragged"), (300, 20, 48, "ragged"),
          (3, 300, 24, (0, 129, 300))]


@pytest.mark.parametrize("shape", STREAM, ids=lambda s: "%dx%dx%d-%s" % (s[0], s[1], s[2], "n" if s[3] else "none"))
def test_streaming_kernels_through_linear_scorer(shape):
    from pytorchltr_amd.fused import LazyScores, LinearScorer
    B, L, F, lengths = shape
    dev = _dev()
    X16, X32, W, b, y, n = _batch(B, L, F, 4000 + L + F, "ragged" if lengths is None else lengths)
    nn = None if lengths is None else n
    g = torch.Generator().manual_seed(B + L)
    gs = torch.randn(B, L, generator=g)
    # torch float64 on the CPU
    wd = W.double().requires_grad_(True)
    bd = b.double().requires_grad_(True)
    real = torch.ones(B, L, dtype=torch.bool) if nn is None else torch.arange(L)[None, :] < nn.clamp(0, L)[:, None]
    sd = torch.where(real, X16.double() @ wd + bd, torch.zeros((), dtype=torch.float64))
    (sd * gs.double()).sum().backward()
    want_s, want_dW, want_db = sd.detach().numpy(), wd.grad.numpy(), float(bd.grad[0])

    sc = LinearScorer(F).to(dev)
    with torch.no_grad():
        sc.weight.copy_(W.reshape(1, F))
        sc.bias.copy_(b)
    xs = X16.to(dev)
    with torch.no_grad():
        s0 = sc(xs, None if nn is None else nn.to(dev))
    assert not isinstance(s0, LazyScores) and s0.dtype is torch.float32 and s0.shape == (B, L, 1)
    got = s0.squeeze(-1).cpu().numpy()
    assert np.allclose(got[real.numpy()], want_s[real.numpy()], rtol=1e-5, atol=2e-6 * F ** 0.5)
    assert np.all(got[~real.numpy()] == 0.0)                        # padded scores exactly 0
    s1 = sc(xs, None if nn is None else nn.to(dev))                 # lazy while gradients are enabled
    assert isinstance(s1, LazyScores)
    (s1.squeeze(-1) * gs.to(dev)).sum().backward()
    assert sc.weight.grad.dtype is torch.float32 and sc.weight.grad.shape == (1, F)
    dW = sc.weight.grad.cpu().numpy().reshape(-1).astype(np.float64)
    assert np.allclose(dW, want_dW, rtol=1e-4, atol=1e-5 * max(1.0, float(np.abs(want_dW).max())))
    assert abs(float(sc.bias.grad[0]) - want_db) <= 1e-4 * max(1.0, abs(want_db))
    assert torch.equal(s1.materialize().detach(), s0)               # and they are the streaming kernel's scores


# ---------------------------------------------------------------------------------------------
# 2. padding is not read; determinism
# ---------------------------------------------------------------------------------------------
def _partial_rows(kind, xs, W, b, y, n):
    """loss and the raw partial rows of ltr_linear_partials_bf16."""
    from pytorchltr_amd import _C
    B, L, F = xs.shape
    lib = _C.lib()
    loss = torch.empty(B, dtype=torch.float32, device=xs.device)
    ws = torch.zeros(lib.ltr_linear_workspace_bytes(B, L, F) // 4, dtype=torch.float32, device=xs.device)
    _C.check(lib.ltr_linear_partials_bf16(O.KINDS[kind], 1.0, _C.ptr(xs), _C.ptr(W), _C.ptr(b), _C.ptr(y), _C.label_dtype(y),
                                          _C.ptr(n), B, L, F, _C.ptr(loss), None, _C.ptr(ws), _C.stream_of(xs)))
    return loss, ws[:B * (F + 4)].clone()


def test_padding_is_not_read_and_runs_are_bit_identical():
    from pytorchltr_amd.fused import _LinearScoreFunction, linear_loss_step
    dev = _dev()
    B, L, F = 50, 64, 136
    X16, X32, W, b, y, n = _batch(B, L, F, 31)
    assert int(n.min()) == 0 and int((n < L).sum()) > 10
    pad = (torch.arange(L)[None, :] >= n[:, None])
    dirty = X16.clone()
    dirty[pad] = float("nan")
    g = torch.randn(B, L, generator=torch.Generator().manual_seed(5))
    gdirty = g.clone()
    gdirty[pad] = float("nan")
    Wd, bd, yd, nd = W.to(dev), b.to(dev), y.to(dev), n.to(dev)

    def pieces(xs, gs):
        w = Wd.clone().reshape(1, F).requires_grad_(True)
        bb = bd.clone().requires_grad_(True)
        s = _LinearScoreFunction.apply(xs, w, bb, nd)
        (s.squeeze(-1) * gs).sum().backward()
        return s.detach(), w.grad, bb.grad

    runs = [pieces(X16.to(dev), g.to(dev)), pieces(X16.to(dev), g.to(dev)), pieces(dirty.to(dev), gdirty.to(dev))]
    for other in runs[1:]:
        for a, c in zip(runs[0], other):
            assert torch.equal(a, c) and bool(torch.isfinite(a).all())
    for kind in ("hinge", "logistic", "ndcg2"):
        assert _on_plan(kind, B, L, F)
        fused = [linear_loss_step(x.to(dev), Wd, bd, yd, nd, loss=kind, return_scores=True) for x in (X16, X16, dirty)]
        rows = [_partial_rows(kind, x.to(dev), Wd, bd, yd, nd) for x in (X16, X16, dirty)]
        for other, orow in zip(fused[1:], rows[1:]):
            for a, c in zip(fused[0] + rows[0], other + orow):
                assert torch.equal(a, c) and bool(torch.isfinite(a).all()), kind
        # the partial rows: [dW row | d bias | zeros], a query without documents a row of zeros
        r = rows[0][1].reshape(B, F + 4)
        assert bool((r[:, F + 1:] == 0).all()) and bool((r[0] == 0).all())


# ---------------------------------------------------------------------------------------------
# 3. the fused step, every kind
# ---------------------------------------------------------------------------------------------
FUSED = [(3, 1, 8, "ragged"), (4, 2, 8, "ragged"), (5, 33, 136, (0, 1, 33, 38, 17)), (6, 64, 64, "ragged"),
         (6, 65, 136, "ragged"), (4, 128, 136, "full"), (3, 256, 224, "ragged"), (3, 128, 512, "ragged"),
         (3000, 8, 8, "ragged"),
         # one shape per sweep-count instantiation at its largest tile: 5 sweeps of 30 rows, 10 of 25, 16 of 16 / of 8
         (2, 150, 136, "full"), (2, 250, 160, "full"), (2, 256, 256, "full"), (2, 128, 504, "full")]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", FUSED, ids=lambda s: "%dx%dx%d" % s[:3])
def test_fused_step_every_kind(shape, kind):
    from pytorchltr_amd.fused import linear_loss_step
    B, L, F, lengths = shape
    dev = _dev()
    seed = 7000 + B + L + F
    assert _on_plan(kind, B, L, F)                                  # (the test cannot silently run the pieces)
    X16, X32, W, b, y, n = _batch(B, L, F, seed, lengths)
    args = (X16.to(dev), W.to(dev), b.to(dev), y.to(dev), n.to(dev))
    loss, dW, db, scores = linear_loss_step(*args, loss=kind, return_scores=True)
    _assert_step(kind, (loss, dW, db), B, L, F, seed, lengths, scores=scores, what="scores")
    out = linear_loss_step(*args, loss=kind)
    _assert_step(kind, out, B, L, F, seed, lengths, what="plain")
    assert all(torch.equal(a, c) for a, c in zip(out, (loss, dW, db)))


@pytest.mark.parametrize("kind", KINDS)
def test_fused_step_non_uniform_grad_out(kind):
    from pytorchltr_amd.fused import linear_loss_step
    B, L, F, seed = 37, 50, 136, 811
    dev = _dev()
    assert _on_plan(kind, B, L, F)
    X16, X32, W, b, y, n = _batch(B, L, F, seed)
    go = torch.from_numpy(_oracle(kind, B, L, F, seed, go="ramp")[4]).float()
    out = linear_loss_step(X16.to(dev), W.to(dev), b.to(dev), y.to(dev), n.to(dev), loss=kind, grad_out=go.to(dev),
                           return_loss_sum=True)
    _assert_step(kind, out[:3], B, L, F, seed, go="ramp", what="grad_out")
    assert float(out[3][0]) == pytest.approx(float(out[0].sum()), rel=1e-5)


@pytest.mark.parametrize("kind", ["logistic", "ndcg2"])
def test_fused_step_sigma_2(kind):
    from pytorchltr_amd.fused import linear_loss_step
    B, L, F, seed = 9, 100, 136, 812
    dev = _dev()
    assert _on_plan(kind, B, L, F)
    X16, X32, W, b, y, n = _batch(B, L, F, seed)
    out = linear_loss_step(X16.to(dev), W.to(dev), b.to(dev), y.to(dev), n.to(dev), loss=_module(kind, 2.0))
    _assert_step(kind, out, B, L, F, seed, sigma=2.0, what="sigma 2")


# ---------------------------------------------------------------------------------------------
# 4. the edges of the plan: the last shape on it (the fused launch), the first off it (the pieces)
# ---------------------------------------------------------------------------------------------
EDGES = [("hinge", 3, 256, 136, True), ("hinge", 3, 257, 136, False), ("ndcg2", 3, 257, 136, False),
         ("hinge", 2, 80, 704, True), ("logistic", 2, 81, 704, False), ("hinge", 2, 300, 704, False),
         ("hinge", 2, 64, 1024, True), ("arp2", 2, 65, 1024, False), ("hinge", 2, 1000, 224, False)]


@pytest.mark.parametrize("case", EDGES, ids=lambda c: "%s-%dx%dx%d" % c[:4])
def test_plan_edges_reach_the_fused_launch_or_the_pieces(case):
    from pytorchltr_amd import fused
    kind, B, L, F, on = case
    dev = _dev()
    seed = 9001 + L + F
    assert _on_plan(kind, B, L, F) == on
    X16, X32, W, b, y, n = _batch(B, L, F, seed)
    xs, yd, nd = X16.to(dev), y.to(dev), n.to(dev)
    assert fused._linear_route_of("step", xs, O.KINDS[kind]) == (fused._LIN_BF16_FUSED if on else fused._LIN_BF16_PIECES)
    loss, dW, db, scores = fused.linear_loss_step(xs, W.to(dev), b.to(dev), yd, nd, loss=kind, return_scores=True)
    _assert_step(kind, (loss, dW, db), B, L, F, seed, scores=scores, what="linear_loss_step")
    m = fused.FusedLinearLoss(F, loss=kind).to(dev)
    with torch.no_grad():
        m.weight.copy_(W.reshape(1, F))
        m.bias.copy_(b)
    out = m(xs, yd, nd)
    out.mean().backward()
    _assert_step(kind, (out, m.weight.grad, m.bias.grad), B, L, F, seed, what="FusedLinearLoss")


def test_long_lists_past_4096_documents():
    from pytorchltr_amd import fused
    B, L, F, seed, wscale = 2, 4100, 8, 79, 100.0       # (far-spread scores: no pair of the millions at the margin)
    dev = _dev()
    lengths = (L, L // 3)
    X16, X32, W, b, y, n = _batch(B, L, F, seed, lengths, wscale)
    xs, yd, nd = X16.to(dev), y.to(dev), n.to(dev)
    long_hinge = _module("hinge", long_lists=True)
    out = fused.linear_loss_step(xs, W.to(dev), b.to(dev), yd, nd, loss=long_hinge)
    _assert_step("hinge", out, B, L, F, seed, lengths, what="linear_loss_step", wscale=wscale)
    m = fused.FusedLinearLoss(F, loss=long_hinge).to(dev)
    sc = fused.LinearScorer(F).to(dev)
    with torch.no_grad():
        for mod in (m, sc):
            mod.weight.copy_(W.reshape(1, F))
            mod.bias.copy_(b)
    loss = m(xs, yd, nd)
    loss.mean().backward()
    _assert_step("hinge", (loss, m.weight.grad, m.bias.grad), B, L, F, seed, lengths, what="FusedLinearLoss", wscale=wscale)
    loss = long_hinge(sc(xs, nd), yd, nd)
    loss.mean().backward()
    _assert_step("hinge", (loss, sc.weight.grad, sc.bias.grad), B, L, F, seed, lengths, what="LinearScorer + module", wscale=wscale)


# ---------------------------------------------------------------------------------------------
# 5. feature counts that are not a multiple of 8, through the modules
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [5, 46, 220])
def test_odd_feature_counts_are_padded_once_and_cropped(F):
    from pytorchltr_amd import fused
    B, L, seed, kind = 6, 40, 600 + F, "logistic"
    dev = _dev()
    X16, X32, W, b, y, n = _batch(B, L, F, seed)
    xs, yd, nd = X16.to(dev), y.to(dev), n.to(dev)
    X8 = fused._prepare_features(xs, bf16=True)
    assert X8.dtype is torch.bfloat16 and X8.shape == (B, L, (F + 7) & ~7) and X8.is_contiguous()
    assert torch.equal(X8[:, :, :F], xs) and bool((X8[:, :, F:] == 0).all())
    assert fused._linear_route_of("step", xs, O.KINDS[kind]) == fused._LIN_BF16_FUSED
    out = fused.linear_loss_step(xs, W.to(dev), b.to(dev), yd, nd, loss=kind)
    _assert_step(kind, out, B, L, F, seed, what="linear_loss_step")
    m = fused.FusedLinearLoss(F, loss=kind).to(dev)
    sc = fused.LinearScorer(F).to(dev)
    with torch.no_grad():
        for mod in (m, sc):
            mod.weight.copy_(W.reshape(1, F))
            mod.bias.copy_(b)
    loss = m(xs, yd, nd)
    loss.mean().backward()
    assert m.weight.grad.shape == (1, F)
    _assert_step(kind, (loss, m.weight.grad, m.bias.grad), B, L, F, seed, what="FusedLinearLoss")
    loss = _module(kind)(sc(xs, nd), yd, nd)
    loss.mean().backward()
    assert sc.weight.grad.shape == (1, F)
    _assert_step(kind, (loss, sc.weight.grad, sc.bias.grad), B, L, F, seed, what="LinearScorer + module")
    # the scorer alone, on the padded copy as well
    with torch.no_grad():
        s = sc(xs, nd).squeeze(-1)
    want_s = _oracle(kind, B, L, F, seed)[1]
    real = (torch.arange(L)[None, :] < n[:, None]).numpy()
    assert np.allclose(s.cpu().numpy()[real], want_s[real], rtol=1e-5, atol=2e-6 * F ** 0.5)


# ---------------------------------------------------------------------------------------------
# 6. drop-in
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hinge", "logistic", "ndcg2"])
def test_drop_in_composition(kind):
    from pytorchltr_amd import fused
    from pytorchltr_amd.evaluation import ndcg
    B, L, F, seed = 40, 60, 136, 1300
    dev = _dev()
    X16, X32, W, b, y, n = _batch(B, L, F, seed)
    xs, yd, nd = X16.to(dev), y.to(dev), n.to(dev)
    loss_fn = _module(kind)
    lin = torch.nn.Linear(F, 1).to(dev)
    keys = {k: v.dtype for k, v in lin.state_dict().items()}
    with torch.no_grad():
        lin.weight.copy_(W.reshape(1, F))
        lin.bias.copy_(b)
    with pytest.raises(RuntimeError):                               # what nn.Linear itself says to a bf16 batch
        lin(xs)
    model = fused.use_linear_scorer(lin)
    scores = model(xs, nd)
    assert isinstance(scores, fused.LazyScores)
    loss = loss_fn(scores, yd, nd)
    loss.mean().backward()
    assert model.weight.grad.dtype is torch.float32 and model.bias.grad.dtype is torch.float32
    assert model.weight.dtype is torch.float32
    assert {k: v.dtype for k, v in model.state_dict().items()} == keys
    _assert_step(kind, (loss, model.weight.grad, model.bias.grad), B, L, F, seed, what="use_linear_scorer")
    direct = fused.LinearScorer(F).to(dev)
    m = fused.FusedLinearLoss(F, loss=loss_fn).to(dev)
    with torch.no_grad():
        for mod in (direct, m):
            mod.weight.copy_(W.reshape(1, F))
            mod.bias.copy_(b)
    loss = loss_fn(direct(xs, nd), yd, nd)
    loss.mean().backward()
    _assert_step(kind, (loss, direct.weight.grad, direct.bias.grad), B, L, F, seed, what="LinearScorer")
    loss = m(xs, yd, nd)
    loss.mean().backward()
    _assert_step(kind, (loss, m.weight.grad, m.bias.grad), B, L, F, seed, what="FusedLinearLoss")
    # a metric on the lazy scores: the streaming kernel's scores
    lazy = direct(xs, nd)
    with torch.no_grad():
        plain = direct(xs, nd)
    assert torch.equal(ndcg(lazy, yd, nd, k=10), ndcg(plain, yd, nd, k=10))
    assert torch.equal(lazy.materialize().detach(), plain)


def test_three_sgd_steps_match_torch_sgd_on_the_fp32_values():
    from pytorchltr_amd import fused
    from pytorchltr_amd.optim import SGD
    B, L, F, lr = 32, 50, 136, 0.05
    dev = _dev()
    loss_fn = _module("logistic")
    data = [_batch(B, L, F, 1400 + i) for i in range(3)]
    torch.manual_seed(11)
    lin = torch.nn.Linear(F, 1).to(dev)
    ref = torch.nn.Linear(F, 1).to(dev)
    ref.load_state_dict(lin.state_dict())
    model = fused.use_linear_scorer(lin)
    opt, opt_ref = SGD(model.parameters(), lr=lr), torch.optim.SGD(ref.parameters(), lr=lr)
    worst = 0.0
    for X16, X32, W, b, y, n in data:
        loss = loss_fn(model(X16.to(dev), n.to(dev)), y.to(dev), n.to(dev)).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        loss_ref = loss_fn(ref(X32.to(dev)), y.to(dev), n.to(dev)).mean()
        opt_ref.zero_grad()
        loss_ref.backward()
        opt_ref.step()
        worst = max(worst, float(ref.weight.grad.abs().max()))
    # the dW tolerance x lr per step
    tol = 3 * lr * 2e-5 * max(1.0, worst)
    assert float((model.weight.detach() - ref.weight.detach()).abs().max()) < tol
    assert float((model.bias.detach() - ref.bias.detach()).abs().max()) < tol


# ---------------------------------------------------------------------------------------------
# 7. capture and replay
# ---------------------------------------------------------------------------------------------
def test_capture_and_replay():
    from pytorchltr_amd.fused import linear_loss_step
    B, L, F = 64, 100, 136
    dev = _dev()
    assert _on_plan("logistic", B, L, F)
    batches = [_batch(B, L, F, 1500 + i) for i in range(3)]
    xs, W, b = batches[0][0].to(dev), batches[0][2].to(dev), batches[0][3].to(dev)
    y, n = batches[0][4].to(dev), batches[0][5].to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                   # warm-up off the capture: caches, LDS attributes
        linear_loss_step(xs, W, b, y, n, loss="logistic")
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                   # one stream, no parallel branches
        out = linear_loss_step(xs, W, b, y, n, loss="logistic")
    for X16, X32, W2, b2, y2, n2 in batches[1:]:
        xs.copy_(X16.to(dev)); W.copy_(W2.to(dev)); b.copy_(b2.to(dev)); y.copy_(y2.to(dev)); n.copy_(n2.to(dev))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in out]
        eager = linear_loss_step(xs, W, b, y, n, loss="logistic")
        assert all(torch.equal(a, c) for a, c in zip(got, eager))


# ---------------------------------------------------------------------------------------------
# 8. collate
# ---------------------------------------------------------------------------------------------
def _split(F, seed=3):
    g = torch.Generator().manual_seed(seed)
    counts = torch.tensor([3, 17, 1, 40, 8, 25, 12])
    off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(counts, 0)])
    N = int(off[-1])
    x = torch.randn(N, F, generator=g).bfloat16().float()           # bf16-representable values
    y = torch.randint(0, 5, (N,), generator=g)
    return x, y, off


@pytest.mark.parametrize("F", [5, 136, 220])
@pytest.mark.parametrize("truncate", [None, 10])
def test_bf16_collate_is_the_fp32_collate(F, truncate):
    from pytorchltr_amd.datasets.list_sampler import ListSampler
    from pytorchltr_amd.datasets.ragged import RaggedQueries
    x, y, off = _split(F)
    r32 = RaggedQueries(x, y, off, device="cuda")
    r16 = RaggedQueries(x, y, off, device="cuda", feature_dtype=torch.bfloat16)
    assert r16.features.dtype is torch.bfloat16 and torch.equal(r16.features.float(), r32.features)
    idx = [3, 0, 5, 2, 6]
    sampler = None if truncate is None else ListSampler(truncate)
    b32, b16 = r32.collate(idx, sampler), r16.collate(idx, sampler)
    assert b16.features.dtype is torch.bfloat16 and b16.features.shape == b32.features.shape
    assert torch.equal(b16.features.float(), b32.features)
    assert torch.equal(b16.relevance, b32.relevance) and torch.equal(b16.n, b32.n) and torch.equal(b16.qid, b32.qid)
    if truncate is not None:
        assert b16.features.shape[1] == truncate


def test_pad_features_to_8_gives_a_marked_view_the_fused_step_takes():
    from pytorchltr_amd import fused
    from pytorchltr_amd.datasets.ragged import RaggedQueries
    F, kind = 220, "hinge"
    x, y, off = _split(F, seed=4)
    r = RaggedQueries(x, y, off, device="cuda", feature_dtype=torch.bfloat16, pad_features_to=8)
    batch = r.collate([1, 3, 5, 4])
    xs = batch.features
    assert xs.shape == (4, 40, F) and xs.dtype is torch.bfloat16 and not xs.is_contiguous()
    assert getattr(xs, "_ltr_zero_padded_rows", False) and xs.stride() == (40 * 224, 224, 1)
    wide = fused._padded_rows(xs)
    assert wide is not None and wide.shape == (4, 40, 224) and wide.data_ptr() == xs.data_ptr()      # no copy
    assert fused._prepare_features(xs, bf16=True).data_ptr() == xs.data_ptr()
    assert bool((wide[:, :, F:] == 0).all())
    g = torch.Generator().manual_seed(9)
    W = (torch.rand(F, generator=g) * 2 - 1) / F ** 0.5
    b = torch.tensor([0.05])
    assert fused._linear_route_of("step", xs, O.KINDS[kind]) == fused._LIN_BF16_FUSED
    loss, dW, db = fused.linear_loss_step(xs, W.cuda(), b.cuda(), batch.relevance, batch.n, loss=kind)
    gout = np.full(4, 0.25)
    want_l, want_s, want_dW, want_db = O.linear_pairwise(kind, xs.cpu().double().numpy(), W.numpy(), float(b[0]),
                                                         batch.relevance.cpu().numpy(), batch.n.cpu().numpy(), gout)
    assert _margin_clear(want_s, batch.relevance.cpu(), batch.n.cpu()) > 1e-5
    tol = 2e-5 * max(1.0, float(np.abs(want_dW).max()))
    assert np.allclose(loss.cpu().numpy(), want_l, rtol=2e-5, atol=1e-5)
    assert dW.shape == (F,) and np.max(np.abs(dW.cpu().numpy() - want_dW)) < tol and abs(float(db[0]) - want_db) < tol
    # a LinearScorer takes the view lazily, like the fp32 one
    sc = fused.LinearScorer(F).cuda()
    assert isinstance(sc(xs, batch.n), fused.LazyScores)


def test_a_csr_split_refuses_bf16():
    from pytorchltr_amd.datasets.ragged import RaggedQueries
    x, y, off = _split(8)
    csr = (torch.arange(x.shape[0] + 1), torch.zeros(x.shape[0], dtype=torch.int32), torch.ones(x.shape[0]))
    assert RaggedQueries(None, y, off, device="cuda", csr=csr).collate([0, 1]).features.dtype is torch.float32
    with pytest.raises(ValueError, match="csr"):
        RaggedQueries(None, y, off, device="cuda", csr=csr, feature_dtype=torch.bfloat16)


# ---------------------------------------------------------------------------------------------
# 9. the empty batch
# ---------------------------------------------------------------------------------------------
def test_empty_batch_through_every_entry_point():
    from pytorchltr_amd import _C, fused
    from pytorchltr_amd.datasets.ragged import RaggedQueries
    dev = _dev()
    L, F = 10, 16
    xs = torch.zeros(0, L, F, dtype=torch.bfloat16, device=dev)
    y = torch.zeros(0, L, dtype=torch.int64, device=dev)
    n = torch.zeros(0, dtype=torch.int64, device=dev)
    W = torch.ones(F, device=dev)
    b = torch.ones(1, device=dev)
    lib = _C.lib()
    out = torch.full((F + 1,), 7.0, device=dev)
    assert lib.ltr_linear_scores_bf16(None, _C.ptr(W), None, None, 0, L, F, None, None) == 0
    assert lib.ltr_linear_grad_workspace_bytes_bf16(0, L, F) == 0
    assert lib.ltr_linear_grad_bf16(None, None, None, 0, L, F, _C.ptr(out), None, 0, _C.stream_of(out)) == 0
    assert bool((out == 0).all())                                   # zero gradients
    assert lib.ltr_linear_partials_bf16(0, 1.0, None, None, None, None, 0, None, 0, L, F, None, None, None, None) == 0
    assert lib.ltr_collate_pad_bf16(None, None, None, None, None, 1, 0, L, F, None, None, None, None) == 0
    loss, dW, db = fused.linear_loss_step(xs, W, b, y, n, loss="hinge")
    assert loss.shape == (0,) and dW.shape == (F,) and bool((dW == 0).all()) and bool((db == 0).all())
    sc = fused.LinearScorer(F).to(dev)
    with torch.no_grad():
        assert sc(xs, n).shape == (0, L, 1)
    s = sc(xs, n)
    s.sum().backward()
    assert bool((sc.weight.grad == 0).all())
    m = fused.FusedLinearLoss(F, loss="logistic").to(dev)
    m(xs, y, n).sum().backward()
    assert bool((m.weight.grad == 0).all())
    x, yy, off = _split(F)
    r = RaggedQueries(x, yy, off, device="cuda", feature_dtype=torch.bfloat16)
    batch = r.collate([])
    assert batch.features.shape[0] == 0 and batch.features.dtype is torch.bfloat16
