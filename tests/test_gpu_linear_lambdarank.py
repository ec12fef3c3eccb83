"""GPU tier of the fused Linear step of LambdaRankLoss (run with `-m gpu` on an MI355X):
ltr_linear_lambdarank_partials_f32 -- scores, LambdaRank row and weight-gradient row in one launch -- against fp64
X.W + b, the stand-alone kernel on its own scores (bit for bit) and fp64 partial rows built from that kernel's
gradient; then FusedLinearLoss, linear_loss_step and the LinearScorer drop-in on top of it.  The tolerances are those
of tests/test_gpu_linear_listwise.py."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import lambdarank_ref as R
from tests.test_gpu_lambdarank import _call as lambdarank_call

pytestmark = pytest.mark.gpu

B = 7
SHAPES = [(L, F) for F in (8, 136, 700) for L in (17, 128, 300, 1000)]


def _dev():
    assert torch.cuda.is_available(), "GPU tier needs a ROCm device"
    return torch.device("cuda:0")


def _data(seed, Bq, L, F):
    """Normal features, normal weights of variance 1 / F (scores N(0, 1) at every width), grades 0..4, n = 0, 1, 2, L,
    then random."""
    rng = np.random.default_rng(seed)
    X = rng.normal(0.0, 1.0, (Bq, L, F)).astype(np.float32)
    W = (rng.normal(0.0, 1.0, F) / np.sqrt(F)).astype(np.float32)
    bias = np.float32(rng.normal())
    y = rng.integers(0, 5, (Bq, L)).astype(np.int64)
    n = rng.integers(0, L + 1, Bq).astype(np.int64)
    for i, v in enumerate((0, 1, 2, L)):
        if i < Bq:
            n[i] = min(v, L)
    return X, W, bias, y, n


def _t(*arrays):
    return [torch.from_numpy(np.asarray(a)).to(_dev()) for a in arrays]


@functools.lru_cache(maxsize=None)
def _case(L, F):
    X, W, bias, y, n = _data(1000 * L + F, B, L, F)
    return (X, W, bias, y, n) + tuple(_t(X, W, np.array([bias]), y, n))


def _fused(X, W, bias, y, n, k=None, sigma=1.0, want_scores=True):
    """One ltr_linear_lambdarank_partials_f32 call on device tensors: (loss_out (B), scores_out (B, L) or None,
    partials (B, PF))."""
    from pytorchltr_amd import _C
    lib = _C.lib()
    Bq, L, F = X.shape
    PF = (F + 4) & ~3
    assert lib.ltr_linear_lambdarank_plan(Bq, L, F) == 1
    nbytes = int(lib.ltr_linear_workspace_bytes(Bq, L, F))
    assert nbytes >= 4 * Bq * PF
    ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=X.device)
    out = torch.full((Bq,), float("nan"), dtype=torch.float32, device=X.device)
    sc = torch.full((Bq, L), float("nan"), dtype=torch.float32, device=X.device) if want_scores else None
    _C.check(lib.ltr_linear_lambdarank_partials_f32(
        int(k or 0), float(sigma), _C.ptr(X), _C.ptr(W), _C.ptr(bias), _C.ptr(y), _C.label_dtype(y), _C.ptr(n), Bq, L, F,
        _C.ptr(out), _C.ptr(sc), _C.ptr(ws), _C.stream_of(X)))
    torch.cuda.synchronize()
    return out, sc, ws[:Bq * PF].reshape(Bq, PF).clone()


def _rows_reference(X, g32, n):
    """fp64 [sum_j g32[b, j] X[b, j, :] | sum_j g32[b, j]] over the real documents."""
    L = X.shape[1]
    real = np.arange(L)[None, :] < np.minimum(n, L)[:, None]
    g = np.where(real, g32.astype(np.float64), 0.0)
    Xm = np.where(real[:, :, None], X.astype(np.float64), 0.0)
    return np.concatenate([np.einsum("bl,blf->bf", g, Xm), g.sum(1, keepdims=True)], axis=1)


@pytest.mark.parametrize("k", [None, 10])
@pytest.mark.parametrize("L,F", SHAPES)
def test_scores_loss_and_partial_rows(L, F, k):
    X, W, bias, y, n, tX, tW, tb, ty, tn = _case(L, F)
    sigma = 2.5 if k else 1.0
    out, sc, part = _fused(tX, tW, tb, ty, tn, k=k, sigma=sigma)
    # the scores
    want_s = X.astype(np.float64) @ W.astype(np.float64) + np.float64(bias)
    real = np.arange(L)[None, :] < np.minimum(n, L)[:, None]
    got_s = sc.cpu().numpy()
    assert np.all(got_s[~real] == 0.0)                                 # padded documents: exactly 0
    np.testing.assert_allclose(got_s[real], want_s[real], rtol=1e-5, atol=1e-5)
    out2, none, part2 = _fused(tX, tW, tb, ty, tn, k=k, sigma=sigma, want_scores=False)
    assert none is None and torch.equal(out, out2) and torch.equal(part, part2)
    # the loss: the stand-alone kernel on these scores, bit for bit (one row function, one launch shape); and so the
    # reference on them, at the stand-alone kernel's tolerance
    loss, g32 = lambdarank_call(sc, ty, tn, k=k, sigma=sigma)
    assert torch.equal(out, loss)
    wl, _ = R.batch(got_s, y, n, k=k, sigma=sigma)
    assert np.all(np.abs(out.cpu().numpy().astype(np.float64) - wl) <= 2e-6 + (1e-5 if L <= 256 else 5e-4) * np.abs(wl))
    # the partial rows
    got = part.cpu().numpy()
    assert np.all(got[:, F + 1:] == 0.0) and np.all(got[n <= 0] == 0.0)
    want = _rows_reference(X, g32.cpu().numpy(), n)
    for b in range(B):
        np.testing.assert_allclose(got[b, :F + 1], want[b], rtol=1e-4, atol=1e-5 * max(1.0, np.abs(want[b]).max()))


def test_padding_is_never_read_and_runs_are_bit_identical():
    L, F = 300, 136
    X, W, bias, y, n, tX, tW, tb, ty, tn = _case(L, F)
    X2, y2 = X.copy(), y.astype(np.float32)
    clean = _fused(tX, tW, tb, _t(y2)[0], tn, k=10)
    for b in range(B):
        X2[b, int(n[b]):] = np.nan
        y2[b, int(n[b]):] = np.nan
    tX2, ty2 = _t(X2, y2)
    for _ in range(2):
        for a, b in zip(clean, _fused(tX2, tW, tb, ty2, tn, k=10)):
            assert torch.equal(a, b)
    assert torch.isfinite(clean[0]).all() and torch.isfinite(clean[2]).all()


# ---- the modules ----
def _close_loss(got, want):
    """tests/test_gpu_linear_listwise.py: the module test's loss tolerance."""
    assert torch.allclose(got.detach(), want.detach(), rtol=2e-5, atol=1e-5), (got - want).abs().max().item()


def _close_grads(dW, db, want_dW, want_db):
    """tests/test_gpu_linear_listwise.py: one absolute tolerance, from the weight gradient, for dW and db."""
    tol = 1e-5 * max(1.0, float(want_dW.abs().max()))
    assert torch.allclose(dW.reshape(-1), want_dW.reshape(-1), rtol=1e-4, atol=tol), (dW.reshape(-1) - want_dW.reshape(-1)).abs().max().item()
    assert torch.allclose(db.reshape(-1), want_db.reshape(-1), rtol=1e-4, atol=tol), (db.reshape(-1) - want_db.reshape(-1)).abs().max().item()


@pytest.mark.parametrize("Bq,L,F", [(64, 100, 136), (6, 50, 46)])
@pytest.mark.parametrize("loss", ["module", "name"])
def test_fused_linear_loss_agrees_with_the_plain_layer(loss, Bq, L, F):
    """(64, 100, 136): the fused launch; F = 46: ltr_linear_lambdarank_plan says 0, the three kernels -- the same
    module result within the same tolerances."""
    from pytorchltr_amd import _C
    from pytorchltr_amd.fused import FusedLinearLoss, LinearScorer, linear_loss_step
    from pytorchltr_amd.loss import LambdaRankLoss
    loss_fn = LambdaRankLoss(k=10) if loss == "module" else LambdaRankLoss()
    X, _, _, y, n = _data(7, Bq, L, F)
    tX, ty, tn = _t(X, y, n)
    assert _C.lib().ltr_linear_lambdarank_plan(Bq, L, F) == (1 if F == 136 else 0)
    torch.manual_seed(3)
    plain = LinearScorer(F, lazy=False).to(_dev())          # (every call computes its scores)
    fused = FusedLinearLoss(F, loss=loss_fn if loss == "module" else "lambdarank").to(_dev())
    fused.load_state_dict(plain.state_dict())                          # the same keys and shapes
    w = torch.rand(Bq, device=_dev())
    for reduce in (lambda out: (out * w).sum(), lambda out: out.mean()):
        plain.zero_grad()
        fused.zero_grad()
        want = loss_fn(plain(tX), ty, tn)                # scorer + LambdaRankLoss + autograd
        reduce(want).backward()
        got = fused(tX, ty, tn)
        reduce(got).backward()
        _close_loss(got, want)
        _close_grads(fused.weight.grad, fused.bias.grad, plain.weight.grad, plain.bias.grad)
    got, scores = fused(tX, ty, tn, return_scores=True)
    real = torch.arange(L, device=_dev())[None, :] < tn.clamp(max=L)[:, None]
    want_s = plain(tX).squeeze(-1).detach() * real
    assert scores.shape == (Bq, L) and torch.allclose(scores * real, want_s, rtol=1e-5, atol=1e-5)
    lossv, dW, db, lsum = linear_loss_step(tX, plain.weight.detach(), plain.bias.detach(), ty, tn,
                                           loss=loss_fn if loss == "module" else "lambdarank", return_loss_sum=True)
    _close_loss(lossv, want)
    _close_grads(dW, db, plain.weight.grad, plain.bias.grad)           # (the last pass above was .mean())
    assert torch.allclose(lsum, want.detach().sum().reshape(1), rtol=2e-5, atol=1e-5)


def test_drop_in_on_lazy_scores_reaches_the_fused_entry_point(monkeypatch):
    from pytorchltr_amd import _C
    from pytorchltr_amd.fused import use_linear_scorer
    from pytorchltr_amd.loss import LambdaRankLoss
    Bq, L, F = 64, 100, 136
    X, _, _, y, n = _data(17, Bq, L, F)
    tX, ty, tn = _t(X, y, np.maximum(n, 1))
    torch.manual_seed(5)
    plain = torch.nn.Sequential(torch.nn.Linear(F, 1)).to(_dev())
    model = use_linear_scorer(copy.deepcopy(plain))
    loss_fn = LambdaRankLoss(sigma=2.5, k=10)
    loss_fn(plain(tX), ty, tn).mean().backward()

    lib = _C.lib()
    calls = {"step": [], "loss": 0}
    real_step, real_loss = lib.ltr_linear_lambdarank_partials_f32, lib.ltr_lambdarank_f32

    def step(k, sigma, *rest):
        calls["step"].append((k, sigma))
        return real_step(k, sigma, *rest)

    def alone(*args):
        calls["loss"] += 1
        return real_loss(*args)

    monkeypatch.setattr(lib, "ltr_linear_lambdarank_partials_f32", step)
    monkeypatch.setattr(lib, "ltr_lambdarank_f32", alone)
    scores = model(tX)
    out = loss_fn(scores, ty, tn)
    assert scores._real is None and calls == {"step": [(10, 2.5)], "loss": 0}    # scorer, loss and rows in one launch
    out.mean().backward()
    monkeypatch.undo()
    _close_loss(out, loss_fn(plain(tX), ty, tn))
    _close_grads(model[0].weight.grad, model[0].bias.grad, plain[0].weight.grad, plain[0].bias.grad)
