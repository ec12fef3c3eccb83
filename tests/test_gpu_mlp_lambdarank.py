"""GPU tier of the fused MLP step of LambdaRankLoss (run with `-m gpu` on an MI355X): ltr_mlp_lambdarank_f32 -- the
guide's network, the LambdaRank row in the loss slot, backward -- on both kernel layouts against an fp64 reference on the
CPU: the network in float64 for the scores, tests/lambdarank_ref.py ON THE SCORES THE GPU RETURNED for the loss and
d loss / d s (the NDCG weights are discontinuous in the ranking: an fp32 / fp64 rank flip is no kernel bug), and torch
float64 autograd of the network with that ds times grad_out as the upstream gradient for the six parameter gradients.

Tolerances: scores rtol 1e-5 / atol 2e-6 (tests/test_gpu_mlp_listwise.py); the loss 2e-6 + 1e-5 |want|, the stand-alone
kernel's bound for L <= 256 (tests/test_gpu_linear_lambdarank.py); loss_sum the sum of the per-query bounds; every
gradient tensor 2e-5 max(|w|max, 0.25 scale) + 1e-6 with scale = max(largest gradient entry, sum |ds| go)."""
import functools

import numpy as np
import pytest
import torch

from tests import lambdarank_ref as R
from tests.test_gpu_mlp_listwise import CASES, _close_module, _data, _grad_out, _Layout, _network64

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tier needs a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(params=["tile", "wide"])
def layout(request):
    """Both kernel layouts of the training step, through ltr_debug_mlp_layout (reset afterwards)."""
    with _Layout(request.param):
        yield request.param


@functools.lru_cache(maxsize=None)
def _scores64(key):
    """The fp64 network's scores for _data(*key); computed once per shape."""
    X, _, _, params = _data(*key)
    with torch.no_grad():
        return _network64(X, params)[0].numpy()


def _step(X, y, n, params, k=None, sigma=1.0, grad_out=None):
    """mlp_lambdarank_step on the device: (loss, grads, scores, loss_sum)."""
    from pytorchltr_amd import fused
    dev = _dev()
    out = fused.mlp_lambdarank_step(torch.from_numpy(X).to(dev), [torch.from_numpy(p).to(dev) for p in params],
                                    torch.from_numpy(y).to(dev), torch.from_numpy(n).to(dev), sigma=sigma, k=k,
                                    grad_out=None if grad_out is None else torch.from_numpy(grad_out).to(dev),
                                    return_scores=True, return_loss_sum=True)
    torch.cuda.synchronize()
    return out


def _check(got, key, k, sigma, y=None, go_seed=None):
    """The whole contract of one call against the references of the module docstring."""
    X, y0, n, params = _data(*key)
    y = y0 if y is None else y
    B, L = y.shape
    lossv, grads, scores, lsum = got
    valid = np.arange(L)[None, :] < np.clip(n, 0, L)[:, None]
    got_s = scores.cpu().numpy()
    assert np.allclose(got_s[valid], _scores64(key)[valid], rtol=1e-5, atol=2e-6)
    assert np.all(got_s[~valid] == 0.0)                                # padded documents: exactly 0
    # the loss and ds on the returned scores
    want_l, ds = R.batch(got_s, y, n, k=k, sigma=sigma)
    got_l = lossv.cpu().numpy().astype(np.float64)
    bound = 2e-6 + 1e-5 * np.abs(want_l)
    err = np.abs(got_l - want_l)
    print("loss: worst err / bound %.3g" % (err / bound).max())
    assert np.all(np.isfinite(got_l)) and np.all(err <= bound), (err.max(), got_l, want_l)
    assert abs(float(lsum) - want_l.sum()) <= bound.sum()
    assert np.all(got_l[n <= 1] == 0.0)
    # the six gradients: fp64 autograd of the network under ds * grad_out
    go = np.full(B, 1.0 / B) if go_seed is None else _grad_out(B, go_seed).astype(np.float64)
    up = np.where(valid, ds, 0.0) * go[:, None]
    s64, leaves = _network64(X, params)
    s64.backward(torch.from_numpy(up))
    want_g = [t.grad.numpy() for t in leaves]
    scale = max(max(np.abs(w).max() for w in want_g), float(np.abs(up).sum()))
    for name, g, w in zip(("W1", "b1", "W2", "b2", "W3", "b3"), grads, want_g):
        tol = 2e-5 * max(np.abs(w).max(), 0.25 * scale) + 1e-6
        e = np.abs(g.cpu().numpy().reshape(w.shape).astype(np.float64) - w).max()
        print("  d%s err %.3g tol %.3g" % (name, e, tol))
        assert e <= tol, (name, e, tol)
    return want_l, ds


# ---- 1. against the reference ----
@pytest.mark.parametrize("shape,lay", CASES)
@pytest.mark.parametrize("sigma", [1.0, 2.5])
@pytest.mark.parametrize("k", [None, 1, 10, 10 ** 6])
def test_against_the_fp64_reference(shape, lay, k, sigma):
    """k = 10 < n: the anchor x tail pass; k >= n and None: the full pass.  Ragged n with L, 1, 0 and L + 7."""
    X, y, n, params = _data(*shape)
    with _Layout(lay):
        got = _step(X, y, n, params, k=k, sigma=sigma)
    _check(got, shape, k, sigma)
    assert (n <= 1).any()                                              # (_check: their losses are exactly 0)


# ---- 2. every list-length class in one batch ----
@pytest.mark.parametrize("k", [None, 10])
@pytest.mark.parametrize("lay,L,lengths", [("tile", 256, (256, 0, 1, 2, 63, 64, 65, 128, 129)),
                                           ("wide", 128, (128, 0, 1, 2, 63, 64, 65, 127, 11))])
def test_every_list_length_class_in_one_batch(lay, L, lengths, k):
    """n on both sides of 64 and 128 and at the longest list: every owners x msplit cut of the counting rank (tile:
    64 x 4, 128 x 2, 256 x 1; 8-wave: 64 x 8, 128 x 4)."""
    key = (9, L, 24, 13, 5, "int64", 5, lengths)
    X, y, n, params = _data(*key)
    with _Layout(lay):
        got = _step(X, y, n, params, k=k, sigma=1.0)
    _check(got, key, k, 1.0)


# ---- 3. degenerate rows ----
@pytest.mark.parametrize("k", [None, 10])
def test_all_labels_equal(layout, k):
    """No pair has y_i > y_j: loss 0 and zero gradient rows, for a grade with a positive gain and for grade 0 (maxDCG
    0 -> 1, no 0 / 0)."""
    key = (5, 50, 24, 13, 5)
    X, y, n, params = _data(*key)
    for grade in (2, 0):
        lossv, grads, _, lsum = _step(X, np.full_like(y, grade), n, params, k=k)
        assert not lossv.cpu().numpy().any() and float(lsum) == 0.0
        assert all(not g.cpu().numpy().any() for g in grads)


@pytest.mark.parametrize("k", [1, None])
def test_max_dcg_zero_counts_as_one(layout, k):
    """Grades 0 and -1 (gains 0 and -0.5): at k = 1 the ideal top document has gain 0, maxDCG is 0 -> 1, and the pairs
    (0 over -1) still carry weight."""
    key = (5, 50, 24, 13, 5)
    X, y, n, params = _data(*key)
    y2 = -(y % 2)
    want_l, _ = _check(_step(X, y2, n, params, k=k), key, k, 1.0, y=y2)
    assert want_l.max() > 0.0


@pytest.mark.parametrize("k", [10, None])
@pytest.mark.parametrize("dtype", ["int32", "float32"])
def test_label_dtypes(layout, dtype, k):
    """int32 grades and float32 labels with half grades (0, 0.5, .. 4.5)."""
    key = (5, 40, 24, 13, 5, dtype)
    X, y, n, params = _data(*key)
    assert dtype != "float32" or (y % 1 != 0).any()
    _check(_step(X, y, n, params, k=k, sigma=2.5), key, k, 2.5)


@pytest.mark.parametrize("k", [10, None])
def test_explicit_grad_out(layout, k):
    key = (7, 70, 44, 50, 10)
    X, y, n, params = _data(*key)
    _check(_step(X, y, n, params, k=k, grad_out=_grad_out(7, 3)), key, k, 1.0, go_seed=3)


# ---- 4. more queries than resident workgroups ----
def test_more_queries_than_workgroups(layout):
    """Short lists, more queries than the grid has workgroups: a workgroup carries several queries.  The same batch in
    two halves gives the same per-query losses and scores bit for bit, and its gradients add up to the whole batch's."""
    cus = torch.cuda.get_device_properties(_dev()).multi_processor_count
    B = 2 * cus + 700
    key = (B, 24, 16, 12, 4)
    X, y, n, params = _data(*key)
    whole = _step(X, y, n, params, k=10)
    _check(whole, key, 10, 1.0)
    h = B // 2
    go = np.full(B, 1.0 / B, dtype=np.float32)
    halves = [_step(X[a:b], y[a:b], n[a:b], params, k=10, grad_out=go[a:b]) for a, b in ((0, h), (h, B))]
    assert torch.equal(whole[0], torch.cat([halves[0][0], halves[1][0]]))
    assert torch.equal(whole[2], torch.cat([halves[0][2], halves[1][2]]))
    # (each side is within the file's gradient tolerance of the fp64 reference: twice that between them)
    scale = max(float(g.abs().max()) for g in whole[1])
    for g, a, b in zip(whole[1], halves[0][1], halves[1][1]):
        tol = 2 * (2e-5 * max(float(g.abs().max()), 0.25 * scale) + 1e-6)
        assert float((g - (a + b)).abs().max()) <= tol


# ---- 5. padding and determinism ----
def test_padding_is_never_read_and_runs_are_bit_identical(layout):
    key = (10, 64, 32, 20, 6)
    X, y, n, params = _data(*key)
    yf = y.astype(np.float32)
    X2, y2 = X.copy(), yf.copy()
    for b in range(10):
        X2[b, min(max(int(n[b]), 0), 64):] = np.nan
        y2[b, min(max(int(n[b]), 0), 64):] = np.nan
    for k in (10, None):
        clean = _step(X, yf, n, params, k=k)
        again = _step(X, yf, n, params, k=k)
        dirty = _step(X2, y2, n, params, k=k)
        for other in (again, dirty):
            assert torch.equal(clean[0], other[0]) and torch.equal(clean[2], other[2]) and torch.equal(clean[3], other[3])
            for u, v in zip(clean[1], other[1]):
                assert torch.equal(u, v)                               # bit-exact
        assert torch.isfinite(clean[0]).all() and all(torch.isfinite(g).all() for g in clean[1])
        assert float(clean[0].max()) > 0.0


# ---- 6. the module ----
def _module_pair(F, sigma, k, reduction, hidden=(50, 10)):
    from pytorchltr_amd.fused import FusedMLPLambdaRankLoss, MLPScorer
    torch.manual_seed(3)
    fused = FusedMLPLambdaRankLoss(F, sigma=sigma, k=k, hidden=hidden, reduction=reduction).to(_dev())
    plain = MLPScorer(F, hidden=hidden).to(_dev())
    plain.load_state_dict(fused.state_dict())                          # the same keys and shapes
    return fused, plain


@pytest.mark.parametrize("sigma,k", [(1.0, 10), (2.5, None)])
@pytest.mark.parametrize("F", [46, 136])
@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_module_agrees_with_the_unfused_composition(layout, F, reduction, sigma, k, monkeypatch):
    from pytorchltr_amd import _C
    from pytorchltr_amd.loss import LambdaRankLoss
    B, L = 12, 100
    X, y, n, _ = _data(B, L, F, 50, 10)
    tX, ty, tn = [torch.from_numpy(a).to(_dev()) for a in (X, y, n)]
    fused, plain = _module_pair(F, sigma, k, reduction)
    loss_fn = LambdaRankLoss(sigma, k)
    per_query = loss_fn(plain(tX, tn), ty, tn)                          # what users run today: three launches + autograd
    want = per_query.mean() if reduction == "mean" else per_query.sum()
    want.backward()
    lib = _C.lib()
    calls = []
    real = lib.ltr_mlp_lambdarank_f32
    monkeypatch.setattr(lib, "ltr_mlp_lambdarank_f32", lambda kk, sg, *rest: calls.append((kk, sg)) or real(kk, sg, *rest))
    got = fused(tX, ty, tn)
    got.backward()
    monkeypatch.undo()
    assert calls == [(k or 0, sigma)]                                  # the fused entry point, once
    _close_module(fused, plain, got, want)
    assert fused.last_losses is not None and fused.last_losses.shape == (B,)
    assert torch.allclose(fused.last_losses, per_query.detach(), rtol=1e-5, atol=1e-5)


# ---- 7. off the plan ----
class _Calls:
    """Counts the calls of the fused entry point and of the stand-alone LambdaRank kernels."""
    NAMES = ("ltr_mlp_lambdarank_f32", "ltr_lambdarank_f32", "ltr_lambdarank_long_f32")

    def __init__(self, monkeypatch):
        from pytorchltr_amd import _C
        lib = _C.lib()
        self.count = dict.fromkeys(self.NAMES, 0)
        for name in self.NAMES:
            monkeypatch.setattr(lib, name, self._wrap(name, getattr(lib, name)))

    def _wrap(self, name, fn):
        def call(*args):
            self.count[name] += 1
            return fn(*args)
        return call


def _finite_grads(m):
    """Every .grad finite, and the first layer's not all zero (the last bias's may be: a query's ds add up to 0)."""
    return (all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
            and float(m.l1.weight.grad.abs().max()) > 0.0)


def test_long_lists_take_the_pieces_and_train(monkeypatch):
    from pytorchltr_amd import fused as fused_mod
    from pytorchltr_amd.loss import LambdaRankLoss
    B, L, F = 4, 300, 24
    X, y, n, params = _data(B, L, F, 50, 10)
    tX, ty, tn = [torch.from_numpy(a).to(_dev()) for a in (X, y, n)]
    fused, plain = _module_pair(F, 1.0, 10, "mean")
    assert not fused_mod.mlp_lambdarank_supported(B, L, F, 50, 10)
    want = LambdaRankLoss(1.0, 10)(plain(tX, tn), ty, tn).mean()
    want.backward()
    calls = _Calls(monkeypatch)
    got = fused(tX, ty, tn)
    got.backward()
    assert calls.count == {"ltr_mlp_lambdarank_f32": 0, "ltr_lambdarank_f32": 1, "ltr_lambdarank_long_f32": 0}
    _close_module(fused, plain, got, want)
    # the function: the same pieces
    lossv, grads, lsum = fused_mod.mlp_lambdarank_step(tX, [torch.from_numpy(p).to(_dev()) for p in params], ty, tn, k=10,
                                                       return_loss_sum=True)
    assert calls.count["ltr_mlp_lambdarank_f32"] == 0 and calls.count["ltr_lambdarank_f32"] == 2
    assert torch.isfinite(lossv).all() and all(torch.isfinite(g).all() for g in grads)
    assert torch.allclose(lsum, lossv.sum().reshape(1))
    monkeypatch.undo()
    opt = torch.optim.SGD(fused.parameters(), lr=1e-2)
    first = got.item()
    for _ in range(20):
        opt.step()
        opt.zero_grad()
        out = fused(tX, ty, tn)
        out.backward()
    print("loss %.6g -> %.6g" % (first, out.item()))
    assert out.item() < first


@pytest.mark.parametrize("what", ["F700", "bf16", "L5000"])
def test_wide_rows_bf16_and_the_long_path_take_the_pieces(what, monkeypatch):
    B, L, F = {"F700": (4, 50, 700), "bf16": (4, 50, 24), "L5000": (4, 5000, 24)}[what]
    X, y, n, _ = _data(B, L, F, 50, 10)
    tX, ty, tn = [torch.from_numpy(a).to(_dev()) for a in (X, y, n)]
    if what == "bf16":
        tX = tX.to(torch.bfloat16)
    fused, _ = _module_pair(F, 1.0, 10, "mean")
    calls = _Calls(monkeypatch)
    out = fused(tX, ty, tn)
    out.backward()
    torch.cuda.synchronize()
    long_path = what == "L5000"
    assert calls.count == {"ltr_mlp_lambdarank_f32": 0, "ltr_lambdarank_f32": 0 if long_path else 1,
                           "ltr_lambdarank_long_f32": 1 if long_path else 0}
    assert torch.isfinite(out) and out.item() > 0.0 and _finite_grads(fused)
    assert fused.last_losses.shape == (B,)


def test_step_on_a_bf16_batch_takes_the_pieces(monkeypatch):
    from pytorchltr_amd import fused as fused_mod
    B, L, F = 4, 50, 24
    X, y, n, params = _data(B, L, F, 50, 10)
    tX, ty, tn = [torch.from_numpy(a).to(_dev()) for a in (X, y, n)]
    P = [torch.from_numpy(p).to(_dev()) for p in params]
    calls = _Calls(monkeypatch)
    lossv, grads = fused_mod.mlp_lambdarank_step(tX.to(torch.bfloat16), P, ty, tn, sigma=2.5, k=10)
    assert calls.count == {"ltr_mlp_lambdarank_f32": 0, "ltr_lambdarank_f32": 1, "ltr_lambdarank_long_f32": 0}
    assert torch.isfinite(lossv).all() and float(lossv.max()) > 0.0
    assert all(torch.isfinite(g).all() for g in grads) and float(grads[0].abs().max()) > 0.0
    # the same call on the fp32 batch is on the plan
    fused_mod.mlp_lambdarank_step(tX, P, ty, tn, sigma=2.5, k=10)
    assert calls.count == {"ltr_mlp_lambdarank_f32": 1, "ltr_lambdarank_f32": 1, "ltr_lambdarank_long_f32": 0}


# ---- 8. capture and replay ----
def test_capture_and_replay():
    """mlp_lambdarank_step captured with torch.cuda.graph and replayed twice: the eager call bit for bit."""
    from pytorchltr_amd import _C, fused
    B, L, F = 32, 60, 24
    X, y, n, params = _data(B, L, F, 50, 10)
    tX, ty, tn = [torch.from_numpy(a).to(_dev()) for a in (X, y, n)]
    P = [torch.from_numpy(p).to(_dev()) for p in params]
    flat = torch.empty(int(_C.lib().ltr_mlp_param_count(F, 50, 10)), dtype=torch.float32, device=_dev())

    def step():
        lossv, _, scores, lsum = fused.mlp_lambdarank_step(tX, P, ty, tn, sigma=2.5, k=10, return_scores=True,
                                                           return_loss_sum=True, out=flat)
        return lossv, scores, lsum

    eager = [t.clone() for t in step()] + [flat.clone()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                      # (warm-up on a side stream, as torch asks)
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        cap = step()
    for _ in range(2):
        for t in cap:
            t.fill_(float("nan"))
        flat.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for g, w in zip(list(cap) + [flat], eager):
            assert torch.equal(g, w)
