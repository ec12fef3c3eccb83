"""GPU tier of the fused MLP step of the listwise losses (run with `-m gpu` on an MI355X): ltr_mlp_listwise_f32 --
the guide's network, ListNet or ListMLE in the loss slot, backward -- on both kernel layouts against an fp64 reference
on the CPU: the network in float64, the loss and d loss / d s from oracle.ltr_oracle.listwise_softmax and
tests.test_listmle_host.oracle on those scores, the parameter gradients from torch float64 autograd with that ds times
grad_out as the upstream gradient.

Tolerances: scores, the ListNet loss and every gradient tensor as tests/test_gpu_mlp.py::_check (the gradient scale
includes sum |ds| go); the ListMLE loss rtol 1e-4 / atol 1e-4 as tests/test_gpu_linear_listwise.py.  Index tie order
unless a test says otherwise."""
import functools

import numpy as np
import pytest
import torch

from oracle import ltr_oracle as O
from tests.test_listmle_host import oracle as listmle_oracle

pytestmark = pytest.mark.gpu

LISTNET, LISTMLE = "listnet", "listmle"
# B, L, F, H1, H2 and the layouts that take the shape
SHAPES = [
    (5, 20, 44, 50, 10, ("tile", "wide")),        # one fill
    (6, 33, 8, 3, 1, ("tile", "wide")),           # subtile and fill edge, tiny network
    (4, 128, 136, 50, 10, ("tile", "wide")),      # last parked fill
    (3, 129, 136, 13, 5, ("tile",)),              # forward-again class
    (3, 256, 24, 13, 5, ("tile",)),
    (4, 100, 220, 64, 16, ("wide",)),             # wide kernel only
    (3, 128, 148, 64, 16, ("wide",)),
]
CASES = [pytest.param(s[:5], lay, id="%dx%dx%d-%s" % (s[0], s[1], s[2], lay)) for s in SHAPES for lay in s[5]]


def _dev():
    assert torch.cuda.is_available(), "GPU tier needs a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(params=["tile", "wide"])
def layout(request):
    """Both kernel layouts of the training step, through ltr_debug_mlp_layout (reset afterwards)."""
    with _Layout(request.param):
        yield request.param


class _Layout:
    def __init__(self, name):
        self.code = {"tile": 2, "wide": 1}[name]

    def __enter__(self):
        from pytorchltr_amd import _C
        _C.lib().ltr_debug_mlp_layout(self.code)

    def __exit__(self, *exc):
        from pytorchltr_amd import _C
        _C.lib().ltr_debug_mlp_layout(0)
        return False


def _params(F, H1, H2, rng):
    def u(*shape, fan):
        return ((rng.random(shape) * 2 - 1) / np.sqrt(fan)).astype(np.float32)
    return [u(H1, F, fan=F), u(H1, fan=F), u(H2, H1, fan=H1), u(H2, fan=H1), u(1, H2, fan=H2), u(1, fan=H2)]


@functools.lru_cache(maxsize=None)
def _data(B, L, F, H1, H2, dtype="int64", grades=5, lengths=None):
    """Normal features, nn.Linear-style parameters, labels in [0, grades), ragged n with L, 1, 0 and L + 7 behind the
    first query (or `lengths`).  Cached and shared: never written to."""
    rng = np.random.default_rng(1000 * L + 10 * F + B)
    X = rng.normal(0.0, 1.0, (B, L, F)).astype(np.float32)
    if dtype == "float32":
        y = (rng.integers(0, 2 * grades, (B, L)) * 0.5).astype(np.float32)
    else:
        y = rng.integers(0, grades, (B, L)).astype(dtype)
    n = rng.integers(2, L + 1, B).astype(np.int64)
    for i, v in enumerate((L, 1, 0, L + 7)):
        if i + 1 < B:
            n[i + 1] = v
    if lengths is not None:
        n[:] = lengths
    return X, y, n, _params(F, H1, H2, rng)


def _network64(X, params):
    W1, b1, W2, b2, W3, b3 = [torch.from_numpy(p.astype(np.float64)).requires_grad_() for p in params]
    x = torch.from_numpy(X.astype(np.float64))
    h = torch.relu(torch.relu(x @ W1.T + b1) @ W2.T + b2)
    return (h @ W3.T + b3).squeeze(-1), (W1, b1, W2, b2, W3, b3)


def _loss64(loss, s, y, n, k, tie=None):
    if loss == LISTNET:
        return O.listwise_softmax(s, y, n)
    return listmle_oracle(s, y, n, k, tie)


@functools.lru_cache(maxsize=None)
def _reference(loss, k, key, go_seed=None):
    """(loss (B), scores (B, L), six gradients, sum |ds| go) in fp64 for _data(*key); computed once per case."""
    X, y, n, params = _data(*key)
    B, L = y.shape
    go = np.full(B, 1.0 / B) if go_seed is None else _grad_out(B, go_seed).astype(np.float64)
    s, leaves = _network64(X, params)
    want_l, ds = _loss64(loss, s.detach().numpy(), y, n, k)
    real = np.arange(L)[None, :] < np.clip(n, 0, L)[:, None]
    up = np.where(real, ds, 0.0) * go[:, None]
    s.backward(torch.from_numpy(up))
    return want_l, s.detach().numpy(), [t.grad.numpy() for t in leaves], float(np.abs(up).sum())


def _grad_out(B, seed):
    return (np.random.default_rng(seed).random(B) + 0.1).astype(np.float32)


def _step(loss, X, y, n, params, k=None, grad_out=None):
    """mlp_loss_step on the device: (loss, grads, scores, loss_sum)."""
    from pytorchltr_amd import fused
    from pytorchltr_amd.loss import ListMLELoss
    dev = _dev()
    obj = ListMLELoss(k) if (loss == LISTMLE and k is not None) else loss
    out = fused.mlp_loss_step(torch.from_numpy(X).to(dev), [torch.from_numpy(p).to(dev) for p in params],
                              torch.from_numpy(y).to(dev), torch.from_numpy(n).to(dev), loss=obj,
                              grad_out=None if grad_out is None else torch.from_numpy(grad_out).to(dev),
                              return_scores=True, return_loss_sum=True)
    torch.cuda.synchronize()
    return out


def _compare(loss, got, want, n, L):
    lossv, grads, scores, lsum = got
    want_l, want_s, want_g, ds_scale = want
    got_l = lossv.cpu().numpy().astype(np.float64)
    err = np.abs(got_l - want_l).max() if len(want_l) else 0.0
    print("loss %s max err %.3g" % (loss, err))
    assert np.all(np.isfinite(got_l))
    if loss == LISTNET:
        assert np.allclose(got_l, want_l, rtol=2e-5, atol=1e-5), err
        assert np.allclose(float(lsum), want_l.sum(), rtol=2e-5, atol=1e-4)
    else:
        np.testing.assert_allclose(got_l, want_l, rtol=1e-4, atol=1e-4)
        assert np.allclose(float(lsum), want_l.sum(), rtol=1e-4, atol=1e-4 * max(1, len(want_l)))
    valid = np.arange(L)[None, :] < np.clip(n, 0, L)[:, None]
    got_s = scores.cpu().numpy()
    assert np.allclose(got_s[valid], want_s[valid], rtol=1e-5, atol=2e-6)
    assert not got_s[~valid].any()
    scale = max(max(np.abs(w).max() for w in want_g), ds_scale)
    for key, g, w in zip(("W1", "b1", "W2", "b2", "W3", "b3"), grads, want_g):
        tol = 2e-5 * max(np.abs(w).max(), 0.25 * scale) + 1e-6
        e = np.abs(g.cpu().numpy().reshape(w.shape).astype(np.float64) - w).max()
        print("  d%s err %.3g tol %.3g" % (key, e, tol))
        assert e <= tol, (loss, key, e, tol)


@pytest.mark.parametrize("shape,lay", CASES)
@pytest.mark.parametrize("loss,k", [(LISTNET, None), (LISTMLE, None), (LISTMLE, 1), (LISTMLE, 10), (LISTMLE, 10 ** 6)])
def test_against_the_fp64_reference(shape, lay, loss, k):
    from pytorchltr_amd.utils import tie_breaking
    X, y, n, params = _data(*shape)
    with _Layout(lay), tie_breaking("index"):
        got = _step(loss, X, y, n, params, k=k)
    _compare(loss, got, _reference(loss, k, shape), n, shape[1])
    lossv = got[0].cpu().numpy()
    assert (n <= 1).any() and np.all(lossv[n <= (0 if loss == LISTNET else 1)] == 0.0)     # n = 0; ListMLE: n = 1 as well


@pytest.mark.parametrize("loss", [LISTNET, LISTMLE])
def test_every_list_length_class_in_one_batch(layout, loss):
    from pytorchltr_amd.utils import tie_breaking
    L = 40
    key = (9, L, 24, 13, 5, "int64", 5, (L, 0, 1, 2, 16, 17, 32, 33, L))
    X, y, n, params = _data(*key)
    with tie_breaking("index"):
        got = _step(loss, X, y, n, params, k=3 if loss == LISTMLE else None)
    _compare(loss, got, _reference(loss, 3 if loss == LISTMLE else None, key), n, L)


def test_all_labels_equal_under_index_ties(layout):
    from pytorchltr_amd.utils import tie_breaking
    key = (5, 50, 24, 13, 5)
    X, y, n, params = _data(*key)
    y0 = np.full_like(y, 2)
    want_l, want_s, _, _ = _reference(LISTMLE, None, key)
    want_l0, _ = listmle_oracle(want_s, y0, n, None)                    # the index order: pi = identity
    with tie_breaking("index"):
        lossv = _step(LISTMLE, X, y0, n, params)[0]
    np.testing.assert_allclose(lossv.cpu().numpy(), want_l0, rtol=1e-4, atol=1e-4)
    assert not np.allclose(want_l0, want_l, rtol=1e-3, atol=1e-3)      # (the labels mattered)


def _standalone_listmle(sc, ty, tn, tie_args):
    """ltr_listmle_f32 with the C ABI's four tie arguments as given: (loss, dscores)."""
    from pytorchltr_amd import _C
    lib = _C.lib()
    B, L = sc.shape
    loss = torch.empty(B, dtype=torch.float32, device=sc.device)
    ds = torch.empty(B, L, dtype=torch.float32, device=sc.device)
    _C.check(lib.ltr_listmle_f32(_C.ptr(sc), _C.ptr(ty), _C.label_dtype(ty), _C.ptr(tn), 0, *tie_args, B, L,
                                 _C.ptr(loss), _C.ptr(ds), None, 0, _C.stream_of(sc)))
    torch.cuda.synchronize()
    return loss, ds


@pytest.mark.parametrize("mode", ["seed", "seed_dev", "priorities"])
@pytest.mark.parametrize("L,lay", [(100, "tile"), (100, "wide"), (256, "tile")])
def test_tie_modes_agree_with_the_stand_alone_kernel(L, lay, mode):
    """Three grades, so ties everywhere.  Each tie mode of the C ABI besides index order -- a host seed, a seed read
    from device memory, explicit priorities -- against ltr_listmle_f32 run on this call's scores_out with the same
    tie arguments: the loss, and ds (not visible alone behind the network) through the fp64 network's gradients."""
    from pytorchltr_amd import _C, fused
    dev = _dev()
    F, H1, H2, B = 24, 13, 5, 6
    seed = 0x1234567 + L
    X, y, n, params = _data(B, L, F, H1, H2, "int64", 3)
    tX, ty, tn = [torch.from_numpy(a).to(dev) for a in (X, y, n)]
    P = [torch.from_numpy(p).to(dev) for p in params]
    keep = None
    if mode == "seed":
        tie_args = (None, 1, seed, None)
    elif mode == "seed_dev":
        keep = torch.tensor([seed], dtype=torch.int64, device=dev)
        tie_args = (None, 1, 0, _C.ptr(keep))                          # the device word overrides the host seed
    else:
        keep = torch.from_numpy(np.random.default_rng(L).permutation(L).astype(np.int32)).to(dev)
        tie_args = (_C.ptr(keep), 0, 0, None)
    lib = _C.lib()
    npar = int(lib.ltr_mlp_param_count(F, H1, H2))
    nbytes = int(lib.ltr_mlp_workspace_bytes(B, F, H1, H2))
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    out = torch.empty(B, dtype=torch.float32, device=dev)
    sc = torch.zeros(B, L, dtype=torch.float32, device=dev)
    flat = torch.empty(npar, dtype=torch.float32, device=dev)

    def run(args):
        _C.check(lib.ltr_mlp_listwise_f32(1, 0, _C.ptr(tX), *[_C.ptr(t) for t in P], _C.ptr(ty), 0, _C.ptr(tn), *args,
                                          None, B, L, F, H1, H2, _C.ptr(out), _C.ptr(sc), _C.ptr(flat), None,
                                          _C.ptr(ws), nbytes, _C.stream_of(tX)))
        torch.cuda.synchronize()
        return out.clone(), flat.clone()

    with _Layout(lay):
        got_l, got_flat = run(tie_args)
        idx_l, _ = run((None, 0, 0, None))
    assert not torch.equal(got_l, idx_l)                               # another order of the tied grades
    want_l, ds = _standalone_listmle(sc, ty, tn, tie_args)
    np.testing.assert_allclose(got_l.cpu().numpy(), want_l.cpu().numpy(), rtol=1e-4, atol=1e-4)
    if mode == "seed_dev":
        assert torch.equal(got_l, run((None, 1, seed, None))[0])       # the same seed from the host: the same bits
    # ds of the stand-alone kernel through the fp64 network: the gradients of this call
    s64, leaves = _network64(X, params)
    s64.backward(torch.from_numpy(ds.cpu().numpy().astype(np.float64) / B))
    want_g = [t.grad.numpy() for t in leaves]
    scale = max(max(np.abs(w).max() for w in want_g), float(np.abs(ds.cpu().numpy()).sum() / B))
    for g, w in zip(fused._split_grads(got_flat, F, H1, H2), want_g):
        tol = 2e-5 * max(np.abs(w).max(), 0.25 * scale) + 1e-6
        assert np.abs(g.cpu().numpy().reshape(w.shape) - w).max() <= tol


@pytest.mark.parametrize("dtype", ["int32", "float32"])
def test_label_dtypes(layout, dtype):
    from pytorchltr_amd.utils import tie_breaking
    key = (5, 40, 24, 13, 5, dtype)
    X, y, n, params = _data(*key)
    for loss, k in ((LISTNET, None), (LISTMLE, 10)):
        with tie_breaking("index"):
            got = _step(loss, X, y, n, params, k=k)
        _compare(loss, got, _reference(loss, k, key), n, 40)


@pytest.mark.parametrize("loss", [LISTNET, LISTMLE])
def test_explicit_grad_out(layout, loss):
    from pytorchltr_amd.utils import tie_breaking
    key = (7, 70, 44, 50, 10)
    X, y, n, params = _data(*key)
    with tie_breaking("index"):
        got = _step(loss, X, y, n, params, k=5 if loss == LISTMLE else None, grad_out=_grad_out(7, 3))
    _compare(loss, got, _reference(loss, 5 if loss == LISTMLE else None, key, 3), n, 70)


@pytest.mark.parametrize("loss", [LISTNET, LISTMLE])
def test_more_queries_than_workgroups(layout, loss):
    """Short lists, more queries than the grid has workgroups: a workgroup carries several queries (the scheduling
    pass deals them out) and loss_sum adds them all."""
    from pytorchltr_amd.utils import tie_breaking
    cus = torch.cuda.get_device_properties(_dev()).multi_processor_count
    B = 2 * cus + 700
    key = (B, 24, 16, 12, 4)
    X, y, n, params = _data(*key)
    with tie_breaking("index"):
        got = _step(loss, X, y, n, params)
    _compare(loss, got, _reference(loss, None, key), n, 24)


def test_padding_is_never_read_and_runs_are_bit_identical(layout):
    from pytorchltr_amd.utils import tie_breaking
    key = (10, 64, 32, 20, 6)
    X, y, n, params = _data(*key)
    X2, y2 = X.copy(), y.astype(np.float32)
    for b in range(10):
        X2[b, min(max(int(n[b]), 0), 64):] = np.nan
        y2[b, min(max(int(n[b]), 0), 64):] = np.nan
    for loss in (LISTNET, LISTMLE):
        with tie_breaking("index"):
            clean = _step(loss, X, y.astype(np.float32), n, params, k=5 if loss == LISTMLE else None)
            again = _step(loss, X, y.astype(np.float32), n, params, k=5 if loss == LISTMLE else None)
            dirty = _step(loss, X2, y2, n, params, k=5 if loss == LISTMLE else None)
        for other in (again, dirty):
            assert torch.equal(clean[0], other[0]) and torch.equal(clean[2], other[2]) and torch.equal(clean[3], other[3])
            for u, v in zip(clean[1], other[1]):
                assert torch.equal(u, v)                               # bit-exact
        assert torch.isfinite(clean[0]).all() and all(torch.isfinite(g).all() for g in clean[1])


# ---- the module ----
def _losses():
    from pytorchltr_amd.loss import ListMLELoss, ListwiseSoftmaxLoss
    return [ListwiseSoftmaxLoss(), ListMLELoss(), ListMLELoss(k=10)]


def _module_pair(F, loss_fn, reduction):
    from pytorchltr_amd.fused import FusedMLPListwiseLoss
    torch.manual_seed(3)
    fused = FusedMLPListwiseLoss(F, loss=loss_fn, reduction=reduction).to(_dev())
    plain = torch.nn.Sequential(torch.nn.Linear(F, 50), torch.nn.ReLU(), torch.nn.Linear(50, 10), torch.nn.ReLU(),
                                torch.nn.Linear(10, 1)).to(_dev())
    for src, dst in ((fused.l1, plain[0]), (fused.l2, plain[2]), (fused.l3, plain[4])):
        dst.load_state_dict(src.state_dict())
    return fused, plain


def _close_module(fused, plain, got, want):
    """The tolerances of tests/test_gpu_mlp.py::test_module_matches_unfused_composition (fp32 against fp32); the
    ListMLE loss as everywhere in this file."""
    listmle = fused.kind.loss == 1
    assert torch.allclose(got.detach(), want.detach(), rtol=1e-4 if listmle else 1e-5, atol=1e-4 if listmle else 1e-6), \
        (got - want).abs().max().item()
    scale = max(float(p.grad.abs().max()) for p in plain.parameters())
    for a, b in zip(fused.parameters(), plain.parameters()):
        assert a.grad is not None
        assert torch.allclose(a.grad, b.grad, rtol=2e-4, atol=2e-5 * max(1.0, scale)), (a.grad - b.grad).abs().max().item()


@pytest.mark.parametrize("i", range(3))
@pytest.mark.parametrize("F", [46, 136])
@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_module_agrees_with_the_unfused_composition(layout, i, F, reduction):
    from pytorchltr_amd.utils import tie_breaking
    loss_fn = _losses()[i]
    B, L = 12, 100
    X, y, n, _ = _data(B, L, F, 50, 10)
    tX, ty, tn = [torch.from_numpy(a).to(_dev()) for a in (X, y, n)]
    fused, plain = _module_pair(F, loss_fn, reduction)
    with tie_breaking("index"):
        per_query = loss_fn(plain(tX), ty, tn)
        want = per_query.mean() if reduction == "mean" else per_query.sum()
        want.backward()
        got = fused(tX, ty, tn)
        got.backward()
    _close_module(fused, plain, got, want)
    assert torch.allclose(fused.last_losses, per_query.detach(), rtol=1e-4 if i else 1e-5, atol=1e-4 if i else 1e-5)
    with torch.no_grad():
        real = torch.arange(L, device=_dev())[None, :] < tn.clamp(0, L)[:, None]
        assert torch.allclose(fused.score(tX, tn).squeeze(-1) * real, plain(tX).squeeze(-1) * real, rtol=1e-5, atol=1e-5)


def test_long_lists_take_the_unfused_path_and_train():
    from pytorchltr_amd import fused as fused_mod
    from pytorchltr_amd.utils import tie_breaking
    B, L, F = 4, 300, 24
    X, y, n, _ = _data(B, L, F, 50, 10)
    tX, ty, tn = [torch.from_numpy(a).to(_dev()) for a in (X, y, n)]
    for loss_fn in _losses()[:2]:
        fused, plain = _module_pair(F, loss_fn, "mean")
        assert not fused_mod.mlp_listwise_supported(fused.kind, B, L, F, 50, 10)
        with tie_breaking("index"):
            want = loss_fn(plain(tX), ty, tn).mean()
            want.backward()
            got = fused(tX, ty, tn)
            got.backward()
            _close_module(fused, plain, got, want)
            opt = torch.optim.SGD(fused.parameters(), lr=1e-3)    # (small steps: the loss must fall)
            first = float(got)
            for _ in range(5):
                opt.step()
                opt.zero_grad()
                out = fused(tX, ty, tn)
                out.backward()
            assert float(out) < first


def test_capture_and_replay():
    """Forward + backward of FusedMLPListwiseLoss(loss="listmle") captured with torch.cuda.graph and replayed twice:
    the eager result bit for bit."""
    from pytorchltr_amd.fused import FusedMLPListwiseLoss
    from pytorchltr_amd.utils import tie_breaking
    B, L, F = 32, 60, 24
    X, y, n, _ = _data(B, L, F, 50, 10)
    tX, ty, tn = [torch.from_numpy(a).to(_dev()) for a in (X, y, n)]
    torch.manual_seed(7)
    m = FusedMLPListwiseLoss(F, loss="listmle").to(_dev())

    def step():
        out = m(tX, ty, tn)
        out.backward()
        return out.detach()

    def grads():
        return [p.grad for p in m.parameters()]

    with tie_breaking("index"):
        eager = [step().clone()] + [g.clone() for g in grads()]
        m.zero_grad(set_to_none=True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                                  # (warm-up on a side stream, as torch asks)
            step()
        torch.cuda.current_stream().wait_stream(side)
        m.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            cap = step()
        for _ in range(2):
            cap.fill_(float("nan"))
            for g in grads():
                g.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(cap, eager[0])
            for g, w in zip(grads(), eager[1:]):
                assert torch.equal(g, w)
