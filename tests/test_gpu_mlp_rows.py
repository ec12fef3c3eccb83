"""GPU tier of the stand-alone MLP scorer (run with `-m gpu` on an MI355X): ltr_mlp_rows_scores_f32 and
ltr_mlp_rows_grad_f32 (include/ltr_mlp_rows.h) through fused._mlp_rows_scores / fused.mlp_grad, the autograd module
fused.MLPScorer, and the routes past the list lengths of the fused kernels (score(), FusedMLPLoss,
FusedMLPListwiseLoss, mlp_loss_step).

Reference: the three layers in torch float64 on the CPU, loss = (s * g).sum(), autograd.  g has |g| in [0.5, 1.5] with
a random sign on the rows it covers, so a dropped or doubled row moves db3 = sum g by >= 0.5.

Tolerances: scores rtol 1e-5 / atol 2e-6 (the MLP score tolerance of tests/test_gpu_mlp.py), padded scores exactly 0;
every gradient tensor <= 2e-5 * max(max|that tensor|, max|any gradient| / 4) + 1e-6."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tier needs a ROCm device"
    return torch.device("cuda:0")


def _params(F, H1, H2, rng):
    def u(*shape, fan):
        return ((rng.random(shape) * 2 - 1) / np.sqrt(fan)).astype(np.float32)
    return [u(H1, F, fan=F), u(H1, fan=F), u(H2, H1, fan=H1), u(H2, fan=H1), u(1, H2, fan=H2), u(1, fan=H2)]


@functools.lru_cache(maxsize=None)
def _case(B, L, F, H1, H2, lengths="ragged", every=1):
    """Features, parameters, n (`lengths`: a tuple, None = no n, "ragged" = random with 0, 1, L and L + 5 in front), g
    (non-zero on every `every`-th real row) and the float64 reference.  Cached and shared: never written to."""
    rng = np.random.default_rng(100000 * every + 1000 * L + 10 * F + B)
    X = rng.normal(0.0, 1.0, (B, L, F)).astype(np.float32)
    params = _params(F, H1, H2, rng)
    if lengths is None:
        n = None
        real = np.ones((B, L), dtype=bool)
    else:
        if lengths == "ragged":
            n = rng.integers(2, L + 1, B).astype(np.int64)
            for i, v in enumerate((0, 1, L, L + 5)):
                if i < B:
                    n[i] = v
        else:
            n = np.asarray(lengths, dtype=np.int64)
        real = np.arange(L)[None, :] < np.clip(n, 0, L)[:, None]
    g = ((rng.random((B, L)) + 0.5) * rng.choice([-1.0, 1.0], (B, L))).astype(np.float32)
    if every > 1:
        order = np.cumsum(real.reshape(-1)).reshape(B, L)            # 1-based index among the real rows
        g = np.where(order % every == 0, g, np.float32(0.0))
    g = np.where(real, g, np.float32(0.0))
    leaves = [torch.from_numpy(p.astype(np.float64)).requires_grad_() for p in params]
    x = torch.from_numpy(X.astype(np.float64))
    h = torch.relu(torch.relu(x @ leaves[0].T + leaves[1]) @ leaves[2].T + leaves[3])
    s = (h @ leaves[4].T + leaves[5]).squeeze(-1)
    (s * torch.from_numpy(g.astype(np.float64))).sum().backward()
    return dict(X=X, params=params, n=n, g=g, real=real, scores=s.detach().numpy(),
                grads=[t.grad.numpy() for t in leaves])


def _device_args(case, X=None, g=None):
    dev = _dev()
    tX = torch.from_numpy(case["X"] if X is None else X).to(dev)
    tP = [torch.from_numpy(p).to(dev) for p in case["params"]]
    tn = None if case["n"] is None else torch.from_numpy(case["n"]).to(dev)
    tg = torch.from_numpy(case["g"] if g is None else g).to(dev)
    return tX, tP, tn, tg


def _run(case, X=None, g=None):
    """(scores (B, L), six gradients) from the two row kernels."""
    from pytorchltr_amd import fused
    tX, tP, tn, tg = _device_args(case, X, g)
    H1, H2 = tP[0].shape[0], tP[2].shape[0]
    scores = fused._mlp_rows_scores(tX, tP, H1, H2, tn)
    grads = fused.mlp_grad(tX, tP, tg, tn)
    torch.cuda.synchronize()
    return scores, grads


def _compare(case, scores, grads):
    real = case["real"]
    got_s = scores.cpu().numpy()
    err = np.abs(got_s[real] - case["scores"][real]).max() if real.any() else 0.0
    print("scores max err %.3g" % err)
    assert np.allclose(got_s[real], case["scores"][real], rtol=1e-5, atol=2e-6), err
    assert not got_s[~real].any()                                       # padded documents: exactly 0
    scale = max(np.abs(w).max() for w in case["grads"])
    for key, got, w in zip(("W1", "b1", "W2", "b2", "W3", "b3"), grads, case["grads"]):
        tol = 2e-5 * max(np.abs(w).max(), 0.25 * scale) + 1e-6
        e = np.abs(got.cpu().numpy().reshape(w.shape).astype(np.float64) - w).max()
        print("  d%s err %.3g tol %.3g" % (key, e, tol))
        assert e <= tol, (key, e, tol)


# ---- 1. tiles against queries ----
@pytest.mark.parametrize("key", [
    (3, 37, 8, 5, 3, (37, 20, 37)),                # one tile of 32 rows holds three queries
    (2, 300, 24, 50, 10, (300, 129)),              # tiles straddle the query boundary; one document in a further tile
    (5, 300, 136, 50, 10, "ragged"),               # n = 0, 1, L, L + 5 (clamped), random
    (3, 37, 8, 5, 3, None),                        # n == NULL: every row is real
    (2, 300, 24, 50, 10, None),
], ids=["3x37", "2x300", "5x300-ragged", "3x37-no-n", "2x300-no-n"])
def test_tiles_against_queries(key):
    case = _case(*key)
    _compare(case, *_run(case))


# ---- 2. buckets and padding of the network ----
@pytest.mark.parametrize("F,H1,H2", [(F, 64, 16) for F in (8, 48, 52, 80, 84, 136, 144, 148, 220, 224)] + [(8, 1, 1)])
def test_buckets_and_padding_of_the_network(F, H1, H2):
    # a full list and one that ends inside subtile 0 of a tile (150 + 97 = 7 * 32 + 23): 247 real rows in 8 of the 10
    # tiles, both subtiles, full and partly real tiles, in every bucket and for both kernels
    case = _case(2, 150, F, H1, H2, (150, 97))
    assert case["real"].sum() == 247
    _compare(case, *_run(case))


@pytest.mark.parametrize("F", [8, 52, 136, 220])
def test_every_bucket_on_a_ragged_batch_with_several_tiles_per_workgroup(F):
    # one case per bucket (NT = 3, 5, 9, 14): 7 x 5000 = 35 000 flat rows = 1094 tiles, more than twice the 512
    # workgroups of a launch (gradient kernel of the widest bucket: 256), so a workgroup carries its dW1 / dW2 tiles,
    # the g ring and the look-ahead fill over several tiles; n = 0, 1, L, L + 5 and random lengths
    case = _case(7, 5000, F, 50, 10, "ragged")
    assert case["real"].sum() > 5000 and (case["n"][:4] == (0, 1, 5000, 5005)).all()
    _compare(case, *_run(case))


# ---- 3. more tiles than workgroups ----
def test_more_tiles_than_workgroups():
    # 40 x 5000 = 200 000 flat rows = 6250 tiles of 32 rows, about 1e5 of the rows real; the launch has at most
    # 2 workgroups x 256 CUs = 512 workgroups x 32 rows per tile = 16 384 rows in flight, so every workgroup loops over
    # ~12 tiles and the real rows are >= 3 x 16 384
    case = _case(40, 5000, 8, 4, 4, "ragged", 7)
    assert case["real"].sum() >= 3 * 512 * 32
    _compare(case, *_run(case))


# ---- 4. padding is not read ----
def test_padding_is_not_read():
    case = _case(5, 300, 136, 50, 10, "ragged")
    real = case["real"]
    Xn = case["X"].copy()
    Xn[~real] = np.nan
    gn = case["g"].copy()
    gn[~real] = np.nan
    assert np.isnan(Xn).any() and np.isnan(gn).any()
    s0, g0 = _run(case)
    s1, g1 = _run(case, X=Xn, g=gn)
    mask = torch.from_numpy(real).to(_dev())
    assert torch.equal(s0[mask], s1[mask]) and not s1[~mask].any()
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)


# ---- 5. determinism ----
def test_deterministic():
    case = _case(40, 5000, 8, 4, 4, "ragged", 7)
    s0, g0 = _run(case)
    s1, g1 = _run(case)
    assert torch.equal(s0, s1)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    case = _case(5, 300, 136, 50, 10, "ragged")
    s0, g0 = _run(case)
    s1, g1 = _run(case)
    assert torch.equal(s0, s1)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)


def test_an_empty_batch_gives_zero_gradients():
    from pytorchltr_amd import fused
    dev = _dev()
    tP = [torch.from_numpy(p).to(dev) for p in _params(8, 5, 3, np.random.default_rng(0))]
    out = torch.full((8 * 5 + 5 + 5 * 3 + 3 + 3 + 1,), float("nan"), device=dev)
    grads = fused.mlp_grad(torch.zeros(0, 7, 8, device=dev), tP, torch.zeros(0, 7, device=dev), out=out)
    assert fused._mlp_rows_scores(torch.zeros(0, 7, 8, device=dev), tP, 5, 3, None).shape == (0, 7)
    torch.cuda.synchronize()
    assert not out.any() and grads[0].shape == (5, 8)
    # the C ABI itself: B == 0 returns LTR_OK from both calls (no data pointers, no workspace) and zeroes the gradients
    from pytorchltr_amd import _C
    lib, st = _C.lib(), _C.stream_of(out)
    ptrs = [t.data_ptr() for t in tP]
    out.fill_(float("nan"))
    assert lib.ltr_mlp_rows_grad_f32(None, *ptrs, None, None, 0, 7, 8, 5, 3, out.data_ptr(), None, 0, st) == 0
    assert lib.ltr_mlp_rows_scores_f32(None, *ptrs, None, 0, 7, 8, 5, 3, None, st) == 0
    torch.cuda.synchronize()
    assert not out.any()


# ---- 6. the autograd module ----
def _module_pair(F):
    from pytorchltr_amd.fused import MLPScorer
    torch.manual_seed(3)
    ours = MLPScorer(F).to(_dev())
    plain = torch.nn.Sequential(torch.nn.Linear(F, 50), torch.nn.ReLU(), torch.nn.Linear(50, 10), torch.nn.ReLU(),
                                torch.nn.Linear(10, 1)).to(_dev())
    for src, dst in ((ours.l1, plain[0]), (ours.l2, plain[2]), (ours.l3, plain[4])):
        dst.load_state_dict(src.state_dict())
    return ours, plain


def _close_module(ours, plain, got, want, listmle):
    """The tolerances of tests/test_gpu_mlp_listwise.py::_close_module (fp32 against fp32)."""
    assert torch.allclose(got.detach(), want.detach(), rtol=1e-4 if listmle else 1e-5, atol=1e-4 if listmle else 1e-6), \
        (got - want).abs().max().item()
    scale = max(float(p.grad.abs().max()) for p in plain.parameters())
    for a, b in zip(ours.parameters(), plain.parameters()):
        assert a.grad is not None
        assert torch.allclose(a.grad, b.grad, rtol=2e-4, atol=2e-5 * max(1.0, scale)), (a.grad - b.grad).abs().max().item()


@pytest.mark.parametrize("name,shape", [("hinge", (4, 300, 24)), ("listmle", (4, 300, 24)), ("logistic-long", (2, 4200, 8))])
def test_module_agrees_with_the_torch_layers(name, shape):
    from pytorchltr_amd.loss import ListMLELoss, PairwiseHingeLoss, PairwiseLogisticLoss
    from pytorchltr_amd.utils import tie_breaking
    loss_fn = {"hinge": PairwiseHingeLoss, "listmle": ListMLELoss,
               "logistic-long": lambda: PairwiseLogisticLoss(long_lists=True)}[name]()
    B, L, F = shape
    rng = np.random.default_rng(L + F)
    dev = _dev()
    tX = torch.from_numpy(rng.normal(0.0, 1.0, shape).astype(np.float32)).to(dev)
    ty = torch.from_numpy(rng.integers(0, 5, (B, L))).to(dev)
    n = rng.integers(2, L + 1, B)
    n[0] = L
    tn = torch.from_numpy(n).to(dev)
    ours, plain = _module_pair(F)
    with tie_breaking("index"):
        want = loss_fn(plain(tX), ty, tn).mean()
        want.backward()
        scores = ours(tX, tn)
        assert scores.shape == (B, L, 1)
        got = loss_fn(scores, ty, tn).mean()
        got.backward()
    _close_module(ours, plain, got, want, name == "listmle")
    real = torch.arange(L, device=dev)[None, :] < tn[:, None]
    assert not scores.detach().squeeze(-1)[~real].any()
    assert torch.allclose(scores.detach().squeeze(-1)[real], plain(tX).detach().squeeze(-1)[real], rtol=1e-5, atol=1e-5)


def test_module_pads_features_and_leaves_other_inputs_to_the_torch_layers():
    from pytorchltr_amd.fused import MLPScorer
    dev = _dev()
    torch.manual_seed(5)
    m = MLPScorer(46, (17, 5)).to(dev)
    X = torch.randn(3, 40, 46, device=dev)
    up = torch.randn(3, 40, 1, device=dev)
    m(X).backward(up)
    got = [p.grad.clone() for p in m.parameters()]
    m.zero_grad()
    Xg = X.clone().requires_grad_(True)                # features that need a gradient: the torch layers
    m(Xg).backward(up)
    assert Xg.grad is not None
    for a, p in zip(got, m.parameters()):
        assert a.shape == p.shape and torch.allclose(a, p.grad, rtol=2e-4, atol=2e-5)


# ---- 7. routing ----
def _no_torch_layers(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError("torch.nn.functional.linear was called")
    monkeypatch.setattr(torch.nn.functional, "linear", refuse)


def _batch(B, L, F, seed):
    rng = np.random.default_rng(seed)
    X = rng.normal(0.0, 1.0, (B, L, F)).astype(np.float32)
    y = rng.integers(0, 5, (B, L))
    n = rng.integers(2, L + 1, B)
    n[0] = L
    return X, y, n


@pytest.mark.parametrize("which", ["pairwise", "listwise"])
def test_long_lists_do_not_touch_the_torch_layers(which, monkeypatch):
    from pytorchltr_amd.fused import FusedMLPListwiseLoss, FusedMLPLoss
    from pytorchltr_amd.utils import tie_breaking
    dev = _dev()
    X, y, n = _batch(3, 300, 24, 11)
    tX, ty, tn = [torch.from_numpy(a).to(dev) for a in (X, y, n)]
    torch.manual_seed(1)
    m = (FusedMLPLoss(24, "hinge") if which == "pairwise" else FusedMLPListwiseLoss(24, "listmle")).to(dev)
    _no_torch_layers(monkeypatch)
    with tie_breaking("index"):
        out = m(tX, ty, tn)
        out.backward()
    assert out.dim() == 0 and torch.isfinite(out) and m.last_losses.shape == (3,)
    for p in m.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all()
    assert float(m.l1.weight.grad.abs().max()) > 0


def test_score_of_long_lists_without_grad_is_the_row_kernel(monkeypatch):
    from pytorchltr_amd.fused import FusedMLPLoss
    dev = _dev()
    case = _case(2, 300, 24, 50, 10, (300, 129))
    m = FusedMLPLoss(24, "hinge").to(dev)
    with torch.no_grad():
        for p, v in zip(m.parameters(), case["params"]):
            p.copy_(torch.from_numpy(v).reshape(p.shape))
    tX, _, tn, _ = _device_args(case)
    _no_torch_layers(monkeypatch)
    with torch.no_grad():
        got = m.score(tX, tn)
    assert got.shape == (2, 300, 1)
    got = got.squeeze(-1).cpu().numpy()
    real = case["real"]
    assert np.allclose(got[real], case["scores"][real], rtol=1e-5, atol=2e-6) and not got[~real].any()


# ---- 8. mlp_loss_step past the limits ----
@pytest.mark.parametrize("kind", ["hinge", "ndcg2"])
def test_loss_step_past_the_limits_pairwise(kind):
    from tests.test_gpu_mlp import _case as mlp_case, _check
    _check(kind, *mlp_case(6, 300, 24, 50, 10, 31))


def test_loss_step_past_the_limits_listmle():
    from pytorchltr_amd.utils import tie_breaking
    from tests.test_gpu_mlp_listwise import LISTMLE, _compare as lw_compare, _data, _reference, _step
    key = (6, 300, 24, 50, 10)
    X, y, n, params = _data(*key)
    with tie_breaking("index"):
        got = _step(LISTMLE, X, y, n, params)
    lw_compare(LISTMLE, got, _reference(LISTMLE, None, key), n, key[1])


def test_loss_step_keeps_refusing_other_networks():
    from pytorchltr_amd import fused
    dev = _dev()
    rng = np.random.default_rng(2)
    y, n = torch.zeros(2, 300, dtype=torch.int64, device=dev), torch.tensor([300, 5], device=dev)
    for F, H1, H2 in ((6, 5, 3), (228, 5, 3), (8, 65, 3)):
        P = [torch.from_numpy(p).to(dev) for p in _params(F, H1, H2, rng)]
        with pytest.raises(ValueError):
            fused.mlp_loss_step(torch.zeros(2, 300, F, device=dev), P, y, n)
        with pytest.raises(ValueError):
            fused.mlp_scores(torch.zeros(2, 300, F, device=dev), P, n)


# ---- 9. capture and replay ----
def test_capture_and_replay():
    """MLPScorer forward + backward captured with torch.cuda.graph and replayed twice: the eager result bit for bit."""
    from pytorchltr_amd.fused import MLPScorer
    dev = _dev()
    case = _case(5, 300, 136, 50, 10, "ragged")
    tX, _, tn, tg = _device_args(case)
    torch.manual_seed(7)
    m = MLPScorer(136).to(dev)

    def step():
        s = m(tX, tn)
        s.backward(tg.unsqueeze(-1))
        return s.detach()

    def grads():
        return [p.grad for p in m.parameters()]

    eager = [step().clone()] + [g.clone() for g in grads()]
    m.zero_grad(set_to_none=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                      # (warm-up on a side stream, as torch asks)
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
