"""GPU tier of the MLP scorer on bf16 feature batches (run with `-m gpu` on an MI355X): ltr_mlp_bf16_scores and
ltr_mlp_bf16_grad (include/ltr_mlp_bf16.h) through fused.mlp_scores_bf16 / fused.mlp_grad_bf16, and the modules
(MLPScorer, FusedMLPLoss, FusedMLPListwiseLoss) on a torch.bfloat16 batch.

Reference and tolerances: tests/test_mlp_bf16_host.py::_case -- the three layers in torch float64 on the CPU on the
bf16-rounded X and the bf16-rounded W1, loss = (s * g).sum(), autograd; scores rtol 1e-5 / atol 2e-6, padded scores
exactly 0; every gradient tensor <= 2e-5 * max(max|that tensor|, max|any gradient| / 4) + 1e-6.  The shapes are the
smallest at which the kernels can still go wrong; 3 x 70 x 136 at 64-16 is the one at which the host tier shows that a
single bf16 term of d loss / d H1 misses the dW1 tolerance."""
import numpy as np
import pytest
import torch

from tests.test_mlp_bf16_host import EMULATED, _case, _errors, _params

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tier needs a ROCm device"
    return torch.device("cuda:0")


def _device_args(case, X=None, g=None):
    dev = _dev()
    tX = torch.from_numpy(case["X"] if X is None else X).to(dev).bfloat16()        # (exact: the values are bf16)
    tP = [torch.from_numpy(p).to(dev) for p in case["params"]]
    tn = None if case["n"] is None else torch.from_numpy(case["n"]).to(dev)
    tg = torch.from_numpy(case["g"] if g is None else g).to(dev)
    return tX, tP, tn, tg


def _run(case, X=None, g=None):
    """(scores (B, L), six gradients) from the two bf16 kernels."""
    from pytorchltr_amd import fused
    tX, tP, tn, tg = _device_args(case, X, g)
    scores = fused.mlp_scores_bf16(tX, tP, tn)
    grads = fused.mlp_grad_bf16(tX, tP, tg, tn)
    torch.cuda.synchronize()
    return scores, grads


def _compare(case, scores, grads):
    got_s = scores.cpu().numpy()
    assert got_s.dtype == np.float32 and got_s.shape == case["real"].shape
    assert not got_s[~case["real"]].any()                                # padded documents: exactly 0
    for name, err, tol in _errors(case, got_s, [t.cpu().numpy() for t in grads]):
        print("%s err %.3g tol %.3g" % (name, err, tol))
        assert err <= tol, (name, err, tol)
    for got, want in zip(grads, case["grads"]):
        assert got.dtype is torch.float32 and tuple(got.shape) == want.shape


# ---- 1. tiles against queries ----
@pytest.mark.parametrize("key", [
    (5, 33, 136, 50, 10, "ragged"),                # a query spans tiles, a tile spans queries; n = 0, 1, L, L + 5
    (3, 16, 8, 50, 10, "ragged"),                  # less than two tiles
    (1, 1, 8, 50, 10, (1,)),                       # one row
    (2, 96, 40, 50, 10, (96, 0)),                  # a whole tile, and a 16-row subtile, of padding
    (5, 33, 136, 50, 10, None),                    # n == NULL: every row is real
    (3, 16, 8, 50, 10, None),
    EMULATED + ("ragged",),                        # where a single bf16 term of dH1 misses the tolerance
], ids=["5x33", "3x16", "1x1", "2x96-padding", "5x33-no-n", "3x16-no-n", "3x70"])
def test_tiles_against_queries(key):
    case = _case(*key)
    _compare(case, *_run(case))


# ---- 2. every K-step count and its padding ----
@pytest.mark.parametrize("F,H1,H2", [(F, 64, 16) for F in (8, 24, 32, 40, 64, 72, 136, 160, 168, 216, 224)]
                         + [(8, 1, 1), (8, 50, 10)])
def test_every_k_step_count_and_its_padding(F, H1, H2):
    case = _case(4, 50, F, H1, H2, "ragged")
    _compare(case, *_run(case))


# ---- 3. more tiles than workgroups ----
def test_more_tiles_than_workgroups():
    # 40 x 1000 = 40 000 flat rows = 1250 tiles of 32 rows; a launch has at most 2 workgroups x 256 CUs = 512, so every
    # workgroup carries its dW1 tile, the g ring and the look-ahead fill over two or three tiles; g is non-zero on
    # every 7th real row
    case = _case(40, 1000, 8, 4, 4, "ragged", 7)
    assert case["real"].sum() > 512 * 32 // 2
    _compare(case, *_run(case))


# ---- 4. padding is not read ----
def test_padding_is_not_read():
    case = _case(5, 33, 136, 50, 10, "ragged")
    real = case["real"]
    Xn = case["X"].copy()
    Xn[~real] = np.nan
    gn = case["g"].copy()
    gn[~real] = np.nan
    assert np.isnan(Xn).any() and np.isnan(gn).any()
    s0, g0 = _run(case)
    s1, g1 = _run(case, X=Xn, g=gn)
    assert torch.equal(s0, s1)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)


# ---- 5. determinism ----
def test_deterministic():
    for key in ((40, 1000, 8, 4, 4, "ragged", 7), (5, 33, 136, 50, 10, "ragged")):
        case = _case(*key)
        s0, g0 = _run(case)
        s1, g1 = _run(case)
        assert torch.equal(s0, s1)
        for a, b in zip(g0, g1):
            assert torch.equal(a, b)


def test_an_empty_batch_gives_zero_gradients():
    from pytorchltr_amd import _C, fused
    dev = _dev()
    tP = [torch.from_numpy(p).to(dev) for p in _params(8, 5, 3, np.random.default_rng(0))]
    out = torch.full((8 * 5 + 5 + 5 * 3 + 3 + 3 + 1,), float("nan"), device=dev)
    x0 = torch.zeros(0, 7, 8, device=dev, dtype=torch.bfloat16)
    grads = fused.mlp_grad_bf16(x0, tP, torch.zeros(0, 7, device=dev), out=out)
    assert fused.mlp_scores_bf16(x0, tP).shape == (0, 7)
    torch.cuda.synchronize()
    assert not out.any() and grads[0].shape == (5, 8)
    # the C ABI itself: B == 0 returns LTR_OK from both calls (no data pointers, no workspace) and zeroes the gradients
    lib, st = _C.lib(), _C.stream_of(out)
    ptrs = [t.data_ptr() for t in tP]
    out.fill_(float("nan"))
    assert lib.ltr_mlp_bf16_grad(None, *ptrs, None, None, 0, 7, 8, 5, 3, out.data_ptr(), None, 0, st) == 0
    assert lib.ltr_mlp_bf16_scores(None, *ptrs, None, 0, 7, 8, 5, 3, None, st) == 0
    torch.cuda.synchronize()
    assert not out.any()


# ---- 6. capture and replay ----
def test_capture_and_replay():
    """Both calls recorded into one graph (one stream, no branches) and replayed twice on changed inputs: the eager
    results bit for bit."""
    from pytorchltr_amd import fused
    dev = _dev()
    case = _case(5, 33, 136, 50, 10, "ragged")
    tX, tP, tn, tg = _device_args(case)
    inputs = []
    for seed in (1, 2):
        gen = torch.Generator(device="cpu").manual_seed(seed)
        inputs.append((torch.randn(tX.shape, generator=gen).to(dev).bfloat16(), torch.randn(tg.shape, generator=gen).to(dev)))
    eager = []
    for X, g in inputs:
        s = fused.mlp_scores_bf16(X, tP, tn)
        eager.append((s, [t.clone() for t in fused.mlp_grad_bf16(X, tP, g, tn)]))
    torch.cuda.synchronize()
    flat = torch.empty(sum(p.numel() for p in tP), device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        cap_s = fused.mlp_scores_bf16(tX, tP, tn)
        cap_g = fused.mlp_grad_bf16(tX, tP, tg, tn, out=flat)
    for (X, g), (want_s, want_g) in zip(inputs, eager):
        tX.copy_(X)
        tg.copy_(g)
        cap_s.fill_(float("nan"))
        flat.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap_s, want_s)
        for a, b in zip(cap_g, want_g):
            assert torch.equal(a, b)


# ---- 7. the modules on a bf16 batch ----
def _no_torch_layers(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError("torch.nn.functional.linear was called")
    monkeypatch.setattr(torch.nn.functional, "linear", refuse)


def _float64_layers(m):
    """The module's three torch layers in float64, W1 rounded to bf16."""
    H1, H2, F = m.l1.out_features, m.l2.out_features, m.l1.in_features
    plain = torch.nn.Sequential(torch.nn.Linear(F, H1), torch.nn.ReLU(), torch.nn.Linear(H1, H2), torch.nn.ReLU(),
                                torch.nn.Linear(H2, 1)).to(_dev())
    for src, dst in ((m.l1, plain[0]), (m.l2, plain[2]), (m.l3, plain[4])):
        dst.load_state_dict(src.state_dict())
    with torch.no_grad():
        plain[0].weight.copy_(plain[0].weight.bfloat16().float())
    return plain.double()


def _close_module(ours, plain, got, want, listmle):
    """The tolerances of tests/test_gpu_mlp_rows.py::_close_module."""
    want = want.detach().float()
    assert torch.allclose(got.detach(), want, rtol=1e-4 if listmle else 1e-5, atol=1e-4 if listmle else 1e-6), \
        (got - want).abs().max().item()
    scale = max(float(p.grad.abs().max()) for p in plain.parameters())
    for a, b in zip(ours.parameters(), plain.parameters()):
        assert a.grad is not None and a.grad.shape == a.shape and a.grad.dtype is torch.float32
        assert torch.allclose(a.grad, b.grad.float(), rtol=2e-4, atol=2e-5 * max(1.0, scale)), \
            (a.grad - b.grad.float()).abs().max().item()


def test_scorer_module_pads_to_8_and_crops_the_gradient(monkeypatch):
    from pytorchltr_amd.fused import MLPScorer
    dev = _dev()
    torch.manual_seed(5)
    m = MLPScorer(46, (17, 5)).to(dev)
    X = torch.randn(3, 40, 46, device=dev).bfloat16()
    tn = torch.tensor([40, 0, 17], device=dev)
    up = torch.randn(3, 40, 1, device=dev)
    plain = _float64_layers(m)
    real = (torch.arange(40, device=dev)[None, :] < tn[:, None]).unsqueeze(-1)
    want_s = torch.where(real, plain(X.double()), 0.0)
    want = (want_s * up.double()).sum()
    want.backward()
    _no_torch_layers(monkeypatch)
    scores = m(X, tn)
    assert scores.shape == (3, 40, 1) and scores.dtype is torch.float32
    got = (scores * up).sum()
    got.backward()
    assert torch.allclose(scores.detach(), want_s.detach().float(), rtol=1e-5, atol=2e-6)
    assert not scores.detach()[~real].any()
    _close_module(m, plain, got, want, False)
    with torch.no_grad():                                               # without gradients: the score kernel alone
        assert torch.equal(m(X, tn), scores.detach())


@pytest.mark.parametrize("which,shape", [("hinge", (4, 300, 24)), ("listmle", (4, 300, 24)), ("hinge", (4, 60, 24))],
                         ids=["hinge-300", "listmle-300", "hinge-60"])
def test_loss_modules_on_a_bf16_batch(which, shape, monkeypatch):
    from pytorchltr_amd.fused import FusedMLPListwiseLoss, FusedMLPLoss
    from pytorchltr_amd.loss import ListMLELoss, PairwiseHingeLoss
    from pytorchltr_amd.utils import tie_breaking
    dev = _dev()
    B, L, F = shape
    rng = np.random.default_rng(L + F)
    tX = torch.from_numpy(rng.normal(0.0, 1.0, shape).astype(np.float32)).to(dev).bfloat16()
    ty = torch.from_numpy(rng.integers(0, 5, (B, L))).to(dev)
    n = rng.integers(2, L + 1, B)
    n[0] = L
    tn = torch.from_numpy(n).to(dev)
    torch.manual_seed(1)
    m = (FusedMLPLoss(F, "hinge") if which == "hinge" else FusedMLPListwiseLoss(F, "listmle")).to(dev)
    plain = _float64_layers(m)
    loss_fn = PairwiseHingeLoss() if which == "hinge" else ListMLELoss()
    with tie_breaking("index"):
        # the module's torch layers in float64; the loss itself is the fp32 HIP loss kernel on both sides
        want_s = plain(tX.double())
        want = loss_fn(want_s.float(), ty, tn).mean()
        want.backward()
        _no_torch_layers(monkeypatch)
        got = m(tX, ty, tn)
        got.backward()
        with torch.no_grad():
            s = m.score(tX, tn)
    assert got.dim() == 0 and m.last_losses.shape == (B,)
    _close_module(m, plain, got, want, which == "listmle")
    real = torch.arange(L, device=dev)[None, :] < tn[:, None]
    assert s.shape == (B, L, 1) and not s.squeeze(-1)[~real].any()
    assert torch.allclose(s.squeeze(-1)[real], want_s.detach().float().squeeze(-1)[real], rtol=1e-5, atol=2e-6)


def test_loss_step_on_a_bf16_batch_is_the_module_s_step():
    from pytorchltr_amd import fused
    dev = _dev()
    case = _case(4, 50, 24, 64, 16, "ragged")
    tX, tP, tn, _ = _device_args(case)
    ty = torch.from_numpy(np.random.default_rng(3).integers(0, 5, (4, 50))).to(dev)
    lossv, grads, scores = fused.mlp_loss_step(tX, tP, ty, tn, loss="hinge", return_scores=True)
    assert torch.equal(scores, fused.mlp_scores_bf16(tX, tP, tn))
    m = fused.FusedMLPLoss(24, "hinge", hidden=(64, 16)).to(dev)
    with torch.no_grad():
        for p, v in zip(m.parameters(), tP):
            p.copy_(v.reshape(p.shape))
    total = m(tX, ty, tn)
    total.backward()
    assert torch.allclose(total, lossv.mean(), rtol=1e-6, atol=1e-7)
    for p, gr in zip(m.parameters(), grads):
        assert torch.allclose(p.grad, gr.reshape(p.shape), rtol=1e-5, atol=1e-6)


def test_networks_past_the_limits_raise_value_error():
    from pytorchltr_amd.fused import FusedMLPLoss, MLPScorer
    dev = _dev()
    y, n = torch.zeros(2, 10, dtype=torch.int64, device=dev), torch.tensor([10, 5], device=dev)
    for F, hidden in ((228, (5, 3)), (16, (65, 3)), (16, (5, 17))):
        X = torch.zeros(2, 10, F, device=dev, dtype=torch.bfloat16)
        with pytest.raises(ValueError, match="bf16 MLP kernels"):
            MLPScorer(F, hidden).to(dev)(X, n)
        with pytest.raises(ValueError, match="bf16 MLP kernels"):
            FusedMLPLoss(F, "hinge", hidden=hidden).to(dev)(X, y, n)


# ---- 8. existing paths are not rerouted ----
def test_an_fp32_batch_still_reaches_the_fp32_row_kernels(monkeypatch):
    from pytorchltr_amd import _C
    from pytorchltr_amd.fused import FusedMLPLoss, MLPScorer
    dev = _dev()
    lib = _C.lib()
    called = []

    def spy(name):
        fn = getattr(lib, name)

        def wrapper(*args):
            called.append(name)
            return fn(*args)
        monkeypatch.setattr(lib, name, wrapper)
    for name in ("ltr_mlp_rows_scores_f32", "ltr_mlp_rows_grad_f32", "ltr_mlp_bf16_scores", "ltr_mlp_bf16_grad"):
        spy(name)
    rng = np.random.default_rng(4)
    X = torch.from_numpy(rng.normal(0.0, 1.0, (3, 300, 24)).astype(np.float32)).to(dev)
    ty = torch.from_numpy(rng.integers(0, 5, (3, 300))).to(dev)
    tn = torch.tensor([300, 17, 129], device=dev)
    torch.manual_seed(2)
    MLPScorer(24).to(dev)(X, tn).sum().backward()
    FusedMLPLoss(24, "hinge").to(dev)(X, ty, tn).backward()
    assert called == ["ltr_mlp_rows_scores_f32", "ltr_mlp_rows_grad_f32"] * 2
    del called[:]
    MLPScorer(24).to(dev)(X.bfloat16(), tn).sum().backward()
    FusedMLPLoss(24, "hinge").to(dev)(X.bfloat16(), ty, tn).backward()
    assert called == ["ltr_mlp_bf16_scores", "ltr_mlp_bf16_grad"] * 2


@pytest.mark.parametrize("L", [60, 300])
def test_mlp_scores_on_a_bf16_batch_keeps_the_full_precision_w1(L):
    from pytorchltr_amd import fused
    case = _case(4, L, 24, 50, 10, "ragged")
    tX, tP, tn, tg = _device_args(case)
    assert torch.equal(fused.mlp_scores(tX, tP, tn), fused.mlp_scores(tX.float(), tP, tn))
    if L == 300:
        for a, b in zip(fused.mlp_grad(tX, tP, tg, tn), fused.mlp_grad(tX.float(), tP, tg, tn)):
            assert torch.equal(a, b)
