"""GPU tier of the wide-row MLP scorer (run with `-m gpu` on an MI355X): ltr_mlp_wide_scores_f32 and
ltr_mlp_wide_grad_f32 (include/ltr_mlp_wide.h) on prepared arguments, fused.mlp_wide_scores / fused.mlp_wide_grad, and
the modules routed to them (MLPScorer, FusedMLPLoss, FusedMLPListwiseLoss, score()) at 228 .. 704 features.

Reference, cases and tolerances are those of tests/test_gpu_mlp_rows.py: the three layers in torch float64 on the CPU;
scores rtol 1e-5 / atol 2e-6 with padded scores exactly 0; every gradient tensor
<= 2e-5 * max(max|that tensor|, max|any gradient| / 4) + 1e-6.  A plain fp32 torch evaluation of these cases at
F = 228 .. 1024 stays below 0.07 of the score tolerance and 0.04 of the gradient tolerances, so they leave room for
another summation order and are not widened.

The kernels walk the features in chunks of 128, the upper 64 of which are skipped when the row ends below them; the
dW1 kernel takes column slices of 128 or 176 features, 1 .. 4 of them (first feature count of each plan: 132, 180, 260,
356, 388, 532)."""
import numpy as np
import pytest
import torch

from tests.test_gpu_mlp_rows import (_case, _close_module, _compare, _dev, _device_args, _module_pair, _no_torch_layers,
                                     _params)

pytestmark = pytest.mark.gpu


def _run(case, X=None, g=None):
    """(scores (B, L), six gradients) from the wide entry points, at any F they take (also F <= 224)."""
    from pytorchltr_amd import fused
    tX, tP, tn, tg = _device_args(case, X, g)
    H1, H2 = tP[0].shape[0], tP[2].shape[0]
    scores = fused._mlp_rows_scores(tX, tP, H1, H2, tn, wide=True)
    grads = fused._mlp_grad_call(tX, tP, H1, H2, tg, tn, None, True)
    torch.cuda.synchronize()
    return scores, grads


def _cus():
    return torch.cuda.get_device_properties(_dev()).multi_processor_count


# ---- 1. chunk boundaries ----
CHUNK = 128
WIDTHS = sorted(F for F in set(
    [8, 224, 228, 232, 448, 452, 700, 704]
    + [k * CHUNK + d for k in range(1, 6) for d in (-4, 0, 4)]                # a chunk ends
    + [k * CHUNK + CHUNK // 2 + d for k in range(0, 6) for d in (0, 4)]       # the upper half of a chunk begins
    + [176, 180, 352, 356, 528, 532]) if F <= 704)                            # the dW1 kernel takes another plan


@pytest.mark.parametrize("F,H1,H2", [(F, 64, 16) for F in WIDTHS] + [(228, 1, 1), (700, 50, 10)])
def test_chunk_boundaries(F, H1, H2):
    # a full list and one that ends inside subtile 0 of a tile (150 + 97 = 7 * 32 + 23): 247 real rows, both subtiles
    case = _case(2, 150, F, H1, H2, (150, 97))
    assert case["real"].sum() == 247
    _compare(case, *_run(case))


# ---- 2. tiles against queries ----
@pytest.mark.parametrize("key", [
    (3, 37, 228, 5, 3, (37, 20, 37)),              # one tile of 32 rows holds three queries
    (2, 300, 228, 50, 10, (300, 129)),             # tiles straddle the query boundary; one document in a further tile
    (3, 37, 228, 5, 3, None),                      # n == NULL: every row is real
    (2, 300, 228, 50, 10, None),
], ids=["3x37", "2x300", "3x37-no-n", "2x300-no-n"])
def test_tiles_against_queries(key):
    case = _case(*key)
    _compare(case, *_run(case))


# ---- 3. several tiles and tile groups per workgroup ----
@pytest.mark.parametrize("F", [452, 700])
def test_several_tiles_per_workgroup(F):
    # 7 x 5000 = 35 000 flat rows = 1094 tiles, more than twice the 2 x CUs workgroups of a launch: a workgroup carries
    # two or three tiles (a partly filled group) through every chunk; n = 0, 1, L, L + 5 and random lengths
    case = _case(7, 5000, F, 50, 10, "ragged")
    assert 1094 > 2 * 2 * _cus()
    assert case["real"].sum() > 5000 and (case["n"][:4] == (0, 1, 5000, 5005)).all()
    _compare(case, *_run(case))


def test_several_groups_per_workgroup():
    # 30 x 5000 = 150 000 flat rows = 4688 tiles, more than eight per workgroup of a full grid: the score kernel runs a
    # full group of eight tiles and a partly filled one, the gradient's forward kernel two groups of four and a partly
    # filled one; 136 features are two chunks (128 + 8), so the accumulators of a group cross a chunk
    case = _case(30, 5000, 136, 50, 10, "ragged")
    tiles = (30 * 5000 + 31) // 32
    assert tiles > 8 * 2 * _cus() and tiles % (2 * _cus()) != 0
    _compare(case, *_run(case))


# ---- 4. padding is not read ----
def test_padding_is_not_read():
    case = _case(5, 300, 700, 50, 10, "ragged")
    real = case["real"]
    Xn = case["X"].copy()
    Xn[~real] = np.nan
    gn = case["g"].copy()
    gn[~real] = np.nan
    assert np.isnan(Xn).any() and np.isnan(gn).any()
    s0, g0 = _run(case)
    s1, g1 = _run(case, X=Xn, g=gn)
    _compare(case, s1, g1)
    mask = torch.from_numpy(real).to(_dev())
    assert torch.equal(s0[mask], s1[mask]) and not s1[~mask].any()
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)


# ---- 5. determinism ----
@pytest.mark.parametrize("key", [(7, 5000, 452, 50, 10, "ragged"), (5, 300, 700, 50, 10, "ragged")], ids=["7x5000", "5x300"])
def test_deterministic(key):
    case = _case(*key)
    s0, g0 = _run(case)
    s1, g1 = _run(case)
    assert torch.equal(s0, s1)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)


# ---- 6. empty batch ----
def test_an_empty_batch_gives_zero_gradients():
    from pytorchltr_amd import _C, fused
    dev = _dev()
    F, H1, H2 = 228, 5, 3
    tP = [torch.from_numpy(p).to(dev) for p in _params(F, H1, H2, np.random.default_rng(0))]
    out = torch.full((F * H1 + H1 + H1 * H2 + H2 + H2 + 1,), float("nan"), device=dev)
    grads = fused.mlp_wide_grad(torch.zeros(0, 7, F, device=dev), tP, torch.zeros(0, 7, device=dev), out=out)
    assert fused.mlp_wide_scores(torch.zeros(0, 7, F, device=dev), tP).shape == (0, 7)
    torch.cuda.synchronize()
    assert not out.any() and grads[0].shape == (H1, F)
    # the C ABI itself: B == 0 returns LTR_OK from both calls (no data pointers, no workspace) and zeroes the gradients
    lib, st = _C.lib(), _C.stream_of(out)
    ptrs = [t.data_ptr() for t in tP]
    out.fill_(float("nan"))
    assert lib.ltr_mlp_wide_grad_f32(None, *ptrs, None, None, 0, 7, F, H1, H2, out.data_ptr(), None, 0, st) == 0
    assert lib.ltr_mlp_wide_scores_f32(None, *ptrs, None, 0, 7, F, H1, H2, None, st) == 0
    torch.cuda.synchronize()
    assert not out.any()


# ---- 7. F <= 224 through the wide entry points ----
@pytest.mark.parametrize("F", [8, 136, 224])
def test_narrow_rows_agree_with_the_row_kernels(F):
    from pytorchltr_amd import fused
    case = _case(5, 300, F, 50, 10, "ragged")
    scores, grads = _run(case)
    _compare(case, scores, grads)
    tX, tP, tn, tg = _device_args(case)
    rows_s = fused._mlp_rows_scores(tX, tP, 50, 10, tn)
    rows_g = fused.mlp_grad(tX, tP, tg, tn)
    torch.cuda.synchronize()
    real = torch.from_numpy(case["real"]).to(_dev())
    assert torch.allclose(scores[real], rows_s[real], rtol=1e-5, atol=2e-6) and not scores[~real].any()
    scale = max(float(w.abs().max()) for w in rows_g)
    for a, b in zip(grads, rows_g):
        assert float((a - b).abs().max()) <= 2e-5 * max(float(b.abs().max()), 0.25 * scale) + 1e-6


# ---- 8. modules ----
def test_function_level_api():
    from pytorchltr_amd import fused
    case = _case(2, 300, 228, 50, 10, (300, 129))
    tX, tP, tn, tg = _device_args(case)
    scores = fused.mlp_wide_scores(tX, tP, tn)
    grads = fused.mlp_wide_grad(tX, tP, tg.unsqueeze(-1), tn)
    torch.cuda.synchronize()
    _compare(case, scores, grads)
    narrow = _case(2, 150, 224, 64, 16, (150, 97))
    nX, nP, nn_, ng = _device_args(narrow)
    with pytest.raises(ValueError):
        fused.mlp_wide_scores(nX, nP, nn_)
    with pytest.raises(ValueError):
        fused.mlp_wide_grad(nX, nP, ng, nn_)
    with pytest.raises(ValueError):                    # the row API keeps its documented limit
        fused.mlp_grad(tX, tP, tg, tn)


@pytest.mark.parametrize("name", ["hinge", "listmle"])
def test_module_agrees_with_the_torch_layers(name):
    from pytorchltr_amd.loss import ListMLELoss, PairwiseHingeLoss
    from pytorchltr_amd.utils import tie_breaking
    loss_fn = {"hinge": PairwiseHingeLoss, "listmle": ListMLELoss}[name]()
    B, L, F = 4, 300, 699                              # padded to 700 on the fly
    rng = np.random.default_rng(L + F)
    dev = _dev()
    tX = torch.from_numpy(rng.normal(0.0, 1.0, (B, L, F)).astype(np.float32)).to(dev)
    ty = torch.from_numpy(rng.integers(0, 5, (B, L))).to(dev)
    n = rng.integers(2, L + 1, B)
    n[0] = L
    tn = torch.from_numpy(n).to(dev)
    ours, plain = _module_pair(F)
    with tie_breaking("index"):
        want = loss_fn(plain(tX), ty, tn).mean()
        want.backward()
        scores = ours(tX, tn)
        assert scores.shape == (B, L, 1) and scores.grad_fn is not None
        assert "MLPScoreFunction" in type(scores.grad_fn).__name__
        got = loss_fn(scores, ty, tn).mean()
        got.backward()
    assert ours.l1.weight.grad.shape == (50, 699)
    _close_module(ours, plain, got, want, name == "listmle")
    real = torch.arange(L, device=dev)[None, :] < tn[:, None]
    assert not scores.detach().squeeze(-1)[~real].any()
    assert torch.allclose(scores.detach().squeeze(-1)[real], plain(tX).detach().squeeze(-1)[real], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("which,F,L", [("pairwise", 700, 40), ("pairwise", 700, 300), ("listwise", 228, 300)])
def test_loss_modules_do_not_touch_the_torch_layers(which, F, L, monkeypatch):
    from pytorchltr_amd.fused import FusedMLPListwiseLoss, FusedMLPLoss
    from pytorchltr_amd.utils import tie_breaking
    dev = _dev()
    rng = np.random.default_rng(F + L)
    tX = torch.from_numpy(rng.normal(0.0, 1.0, (3, L, F)).astype(np.float32)).to(dev)
    ty = torch.from_numpy(rng.integers(0, 5, (3, L))).to(dev)
    n = rng.integers(2, L + 1, 3)
    n[0] = L
    tn = torch.from_numpy(n).to(dev)
    torch.manual_seed(1)
    m = (FusedMLPLoss(F, "hinge") if which == "pairwise" else FusedMLPListwiseLoss(F, "listmle")).to(dev)
    _no_torch_layers(monkeypatch)
    with tie_breaking("index"):
        out = m(tX, ty, tn)
        out.backward()
    assert out.dim() == 0 and torch.isfinite(out) and m.last_losses.shape == (3,)
    for p in m.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all()
    assert float(m.l1.weight.grad.abs().max()) > 0


def test_score_without_grad_is_the_wide_kernel(monkeypatch):
    from pytorchltr_amd.fused import FusedMLPLoss
    dev = _dev()
    case = _case(2, 300, 228, 50, 10, (300, 129))
    m = FusedMLPLoss(228, "hinge").to(dev)
    with torch.no_grad():
        for p, v in zip(m.parameters(), case["params"]):
            p.copy_(torch.from_numpy(v).reshape(p.shape))
    tX, _, tn, _ = _device_args(case)
    _no_torch_layers(monkeypatch)
    with torch.no_grad():
        got = m.score(tX, tn)
        short = m.score(tX[:, :40].contiguous(), torch.tensor([40, 7], device=dev))     # a short list as well
    assert got.shape == (2, 300, 1) and short.shape == (2, 40, 1)
    got = got.squeeze(-1).cpu().numpy()
    real = case["real"]
    assert np.allclose(got[real], case["scores"][real], rtol=1e-5, atol=2e-6) and not got[~real].any()
    short = short.squeeze(-1).cpu().numpy()
    assert np.allclose(short[0], case["scores"][0, :40], rtol=1e-5, atol=2e-6)
    assert np.allclose(short[1, :7], case["scores"][1, :7], rtol=1e-5, atol=2e-6) and not short[1, 7:].any()


def test_features_that_require_a_gradient_stay_on_the_torch_layers():
    from pytorchltr_amd.fused import MLPScorer
    dev = _dev()
    torch.manual_seed(5)
    m = MLPScorer(228, (17, 5)).to(dev)
    X = torch.randn(3, 40, 228, device=dev)
    up = torch.randn(3, 40, 1, device=dev)
    m(X).backward(up)
    got = [p.grad.clone() for p in m.parameters()]
    m.zero_grad()
    Xg = X.clone().requires_grad_(True)
    m(Xg).backward(up)
    assert Xg.grad is not None and float(Xg.grad.abs().max()) > 0
    for a, p in zip(got, m.parameters()):
        assert a.shape == p.shape and torch.allclose(a, p.grad, rtol=2e-4, atol=2e-5)


# ---- 9. capture and replay ----
def test_capture_and_replay():
    """MLPScorer(700) forward + backward captured with torch.cuda.graph and replayed twice: the eager result bit for bit."""
    from pytorchltr_amd.fused import MLPScorer
    dev = _dev()
    case = _case(5, 300, 700, 50, 10, "ragged")
    tX, _, tn, tg = _device_args(case)
    torch.manual_seed(7)
    m = MLPScorer(700).to(dev)

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
