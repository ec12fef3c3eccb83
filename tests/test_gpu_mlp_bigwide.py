"""GPU tier of the MLP scorer with wide hidden layers on wide rows (run with `-m gpu` on an MI355X):
ltr_mlp_bigwide_scores_f32 and ltr_mlp_bigwide_grad_f32 (include/ltr_mlp_bigwide.h) through the launchers with
family=_MLP_BIG_WIDE, and the opt-in route ``big_hidden_wide=True`` of MLPScorer, the loss modules, mlp_loss_step and
MLPTrainer.

Reference and tolerances: those of tests/test_gpu_mlp_rows.py, unchanged -- the three layers in float64, scores rtol 1e-5 /
atol 2e-6, padded scores exactly 0, every gradient tensor <= 2e-5 * max(max|tensor|, max|any gradient| / 4) + 1e-6.
Plain float32 torch layers on the CPU stay within 0.10 of the score tolerance and 0.04 of the gradient tolerances on
the cases below (2 x 150 rows at (256, 64): 0.04 / 0.02 at F = 148 and at F = 704; 7 x 5000 rows: 0.05 / 0.02;
9 x 7300 rows at (128, 32): 0.10 / 0.03), so the tolerances leave room for another summation order and the cases keep
the scale of the rows file.
One thing no tolerance covers: a hidden pre-activation within float32 rounding of zero (about 1.5e-7 for these sums of
148 .. 704 products) lets the summation order decide ReLU', and with it whole rows of dW1 and dW2.  Among the 11 million
pre-activations of 35 000 rows under (256, 64) several are that small, so the two large cases put g on every 16th real
row (`every` of `_case`; a row without g adds nothing to any gradient), and every case here keeps, in float64,
min |pre-activation| >= 8e-7 over the rows that carry g (the large ones: 3.1e-6 and 1.7e-6).

The kernels walk the features in chunks of 64 (16-feature steps past the row's end are skipped), the dW1 kernel takes
column slices of 128 or 176 features (one slice up to 176 features, two from 180); a workgroup takes its tiles -- w,
w + G, w + 2G, ... on a grid of G = min(tiles, CUs) -- in groups of eight (scores) or four (gradient)."""
import numpy as np
import pytest
import torch

from tests.test_gpu_mlp_rows import _batch, _case, _close_module, _compare, _dev, _device_args, _no_torch_layers

pytestmark = pytest.mark.gpu


def _run(case, X=None, g=None, family=None):
    from pytorchltr_amd import fused
    family = family or fused._MLP_BIG_WIDE
    tX, tP, tn, tg = _device_args(case, X, g)
    H1, H2 = tP[0].shape[0], tP[2].shape[0]
    scores = fused._mlp_rows_scores(tX, tP, H1, H2, tn, family=family)
    grads = fused._mlp_grad_call(tX, tP, H1, H2, tg, tn, None, family=family)
    torch.cuda.synchronize()
    return scores, [t.clone() for t in grads]


# ---- 1. hidden-block boundaries at F = 148 (247 real rows, one list ends inside a subtile); feature boundaries at
#      (256, 64): a chunk ends at 256, the dW1 kernel takes two slices from 180, 700 skips nothing but pays for 704;
#      tiles against groups and the grid: ten one-tile groups, n = None, a subtile / a tile / a group of padding only
#      ((20, 48, 0) on 3 x 48 rows: tile 1 starts with 16 padded rows, tiles 3 and 4 are padding), a second group in the
#      gradient kernel (1094 tiles) and in the score kernel (2054 tiles: up to nine per workgroup at 256 CUs) ----
HIDDEN = [(65, 3), (4, 17), (128, 32), (129, 33), (255, 63), (256, 64), (256, 1), (1, 64)]
@pytest.mark.parametrize("key", [(2, 150, 148, H1, H2, (150, 97)) for H1, H2 in HIDDEN]
                         + [(2, 150, F, 256, 64, (150, 97)) for F in (172, 176, 180, 220, 252, 256, 260, 700, 704)]
                         + [(3, 37, 148, 256, 64, (37, 20, 37)), (2, 300, 148, 128, 32, (300, 129)),
                            (3, 37, 148, 256, 64, None), (3, 48, 148, 256, 64, (20, 48, 0)),
                            (7, 5000, 148, 256, 64, "ragged", 16), (9, 7300, 148, 128, 32, "ragged", 16)], ids=str)
def test_against_the_float64_layers(key):
    from pytorchltr_amd import fused
    case = _case(*key)
    assert fused.MLP_BIG_WIDE_MAX_FEATURES == 704 and (key[1] != 150 or case["real"].sum() == 247)
    if key[1] >= 5000:
        cus = torch.cuda.get_device_properties(_dev()).multi_processor_count
        tiles = (key[0] * key[1] + 31) // 32
        assert tiles > (4 if key[1] == 5000 else 8) * cus and (case["n"][:4] == (0, 1, key[1], key[1] + 5)).all()
    _compare(case, *_run(case))


# ---- 2. padding is not read, and two runs are equal ----
def test_padding_is_not_read_and_runs_are_equal():
    case = _case(5, 300, 220, 128, 32, "ragged")
    real = case["real"]
    Xn, gn = np.where(real[..., None], case["X"], np.float32(np.nan)), np.where(real, case["g"], np.float32(np.nan))
    assert np.isnan(Xn).any() and np.isnan(gn).any()
    s0, g0 = _run(case)
    s1, g1 = _run(case, Xn, gn)
    _compare(case, s1, g1)
    assert torch.equal(s0, s1) and all(torch.equal(a, b) for a, b in zip(g0, g1))
    s2, g2 = _run(case, Xn, gn)
    assert torch.equal(s1, s2) and all(torch.equal(a, b) for a, b in zip(g1, g2)) and len(g1) == 6


# ---- 3. the narrow rows and the small networks the C ABI takes too: agreement with the neighbours ----
@pytest.mark.parametrize("F,H1,H2,other", [(136, 256, 64, "_MLP_BIG"), (452, 64, 16, "_MLP_WIDE")])
def test_agreement_with_the_neighbours(F, H1, H2, other):
    from pytorchltr_amd import fused
    case = _case(2, 150, F, H1, H2, (150, 97))
    _compare(case, *_run(case))
    _compare(case, *_run(case, family=getattr(fused, other)))


# ---- 4. edge behaviour: an empty batch; capture and replay of both calls; the ValueError of the two functions ----
def test_empty_batch_and_capture_and_replay():
    from pytorchltr_amd import fused
    bw = dict(family=fused._MLP_BIG_WIDE)
    case = _case(2, 150, 220, 128, 32, (150, 97))
    tX, tP, tn, tg = _device_args(case)
    eager_s, eager_g = _run(case)
    out = torch.full((sum(p.numel() for p in tP),), 7.0, device=tX.device)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                  # (warm-up on the empty batch: attributes; zero gradients, no scores)
        assert fused._mlp_rows_scores(tX[:0], tP, 128, 32, None, **bw).shape == (0, 150)
        fused._mlp_grad_call(tX[:0], tP, 128, 32, tg[:0], None, out, **bw)
        assert not out.any()
        fused._mlp_grad_call(tX, tP, 128, 32, tg, tn, out, **bw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = fused._mlp_rows_scores(tX, tP, 128, 32, tn, **bw)
        fused._mlp_grad_call(tX, tP, 128, 32, tg, tn, out, **bw)
    for _ in range(3):
        s.fill_(-1.0)
        out.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(s, eager_s)
        assert all(torch.equal(a, b) for a, b in zip(fused._split_grads(out, 220, 128, 32), eager_g))


@pytest.mark.parametrize("F,H1", [(144, 256), (708, 256), (148, 257)])
def test_value_error_of_the_two_functions(F, H1):
    from pytorchltr_amd import fused
    case = _case(1, 5, F, H1, 64, None)
    tX, tP, _, tg = _device_args(case)
    for call in (lambda: fused.mlp_bigwide_scores(tX, tP), lambda: fused.mlp_bigwide_grad(tX, tP, tg)):
        with pytest.raises(ValueError, match=r"144 < F <= 704 with F % 4 == 0, hidden <= \(256, 64\) and L >= 1; got L=5 "
                                             + r"F=%d hidden=\(%d, 64\)" % (F, H1)):
            call()


# ---- 5. public interface ----
def _plain(model):
    import copy
    return torch.nn.Sequential(copy.deepcopy(model.l1), torch.nn.ReLU(), copy.deepcopy(model.l2), torch.nn.ReLU(),
                               copy.deepcopy(model.l3))


def test_scorer_module_forward_and_backward(monkeypatch):
    from pytorchltr_amd.fused import MLPScorer
    dev = _dev()
    torch.manual_seed(3)
    ours = MLPScorer(700, hidden=(256, 64), big_hidden_wide=True).to(dev)
    plain = _plain(ours)
    X = torch.randn(3, 70, 700, device=dev)
    up = torch.randn(3, 70, 1, device=dev)
    want = plain(X)
    want.backward(up)
    _no_torch_layers(monkeypatch)
    for kw in (dict(), dict(big_hidden=True)):     # without the flag, and with big_hidden alone: the torch layers
        with pytest.raises(AssertionError, match="functional.linear was called"):
            MLPScorer(700, hidden=(256, 64), **kw).to(dev)(X)
    got = ours(X)
    got.backward(up)
    assert torch.allclose(got, want.detach(), rtol=1e-5, atol=1e-5)
    _close_module(ours, plain, got.sum(), want.sum(), True)


@pytest.mark.parametrize("name,L", [("hinge", 60), ("hinge", 300), ("listmle", 300), ("lambdarank", 60)])
def test_loss_modules_step_and_trainer(monkeypatch, name, L):
    from pytorchltr_amd import fused
    from pytorchltr_amd.loss import LambdaRankLoss, ListMLELoss, PairwiseHingeLoss
    from pytorchltr_amd.utils import tie_breaking
    dev = _dev()
    torch.manual_seed(11)
    cls, kw, loss_fn = {"hinge": (fused.FusedMLPLoss, dict(loss="hinge"), PairwiseHingeLoss()),
                        "listmle": (fused.FusedMLPListwiseLoss, dict(loss="listmle"), ListMLELoss()),
                        "lambdarank": (fused.FusedMLPLambdaRankLoss, dict(k=10), LambdaRankLoss(k=10))}[name]
    make = lambda: cls(148, hidden=(128, 32), **kw).to(dev)     # noqa: E731
    ours = make()
    ours.big_hidden_wide = True
    plain = _plain(ours)
    X, y, n = _batch(4, L, 148, 7)
    tX, ty, tn = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(n).to(dev)
    with tie_breaking("index"):
        want = loss_fn(plain(tX), ty, tn).mean()
        want.backward()
        with monkeypatch.context() as mp:
            _no_torch_layers(mp)
            with pytest.raises(AssertionError, match="functional.linear was called"):
                make()(tX, ty, tn)                 # without the flag the route is unchanged: the torch layers
            got = ours(tX, ty, tn)
            got.backward()
            _close_module(ours, plain, got, want, name == "listmle")
            if name == "hinge":
                params = [p.detach() for p in ours.parameters()]
                lossv, grads = fused.mlp_loss_step(tX, params, ty, tn, "hinge", big_hidden_wide=True)
                assert torch.allclose(lossv.mean(), got.detach(), rtol=1e-5, atol=1e-6)
                for a, p in zip(grads, ours.parameters()):
                    assert torch.allclose(a.reshape(p.shape), p.grad, rtol=2e-4, atol=2e-5)
                torch.optim.SGD(plain.parameters(), lr=0.1).step()      # one step: the trainer against torch's optimizer
                fused.MLPTrainer(ours, "sgd", lr=0.1).step(tX, ty, tn)
                for a, b in zip(ours.parameters(), plain.parameters()):
                    assert torch.allclose(a, b, rtol=2e-4, atol=2e-5)
