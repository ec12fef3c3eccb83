"""GPU tier of the MLP scorer with wide hidden layers (run with `-m gpu` on an MI355X): ltr_mlp_big_scores_f32 and
ltr_mlp_big_grad_f32 (include/ltr_mlp_big.h) through the launchers with family=_MLP_BIG, and the opt-in route
``big_hidden=True`` of MLPScorer, the loss modules, mlp_loss_step and MLPTrainer.

Reference and tolerances: those of tests/test_gpu_mlp_rows.py, unchanged -- the three layers in float64, scores rtol 1e-5 /
atol 2e-6, padded scores exactly 0, every gradient tensor <= 2e-5 * max(max|tensor|, max|any gradient| / 4) + 1e-6."""
import numpy as np
import pytest
import torch

from tests.test_gpu_mlp_rows import _batch, _case, _close_module, _compare, _dev, _device_args, _no_torch_layers

pytestmark = pytest.mark.gpu


def _run(case, X=None, g=None, family=None):
    from pytorchltr_amd import fused
    family = family or fused._MLP_BIG
    tX, tP, tn, tg = _device_args(case, X, g)
    H1, H2 = tP[0].shape[0], tP[2].shape[0]
    scores = fused._mlp_rows_scores(tX, tP, H1, H2, tn, family=family)
    grads = fused._mlp_grad_call(tX, tP, H1, H2, tg, tn, None, family=family)
    torch.cuda.synchronize()
    return scores, [t.clone() for t in grads]


# ---- 1 - 4. hidden-block boundaries (F = 136: 247 real rows, one list ends inside a subtile), feature-chunk boundaries
#      at (256, 64) (every F the fill and the buckets F <= 48, 80, 144 treat differently), tiles against queries (three
#      queries in a tile, a straddled boundary, n = None), more tiles than the one-workgroup-per-CU grid ----
HIDDEN = [(65, 3), (4, 17), (64, 17), (80, 16), (128, 32), (129, 33), (240, 48), (255, 63), (256, 64), (256, 1), (1, 64)]
@pytest.mark.parametrize("key", [(2, 150, 136, H1, H2, (150, 97)) for H1, H2 in HIDDEN]
                         + [(2, 150, F, 256, 64, (150, 97)) for F in (4, 8, 16, 20, 52, 84, 132, 144)]
                         + [(3, 37, 24, 256, 64, (37, 20, 37)), (2, 300, 24, 128, 32, (300, 129)),
                            (3, 37, 24, 256, 64, None), (2, 300, 24, 128, 32, None), (7, 5000, 136, 256, 64, "ragged")], ids=str)
def test_against_the_float64_layers(key):
    from pytorchltr_amd import fused
    case = _case(*key)
    assert fused.MLP_BIG_MAX_FEATURES == 144 and (key[1] != 150 or case["real"].sum() == 247)
    if key[1] == 5000:
        cus = torch.cuda.get_device_properties(_dev()).multi_processor_count
        assert (7 * 5000 + 31) // 32 == 1094 > cus and (case["n"][:4] == (0, 1, 5000, 5005)).all()
    _compare(case, *_run(case))


# ---- 5. padding is not read, and two runs are equal ----
def test_padding_is_not_read_and_runs_are_equal():
    case = _case(5, 300, 136, 128, 32, "ragged")
    real = case["real"]
    Xn, gn = np.where(real[..., None], case["X"], np.float32(np.nan)), np.where(real, case["g"], np.float32(np.nan))
    assert np.isnan(Xn).any() and np.isnan(gn).any()
    s0, g0 = _run(case)
    s1, g1 = _run(case, Xn, gn)
    _compare(case, s1, g1)
    assert torch.equal(s0[torch.from_numpy(real)], s1[torch.from_numpy(real)])
    s2, g2 = _run(case, Xn, gn)
    assert torch.equal(s1, s2) and all(torch.equal(a, b) for a, b in zip(g1, g2)) and len(g1) == 6
    assert all(torch.equal(a, b) for a, b in zip(g0, g1))


# ---- 6. small networks agree with the rows family ----
@pytest.mark.parametrize("H1,H2", [(50, 10), (64, 16)])
def test_small_networks_agree_with_the_rows_family(H1, H2):
    from pytorchltr_amd import fused
    case = _case(2, 150, 136, H1, H2, (150, 97))
    _compare(case, *_run(case))
    _compare(case, *_run(case, family=fused._MLP_ROWS))


# ---- 7. edge behaviour: an empty batch; capture and replay of both calls; the ValueError of the two functions ----
def test_empty_batch_and_capture_and_replay():
    from pytorchltr_amd import fused
    big = dict(family=fused._MLP_BIG)
    case = _case(2, 150, 136, 128, 32, (150, 97))
    tX, tP, tn, tg = _device_args(case)
    eager_s, eager_g = _run(case)
    out = torch.full((sum(p.numel() for p in tP),), 7.0, device=tX.device)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                  # (warm-up on the empty batch: attributes; zero gradients, no scores)
        assert fused._mlp_rows_scores(tX[:0], tP, 128, 32, None, **big).shape == (0, 150)
        fused._mlp_grad_call(tX[:0], tP, 128, 32, tg[:0], None, out, **big)
        assert not out.any()
        fused._mlp_grad_call(tX, tP, 128, 32, tg, tn, out, **big)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = fused._mlp_rows_scores(tX, tP, 128, 32, tn, **big)
        fused._mlp_grad_call(tX, tP, 128, 32, tg, tn, out, **big)
    for _ in range(3):
        s.fill_(-1.0)
        out.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(s, eager_s)
        assert all(torch.equal(a, b) for a, b in zip(fused._split_grads(out, 136, 128, 32), eager_g))


@pytest.mark.parametrize("F,H1,got", [(148, 256, r"F=148 hidden=\(256, 64\)"), (8, 257, r"F=8 hidden=\(257, 64\)")])
def test_value_error_of_the_two_functions(F, H1, got):
    from pytorchltr_amd import fused
    case = _case(1, 5, F, H1, 64, None)
    tX, tP, _, tg = _device_args(case)
    for call in (lambda: fused.mlp_big_scores(tX, tP), lambda: fused.mlp_big_grad(tX, tP, tg)):
        with pytest.raises(ValueError, match=r"F <= 144 with F % 4 == 0, hidden <= \(256, 64\) and L >= 1; got L=5 " + got):
            call()


# ---- 8. public interface ----
def _plain(model):
    import copy
    return torch.nn.Sequential(copy.deepcopy(model.l1), torch.nn.ReLU(), copy.deepcopy(model.l2), torch.nn.ReLU(),
                               copy.deepcopy(model.l3))


def test_scorer_module_forward_and_backward(monkeypatch):
    from pytorchltr_amd.fused import MLPScorer
    dev = _dev()
    torch.manual_seed(3)
    ours = MLPScorer(136, hidden=(256, 64), big_hidden=True).to(dev)
    plain = _plain(ours)
    X = torch.randn(3, 70, 136, device=dev)
    up = torch.randn(3, 70, 1, device=dev)
    want = plain(X)
    want.backward(up)
    _no_torch_layers(monkeypatch)
    with pytest.raises(AssertionError, match="functional.linear was called"):      # without the flag: the torch layers
        MLPScorer(136, hidden=(256, 64)).to(dev)(X)
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
    make = lambda: cls(24, hidden=(128, 32), **kw).to(dev)      # noqa: E731
    ours = make()
    ours.big_hidden = True
    plain = _plain(ours)
    X, y, n = _batch(4, L, 24, 7)
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
                lossv, grads = fused.mlp_loss_step(tX, params, ty, tn, "hinge", big_hidden=True)
                assert torch.allclose(lossv.mean(), got.detach(), rtol=1e-5, atol=1e-6)
                for a, p in zip(grads, ours.parameters()):
                    assert torch.allclose(a.reshape(p.shape), p.grad, rtol=2e-4, atol=2e-5)
                torch.optim.SGD(plain.parameters(), lr=0.1).step()      # one step: the trainer against torch's optimizer
                fused.MLPTrainer(ours, "sgd", lr=0.1).step(tX, ty, tn)
                for a, b in zip(ours.parameters(), plain.parameters()):
                    assert torch.allclose(a, b, rtol=2e-4, atol=2e-5)
