"""GPU tier of the wide-hidden MLP scorer on bf16 batches (`-m gpu`, MI355X): fused.mlp_big_scores_bf16 / mlp_big_grad_bf16
(include/ltr_mlp_bigbf16.h) and the opt-in route ``big_hidden_bf16=True``.  Reference and tolerances, unchanged:
tests/test_mlp_bf16_host.py::_case / _errors (float64 layers on the bf16-rounded X and W1; scores rtol 1e-5 / atol 2e-6,
gradients <= 2e-5 * max(max|tensor|, max|any gradient| / 4) + 1e-6); modules: those of tests/test_gpu_mlp_bf16.py."""
import numpy as np
import pytest
import torch

from tests.test_gpu_mlp_bf16 import _close_module, _compare, _dev, _device_args, _float64_layers, _no_torch_layers
from tests.test_mlp_bf16_host import _case

pytestmark = pytest.mark.gpu


def _run(case, X=None, g=None, bf16=False):
    from pytorchltr_amd import fused
    tX, tP, tn, tg = _device_args(case, X, g)
    scores = (fused.mlp_scores_bf16 if bf16 else fused.mlp_big_scores_bf16)(tX, tP, tn)
    grads = (fused.mlp_grad_bf16 if bf16 else fused.mlp_big_grad_bf16)(tX, tP, tg, tn)
    torch.cuda.synchronize()
    return scores, [t.clone() for t in grads]


# hidden blocks, K-steps and buckets (F <= 64, 160), tiles against queries; small networks also through the bf16 family
HIDDEN = [(65, 3), (4, 17), (128, 32), (129, 33), (255, 63), (256, 64), (256, 1), (1, 64), (50, 10), (64, 16)]
@pytest.mark.parametrize("key", [(2, 150, 136, H1, H2, (150, 97)) for H1, H2 in HIDDEN]
                         + [(2, 150, F, 256, 64, (150, 97)) for F in (8, 24, 32, 40, 64, 72, 160)]      # (168 .. 224: past the limit)
                         + [(3, 37, 24, 256, 64, None), (2, 96, 40, 128, 32, (96, 0)), (1, 1, 8, 256, 64, (1,)),
                            (7, 5000, 136, 256, 64, "ragged")], ids=str)
def test_against_the_float64_layers(key):
    case = _case(*key)
    _compare(case, *_run(case))
    if key[3] <= 64 and key[4] <= 16:
        _compare(case, *_run(case, bf16=True))


def test_padding_is_not_read_and_runs_are_equal():
    case = _case(5, 300, 136, 128, 32, "ragged")
    real = case["real"]
    Xn, gn = np.where(real[..., None], case["X"], np.float32(np.nan)), np.where(real, case["g"], np.float32(np.nan))
    s0, g0 = _run(case)
    s1, g1 = _run(case, Xn, gn)
    s2, g2 = _run(case, Xn, gn)
    _compare(case, s1, g1)
    assert torch.equal(s0, s1) and torch.equal(s1, s2) and len(g1) == 6
    assert all(torch.equal(a, b) and torch.equal(b, c) for a, b, c in zip(g0, g1, g2))


def test_empty_batch_and_capture_and_replay():
    from pytorchltr_amd import fused
    case = _case(2, 150, 136, 128, 32, (150, 97))
    tX, tP, tn, tg = _device_args(case)
    eager_s, eager_g = _run(case)
    out = torch.full((sum(p.numel() for p in tP),), 7.0, device=tX.device)
    assert fused.mlp_big_scores_bf16(tX[:0], tP).shape == (0, 150)         # the empty batch: zero gradients, no scores
    fused.mlp_big_grad_bf16(tX[:0], tP, tg[:0], None, out)
    assert not out.any()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = fused.mlp_big_scores_bf16(tX, tP, tn)
        fused.mlp_big_grad_bf16(tX, tP, tg, tn, out)
    for _ in range(3):
        s.fill_(-1.0)
        out.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(s, eager_s)
        assert all(torch.equal(a, b) for a, b in zip(fused._split_grads(out, 136, 128, 32), eager_g))


def test_scorer_module_forward_and_backward(monkeypatch):
    from pytorchltr_amd.fused import MLPScorer
    dev = _dev()
    torch.manual_seed(3)
    ours = MLPScorer(136, hidden=(256, 64), big_hidden_bf16=True).to(dev)
    plain = _float64_layers(ours)
    X = torch.randn(3, 70, 136, device=dev).bfloat16()
    up = torch.randn(3, 70, 1, device=dev)
    want = plain(X.double())
    want.backward(up.double())
    _no_torch_layers(monkeypatch)
    with pytest.raises(ValueError, match="bf16 MLP kernels"):              # without the flag: as today
        MLPScorer(136, hidden=(256, 64)).to(dev)(X)
    got = ours(X)
    got.backward(up)
    assert torch.allclose(got, want.detach().float(), rtol=1e-5, atol=2e-6)
    _close_module(ours, plain, got.sum(), want.sum(), False)


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
    ours = cls(24, hidden=(128, 32), **kw).to(dev)
    ours.big_hidden_bf16 = True
    plain = _float64_layers(ours)
    rng = np.random.default_rng(L)
    tX = torch.from_numpy(rng.normal(0.0, 1.0, (4, L, 24)).astype(np.float32)).to(dev).bfloat16()
    ty = torch.from_numpy(rng.integers(0, 5, (4, L))).to(dev)
    tn = torch.from_numpy(np.concatenate([[L], rng.integers(2, L + 1, 3)])).to(dev)
    with tie_breaking("index"):
        want = loss_fn(plain(tX.double()).float(), ty, tn).mean()       # (the loss is the fp32 HIP kernel on both sides)
        want.backward()
        _no_torch_layers(monkeypatch)
        got = ours(tX, ty, tn)
        got.backward()
        _close_module(ours, plain, got, want, name == "listmle")
        if name == "hinge":
            params = [p.detach() for p in ours.parameters()]
            lossv, grads = fused.mlp_loss_step(tX, params, ty, tn, "hinge", big_hidden_bf16=True)
            assert torch.allclose(lossv.mean(), got.detach(), rtol=1e-5, atol=1e-6)
            for a, p in zip(grads, ours.parameters()):
                assert torch.allclose(a.reshape(p.shape), p.grad, rtol=2e-4, atol=2e-5)
            ref = [p.detach().clone().requires_grad_() for p in ours.parameters()]
            for r, b in zip(ref, plain.parameters()):
                r.grad = b.grad.float()
            torch.optim.SGD(ref, lr=0.1).step()
            fused.MLPTrainer(ours, "sgd", lr=0.1).step(tX, ty, tn)
            for a, b in zip(ours.parameters(), ref):
                assert torch.allclose(a, b, rtol=2e-4, atol=2e-5)
