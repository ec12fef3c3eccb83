"""GPU tier of the wide-hidden MLP scorer on wide bf16 rows (`-m gpu`, MI355X): ltr_mlp_bigwidebf16_scores / _grad
(include/ltr_mlp_bigwidebf16.h) through the launchers with family=_MLP_BIG_WIDE_BF16, and the opt-in route
``big_hidden_wide_bf16=True``.  Reference and tolerances, unchanged: tests/test_mlp_bf16_host.py::_case / _errors (float64
layers on the bf16-rounded X and W1; scores rtol 1e-5 / atol 2e-6, gradients <= 2e-5 * max(max|tensor|, max|any
gradient| / 4) + 1e-6); modules: those of tests/test_gpu_mlp_bf16.py.

The forward kernels walk the features in chunks of 128 (four K = 32 steps; a partial K-step multiplies stored zeros);
the dW1 kernel takes column slices of 8 or 15 sixteen-feature steps: one slice up to 240 features, two from 248 (of 8
steps up to 256, of 15 from 264), three from 488.  A workgroup takes its tiles in groups of eight (scores) or
four (gradient) on a grid of min(tiles, CUs).

A condition, not a tolerance (tests/test_gpu_mlp_bigwide.py): a pre-activation within fp32 rounding of zero lets the
summation order decide ReLU', so every case keeps, in float64 on the rounded operands, min |pre-activation| >= 8e-7
over the rows that carry g.  Checked on the CPU for every case of this file: the smallest is 9.7e-7 (F = 264, and the
(128, 32) network at 224 features), 7 x 5000 rows with g on every 16th real row have 1.4e-6.  The seed of `_case` follows
its shape, so where a shape misses the condition g is thinned instead (`every`): F = 224 at (256, 64) has 7.2e-7 on
every row and 1.5e-5 on every second one, the two neighbour cases 3.1e-7 / 2.4e-7 and, on every third row, 3.4e-5 /
2.7e-4.  9 x 7300 rows at (128, 32) with every = 16 have ONE hidden-2 pre-activation of 1.3e-7: the case is kept as the
precedents state it (the kernels and the reference agree on its sign) and runs a second time with every = 32 (9.3e-6),
which is the one that holds the condition."""
import numpy as np
import pytest
import torch

from tests.test_gpu_mlp_bf16 import _close_module, _compare, _dev, _device_args, _float64_layers, _no_torch_layers
from tests.test_mlp_bf16_host import _case

pytestmark = pytest.mark.gpu


def _run(case, X=None, g=None, family="_MLP_BIG_WIDE_BF16"):
    from pytorchltr_amd import fused
    family = getattr(fused, family)
    tX, tP, tn, tg = _device_args(case, X, g)
    H1, H2 = tP[0].shape[0], tP[2].shape[0]
    scores = fused._mlp_rows_scores(tX, tP, H1, H2, tn, family=family)
    grads = fused._mlp_grad_call(tX, tP, H1, H2, tg, tn, None, family=family)
    torch.cuda.synchronize()
    return scores, [t.clone() for t in grads]


HIDDEN = [(65, 3), (4, 17), (128, 32), (129, 33), (255, 63), (256, 64), (256, 1), (1, 64)]          # at F = 168, the minimum
# F % 32 = 8, 16, 24; chunk ends 256 / 384 / 512 / 640; the dW1 plan changes at 240 / 256 / 480; Istella, Yahoo
FEATURES = (176, 184, 240, 248, 256, 264, 384, 392, 480, 488, 512, 520, 640, 648, 696, 704)
KEYS = ([(2, 150, 168, H1, H2, (150, 97)) for H1, H2 in HIDDEN] + [(2, 150, F, 256, 64, (150, 97)) for F in FEATURES]
        + [(2, 150, 224, 256, 64, (150, 97), 2), (3, 37, 168, 256, 64, None), (3, 48, 168, 256, 64, (20, 48, 0)),
           (7, 5000, 168, 256, 64, "ragged", 16), (9, 7300, 168, 128, 32, "ragged", 16),
           (9, 7300, 168, 128, 32, "ragged", 32)])


@pytest.mark.parametrize("key", KEYS, ids=str)
def test_against_the_float64_layers(key):
    case = _case(*key)
    assert key[1] != 150 or case["real"].sum() == 247
    if key[1] >= 5000:
        cus = torch.cuda.get_device_properties(_dev()).multi_processor_count
        assert (key[0] * key[1] + 31) // 32 > (4 if key[1] == 5000 else 8) * cus
    _compare(case, *_run(case))


def test_padding_is_not_read_and_runs_are_equal():
    case = _case(5, 300, 224, 128, 32, "ragged")
    real = case["real"]
    Xn, gn = np.where(real[..., None], case["X"], np.float32(np.nan)), np.where(real, case["g"], np.float32(np.nan))
    assert np.isnan(Xn).any() and np.isnan(gn).any()
    (s0, g0), (s1, g1), (s2, g2) = _run(case), _run(case, Xn, gn), _run(case, Xn, gn)
    _compare(case, s1, g1)
    assert torch.equal(s0, s1) and torch.equal(s1, s2) and len(g1) == 6
    assert all(torch.equal(a, b) and torch.equal(b, c) for a, b, c in zip(g0, g1, g2))


@pytest.mark.parametrize("F,H1,H2,other", [(136, 256, 64, "_MLP_BIG_BF16"), (456, 64, 16, "_MLP_WIDE_BF16")])
def test_agreement_with_the_neighbours(F, H1, H2, other):
    case = _case(2, 150, F, H1, H2, (150, 97), 3)
    _compare(case, *_run(case))
    _compare(case, *_run(case, family=other))


def test_empty_batch_and_capture_and_replay():
    from pytorchltr_amd import fused
    case = _case(2, 150, 224, 128, 32, (150, 97))
    tX, tP, tn, tg = _device_args(case)
    eager_s, eager_g = _run(case)
    out = torch.full((sum(p.numel() for p in tP),), 7.0, device=tX.device)
    assert fused.mlp_bigwide_scores_bf16(tX[:0], tP).shape == (0, 150)     # the empty batch: zero gradients, no scores
    fused.mlp_bigwide_grad_bf16(tX[:0], tP, tg[:0], None, out)
    assert not out.any()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = fused.mlp_bigwide_scores_bf16(tX, tP, tn)
        fused.mlp_bigwide_grad_bf16(tX, tP, tg, tn, out)
    for _ in range(3):
        s.fill_(-1.0)
        out.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(s, eager_s)
        assert all(torch.equal(a, b) for a, b in zip(fused._split_grads(out, 224, 128, 32), eager_g))


def test_scorer_module_forward_and_backward(monkeypatch):
    from pytorchltr_amd.fused import MLPScorer
    dev = _dev()
    torch.manual_seed(3)
    ours = MLPScorer(699, hidden=(256, 64), big_hidden_wide_bf16=True).to(dev)
    plain = _float64_layers(ours)
    X = torch.randn(3, 70, 699, device=dev).bfloat16()
    up = torch.randn(3, 70, 1, device=dev)
    want = plain(X.double())
    want.backward(up.double())
    _no_torch_layers(monkeypatch)
    with pytest.raises(ValueError, match="bf16 MLP kernels"):              # without the flag: as today
        MLPScorer(699, hidden=(256, 64)).to(dev)(X)
    got = ours(X)
    got.backward(up)
    assert torch.allclose(got, want.detach().float(), rtol=1e-5, atol=2e-6)
    _close_module(ours, plain, got.sum(), want.sum(), False)


@pytest.mark.parametrize("name,L", [("hinge", 60), ("listmle", 300), ("lambdarank", 60)])
def test_loss_modules_step_and_trainer(monkeypatch, name, L):
    from pytorchltr_amd import fused
    from pytorchltr_amd.loss import LambdaRankLoss, ListMLELoss, PairwiseHingeLoss
    from pytorchltr_amd.utils import tie_breaking
    dev = _dev()
    torch.manual_seed(11)
    cls, kw, loss_fn = {"hinge": (fused.FusedMLPLoss, dict(loss="hinge"), PairwiseHingeLoss()),
                        "listmle": (fused.FusedMLPListwiseLoss, dict(loss="listmle"), ListMLELoss()),
                        "lambdarank": (fused.FusedMLPLambdaRankLoss, dict(k=10), LambdaRankLoss(k=10))}[name]
    ours = cls(224, hidden=(128, 32), **kw).to(dev)
    ours.big_hidden_wide_bf16 = True
    plain = _float64_layers(ours)
    rng = np.random.default_rng(L)
    tX = torch.from_numpy(rng.normal(0.0, 1.0, (4, L, 224)).astype(np.float32)).to(dev).bfloat16()
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
            lossv, grads = fused.mlp_loss_step(tX, params, ty, tn, "hinge", big_hidden_wide_bf16=True)
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
