"""CPU tier of the loss-steepness parity (tests/test_gpu_sigma.py is the GPU tier): what the GPU tests stand on.

  - the oracle's scaling identity, the five log-sigmoid kinds: loss(sigma; s) == loss(1; sigma s) and
    d loss / d s (sigma; s) == sigma * d loss / d s' (1; s' = sigma s) -- exactly at the powers of two 0.5 and 2.0
    (the factor moves through every product and the ranks do not move), within 1e-12 at 0.7 (observed: 1e-13 for
    LambdaNDCG1 at 37 documents, 2e-15 elsewhere);
  - the hinge kinds take no sigma: bit-identical at every sigma;
  - O.linear_pairwise / O.mlp_pairwise at a sigma are O.pairwise_loss at that sigma on their own scores pushed through
    X / through the network in float64 (bounds: tests/test_degenerate_host.py::test_linear_step_is_loss_plus_gradient,
    tests/test_oracle_golden.py::test_mlp_oracle_matches_reference_autograd);
  - the host side hands every module's sigma on: fused._resolve_loss, FusedLinearLoss, FusedMLPLoss, the loss modules'
    call into LazyScores.fused_loss, and the lazy launch of pytorchltr_amd.optim.SGD's state, call by call.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

from oracle import ltr_oracle as O
from tests.degenerate import degenerate_batch, exact_scores

LOGISTIC_KINDS = ("logistic", "arp1", "arp2", "ndcg1", "ndcg2")
HINGES = ("hinge", "dcg_hinge")
SIGMAS = (0.5, 0.7, 2.0)
LENGTHS = (37, 300)


@functools.lru_cache(maxsize=None)
def _batch(L, F=1):
    X, W, b, y, n, fl = degenerate_batch(24, L, F, 7000 + 13 * L + F + 24, scores="grid")
    return X, W, b, y.numpy(), n.numpy(), tuple(fl)


def _modules():
    import pytorchltr_amd.loss as losses
    from pytorchltr_amd import _C
    return {"logistic": (losses.PairwiseLogisticLoss, _C.LOGISTIC), "arp1": (losses.LambdaARPLoss1, _C.ARP1),
            "arp2": (losses.LambdaARPLoss2, _C.ARP2), "ndcg1": (losses.LambdaNDCGLoss1, _C.NDCG1),
            "ndcg2": (losses.LambdaNDCGLoss2, _C.NDCG2)}


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("sigma", SIGMAS)
def test_oracle_scaling_identity(sigma, L):
    X, W, b, y, n, fl = _batch(L)
    s = exact_scores(X)
    exact = sigma in (0.5, 2.0)
    for kind in LOGISTIC_KINDS:
        loss, grad = O.pairwise_loss(kind, s, y, n, sigma=sigma)
        loss1, grad1 = O.pairwise_loss(kind, sigma * s, y, n, sigma=1.0)
        assert np.all(np.isfinite(loss)) and np.all(np.isfinite(grad)), kind
        assert loss.any() and grad.any(), kind
        if exact:
            assert np.array_equal(loss, loss1) and np.array_equal(grad, sigma * grad1), kind
        scale = np.max(np.abs(grad), axis=1, keepdims=True)
        rel_l = np.max(np.abs(loss - loss1) / np.maximum(np.abs(loss1), 1e-300))
        rel_g = np.max(np.abs(grad - sigma * grad1) / np.maximum(scale, 1e-300))
        print("%s sigma %.1f L %d: loss rel %.2e grad rel %.2e" % (kind, sigma, L, rel_l, rel_g))
        assert rel_l <= 1e-12 and rel_g <= 1e-12, (kind, rel_l, rel_g)
        # sigma is not a no-op: the comparisons above are between two different computations
        loss_s1, _ = O.pairwise_loss(kind, s, y, n, sigma=1.0)
        assert not np.allclose(loss, loss_s1, rtol=1e-3, atol=0.0), kind


@pytest.mark.parametrize("L", LENGTHS)
def test_oracle_hinge_kinds_take_no_sigma(L):
    X, W, b, y, n, fl = _batch(L)
    s = exact_scores(X)
    for kind in HINGES:
        loss1, grad1 = O.pairwise_loss(kind, s, y, n, sigma=1.0)
        for sigma in SIGMAS:
            loss, grad = O.pairwise_loss(kind, s, y, n, sigma=sigma)
            assert np.array_equal(loss, loss1) and np.array_equal(grad, grad1), (kind, sigma)


@pytest.mark.parametrize("sigma", SIGMAS)
def test_oracle_linear_step_is_its_loss_at_that_sigma_through_x(sigma):
    L, F = 37, 5
    X, W, b, y, n, fl = _batch(L, F)
    B = X.shape[0]
    s = exact_scores(X)
    go = np.linspace(-0.5, 1.5, B)
    real = np.arange(L)[None, :] < n[:, None]
    for kind in LOGISTIC_KINDS + HINGES:
        loss, grad = O.pairwise_loss(kind, s, y, n, sigma=sigma)
        l2, s2, dW, db = O.linear_pairwise(kind, X.numpy(), W.numpy(), float(b[0]), y, n, go, sigma=sigma)
        assert np.array_equal(np.where(real, s2, 0.0), np.where(real, s, 0.0))
        assert np.array_equal(l2, loss), kind
        want_dW = np.einsum("bl,blf->f", grad * go[:, None], X.double().numpy())
        tol = 1e-12 * max(1.0, float(np.abs(want_dW).max()))
        assert np.max(np.abs(dW - want_dW)) <= tol and abs(db - float((grad * go[:, None]).sum())) <= tol, kind


@pytest.mark.parametrize("sigma", SIGMAS)
def test_oracle_mlp_step_is_its_loss_at_that_sigma_through_the_network(sigma):
    from tests.test_gpu_mlp import _mlp_params
    from tests.test_gpu_mlp_listwise import _network64
    L, F = 37, 8
    X, W, b, y, n, fl = _batch(L, F)
    B = X.shape[0]
    params = [p.numpy() for p in _mlp_params(F, 6, 3, 41)]
    go = np.linspace(-0.5, 1.5, B)
    real = np.arange(L)[None, :] < n[:, None]
    for kind in LOGISTIC_KINDS + HINGES:
        s, leaves = _network64(X.numpy(), params)
        loss, grad = O.pairwise_loss(kind, s.detach().numpy(), y, n, sigma=sigma)
        s.backward(torch.from_numpy(np.where(real, grad, 0.0) * go[:, None]))
        l2, s2, grads = O.mlp_pairwise(kind, X.numpy(), params, y, n, go, sigma=sigma)
        assert np.allclose(s2[real], s.detach().numpy()[real], rtol=1e-13, atol=1e-13)
        assert np.allclose(l2, loss, rtol=1e-12, atol=1e-13), kind
        scale = max(float(t.grad.abs().max()) for t in leaves)
        for key, t in zip(("W1", "b1", "W2", "b2", "W3", "b3"), leaves):
            want = t.grad.numpy()
            assert np.abs(grads[key].reshape(want.shape) - want).max() <= 1e-12 * scale + 1e-15, (kind, key)


def test_resolve_loss_and_the_fused_modules_carry_sigma():
    import pytorchltr_amd.loss as losses
    from pytorchltr_amd import _C, fused
    for kind, (cls, code) in _modules().items():
        assert fused._resolve_loss(cls()) == (code, 1.0), kind
        for sigma in SIGMAS:
            assert fused._resolve_loss(cls(sigma)) == (code, sigma), kind
            assert fused._resolve_loss(cls(sigma=sigma)) == (code, sigma), kind
            assert fused._resolve_pairwise_loss(cls(sigma)) == (code, sigma), kind
            m = fused.FusedLinearLoss(8, loss=cls(sigma))
            assert (m.kind, m.sigma) == (code, sigma), kind
            m = fused.FusedMLPLoss(8, loss=cls(sigma), hidden=(6, 3))
            assert (m.kind, m.sigma) == (code, sigma), kind
            assert isinstance(m.sigma, float)
    # a kind name and the hinge modules: sigma 1
    for name in LOGISTIC_KINDS + HINGES:
        assert fused._resolve_loss(name)[1] == 1.0
    assert fused._resolve_loss(losses.PairwiseHingeLoss()) == (_C.HINGE, 1.0)
    assert fused._resolve_loss(losses.PairwiseDCGHingeLoss()) == (_C.DCG_HINGE, 1.0)
    assert fused.FusedLinearLoss(8, loss="ndcg2").sigma == 1.0 and fused.FusedMLPLoss(8, loss="logistic").sigma == 1.0


class _Scores:
    """Stands in for fused.LazyScores: records what a loss module hands to `fused_loss`."""

    def __init__(self):
        self.calls = []

    def fused_loss(self, relevance, n, kind, sigma):
        self.calls.append((int(kind), sigma))
        return "fused"


def test_loss_modules_hand_their_sigma_to_lazy_scores_call_by_call():
    y, n = torch.zeros(2, 4, dtype=torch.int64), torch.tensor([4, 4])
    for kind, (cls, code) in _modules().items():
        sc = _Scores()
        mod = cls(2.0)
        assert mod(sc, y, n) == "fused"
        mod.sigma = 0.7                      # (a plain attribute, as in the reference: read at every call)
        assert mod(sc, y, n) == "fused"
        assert cls()(sc, y, n) == "fused"
        assert sc.calls == [(code, 2.0), (code, 0.7), (code, 1.0)], kind
    import pytorchltr_amd.loss as losses
    sc = _Scores()
    losses.PairwiseHingeLoss()(sc, y, n)
    losses.PairwiseDCGHingeLoss()(sc, y, n)
    assert [c[1] for c in sc.calls] == [1.0, 1.0]


class _Ctx:
    pass


def test_lazy_sgd_state_launches_with_each_calls_sigma(monkeypatch):
    """optim.SGD's per-scorer state (_LazyLinear) keeps no steepness of its own: the lazy launch gets the sigma and the
    kind of the call that makes it, also when the module changes between two steps on the same state."""
    from pytorchltr_amd import _C, optim
    launches = []

    class _Lib:
        def ltr_linear_workspace_bytes(self, B, L, F):
            return 4 * B * (F + 4) + 256

        def ltr_linear_sgd_lazy_step_dp_f32(self, kind, sigma, *rest):
            launches.append((int(kind), sigma))
            return 0

    monkeypatch.setattr(_C, "lib", lambda: _Lib())
    monkeypatch.setattr(_C, "device_ctx", lambda t: contextlib.nullcontext())
    monkeypatch.setattr(_C, "stream_of", lambda t: 0)
    B, L, F = 4, 8, 8
    weight, bias = torch.zeros(1, F), torch.zeros(1)
    st = optim._LazyLinear(weight, bias, {"lr": 0.1})
    X = torch.zeros(B, L, F)
    r, nn = torch.zeros(B, L, dtype=torch.int64), torch.full((B,), L)
    assert X.data_ptr() % 16 == 0
    keep = []
    for kind, sigma in ((_C.NDCG2, 2.0), (_C.NDCG2, 2.0), (_C.LOGISTIC, 0.7), (_C.ARP1, 1.0)):
        ctx = _Ctx()
        keep.append(ctx)
        loss = st.forward(ctx, X, r, _C.LABEL_I64, nn, kind, sigma)
        assert loss is not None and loss.shape == (B,)
        assert ctx.lazy[0] is st and ctx.lazy[2] == (kind, B, L, F)
        st.node = None                       # (the backward pass of this step has run)
    assert launches == [(_C.NDCG2, 2.0), (_C.NDCG2, 2.0), (_C.LOGISTIC, 0.7), (_C.ARP1, 1.0)]
