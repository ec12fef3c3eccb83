"""GPU tier: the pairwise losses on lists longer than ltr_max_list_len() documents (include/ltr_longpair.h,
``long_lists=True``) against the fp64 oracle, against the one-workgroup kernels (the long path forced onto short lists
by ltr_debug_long_pairs_all), run to run, and through the modules and the fused Linear entry points.

The oracle is O(L^2) on the CPU, so nothing here goes above 6000 documents; tests/test_gpu_long_pairs_max.py runs the
same kernels at ltr_max_pair_list_len() against the references of oracle/long_pairs_ref.py, which need no pair loop."""
import functools

import numpy as np
import pytest
import torch

from oracle import ltr_oracle as O
from tests.conftest import synth
from tests.test_gpu_parity import _check_grad, _loss_tol

pytestmark = pytest.mark.gpu
KINDS = list(O.KINDS)
DEV = torch.device("cuda:0")


def _code(kind):
    from pytorchltr_amd import _C
    return _C.__dict__[kind.upper()]


def _grid_scores(B, L, seed):
    """Scores on the grid 3k / 1024, |k| <= 1365: every hinge margin 1 - (s_i - s_j) = (1024 - 3m) / 1024 is exact in
    fp32 and in fp64 and never 0 (3m = 1024 has no integer solution), so the one-ulp caveat of DESIGN 7.3 cannot fire."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(-1365, 1366, (B, L), generator=g)
    return (k.to(torch.float32) * 3.0) / 1024.0


@functools.lru_cache(maxsize=None)
def _long_batch(B, L):
    """(scores, labels, n) of the oracle-parity cases, read-only: synth scores, row 1 quantised to 16 levels (heavy ties:
    the index tie order inside the LambdaNDCG kinds), integer labels 0..4, n = (L, L // 3, 1, 0) trimmed to B."""
    s, y, _ = synth(B, L, 4100 + L)
    s[1] = torch.round(s[1] * 2.0).clamp(-8, 7) / 2.0
    n = torch.tensor([L, L // 3, 1, 0][:B], dtype=torch.int64)
    out = (s.numpy(), y.numpy(), n.numpy())
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _oracle(kind, B, L):
    s, y, n = _long_batch(B, L)
    return O.pairwise_loss(kind, s, y, n)


def _run_long(kind, s, y, n, sigma=1.0):
    from pytorchltr_amd._autograd import pairwise_loss_and_grad
    loss, ds = pairwise_loss_and_grad(torch.as_tensor(s).to(DEV), torch.as_tensor(y).to(DEV), torch.as_tensor(n).to(DEV),
                                      _code(kind), sigma, long_lists=True)
    return loss.cpu().numpy(), ds.cpu().numpy()


def _check_loss_vs_oracle(kind, loss, want_l, what):
    """The project's loss tolerance for ~1e7-term fp32 sums (tests/test_gpu_stress.py::test_maximum_list_length)."""
    rtol = 2e-3 if kind in ("ndcg1", "ndcg2") else 5e-4
    lerr = np.abs(loss - want_l)
    print("%s: loss rel err %.3e" % (what, np.max(lerr / np.maximum(np.abs(want_l), 1e-30))))
    assert np.all(np.isfinite(loss)), what
    assert np.allclose(loss, want_l, rtol=rtol, atol=1e-5), what


def _check_grad_vs_oracle(ds, want_g, what):
    """... and its gradient tolerance: 2e-4 of the largest entry of the row handed in (a whole row, or a sample of one)."""
    scale = np.max(np.abs(want_g), axis=1, keepdims=True)
    gerr = np.abs(ds.astype(np.float64) - want_g)
    print("%s: grad err / max|row| %.3e" % (what, np.max(gerr / np.maximum(scale, 1e-30))))
    assert np.all(np.isfinite(ds)), what
    assert np.all(gerr <= 2e-4 * scale + 1e-5), what


def _check_vs_oracle(kind, loss, ds, want_l, want_g, n, what):
    _check_loss_vs_oracle(kind, loss, want_l, what)
    _check_grad_vs_oracle(ds, want_g, what)
    for b in range(len(n)):
        assert np.all(ds[b, int(n[b]):] == 0.0), what                  # exactly 0 past n[b]


@pytest.mark.parametrize("B,L", [(4, 4097), (3, 6000)])
@pytest.mark.parametrize("kind", KINDS)
def test_long_path_vs_oracle(kind, B, L):
    s, y, n = _long_batch(B, L)
    loss, ds = _run_long(kind, s, y, n)
    want_l, want_g = _oracle(kind, B, L)
    _check_vs_oracle(kind, loss, ds, want_l, want_g, n, "%s %dx%d" % (kind, B, L))


def test_hinge_gradient_is_bit_exact_on_grid_scores():
    """Counts of active pairs are integers below 2^24: with margins that are exact in both precisions the fp32 gradient
    IS the fp64 one."""
    B, L = 2, 4097
    s = _grid_scores(B, L, 7).numpy()
    _, y, _ = synth(B, L, 8)
    n = np.array([L, L // 2], dtype=np.int64)
    loss, ds = _run_long("hinge", s, y.numpy(), n)
    want_l, want_g = O.pairwise_loss("hinge", s, y.numpy(), n)
    assert np.array_equal(ds.astype(np.float64), want_g)
    assert np.allclose(loss, want_l, rtol=5e-4, atol=1e-5)


def _forced_lengths():
    from pytorchltr_amd import _C
    own, ch = _C.long_pair_geometry()
    cap = _C.max_list_len()
    return sorted({min(L, cap) for L in (1, 2, 63, 64, 65, own - 1, own, own + 1, ch + 1, 2 * ch + own + 3) if L >= 1})


def _forced_vs_existing(kind, L, sort_all=False):
    """The long path forced onto a list the one-workgroup kernels take, against those kernels."""
    from pytorchltr_amd import _C
    from pytorchltr_amd._autograd import pairwise_loss_and_grad
    lib = _C.lib()
    B = 3
    s, y, _ = synth(B, L, 900 + L)
    hinge = kind in ("hinge", "dcg_hinge")
    if hinge:
        s = _grid_scores(B, L, 900 + L)
    n = torch.tensor([L, max(L // 2, 1), 1], dtype=torch.int64)
    sd, yd, nd = s.to(DEV), y.to(DEV), n.to(DEV)
    want_l, want_g = pairwise_loss_and_grad(sd, yd, nd, _code(kind))
    prev = lib.ltr_debug_long_pairs_all(1)
    prev_sort = lib.ltr_debug_long_sort_all(1) if sort_all else None
    try:
        assert lib.ltr_pairwise_loss_long_workspace_bytes(_code(kind), B, L) > 0
        loss, ds = pairwise_loss_and_grad(sd, yd, nd, _code(kind), long_lists=True)
    finally:
        if sort_all:
            lib.ltr_debug_long_sort_all(prev_sort)
        lib.ltr_debug_long_pairs_all(prev)
    what = "%s L=%d%s" % (kind, L, " (sorted preparation)" if sort_all else "")
    loss, ds = loss.cpu().numpy().astype(np.float64), ds.cpu().numpy()
    want_l, want_g = want_l.cpu().numpy().astype(np.float64), want_g.cpu().numpy()
    rtol, atol = _loss_tol(L)
    print("%s: loss rel diff %.3e" % (what, np.max(np.abs(loss - want_l) / np.maximum(np.abs(want_l), 1e-30))))
    assert np.all(np.isfinite(loss)), what
    assert np.all(np.abs(loss - want_l) <= atol + rtol * np.abs(want_l)), what
    _check_grad(ds, want_g.astype(np.float64), what, exact=(kind == "hinge"))
    for b in range(B):
        assert np.all(ds[b, int(n[b]):] == 0.0), what


@pytest.mark.parametrize("kind", KINDS)
def test_forced_long_path_vs_existing_kernels(kind):
    for L in _forced_lengths():
        _forced_vs_existing(kind, L)


@pytest.mark.parametrize("kind", ["ndcg1", "ndcg2"])
def test_sorted_preparation_vs_ndcg_prepare_kernel(kind):
    """The long path prepares the LambdaNDCG kinds from the key sort and the label sort at every length (the forced
    lengths of test_forced_long_path_vs_existing_kernels included); here once more with ltr_debug_long_sort_all set,
    against the one-workgroup kernels and their ndcg_prepare_kernel, at a length of more than one tile."""
    from pytorchltr_amd import _C
    own, _ = _C.long_pair_geometry()
    _forced_vs_existing(kind, own + 1, sort_all=True)


@pytest.mark.parametrize("kind", ["logistic", "ndcg2"])
def test_long_path_is_deterministic(kind):
    from pytorchltr_amd import _C
    B, L = 3, 6000
    s, y, n = _long_batch(B, L)
    first = _run_long(kind, s, y, n)
    again = _run_long(kind, s, y, n)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    # the workspace's contents do not matter: all NaN bytes in
    lib = _C.lib()
    sd, yd, nd = torch.as_tensor(s).to(DEV), torch.as_tensor(y).to(DEV), torch.as_tensor(n).to(DEV)
    nbytes = int(lib.ltr_pairwise_loss_long_workspace_bytes(_code(kind), B, L))
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    loss = torch.full((B,), float("nan"), device=DEV)
    ds = torch.full((B, L), float("nan"), device=DEV)
    _C.check(lib.ltr_pairwise_loss_long_f32(_code(kind), 1.0, sd.data_ptr(), yd.data_ptr(), _C.label_dtype(yd), nd.data_ptr(),
                                            B, L, loss.data_ptr(), ds.data_ptr(), ws.data_ptr(), nbytes, _C.stream_of(sd)))
    assert np.array_equal(first[0], loss.cpu().numpy()) and np.array_equal(first[1], ds.cpu().numpy())
    # forward only: the same loss, no gradient written
    loss2 = torch.empty(B, device=DEV)
    _C.check(lib.ltr_pairwise_loss_long_f32(_code(kind), 1.0, sd.data_ptr(), yd.data_ptr(), _C.label_dtype(yd), nd.data_ptr(),
                                            B, L, loss2.data_ptr(), None, ws.data_ptr(), nbytes, _C.stream_of(sd)))
    assert np.array_equal(first[0], loss2.cpu().numpy())


@pytest.mark.parametrize("cls_name,kind", [("PairwiseLogisticLoss", "logistic"), ("LambdaNDCGLoss2", "ndcg2")])
def test_modules_with_long_lists(cls_name, kind):
    import pytorchltr_amd.loss as losses
    B, L = 2, 4097
    s, y, n = _long_batch(4, L)
    s, y, n = s[:B], y[:B], n[:B]
    want_l, want_g = _oracle(kind, 4, L)
    cls = getattr(losses, cls_name)
    sd = torch.as_tensor(s).to(DEV).unsqueeze(-1).requires_grad_(True)          # (B, L, 1), as a scorer returns them
    yd, nd = torch.as_tensor(y).to(DEV), torch.as_tensor(n).to(DEV)
    loss = cls(long_lists=True)(sd, yd, nd)
    assert loss.shape == (B,)
    loss.mean().backward()
    got_g = sd.grad.reshape(B, L).cpu().numpy() * B
    _check_vs_oracle(kind, loss.detach().cpu().numpy(), got_g, want_l[:B], want_g[:B], n, cls_name)
    with pytest.raises(ValueError, match="exceeds"):
        cls()(sd.detach(), yd, nd)
    with pytest.raises(ValueError, match="exceeds"):                             # fp64 keeps its bound
        cls(long_lists=True)(sd.detach().double(), yd, nd)


def test_fused_linear_fallback_on_long_lists():
    """FusedLinearLoss, linear_loss_step and a loss module on LazyScores past 4096 documents: the scorer, the long loss
    and the weight-gradient kernel.  Tolerances: the loss as above; the weight gradient is a linear image of the score
    gradient, held to the same 2e-4 of its largest entry."""
    import pytorchltr_amd.loss as losses
    from pytorchltr_amd import fused
    B, L, F = 2, 4100, 8
    s, y, _, X, W, b = synth(B, L, 77, F=F)
    n = torch.tensor([L, L // 3], dtype=torch.int64)
    go = np.full(B, 1.0 / B)
    want_l, _, want_dW, want_db = O.linear_pairwise("hinge", X.numpy(), W.numpy(), float(b), y.numpy(), n.numpy(), go)
    Xd, yd, nd = X.to(DEV), y.to(DEV), n.to(DEV)

    def check(loss, dW, db, what):
        loss, dW, db = (np.asarray(t.detach().cpu().numpy(), dtype=np.float64).reshape(-1) for t in (loss, dW, db))
        print("%s: loss rel err %.3e, dW err / max %.3e" % (
            what, np.max(np.abs(loss - want_l) / np.abs(want_l)), np.max(np.abs(dW - want_dW)) / np.max(np.abs(want_dW))))
        assert np.allclose(loss, want_l, rtol=5e-4, atol=1e-5), what
        assert np.all(np.abs(dW - want_dW) <= 2e-4 * np.max(np.abs(want_dW)) + 1e-5), what
        assert np.all(np.abs(db - want_db) <= 2e-4 * np.max(np.abs(want_dW)) + 1e-5), what

    m = fused.FusedLinearLoss(F, loss=losses.PairwiseHingeLoss(long_lists=True)).to(DEV)
    with torch.no_grad():
        m.weight.copy_(W.reshape(1, F))
        m.bias.copy_(b)
    loss = m(Xd, yd, nd)
    loss.mean().backward()
    check(loss, m.weight.grad, m.bias.grad, "FusedLinearLoss")

    out = fused.linear_loss_step(Xd, m.weight.detach(), m.bias.detach(), yd, nd, loss=losses.PairwiseHingeLoss(long_lists=True))
    check(out[0], out[1], out[2], "linear_loss_step")

    model = torch.nn.Linear(F, 1).to(DEV)
    with torch.no_grad():
        model.weight.copy_(W.reshape(1, F))
        model.bias.copy_(b)
    model = fused.use_linear_scorer(model)
    loss = losses.PairwiseHingeLoss(long_lists=True)(model(Xd), yd, nd)
    loss.mean().backward()
    check(loss, model.weight.grad, model.bias.grad, "LinearScorer + module")

    # without the opt-in nothing changes: the fused entry points refuse the shape
    plain = fused.FusedLinearLoss(F, loss="hinge").to(DEV)
    with pytest.raises((ValueError, RuntimeError)):
        plain(Xd, yd, nd)
    with pytest.raises((ValueError, RuntimeError)):
        losses.PairwiseHingeLoss()(model(Xd), yd, nd)
