"""GPU tier of the general fused Linear step on bf16 batches (include/ltr_bf16_general.h).  Reference, tolerances and the
hinge / rank-flip allowances are tests/test_gpu_linear_bf16.py's, taken as they are (`_batch`, `_oracle`, `_assert_step`:
the fp64 oracle on the bf16 values).  Shapes: F = 8 (64 rows per wave), 136 (groups of 32 lanes, 15 idle), 520 (65 column
vectors: the lanes stride the row); L = 5, 257 (past the register tile), kSymMaxLen + 1 (the both-ends pair pass)."""
import pytest
import torch

from oracle import ltr_oracle as O
from tests.test_gpu_linear_bf16 import _assert_step, _batch, _dev

pytestmark = pytest.mark.gpu
# (F, L, n[0] > L); 1025 = kSymMaxLen + 1 (csrc/ltr_common.inc): the first list of the both-ends pair pass
CASES = [(F, L, False) for F in (8, 136, 520) for L in (5, 257, 1025)] + [(136, 257, True)]


def _ref(kind, L):
    """A full, a half and an empty list; hinge on long lists: far-spread scores keep every pair off the margin."""
    return dict(lengths=(L, L // 2 + 1, 0), wscale=100.0 if kind == "hinge" and L > 256 else 1.0)


def _rows(kind, xs, W, b, y, n, want_scores=False):
    """loss, the raw partial rows and the scores of ltr_bf16_general_linear_partials."""
    from pytorchltr_amd import _C
    B, L, F = xs.shape
    lib = _C.lib()
    assert lib.ltr_bf16_general_linear_plan(O.KINDS[kind], B, L, F) == 1
    loss = torch.empty(B, dtype=torch.float32, device=xs.device)
    scores = torch.full((B, L), float("nan"), dtype=torch.float32, device=xs.device) if want_scores else None
    ws = torch.zeros(lib.ltr_linear_workspace_bytes(B, L, F) // 4, dtype=torch.float32, device=xs.device)
    _C.check(lib.ltr_bf16_general_linear_partials(O.KINDS[kind], 1.0, _C.ptr(xs), _C.ptr(W), _C.ptr(b), _C.ptr(y),
                                                  _C.label_dtype(y), _C.ptr(n), B, L, F, _C.ptr(loss), _C.ptr(scores),
                                                  _C.ptr(ws), _C.stream_of(xs)))
    return loss, ws[:B * (F + 4)].clone().reshape(B, F + 4), scores


@pytest.mark.parametrize("full", [True, False], ids=["scores-bias", "plain"])
@pytest.mark.parametrize("kind", ["hinge", "logistic", "ndcg2"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "F%d-L%d%s" % (c[0], c[1], "-over" if c[2] else ""))
def test_parity_with_the_fp64_oracle(case, kind, full):
    from pytorchltr_amd import fused
    F, L, over = case
    B, seed, dev = 3, 3600 + F + L, _dev()
    ref = _ref(kind, L)
    X16, X32, W, b, y, n = _batch(B, L, F, seed, **ref)
    if over:
        n = n + torch.tensor([9, 0, 0])                                     # n[0] > L: clamped to L
    xs, Wd, yd, nd = X16.to(dev), W.to(dev), y.to(dev), n.to(dev)
    bd = b.to(dev) if full else None                                        # (pairwise: the loss and its gradient do not move with the bias)
    real = (torch.arange(L)[None, :] < n.clamp(0, L)[:, None]).to(dev)
    scores_of = lambda s: None if s is None else torch.where(real, s + (0.0 if full else float(b[0])), s)      # noqa: E731
    loss, rows, scores = _rows(kind, xs, Wd, bd, yd, nd, want_scores=full)
    assert bool((rows[:, F + 1:] == 0).all()) and bool((rows[2] == 0).all()) and float(loss[2]) == 0.0
    mean = rows.double().mean(0)                                            # go_b = 1 / B
    _assert_step(kind, (loss, mean[:F], mean[F:F + 1]), B, L, F, seed, scores=scores_of(scores), what="partials", **ref)
    assert (fused._linear_route_of("step", xs, O.KINDS[kind]) == fused._LIN_BF16_FUSED) == (L <= 256)
    if L > 256:                                                             # (the flag changes nothing on the tile's plan)
        assert fused._linear_routed("step", xs, O.KINDS[kind], bf16_general=True)[0] == fused._LIN_BF16_GENERAL
        out = fused.linear_loss_step(xs, Wd, bd, yd, nd, loss=kind, return_scores=full, bf16_general=True)
        _assert_step(kind, out[:3], B, L, F, seed, scores=scores_of(out[3] if full else None), what="linear_loss_step", **ref)
        assert torch.equal(out[0], loss)                                    # the same launch


@pytest.mark.parametrize("kind", ["hinge", "logistic", "ndcg2"])
def test_padded_rows_are_never_read(kind):
    B, L, F, dev = 3, 257, 136, _dev()
    X16, X32, W, b, y, n = _batch(B, L, F, 3600 + F + L, _ref(kind, L)["lengths"])
    dirty = X16.clone()
    dirty[torch.arange(L)[None, :] >= n[:, None]] = float("nan")
    args = (W.to(dev), b.to(dev), y.to(dev), n.to(dev))
    clean = _rows(kind, X16.to(dev), *args, want_scores=True)
    for a, c in zip(clean, _rows(kind, dirty.to(dev), *args, want_scores=True)):
        assert torch.equal(a, c) and bool(torch.isfinite(a).all())


def test_two_runs_are_bit_identical_and_the_module_takes_the_flag():
    from pytorchltr_amd import fused
    B, L, F, seed, dev = 130, 257, 8, 4002, _dev()      # (more than half a query per CU: the module keeps the fused step)
    X16, X32, W, b, y, n = _batch(B, L, F, seed, wscale=100.0)
    xs, yd, nd = X16.to(dev), y.to(dev), n.to(dev)
    runs = [_rows("hinge", xs, W.to(dev), b.to(dev), yd, nd, want_scores=True) for _ in range(2)]
    assert all(torch.equal(a, c) for a, c in zip(*runs))
    m = fused.FusedLinearLoss(F, loss="hinge").to(dev)
    with torch.no_grad():
        m.weight.copy_(W.reshape(1, F))
        m.bias.copy_(b)
    assert fused._linear_routed("module", xs, m.kind, F, bf16_general=m.bf16_general)[0] == fused._LIN_BF16_PIECES
    m.bf16_general = True
    assert fused._linear_routed("module", xs, m.kind, F, bf16_general=m.bf16_general)[0] == fused._LIN_BF16_GENERAL
    out = m(xs, yd, nd)
    out.mean().backward()
    assert torch.equal(out.detach(), runs[0][0])                            # the same launch; gradients: the ordinary reduction
    _assert_step("hinge", (out, m.weight.grad, m.bias.grad), B, L, F, seed, what="FusedLinearLoss", wscale=100.0)
