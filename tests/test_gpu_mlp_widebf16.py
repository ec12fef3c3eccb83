"""GPU tier of the MLP scorer on wide bf16 rows (run with `-m gpu` on an MI355X): ltr_mlp_widebf16_scores and
ltr_mlp_widebf16_grad (include/ltr_mlp_widebf16.h) through fused.mlp_wide_scores_bf16 / fused.mlp_wide_grad_bf16, and
the modules with the opt-in `wide_bf16`.

Reference and tolerances: those of tests/test_gpu_mlp_bf16.py, whose helpers are used as they are (`_case` / `_errors`
of tests/test_mlp_bf16_host.py: float64 layers on the bf16-rounded X and W1; `_float64_layers` / `_close_module`).
The plan under test (csrc/ltr_mlp_widebf16.inc): the forward kernel walks image chunks of 256 features (1, 2 or 3 of
them: boundaries at 256 and 512); the dW1 kernel takes one slice up to 352 features and two past them, of 8 K-steps
each up to 256 / 512 features and of 11 above (boundaries at 256, 352 and 512)."""
import numpy as np
import pytest
import torch

from tests.test_gpu_mlp_bf16 import _close_module, _compare, _dev, _device_args, _float64_layers, _no_torch_layers
from tests.test_mlp_bf16_host import _case, _params

pytestmark = pytest.mark.gpu


def _abi(prefix, tX, tP, tn, tg):
    """(scores, flat gradient) from the C ABI of one family: `ltr_mlp_widebf16` or `ltr_mlp_bf16`."""
    from pytorchltr_amd import _C
    lib, st = _C.lib(), _C.stream_of(tX)
    B, L, F = tX.shape
    H1, H2 = tP[0].shape[0], tP[2].shape[0]
    ptrs = [t.data_ptr() for t in tP]
    scores = torch.empty(B, L, device=tX.device)
    flat = torch.empty(sum(t.numel() for t in tP), device=tX.device)
    nbytes = getattr(lib, prefix + "_grad_workspace_bytes")(B, L, F, H1, H2)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=tX.device)
    _C.check(getattr(lib, prefix + "_scores")(tX.data_ptr(), *ptrs, _C.ptr(tn), B, L, F, H1, H2, scores.data_ptr(), st))
    _C.check(getattr(lib, prefix + "_grad")(tX.data_ptr(), *ptrs, tg.data_ptr(), _C.ptr(tn), B, L, F, H1, H2,
                                            flat.data_ptr(), ws.data_ptr(), nbytes, st))
    torch.cuda.synchronize()
    return scores, flat


def _run(case, X=None, g=None):
    """(scores (B, L), six gradients) from the two wide bf16 kernels."""
    from pytorchltr_amd import fused
    tX, tP, tn, tg = _device_args(case, X, g)
    scores = fused.mlp_wide_scores_bf16(tX, tP, tn)
    grads = fused.mlp_wide_grad_bf16(tX, tP, tg, tn)
    torch.cuda.synchronize()
    return scores, grads


# ---- 1. tiles against queries ----
@pytest.mark.parametrize("F", [232, 704])
@pytest.mark.parametrize("B,L,lengths", [
    (5, 33, "ragged"),                             # a query spans tiles, a tile spans queries; n = 0, 1, L, L + 5
    (3, 16, "ragged"),                             # less than two tiles
    (1, 1, (1,)),                                  # one row
    (2, 96, (96, 0)),                              # whole tiles of padding
    (5, 33, None),                                 # n == NULL: every row is real
], ids=["5x33", "3x16", "1x1", "2x96-padding", "5x33-no-n"])
def test_tiles_against_queries(B, L, lengths, F):
    case = _case(B, L, F, 50, 10, lengths)
    _compare(case, *_run(case))


# ---- 2. every chunk and slice boundary of the plan ----
@pytest.mark.parametrize("F,H1,H2", [(F, 64, 16) for F in (232, 256, 264, 352, 360, 456, 512, 520, 704)] + [(456, 1, 1)])
def test_every_chunk_and_slice_boundary(F, H1, H2):
    case = _case(4, 50, F, H1, H2, "ragged")
    _compare(case, *_run(case))


@pytest.mark.parametrize("F", [8, 136, 224])
def test_narrow_rows_through_the_c_abi_agree_with_the_bf16_row_kernels(F):
    """F <= 224 is accepted by the C ABI.  The SCORES are bit-identical to ltr_mlp_bf16_scores: both kernels run the
    same MFMA sequence over a row (K-steps in ascending order from b1; the K-steps past F multiply zero weights with
    zero columns) and the same fp32 chains behind it.  The GRADIENTS agree within the tolerance only: the two plans
    group the partial sums differently (row ranges x slices against one vector per workgroup)."""
    case = _case(4, 50, F, 64, 16, "ragged")
    args = _device_args(case)
    s_wide, flat_wide = _abi("ltr_mlp_widebf16", *args)
    s_rows, flat_rows = _abi("ltr_mlp_bf16", *args)
    assert torch.equal(s_wide, s_rows)
    from pytorchltr_amd import fused
    for flat in (flat_wide, flat_rows):
        _compare(case, s_wide, fused._split_grads(flat, F, 64, 16))


# ---- 3. more tiles than workgroups ----
def test_more_tiles_than_workgroups():
    # 40 x 1000 = 40 000 flat rows = 1250 tiles of 32 rows; a launch has at most 2 workgroups x 256 CUs = 512, so every
    # workgroup of both kernels carries its sums, the ring and the look-ahead piece over two or three tiles; g is
    # non-zero on every 7th real row
    case = _case(40, 1000, 232, 4, 4, "ragged", 7)
    assert case["real"].sum() > 512 * 32 // 2
    s0, g0 = _run(case)
    _compare(case, s0, g0)
    s1, g1 = _run(case)                             # 5. determinism, where workgroups carry sums across tiles
    assert torch.equal(s0, s1) and all(torch.equal(a, b) for a, b in zip(g0, g1))


# ---- 4. padding is never read, 5. determinism ----
def test_padding_is_not_read_and_two_runs_are_equal():
    case = _case(5, 33, 264, 50, 10, "ragged")
    Xn, gn = case["X"].copy(), case["g"].copy()
    Xn[~case["real"]] = gn[~case["real"]] = np.nan
    assert np.isnan(Xn).any() and np.isnan(gn).any()
    s0, g0 = _run(case)
    for s1, g1 in (_run(case, X=Xn, g=gn), _run(case)):
        assert torch.equal(s0, s1) and all(torch.equal(a, b) for a, b in zip(g0, g1))


# ---- 6. empty batch ----
def test_an_empty_batch_gives_zero_gradients():
    from pytorchltr_amd import _C, fused
    dev = _dev()
    tP = [torch.from_numpy(p).to(dev) for p in _params(232, 5, 3, np.random.default_rng(0))]
    out = torch.full((sum(p.numel() for p in tP),), float("nan"), device=dev)
    x0 = torch.zeros(0, 7, 232, device=dev, dtype=torch.bfloat16)
    grads = fused.mlp_wide_grad_bf16(x0, tP, torch.zeros(0, 7, device=dev), out=out)
    assert fused.mlp_wide_scores_bf16(x0, tP).shape == (0, 7) and grads[0].shape == (5, 232) and not out.any()
    # the C ABI itself: B == 0 returns LTR_OK from both calls (no data pointers, no workspace) and zeroes the gradients
    lib, st, ptrs = _C.lib(), _C.stream_of(out), [t.data_ptr() for t in tP]
    out.fill_(float("nan"))
    assert lib.ltr_mlp_widebf16_grad(None, *ptrs, None, None, 0, 7, 232, 5, 3, out.data_ptr(), None, 0, st) == 0
    assert lib.ltr_mlp_widebf16_scores(None, *ptrs, None, 0, 7, 232, 5, 3, None, st) == 0
    assert not out.any()


# ---- 7. capture and replay ----
def test_capture_and_replay():
    """Both calls recorded into one graph (one stream, no branches) and replayed twice on changed inputs: the eager
    results bit for bit."""
    from pytorchltr_amd import fused
    tX, tP, tn, tg = _device_args(_case(5, 33, 264, 50, 10, "ragged"))
    inputs = [(torch.randn_like(tX), torch.randn_like(tg)) for _ in range(2)]
    eager = [(fused.mlp_wide_scores_bf16(X, tP, tn), [t.clone() for t in fused.mlp_wide_grad_bf16(X, tP, g, tn)])
             for X, g in inputs]
    torch.cuda.synchronize()
    flat = torch.empty(sum(p.numel() for p in tP), device=tX.device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        cap_s = fused.mlp_wide_scores_bf16(tX, tP, tn)
        cap_g = fused.mlp_wide_grad_bf16(tX, tP, tg, tn, out=flat)
    for (X, g), (want_s, want_g) in zip(inputs, eager):
        tX.copy_(X)
        tg.copy_(g)
        cap_s.fill_(float("nan"))
        flat.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap_s, want_s) and all(torch.equal(a, b) for a, b in zip(cap_g, want_g))


# ---- 8. the modules with the opt-in, 9. and without it ----
def test_scorer_module_pads_to_704_and_crops_the_gradient(monkeypatch):
    from pytorchltr_amd.fused import MLPScorer
    dev = _dev()
    torch.manual_seed(5)
    m = MLPScorer(699, (17, 5), wide_bf16=True).to(dev)
    X = torch.randn(3, 40, 699, device=dev).bfloat16()
    tn = torch.tensor([40, 0, 17], device=dev)
    up = torch.randn(3, 40, 1, device=dev)
    plain = _float64_layers(m)
    real = (torch.arange(40, device=dev)[None, :] < tn[:, None]).unsqueeze(-1)
    want_s = torch.where(real, plain(X.double()), 0.0)
    want = (want_s * up.double()).sum()
    want.backward()
    _no_torch_layers(monkeypatch)
    scores = m(X, tn)
    got = (scores * up).sum()
    got.backward()
    assert torch.allclose(scores.detach(), want_s.detach().float(), rtol=1e-5, atol=2e-6)
    assert scores.shape == (3, 40, 1) and not scores.detach()[~real].any()
    _close_module(m, plain, got, want, False)
    with torch.no_grad():                                               # without gradients: the score kernel alone
        assert torch.equal(m(X, tn), scores.detach())
    with pytest.raises(ValueError, match="bf16 MLP kernels"):           # the default: the narrow family's limit
        MLPScorer(699, (17, 5)).to(dev)(X, tn)


@pytest.mark.parametrize("which,L", [("hinge", 300), ("listmle", 300), ("hinge", 60)], ids=["hinge-300", "listmle-300", "hinge-60"])
def test_loss_modules_with_the_opt_in(which, L, monkeypatch):
    from pytorchltr_amd.fused import FusedMLPListwiseLoss, FusedMLPLoss
    from pytorchltr_amd.loss import ListMLELoss, PairwiseHingeLoss
    from pytorchltr_amd.utils import tie_breaking
    dev = _dev()
    B, F = 4, 700
    torch.manual_seed(L)
    tX = torch.randn(B, L, F, device=dev).bfloat16()
    ty = torch.randint(0, 5, (B, L), device=dev)
    tn = torch.tensor([L, 2, L // 2, L - 1], device=dev)
    if which == "hinge":
        m, default = FusedMLPLoss(F, "hinge", wide_bf16=True).to(dev), FusedMLPLoss(F, "hinge").to(dev)
    else:
        m, default = FusedMLPListwiseLoss(F, "listmle").to(dev), FusedMLPListwiseLoss(F, "listmle").to(dev)
        m.wide_bf16 = True
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
    with pytest.raises(ValueError, match="bf16 MLP kernels"):           # the default is what it was
        default(tX, ty, tn)


def test_loss_step_and_trainer_step_are_the_module_s_step():
    from pytorchltr_amd import fused
    dev = _dev()
    case = _case(4, 50, 704, 64, 16, "ragged")
    tX, tP, tn, _ = _device_args(case)
    ty = torch.from_numpy(np.random.default_rng(3).integers(0, 5, (4, 50))).to(dev)
    with pytest.raises(ValueError):                                     # the default is what it was
        fused.mlp_loss_step(tX, tP, ty, tn, loss="hinge")
    lossv, grads, scores = fused.mlp_loss_step(tX, tP, ty, tn, loss="hinge", return_scores=True, wide_bf16=True)
    assert torch.equal(scores, fused.mlp_wide_scores_bf16(tX, tP, tn))
    m = fused.FusedMLPLoss(704, "hinge", hidden=(64, 16), wide_bf16=True).to(dev)
    with torch.no_grad():
        for p, v in zip(m.parameters(), tP):
            p.copy_(v.reshape(p.shape))
    total = m(tX, ty, tn)
    total.backward()
    assert torch.allclose(total, lossv.mean(), rtol=1e-6, atol=1e-7)
    for p, gr in zip(m.parameters(), grads):
        assert torch.allclose(p.grad, gr.reshape(p.shape), rtol=1e-5, atol=1e-6)
    # one MLPTrainer step (Adagrad) against torch.optim.Adagrad fed the module's gradients: the update itself is
    # ltr_mlp_apply_update_f32, held to its own bounds by tests/test_gpu_mlp_update.py -- here: fp32 rounding of one step
    opt = torch.optim.Adagrad(m.parameters(), lr=0.05, eps=1e-10)
    twin = fused.FusedMLPLoss(704, "hinge", hidden=(64, 16), wide_bf16=True).to(dev)
    twin.load_state_dict(m.state_dict())
    trainer = fused.MLPTrainer(twin, "adagrad", lr=0.05, eps=1e-10)
    loss, tgrads = trainer.step(tX, ty, tn, return_grads=True)
    assert torch.allclose(loss, total.detach(), rtol=1e-6, atol=1e-7)
    for p, gr in zip(m.parameters(), tgrads):
        assert torch.allclose(p.grad, gr.reshape(p.shape), rtol=1e-5, atol=1e-6)
    opt.step()
    for a, b in zip(twin.parameters(), m.parameters()):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)
