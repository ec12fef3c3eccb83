"""GPU tier of LambdaRankLoss (run with `-m gpu` on an MI355X): ltr_lambdarank_f32 against the fp64 reference of
tests/lambdarank_ref.py on every launch shape of the ranked-row core, the many-rounds shapes, bit identity (no cutoff
reached, repeated calls, forward only), degenerate rows, score ties, label dtypes, garbage in padded slots, far-apart
scores, and the module in autograd, with other dtypes and under stream capture.

Tolerances: the project's for the Lambda losses against the fp64 oracle (tests/test_gpu_parity.py) -- loss
|err| <= 2e-6 + rtol |want| with rtol 1e-5 up to 256 documents and 5e-4 above, gradient |err| <= 1e-5 max_row |want| +
1e-6."""
import functools

import numpy as np
import pytest
import torch

from tests import lambdarank_ref as R

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 17, 64, 65, 128, 200, 256, 257, 300, 512, 513, 1000, 1025, 2048, 2049, 4096]
KS = [None, 1, 5, 10, 1 << 20]
SIGMAS = [1.0, 2.5]
B = 7


def _dev():
    assert torch.cuda.is_available(), "GPU tier needs a ROCm device"
    return torch.device("cuda:0")


def _lengths(rng, L):
    """Ragged n of B = 7 queries with 0, 1, 2 and L; the rest: about a half, a fifth and a few documents."""
    n = np.array([0, 1, 2, L, L // 2 + 1, L // 5 + 3, 3 + int(rng.integers(0, 20))], dtype=np.int64)
    return np.minimum(n, L)


@functools.lru_cache(maxsize=None)
def _batch(L, seed=0, spread=2.0, shift=0.0):
    """Normal scores, integer grades 0..4, ragged n (`_lengths`).  Cached: the tests of one length share it."""
    rng = np.random.default_rng(1000 * L + seed)
    s = (rng.normal(0.0, spread, (B, L)) + shift).astype(np.float32)
    y = rng.integers(0, 5, (B, L)).astype(np.int64)
    n = _lengths(rng, L)
    for a in (s, y, n):
        a.setflags(write=False)
    return s, y, n


@functools.lru_cache(maxsize=None)
def _want(L, k, sigma, seed=0, spread=2.0, shift=0.0):
    """The reference of `_batch`, computed once per case and left unchanged."""
    loss, ds = R.batch(*_batch(L, seed, spread, shift), k=k, sigma=sigma)
    loss.setflags(write=False)
    ds.setflags(write=False)
    return loss, ds


def _t(s, y, n):
    dev = _dev()
    # (copies: the cached batches are read-only, and views such as s[:, ::-1] are not contiguous)
    return torch.from_numpy(np.array(s)).to(dev), torch.from_numpy(np.array(y)).to(dev), torch.from_numpy(np.array(n)).to(dev)


def _call(ts, ty, tn, k=None, sigma=1.0, grad=True):
    """ltr_lambdarank_f32 on the current stream: (loss, dscores or None)."""
    from pytorchltr_amd import _C
    Bq, L = ts.shape
    loss = torch.empty(Bq, dtype=torch.float32, device=ts.device)
    ds = torch.empty(Bq, L, dtype=torch.float32, device=ts.device) if grad else None
    _C.check(_C.lib().ltr_lambdarank_f32(_C.ptr(ts), _C.ptr(ty), _C.label_dtype(ty), _C.ptr(tn), int(k or 0), float(sigma),
                                         Bq, L, _C.ptr(loss), _C.ptr(ds), _C.stream_of(ts)))
    torch.cuda.synchronize()
    return loss, ds


def _loss_rtol(L):
    return 1e-5 if L <= 256 else 5e-4


def _check(got, want, L):
    gl, gd = got
    wl, wd = want
    gl = gl.cpu().numpy().astype(np.float64)
    err = np.abs(gl - wl)
    bound = 2e-6 + _loss_rtol(L) * np.abs(wl)
    print("L=%d loss: max err %.3e (worst err / bound %.3f)" % (L, err.max(), (err / bound).max()))
    assert np.all(np.isfinite(gl))
    assert np.all(err <= bound), (gl, wl)
    if gd is not None:
        gd = gd.cpu().numpy().astype(np.float64)
        gerr = np.abs(gd - wd).max(axis=1)
        gbound = 1e-5 * np.abs(wd).max(axis=1) + 1e-6
        print("L=%d grad: max err %.3e (worst err / bound %.3f)" % (L, gerr.max(), (gerr / gbound).max()))
        assert np.all(np.isfinite(gd))
        assert np.all(gerr <= gbound), (gerr, gbound)


# ---- parity ----
@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("L", LENGTHS)
def test_parity_against_the_reference(L, k, sigma):
    _check(_call(*_t(*_batch(L)), k=k, sigma=sigma), _want(L, k, sigma), L)


@pytest.mark.parametrize("per_cu,L", [(16, 300), (64, 100)])
def test_many_rounds_launch_shapes(per_cu, L):
    """From 16 queries per CU on the sort shapes run half the threads with two keys each, from 64 on lists of up to
    128 documents run one wave per query: 64 distinct queries tiled, every row against the reference of its original."""
    dev = _dev()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    rng = np.random.default_rng(L)
    s = rng.normal(0.0, 2.0, (64, L)).astype(np.float32)
    y = rng.integers(0, 5, (64, L)).astype(np.int64)
    n = rng.integers(0, L + 1, 64).astype(np.int64)
    n[:4] = (0, 1, 2, L)
    wl, wd = R.batch(s, y, n, k=10, sigma=1.0)
    reps = -(-per_cu * cus // 64)                                       # (at least per_cu queries per CU)
    ts, ty, tn = _t(s, y, n)
    gl, gd = _call(ts.repeat(reps, 1), ty.repeat(reps, 1), tn.repeat(reps), k=10)
    gl = gl.reshape(reps, 64)
    gd = gd.reshape(reps, 64, L)
    assert torch.equal(gl, gl[:1].expand_as(gl)) and torch.equal(gd, gd[:1].expand_as(gd))   # every copy, the same bits
    _check((gl[reps - 1], gd[reps - 1]), (wl, wd), L)


# ---- exactness ----
@pytest.mark.parametrize("L", [17, 128, 300, 1000])
def test_a_cutoff_no_row_reaches_is_no_cutoff(L):
    ts, ty, tn = _t(*_batch(L))
    full = _call(ts, ty, tn, k=None, sigma=2.5)
    for k in (L, L + 1, 1 << 20):
        got = _call(ts, ty, tn, k=k, sigma=2.5)
        assert torch.equal(got[0], full[0]) and torch.equal(got[1], full[1]), k


@pytest.mark.parametrize("L", [128, 300, 1000])
def test_repeated_and_forward_only_calls_are_bit_identical(L):
    ts, ty, tn = _t(*_batch(L))
    for k in (None, 10):
        a = _call(ts, ty, tn, k=k)
        for _ in range(2):
            b = _call(ts, ty, tn, k=k)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        fwd, none = _call(ts, ty, tn, k=k, grad=False)
        assert none is None and torch.equal(fwd, a[0])


# ---- degenerate rows ----
@pytest.mark.parametrize("L", [17, 200, 1000])
def test_degenerate_rows(L):
    s, _, n = _batch(L)
    ts, _, tn = _t(s, s, n)
    for labels in (torch.full((B, L), 3, dtype=torch.int64), torch.zeros((B, L), dtype=torch.int64),
                   torch.full((B, L), 1.5, dtype=torch.float32)):
        for k in (None, 5):
            loss, ds = _call(ts, labels.to(ts.device), tn, k=k)
            assert not loss.any() and not ds.any()
    # n_b in {0, 1}: rows 0 and 1 of every batch
    loss, ds = _call(*_t(*_batch(L)), k=5)
    assert not loss[:2].any() and not ds[:2].any()
    assert L < 3 or loss[3] > 0


@pytest.mark.parametrize("L", [17, 200, 1000])
@pytest.mark.parametrize("k", [None, 5])
def test_duplicate_scores_rank_in_index_order(L, k):
    s, y, n = _batch(L)
    s = (np.round(s * 2.0) / 2.0).astype(np.float32)                   # a handful of distinct values: ties everywhere
    _check(_call(*_t(s, y, n), k=k), R.batch(s, y, n, k=k), L)


def test_a_tie_straddling_the_cutoff():
    L, k = 17, 5
    rng = np.random.default_rng(5)
    base = np.array([9, 8, 7, 6, 5, 5, 5, 4, 3, 3, 2, 1, 0, -1, -2, -3, -4], dtype=np.float32)   # ranks 4, 5, 6 tie: K - 1 | K
    s = np.stack([base[rng.permutation(L)] for _ in range(B)])
    y = rng.integers(0, 5, (B, L)).astype(np.int64)
    n = np.full(B, L, dtype=np.int64)
    got = _call(*_t(s, y, n), k=k)
    _check(got, R.batch(s, y, n, k=k), L)
    # the rule matters here: the tied documents in the reverse order are another loss
    rev = R.batch(s[:, ::-1], y[:, ::-1], n, k=k)[0]
    assert not np.allclose(got[0].cpu().numpy(), rev, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("L", [17, 300])
def test_a_float_label_of_minus_one_has_gain_minus_a_half(L):
    s, y, n = _batch(L)
    yf = (y - 1).astype(np.float32)                                    # -1 .. 3
    assert (yf == -1).any()
    _check(_call(*_t(s, yf, n), k=5), R.batch(s, yf, n, k=5), L)
    # the same grades as integers: the float formula whatever the dtype
    got_i = _call(*_t(s, (y - 1), n), k=5)
    got_f = _call(*_t(s, yf, n), k=5)
    assert torch.equal(got_i[0], got_f[0]) and torch.equal(got_i[1], got_f[1])


@pytest.mark.parametrize("L", [64, 300, 1000])
def test_garbage_in_padded_slots_changes_nothing(L):
    s, y, n = _batch(L)
    yf = y.astype(np.float32)
    want = _call(*_t(s, yf, n), k=10)
    s2, y2 = s.copy(), yf.copy()
    for b in range(B):
        s2[b, n[b]:] = np.nan
        y2[b, n[b]:] = np.nan
    got = _call(*_t(s2, y2, n), k=10)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("L", [17, 300, 1000])
def test_label_dtypes_agree_bit_for_bit(L):
    s, y, n = _batch(L)
    a = _call(*_t(s, y, n), k=10)
    for dtype in (np.int32, np.float32):
        b = _call(*_t(s, y.astype(dtype), n), k=10)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), dtype


# ---- stability ----
@pytest.mark.parametrize("L", [50, 300, 1000])
@pytest.mark.parametrize("shift,spread", [(1000.0, 2.0), (-1000.0, 2.0), (0.0, 200.0)])
def test_far_apart_scores_stay_finite_and_on_the_reference(L, shift, spread):
    for k in (None, 10):
        _check(_call(*_t(*_batch(L, 7, spread, shift)), k=k), _want(L, k, 1.0, 7, spread, shift), L)


# ---- the module ----
def test_module_backward_matches_the_reference():
    from pytorchltr_amd.loss import LambdaRankLoss
    for L in (40, 1000):
        s, y, n = _batch(L)
        ts, ty, tn = _t(s, y, n)
        wl, wd = _want(L, 10, 2.5)
        ts.requires_grad_(True)
        loss = LambdaRankLoss(sigma=2.5, k=10)(ts.unsqueeze(-1), ty, tn)
        assert loss.shape == (B,)
        loss.mean().backward()
        _check((loss.detach(), ts.grad * B), (wl, wd), L)
        # a per-query weighted sum
        wts = torch.linspace(0.5, 2.0, B, device=ts.device)
        ts.grad = None
        (LambdaRankLoss(sigma=2.5, k=10)(ts, ty, tn) * wts).sum().backward()
        _check((loss.detach(), ts.grad), (wl, wd * wts.cpu().numpy()[:, None].astype(np.float64)), L)


def test_loss_on_the_scores_of_an_mlp_scorer():
    """loss_fn(MLPScorer(...)(xs, n), ys, n) as with any loss: real scores in, gradients out to the layers."""
    from pytorchltr_amd.fused import MLPScorer
    from pytorchltr_amd.loss import LambdaRankLoss
    _, y, n = _batch(40)
    _, ty, tn = _t(y, y, n)
    torch.manual_seed(2)
    m = MLPScorer(24).to(_dev())
    X = torch.randn(B, 40, 24, device=_dev())
    scores = m(X, tn)
    loss = LambdaRankLoss(k=5)(scores, ty, tn)
    loss.mean().backward()
    _check((loss.detach(), None), R.batch(scores.detach().squeeze(-1).cpu().numpy(), y, n, k=5), 40)
    for p in m.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all()
    assert m.l1.weight.grad.abs().max() > 0


@pytest.mark.parametrize("dtype", [torch.float64, torch.bfloat16, torch.float16])
def test_module_dtypes_round_trip(dtype):
    from pytorchltr_amd.loss import LambdaRankLoss
    ts, ty, tn = _t(*_batch(30))
    x = ts.to(dtype).requires_grad_(True)
    loss = LambdaRankLoss(k=10)(x, ty, tn)
    loss.sum().backward()
    ref = LambdaRankLoss(k=10)(x.detach().float(), ty, tn)
    assert loss.dtype == dtype and x.grad.dtype == dtype and x.grad.shape == x.shape
    tol = 1e-6 if dtype == torch.float64 else 2e-2
    torch.testing.assert_close(loss.float(), ref, rtol=tol, atol=tol)


@pytest.mark.parametrize("L", [100, 1000])
def test_graph_capture_replays_equal_to_eager(L):
    from pytorchltr_amd.loss import LambdaRankLoss
    ts, ty, tn = _t(*_batch(L))
    fn = LambdaRankLoss(k=10)
    x = ts.clone().requires_grad_(True)
    eager = fn(x, ty, tn)
    eager.sum().backward()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn(ts, ty, tn)                                             # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = fn(ts, ty, tn)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap, eager.detach())
    assert torch.isfinite(x.grad).all()
