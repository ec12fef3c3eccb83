"""GPU tier of ListMLE (run with `-m gpu` on an MI355X): ltr_listmle_f32 against the fp64 oracle of
tests/test_listmle_host.py on both paths (one workgroup per query up to 4096 documents, the sort path beyond and under
ltr_debug_long_sort_all), the random tie mode against the oracle fed with the kernels' tie words, numerical stability,
run-to-run bit identity, and ListMLELoss in autograd, stream capture and the drop-in training loop."""
import copy

import numpy as np
import pytest
import torch

from tests.test_listmle_host import oracle

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 17, 64, 128, 129, 1000, 4096, 4097, 10000, 100000]


def _dev():
    assert torch.cuda.is_available(), "GPU tier needs a ROCm device"
    return torch.device("cuda:0")


def _batch(seed, B, L, dtype=np.int64, grades=5, spread=2.0):
    """Normal scores, labels in [0, grades) (tie-heavy), ragged n with 0, 1, L and more than L."""
    rng = np.random.default_rng(seed)
    s = rng.normal(0.0, spread, (B, L)).astype(np.float32)
    if dtype == np.float32:
        y = (rng.integers(0, 2 * grades, (B, L)) * 0.5).astype(np.float32)
    else:
        y = rng.integers(0, grades, (B, L)).astype(dtype)
    n = rng.integers(0, L + 1, B).astype(np.int64)
    for i, v in enumerate((0, 1, L, L + 7)):
        if i < B:
            n[i] = v
    return s, y, n


def _rows(L):
    return 6 if L <= 4096 else (3 if L <= 10000 else 2)


def _t(s, y, n):
    dev = _dev()
    return torch.from_numpy(s).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(n).to(dev)


def _call(ts, ty, tn, k=None, grad=True, seed=None):
    """ltr_listmle_f32 on the current stream: (loss, dscores or None).  seed None: index order."""
    from pytorchltr_amd import _C
    lib = _C.lib()
    B, L = ts.shape
    loss = torch.empty(B, dtype=torch.float32, device=ts.device)
    ds = torch.empty(B, L, dtype=torch.float32, device=ts.device) if grad else None
    nbytes = int(lib.ltr_listmle_workspace_bytes(B, L))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=ts.device) if nbytes > 0 else None
    _C.check(lib.ltr_listmle_f32(_C.ptr(ts), _C.ptr(ty), _C.label_dtype(ty), _C.ptr(tn), int(k or 0), None,
                                 int(seed is not None), seed or 0, None, B, L, _C.ptr(loss), _C.ptr(ds), _C.ptr(ws),
                                 nbytes, _C.stream_of(ts)))
    torch.cuda.synchronize()
    return loss, ds


def _check(got, want, L, ks=1.0):
    gl, gd = got
    wl, wd = want
    gl = gl.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(gl))
    np.testing.assert_allclose(gl, wl, rtol=1e-4, atol=1e-4 * ks)
    if gd is not None:
        gd = gd.cpu().numpy().astype(np.float64)
        assert np.all(np.isfinite(gd))
        np.testing.assert_allclose(gd, wd, rtol=1e-3, atol=2e-4 * ks)


class _LongSortAll:
    def __enter__(self):
        from pytorchltr_amd import _C
        self.prev = _C.lib().ltr_debug_long_sort_all(1)

    def __exit__(self, *exc):
        from pytorchltr_amd import _C
        _C.lib().ltr_debug_long_sort_all(self.prev)
        return False


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("k", [None, 1, 10, 1 << 20])
def test_parity_against_the_oracle(L, k):
    s, y, n = _batch(L * 7 + (k or 0) % 97, _rows(L), L)
    _check(_call(*_t(s, y, n), k=k), oracle(s, y, n, k), L)


@pytest.mark.parametrize("L", [17, 128, 1000, 4096, 10000])
@pytest.mark.parametrize("dtype", [np.int32, np.float32])
def test_label_dtypes(L, dtype):
    s, y, n = _batch(L + 11, _rows(L), L, dtype=dtype)
    _check(_call(*_t(s, y, n), k=10), oracle(s, y, n, 10), L)


@pytest.mark.parametrize("L", [64, 1000, 10000])
def test_forward_only_and_garbage_in_padded_slots(L):
    s, y, n = _batch(L + 23, _rows(L), L)
    ts, ty, tn = _t(s, y, n)
    loss, ds = _call(ts, ty, tn, k=5)
    fwd, none = _call(ts, ty, tn, k=5, grad=False)
    assert none is None and torch.equal(fwd, loss)
    s2, y2 = s.copy(), y.copy()
    for b in range(s.shape[0]):
        s2[b, n[b]:] = np.nan
        y2[b, n[b]:] = 1 << 40
    loss2, ds2 = _call(*_t(s2, y2, n), k=5)
    assert torch.equal(loss2, loss) and torch.equal(ds2, ds)


@pytest.mark.parametrize("L", [100, 1000, 4096, 5000])
def test_random_ties_follow_the_seeded_tie_words(L):
    from pytorchltr_amd import _ties
    s, y, n = _batch(L + 31, 4, L, grades=3)
    seed = 0x2545F4914F6CDD1D & ((1 << 62) - 1)
    words = _ties.hash_words(seed, L) if L <= 4096 else _ties.hash_words_long(seed, L)
    got = _call(*_t(s, y, n), seed=seed)
    _check(got, oracle(s, y, n, tie=words), L)
    # the tie words decide: index order is another ranking
    idx = oracle(s, y, n)[0]
    assert not np.allclose(got[0].cpu().numpy(), idx, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("L", [1, 17, 128, 300, 1000, 4096])
def test_forced_sort_path_agrees_with_one_workgroup(L):
    s, y, n = _batch(L + 41, 8, L)
    ts, ty, tn = _t(s, y, n)
    for k in (None, 3):
        one = _call(ts, ty, tn, k=k)
        with _LongSortAll():
            srt = _call(ts, ty, tn, k=k)
        torch.testing.assert_close(srt[0], one[0], rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(srt[1], one[1], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("L", [128, 1000, 20000])
def test_repeated_calls_are_bit_identical(L):
    s, y, n = _batch(L + 51, 8, L)
    ts, ty, tn = _t(s, y, n)
    a = _call(ts, ty, tn, seed=12345)
    for _ in range(2):
        b = _call(ts, ty, tn, seed=12345)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("L", [50, 1000, 6000])
@pytest.mark.parametrize("shift,spread", [(1000.0, 2.0), (-1000.0, 2.0), (0.0, 100.0)])
def test_stability(L, shift, spread):
    s, y, n = _batch(L + 61, 4, L, spread=spread)
    s = (s + np.float32(shift)).astype(np.float32)
    for k in (None, 10):
        # (spread 100: scores over about +-200 apart; the loss is large, tolerance relative to its scale)
        _check(_call(*_t(s, y, n), k=k), oracle(s, y, n, k), L, ks=max(1.0, spread / 10))


def test_module_backward_matches_the_oracle():
    from pytorchltr_amd.loss import ListMLELoss
    from pytorchltr_amd.utils import tie_breaking
    for L in (40, 5000):
        s, y, n = _batch(L + 71, 5, L)
        ts, ty, tn = _t(s, y, n)
        ts.requires_grad_(True)
        with tie_breaking("index"):
            loss = ListMLELoss(k=7)(ts.unsqueeze(-1), ty, tn)
            loss.mean().backward()
        wl, wd = oracle(s, y, n, 7)
        np.testing.assert_allclose(loss.detach().cpu().numpy(), wl, rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(ts.grad.cpu().numpy(), wd / s.shape[0], rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("dtype", [torch.float64, torch.bfloat16, torch.float16])
def test_module_dtypes_round_trip(dtype):
    from pytorchltr_amd.loss import ListMLELoss
    from pytorchltr_amd.utils import tie_breaking
    s, y, n = _batch(81, 6, 30)
    ts, ty, tn = _t(s, y, n)
    x = ts.to(dtype).requires_grad_(True)
    with tie_breaking("index"):
        loss = ListMLELoss()(x, ty, tn)
        loss.sum().backward()
        ref = ListMLELoss()(x.detach().float(), ty, tn)
    assert loss.dtype == dtype and x.grad.dtype == dtype and x.grad.shape == x.shape
    tol = 1e-6 if dtype == torch.float64 else 2e-2
    torch.testing.assert_close(loss.float(), ref, rtol=tol, atol=tol)


@pytest.mark.parametrize("L", [100, 5000])
def test_graph_capture_replays_equal_to_eager(L):
    from pytorchltr_amd.loss import ListMLELoss
    from pytorchltr_amd.utils import tie_breaking
    s, y, n = _batch(91 + L, 16, L)
    ts, ty, tn = _t(s, y, n)
    fn = ListMLELoss(k=10)
    with tie_breaking("index"):
        x = ts.clone().requires_grad_(True)
        eager = fn(x, ty, tn)
        eager.sum().backward()
        eager_grad = x.grad.clone()
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
    assert torch.isfinite(eager_grad).all()


def test_drop_in_loop_with_linear_scorer_and_lazy_sgd():
    """Three steps of the reference's loop body with use_linear_scorer + pytorchltr_amd.optim.SGD give the weights of
    torch.optim.SGD on a plain nn.Linear with the same loss."""
    from pytorchltr_amd.fused import use_linear_scorer
    from pytorchltr_amd.loss import ListMLELoss
    from pytorchltr_amd.optim import SGD
    from pytorchltr_amd.utils import tie_breaking
    dev = _dev()
    B, L, F = 32, 60, 24
    g = torch.Generator().manual_seed(5)
    data = [(torch.randn(B, L, F, generator=g).to(dev), torch.randint(0, 5, (B, L), generator=g).to(dev),
             torch.randint(1, L + 1, (B,), generator=g).to(dev)) for _ in range(3)]
    torch.manual_seed(3)
    plain = torch.nn.Linear(F, 1).to(dev)
    fused = use_linear_scorer(copy.deepcopy(plain))
    loss_fn = ListMLELoss(k=10)
    runs = []
    with tie_breaking("index"):
        for model, opt in ((plain, torch.optim.SGD(plain.parameters(), lr=0.05)), (fused, SGD(fused.parameters(), lr=0.05))):
            losses = []
            for xs, ys, n in data:
                loss = loss_fn(model(xs), ys, n).mean()
                opt.zero_grad()
                loss.backward()
                opt.step()
                losses.append(float(loss))
            runs.append(losses)
    np.testing.assert_allclose(runs[1], runs[0], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(fused.weight.detach(), plain.weight.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(fused.bias.detach(), plain.bias.detach(), rtol=1e-5, atol=1e-6)
