"""GPU tier of the fused Linear step of the listwise losses (run with `-m gpu` on an MI355X):
ltr_linear_listwise_partials_f32 -- scores, ListNet / ListMLE row and weight-gradient row in one launch -- against fp64
references built from its own scores and the stand-alone kernels' gradients, then FusedLinearLoss, linear_loss_step and
the LinearScorer drop-in on top of it.  Index tie order unless a test says otherwise."""
import copy
import functools

import numpy as np
import pytest
import torch

from oracle import ltr_oracle as O
from tests.test_gpu_listmle import _call as listmle_call
from tests.test_listmle_host import oracle

pytestmark = pytest.mark.gpu

LISTNET, LISTMLE = 0, 1
LENGTHS = [1, 2, 17, 64, 65, 128, 129, 256, 257, 1000, 2000, 4096]
SHAPES = [(L, F) for L in LENGTHS for F in (4, 24, 136)] + [(128, 700), (4096, 700)]


def _dev():
    assert torch.cuda.is_available(), "GPU tier needs a ROCm device"
    return torch.device("cuda:0")


def _data(seed, B, L, F, dtype=np.int64, grades=5):
    """Normal features; normal weights of variance 1 / F, so the scores are N(0, 1) at every width and neither softmax
    saturates; labels in [0, grades); n = 0, 1, L, L + 7, then random."""
    rng = np.random.default_rng(seed)
    X = rng.normal(0.0, 1.0, (B, L, F)).astype(np.float32)
    W = (rng.normal(0.0, 1.0, F) / np.sqrt(F)).astype(np.float32)
    bias = np.float32(rng.normal())
    if dtype == np.float32:
        y = (rng.integers(0, 2 * grades, (B, L)) * 0.5).astype(np.float32)
    else:
        y = rng.integers(0, grades, (B, L)).astype(dtype)
    n = rng.integers(0, L + 1, B).astype(np.int64)
    for i, v in enumerate((0, 1, L, L + 7)):
        if i < B:
            n[i] = v
    return X, W, bias, y, n


def _t(*arrays):
    return [torch.from_numpy(np.asarray(a)).to(_dev()) for a in arrays]


def _fused(loss, X, W, bias, y, n, k=None, seed=None, want_scores=True):
    """One ltr_linear_listwise_partials_f32 call on device tensors: (loss_out (B), scores_out (B, L) or None,
    partials (B, PF))."""
    from pytorchltr_amd import _C
    lib = _C.lib()
    B, L, F = X.shape
    PF = (F + 4) & ~3
    assert lib.ltr_linear_listwise_plan(loss, B, L, F) == 1
    nbytes = int(lib.ltr_linear_workspace_bytes(B, L, F))
    assert nbytes >= 4 * B * PF
    ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=X.device)
    out = torch.full((B,), float("nan"), dtype=torch.float32, device=X.device)
    sc = torch.full((B, L), float("nan"), dtype=torch.float32, device=X.device) if want_scores else None
    _C.check(lib.ltr_linear_listwise_partials_f32(
        loss, int(k or 0), _C.ptr(X), _C.ptr(W), _C.ptr(bias), _C.ptr(y), _C.label_dtype(y), _C.ptr(n), None,
        int(seed is not None), seed or 0, None, B, L, F, _C.ptr(out), _C.ptr(sc), _C.ptr(ws), _C.stream_of(X)))
    torch.cuda.synchronize()
    return out, sc, ws[:B * PF].reshape(B, PF).clone()


def _softmax(sc, y, n):
    from pytorchltr_amd._autograd import LISTWISE_SOFTMAX, pairwise_loss_and_grad
    return pairwise_loss_and_grad(sc, y, n, LISTWISE_SOFTMAX)


def _standalone(loss, sc, y, n, k=None, seed=None):
    """(loss, dscores) of the stand-alone kernel on the scores `sc`."""
    return _softmax(sc, y, n) if loss == LISTNET else listmle_call(sc, y, n, k=k, seed=seed)


def _rows_reference(X, g32, n):
    """fp64 [sum_j g32[b, j] X[b, j, :] | sum_j g32[b, j]] over the real documents."""
    B, L, F = X.shape
    g = np.where(np.arange(L)[None, :] < np.minimum(n, L)[:, None], g32.astype(np.float64), 0.0)
    Xm = np.where((np.arange(L)[None, :] < np.minimum(n, L)[:, None])[:, :, None], X.astype(np.float64), 0.0)
    return np.concatenate([np.einsum("bl,blf->bf", g, Xm), g.sum(1, keepdims=True)], axis=1)


def _check_rows(part, X, g32, n):
    """The partial rows against the fp64 reference (tolerance of tests/test_gpu_fused.py's gradient checks): pad columns
    and the rows of empty queries exactly 0."""
    F = X.shape[2]
    got = part.cpu().numpy()
    assert np.all(got[:, F + 1:] == 0.0)
    assert np.all(got[np.asarray(n) <= 0] == 0.0)
    want = _rows_reference(X, g32, n)
    for b in range(X.shape[0]):
        np.testing.assert_allclose(got[b, :F + 1], want[b], rtol=1e-4, atol=1e-5 * max(1.0, np.abs(want[b]).max()))
    return want


def _reduce(part, go, F):
    from pytorchltr_amd import _C
    B = part.shape[0]
    dW = torch.empty(F, dtype=torch.float32, device=part.device)
    db = torch.empty(1, dtype=torch.float32, device=part.device)
    _C.check(_C.lib().ltr_linear_reduce_f32(_C.ptr(part), _C.ptr(go), B, F, _C.ptr(dW), _C.ptr(db), _C.stream_of(part)))
    torch.cuda.synchronize()
    return np.concatenate([dW.cpu().numpy(), db.cpu().numpy()])


@functools.lru_cache(maxsize=None)
def _case(L, F):
    X, W, bias, y, n = _data(1000 * L + F, 6, L, F)
    return (X, W, bias, y, n) + tuple(_t(X, W, np.array([bias]), y, n))


@pytest.mark.parametrize("L,F", SHAPES)
def test_scores(L, F):
    X, W, bias, y, n, tX, tW, tb, ty, tn = _case(L, F)
    want = X.astype(np.float64) @ W.astype(np.float64) + np.float64(bias)
    real = np.arange(L)[None, :] < np.minimum(n, L)[:, None]
    for loss in (LISTNET, LISTMLE):
        out, sc, part = _fused(loss, tX, tW, tb, ty, tn)
        got = sc.cpu().numpy()
        assert np.all(got[~real] == 0.0)                               # padded documents: exactly 0
        np.testing.assert_allclose(got[real], want[real], rtol=1e-5, atol=1e-5)
        out2, none, part2 = _fused(loss, tX, tW, tb, ty, tn, want_scores=False)
        assert none is None and torch.equal(out, out2) and torch.equal(part, part2)
        # no bias: the scores move by it
        _, sc0, _ = _fused(loss, tX, tW, None, ty, tn)
        np.testing.assert_allclose(sc0.cpu().numpy()[real], (want - np.float64(bias))[real], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("L,F", SHAPES)
@pytest.mark.parametrize("k", [None, 1, 10])
def test_listmle_row_and_partial_rows(L, F, k):
    X, W, bias, y, n, tX, tW, tb, ty, tn = _case(L, F)
    out, sc, part = _fused(LISTMLE, tX, tW, tb, ty, tn, k=k)
    loss, g32 = listmle_call(sc, ty, tn, k=k)
    assert torch.equal(out, loss)                                      # one row function: bit for bit
    wl, _ = oracle(sc.cpu().numpy(), y, n, k)
    np.testing.assert_allclose(out.cpu().numpy().astype(np.float64), wl, rtol=1e-4, atol=1e-4)
    want = _check_rows(part, X, g32.cpu().numpy(), n)
    go = torch.from_numpy(np.random.default_rng(L + F).normal(size=6).astype(np.float32)).to(_dev())
    ref = go.cpu().numpy().astype(np.float64) @ want
    np.testing.assert_allclose(_reduce(part, go, F), ref, rtol=1e-4, atol=1e-5 * max(1.0, np.abs(ref).max()))


@pytest.mark.parametrize("L,F", SHAPES)
def test_listnet_row_and_partial_rows(L, F):
    X, W, bias, y, n, tX, tW, tb, ty, tn = _case(L, F)
    out, sc, part = _fused(LISTNET, tX, tW, tb, ty, tn)
    wl, _ = O.listwise_softmax(sc.cpu().numpy(), y, n)
    np.testing.assert_allclose(out.cpu().numpy().astype(np.float64), wl, rtol=1e-5, atol=2e-6)
    assert out[0].item() == 0.0                                        # n = 0
    _, g32 = _softmax(sc, ty, tn)
    want = _check_rows(part, X, g32.cpu().numpy(), n)
    go = torch.from_numpy(np.random.default_rng(L + F).normal(size=6).astype(np.float32)).to(_dev())
    ref = go.cpu().numpy().astype(np.float64) @ want
    np.testing.assert_allclose(_reduce(part, go, F), ref, rtol=1e-4, atol=1e-5 * max(1.0, np.abs(ref).max()))


def _cus():
    return torch.cuda.get_device_properties(_dev()).multi_processor_count


@pytest.mark.parametrize("which", ["one_wave", "half_width_sort"])
def test_launch_shapes_picked_from_the_batch_size(which):
    if which == "one_wave":
        # linear_listwise_kernel<1, 2> on 64 threads (ListNet: <0, 0> on 64 threads): metric_shape gives lists of
        # 65..128 documents one wave per query from 64 queries per CU on
        B, L, F = max(16384, 64 * _cus()), 100, 8
        assert B >= 64 * _cus()
    else:
        # linear_listwise_kernel<1, -2> on 256 threads: metric_shape halves the sort workgroups (two keys per thread)
        # from 16 queries per CU on
        B, L, F = max(4096, 16 * _cus()), 300, 4
        assert B >= 16 * _cus()
    X, W, bias, y, n = _data(5, B, L, F)
    tX, tW, tb, ty, tn = _t(X, W, np.array([bias]), y, n)
    real = np.arange(L)[None, :] < np.minimum(n, L)[:, None]
    want_s = X.astype(np.float64) @ W.astype(np.float64) + np.float64(bias)
    for loss in (LISTNET, LISTMLE):
        out, sc, part = _fused(loss, tX, tW, tb, ty, tn)
        got = sc.cpu().numpy()
        assert np.all(got[~real] == 0.0)
        np.testing.assert_allclose(got[real], want_s[real], rtol=1e-5, atol=1e-5)
        sl, g32 = _standalone(loss, sc, ty, tn)
        if loss == LISTMLE:
            assert torch.equal(out, sl)
        else:
            np.testing.assert_allclose(out.cpu().numpy(), O.listwise_softmax(got, y, n)[0], rtol=1e-5, atol=2e-6)
        got_rows, want = part.cpu().numpy(), _rows_reference(X, g32.cpu().numpy(), n)
        assert np.all(got_rows[:, F + 1:] == 0.0) and np.all(got_rows[n <= 0] == 0.0)
        tol = 1e-5 * np.maximum(1.0, np.abs(want).max(1, keepdims=True))
        assert np.all(np.abs(got_rows[:, :F + 1] - want) <= tol + 1e-4 * np.abs(want))


@pytest.mark.parametrize("L,F", [(300, 64), (64, 136), (4096, 700)])
@pytest.mark.parametrize("loss", [LISTNET, LISTMLE])
def test_no_row_lost_or_counted_twice(L, F, loss):
    """Indicator features X[b, j, f] = (f == j % F), W = 1, bias = 0: dW_b[f] is the sum of the g_j with j = f (mod F),
    j < n_b -- at most ceil(L / F) terms; one term for F >= L, where it must be g itself."""
    _, _, _, y, n = _data(L + F, 6, L, F)
    X = np.zeros((6, L, F), dtype=np.float32)
    j = np.arange(L)
    X[:, j, j % F] = 1.0
    tX, tW, ty, tn = _t(X, np.ones(F, dtype=np.float32), y, n)
    out, sc, part = _fused(loss, tX, tW, None, ty, tn)
    real = np.arange(L)[None, :] < np.minimum(n, L)[:, None]
    assert np.all(sc.cpu().numpy() == real.astype(np.float32))
    _, g32 = _standalone(loss, sc, ty, tn)
    g32 = np.where(real, g32.cpu().numpy(), np.float32(0.0))
    got = part.cpu().numpy()
    want = np.zeros((6, F))
    for f in range(min(F, L)):
        want[:, f] = g32[:, f::F].astype(np.float64).sum(1)
    np.testing.assert_allclose(got[:, :F], want, rtol=1e-6, atol=1e-7)
    # db, a sum that cancels (ListMLE: to 0): at most 4 additions in a thread, 6 in its wave and 16 over the waves, each
    # off by at most 2^-24 of the magnitudes added; ListNet's g carries another few 2^-24 from the other sum order
    assert np.all(np.abs(got[:, F] - g32.astype(np.float64).sum(1)) <= 32 * 2.0 ** -24 * np.abs(g32).sum(1))
    if F >= L:
        assert np.array_equal(got[:, :L], g32) and np.all(got[:, L:F] == 0.0)


@pytest.mark.parametrize("L,F", [(17, 24), (129, 136), (1000, 24), (4096, 136)])
def test_padding_is_never_read(L, F):
    X, W, bias, y, n = _data(L + 3, 6, L, F)
    X2, y2 = X.copy(), y.copy()
    for b in range(6):
        X2[b, max(int(n[b]), 0):] = np.nan
        y2[b, max(int(n[b]), 0):] = 1 << 40
    tX, tW, tb, ty, tn = _t(X, W, np.array([bias]), y, n)
    tX2, ty2 = _t(X2, y2)
    for loss in (LISTNET, LISTMLE):
        clean = _fused(loss, tX, tW, tb, ty, tn, k=5)
        dirty = _fused(loss, tX2, tW, tb, ty2, tn, k=5)
        for a, b in zip(clean, dirty):
            assert torch.equal(a, b)
        assert torch.isfinite(clean[0]).all() and torch.isfinite(clean[2]).all()


@pytest.mark.parametrize("L", [17, 1000])
@pytest.mark.parametrize("dtype", [np.int32, np.float32])
def test_label_dtypes(L, dtype):
    F = 24
    X, W, bias, y, n = _data(L + 11, 6, L, F, dtype=dtype)
    tX, tW, tb, ty, tn = _t(X, W, np.array([bias]), y, n)
    out, sc, part = _fused(LISTMLE, tX, tW, tb, ty, tn, k=10)
    loss, g32 = listmle_call(sc, ty, tn, k=10)
    assert torch.equal(out, loss)
    np.testing.assert_allclose(out.cpu().numpy(), oracle(sc.cpu().numpy(), y, n, 10)[0], rtol=1e-4, atol=1e-4)
    _check_rows(part, X, g32.cpu().numpy(), n)
    out, sc, part = _fused(LISTNET, tX, tW, tb, ty, tn)
    np.testing.assert_allclose(out.cpu().numpy(), O.listwise_softmax(sc.cpu().numpy(), y, n)[0], rtol=1e-5, atol=2e-6)
    _check_rows(part, X, _softmax(sc, ty, tn)[1].cpu().numpy(), n)


@pytest.mark.parametrize("L", [100, 1000])
def test_seeded_ties(L):
    F, seed = 24, 0x1234567 + L
    X, W, bias, y, n = _data(L + 29, 6, L, F, grades=3)
    tX, tW, tb, ty, tn = _t(X, W, np.array([bias]), y, n)
    out, sc, part = _fused(LISTMLE, tX, tW, tb, ty, tn, seed=seed)
    loss, g32 = listmle_call(sc, ty, tn, seed=seed)
    assert torch.equal(out, loss)
    _check_rows(part, X, g32.cpu().numpy(), n)
    idx, _, _ = _fused(LISTMLE, tX, tW, tb, ty, tn)
    assert not torch.equal(out, idx)                                   # another order of the tied grades


@pytest.mark.parametrize("L", [128, 4096])
def test_run_to_run_bit_identity(L):
    X, W, bias, y, n = _data(L + 31, 6, L, 136)
    tX, tW, tb, ty, tn = _t(X, W, np.array([bias]), y, n)
    for loss in (LISTNET, LISTMLE):
        first = _fused(loss, tX, tW, tb, ty, tn)
        for _ in range(2):
            for a, b in zip(first, _fused(loss, tX, tW, tb, ty, tn)):
                assert torch.equal(a, b)


# ---- the modules ----
def _losses():
    from pytorchltr_amd.loss import ListMLELoss, ListwiseSoftmaxLoss
    return [ListwiseSoftmaxLoss(), ListMLELoss(), ListMLELoss(k=10)]


def _close_loss(got, want):
    """tests/test_gpu_fused.py:371."""
    assert torch.allclose(got.detach(), want.detach(), rtol=2e-5, atol=1e-5), (got - want).abs().max().item()


def _close_grads(dW, db, want_dW, want_db):
    """tests/test_gpu_fused.py:372-374: one absolute tolerance, from the weight gradient, for dW and db (the bias
    gradient of ListMLE is 0 up to rounding, as a pairwise loss's is)."""
    tol = 1e-5 * max(1.0, float(want_dW.abs().max()))
    assert torch.allclose(dW.reshape(-1), want_dW.reshape(-1), rtol=1e-4, atol=tol), (dW.reshape(-1) - want_dW.reshape(-1)).abs().max().item()
    assert torch.allclose(db.reshape(-1), want_db.reshape(-1), rtol=1e-4, atol=tol), (db.reshape(-1) - want_db.reshape(-1)).abs().max().item()


@pytest.mark.parametrize("i", range(3))
@pytest.mark.parametrize("B,L,F", [(64, 100, 136), (6, 50, 46), (3, 4100, 8)])
def test_fused_linear_loss_agrees_with_the_plain_layer(i, B, L, F):
    """(64, 100, 136): the fused launch; F = 46 and L = 4100: ltr_linear_listwise_plan says 0, the three kernels."""
    from pytorchltr_amd import _C
    from pytorchltr_amd.fused import FusedLinearLoss, linear_loss_step
    from pytorchltr_amd.utils import tie_breaking
    loss_fn = _losses()[i]
    X, _, _, y, n = _data(7 + i, B, L, F)
    tX, ty, tn = _t(X, y, n)
    assert _C.lib().ltr_linear_listwise_plan(LISTNET, B, L, F) == (1 if F == 136 else 0)
    torch.manual_seed(3)
    plain = torch.nn.Linear(F, 1).to(_dev())
    fused = FusedLinearLoss(F, loss=loss_fn).to(_dev())
    fused.load_state_dict(plain.state_dict())                          # the same keys and shapes
    w = torch.rand(B, device=_dev())
    with tie_breaking("index"):
        for reduce in (lambda out: (out * w).sum(), lambda out: out.mean()):
            plain.zero_grad()
            fused.zero_grad()
            want = loss_fn(plain(tX), ty, tn)
            reduce(want).backward()
            got = fused(tX, ty, tn)
            reduce(got).backward()
            _close_loss(got, want)
            _close_grads(fused.weight.grad, fused.bias.grad, plain.weight.grad, plain.bias.grad)
        got, scores = fused(tX, ty, tn, return_scores=True)
        real = torch.arange(L, device=_dev())[None, :] < tn.clamp(max=L)[:, None]
        want_s = plain(tX).squeeze(-1).detach() * real
        assert scores.shape == (B, L) and torch.allclose(scores * real, want_s, rtol=1e-5, atol=1e-5)
        lossv, dW, db, lsum = linear_loss_step(tX, plain.weight.detach(), plain.bias.detach(), ty, tn, loss=loss_fn,
                                               return_loss_sum=True)
        _close_loss(lossv, want)
        _close_grads(dW, db, plain.weight.grad, plain.bias.grad)       # (the last pass above was .mean())
        assert torch.allclose(lsum, want.detach().sum().reshape(1), rtol=2e-5, atol=1e-5)


@pytest.mark.parametrize("i", range(3))
def test_drop_in_never_writes_a_score_matrix(i):
    from pytorchltr_amd.evaluation import ndcg
    from pytorchltr_amd.fused import use_linear_scorer
    from pytorchltr_amd.utils import tie_breaking
    loss_fn = _losses()[i]
    B, L, F = 64, 100, 136
    X, _, _, y, n = _data(17 + i, B, L, F)
    n = np.maximum(n, 1)
    tX, ty, tn = _t(X, y, n)
    torch.manual_seed(5)
    plain = torch.nn.Sequential(torch.nn.Linear(F, 1)).to(_dev())
    model = use_linear_scorer(copy.deepcopy(plain))
    with tie_breaking("index"):
        loss_fn(plain(tX), ty, tn).mean().backward()
        scores = model(tX)
        out = loss_fn(scores, ty, tn)
        assert scores._real is None                                    # scorer, loss and rows in one launch
        out.mean().backward()
        _close_loss(out, loss_fn(plain(tX), ty, tn))
        _close_grads(model[0].weight.grad, model[0].bias.grad, plain[0].weight.grad, plain[0].bias.grad)
        # scores a metric has used are real; the loss takes them as they are
        model.zero_grad()
        scores = model(tX)
        ndcg(scores, ty, tn, k=10)
        assert scores._real is not None
        out = loss_fn(scores, ty, tn)
        out.mean().backward()
        _close_loss(out, loss_fn(plain(tX), ty, tn))
        _close_grads(model[0].weight.grad, model[0].bias.grad, plain[0].weight.grad, plain[0].bias.grad)


def test_capture_and_replay():
    """Forward + backward of FusedLinearLoss(loss="listmle") captured with torch.cuda.graph and replayed twice: the
    eager result bit for bit."""
    from pytorchltr_amd.fused import FusedLinearLoss
    from pytorchltr_amd.utils import tie_breaking
    B, L, F = 32, 60, 24
    X, _, _, y, n = _data(41, B, L, F)
    tX, ty, tn = _t(X, y, n)
    torch.manual_seed(7)
    m = FusedLinearLoss(F, loss="listmle").to(_dev())

    def step():
        out = m(tX, ty, tn)
        out.mean().backward()
        return out.detach()

    with tie_breaking("index"):
        eager = (step().clone(), m.weight.grad.clone(), m.bias.grad.clone())
        m.zero_grad(set_to_none=True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                                  # (warm-up on a side stream, as torch asks)
            step()
        torch.cuda.current_stream().wait_stream(side)
        m.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        # (backward runs on autograd's thread: the capture is this thread's and the streams it hands on, as in
        # pytorchltr_amd.graphed.GraphedStep)
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            cap = step()
        for _ in range(2):
            cap.fill_(float("nan"))
            m.weight.grad.zero_()
            m.bias.grad.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(cap, eager[0])
            assert torch.equal(m.weight.grad, eager[1]) and torch.equal(m.bias.grad, eager[2])
