"""GPU tier of LambdaRankLoss on lists longer than ltr_max_list_len() documents (run with `-m gpu` on an MI355X):
ltr_lambdarank_long_f32 (include/ltr_lambdarank_long.h) against the blocked fp64 reference of
tests/lambdarank_long_ref.py -- the first long length, one sort chunk, a merge pass, three runs, the bound itself --,
the long path forced onto lists the one-workgroup kernel takes, bit identity (run to run, forward only, a cutoff no row
reaches, garbage in padded slots, label dtypes), degenerate rows, score ties, far-apart scores, stream capture, and the
Python entry points that end in _LambdaRankFunction.  Scores are inputs drawn on the host: the reference ranks the same
fp32 values as the kernel.

Tolerances: on the long path the project's for NDCG-weighted losses there (tests/test_gpu_long_pairs.py::_check_vs_oracle):
loss rtol 2e-3, atol 1e-5; gradient |err| <= 2e-4 max|row| + 1e-5; exactly 0 past n_b.  On lists of at most 4096
documents (the forced path) the short kernel's (tests/test_gpu_lambdarank.py): loss |err| <= 2e-6 + rtol |want| with rtol
1e-5 up to 256 documents and 5e-4 above, gradient |err| <= 1e-5 max|row| + 1e-6.  Every check prints its worst error as
a fraction of its bound."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import lambdarank_long_ref as RL

pytestmark = pytest.mark.gpu

SIGMAS = [1.0, 2.5]
BIG = 1 << 20
PARITY = [(L, k) for L in (4097, 8192, 8193, 12289) for k in (1, 10, 5000, BIG)] + [(4097, None), (8193, None)]


def _dev():
    assert torch.cuda.is_available(), "GPU tier needs a ROCm device"
    return torch.device("cuda:0")


def _ragged(L):
    """B = 3: a full row, a half (at 4097 .. 8192 a row the short kernel would take), a single document."""
    return np.array([L, L // 2, 1], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _batch(L, seed=0, spread=2.0, shift=0.0):
    """Normal scores, integer grades 0..4, n = (L, L // 2, 1).  Cached and read-only: the tests of one length share it."""
    rng = np.random.default_rng(1000 * L + seed)
    s = (rng.normal(0.0, spread, (3, L)) + shift).astype(np.float32)
    y = rng.integers(0, 5, (3, L)).astype(np.int64)
    n = np.minimum(_ragged(L), L)
    for a in (s, y, n):
        a.setflags(write=False)
    return s, y, n


def _no_cutoff(k, n):
    """None where no row reaches the cutoff: the specification is the one without a cutoff, and so is its reference."""
    return None if k is None or k >= int(np.max(n)) else k


@functools.lru_cache(maxsize=None)
def _want_cached(L, k, sigma, seed, spread, shift):
    loss, ds = RL.batch(*_batch(L, seed, spread, shift), k=k, sigma=sigma)
    loss.setflags(write=False)
    ds.setflags(write=False)
    return loss, ds


def _want(L, k, sigma, seed=0, spread=2.0, shift=0.0):
    """The reference of `_batch`, computed once per distinct case and left unchanged."""
    return _want_cached(L, _no_cutoff(k, _batch(L, seed, spread, shift)[2]), sigma, seed, spread, shift)


def _t(*arrays):
    # (copies: the cached batches are read-only)
    return [torch.from_numpy(np.array(a)).to(_dev()) for a in arrays]


def _call(ts, ty, tn, k=None, sigma=1.0, grad=True, short=False):
    """ltr_lambdarank_long_f32 on the current stream, outputs and workspace preset to NaN bytes: (loss, dscores or None).
    `short`: ltr_lambdarank_f32 instead."""
    from pytorchltr_amd import _C
    lib = _C.lib()
    Bq, L = ts.shape
    loss = torch.full((Bq,), float("nan"), dtype=torch.float32, device=ts.device)
    ds = torch.full((Bq, L), float("nan"), dtype=torch.float32, device=ts.device) if grad else None
    if short:
        _C.check(lib.ltr_lambdarank_f32(_C.ptr(ts), _C.ptr(ty), _C.label_dtype(ty), _C.ptr(tn), int(k or 0), float(sigma),
                                        Bq, L, _C.ptr(loss), _C.ptr(ds), _C.stream_of(ts)))
    else:
        nbytes = int(lib.ltr_lambdarank_long_workspace_bytes(int(k or 0), Bq, L))
        assert nbytes > 0
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=ts.device)
        _C.check(lib.ltr_lambdarank_long_f32(_C.ptr(ts), _C.ptr(ty), _C.label_dtype(ty), _C.ptr(tn), int(k or 0),
                                             float(sigma), Bq, L, _C.ptr(loss), _C.ptr(ds), _C.ptr(ws), nbytes,
                                             _C.stream_of(ts)))
    torch.cuda.synchronize()
    return loss, ds


def _check_long(got, want, n, what):
    """The long path's tolerances (module docstring)."""
    gl, gd = got
    wl, wd = want
    gl = gl.detach().cpu().numpy().astype(np.float64)
    err = np.abs(gl - wl)
    bound = 1e-5 + 2e-3 * np.abs(wl)
    print("%s: loss worst err / bound %.4f (max err %.3e)" % (what, (err / bound).max(), err.max()))
    assert np.all(np.isfinite(gl)), what
    assert np.all(err <= bound), (what, gl, wl)
    if gd is not None:
        gd = gd.detach().cpu().numpy().astype(np.float64)
        gerr = np.abs(gd - wd).max(axis=1)
        gbound = 2e-4 * np.abs(wd).max(axis=1) + 1e-5
        print("%s: grad worst err / bound %.4f (max err %.3e)" % (what, (gerr / gbound).max(), gerr.max()))
        assert np.all(np.isfinite(gd)), what
        assert np.all(gerr <= gbound), (what, gerr, gbound)
        for b in range(len(n)):
            assert np.all(gd[b, int(n[b]):] == 0.0), what              # exactly 0 past n[b]


def _check_short(got, want, L, what):
    """The short kernel's tolerances (tests/test_gpu_lambdarank.py::_check)."""
    gl, gd = got
    wl, wd = want
    gl = gl.cpu().numpy().astype(np.float64)
    err = np.abs(gl - wl)
    bound = 2e-6 + (1e-5 if L <= 256 else 5e-4) * np.abs(wl)
    print("%s: loss worst err / bound %.4f (max err %.3e)" % (what, (err / bound).max(), err.max()))
    assert np.all(np.isfinite(gl)), what
    assert np.all(err <= bound), (what, gl, wl)
    gd = gd.cpu().numpy().astype(np.float64)
    gerr = np.abs(gd - wd).max(axis=1)
    gbound = 1e-5 * np.abs(wd).max(axis=1) + 1e-6
    print("%s: grad worst err / bound %.4f (max err %.3e)" % (what, (gerr / gbound).max(), gerr.max()))
    assert np.all(np.isfinite(gd)), what
    assert np.all(gerr <= gbound), (what, gerr, gbound)


def _same(a, b):
    return torch.equal(a[0], b[0]) and (a[1] is None or b[1] is None or torch.equal(a[1], b[1]))


# ---- parity ----
@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("L,k", PARITY)
def test_parity_against_the_reference(L, k, sigma):
    s, y, n = _batch(L)
    _check_long(_call(*_t(s, y, n), k=k, sigma=sigma), _want(L, k, sigma), n, "parity L=%d k=%s sigma=%s" % (L, k, sigma))


def test_the_bound_itself():
    """65 536 documents, NDCG@10: K n work on both sides."""
    from pytorchltr_amd import _C
    L, k = 65536, 10
    assert L == _C.max_pair_list_len()
    rng = np.random.default_rng(65536)
    s = rng.normal(0.0, 2.0, (2, L)).astype(np.float32)
    y = rng.integers(0, 5, (2, L)).astype(np.int64)
    n = np.array([65536, 40000], dtype=np.int64)
    _check_long(_call(*_t(s, y, n), k=k), RL.batch(s, y, n, k=k), n, "the bound")


# ---- the long path on lists the short kernel takes ----
@pytest.mark.parametrize("k", [None, 1, 10])
@pytest.mark.parametrize("L", [1, 2, 3, 64, 65, 257, 1000, 4096])
def test_forced_long_path_on_short_lists(L, k):
    """Each of the two paths against the fp64 reference at the short kernel's tolerances (not against each other: the
    orders of summation differ)."""
    from pytorchltr_amd import _C
    lib = _C.lib()
    rng = np.random.default_rng(77 * L + (k or 0))
    s = rng.normal(0.0, 2.0, (3, L)).astype(np.float32)
    y = rng.integers(0, 5, (3, L)).astype(np.int64)
    n = np.array([L, max(L // 2, 1), 1], dtype=np.int64)
    sigma = 2.5 if k == 10 else 1.0
    want = RL.batch(s, y, n, k=k, sigma=sigma)
    ts, ty, tn = _t(s, y, n)
    prev = lib.ltr_debug_lambdarank_long_all(1)
    try:
        assert lib.ltr_debug_lambdarank_long_all(1) == 1               # returns the old value
        forced = _call(ts, ty, tn, k=k, sigma=sigma)
    finally:
        lib.ltr_debug_lambdarank_long_all(prev)
    assert lib.ltr_lambdarank_long_workspace_bytes(int(k or 0), 3, L) == 0
    _check_short(forced, want, L, "forced long path L=%d k=%s" % (L, k))
    _check_short(_call(ts, ty, tn, k=k, sigma=sigma, short=True), want, L, "ltr_lambdarank_f32 L=%d k=%s" % (L, k))
    gd = forced[1].cpu().numpy()
    for b in range(3):
        assert np.all(gd[b, int(n[b]):] == 0.0)
    # without the hook the long entry point IS the short one there: no workspace, the same bits
    loss = torch.empty(3, dtype=torch.float32, device=ts.device)
    ds = torch.empty(3, L, dtype=torch.float32, device=ts.device)
    _C.check(lib.ltr_lambdarank_long_f32(_C.ptr(ts), _C.ptr(ty), _C.label_dtype(ty), _C.ptr(tn), int(k or 0), sigma, 3, L,
                                         _C.ptr(loss), _C.ptr(ds), None, 0, _C.stream_of(ts)))
    torch.cuda.synchronize()
    assert _same((loss, ds), _call(ts, ty, tn, k=k, sigma=sigma, short=True))


# ---- exactness at 8193 documents ----
EX = 8193


def test_repeated_and_forward_only_calls_are_bit_identical():
    ts, ty, tn = _t(*_batch(EX))
    for k in (None, 10, 5000):
        a = _call(ts, ty, tn, k=k)
        b = _call(ts, ty, tn, k=k)
        assert _same(a, b), k
        fwd, none = _call(ts, ty, tn, k=k, grad=False)
        assert none is None and torch.equal(fwd, a[0]), k


def test_a_cutoff_no_row_reaches_is_no_cutoff():
    ts, ty, tn = _t(*_batch(EX))
    full = _call(ts, ty, tn, k=None, sigma=2.5)
    for k in (EX, EX + 1, BIG):
        assert _same(_call(ts, ty, tn, k=k, sigma=2.5), full), k


def test_garbage_in_padded_slots_changes_nothing():
    s, y, n = _batch(EX)
    yf = y.astype(np.float32)
    for k in (10, 5000):
        want = _call(*_t(s, yf, n), k=k)
        for junk in (np.nan, 1e30):
            s2, y2 = s.copy(), yf.copy()
            for b in range(3):
                s2[b, n[b]:] = junk
                y2[b, n[b]:] = junk
            assert _same(_call(*_t(s2, y2, n), k=k), want), (k, junk)
        assert torch.isfinite(want[0]).all() and torch.isfinite(want[1]).all()


def test_label_dtypes_agree_bit_for_bit():
    s, y, n = _batch(EX)
    a = _call(*_t(s, y, n), k=10)
    for dtype in (np.int32, np.float32):
        assert _same(_call(*_t(s, y.astype(dtype), n), k=10), a), dtype


# ---- degenerate rows at 4097 documents ----
DG = 4097


def test_degenerate_list_lengths():
    k = 10
    s, y, _ = _batch(DG)
    rng = np.random.default_rng(4)
    s = np.concatenate([s, rng.normal(0.0, 2.0, (3, DG)).astype(np.float32)])
    y = np.concatenate([y, rng.integers(0, 5, (3, DG))])
    n = np.array([0, 1, 2, k, k + 1, DG], dtype=np.int64)
    got = _call(*_t(s, y, n), k=k)
    _check_long(got, RL.batch(s, y, n, k=k), n, "n_b in {0, 1, 2, k, k + 1}")
    assert not got[0][:2].any() and not got[1][:2].any()
    assert got[0][5] > 0


def test_equal_labels_give_zero():
    s, _, n = _batch(DG)
    ts, tn = _t(s, n)
    for labels in (torch.full((3, DG), 3, dtype=torch.int64), torch.zeros((3, DG), dtype=torch.int64),
                   torch.full((3, DG), 1.5, dtype=torch.float32)):
        for k in (None, 5):
            loss, ds = _call(ts, labels.to(ts.device), tn, k=k)
            assert not loss.any() and not ds.any()


def test_no_positive_gain_has_max_dcg_one():
    s, y, n = _batch(DG)
    yf = np.where(y >= 2, 0.0, -1.0).astype(np.float32)                # gains 0 and -0.5: maxDCG@10 = 0 -> 1
    assert RL.max_dcg(yf[0], 10) == 1.0
    got = _call(*_t(s, yf, n), k=10)
    _check_long(got, RL.batch(s, yf, n, k=10), n, "no positive gain")
    assert got[0][0] > 0


def test_a_float_label_of_minus_one_has_gain_minus_a_half():
    s, y, n = _batch(DG)
    yf = (y - 1).astype(np.float32)                                    # -1 .. 3
    assert (yf == -1).any()
    got_f = _call(*_t(s, yf, n), k=5)
    _check_long(got_f, RL.batch(s, yf, n, k=5), n, "a grade of -1")
    assert _same(_call(*_t(s, y - 1, n), k=5), got_f)                  # the float formula whatever the dtype


# ---- ties ----
def test_all_scores_equal_rank_in_index_order():
    _, y, n = _batch(DG)
    s = np.full((3, DG), 0.25, dtype=np.float32)
    for k in (10, None):
        _check_long(_call(*_t(s, y, n), k=k), RL.batch(s, y, n, k=k), n, "all scores equal k=%s" % k)


def _descending_with_a_tie(rng, L, lo, hi):
    """Distinct scores, 0.01 apart, with the ranks [lo, hi) tied, in a random document order."""
    base = (np.arange(L, 0, -1) * 0.01).astype(np.float32)
    base[lo:hi] = base[lo]
    return base[rng.permutation(L)]


def test_a_tie_straddling_the_cutoff():
    L, k = DG, 10
    rng = np.random.default_rng(5)
    s = np.stack([_descending_with_a_tie(rng, L, k - 2, k + 3) for _ in range(3)])
    _, y, _ = _batch(L)
    n = np.full(3, L, dtype=np.int64)
    got = _call(*_t(s, y, n), k=k)
    _check_long(got, RL.batch(s, y, n, k=k), n, "a tie straddling K")
    # the rule matters here: the tied documents in the reverse order are another loss
    rev = RL.batch(s[:, ::-1], y[:, ::-1], n, k=k)[0]
    assert not np.allclose(got[0].cpu().numpy(), rev, rtol=1e-4, atol=1e-6)


def test_a_tie_straddling_a_sort_chunk_boundary():
    """The documents at positions 8188 .. 8196 of 12 289 -- two sort chunks, put in index order by the merge -- share
    the highest score, and the cutoff lies inside the block: their order decides who has a discount."""
    L, k = 12289, 5
    rng = np.random.default_rng(6)
    s = rng.normal(0.0, 2.0, (2, L)).astype(np.float32)
    y = rng.integers(0, 5, (2, L)).astype(np.int64)
    s[:, 8188:8197] = 50.0
    y[:, 8188:8197] = np.array([0, 4, 1, 3, 2, 0, 4, 1, 3])
    n = np.array([L, 8195], dtype=np.int64)                            # (the second row ends inside the block)
    got = _call(*_t(s, y, n), k=k)
    _check_long(got, RL.batch(s, y, n, k=k), n, "a tie straddling position 8192")
    # the rule matters here: the tied documents in the reverse order are another loss
    rev = RL.batch(s[:, ::-1], y[:, ::-1], np.array([L, L], dtype=np.int64), k=k)[0]
    assert abs(got[0][0].item() - rev[0]) > 1e-3 * abs(rev[0])


# ---- stability ----
@pytest.mark.parametrize("k", [None, 10])
def test_far_apart_scores_stay_finite_and_on_the_reference(k):
    s, y, n = _batch(DG, 7, 1e3, 1e4)
    _check_long(_call(*_t(s, y, n), k=k), _want(DG, k, 1.0, 7, 1e3, 1e4), n, "far-apart scores k=%s" % k)


# ---- stream capture ----
def test_graph_capture_replays_equal_to_eager():
    from pytorchltr_amd.loss import LambdaRankLoss
    s, y, n = _batch(DG)
    ts, ty, tn = _t(s[:2], y[:2], n[:2])
    fn = LambdaRankLoss(k=10)
    x = ts.clone().requires_grad_(True)
    eager = fn(x, ty, tn)
    eager.sum().backward()
    want_grad = x.grad.clone()
    static = ts.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn(static, ty, tn).sum().backward()                            # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    static.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = fn(static, ty, tn)
        cap.sum().backward()
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap.detach(), eager.detach())
    assert torch.equal(static.grad, want_grad)


# ---- the Python paths, each at 2 x 4100 ----
PB, PL, PF, PK = 2, 4100, 8, 10


@functools.lru_cache(maxsize=None)
def _py_data():
    rng = np.random.default_rng(41)
    X = rng.normal(0.0, 1.0, (PB, PL, PF)).astype(np.float32)
    y = rng.integers(0, 5, (PB, PL)).astype(np.int64)
    n = np.array([PL, PL // 3], dtype=np.int64)
    s = rng.normal(0.0, 2.0, (PB, PL)).astype(np.float32)
    for a in (X, y, n, s):
        a.setflags(write=False)
    return X, y, n, s


def test_module_backward_matches_the_reference():
    from pytorchltr_amd.loss import LambdaRankLoss
    _, y, n, s = _py_data()
    ts, ty, tn = _t(s, y, n)
    want = RL.batch(s, y, n, k=PK, sigma=2.5)
    ts.requires_grad_(True)
    loss = LambdaRankLoss(sigma=2.5, k=PK)(ts.unsqueeze(-1), ty, tn)
    assert loss.shape == (PB,)
    loss.mean().backward()
    _check_long((loss, ts.grad * PB), want, n, "module")
    wts = torch.tensor([0.5, 2.0], device=ts.device)
    ts.grad = None
    (LambdaRankLoss(sigma=2.5, k=PK)(ts, ty, tn) * wts).sum().backward()
    _check_long((loss, ts.grad), (want[0], want[1] * wts.cpu().numpy()[:, None].astype(np.float64)), n, "weighted sum")


def test_a_list_past_the_bound_raises():
    from pytorchltr_amd.loss import LambdaRankLoss
    L = 65537
    dev = _dev()
    with pytest.raises(ValueError, match=r"max_pair_list_len\(\)"):
        LambdaRankLoss(k=10)(torch.zeros(1, L, device=dev), torch.zeros(1, L, dtype=torch.int64, device=dev),
                             torch.tensor([L], device=dev))


def _close_loss(got, want):
    """tests/test_gpu_linear_lambdarank.py: the module tests' loss tolerance."""
    assert torch.allclose(got.detach(), want.detach(), rtol=2e-5, atol=1e-5), (got - want).abs().max().item()


def _close_grads(dW, db, want_dW, want_db):
    """tests/test_gpu_linear_lambdarank.py: one absolute tolerance, from the weight gradient, for dW and db."""
    tol = 1e-5 * max(1.0, float(want_dW.abs().max()))
    assert torch.allclose(dW.reshape(-1), want_dW.reshape(-1), rtol=1e-4, atol=tol), (dW.reshape(-1) - want_dW.reshape(-1)).abs().max().item()
    assert torch.allclose(db.reshape(-1), want_db.reshape(-1), rtol=1e-4, atol=tol), (db.reshape(-1) - want_db.reshape(-1)).abs().max().item()


def _on_own_scores(loss, scores, y, n, sigma, what):
    """The loss of a launch against the reference on the scores that launch computed."""
    sc = scores.detach().reshape(PB, PL).cpu().numpy().copy()
    for b in range(PB):
        sc[b, int(n[b]):] = 0.0
    _check_long((loss, None), RL.batch(sc, y, n, k=PK, sigma=sigma), n, what)


def test_fused_linear_entry_points_agree_with_the_plain_layer():
    """FusedLinearLoss, linear_loss_step and the drop-in on LazyScores past 4096 documents: the plan declines, and the
    scorer, ltr_lambdarank_long_f32 and the weight-gradient kernel run -- against LinearScorer + module + autograd."""
    from pytorchltr_amd import _C
    from pytorchltr_amd.fused import FusedLinearLoss, LinearScorer, linear_loss_step, use_linear_scorer
    from pytorchltr_amd.loss import LambdaRankLoss
    X, y, n, _ = _py_data()
    tX, ty, tn = _t(X, y, n)
    assert _C.lib().ltr_linear_lambdarank_plan(PB, PL, PF) == 0
    loss_fn = LambdaRankLoss(sigma=2.5, k=PK)
    torch.manual_seed(3)
    plain = LinearScorer(PF, lazy=False).to(_dev())                     # (every call computes its scores)
    plain_scores = plain(tX)
    want = loss_fn(plain_scores, ty, tn)                               # scorer + LambdaRankLoss + autograd
    want.mean().backward()
    _on_own_scores(want, plain_scores, y, n, 2.5, "LinearScorer + module")

    fused = FusedLinearLoss(PF, loss=loss_fn).to(_dev())
    fused.load_state_dict(plain.state_dict())
    got, scores = fused(tX, ty, tn, return_scores=True)
    got.mean().backward()
    _on_own_scores(got, scores, y, n, 2.5, "FusedLinearLoss")
    _close_loss(got, want)
    _close_grads(fused.weight.grad, fused.bias.grad, plain.weight.grad, plain.bias.grad)

    lossv, dW, db, sc = linear_loss_step(tX, plain.weight.detach(), plain.bias.detach(), ty, tn, loss=loss_fn,
                                         return_scores=True)
    _on_own_scores(lossv, sc, y, n, 2.5, "linear_loss_step")
    _close_loss(lossv, want)
    _close_grads(dW, db, plain.weight.grad, plain.bias.grad)
    lossv2, dW2, db2 = linear_loss_step(tX, plain.weight.detach(), plain.bias.detach(), ty, tn, loss="lambdarank")[:3]
    assert lossv2.shape == (PB,) and torch.isfinite(lossv2).all() and torch.isfinite(dW2).all()

    lin = torch.nn.Sequential(torch.nn.Linear(PF, 1)).to(_dev())
    with torch.no_grad():
        lin[0].weight.copy_(plain.weight.reshape(1, PF))
        lin[0].bias.copy_(plain.bias.reshape(1))
    model = use_linear_scorer(copy.deepcopy(lin))
    lazy = model(tX)
    out = loss_fn(lazy, ty, tn)
    out.mean().backward()
    _close_loss(out, want)
    _close_grads(model[0].weight.grad, model[0].bias.grad, plain.weight.grad, plain.bias.grad)


def test_a_bf16_batch_through_fused_linear_loss():
    """The bf16 scorer and weight-gradient kernels around the long loss: the loss against the reference on the launch's
    own scores, the weight gradient against fp64 sums of the loss gradient on those scores times the bf16 features."""
    from pytorchltr_amd.fused import FusedLinearLoss
    from pytorchltr_amd.loss import LambdaRankLoss
    X, y, n, _ = _py_data()
    tX, ty, tn = _t(X, y, n)
    x16 = tX.to(torch.bfloat16)
    torch.manual_seed(4)
    m = FusedLinearLoss(PF, loss=LambdaRankLoss(k=PK)).to(_dev())
    loss, scores = m(x16, ty, tn, return_scores=True)
    loss.mean().backward()
    _on_own_scores(loss, scores, y, n, 1.0, "FusedLinearLoss on bf16")
    # the scores are the bf16 features times the fp32 weights
    Xd = x16.float().cpu().numpy().astype(np.float64)
    want_s = Xd @ m.weight.detach().cpu().numpy().astype(np.float64).reshape(-1) + float(m.bias.detach())
    real = np.arange(PL)[None, :] < n[:, None]
    np.testing.assert_allclose(scores.cpu().numpy()[real], want_s[real], rtol=1e-4, atol=1e-5)
    # dW from the stand-alone loss gradient on those scores
    sc = (scores * torch.from_numpy(real).to(scores.device)).contiguous()
    _, g = _call(sc, ty, tn, k=PK)
    g = g.cpu().numpy().astype(np.float64) / PB
    want_dW = np.einsum("bl,blf->f", g, Xd)
    want_db = g.sum()
    dW = m.weight.grad.cpu().numpy().astype(np.float64).reshape(-1)
    db = float(m.bias.grad)
    tol = 2e-4 * np.max(np.abs(want_dW)) + 1e-5
    print("bf16: dW err / bound %.4f" % (np.max(np.abs(dW - want_dW)) / tol))
    assert np.all(np.abs(dW - want_dW) <= tol) and abs(db - want_db) <= tol


def test_loss_on_the_scores_of_an_mlp_scorer():
    """loss_fn(MLPScorer(...)(xs, n), ys, n) as with any loss: real scores in, gradients out to the layers."""
    from pytorchltr_amd.fused import MLPScorer
    from pytorchltr_amd.loss import LambdaRankLoss
    X, y, n, _ = _py_data()
    tX, ty, tn = _t(X, y, n)
    torch.manual_seed(2)
    m = MLPScorer(PF).to(_dev())
    scores = m(tX, tn)
    loss = LambdaRankLoss(k=PK)(scores, ty, tn)
    loss.mean().backward()
    _on_own_scores(loss, scores, y, n, 1.0, "MLPScorer + module")
    for p in m.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all()
    assert m.l1.weight.grad.abs().max() > 0
