"""GPU tier: the lazy SGD step across CHANGING batch sizes and list lengths.

Every other test of the one-launch lazy step (test_gpu_step.py, test_gpu_lazy_quiet.py, test_gpu_optim.py, the two-process
worker) keeps one (B, L, F) for the whole run, so pending_B == B in every launch they make.  Training does not look like that: the
last batch of an epoch is shorter, the first one of the next epoch longer than the pending one, and collate pads every batch to its
own longest list.  Here each step has its own B:

* through the C ABI -- ltr_linear_sgd_lazy_step_f32 + ltr_linear_sgd_flush_f32 against ltr_linear_sgd_step_f32 on ONE workspace
  (NaN-filled, sized for the largest batch) and ONE loss buffer, the header's same-buffer contract: shrinking and growing batches
  inside the one-round range, B = 1, a pending batch of exactly R = 4 x CUs queries, both crossings of R (rows column-group major
  pending with the next batch by query, and back), the empty batch between two steps, the quiet workgroups' range (3 x CUs, R] with
  a pending batch of another size, a scorer without bias (rows by query at every B); and, for the smooth kinds, against an fp64
  trajectory built from the oracle's gradients, so that the eager step is not the only reference;
* through the drop-in path -- the reference's loop body with use_linear_scorer and pytorchltr_amd.optim.SGD against torch.optim.SGD
  on a plain nn.Linear(F, 1), over two epochs with a short last batch, a changing L and a change of the loss: the losses, the
  weights, exactly the flushes _LazyLinear.forward's rule calls for (none on a change of B alone), and the per-query loss buffer
  of every step: large enough for what the launch reads through it, and never recycled."""
import copy

import numpy as np
import pytest
import torch

from oracle import ltr_oracle as O
from tests.conftest import synth

pytestmark = pytest.mark.gpu

LR = 0.05


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _one_round():
    """R: the largest batch whose update rides in the next launch (csrc/ltr_linear_lazy.inc: lazy_one_round) -- 1024 on an MI355X."""
    return 4 * torch.cuda.get_device_properties(_dev()).multi_processor_count


def _sequence():
    R = _one_round()
    return [300, 300, 77, 300, 1, R, R // 2 + 1, R + 1, 300, 2 * R + 452, 64, 0, R - 24, R - 224, 300]


FLUSH_AFTER = (2, 7, 11, 14)          # (0-based: after the 3rd, 8th, 12th and last step)


@pytest.fixture(scope="module")
def steps_of():
    """(B, L) per step -> [(B, L, host tensors, device tensors)], one seed per step; generated once per (shapes, F) and shared by
    the cases (never modified)."""
    cache = {}

    def get(shapes, F, seed=700):
        key = (tuple(shapes), F, seed)
        if key not in cache:
            dev = _dev()
            out = []
            for i, (B, L) in enumerate(shapes):
                if B == 0:
                    out.append((0, L, None, None))
                    continue
                s, y, n, X, W, b = synth(B, L, seed + i, F=F)
                out.append((B, L, (X, y, n), tuple(t.to(dev) for t in (X, y, n))))
            cache[key] = out
        return cache[key]
    yield get
    cache.clear()


def _initial(L, F):
    _, _, _, _, W0, b0 = synth(1, L, 699, F=F)
    return W0, b0


def _run(kind_id, steps, F, W0, b0, lazy, flush_after, has_bias=True):
    """One pass over `steps` with the eager two-launch step or the lazy step (+ the flush at the flush points, and with the
    pending step's own L in front of a step with another L, as the header requires).  The trace: ("loss", k) the first B per-query
    losses of step k, ("bucket", k) its [dW | db | loss_sum], ("W", k) the weights (and the bias) after flush point k."""
    from pytorchltr_amd import _C
    lib = _C.lib()
    dev = _dev()
    R = _one_round()
    st = torch.cuda.current_stream(dev).cuda_stream
    nws = max(lib.ltr_linear_workspace_bytes(B, L, F) for B, L, _, _ in steps)
    Bmax = max(B for B, _, _, _ in steps)
    Wd = W0.clone().to(dev)
    bd = b0.clone().to(dev) if has_bias else None
    bp = bd.data_ptr() if has_bias else None
    ws = torch.full((nws // 4 + 64,), float("nan"), device=dev)
    loss = torch.full((Bmax,), float("nan"), device=dev)
    bucket = torch.zeros(F + 2, device=dev)
    trace = []
    pending, pending_L = 0, 0

    def flush(k):
        nonlocal pending
        _C.check(lib.ltr_linear_sgd_flush_f32(kind_id, Wd.data_ptr(), bp, pending, pending_L, F, LR, loss.data_ptr(),
                                              bucket.data_ptr(), ws.data_ptr(), st))
        pending = 0
        trace.append(("bucket", k, bucket.clone()))

    for k, (B, L, _, d) in enumerate(steps):
        if 0 < B <= R:      # (a re-tuned planner must not quietly take these shapes off the path under test)
            assert lib.ltr_linear_fused_plan(kind_id, B, L, F) == _C.PLAN_REGISTER_TILE, (B, L, F)
        Xp, yp, np_ = (t.data_ptr() for t in d) if B else (None, None, None)
        if lazy:
            if pending and pending_L != L:
                flush(k - 1)
            _C.check(lib.ltr_linear_sgd_lazy_step_f32(kind_id, 1.0, Xp, Wd.data_ptr(), bp, yp, _C.LABEL_I64, np_, B, L, F, LR,
                                                      loss.data_ptr(), bucket.data_ptr(), ws.data_ptr(), ws.numel() * 4, pending,
                                                      st))
            if pending:
                trace.append(("bucket", k - 1, bucket.clone()))          # (the previous step's, written by this call)
            pending, pending_L = B, L       # (B == 0: the call applied the pending update, nothing is pending -- no flush below)
            if B:
                trace.append(("loss", k, loss[:B].clone()))
            if k in flush_after:
                if pending:
                    flush(k)
                trace.append(("W", k, Wd.clone()) + ((bd.clone(),) if has_bias else ()))
        else:
            if B:
                _C.check(lib.ltr_linear_sgd_step_f32(kind_id, 1.0, Xp, Wd.data_ptr(), bp, yp, _C.LABEL_I64, np_, None, B, L, F, LR,
                                                     loss.data_ptr(), bucket.data_ptr(), ws.data_ptr(), ws.numel() * 4, None, st))
                trace.append(("loss", k, loss[:B].clone()))
                trace.append(("bucket", k, bucket.clone()))
            if k in flush_after:
                trace.append(("W", k, Wd.clone()) + ((bd.clone(),) if has_bias else ()))
    torch.cuda.synchronize()
    _C.device_status()                                                   # (e) raises on anything but a clean status
    out = {(e[0], e[1]): [t.cpu().numpy() for t in e[2:]] for e in trace}
    assert len(out) == len(trace)
    return out


def _compare(eager, lazy, again, steps):
    """(a) bit for bit while every batch so far has at most 1024 queries; (b) from the first larger one on the bounds
    test_lazy_sgd_steps_are_the_eager_steps_bit_for_bit states for that regime (reducers that share a column group add their partial
    sums in another -- fixed -- order), and the same BITS run after run; (c) every value finite."""
    assert set(eager) == set(lazy) == set(again)
    big = [k for k, (B, _, _, _) in enumerate(steps) if B > 1024]
    first_big = big[0] if big else len(steps)
    for key in sorted(eager):
        for a, b2, c in zip(eager[key], lazy[key], again[key]):
            assert a.shape == b2.shape
            assert np.all(np.isfinite(a)) and np.all(np.isfinite(b2)), key
            if key[1] < first_big:
                assert np.array_equal(a, b2), (key, float(np.abs(a - b2).max()))
            else:
                assert np.allclose(a, b2, rtol=1e-4, atol=1e-5 * max(1.0, float(np.abs(a).max()))), \
                    (key, float(np.abs(a - b2).max()), float(np.abs(a).max()))
            assert np.array_equal(b2, c), key


def _oracle_trajectory(kind, steps, F, W0, b0, trace, flush_after):
    """(d) the construction and the bounds of test_sgd_step_follows_the_oracles_trajectory: W_{k+1} = W_k - lr * d mean loss / dW at
    W_k with the oracle's fp64 gradients and fp32 weights -- every step's dW, and the weights at the flush points."""
    Wh, bh = W0.clone(), b0.clone()
    for k, (B, L, h, _) in enumerate(steps):
        if B:
            X, y, n = h
            _, _, want_dW, want_db = O.linear_pairwise(kind, X.numpy(), Wh.numpy(), float(bh[0]), y.numpy(), n.numpy(),
                                                       np.full(B, 1.0 / B))
            got = trace[("bucket", k)][0]
            tol = 5e-5 * max(1.0, float(np.max(np.abs(want_dW)))) + 1e-6
            assert np.max(np.abs(got[:F] - want_dW)) < tol, (k, float(np.max(np.abs(got[:F] - want_dW))), tol)
            Wh = (Wh.double() - LR * torch.from_numpy(want_dW)).float()
            bh = (bh.double() - LR * want_db).float()
        if k in flush_after:
            Wg, bg = trace[("W", k)]
            assert np.allclose(Wg, Wh.numpy(), rtol=1e-4, atol=1e-5), (k, float(np.abs(Wg - Wh.numpy()).max()))
            assert np.allclose(bg, bh.numpy(), rtol=1e-4, atol=1e-5), k


# (L > 64: the launch deals its queries in list-length order, p.sched != 0; L <= 64: block id = query)
@pytest.mark.parametrize("kind,L,F,has_bias", [("hinge", 72, 136, True), ("logistic", 72, 136, True), ("ndcg2", 72, 136, True),
                                               ("hinge", 40, 24, True), ("arp2", 40, 24, True), ("hinge", 72, 136, False)],
                         ids=["hinge-72x136", "logistic-72x136", "ndcg2-72x136", "hinge-40x24", "arp2-40x24", "hinge-72x136-no_bias"])
def test_lazy_steps_over_changing_batch_sizes_are_the_eager_steps(steps_of, kind, L, F, has_bias):
    """300, 300, 77, 300, 1, R, R/2 + 1, R + 1, 300, 2R + 452, 64, 0, R - 24, R - 224, 300 queries, each step's update applied by
    the NEXT step's call whatever the two sizes (in its launch when both are at most R, by a flush in front of it otherwise; the
    empty batch -- NULL X / rel / n -- applies it and leaves nothing pending: the weights recorded after it without a flush are
    the eager run's)."""
    from pytorchltr_amd import _C
    kind_id = getattr(_C, kind.upper())
    steps = steps_of([(B, L) for B in _sequence()], F)
    W0, b0 = _initial(L, F)
    eager = _run(kind_id, steps, F, W0, b0, False, FLUSH_AFTER, has_bias)
    lazy = _run(kind_id, steps, F, W0, b0, True, FLUSH_AFTER, has_bias)
    again = _run(kind_id, steps, F, W0, b0, True, FLUSH_AFTER, has_bias)
    _compare(eager, lazy, again, steps)
    # (the hinge kinds' trajectories fork at every pair on the margin -- test_gpu_step.py --: (a) / (b) only)
    if kind in ("logistic", "ndcg2"):
        _oracle_trajectory(kind, steps, F, W0, b0, lazy, FLUSH_AFTER)


@pytest.mark.parametrize("kind", ["logistic", "ndcg2"])
def test_lazy_steps_over_changing_list_lengths_on_one_workspace(steps_of, kind):
    """(B, L) = (300, 72) -> (300, 100) -> (77, 72) on one workspace: the caller flushes with the PENDING step's L in front of a
    step with another L, and the flush finds the rows where that step left them -- their layout follows from (kind, pending_B, L, F)."""
    from pytorchltr_amd import _C
    F = 136
    steps = steps_of([(300, 72), (300, 100), (77, 72)], F)
    W0, b0 = _initial(72, F)
    every = (0, 1, 2)
    eager = _run(getattr(_C, kind.upper()), steps, F, W0, b0, False, every)
    lazy = _run(getattr(_C, kind.upper()), steps, F, W0, b0, True, every)
    _compare(eager, lazy, lazy, steps)
    _oracle_trajectory(kind, steps, F, W0, b0, lazy, every)


# ---------------------------------------------------------------------------------------------
# the drop-in path
# ---------------------------------------------------------------------------------------------
EPOCH = ((300, 72), (300, 72), (300, 60), (77, 72))         # (B, L) of an epoch's four batches: a shorter list, a short last batch
ONE_LENGTH = ((300, 72), (300, 72), (300, 72), (77, 72))    # ... and with B the only thing that changes
DROP_IN_SEED = 1000     # (synth seed base of these batches: test_drop_in_loop_over_two_epochs_with_a_short_last_batch says why)


def _loss_fns(names):
    from pytorchltr_amd import loss as L_
    return [{"logistic": L_.PairwiseLogisticLoss, "ndcg2": L_.LambdaNDCGLoss2}[nm]() for nm in names]


def _train(model, opt, loss_fns, data, sum_on_odd_steps, seen=None):
    """The reference's loop body (examples/01-basic-usage.py:70-75), one loss module per epoch."""
    losses = []
    k = 0
    for loss_fn in loss_fns:
        for xs, ys, n in data:
            per_query = loss_fn(model(xs), ys, n)
            if seen is not None:
                seen(k, per_query)
            loss = per_query.sum() / 300 if (sum_on_odd_steps and k % 2 == 1) else per_query.mean()
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(loss.detach())
            k += 1
    return torch.stack(losses)


def _counting_flushes(fn):
    """Runs fn() and returns how many pending updates were applied by a launch of their own (counted as test_gpu_optim.py does)."""
    from pytorchltr_amd import optim as O_
    count = [0]
    real_flush = O_._LazyLinear.flush

    def flush(self):
        count[0] += 1 if self.pending is not None else 0
        return real_flush(self)
    O_._LazyLinear.flush = flush
    try:
        out = fn()
    finally:
        O_._LazyLinear.flush = real_flush
    return out, count[0]


def _models(F, dev, seed=3):
    """nn.Linear(F, 1) and two use_linear_scorer copies of it (test_gpu_optim.py: _models)."""
    from pytorchltr_amd.fused import use_linear_scorer
    torch.manual_seed(seed)
    lin = torch.nn.Linear(F, 1).to(dev)
    return lin, use_linear_scorer(copy.deepcopy(lin)), use_linear_scorer(copy.deepcopy(lin))


def _oracle_training(lin, epochs, host, sum_on_odd_steps, lr):
    """The same loop with the oracle's fp64 losses and gradients and fp32 weights: (per-step losses, W, bias)."""
    Wh, bh = lin.weight.detach().cpu().reshape(-1).clone(), lin.bias.detach().cpu().clone()
    losses = []
    k = 0
    for kind in epochs:
        for X, y, n in host:
            B = X.shape[0]
            go = np.full(B, 1.0 / 300 if (sum_on_odd_steps and k % 2 == 1) else 1.0 / B)
            loss, _, dW, db = O.linear_pairwise(kind, X.numpy(), Wh.numpy(), float(bh[0]), y.numpy(), n.numpy(), go)
            losses.append(float(np.sum(loss * go)))
            Wh = (Wh.double() - lr * torch.from_numpy(dW)).float()
            bh = (bh.double() - lr * db).float()
            k += 1
    return torch.tensor(losses, dtype=torch.float64), Wh, bh


@pytest.mark.parametrize("shapes,epochs,sum_on_odd_steps,want_flushes", [
    (EPOCH, ("logistic", "ndcg2"), False, 5), (EPOCH, ("logistic", "ndcg2"), True, 5), (ONE_LENGTH, ("logistic", "logistic"), False, 0)],
    ids=["mean", "sum_over_300_on_odd_steps", "only_B_changes"])
def test_drop_in_loop_over_two_epochs_with_a_short_last_batch(steps_of, shapes, epochs, sum_on_odd_steps, want_flushes):
    """Two epochs of B = 300, 300, 300, 77 on one model and optimizer (the logistic loss, then LambdaNDCG2), the loop body of the
    reference unchanged, at the bounds of test_same_training_as_torch_sgd (losses rtol 2e-5 / atol 1e-6, weights rtol 1e-5 / atol
    1e-6) against three references: torch.optim.SGD on a use_linear_scorer copy (that test's set-up), the same loop on the oracle
    (fp64 losses and gradients), and torch.optim.SGD on the plain nn.Linear(F, 1).  `.sum() / 300` on the odd steps: the pending
    upstream gradient alternates between stride 0 and stride 1 with a length that differs from the new B.  `only_B_changes`: one L
    and one loss, so that a change of B is the ONLY thing that happens between two steps (in the two-epoch sequence every change of
    B comes with a change of L or of the loss, which flush for their own reasons).

    The data.  The plain nn.Linear run is an fp32 computation of its own (rocBLAS scores, autograd's gradient), and at these
    shapes -- 300 queries of 72 documents, logistic losses of ~5000 per query, eight steps -- its OWN distance from the oracle's
    fp64 trajectory is of the size of the bound it is held to: measured on an MI355X over the synth seed bases 500, 700, 800, 900,
    1000, 1100 (x the weights' bound; `mean` / `sum_over_300_on_odd_steps` / `only_B_changes`)
        the plain run from the fp64 trajectory   1.28 0.21 0.51 | 0.81 2.66 0.99 | 1.39 2.57 1.68 | 1.41 0.32 1.43 | 0.70 0.26 0.76 | 0.93 0.19 0.59
        the lazy run from the fp64 trajectory    0.33 0.06 0.11 | 0.18 0.04 0.12 | 0.52 2.56 0.13 | 0.40 0.06 0.21 | 0.55 0.05 0.31 | 0.21 0.05 0.17
    (the lazy run bit-identical to torch.optim.SGD on the use_linear_scorer copy in all eighteen).  The figures above 2 are forks,
    not rounding: at the first LambdaNDCG2 step one query's fp32 ranking differs from the fp64 scores' (base 700: two documents
    1.6e-7 apart, in the plain run only; base 800: in every fp32 run), the ranks decide LambdaNDCG2's discounts and the losses are
    1e-5 apart from there on (tests/conftest.py: assert_rank_dependent_losses treats the same thing per row).  A reference that is
    further from the truth than the bound cannot hold anybody to it, so the batches are drawn from the first seed base of that
    list at which the REFERENCE is good -- the plain run within 0.8 x the bound of the fp64 trajectory in all three loops, a
    criterion the code under test has no part in: DROP_IN_SEED = 1000.  The test asserts that property of the reference first, so
    that a reference gone bad is reported as that.  Bounds, references and loops are unchanged; measured there, the lazy run
    from the plain one: 0.65 / 0.26 / 0.69 x the bound."""
    from pytorchltr_amd import _C
    from pytorchltr_amd.optim import SGD
    dev = _dev()
    F = 136
    lr = 0.03
    steps = steps_of(shapes, F, DROP_IN_SEED)
    data = [d for _, _, _, d in steps]
    lin, m_fused, m_lazy = _models(F, dev)
    m_plain = copy.deepcopy(lin)
    l_plain = _train(m_plain, torch.optim.SGD(m_plain.parameters(), lr=lr), _loss_fns(epochs), data, sum_on_odd_steps)
    l_fused = _train(m_fused, torch.optim.SGD(m_fused.parameters(), lr=lr), _loss_fns(epochs), data, sum_on_odd_steps)
    o_lazy = SGD(m_lazy.parameters(), lr=lr)
    l_lazy, flushes = _counting_flushes(lambda: _train(m_lazy, o_lazy, _loss_fns(epochs), data, sum_on_odd_steps))
    # _LazyLinear.forward flushes in front of a step whose (kind, L, F) differs from the pending one's and on nothing else: with
    # L = 72, 72, 60, 72 that is steps 3 and 4 of each epoch (L changes: 2 + 2) and the first step of the second epoch (the kind
    # changes; its B = 300 after 77 alone would not) = 5; with one L and one loss NONE -- the 77-query step takes the 300-query
    # batch's update along, and the 300-query step after it the 77-query batch's
    sig = [(kind, L) for kind in epochs for _, L in shapes]
    assert want_flushes == sum(1 for a, b in zip(sig, sig[1:]) if a != b)
    assert flushes == want_flushes
    st = m_lazy.weight._ltr_lazy
    assert st.pending is not None                                       # the last update: applied when somebody reads the weights
    w = m_lazy.weight.detach().clone()
    assert st.pending is None
    bias = m_lazy.bias.detach().clone()
    _C.device_status()
    l_orc, W_orc, b_orc = _oracle_training(lin, epochs, [h for _, _, h, _ in steps], sum_on_odd_steps, lr)
    W_orc = W_orc.reshape(1, F).to(dev)
    # the reference first (the docstring): the plain fp32 run is itself on the fp64 trajectory at these bounds on this data
    w_plain = m_plain.weight.detach()
    print("the plain nn.Linear run from the oracle's fp64 trajectory: weights %.3g (%.2f x the bound)" % (
        float((w_plain - W_orc).abs().max()), float(((w_plain - W_orc).abs() / (1e-6 + 1e-5 * W_orc.abs())).max())))
    assert torch.allclose(w_plain, W_orc, rtol=1e-5, atol=1e-6), "the REFERENCE left the fp64 trajectory"
    refs = [("torch.optim.SGD on the use_linear_scorer copy", l_fused, m_fused.weight.detach(), m_fused.bias.detach()),
            ("the oracle's fp64 trajectory", l_orc.float().to(dev), W_orc, b_orc.to(dev)),
            ("torch.optim.SGD on the plain nn.Linear", l_plain, w_plain, m_plain.bias.detach())]
    for name, l_want, w_want, b_want in refs:
        print("%s: losses %.3g, weights %.3g (%.2f x the bound), bias %.3g" % (
            name, float((l_lazy - l_want).abs().max()), float((w - w_want).abs().max()),
            float(((w - w_want).abs() / (1e-6 + 1e-5 * w_want.abs())).max()), float((bias - b_want).abs().max())))
        assert torch.allclose(l_lazy, l_want, rtol=2e-5, atol=1e-6), (name, float((l_lazy - l_want).abs().max()))
        assert torch.allclose(w, w_want, rtol=1e-5, atol=1e-6), (name, float((w - w_want).abs().max()))
        assert torch.allclose(bias, b_want, rtol=1e-5, atol=1e-6), name


@pytest.mark.parametrize("shapes,epochs", [(EPOCH, ("logistic", "ndcg2")), (ONE_LENGTH, ("logistic", "logistic"))],
                         ids=["mean", "only_B_changes"])
def test_drop_in_loss_buffer_covers_the_pending_batch_and_is_not_recycled(steps_of, shapes, epochs):
    """The launch that takes the pending update along reads pending_B floats through the CURRENT call's loss pointer (the losses'
    reducer, include/ltr_hip.h): the per-query loss tensor of every step must sit in a storage of at least 4 * max(B, pending_B)
    bytes -- pending_B the previous batch's B unless a flush intervened -- while the user still sees exactly B losses, and the
    tensors of earlier steps keep their values (a user may collect them: no recycled buffer).
    (On a change of B alone nothing flushes: the 77-query step behind a 300-query batch is the case a B-float buffer is too small
    for -- 308 bytes where the launch reads 1200.)"""
    from pytorchltr_amd.optim import SGD
    dev = _dev()
    F = 136
    data = [d for _, _, _, d in steps_of(shapes, F, DROP_IN_SEED)]
    _, _, m_lazy = _models(F, dev)
    o_lazy = SGD(m_lazy.parameters(), lr=0.03)
    kept = []
    # forward's rule: the update of step k - 1 is still pending in step k's launch unless (kind, L) changed in between
    sig = [(kind, L) for kind in epochs for _, L in shapes]
    sizes = [B for _ in epochs for B, _ in shapes]

    def seen(k, per_query):
        B = sizes[k]
        pending_B = sizes[k - 1] if k > 0 and sig[k] == sig[k - 1] else 0
        assert per_query.shape == (B,) and per_query.numel() == B
        assert per_query.untyped_storage().nbytes() >= 4 * max(B, pending_B), (k, B, pending_B, per_query.untyped_storage().nbytes())
        kept.append((per_query, per_query.detach().clone()))

    _train(m_lazy, o_lazy, _loss_fns(epochs), data, False, seen)
    torch.cuda.synchronize()
    assert len(kept) == 8
    for k, (t, copy_) in enumerate(kept):
        assert torch.equal(t.detach(), copy_), k
        assert torch.isfinite(copy_).all(), k
    storages = {t.untyped_storage().data_ptr() for t, _ in kept}
    assert len(storages) == len(kept)


def test_lazy_sgd_module_refuses_a_batch_of_another_size():
    """fused.LazySGD keeps ONE loss buffer and workspace sized for its first batch: a batch of another B is a ValueError (its
    documented limit -- lifting it is a deliberate change), raised before anything is launched: the pending update is still the
    first batch's and flush() applies it."""
    from pytorchltr_amd.fused import LazySGD
    dev = _dev()
    L, F = 40, 24
    _, y, n, X, W, b = synth(32, L, 5, F=F)
    w, bias = W.clone().to(dev), b.clone().to(dev)
    opt = LazySGD(w, bias, LR, loss="logistic")
    opt.step(X.to(dev), y.to(dev), n.to(dev))
    with pytest.raises(ValueError, match="every batch must have the shape of the first one"):
        opt.step(X[:20].to(dev), y[:20].to(dev), n[:20].to(dev))
    assert opt.pending == 32
    _, grad = opt.flush()
    _, _, want_dW, want_db = O.linear_pairwise("logistic", X.numpy(), W.numpy(), float(b[0]), y.numpy(), n.numpy(), np.full(32, 1.0 / 32))
    tol = 5e-5 * max(1.0, float(np.max(np.abs(want_dW)))) + 1e-6
    assert np.max(np.abs(grad[:F].cpu().numpy() - want_dW)) < tol
    assert np.allclose(w.cpu().numpy(), (W.double() - LR * torch.from_numpy(want_dW)).float().numpy(), rtol=1e-4, atol=1e-5)
