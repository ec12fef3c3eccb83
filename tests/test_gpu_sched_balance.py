"""GPU tier: the register tile's dealing by hosting CU (csrc/ltr_common.inc: sched_slot_cu) on grids of whole rounds.

Which block id takes which query decides speed only.  On B = 2, 3 and 4 x #CUs queries of ragged lists (L = 72: the scheduling
needs L > 64; n from 1 to L), narrow rows (F = 8: the lazy launch's quiet rule off), F = 64 (quiet rule on for hinge at four
rounds) and once the headline's F = 136 (36 reducers), hinge and LambdaNDCG2, int64 labels:
  * the plain launch (ltr_linear_partials_f32) writes every loss -- none of the NaNs the buffer was filled with is left -- and
    loss[b] and query b's partial row are BIT-IDENTICAL to the same queries launched in sub-batches of one round of CUs (at
    B <= #CUs + #CUs / 8 there is no scheduling, and a query's arithmetic does not depend on its workgroup);
  * three lazy steps (ltr_linear_sgd_lazy_step_dp_f32) over two batches + the flush give the weights, bias, buckets and losses
    of ltr_linear_sgd_step_f32 on the same inputs, bit for bit;
  * the device status word stays clear."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

L = 72


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _batches(T, F):
    """two batches of T x #CUs queries and the initial weights, on the device; made once per shape, never written"""
    dev = _dev()
    B = T * _cus()
    g = torch.Generator().manual_seed(1000 * T + F)
    out = []
    for _ in range(2):
        y = torch.randint(0, 5, (B, L), generator=g)
        n = torch.randint(1, L + 1, (B,), generator=g)
        n[0], n[1], n[B // 2], n[B - 1] = 1, L, L, 1
        X = torch.randn(B, L, F, generator=g)
        out.append((X.to(dev), y.to(dev), n.to(dev)))
    W = (torch.rand(F, generator=g) * 2 - 1) / F ** 0.5
    b = (torch.rand(1, generator=g) * 2 - 1) / F ** 0.5
    return B, out, W.to(dev), b.to(dev)


CASES = [(T, F) for T in (2, 3, 4) for F in (8, 64)] + [(4, 136)]


@pytest.mark.parametrize("kind", ["hinge", "ndcg2"])
@pytest.mark.parametrize("T,F", CASES)
def test_plain_launch_is_the_sub_batches_bit_for_bit(T, F, kind):
    from pytorchltr_amd import _C
    lib = _C.lib()
    dev = _dev()
    cus = _cus()
    B, batches, W, b = _batches(T, F)
    X, y, n = batches[0]
    kind_id = getattr(_C, kind.upper())
    st = _C.stream_of(X)
    PF = (F + 4) & ~3                                       # pitch of a query's partial row [dW | db]

    def launch(Xs, ys, ns):
        Bs = Xs.shape[0]
        loss = torch.full((Bs,), float("nan"), device=dev)
        part = torch.full((lib.ltr_linear_workspace_bytes(Bs, L, F) // 4,), float("nan"), device=dev)
        _C.check(lib.ltr_linear_partials_f32(kind_id, 1.0, Xs.data_ptr(), W.data_ptr(), b.data_ptr(), ys.data_ptr(), _C.LABEL_I64,
                                             ns.data_ptr(), Bs, L, F, loss.data_ptr(), None, part.data_ptr(), st))
        torch.cuda.synchronize()
        return loss.cpu().numpy(), part[:Bs * PF].view(Bs, PF)[:, :F + 1].cpu().numpy()

    loss, rows = launch(X, y, n)
    assert not np.isnan(loss).any()
    assert not np.isnan(rows).any()
    for s in range(0, B, cus):
        want_loss, want_rows = launch(X[s:s + cus], y[s:s + cus], n[s:s + cus])
        assert np.array_equal(loss[s:s + cus], want_loss), s
        assert np.array_equal(rows[s:s + cus], want_rows), s
    assert lib.ltr_device_status(0) == 0


@pytest.mark.parametrize("kind", ["hinge", "ndcg2"])
@pytest.mark.parametrize("T,F", CASES)
def test_lazy_steps_are_the_eager_steps_bit_for_bit(T, F, kind):
    from pytorchltr_amd import _C
    lib = _C.lib()
    dev = _dev()
    B, batches, W0, b0 = _batches(T, F)
    kind_id = getattr(_C, kind.upper())
    st = _C.stream_of(W0)
    nws = lib.ltr_linear_workspace_bytes(B, L, F)
    lr = 0.05

    def run(lazy):
        Wd, bd = W0.clone(), b0.clone()
        ws = torch.full((nws // 4 + 64,), float("nan"), device=dev)
        loss = torch.empty(B, device=dev)
        bucket = torch.zeros(F + 2, device=dev)
        trace = []
        pending = 0
        for k in range(3):
            Xd, yd, nd = batches[k % 2]
            if lazy:
                _C.check(lib.ltr_linear_sgd_lazy_step_dp_f32(kind_id, 1.0, Xd.data_ptr(), Wd.data_ptr(), bd.data_ptr(), yd.data_ptr(),
                                                             _C.LABEL_I64, nd.data_ptr(), B, L, F, lr, loss.data_ptr(), bucket.data_ptr(),
                                                             ws.data_ptr(), ws.numel() * 4, pending, 0.0, None, 0, None, st))
                if pending:
                    trace.append(("bucket", k - 1, bucket.clone()))      # (the previous step's, written by this launch)
                pending = B
                trace.append(("loss", k, loss.clone()))
                if k == 2:
                    _C.check(lib.ltr_linear_sgd_flush_dp_f32(kind_id, Wd.data_ptr(), bd.data_ptr(), pending, L, F, lr, 0.0, None, 0,
                                                             loss.data_ptr(), bucket.data_ptr(), ws.data_ptr(), None, st))
                    pending = 0
                    trace.append(("bucket", k, bucket.clone()))
                    trace.append(("W", k, Wd.clone(), bd.clone()))
            else:
                _C.check(lib.ltr_linear_sgd_step_f32(kind_id, 1.0, Xd.data_ptr(), Wd.data_ptr(), bd.data_ptr(), yd.data_ptr(),
                                                     _C.LABEL_I64, nd.data_ptr(), None, B, L, F, lr, loss.data_ptr(),
                                                     bucket.data_ptr(), ws.data_ptr(), ws.numel() * 4, None, st))
                trace.append(("loss", k, loss.clone()))
                trace.append(("bucket", k, bucket.clone()))
                if k == 2:
                    trace.append(("W", k, Wd.clone(), bd.clone()))
        torch.cuda.synchronize()
        assert lib.ltr_device_status(0) == 0
        return {(e[0], e[1]): [t.cpu().numpy() for t in e[2:]] for e in trace}

    eager, lazy = run(False), run(True)
    assert set(eager) == set(lazy)
    for key in sorted(eager):
        for a, b2 in zip(eager[key], lazy[key]):
            assert np.all(np.isfinite(a)), key
            assert np.array_equal(a, b2), key
