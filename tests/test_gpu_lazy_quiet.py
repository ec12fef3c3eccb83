"""GPU tier: the lazy step under the list-length order with QUIET workgroups (csrc/ltr_common.inc: sched_slot, sched_quiet).

A lazy launch puts its reducer workgroups in front of the grid; the query workgroups that share the reducers' CUs take the
batch's shortest lists and hold their bursts back longer than everybody else.  Which block id takes which query decides speed
only: three lazy steps over two batches + the flush are held BIT FOR BIT against the eager two-launch steps
(ltr_linear_sgd_step_f32) -- weights, every step's bucket [dW | db | loss sum] and per-query losses -- at the batch sizes where
the map changes shape: a full last round (4 x #CUs), one short of it, 400 (a batch size whose snake dealing left workgroups
without a query before the rounds were reversed only when complete), 300 (one round and a bit), LambdaNDCG2 with the lists in
ascending order of n (the map moves every query), and narrow rows (four reducers only).  The library turns the quiet rule on
where it was measured to pay (the hinge kinds on wide rows and a full grid); every case runs a second time with the rule forced
on through ltr_debug_lazy_holdback, so that the map is held at every shape."""
import numpy as np
import pytest
import torch

from tests.conftest import synth

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


CASES = {
    "a_four_per_cu": ("hinge", lambda: 4 * _cus(), 128, 136, False),
    "b_one_short": ("hinge", lambda: 4 * _cus() - 1, 128, 136, False),
    "c_400": ("hinge", lambda: 400, 128, 136, False),
    "d_300": ("hinge", lambda: 300, 128, 136, False),
    "e_ndcg2_ascending": ("ndcg2", lambda: 512, 128, 136, True),
    "f_narrow_rows": ("hinge", lambda: 1024, 128, 8, False),
}


@pytest.mark.parametrize("forced", [False, True], ids=["library", "quiet_forced"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_lazy_steps_with_quiet_workgroups_are_the_eager_steps_bit_for_bit(case, forced):
    from pytorchltr_amd import _C
    lib = _C.lib()
    if forced:
        lib.ltr_debug_lazy_holdback(0 | 8 << 8)       # everybody's hold-back 0, the quiet workgroups' 8 x 512 cycles
    try:
        _lazy_against_eager(_C, lib, case)
    finally:
        lib.ltr_debug_lazy_holdback(-1)


def _lazy_against_eager(_C, lib, case):
    dev = _dev()
    kind, Bf, L, F, ascending = CASES[case]
    B = Bf()
    kind_id = getattr(_C, kind.upper())
    lr = 0.05
    batches = []
    for i in range(2):
        s, y, n, X, W, b = synth(B, L, 41 + i, F=F)
        if ascending:
            n = torch.sort(n).values
        batches.append([t.to(dev) for t in (X, y, n)])
    _, _, _, _, W0, b0 = synth(B, L, 41, F=F)
    st = _C.stream_of(batches[0][0])
    nws = lib.ltr_linear_workspace_bytes(B, L, F)

    def run(lazy):
        Wd, bd = W0.clone().to(dev), b0.clone().to(dev)
        ws = torch.full((nws // 4 + 64,), float("nan"), device=dev)
        loss = torch.empty(B, device=dev)
        bucket = torch.zeros(F + 2, device=dev)
        trace = []
        pending = 0
        for k in range(3):
            Xd, yd, nd = batches[k % 2]
            if lazy:
                _C.check(lib.ltr_linear_sgd_lazy_step_f32(kind_id, 1.0, Xd.data_ptr(), Wd.data_ptr(), bd.data_ptr(), yd.data_ptr(),
                                                          _C.LABEL_I64, nd.data_ptr(), B, L, F, lr, loss.data_ptr(), bucket.data_ptr(),
                                                          ws.data_ptr(), ws.numel() * 4, pending, st))
                if pending:
                    trace.append(("bucket", k - 1, bucket.clone()))      # (the previous step's, written by this launch)
                pending = B
                trace.append(("loss", k, loss.clone()))
                if k == 2:
                    _C.check(lib.ltr_linear_sgd_flush_f32(kind_id, Wd.data_ptr(), bd.data_ptr(), pending, L, F, lr, loss.data_ptr(),
                                                          bucket.data_ptr(), ws.data_ptr(), st))
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
        _C.device_status()
        return {(e[0], e[1]): [t.cpu().numpy() for t in e[2:]] for e in trace}

    eager, lazy = run(False), run(True)
    assert set(eager) == set(lazy)
    for key in sorted(eager):
        for a, b2 in zip(eager[key], lazy[key]):
            assert np.all(np.isfinite(a)), key
            assert np.array_equal(a, b2), key


def test_every_query_is_visited_at_a_batch_of_400():
    """ltr_linear_partials_f32 at 400 x 128 x 136 on NaN-prefilled outputs: 400 workgroups, 400 losses and partial rows written
    (an incomplete round dealt backwards left some of them to a workgroup that had taken another's query)."""
    from pytorchltr_amd import _C
    from pytorchltr_amd.fused import linear_loss_step
    dev = _dev()
    B, L, F = 400, 128, 136
    s, y, n, X, W, b = synth(B, L, 77, F=F)
    X, W, b, y, n = X.to(dev), W.to(dev), b.to(dev), y.to(dev), n.to(dev)
    lib = _C.lib()
    loss = torch.full((B,), float("nan"), device=dev)
    part = torch.full((lib.ltr_linear_workspace_bytes(B, L, F) // 4,), float("nan"), device=dev)
    _C.check(lib.ltr_linear_partials_f32(0, 1.0, X.data_ptr(), W.data_ptr(), b.data_ptr(), y.data_ptr(),
                                         _C.label_dtype(y), n.data_ptr(), B, L, F, loss.data_ptr(), None,
                                         part.data_ptr(), _C.stream_of(X)))
    torch.cuda.synchronize()
    assert not torch.isnan(loss).any()
    assert not torch.isnan(part[:B * (F + 1)]).any()
    # the values do not depend on the map: the unscheduled general kernel, which the score output selects
    want, _, _, _ = linear_loss_step(X, W, b, y, n, loss="hinge", return_scores=True)
    assert torch.allclose(loss, want, rtol=2e-5, atol=1e-5)
