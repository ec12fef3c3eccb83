"""CPU tier: the register tile's dealing by hosting CU (csrc/ltr_common.inc: sched_slot_cu), enumerated on the host through
ltr_debug_sched_slots_cu -- the same function the kernel calls.

Block id nred + i of a launch sits on CU slot (nred + i) % cus; it takes member `rank` of sample group `group`, the group's
members ranked by n descending (the low three bits ignored, ties by member order, as in test_sched_slot.py::_order).  A CU's
load is modelled as the sum of n over the ids it hosts.
  * Bijection: every rank below its group's size, every query taken once, the quiet workgroups on the last order indices.
  * Lists linear in rank: the CUs' sums are equal (T = 2, 4) or two rank steps apart (the quiet launch; T = 3).
  * bench.py's own list lengths: max / mean rows per CU under the caps, and below sched_slot's on every batch."""
import ctypes

import numpy as np
import pytest
import torch

L = 128
LOW_BITS = 3


def _hooks():
    from pytorchltr_amd import _C
    return _C.lib().ltr_debug_sched_slots_cu, _C.lib().ltr_debug_sched_slots


def _order(B, G, n, low=LOW_BITS):
    """order[g, r] = the query that member rank r of group g selects (-1 past the group's size), size[g]."""
    k = np.arange(64)
    ids = ((k[None, :] >> 3) * G + np.arange(G)[:, None]) * 8 + (k[None, :] & 7)          # (G, 64): member k of group g
    valid = ids < B
    key = np.where(valid, np.clip(n[np.minimum(ids, B - 1)], 0, L) >> low, -1)
    perm = np.argsort(-key, axis=1, kind="stable")                                        # descending n, ties by member order
    order = np.take_along_axis(np.where(valid, ids, -1), perm, axis=1)
    return order, valid.sum(axis=1)


def _slots(hook, B, cus, nred, *quiet):
    G = (B + 63) // 64
    group = np.empty(B, dtype=np.int32)
    rank = np.empty(B, dtype=np.int32)
    rc = hook(B, G, cus, nred, *quiet, group.ctypes.data_as(ctypes.c_void_p), rank.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, (rc, B, cus, nred, quiet)
    return group, rank


def _cu_rows(n, group, rank, B, cus, nred, low=LOW_BITS):
    """rows (sum of n) of the queries every CU slot hosts"""
    order, size = _order(B, B // 64, n, low)
    assert np.all(rank < size[group])
    q = order[group, rank]
    assert np.array_equal(np.sort(q), np.arange(B))
    rows = np.zeros(cus)
    np.add.at(rows, (nred + np.arange(B)) % cus, n[q])
    return rows


def _linear_lengths(B):
    """n = 2 (64 - rank) in every group"""
    G = B // 64
    k = np.arange(64)
    ids = ((k[None, :] >> 3) * G + np.arange(G)[:, None]) * 8 + (k[None, :] & 7)
    n = np.empty(B, dtype=np.int64)
    n[ids] = 2 * (64 - k)[None, :]
    return n


@pytest.mark.parametrize("cus", [64, 256])
@pytest.mark.parametrize("T", [2, 3, 4])
def test_bijection(cus, T):
    new, _ = _hooks()
    B = T * cus
    assert B % 64 == 0
    G = B // 64
    n = np.random.default_rng(100 * cus + T).integers(1, L + 1, size=B)
    order, size = _order(B, G, n)
    for nred in (0, 2, 36, 56):
        for quiet in ((0, 1) if nred > 0 else (0,)):
            group, rank = _slots(new, B, cus, nred, quiet)
            assert group.min() >= 0 and group.max() < G and rank.min() >= 0, (nred, quiet)
            assert np.all(rank < size[group]), (nred, quiet)
            assert np.array_equal(np.sort(order[group, rank]), np.arange(B)), (nred, quiet)
            if quiet:
                ids = nred + np.arange(B)
                is_quiet = (ids >= cus) & (ids % cus < nred)
                tail = B - T * (cus - nred)
                assert is_quiet.sum() == tail
                o = rank.astype(np.int64) * G + group                      # the order index
                assert np.array_equal(np.sort(o[is_quiet]), np.arange(B - tail, B)), nred
                assert o[~is_quiet].max() < B - tail


def test_where_the_dealing_does_not_apply():
    new, _ = _hooks()
    buf = np.empty(4096, dtype=np.int32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    for B, cus, nred, quiet in ((1024, 0, 0, 0), (1000, 250, 0, 0), (1024, 304, 0, 0), (1280, 256, 0, 0), (256, 256, 0, 0),
                                (1024, 256, 0, 1), (1024, 256, 256, 1), (1024, 256, 256, 0), (1024, 256, -1, 0)):
        assert new(B, (B + 63) // 64, cus, nred, quiet, p, p) == -2, (B, cus, nred, quiet)       # LTR_ERR_SHAPE


def test_linear_lengths_every_cu_the_same_rows():
    new, old = _hooks()
    cus = 256
    # T = 4
    n = _linear_lengths(1024)
    rows = _cu_rows(n, *_slots(new, 1024, cus, 0, 0), 1024, cus, 0, low=0)
    assert rows.min() == 260 and rows.max() == 260
    rows = _cu_rows(n, *_slots(new, 1024, cus, 36, 0), 1024, cus, 36, low=0)                    # lazy launch, quiet rule off
    assert rows.min() == 260 and rows.max() == 260
    rows = _cu_rows(n, *_slots(new, 1024, cus, 36, 1), 1024, cus, 36, low=0)[36:]
    assert rows.min() >= 294 and rows.max() <= 298 and rows.max() - rows.min() <= 4, (rows.min(), rows.max())
    # T = 2: the same exactness
    n = _linear_lengths(512)
    rows = _cu_rows(n, *_slots(new, 512, cus, 0, 0), 512, cus, 0, low=0)
    assert rows.min() == 130 and rows.max() == 130
    rows = _cu_rows(n, *_slots(new, 512, cus, 36, 1), 512, cus, 36, low=0)[36:]
    assert rows.max() - rows.min() <= 4, (rows.min(), rows.max())
    # T = 3: straight, then the slots' halves by parity -- even and odd slots one order index apart, which is at most one rank
    # step (2 rows) per round that crosses a rank boundary: 4 rows, against sched_slot's 174 .. 216
    n = _linear_lengths(768)
    for nred, quiet in ((0, 0), (36, 1)):
        rows = _cu_rows(n, *_slots(new, 768, cus, nred, quiet), 768, cus, nred, low=0)[nred if quiet else 0:]
        was = _cu_rows(n, *_slots(old, 768, cus, nred if quiet else 0), 768, cus, nred, low=0)[nred if quiet else 0:]
        assert rows.max() - rows.min() <= 4, (rows.min(), rows.max())
        assert rows.max() - rows.min() < was.max() - was.min()


def test_the_benchmarks_own_lengths():
    """Seeds 0-4 of bench.synth (X, drawn last, left out).  The caps are the midpoints between the model of this dealing and
    sched_slot's figures: plain 1.149 (1.125-1.186) against 1.238 (1.204-1.268); the quiet lazy launch's non-quiet CUs 1.108
    (1.087-1.123) against 1.348 (1.288-1.382)."""
    new, old = _hooks()
    B, cus, nred = 1024, 256, 36
    plain, lazy = [], []
    for seed in range(5):
        g = torch.Generator().manual_seed(seed)
        torch.randn(B, L, generator=g)
        torch.randint(0, 5, (B, L), generator=g)
        n = torch.randint(1, L + 1, (B,), generator=g).numpy()
        rows = _cu_rows(n, *_slots(new, B, cus, 0, 0), B, cus, 0)
        was = _cu_rows(n, *_slots(old, B, cus, 0), B, cus, 0)
        plain.append(rows.max() / rows.mean())
        assert plain[-1] < was.max() / was.mean(), seed
        rows = _cu_rows(n, *_slots(new, B, cus, nred, 1), B, cus, nred)[nred:]
        was = _cu_rows(n, *_slots(old, B, cus, nred), B, cus, nred)[nred:]
        lazy.append(rows.max() / rows.mean())
        assert lazy[-1] < was.max() / was.mean(), seed
    print("plain max/mean", plain, "quiet lazy, non-quiet CUs", lazy)
    assert np.mean(plain) <= 1.19
    assert np.mean(lazy) <= 1.22
