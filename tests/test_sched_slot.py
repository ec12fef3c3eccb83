"""CPU tier: the block id -> list-length position map of the in-kernel scheduling (csrc/ltr_common.inc: sched_slot), enumerated
on the host through ltr_debug_sched_slots -- the same function the kernels call.

Block id nred + i of a launch takes member `rank` of sample group `group`; the group's members are ranked by n descending (the
low three bits ignored, ties by member order: sched_query_sampled's radix select) and the block takes that member's query.
For every batch size the scheduling applies to -- cus + cus / 8 < B <= 4 cus -- with the snake dealing of the register tile
(cus > 0) and with 0, 2, 36 and 56 reducer workgroups in front of the grid (a lazy launch: the workgroups on the reducers' CUs
take the last positions), on random list lengths:
  * every rank lies below its group's size (a rank past it selects NO query: the workgroup would take an index no lane wrote --
    what B = 385 .. 447 and 449 .. 511 did on 256 CUs while a round was dealt backwards whenever `base + per <= 8`);
  * the B blocks select every query exactly once."""
import ctypes

import numpy as np
import pytest

L = 128


def _hook():
    from pytorchltr_amd import _C
    return _C.lib().ltr_debug_sched_slots


def _order(B, G, n):
    """order[g, r] = the query that member rank r of group g selects (-1 past the group's size), size[g]."""
    k = np.arange(64)
    ids = ((k[None, :] >> 3) * G + np.arange(G)[:, None]) * 8 + (k[None, :] & 7)          # (G, 64): member k of group g
    valid = ids < B
    key = np.where(valid, np.clip(n[np.minimum(ids, B - 1)], 0, L) >> 3, -1)
    perm = np.argsort(-key, axis=1, kind="stable")                                        # descending n, ties by member order
    order = np.take_along_axis(np.where(valid, ids, -1), perm, axis=1)
    return order, valid.sum(axis=1)


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_every_block_takes_a_query_of_its_own(cus):
    hook = _hook()
    rng = np.random.default_rng(cus)
    for B in range(cus + cus // 8 + 1, 4 * cus + 1):
        G = (B + 63) // 64
        n = rng.integers(1, L + 1, size=B)
        order, size = _order(B, G, n)
        group = np.empty(B, dtype=np.int32)
        rank = np.empty(B, dtype=np.int32)
        for nred in (0, 2, 36, 56):
            assert hook(B, G, cus, nred, group.ctypes.data_as(ctypes.c_void_p), rank.ctypes.data_as(ctypes.c_void_p)) == 0
            assert group.min() >= 0 and group.max() < G and rank.min() >= 0, (B, nred)
            assert np.all(rank < size[group]), (B, nred, int(np.argmax(rank >= size[group])))
            q = order[group, rank]
            assert np.array_equal(np.sort(q), np.arange(B)), (B, nred)


def test_quiet_blocks_take_the_shortest_lists_in_id_order():
    """C2's lazy launch (B = 1024 on 256 CUs, 36 reducers): the 144 workgroups whose id mod 256 < 36 take the last 144 positions
    of the order -- ranks 48 and up of their groups --, everybody else the 880 in front, and both keep their id order."""
    B, cus, nred = 1024, 256, 36
    G = B // 64
    group = np.empty(B, dtype=np.int32)
    rank = np.empty(B, dtype=np.int32)
    assert _hook()(B, G, cus, nred, group.ctypes.data_as(ctypes.c_void_p), rank.ctypes.data_as(ctypes.c_void_p)) == 0
    ids = nred + np.arange(B)
    quiet = (ids >= cus) & (ids % cus < nred)
    assert quiet.sum() == 144
    assert rank[quiet].min() >= (B - 144) // (8 * G) * 8 and rank[~quiet].max() < 56
    # without reducers the same grid is the plain snake order
    plain_g = np.empty(B, dtype=np.int32)
    plain_r = np.empty(B, dtype=np.int32)
    assert _hook()(B, G, cus, 0, plain_g.ctypes.data_as(ctypes.c_void_p), plain_r.ctypes.data_as(ctypes.c_void_p)) == 0
    assert np.array_equal(group[~quiet], plain_g[:B - 144]) and np.array_equal(rank[~quiet], plain_r[:B - 144])
    assert np.array_equal(group[quiet], plain_g[B - 144:]) and np.array_equal(rank[quiet], plain_r[B - 144:])
