"""GPU tier: the long-list pairwise losses (include/ltr_longpair.h, ``long_lists=True``) at ltr_max_pair_list_len() = M
documents and at M - 1, where tests/test_gpu_long_pairs.py stops at 6000: 64 owner tiles and 64 chunks per query, ranks
and gradient counts up to M - 1, the key sort over 16 sort chunks, tiles that exit at once next to full rows.

The references are oracle/long_pairs_ref.py (fp64, no pair loop; tests/test_long_pairs_ref_host.py pins them to the C
oracle):
  * sparse family -- R = 96 documents with a label above 0: loss and the WHOLE gradient of all seven kinds;
  * dense family  -- labels 0..4 on every document: the gradient at ~200 sampled documents of all seven kinds, the hinge
    and DCG-hinge losses.  The dense losses of the five other kinds at M stay UNVERIFIED: no exact reference cheaper
    than O(L^2) is known.
Tolerances are the project's (tests/test_gpu_long_pairs.py), imported; the hinge gradient is compared with ==.

What a wrong kernel would trip (B = 4 rows, n = L, 16 OWN + 1, 3 CH + 5, 0):
  * the last chunk skipped: row 0 loses every pair with a streamed document past 63 CH, >= 1/64 of its terms (loss), and
    the document at n - 1 carries a label in the sparse family, so every other hinge count is off by one or more (==);
  * only the first 63 tile partials added: tile 63 owns the labelled documents 63 OWN and n - 1, at least 2 / 96 of the
    sparse loss; the dense hinge loss drops by 1/64;
  * an idle owner's label 0 instead of NaN: invisible while every label is >= 0 (0 beats nothing), so
    test_negative_grades runs grades -2..2: each of the 1023 idle owners of row 1's last tile would add the loss of a
    document with grade 0 and score 0 against ~6500 lower grades, ~10 % of that row's hinge loss;
  * ranks off by one from 2^15 on: the documents at ranks 2^15 - 1 and 2^15 carry the labels 4 and 1 (sparse) and are in
    the sample (dense); their distance would become 2, delta_2 / delta_1 = 0.53 on the heaviest pair of both entries.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import long_pairs_ref as R
from tests.test_gpu_long_pairs import (DEV, KINDS, _check_grad_vs_oracle, _check_loss_vs_oracle, _check_vs_oracle,
                                       _run_long)

pytestmark = pytest.mark.gpu
B = 4
RELEVANT = 96
SAMPLE = 200


def _geometry():
    from pytorchltr_amd import _C
    own, ch = _C.long_pair_geometry()
    return own, ch, _C.max_pair_list_len()


def _length(which):
    M = _geometry()[2]
    return {"max": M, "max-1": M - 1}[which]


def _readonly(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _scores_and_n(L):
    """N(0, 2^2) scores in fp32 and n = (L, 16 OWN + 1, 3 CH + 5, 0); one row on half-integers (heavy ties: the index tie
    order decides the LambdaNDCG ranks, and margins of exactly 0 sit on the hinge gate): the full row at M - 1, the
    17-tile row at M."""
    own, ch, M = _geometry()
    rng = np.random.default_rng(1000 + L)
    s = rng.normal(0.0, 2.0, (B, L)).astype(np.float32)
    tied = 1 if L == M else 0
    s[tied] = np.round(s[tied] * 2.0) / 2.0
    n = np.array([L, 16 * own + 1, 3 * ch + 5, 0], dtype=np.int64)
    assert n[1] < L and 4096 > n[2] > 0
    return _readonly(s, n)


def _rank_neighbours(s, nb):
    """The documents at ranks 2^15 - 1 and 2^15 (score descending, ties by index), if the row has them."""
    if nb <= 1 << 15:
        return []
    order = np.lexsort((np.arange(nb), -s[:nb].astype(np.float64)))
    return [int(order[(1 << 15) - 1]), int(order[1 << 15])]


@functools.lru_cache(maxsize=None)
def _sparse_batch(L, labels):
    """RELEVANT labelled documents per row at random positions, among them 0, n - 1, both sides of the last tile
    boundary below n, and the two documents around rank 2^15 (labels 4 and 1).  labels: "i64" 1..4, "f32" half-grades."""
    own = _geometry()[0]
    s, n = _scores_and_n(L)
    rng = np.random.default_rng(2000 + L)
    y = np.zeros((B, L), dtype=np.float32 if labels == "f32" else np.int64)
    for b in range(B):
        nb = int(n[b])
        if nb == 0:
            continue
        edge = (nb - 1) // own * own
        around = _rank_neighbours(s[b], nb)
        forced = {0, nb - 1, edge - 1, edge} | set(around)
        rest = [k for k in rng.permutation(nb) if k not in forced][:RELEVANT - len(forced)]
        where = np.array(sorted(forced) + rest)
        y[b, where] = rng.integers(1, 9, where.size) / 2.0 if labels == "f32" else rng.integers(1, 5, where.size)
        if around:
            y[b, around[0]], y[b, around[1]] = 4, 1
        assert np.count_nonzero(y[b]) == RELEVANT
    return _readonly(s, y, n)


@functools.lru_cache(maxsize=None)
def _sparse_reference(kind, L, labels):
    return _readonly(*R.sparse_pairwise(kind, *_sparse_batch(L, labels)))


@functools.lru_cache(maxsize=None)
def _dense_batch(L, lowest):
    """Labels uniform over lowest .. lowest + 4 on every document."""
    s, n = _scores_and_n(L)
    y = np.random.default_rng(3000 + L).integers(lowest, lowest + 5, (B, L))
    return _readonly(s, y, n)


@functools.lru_cache(maxsize=None)
def _sample(L):
    """Per row SAMPLE documents below n[b]: the first and last of every owner tile, n - 1, the two around rank 2^15 and
    a seeded random rest (the row with n = 0 has none)."""
    own = _geometry()[0]
    s, n = _scores_and_n(L)
    rng = np.random.default_rng(4000 + L)
    docs = []
    for b in range(B):
        nb = int(n[b])
        fixed = {k for t in range(0, nb, own) for k in (t, min(t + own, nb) - 1)} | set(_rank_neighbours(s[b], nb))
        rest = [k for k in rng.permutation(nb)[:SAMPLE] if k not in fixed][:max(SAMPLE - len(fixed), 0)]
        docs.append(np.array(sorted(fixed) + rest, dtype=np.int64))
    return docs


@functools.lru_cache(maxsize=None)
def _dense_reference(kind, L, lowest):
    s, y, n = _dense_batch(L, lowest)
    return R.sampled_gradient(kind, s, y, n, _sample(L))


@functools.lru_cache(maxsize=None)
def _dense_hinge_total(L, lowest):
    return _readonly(R.hinge_total(*_dense_batch(L, lowest)))[0]


def _check_sparse(kind, loss, ds, L, labels, what):
    s, y, n = _sparse_batch(L, labels)
    want_l, want_g = _sparse_reference(kind, L, labels)
    _check_vs_oracle(kind, loss, ds, want_l, want_g, n, what)          # with exact zeros past n[b]
    if kind == "hinge":                                                # integer counts below 2^24 behind an exact gate
        assert np.array_equal(ds.astype(np.float64), want_g), what
    if kind == "dcg_hinge":
        _check_dcg_hinge_counts(ds, _sparse_reference("hinge", L, labels), what)


def _check_dcg_hinge_counts(ds, hinge, what, docs=None):
    """The DCG-hinge gradient is the hinge count times f(H) = 1 / ((2 + H) ln^2(2 + H)), ~1e-12 at M: far below the
    absolute term of the project's gradient tolerance, which therefore says nothing about it.  Divided by the fp64
    factor it must give the counts back within the relative error of the kernel's factor, which is that of its fp32 H
    (held to 5e-4 by the loss check) times |d ln f / d ln H| = 1 + 2 / ln(2 + H) < 2 for H > 6: 1e-3 of each count."""
    H, counts = hinge
    for b in range(B):
        if H[b] <= 6.0:
            continue
        cols = slice(None) if docs is None else docs[b]
        got = ds[b, cols].astype(np.float64) / R.dcg_hinge_modifier(H[b])[1]
        want = counts[b, cols] if docs is None else counts[b]
        assert np.all(np.abs(got - want) <= 1e-3 * np.abs(want)), "%s row %d" % (what, b)


SPARSE_CASES = [("max", "i64"), ("max-1", "i64"), ("max", "f32")]


@pytest.mark.parametrize("which,labels", SPARSE_CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_sparse_labels_vs_reference(kind, which, labels):
    L = _length(which)
    s, y, n = _sparse_batch(L, labels)
    loss, ds = _run_long(kind, s, y, n)
    _check_sparse(kind, loss, ds, L, labels, "%s sparse %s labels %dx%d" % (kind, labels, B, L))


@pytest.mark.parametrize("which", ["max", "max-1"])
@pytest.mark.parametrize("kind", KINDS)
def test_dense_labels_vs_reference(kind, which):
    L = _length(which)
    _dense_case(kind, L, 0)


@pytest.mark.parametrize("kind", ["hinge", "dcg_hinge", "logistic", "arp2"])
def test_negative_grades(kind):
    """Grades -2..2 at M - 1: an idle owner (rows 0 and 1 have 1 and OWN - 1 of them in their last tile) must lose to
    nothing and beat nothing, whatever the sign of the labels around it."""
    _dense_case(kind, _length("max-1"), -2)


def _dense_case(kind, L, lowest):
    s, y, n = _dense_batch(L, lowest)
    docs = _sample(L)
    loss, ds = _run_long(kind, s, y, n)
    what = "%s dense labels from %d %dx%d" % (kind, lowest, B, L)
    assert np.all(np.isfinite(loss)), what
    want = _dense_reference(kind, L, lowest)
    for b in range(B):
        assert np.all(ds[b, int(n[b]):] == 0.0), what
        if len(docs[b]) == 0:
            continue
        got = ds[b, docs[b]]
        _check_grad_vs_oracle(got[None, :], want[b][None, :], "%s row %d, %d sampled" % (what, b, len(docs[b])))
        if kind == "hinge":
            assert np.array_equal(got.astype(np.float64), want[b]), what
    if kind in R.HINGE:
        H = _dense_hinge_total(L, lowest)
        want_l = H if kind == "hinge" else np.array([R.dcg_hinge_modifier(h)[0] for h in H])
        _check_loss_vs_oracle(kind, loss, want_l, what)
    if kind == "dcg_hinge":
        _check_dcg_hinge_counts(ds, (_dense_hinge_total(L, lowest), _dense_reference("hinge", L, lowest)), what, docs)


def test_module_at_the_maximum_length():
    from pytorchltr_amd.loss import LambdaNDCGLoss2
    L = _length("max")
    s, y, n = _sparse_batch(L, "i64")
    sd = torch.as_tensor(s).to(DEV).unsqueeze(-1).requires_grad_(True)          # (B, L, 1), as a scorer returns them
    loss = LambdaNDCGLoss2(long_lists=True)(sd, torch.as_tensor(y).to(DEV), torch.as_tensor(n).to(DEV))
    assert loss.shape == (B,)
    loss.mean().backward()
    got_g = sd.grad.reshape(B, L).cpu().numpy() * B
    _check_sparse("ndcg2", loss.detach().cpu().numpy(), got_g, L, "i64", "LambdaNDCGLoss2 %dx%d" % (B, L))


@pytest.mark.parametrize("kind", ["dcg_hinge", "ndcg2"])
def test_run_to_run_at_the_maximum_length(kind):
    s, y, n = _sparse_batch(_length("max"), "i64")
    first = _run_long(kind, s, y, n)
    again = _run_long(kind, s, y, n)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
