"""CPU tier: oracle/long_pairs_ref.py -- the fp64 references that tests/test_gpu_long_pairs_max.py uses at 65 536
documents -- pinned to oracle_pairwise_loss (oracle/ltr_oracle.c, every pair, O(L^2)) at lengths that file can afford.

Scores are fp32 values on the grid k / 4096: every hinge margin and every sum of margins below 2^40 is exact in fp64,
whatever the order of summation, so the hinge kinds are compared with ==.  A seventh of them is rounded to integers
(ties: the index tie order decides LambdaNDCG ranks, and margins of exactly 0 are on the gate).  The log-based kinds are
held to 1e-12 of the loss and 1e-12 of the row's largest gradient entry: both sides are fp64 sums of at most 9e6
positive terms in different orders (measured: <= 1e-13)."""
import functools

import numpy as np
import pytest

from oracle import long_pairs_ref as R
from oracle import ltr_oracle as O

KINDS = list(R.KINDS)
SIGMOID = [k for k in KINDS if k not in R.HINGE]


def _scores(rng, B, L):
    s = np.round(rng.normal(0.0, 2.0, (B, L)) * 4096.0) / 4096.0
    ties = rng.random((B, L)) < 1.0 / 7.0
    return np.where(ties, np.round(s), s).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(scores fp32, labels, n) of a named shape, read-only."""
    rng = np.random.default_rng({"sparse": 11, "sparse_half": 12, "dense": 13, "dense_half": 14, "short": 15}[name])
    if name.startswith("sparse"):
        B, L, rel = 4, 3000, 40
        n = np.array([2983, 1025, 1, 0], dtype=np.int64)
        y = np.zeros((B, L), dtype=np.float32 if name == "sparse_half" else np.int64)
        for b in range(B):
            where = rng.choice(L, rel, replace=False)              # some past n[b]: they must not count
            y[b, where] = rng.integers(1, 9, rel) / 2.0 if name == "sparse_half" else rng.integers(1, 5, rel)
        y[0, 0], y[0, n[0] - 1], y[2, 0] = 3, 2, 1
    elif name.startswith("dense"):
        B, L = 3, 1500
        n = np.array([1500, 733, 2], dtype=np.int64)
        y = (rng.integers(0, 9, (B, L)) / 2.0).astype(np.float32) if name == "dense_half" else rng.integers(0, 5, (B, L))
    else:                                                          # n = 0, 1 and more than L
        B, L = 3, 70
        n = np.array([0, 1, 99], dtype=np.int64)
        y = rng.integers(0, 5, (B, L))
    out = (_scores(rng, B, L), y, n)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _oracle(kind, name, sigma):
    s, y, n = _case(name)
    return O.pairwise_loss(kind, s, y, n, sigma=sigma)


def _same(kind, got, want, scale, what):
    if kind in R.HINGE:
        assert np.array_equal(got, want), what
    else:
        err = np.max(np.abs(got - want) / scale) if np.size(got) else 0.0
        print("%s: %.3e" % (what, err))
        assert err <= 1e-12, what


def _sigmas(kind):
    return (1.0,) if kind in R.HINGE else (1.0, 2.0)


@pytest.mark.parametrize("name", ["sparse", "sparse_half", "short"])
@pytest.mark.parametrize("kind", KINDS)
def test_sparse_reference_vs_oracle(kind, name):
    s, y, n = _case(name)
    if name == "short":                                            # dense labels: only the rows with n <= 1 qualify
        s, y, n = s[:2], y[:2], n[:2]
    for sigma in _sigmas(kind):
        want_l, want_g = _oracle(kind, name, sigma)
        want_l, want_g = want_l[:len(n)], want_g[:len(n)]
        loss, grad = R.sparse_pairwise(kind, s, y, n, sigma=sigma)
        what = "%s %s sigma=%g" % (kind, name, sigma)
        _same(kind, loss, want_l, np.maximum(np.abs(want_l), 1e-300), what + " loss")
        _same(kind, grad, want_g, np.maximum(np.max(np.abs(want_g), axis=1, keepdims=True), 1e-300), what + " gradient")
        for b in range(len(n)):
            assert np.all(grad[b, min(int(n[b]), s.shape[1]):] == 0.0), what


def test_sparse_reference_refuses_negative_labels():
    s, y, n = _case("short")
    with pytest.raises(ValueError, match=">= 0"):
        R.sparse_pairwise("hinge", s, y - 1, n)


@pytest.mark.parametrize("name", ["dense", "dense_half", "sparse", "short"])
@pytest.mark.parametrize("kind", KINDS)
def test_sampled_gradient_vs_oracle(kind, name):
    s, y, n = _case(name)
    L = s.shape[1]
    rng = np.random.default_rng(5)
    docs = []
    for b in range(len(n)):
        nb = min(int(n[b]), L)
        some = rng.choice(nb, min(nb, 24), replace=False) if nb else np.zeros(0, dtype=np.int64)
        docs.append(np.unique(np.concatenate((some, [0, nb - 1] if nb else []))).astype(np.int64))
    for sigma in _sigmas(kind):
        _, want_g = _oracle(kind, name, sigma)
        got = R.sampled_gradient(kind, s, y, n, docs, sigma=sigma)
        for b in range(len(n)):
            _same(kind, got[b], want_g[b, docs[b]], max(np.max(np.abs(want_g[b])), 1e-300),
                  "%s %s sigma=%g row %d sampled gradient" % (kind, name, sigma, b))


@pytest.mark.parametrize("name", ["dense", "dense_half", "sparse", "short"])
def test_hinge_total_vs_oracle(name):
    s, y, n = _case(name)
    H = R.hinge_total(s, y, n)
    assert np.array_equal(H, _oracle("hinge", name, 1.0)[0])
    assert np.array_equal([R.dcg_hinge_modifier(h)[0] for h in H], _oracle("dcg_hinge", name, 1.0)[0])


def test_hinge_total_with_negative_grades():
    """The gate and the pair sum depend on the order of the grades only: shifted labels give the same total."""
    s, y, n = _case("dense")
    assert np.array_equal(R.hinge_total(s, y - 2, n), _oracle("hinge", "dense", 1.0)[0])
    docs = [np.arange(0, min(int(v), s.shape[1]), 97) for v in n]
    got = R.sampled_gradient("hinge", s, y - 2, n, docs)
    for b in range(len(n)):
        assert np.array_equal(got[b], _oracle("hinge", "dense", 1.0)[1][b, docs[b]])
