"""Degenerate queries for the parity tests: the lists a real collection holds and `conftest.synth` never draws.

`synth` gives every query labels randint(0, 5) and a random length: beyond a dozen documents every grade is present
and there are many `y_i > y_j` pairs.  `degenerate_batch` cycles the queries of a batch through the opposite cases
(FLAVOURS below): no relevant document, one relevant document, all labels equal, empty / one / two document lists,
padded labels that must not count, a grade above 4, a negative grade -- next to one `control` query of the usual kind.

Scores are EXACT, so fp32 and fp64 rank alike and no row of a rank-dependent loss needs a tie explanation:
W = e_0 and b = 0.25, so a score is X[b, i, 0] + 0.25, and X[:, :, 0] is a per-query permutation of a grid of
multiples of 1/64 spanning about +-2 (lists beyond 320 documents take the power of two that keeps the span: 4 / L
rounded down, still exact in fp32).  The other feature columns are N(0, 1): 0 * x adds nothing to a score, and they
carry the weight gradient.  `scores="constant"` sets column 0 to 0.5: every score is tied and the index tie rule
(the suite's autouse fixture selects it) decides every rank.

A plain module: tests import it, the golden generator imports it, nothing else does.
"""
import numpy as np
import torch

FLAVOURS = ("zero", "equal3", "one_rel_last", "n0", "n1", "n2_equal", "n2_pair", "zero_real_pad_nonzero",
            "binary", "grade7", "negative", "control")
# (flavours whose list length is part of the case; the others draw n and every fifth query is full)
_FIXED_N = ("n0", "n1", "n2_equal", "n2_pair", "zero_real_pad_nonzero")
# no `y_i > y_j` pair among the real documents: loss 0 and gradient 0 -- see zero_rows() for the two exceptions
ZERO_LOSS = ("zero", "n0", "n1", "n2_equal", "zero_real_pad_nonzero")
DCG_HINGE_ZERO = -1.0 / np.log(2.0)       # PairwiseDCGHingeLoss of a query without an active pair: -1 / ln(2 + 0)
# no real document with a label above 0: MAP, MRR, P, recall and ERR are exactly 0
NO_RELEVANT = ("zero", "n0", "zero_real_pad_nonzero")
BIAS = 0.25


def grid_step(L):
    """Spacing of the score grid: a multiple of 1/64 up to 320 documents, the power of two below 4 / L beyond."""
    if L <= 320:
        return max(1, 256 // max(L, 1)) / 64.0
    return 2.0 ** -int(np.ceil(np.log2(L / 4.0)))


def flavour_of(q):
    return FLAVOURS[q % len(FLAVOURS)]


def degenerate_batch(B, L, F, seed, scores="grid", label_dtype=torch.int64):
    """-> X (B, L, F) f32, W (F) f32, b (1) f32, y (B, L) label_dtype, n (B) int64, flavours (list of B names).
    The labels have the same VALUES whatever the dtype.  L >= 3."""
    assert L >= 3 and F >= 1 and scores in ("grid", "constant")
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(B, L, F, generator=g)
    W = torch.zeros(F)
    W[0] = 1.0
    b = torch.full((1,), BIAS)
    if scores == "grid":
        grid = (torch.arange(L, dtype=torch.float64) - L // 2) * grid_step(L)
        for q in range(B):
            X[q, :, 0] = grid[torch.randperm(L, generator=g)].float()
    else:
        X[:, :, 0] = 0.5
    y = torch.randint(0, 5, (B, L), generator=g)              # the padded labels stay as drawn: garbage a kernel must mask
    n = torch.randint(3, L + 1, (B,), generator=g)
    where = torch.randint(0, 1 << 30, (B,), generator=g)      # position of the one special label, modulo n
    flavours = [flavour_of(q) for q in range(B)]
    for q, fl in enumerate(flavours):
        if fl not in _FIXED_N and q % 5 == 0:
            n[q] = L
        if fl == "zero":
            y[q] = 0
        elif fl == "equal3":
            y[q] = 3
        elif fl == "one_rel_last":
            y[q] = 0
            y[q, int(n[q]) - 1] = 4
        elif fl == "n0":
            n[q] = 0
        elif fl == "n1":
            n[q] = 1
        elif fl == "n2_equal":
            n[q] = 2
            y[q, :2] = 2
        elif fl == "n2_pair":
            n[q] = 2
            y[q, 0], y[q, 1] = 0, 1
        elif fl == "zero_real_pad_nonzero":
            n[q] = max(3, L // 2)
            y[q, :int(n[q])] = 0
            y[q, int(n[q]):] = 4
        elif fl == "binary":
            y[q] = y[q] % 2
        elif fl == "grade7":
            y[q, int(where[q]) % int(n[q])] = 7
        elif fl == "negative":
            y[q, int(where[q]) % int(n[q])] = -1
    return X, W, b, y.to(label_dtype), n, flavours


def exact_scores(X):
    """The scores of the batch in fp64: X[:, :, 0] + 0.25, exact in fp32 too."""
    return X[:, :, 0].double().numpy() + BIAS


def zero_rows(kind, y, n):
    """Rows whose loss AND gradient are exactly 0 in exact arithmetic, read off the labels (not the flavour names, so the
    control and binary rows that happen to qualify are held to it too):
      hinge, dcg_hinge, logistic, arp2, ndcg2 sum over the pairs with y_i > y_j: rows whose real labels are all equal
        (ZERO_LOSS and equal3).  dcg_hinge's gradient is 0 there and its loss the constant DCG_HINGE_ZERO;
      arp1, ndcg1 sum y_i (or the gain of y_i) times a pair term over ALL pairs, the diagonal included: rows whose real
        labels are all 0 -- n2_equal (labels 2, 2) and an n1 row with a non-zero label are not among them."""
    y = np.asarray(y, dtype=np.float64)
    L = y.shape[1]
    real = np.arange(L)[None, :] < np.clip(np.asarray(n), 0, L)[:, None]
    if kind in ("arp1", "ndcg1"):
        ok = np.where(real, y, 0.0) == 0.0
        return np.nonzero(ok.all(axis=1))[0]
    hi = np.where(real, y, -np.inf).max(axis=1)
    lo = np.where(real, y, np.inf).min(axis=1)
    return np.nonzero(~real.any(axis=1) | (hi == lo))[0]


def rows_of(flavours, names):
    return np.array([i for i, f in enumerate(flavours) if f in names], dtype=np.int64)
