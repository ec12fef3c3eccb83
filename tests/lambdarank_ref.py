"""The fp64 reference of LambdaRankLoss (include/ltr_lambdarank.h): numpy, an O(L^2) mask formulation of the
specification, one query at a time.  Ranking: np.lexsort((index, -score)) on the fp32 scores -- descending, equal scores
by document index.  Shared by tests/test_lambdarank_host.py (which checks the reference itself) and the GPU tests."""
import numpy as np

LN2 = np.log(2.0)


def cutoff(k, nb):
    return nb if k is None or k <= 0 else min(int(k), nb)


def ranks_by_score(s):
    """0-based rank of every document of the fp32 scores s, descending, ties by index."""
    s = np.asarray(s, dtype=np.float32)
    order = np.lexsort((np.arange(s.size), -s.astype(np.float64)))
    r = np.empty(s.size, dtype=np.int64)
    r[order] = np.arange(s.size)
    return r


def discounts(ranks, K):
    return np.where(ranks < K, 1.0 / np.log2(2.0 + ranks.astype(np.float64)), 0.0)


def gains(y):
    return np.exp2(np.asarray(y, dtype=np.float32).astype(np.float64)) - 1.0


def max_dcg(y, K):
    g = np.sort(gains(y))[::-1][:K]
    m = float(np.sum(g / np.log2(2.0 + np.arange(g.size))))
    return m if m != 0.0 else 1.0


def pair_weights(s, y, k):
    """(w, mask): w_ij = |G_i - G_j| |d(r_i) - d(r_j)| and mask_ij = y_i > y_j of one query's real documents."""
    nb = len(s)
    K = cutoff(k, nb)
    y32 = np.asarray(y, dtype=np.float32).astype(np.float64)
    G = gains(y) / max_dcg(y, K)
    d = discounts(ranks_by_score(s), K)
    w = np.abs(G[:, None] - G[None, :]) * np.abs(d[:, None] - d[None, :])
    return w, y32[:, None] > y32[None, :]


def softplus(x):
    """log(1 + exp(x)), stable."""
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def row(s, y, k=None, sigma=1.0, frozen=None):
    """(loss, dscores) of one query's real documents.  `frozen`: (w, mask) taken elsewhere (finite differences keep the
    ranking and the weights constant)."""
    s32 = np.asarray(s, dtype=np.float32)
    nb = s32.size
    if nb <= 1:
        return 0.0, np.zeros(nb)
    w, mask = pair_weights(s32, y, k) if frozen is None else frozen
    sd = np.asarray(s, dtype=np.float64)
    diff = sigma * (sd[:, None] - sd[None, :])
    wm = np.where(mask, w, 0.0)
    sp = softplus(-diff)
    loss = float(np.sum(wm * sp) / LN2)
    sig = np.exp(-(sp + diff))                                          # sigmoid(-diff) = exp(-softplus(diff)), stable
    lam = sigma * wm / LN2 * sig
    return loss, -lam.sum(axis=1) + lam.sum(axis=0)


def batch(scores, rel, n, k=None, sigma=1.0):
    """(loss (B), dscores (B, L)) of a padded batch: n clamped to [0, L], zeros on the padded documents."""
    scores = np.asarray(scores)
    rel = np.asarray(rel)
    B, L = scores.shape
    loss = np.zeros(B)
    ds = np.zeros((B, L))
    for b in range(B):
        nb = int(min(max(int(n[b]), 0), L))
        loss[b], ds[b, :nb] = row(scores[b, :nb], rel[b, :nb], k, sigma)
    return loss, ds
