"""The fp64 reference of LambdaRankLoss (include/ltr_lambdarank.h) for long lists: the specification of
tests/lambdarank_ref.py, evaluated in rank order in blocks of owner rows against only the partners that can have
weight -- the anchors (ranks below the cutoff K) for an owner at a rank >= K, every rank for an anchor.  Memory is
O(block n); with a cutoff the time is O(K n).  The same ranking rule: np.lexsort on the fp32 scores, ties by index.
tests/test_lambdarank_long_host.py checks it against lambdarank_ref.batch; the GPU tests take it as their oracle."""
import numpy as np

from tests.lambdarank_ref import LN2, cutoff, gains, max_dcg

BLOCK = 256


def _block(so, yo, Go, do, sp, yp, Gp, dp, sigma):
    """(loss, gradient of the owners in units of sigma / ln 2) of the owner rows against the partner columns: the loss
    of a pair is counted on its winner's row (y_owner > y_partner)."""
    x = sigma * (so[:, None] - sp[None, :])
    w = np.abs(Go[:, None] - Gp[None, :]) * np.abs(do[:, None] - dp[None, :])
    gt = yo[:, None] > yp[None, :]
    lt = yo[:, None] < yp[None, :]
    spn = np.maximum(-x, 0.0) + np.log1p(np.exp(-np.abs(x)))           # softplus(-x), stable
    loss = float(np.sum(np.where(gt, w * spn, 0.0)))
    # the owner wins: -w sigmoid(-x); the owner loses: +w sigmoid(x) (sigmoid(-x) = exp(-softplus(x)))
    g = np.where(gt, -w * np.exp(-(spn + x)), 0.0) + np.where(lt, w * np.exp(-spn), 0.0)
    return loss, g.sum(axis=1)


def row(s, y, k=None, sigma=1.0, block=BLOCK):
    """(loss, dscores) of one query's real documents."""
    s32 = np.asarray(s, dtype=np.float32)
    nb = s32.size
    if nb <= 1:
        return 0.0, np.zeros(nb)
    K = cutoff(k, nb)
    order = np.lexsort((np.arange(nb), -s32.astype(np.float64)))        # the document at each rank
    sr = np.asarray(s, dtype=np.float64)[order]
    yr = np.asarray(y, dtype=np.float32).astype(np.float64)[order]
    Gr = gains(y)[order] / max_dcg(y, K)
    ranks = np.arange(nb)
    dr = np.where(ranks < K, 1.0 / np.log2(2.0 + ranks.astype(np.float64)), 0.0)
    loss = 0.0
    g = np.zeros(nb)
    for o0 in range(0, nb, block):
        o1 = min(o0 + block, nb)
        # the anchors of the block against every rank, its ranks from K on against the anchors
        for lo, hi, pn in ((o0, min(o1, K), nb), (max(o0, K), o1, K)):
            if lo >= hi:
                continue
            l, gg = _block(sr[lo:hi], yr[lo:hi], Gr[lo:hi], dr[lo:hi], sr[:pn], yr[:pn], Gr[:pn], dr[:pn], sigma)
            loss += l
            g[lo:hi] = gg
    out = np.zeros(nb)
    out[order] = g * (sigma / LN2)
    return loss / LN2, out


def batch(scores, rel, n, k=None, sigma=1.0, block=BLOCK):
    """(loss (B), dscores (B, L)) of a padded batch: n clamped to [0, L], zeros on the padded documents."""
    scores = np.asarray(scores)
    rel = np.asarray(rel)
    B, L = scores.shape
    loss = np.zeros(B)
    ds = np.zeros((B, L))
    for b in range(B):
        nb = int(min(max(int(n[b]), 0), L))
        loss[b], ds[b, :nb] = row(scores[b, :nb], rel[b, :nb], k, sigma, block)
    return loss, ds
