"""fp64 references of the seven pairwise losses that stay affordable at 65 536 documents.

TEST INFRASTRUCTURE ONLY -- plain numpy, not part of the product.  ``oracle/ltr_oracle.c`` evaluates every pair and is
O(L^2) per query: minutes at ltr_max_pair_list_len().  The three references here need no pair loop over the whole list:

  (a) sparse_pairwise    loss and the whole gradient when only R documents carry a label above 0, O(R n) per query;
  (b) sampled_gradient   the gradient entries of S chosen documents under any labels, O(S n) per query;
  (c) hinge_total        the hinge pair sum under any labels, O(G^2 n log n) for G distinct grades.

Ranks (score descending, ties in document-index order), maxDCG, the gains, LambdaNDCG2's delta and the DCG-hinge
modifier are written as in ltr_oracle.c; tests/test_long_pairs_ref_host.py pins all three to oracle_pairwise_loss.
Scores are expected to be fp32-valued (differences and the hinge gate are then exact in fp64, as in the C file).
"""
import math
from types import SimpleNamespace

import numpy as np

KINDS = ("hinge", "dcg_hinge", "logistic", "arp1", "arp2", "ndcg1", "ndcg2")
HINGE = ("hinge", "dcg_hinge")
ORIENTED = ("hinge", "dcg_hinge", "logistic", "arp2", "ndcg2")      # only pairs with y_i > y_j count
LN2 = math.log(2.0)


def _clamp_n(n, L):
    return min(max(int(n), 0), L)


def _batch(scores, relevance, n):
    s = np.asarray(scores, dtype=np.float64)
    y = np.asarray(relevance, dtype=np.float64)
    s, y = s.reshape(s.shape[0], s.shape[1]), y.reshape(y.shape[0], y.shape[1])
    return s, y, [_clamp_n(v, s.shape[1]) for v in np.asarray(n).reshape(-1)]


def _row(kind, s, y, nb):
    """One query cut to its real documents; for the LambdaNDCG kinds with rank and gain per document."""
    q = SimpleNamespace(s=s[:nb], y=y[:nb], n=nb)
    if kind in ("ndcg1", "ndcg2"):
        order = np.lexsort((np.arange(nb), -q.s))                  # rank_row: score descending, then index
        q.rank = np.empty(nb, dtype=np.float64)
        q.rank[order] = np.arange(nb)
        ideal = np.sort(q.y)[::-1]                                 # max_dcg_row
        maxdcg = float(np.sum((np.power(2.0, ideal) - 1.0) / np.log2(2.0 + np.arange(nb))))
        q.G = (np.power(2.0, q.y) - 1.0) / (maxdcg if maxdcg != 0.0 else 1.0)
    return q


def _weight(kind, q, i, j):
    """w of pair (i, j) in lambda_row; one of i, j may be an index array."""
    if kind == "logistic":
        return 1.0
    if kind == "arp1":
        return q.y[i]
    if kind == "arp2":
        return q.y[i] - q.y[j]
    if kind == "ndcg1":
        return q.G[i] / np.log2(2.0 + q.rank[i])
    k = np.abs(q.rank[i] - q.rank[j])
    return np.abs(1.0 / np.log2(2.0 + k) - 1.0 / np.log2(3.0 + k)) * np.abs(q.G[i] - q.G[j])


def _softplus2(x):
    """log2(1 + e^x)"""
    return np.logaddexp(0.0, x) / LN2


def _sigmoid(x):
    return np.exp(-np.logaddexp(0.0, -x))


def dcg_hinge_modifier(total):
    """(-1 / ln(2 + H), d/dH of it): the loss modifier of PairwiseDCGHingeLoss."""
    lg = math.log(2.0 + total)
    return -1.0 / lg, 1.0 / ((2.0 + total) * lg * lg)


def sparse_pairwise(kind, scores, relevance, n, sigma=1.0):
    """(loss[B], dscores[B, L]) when every label is >= 0 and few are above it.

    Every term of every kind has a document with a label above 0 at its `i` end: the oriented kinds need y_i > y_j >= 0,
    and the row weight of ARP1 (y_i) and LambdaNDCG1 (G_i / D(rank_i)) is 0 on a label of 0.  So a loop over those
    documents, each against all n[b] in one vector, visits every term once."""
    s, y, ns = _batch(scores, relevance, n)
    B, L = s.shape
    loss, grad = np.zeros(B), np.zeros((B, L))
    for b in range(B):
        q = _row(kind, s[b], y[b], ns[b])
        if np.any(q.y < 0.0):
            raise ValueError("sparse_pairwise needs labels >= 0")
        g, acc = grad[b, :q.n], 0.0
        everyone = np.arange(q.n)
        for i in np.flatnonzero(q.y > 0.0):
            d = q.s[i] - q.s
            wins = q.y[i] > q.y if kind in ORIENTED else np.ones(q.n, dtype=bool)
            if kind in HINGE:
                t = 1.0 - d
                act = wins & ~(t < 0.0)                            # at exactly the margin the gradient still flows
                acc += float(np.sum(t[act]))
                g[i] -= np.count_nonzero(act)
                g[act] += 1.0
            else:
                w = np.where(wins, _weight(kind, q, i, everyone), 0.0)
                acc += float(np.sum(w * _softplus2(-sigma * d)))
                dd = -w * sigma * _sigmoid(-sigma * d) / LN2       # d term / d (s_i - s_j)
                g[i] += float(np.sum(dd))
                g -= dd
        if kind == "dcg_hinge":
            acc, scale = dcg_hinge_modifier(acc)
            g *= scale
        loss[b] = acc
    return loss, grad


def hinge_total(scores, relevance, n):
    """H[b] = sum over y_i > y_j, s_i - s_j <= 1 of 1 - (s_i - s_j), per ordered pair of grades: the lower grade's scores
    sorted, the active ones of each s_i found by bisection (s_j >= s_i - 1), their sum from prefix sums."""
    s, y, ns = _batch(scores, relevance, n)
    out = np.zeros(s.shape[0])
    for b in range(s.shape[0]):
        sb, yb = s[b, :ns[b]], y[b, :ns[b]]
        grades = np.unique(yb)
        for lo in grades:
            sj = np.sort(sb[yb == lo])
            prefix = np.concatenate(([0.0], np.cumsum(sj)))
            for hi in grades[grades > lo]:
                si = sb[yb == hi]
                first = np.searchsorted(sj, si - 1.0, side="left")
                out[b] += float(np.sum((sj.size - first) * (1.0 - si) + (prefix[-1] - prefix[first])))
    return out


def sampled_gradient(kind, scores, relevance, n, docs, sigma=1.0):
    """d loss[b] / d scores[b, k] for k in docs[b] (indices below n[b]), any labels: one pass over the query per entry.
    Returns a list of B arrays.  DCG-hinge is the hinge entry times the modifier's factor at hinge_total."""
    s, y, ns = _batch(scores, relevance, n)
    base = "hinge" if kind == "dcg_hinge" else kind
    H = hinge_total(s, y, ns) if kind == "dcg_hinge" else None
    out = []
    for b in range(s.shape[0]):
        q = _row(base, s[b], y[b], ns[b])
        everyone = np.arange(q.n)
        got = np.zeros(len(docs[b]))
        for x, k in enumerate(docs[b]):
            k = int(k)
            assert 0 <= k < q.n
            d_k = q.s[k] - q.s                                     # k at the i end of (k, j)
            d_i = -d_k                                             # k at the j end of (i, k)
            all_pairs = np.ones(q.n, dtype=bool)
            wins = q.y[k] > q.y if base in ORIENTED else all_pairs
            loses = q.y > q.y[k] if base in ORIENTED else all_pairs
            if base == "hinge":
                got[x] = np.count_nonzero(loses & ~(1.0 - d_i < 0.0)) - np.count_nonzero(wins & ~(1.0 - d_k < 0.0))
            else:
                w_k = np.where(wins, _weight(base, q, k, everyone), 0.0)
                w_i = np.where(loses, _weight(base, q, everyone, k), 0.0)
                got[x] = (float(np.sum(w_i * _sigmoid(-sigma * d_i))) - float(np.sum(w_k * _sigmoid(-sigma * d_k)))) \
                    * sigma / LN2
        if kind == "dcg_hinge":
            got *= dcg_hinge_modifier(H[b])[1]
        out.append(got)
    return out
