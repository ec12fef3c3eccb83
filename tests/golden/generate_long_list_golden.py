#!/usr/bin/env python
"""Generate golden vectors for lists longer than 4096 documents by importing the REAL reference
(rjagerman/pytorchltr), which runs on the CPU here:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/generate_long_list_golden.py

Writes tests/golden/long_list_vectors.npz (+ long_list_vectors.json manifest): DATA only -- the
reference's outputs.  The inputs are not stored: `batch()` below makes them from integer arithmetic
alone (a splitmix64 hash of the position), and the GPU test makes the same inputs with it.  Stored:
  - rank_by_score as a SHA-256 digest of every row's real documents (int64, little-endian) in the
    manifest, and the full ranking of the shortest shape (int32);
  - dcg / ndcg at k in {1, 10, 100} and arp per query;
  - the dcg / ndcg curves of the two shorter shapes at the positions `curve_positions()` picks (the
    first 128 ranks and every 61st after) -- the fixture stays under 100 KB.
Scores are distinct within a row and padded labels are 0, so the reference's random tie-break (which
also orders its padded tail) does not enter the real documents' ranks or the metrics.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(4, 4097), (3, 12000), (2, 70000)]
KS = (1, 10, 100)


def _splitmix64(x):
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def batch(B, L):
    """(scores float32 (B, L), labels int64 (B, L), n int64 (B)) of one shape: every row's scores are a
    permutation of k / L - 0.5 (distinct), labels 0..4 with the padded ones 0."""
    idx = np.arange(B * L, dtype=np.uint64).reshape(B, L) + (np.uint64(L) << np.uint64(32))
    h = _splitmix64(idx)                                   # a bijection of distinct inputs: distinct
    perm = np.argsort(h, axis=1, kind="stable")
    scores = (perm.astype(np.float64) / L - 0.5).astype(np.float32)
    y = ((h >> np.uint64(40)) % np.uint64(5)).astype(np.int64)
    n = np.array([L, L - 1, L // 3 + 1, 1][:B], dtype=np.int64)
    y[np.arange(L)[None, :] >= n[:, None]] = 0
    return scores, y, n


def curve_positions(L):
    return np.union1d(np.arange(128), np.arange(128, L, 61))


def rank_digest(rank, n):
    return [hashlib.sha256(np.ascontiguousarray(rank[b, :int(nb)], dtype="<i8").tobytes()).hexdigest()
            for b, nb in enumerate(n)]


def main():
    import torch
    REFERENCE = os.environ.get("PYTORCHLTR_REFERENCE", "/root/reference")
    sys.dont_write_bytecode = True
    sys.path.insert(0, REFERENCE)
    from pytorchltr.evaluation import arp, dcg, ndcg
    from pytorchltr.utils import rank_by_score

    out, manifest = {}, {}
    for B, L in SHAPES:
        s_np, y_np, n_np = batch(B, L)
        scores, y, n = torch.from_numpy(s_np), torch.from_numpy(y_np), torch.from_numpy(n_np)
        tag = "L%d" % L
        rank = rank_by_score(scores, n).numpy()
        if L == SHAPES[0][1]:
            out[tag + "_rank"] = rank.astype(np.int32)
        for k in KS:
            out["%s_dcg%d" % (tag, k)] = dcg(scores, y, n, k=k).numpy()
            out["%s_ndcg%d" % (tag, k)] = ndcg(scores, y, n, k=k).numpy()
        out[tag + "_arp"] = arp(scores, y, n).numpy()
        curves = L < SHAPES[-1][1]
        if curves:
            pos = curve_positions(L)
            out[tag + "_dcg_curve"] = dcg(scores, y, n).numpy()[:, pos].astype(np.float32)
            out[tag + "_ndcg_curve"] = ndcg(scores, y, n).numpy()[:, pos].astype(np.float32)
        manifest[tag] = {"B": B, "L": L, "n": n_np.tolist(), "curves": curves, "rank_sha256": rank_digest(rank, n_np)}
    np.savez_compressed(os.path.join(HERE, "long_list_vectors.npz"), **out)
    with open(os.path.join(HERE, "long_list_vectors.json"), "w") as f:
        json.dump({"shapes": manifest, "k": list(KS), "source": "rjagerman/pytorchltr v0.2.1 on CPU"}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
