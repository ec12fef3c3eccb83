"""evaluate(): many ranking metrics of a batch from ONE ranking pass on the GPU (include/ltr_eval.h).

Each query is ranked once -- one workgroup per query up to 4096 documents, the sort path beyond -- and
every requested metric is read off that ranking, so all metrics of a call see the same order of tied
documents (two separate ``ndcg`` calls may not, under the default "random" tie-breaking).

Metric names (ranks r start at 1; a name without ``@k`` means the whole list, k = list_size):

``dcg``, ``dcg@k``, ``ndcg``, ``ndcg@k``
    exactly ``dcg(..., k)`` / ``ndcg(..., k)`` of this package (``ndcg`` without k: the last column of
    ``ndcg(..., k=None)``); as in the reference, labels of padded documents are counted.  ``exp`` applies
    to these two only.
``arp``
    exactly ``arp(...)``.

The others follow trec_eval and look at the real documents j < n[b] only.  A document is relevant iff
its label is at least ``relevance_level``; R is the number of relevant real documents.  Each of them is
0 when R = 0, and so when n = 0.

``p@k``
    relevant documents in the top min(k, n), divided by k (trec_eval's P_k: divided by k even when n < k).
``recall@k``
    relevant documents in the top k, divided by R.
``map``, ``map@k``
    sum over relevant ranks r <= k of (relevant documents in the top r) / r, divided by R (the full R
    also for ``map@k``, as trec_eval's map_cut).
``mrr``, ``mrr@k``
    1 / (rank of the first relevant document), 0 when that rank is beyond k.
``err``, ``err@k``
    sum over r <= k of (1 / r) R_r prod_{i < r} (1 - R_i), R_i = (2^g - 1) / 2^gmax, g = the label clamped
    to [0, gmax], gmax = ``err_max_grade`` (Chapelle et al. 2009).
"""
import ctypes
import re
from typing import Dict, Optional, Sequence

import torch as _torch

from pytorchltr_amd import _C
from pytorchltr_amd import _ties
from pytorchltr_amd._prepare import prepare as _prepare

# enum ltr_eval_op (include/ltr_eval.h)
_OPS = {"dcg": 0, "ndcg": 1, "arp": 2, "map": 3, "mrr": 4, "p": 5, "recall": 6, "err": 7}
MAX_METRICS = 32
_NAME = re.compile(r"^([a-z]+)(?:@([0-9]+))?$")
_specs = {}


def parse_metrics(metrics: Sequence[str]):
    """(names, ctypes int32 array of (op, k) pairs) for a list of metric names; k = 0 for no cutoff.
    Raises ValueError for an unknown or malformed name, k <= 0, a repeated name, no names or more than 32."""
    if isinstance(metrics, str):
        metrics = (metrics,)
    names = tuple(metrics)
    hit = _specs.get(names)
    if hit is not None:
        return hit
    if not names:
        raise ValueError("evaluate() needs at least one metric")
    if len(names) > MAX_METRICS:
        raise ValueError("evaluate() takes at most %d metrics, got %d" % (MAX_METRICS, len(names)))
    if len(set(names)) != len(names):
        raise ValueError("repeated metric name in %r" % (names,))
    pairs = []
    for name in names:
        m = _NAME.match(name) if isinstance(name, str) else None
        if m is None or m.group(1) not in _OPS:
            raise ValueError("unknown metric %r (known: %s, with an optional @k)" % (name, ", ".join(sorted(_OPS))))
        base, k = m.group(1), m.group(2)
        if k is not None:
            if base == "arp":
                raise ValueError("metric %r: arp takes no cutoff" % name)
            if k.startswith("0"):
                raise ValueError("metric %r: the cutoff must be a positive integer" % name)
        pairs += [_OPS[base], int(k) if k is not None else 0]
    hit = (names, (ctypes.c_int32 * len(pairs))(*pairs))
    _specs[names] = hit
    return hit


def evaluate(scores: _torch.Tensor, relevance: _torch.Tensor, n: _torch.Tensor,
             metrics: Sequence[str] = ("ndcg@10",), exp: bool = True, relevance_level: float = 1,
             err_max_grade: float = 4) -> Dict[str, _torch.Tensor]:
    """The requested metrics of every query, from one ranking per query (see the module docstring).

    Args:
        scores: (batch, list_size[, 1]) scores (half / fp64 are computed in fp32).
        relevance: (batch, list_size[, 1]) labels, int64, int32 or fp32.
        n: (batch,) number of documents per query (clamped to list_size).
        metrics: metric names, e.g. ("ndcg@10", "map", "mrr", "p@10").
        exp: gain 2^y - 1 (True) or y for dcg / ndcg.
        relevance_level: the smallest label that counts as relevant for the trec_eval metrics.
        err_max_grade: gmax of ERR.

    Returns:
        dict name -> (batch,) fp32 tensor on the device of `scores`, in request order; the values are
        rows of one (len(metrics), batch) buffer.
    """
    names, spec = parse_metrics(metrics)
    s, r, nn = _prepare(scores, relevance, n, limit_len=False)
    B, L = s.shape
    if L > _C.max_sort_list_len():
        raise ValueError("list_size %d exceeds the supported maximum %d" % (L, _C.max_sort_list_len()))
    M = len(names)
    out = _torch.empty((M, B), dtype=_torch.float32, device=s.device)
    if B > 0:
        lib = _C.lib()
        sd = _ties.draw_seed(L, s.device)            # one draw per call: every metric sees the same ranking
        ws, nbytes = _C.workspace(lib.ltr_eval_workspace_bytes(B, L, spec, M), s.device)
        with _C.device_ctx(s):
            _C.check(lib.ltr_eval_f32(
                _C.ptr(s), _C.ptr(r), _C.label_dtype(r), _C.ptr(nn), *_ties.tie_args(sd), B, L, spec, M,
                float(relevance_level), int(bool(exp)), float(err_max_grade), _C.ptr(out), _C.ptr(ws), nbytes,
                _C.stream_of(s)))
    return {name: out[i] for i, name in enumerate(names)}


def _one(scores, relevance, n, base, k, **kw):
    name = base if k is None else "%s@%d" % (base, int(k))
    return evaluate(scores, relevance, n, metrics=(name,), **kw)[name]


def average_precision(scores: _torch.Tensor, relevance: _torch.Tensor, n: _torch.Tensor, k: Optional[int] = None,
                      relevance_level: float = 1) -> _torch.Tensor:
    """(batch,) average precision (``map`` / ``map@k`` of evaluate) per query."""
    return _one(scores, relevance, n, "map", k, relevance_level=relevance_level)


def reciprocal_rank(scores: _torch.Tensor, relevance: _torch.Tensor, n: _torch.Tensor, k: Optional[int] = None,
                    relevance_level: float = 1) -> _torch.Tensor:
    """(batch,) reciprocal rank of the first relevant document (``mrr`` / ``mrr@k`` of evaluate)."""
    return _one(scores, relevance, n, "mrr", k, relevance_level=relevance_level)


def precision(scores: _torch.Tensor, relevance: _torch.Tensor, n: _torch.Tensor, k: Optional[int] = None,
              relevance_level: float = 1) -> _torch.Tensor:
    """(batch,) precision at k (``p@k`` of evaluate; k = None: k = list_size)."""
    return _one(scores, relevance, n, "p", k, relevance_level=relevance_level)


def recall(scores: _torch.Tensor, relevance: _torch.Tensor, n: _torch.Tensor, k: Optional[int] = None,
           relevance_level: float = 1) -> _torch.Tensor:
    """(batch,) recall at k (``recall@k`` of evaluate; k = None: the whole list)."""
    return _one(scores, relevance, n, "recall", k, relevance_level=relevance_level)


def err(scores: _torch.Tensor, relevance: _torch.Tensor, n: _torch.Tensor, k: Optional[int] = None,
        max_grade: float = 4) -> _torch.Tensor:
    """(batch,) expected reciprocal rank (``err`` / ``err@k`` of evaluate, gmax = max_grade)."""
    return _one(scores, relevance, n, "err", k, err_max_grade=max_grade)
