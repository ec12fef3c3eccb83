"""CPU tier of evaluate() (pytorchltr_amd/evaluation/metrics.py, include/ltr_eval.h): metric-name parsing, the fp64
numpy oracle of the metric definitions against hand-worked values and scikit-learn, and the host-side return codes of
the new entry points.  The GPU tier (tests/test_gpu_eval.py) checks the kernels against the same oracle."""
import ctypes
import math
import os

import numpy as np
import pytest

# ---- the oracle: an fp64 restatement of the definitions in include/ltr_eval.h ----


def oracle_ranking(scores, n):
    """Score descending, ties by document index, over the real documents; padded ones keep their positions."""
    B, L = scores.shape
    out = np.tile(np.arange(L), (B, 1))
    for b in range(B):
        nb = int(min(max(n[b], 0), L))
        out[b, :nb] = np.lexsort((np.arange(nb), -scores[b, :nb].astype(np.float64)))
    return out


def _parse(name):
    base, _, k = name.partition("@")
    return base, (int(k) if k else 0)


def oracle(name, ranking, relevance, n, exp=True, relevance_level=1, err_max_grade=4):
    """(B,) fp64 value of metric `name` for rows ranked by `ranking` ((B, L) document indices, real documents first)."""
    base, k = _parse(name)
    y = np.asarray(relevance, dtype=np.float64)
    B, L = y.shape
    out = np.zeros(B)
    for b in range(B):
        nb = int(min(max(n[b], 0), L))
        lab = y[b, ranking[b, :nb]]
        if base in ("dcg", "ndcg"):
            kk = min(k, L) if k > 0 else L
            disc = 1.0 / np.log2(np.arange(L) + 2.0)
            gain = (lambda v: 2.0 ** v - 1.0) if exp else (lambda v: v)
            dcg = np.sum(gain(np.concatenate([lab, y[b, nb:]])[:kk]) * disc[:kk])     # padded labels counted
            if base == "ndcg":
                ideal = np.concatenate([np.sort(y[b, :nb])[::-1], y[b, nb:]])
                idcg = np.sum(gain(ideal[:kk]) * disc[:kk])
                dcg /= idcg if idcg != 0 else 1.0
            out[b] = dcg
            continue
        if base == "arp":
            s = np.sum((np.arange(nb) + 1.0) * lab)
            c = np.sum(lab)
            out[b] = s / (c if c != 0 else 1.0)
            continue
        rel = lab >= relevance_level
        R = rel.sum()
        if R == 0:
            continue
        kc = min(k, nb) if k > 0 else nb
        ranks = np.arange(1, nb + 1, dtype=np.float64)
        if base == "p":
            out[b] = rel[:kc].sum() / (k if k > 0 else L)
        elif base == "recall":
            out[b] = rel[:kc].sum() / R
        elif base == "map":
            hits = np.cumsum(rel)
            out[b] = np.sum((hits / ranks)[:kc][rel[:kc]]) / R
        elif base == "mrr":
            first = int(np.argmax(rel))
            out[b] = 1.0 / (first + 1) if first < kc else 0.0
        elif base == "err":
            g = np.clip(lab, 0, err_max_grade)
            p = (2.0 ** g - 1.0) / 2.0 ** err_max_grade
            keep = np.concatenate([[1.0], np.cumprod(1.0 - p)[:-1]])
            out[b] = np.sum((p * keep / ranks)[:kc])
        else:
            raise ValueError(name)
    return out


# ---- metric names ----

def test_parse_metric_names():
    from pytorchltr_amd.evaluation.metrics import parse_metrics
    names, spec = parse_metrics(("ndcg@1", "ndcg", "dcg@3", "arp", "map", "map@5", "mrr", "mrr@2", "p@10",
                                 "recall@10", "err", "err@10", "p", "recall"))
    assert names[0] == "ndcg@1" and len(names) == 14
    assert list(spec) == [1, 1, 1, 0, 0, 3, 2, 0, 3, 0, 3, 5, 4, 0, 4, 2, 5, 10, 6, 10, 7, 0, 7, 10, 5, 0, 6, 0]
    assert parse_metrics("map")[0] == ("map",)
    assert parse_metrics(["ndcg@%d" % k for k in range(1, 33)])[0][-1] == "ndcg@32"


@pytest.mark.parametrize("bad", [(), ("ndcg@0",), ("ndcg@-1",), ("ndcg@",), ("ndcg@1.5",), ("ndcg@01",),
                                 ("NDCG@10",), ("precision@10",), ("arp@5",), ("map@k",), ("",), (" map",),
                                 ("map", "map"), tuple("ndcg@%d" % k for k in range(1, 34)), (10,)])
def test_bad_metric_names_raise_value_error(bad):
    from pytorchltr_amd.evaluation.metrics import parse_metrics
    with pytest.raises(ValueError):
        parse_metrics(bad)


def test_evaluate_checks_names_before_touching_tensors():
    import torch
    from pytorchltr_amd.evaluation import evaluate
    s = torch.zeros(2, 4)
    with pytest.raises(ValueError):
        evaluate(s, s.long(), torch.full((2,), 4), metrics=("nope",))
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # CPU tensors are refused, as everywhere
        evaluate(s, s.long(), torch.full((2,), 4), metrics=("map",))


def test_wrappers_mirror_the_reference_argument_order():
    import inspect
    import pytorchltr_amd.evaluation as ev
    for fn in (ev.average_precision, ev.reciprocal_rank, ev.precision, ev.recall, ev.err):
        params = list(inspect.signature(fn).parameters)
        assert params[:4] == ["scores", "relevance", "n", "k"], fn.__name__
        assert inspect.signature(fn).parameters["k"].default is None
    assert "max_grade" in inspect.signature(ev.err).parameters


# ---- the oracle against hand-worked values ----

ERR_FULL = 1 / 2 * 1 / 16 + 1 / 3 * 3 / 16 * 15 / 16 + 1 / 4 * 1 / 16 * 15 / 16 * 13 / 16


@pytest.mark.parametrize("name, level, want", [
    ("p@2", 1, 1 / 2), ("p@10", 1, 3 / 10), ("p", 1, 3 / 4), ("recall@2", 1, 1 / 3), ("recall@10", 1, 1.0),
    ("map", 1, (1 / 2 + 2 / 3 + 3 / 4) / 3), ("map@2", 1, (1 / 2) / 3), ("map@10", 1, (1 / 2 + 2 / 3 + 3 / 4) / 3),
    ("mrr", 1, 1 / 2), ("mrr@1", 1, 0.0), ("mrr@2", 1, 1 / 2), ("err", 1, ERR_FULL), ("err@2", 1, 1 / 32),
    ("err@10", 1, ERR_FULL),
    ("map", 2, 1 / 3), ("mrr", 2, 1 / 3), ("p@2", 2, 0.0), ("p@3", 2, 1 / 3), ("recall@2", 2, 0.0),
    ("recall@3", 2, 1.0), ("err", 2, ERR_FULL),
    ("dcg", 1, 1 / math.log2(3) + 3 / 2 + 1 / math.log2(5)),
    ("ndcg", 1, (1 / math.log2(3) + 3 / 2 + 1 / math.log2(5)) / (3 + 1 / math.log2(3) + 1 / 2)),
    ("ndcg@1", 1, 0.0), ("arp", 1, (2 * 1 + 3 * 2 + 4 * 1) / 4),
])
def test_oracle_hand_worked(name, level, want):
    scores = np.array([[3.0, 2.0, 1.0, 0.0]])
    labels = np.array([[0, 1, 2, 1]])
    n = np.array([4])
    got = oracle(name, oracle_ranking(scores, n), labels, n, relevance_level=level)
    assert got[0] == pytest.approx(want, rel=1e-12, abs=1e-15)


@pytest.mark.parametrize("name", ["map", "map@3", "mrr", "p@2", "recall@2", "err", "err@1"])
def test_oracle_no_relevant_document_and_empty_lists(name):
    scores = np.array([[3.0, 2.0, 1.0, 0.0]] * 3)
    labels = np.array([[0, 0, 0, 0], [1, 1, 0, 0], [4, 4, 4, 4]])
    n = np.array([4, 4, 0])
    got = oracle(name, oracle_ranking(scores, n), labels, n, relevance_level=2)
    assert np.array_equal(got, np.zeros(3))          # R = 0 (ERR too, though R_i > 0 for label 1), n = 0


def test_oracle_k_beyond_n_and_padding():
    scores = np.array([[1.0, 3.0, 2.0, 9.0, 9.0]])
    labels = np.array([[1, 0, 1, 4, 4]])
    n = np.array([3])                                 # documents 3, 4 are padding: ignored by the trec_eval metrics
    r = oracle_ranking(scores, n)
    assert r[0].tolist() == [1, 2, 0, 3, 4]
    assert oracle("p@10", r, labels, n)[0] == pytest.approx(2 / 10)
    assert oracle("recall@10", r, labels, n)[0] == pytest.approx(1.0)
    assert oracle("map@10", r, labels, n)[0] == pytest.approx((1 / 2 + 2 / 3) / 2)
    assert oracle("mrr@10", r, labels, n)[0] == pytest.approx(1 / 2)
    # dcg counts the padded labels at their own positions (the reference's quirk)
    want = 1 / math.log2(3) + 1 / 2 + 15 / math.log2(5) + 15 / math.log2(6)
    assert oracle("dcg", r, labels, n)[0] == pytest.approx(want)


def _tie_free(seed, B, L, grades):
    rng = np.random.default_rng(seed)
    scores = np.stack([rng.permutation(L) for _ in range(B)]).astype(np.float64) + rng.random((B, L)) * 0.5
    labels = rng.integers(0, grades, (B, L))
    labels[:, 0] = grades - 1                            # at least one relevant document per row
    return scores, labels, np.full(B, L)


def test_oracle_average_precision_against_sklearn():
    from sklearn.metrics import average_precision_score
    scores, labels, n = _tie_free(11, 40, 37, 2)
    got = oracle("map", oracle_ranking(scores, n), labels, n)
    want = [average_precision_score(labels[b], scores[b]) for b in range(len(n))]
    assert np.allclose(got, want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("k", [None, 1, 5, 10])
def test_oracle_ndcg_against_sklearn(k):
    from sklearn.metrics import ndcg_score
    scores, labels, n = _tie_free(12, 30, 23, 5)
    name = "ndcg" if k is None else "ndcg@%d" % k
    got = oracle(name, oracle_ranking(scores, n), labels, n, exp=False)
    want = [ndcg_score(labels[b][None], scores[b][None], k=k) for b in range(len(n))]
    assert np.allclose(got, want, rtol=1e-12, atol=0)


# ---- return codes of include/ltr_eval.h, no GPU (no case below gets as far as a launch) ----

P = 256                                        # dummy non-NULL device pointer: never dereferenced below
_SPEC2 = (ctypes.c_int32 * 4)(1, 10, 3, 0)     # ndcg@10, map
_BADOP = (ctypes.c_int32 * 4)(1, 10, 8, 0)
_NEGK = (ctypes.c_int32 * 4)(1, -1, 3, 0)
_ARGS = ["scores", "rel", "rel_dtype", "n", "tie", "use_seed", "seed", "seed_dev", "B", "L", "spec", "M",
         "relevance_level", "use_exp", "err_max_grade", "out", "workspace", "workspace_bytes", "stream"]
_VALID = dict(scores=P, rel=P, rel_dtype=0, n=P, tie=None, use_seed=0, seed=0, seed_dev=None, B=2, L=16, spec=_SPEC2,
              M=2, relevance_level=1.0, use_exp=1, err_max_grade=4.0, out=P, workspace=P, workspace_bytes=1 << 40,
              stream=None)
LONG = dict(L=5000)                            # past 4096 documents: the sort path, which needs the workspace

# (changed arguments, expected return code); every case fails a check or is the B = 0 no-op
EVAL_CASES = [
    (dict(scores=None), -1), (dict(rel=None), -1), (dict(n=None), -1), (dict(spec=None), -1), (dict(out=None), -1),
    (dict(B=-1), -2), (dict(B=0), 0), (dict(B=0, scores=None), 0), (dict(L=0), -2), (dict(L=(1 << 24) + 1), -4),
    (dict(rel_dtype=7), -3), (dict(spec=_BADOP), -3), (dict(M=0), -2), (dict(M=33), -2), (dict(spec=_NEGK), -2),
    (dict(LONG, workspace_bytes=1), -5), (dict(LONG, workspace=None), -5), (dict(LONG, workspace_bytes=0), -5),
    # two at once: kind / dtype, then shape (M, k), then the lists, then NULL, then the workspace
    (dict(rel_dtype=7, B=-1), -3), (dict(spec=_BADOP, M=0), -2), (dict(spec=_BADOP, B=-1), -3),
    (dict(spec=_NEGK, L=0), -2), (dict(M=33, scores=None), -2), (dict(M=0, B=0), -2), (dict(L=0, out=None), -2),
    (dict(L=(1 << 24) + 1, scores=None), -4), (dict(B=-1, spec=None), -2), (dict(LONG, workspace=None, n=None), -1),
    (dict(LONG, workspace_bytes=1, B=0), 0), (dict(spec=None, M=0), -2),
]


@pytest.fixture(scope="module")
def lib():
    from pytorchltr_amd import _C
    from pytorchltr_amd.build import build_extension
    if not os.environ.get("LTR_HIP_LIB"):
        build_extension()
    return _C.lib()


@pytest.mark.parametrize("i", range(len(EVAL_CASES)))
def test_eval_return_codes(lib, i):
    change, want = EVAL_CASES[i]
    args = dict(_VALID, **change)
    assert lib.ltr_eval_f32(*[args[a] for a in _ARGS]) == want, change


def test_eval_workspace_bytes(lib):
    ws = lib.ltr_eval_workspace_bytes
    assert ws(2, 16, _SPEC2, 2) == 0                                   # one workgroup per query: none
    tiles = -(-5000 // 4096)
    al = lambda x: -(-x // 256) * 256                                  # noqa: E731
    assert ws(2, 5000, _SPEC2, 2) == al(16 * 2 * 5000) + al(4 * 5000) + 4 * 2 * tiles * (2 * 2 + 3)
    for bad in [(-1, 5000, _SPEC2, 2), (2, 0, _SPEC2, 2), (2, (1 << 24) + 1, _SPEC2, 2), (2, 5000, None, 2),
                (2, 5000, _SPEC2, 0), (2, 5000, _SPEC2, 33), (2, 5000, _BADOP, 2), (2, 5000, _NEGK, 2)]:
        assert ws(*bad) == 0, bad
    prev = lib.ltr_debug_long_sort_all(1)                              # the forced sort path needs it at any L
    try:
        assert ws(2, 16, _SPEC2, 2) == al(16 * 2 * 16) + al(4 * 16) + 4 * 2 * 1 * 7
    finally:
        lib.ltr_debug_long_sort_all(prev)


def test_eval_header_matches_the_ctypes_table():
    import re
    from pytorchltr_amd import _C
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "ltr_eval.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(ltr_[a-z0-9_]+)\s*\(", text))) == sorted(_C.EVAL_SIGNATURES)
    assert not set(_C.EVAL_SIGNATURES) & set(_C.SIGNATURES)


def test_eval_kernels_do_not_spill():
    """tests/test_codeobj.py's rule for the new kernels: no VGPR spill, no scratch."""
    from pytorchltr_amd import _codeobj
    from pytorchltr_amd.build import LIB_PATH, build_extension
    build_extension()
    try:
        recs = _codeobj.kernel_records(LIB_PATH)
    except FileNotFoundError as exc:          # no llvm tools on this machine
        pytest.skip(str(exc))
    names = [r.get("demangled", r["name"]) for r in recs]
    ours = [r for r, n in zip(recs, names) if "eval_kernel<" in n or "eval_long_" in n]
    assert len(ours) == 10, names
    for r in ours:
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, r.get("demangled")
