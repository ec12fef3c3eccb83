"""GPU tier of evaluate() (run with `-m gpu` on an MI355X): every metric against the fp64 oracle of
tests/test_eval_host.py, the DCG family and ARP against dcg / ndcg / arp and the reference's golden vectors, one
ranking for all metrics of a call under random tie-breaking, the forced sort path against the one-workgroup
kernel, run-to-run bit identity and stream capture."""
import ctypes

import numpy as np
import pytest
import torch

from tests.conftest import load_golden
from tests.test_eval_host import oracle, oracle_ranking

pytestmark = pytest.mark.gpu

ALL = ("ndcg@1", "ndcg@3", "ndcg@5", "ndcg@10", "ndcg", "dcg@10", "dcg", "arp", "map", "map@10", "mrr", "mrr@5",
       "p@1", "p@10", "recall@10", "err@10", "err", "recall")
NEW = tuple(m for m in ALL if m.split("@")[0] in ("map", "mrr", "p", "recall", "err"))
LENGTHS = [1, 2, 17, 64, 128, 129, 1000, 4096, 4097, 10000]


def _dev():
    assert torch.cuda.is_available(), "GPU tier needs a ROCm device"
    return torch.device("cuda:0")


def _batch(seed, B, L, dtype=np.int64, ties=False, grades=5):
    """Tie-free (or tie-heavy) scores, labels in [0, grades), ragged n with 0, 1, L and more than L."""
    rng = np.random.default_rng(seed)
    if ties:
        s = rng.integers(0, 3, (B, L)).astype(np.float32)
    else:
        s = np.stack([rng.permutation(L) for _ in range(B)]).astype(np.float32) * 0.5 - L / 4
    y = rng.integers(0, grades, (B, L)).astype(dtype)
    n = rng.integers(0, L + 1, B).astype(np.int64)
    for i, v in enumerate((0, 1, L, L + 7)):
        if i < B:
            n[i] = v
    return s, y, n


def _t(*arrays):
    dev = _dev()
    return [torch.as_tensor(a).to(dev) for a in arrays]


def _check(got, want, what, rtol=1e-5, atol=1e-6):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, what
    err = np.abs(got - want) - (atol + rtol * np.abs(want))
    assert np.all(err <= 0), "%s: worst excess %.3e (got %s, want %s)" % (
        what, err.max(), got[np.argmax(err)], want[np.argmax(err)])


@pytest.mark.parametrize("exp", [True, False])
@pytest.mark.parametrize("dtype", [np.int64, np.int32, np.float32])
@pytest.mark.parametrize("L", LENGTHS)
def test_every_metric_against_the_oracle(L, dtype, exp):
    from pytorchltr_amd.evaluation import evaluate
    from pytorchltr_amd.utils import tie_breaking
    B = 64 if L <= 1000 else 6
    s, y, n = _batch(L * 7 + (dtype is np.int32) + 2 * (dtype is np.float32), B, L, dtype)
    ts, ty, tn = _t(s, y, n)
    with tie_breaking("index"):
        out = evaluate(ts, ty, tn, metrics=ALL, exp=exp)
    assert list(out) == list(ALL)
    ranking = oracle_ranking(s, n)
    for name in ALL:
        assert out[name].shape == (B,) and out[name].dtype == torch.float32 and out[name].device == ts.device
        _check(out[name].cpu().numpy(), oracle(name, ranking, y, n, exp=exp), "L=%d %s %s" % (L, name, dtype.__name__))


@pytest.mark.parametrize("L", [17, 1000, 5000])
def test_relevance_level_and_err_max_grade(L):
    from pytorchltr_amd.evaluation import evaluate
    from pytorchltr_amd.utils import tie_breaking
    s, y, n = _batch(3 + L, 16, L, np.float32, grades=7)
    y = y * 0.75                                                      # fractional labels: fp32 relevance
    ts, ty, tn = _t(s, y.astype(np.float32), n)
    with tie_breaking("index"):
        out = evaluate(ts, ty, tn, metrics=NEW, relevance_level=2.5, err_max_grade=3)
    ranking = oracle_ranking(s, n)
    for name in NEW:
        _check(out[name].cpu().numpy(), oracle(name, ranking, y, n, relevance_level=2.5, err_max_grade=3), name)


def test_input_conventions():
    from pytorchltr_amd.evaluation import evaluate, ndcg
    from pytorchltr_amd.utils import tie_breaking
    s, y, n = _batch(5, 8, 33)
    ts, ty, tn = _t(s, y, n)
    with tie_breaking("index"):
        want = evaluate(ts, ty, tn, metrics=("ndcg@5", "map"))
        for ss in (ts[:, :, None], ts.double()):                               # (B, L, 1), fp64 cast to fp32
            got = evaluate(ss, ty, tn, metrics=("ndcg@5", "map"))
            assert torch.equal(got["ndcg@5"], want["ndcg@5"]) and torch.equal(got["map"], want["map"])
        got = evaluate(ts.half(), ty, tn, metrics=("ndcg@5",))["ndcg@5"]       # half: the rounded scores, ranked in fp32
        assert torch.equal(got, ndcg(ts.half().float(), ty, tn, k=5))
        assert torch.equal(evaluate(ts, ty, tn.clamp(max=33) + 100, metrics=("map",))["map"],
                           evaluate(ts, ty, torch.full_like(tn, 33), metrics=("map",))["map"])
        empty = evaluate(ts[:0], ty[:0], tn[:0], metrics=("ndcg@5", "err"))
        assert [v.shape for v in empty.values()] == [(0,), (0,)]
        # the values are rows of one (M, B) buffer
        assert want["map"].data_ptr() - want["ndcg@5"].data_ptr() == 8 * 4


def test_wrappers_are_evaluate_with_one_name():
    import pytorchltr_amd.evaluation as ev
    from pytorchltr_amd.utils import tie_breaking
    s, y, n = _batch(6, 32, 50)
    ts, ty, tn = _t(s, y, n)
    with tie_breaking("index"):
        for fn, name, kw in ((ev.average_precision, "map", {}), (ev.reciprocal_rank, "mrr", {}),
                             (ev.precision, "p", {}), (ev.recall, "recall", {}), (ev.err, "err", {"max_grade": 3})):
            for k in (None, 5):
                full = name if k is None else "%s@%d" % (name, k)
                extra = {"err_max_grade": 3} if kw else {}
                assert torch.equal(fn(ts, ty, tn, k, **kw), ev.evaluate(ts, ty, tn, metrics=(full,), **extra)[full])


@pytest.mark.parametrize("L", [37, 128, 1000, 4097])
def test_index_mode_equals_dcg_ndcg_arp(L):
    import pytorchltr_amd.evaluation as ev
    from pytorchltr_amd.utils import tie_breaking
    s, y, n = _batch(L, 32, L, ties=True)                             # ties: decided by the index in both
    ts, ty, tn = _t(s, y, n)
    names = ("ndcg@1", "ndcg@10", "ndcg", "dcg@3", "dcg", "arp", "ndcg@%d" % (2 * L))
    for exp in (True, False):
        with tie_breaking("index"):
            out = ev.evaluate(ts, ty, tn, metrics=names, exp=exp)
            for name in names:
                base, _, k = name.partition("@")
                if base == "arp":
                    want = ev.arp(ts, ty, tn)
                else:
                    fn = ev.ndcg if base == "ndcg" else ev.dcg
                    want = fn(ts, ty, tn, k=int(k), exp=exp) if k else fn(ts, ty, tn, exp=exp)[:, -1]
                _check(out[name].cpu().numpy(), want.cpu().numpy().astype(np.float64), name, rtol=1e-6, atol=0)


G = load_golden()


@pytest.mark.parametrize("name", [c["name"] for c in G.by_op("metrics")])
def test_reference_golden_vectors(name):
    from pytorchltr_amd.evaluation import evaluate
    from pytorchltr_amd.utils import tie_breaking
    case = G.cases[name]
    s, y, n = G.inputs(name)
    ts, ty, tn = _t(s, y, n)
    L = s.shape[1]
    rtol = 2e-5 if L > 256 else 2e-6
    for exp in (True, False):
        names, fields = [], []
        for k in case["ks"]:
            tag = "k%s_%s" % ("all" if k is None else k, "exp" if exp else "lin")
            for base in ("ndcg", "dcg"):
                names.append(base if k is None else "%s@%d" % (base, k))
                fields.append(base + "_" + tag)
        with tie_breaking("index"):
            out = evaluate(ts, ty, tn, metrics=tuple(names) + ("arp",), exp=exp)
        for nm, field in zip(names, fields):
            want = G.get(name, field)
            want = want[:, -1] if want.ndim == 2 else want
            assert np.allclose(out[nm].cpu().numpy(), want, rtol=rtol, atol=1e-6), (nm, field)
        assert np.allclose(out["arp"].cpu().numpy(), G.get(name, "arp"), rtol=rtol, atol=1e-6)


@pytest.mark.parametrize("L", [64, 1000, 5000])
def test_random_ties_one_ranking_for_all_metrics(L):
    import pytorchltr_amd.evaluation as ev
    from pytorchltr_amd.utils import rank_by_score, tie_breaking
    s, y, n = _batch(100 + L, 16, L, ties=True)
    ts, ty, tn = _t(s, y, n)
    with tie_breaking("random"):
        torch.manual_seed(1234)
        out = ev.evaluate(ts, ty, tn, metrics=("ndcg@10",) + NEW)
        torch.manual_seed(1234)
        want = ev.ndcg(ts, ty, tn, k=10)
        torch.manual_seed(1234)
        ranking = rank_by_score(ts, tn).cpu().numpy()
        torch.manual_seed(999)
        other = ev.evaluate(ts, ty, tn, metrics=("map",))["map"]
    assert torch.equal(out["ndcg@10"], want)
    assert not np.array_equal(ranking, oracle_ranking(s, n))          # the ties really were shuffled
    for name in NEW:
        _check(out[name].cpu().numpy(), oracle(name, ranking, y, n), name)
    assert not torch.equal(other, out["map"])                          # another seed, another ranking of the ties


@pytest.mark.parametrize("L", [17, 129, 1000, 4096])
def test_forced_sort_path_agrees_with_one_workgroup(L):
    from pytorchltr_amd import _C
    from pytorchltr_amd.evaluation import evaluate
    from pytorchltr_amd.utils import tie_breaking
    s, y, n = _batch(200 + L, 24, L, np.int32)
    ts, ty, tn = _t(s, y, n)
    lib = _C.lib()
    with tie_breaking("index"):
        one = evaluate(ts, ty, tn, metrics=ALL)
        prev = lib.ltr_debug_long_sort_all(1)
        try:
            assert lib.ltr_eval_workspace_bytes(24, L, (ctypes.c_int32 * 2)(3, 0), 1) > 0
            srt = evaluate(ts, ty, tn, metrics=ALL)
        finally:
            lib.ltr_debug_long_sort_all(prev)
    for name in ALL:
        _check(srt[name].cpu().numpy(), one[name].cpu().numpy().astype(np.float64), name)


@pytest.mark.parametrize("L", [100, 1000, 10000])
def test_bit_identical_run_to_run(L):
    from pytorchltr_amd.evaluation import evaluate
    from pytorchltr_amd.utils import tie_breaking
    s, y, n = _batch(300 + L, 32, L, ties=True)
    ts, ty, tn = _t(s, y, n)
    for mode in ("index", "random"):
        with tie_breaking(mode):
            torch.manual_seed(7)
            a = evaluate(ts, ty, tn, metrics=ALL)
            torch.manual_seed(7)
            b = evaluate(ts, ty, tn, metrics=ALL)
        for name in ALL:
            assert torch.equal(a[name], b[name]), (mode, name)


@pytest.mark.parametrize("L", [128, 5000])
def test_graph_capture_replays_equal_to_eager(L):
    from pytorchltr_amd.evaluation import evaluate
    from pytorchltr_amd.utils import tie_breaking
    s, y, n = _batch(400 + L, 16, L)
    ts, ty, tn = _t(s, y, n)
    with tie_breaking("index"):
        eager = evaluate(ts, ty, tn, metrics=ALL)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            evaluate(ts, ty, tn, metrics=ALL)                          # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            cap = evaluate(ts, ty, tn, metrics=ALL)
        g.replay()
        torch.cuda.synchronize()
    for name in ALL:
        assert torch.equal(cap[name], eager[name]), name
