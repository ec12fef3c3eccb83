"""GPU tier: rankings and ranking metrics on lists longer than 4096 documents (the sort path behind
include/ltr_hip.h: ltr_*_long_f32) against the oracle, the reference's golden vectors, the one-workgroup
kernels (ltr_debug_long_sort_all) and numpy.

The oracle ranks by counting (O(L^2) per row), so it judges lists up to 16 385 documents; longer ones are
judged by `_np_rank`, a numpy statement of the same rule (score descending, -0.0 == +0.0, index ascending,
padded tail in index order) that is itself checked against the oracle here."""
import numpy as np
import pytest
import torch

from oracle import ltr_oracle as O
from tests.conftest import synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _np_rank(scores, n):
    B, L = scores.shape
    out = np.empty((B, L), dtype=np.int64)
    for b in range(B):
        nb = int(min(max(int(n[b]), 0), L))
        s = scores[b, :nb].astype(np.float32) + np.float32(0.0)
        out[b, :nb] = np.argsort(-s, kind="stable")
        out[b, nb:] = np.arange(nb, L)
    return out


def _np_dcg(scores, y, n, k=None, exp=True, normalize=False):
    """The reference's dcg / ndcg (padded labels counted, maxDCG 0 -> 1) in float64 over _np_rank."""
    B, L = scores.shape
    y = y.astype(np.float64)
    gain = (lambda v: 2.0 ** v - 1.0) if exp else (lambda v: v)
    disc = 1.0 / np.log2(np.arange(L) + 2.0)
    curve = np.cumsum(gain(np.take_along_axis(y, _np_rank(scores, n), 1)) * disc, 1)
    if normalize:
        ideal = y.copy()
        for b in range(B):
            nb = int(min(max(int(n[b]), 0), L))
            ideal[b, :nb] = np.sort(y[b, :nb])[::-1]
        icurve = np.cumsum(gain(ideal) * disc, 1)
        curve = curve / np.where(icurve == 0, 1.0, icurve)
    return curve if k is None else curve[:, min(k, L) - 1]


def _np_arp(scores, y, n):
    B, L = scores.shape
    rank = _np_rank(scores, n)
    out = np.zeros(B)
    for b in range(B):
        nb = int(min(max(int(n[b]), 0), L))
        yr = y[b, rank[b, :nb]].astype(np.float64)
        s = yr.sum()
        out[b] = (np.arange(1, nb + 1) * yr).sum() / (s if s != 0 else 1.0)
    return out


def _tie_rows(L, seed):
    """Rows full of ties, in the style of test_gpu_stress.py::test_sorted_ranks_with_ties_on_long_lists."""
    g = torch.Generator().manual_seed(seed)
    s = torch.randint(-3, 4, (4, L), generator=g).float() * 0.5            # 7 distinct values
    s[1] = 1.25                                                             # one value only
    s[2, ::2] = 0.0
    s[2, 1::2] = -0.0                                                       # signed zeros tie
    s[3] = torch.randn(L, generator=g)
    s[3, ::5] = float("-inf")
    return s


def _batch(L, seed):
    s, y, _ = synth(6, L, seed)
    s = torch.cat([s, _tie_rows(L, seed + 1)])
    y = torch.cat([y, torch.randint(0, 5, (4, L), generator=torch.Generator().manual_seed(seed + 2))])
    n = torch.tensor([L, L - 1, L // 3 + 1, 1, 0, L + 3, L, L, L - 1, L // 2 + 1])
    return s, y, n


def _index():
    from pytorchltr_amd.utils import tie_breaking
    return tie_breaking("index")


@pytest.mark.parametrize("L", [4097, 5000, 8192, 16384, 16385, 65537, 300000])
def test_rank_by_score_matches_oracle(L):
    from pytorchltr_amd.utils import rank_by_score
    s, _, n = _batch(L, L)
    with _index():
        got = rank_by_score(s.to(DEV), n.to(DEV)).cpu().numpy()
    want = _np_rank(s.numpy(), n.numpy())
    assert np.array_equal(got, want)
    if L <= 16385:
        assert np.array_equal(want, O.rank_by_score(s.numpy(), n.numpy()))


@pytest.mark.parametrize("ydt", [torch.int64, torch.int32, torch.float32])
def test_metrics_match_oracle(ydt):
    from pytorchltr_amd.evaluation import arp, dcg, ndcg
    L = 5000
    s, y, n = _batch(L, 7)
    if ydt == torch.float32:
        y = y.float() * 0.75 + 0.1                                          # non-integer grades
    y = y.to(ydt)                                                           # padded labels are non-zero in most rows
    sn, yn, nn = s.numpy(), y.numpy(), n.numpy()
    # the numpy statement of the metrics against the oracle, once
    assert np.allclose(_np_dcg(sn, yn, nn, normalize=True), O.ndcg(sn, yn, nn), rtol=1e-9, atol=1e-12)
    assert np.allclose(_np_arp(sn, yn, nn), O.arp(sn, yn, nn), rtol=1e-9)
    sd, yd, nd = s.to(DEV), y.to(DEV), n.to(DEV)
    with _index():
        for exp in (True, False):
            for k in (None, 1, 10, 1000, L, L + 5):
                for fn, norm in ((dcg, False), (ndcg, True)):
                    got = fn(sd, yd, nd, k=k, exp=exp).cpu().numpy()
                    want = _np_dcg(sn, yn, nn, k=k, exp=exp, normalize=norm)
                    tol = dict(rtol=2e-5, atol=1e-6) if k is not None else dict(rtol=5e-5, atol=1e-5)
                    assert np.allclose(got, want, **tol), (fn.__name__, k, exp)
        assert np.allclose(arp(sd, yd, nd).cpu().numpy(), _np_arp(sn, yn, nn), rtol=2e-5, atol=1e-6)


def _direct(lib, name, *args):
    from pytorchltr_amd import _C
    _C.check(getattr(lib, name)(*args))


@pytest.mark.parametrize("L", [129, 1000, 2049, 4096])
def test_long_path_equals_one_workgroup_path(L):
    """ltr_debug_long_sort_all(1): the sort path at lists the one-workgroup kernels take too."""
    from pytorchltr_amd import _C
    lib = _C.lib()
    s, y, n = _batch(L, 100 + L)
    sd, yd, nd = s.to(DEV).contiguous(), y.to(DEV).contiguous(), n.to(DEV)
    B = s.shape[0]
    st = _C.stream_of(sd)
    tie = torch.randperm(L, generator=torch.Generator().manual_seed(L), dtype=torch.int32).to(DEV)
    ws = [torch.empty(lib.ltr_sort_workspace_bytes(op, B, L), dtype=torch.uint8, device=DEV) for op in range(3)]

    def both(fn):
        prev = lib.ltr_debug_long_sort_all(1)
        try:
            a = fn(True)
        finally:
            lib.ltr_debug_long_sort_all(prev)
        return a, fn(False)

    for t in (None, tie):
        def rank(long):
            out = torch.empty(B, L, dtype=torch.int64, device=DEV)
            if long:
                _direct(lib, "ltr_rank_by_score_long_f32", sd.data_ptr(), nd.data_ptr(), _C.ptr(t), 0, 0, None, B, L,
                        out.data_ptr(), ws[0].data_ptr(), ws[0].numel(), st)
            else:
                _direct(lib, "ltr_rank_by_score_tie_f32", sd.data_ptr(), nd.data_ptr(), _C.ptr(t), B, L, out.data_ptr(), st)
            return out.cpu().numpy()
        a, b = both(rank)
        assert np.array_equal(a, b)
        for k in (0, 10, L):
            for norm in (0, 1):
                def metric(long):
                    out = torch.empty((B,) if k else (B, L), dtype=torch.float32, device=DEV)
                    if long:
                        _direct(lib, "ltr_dcg_long_f32", sd.data_ptr(), yd.data_ptr(), 0, nd.data_ptr(), _C.ptr(t), 0, 0,
                                None, B, L, k, 1, norm, out.data_ptr(), ws[1].data_ptr(), ws[1].numel(), st)
                    else:
                        _direct(lib, "ltr_dcg_tie_f32", sd.data_ptr(), yd.data_ptr(), 0, nd.data_ptr(), _C.ptr(t), B, L,
                                k, 1, norm, out.data_ptr(), st)
                    return out.cpu().numpy()
                a, b = both(metric)
                tol = dict(rtol=2e-5, atol=1e-6) if k else dict(rtol=5e-5, atol=1e-5)
                assert np.allclose(a, b, **tol), (k, norm)

        def arp(long):
            out = torch.empty(B, dtype=torch.float32, device=DEV)
            if long:
                _direct(lib, "ltr_arp_long_f32", sd.data_ptr(), yd.data_ptr(), 0, nd.data_ptr(), _C.ptr(t), 0, 0, None,
                        B, L, out.data_ptr(), ws[2].data_ptr(), ws[2].numel(), st)
            else:
                _direct(lib, "ltr_arp_tie_f32", sd.data_ptr(), yd.data_ptr(), 0, nd.data_ptr(), _C.ptr(t), B, L,
                        out.data_ptr(), st)
            return out.cpu().numpy()
        a, b = both(arp)
        assert np.allclose(a, b, rtol=2e-5, atol=1e-6)


def test_random_ties_follow_the_long_hash():
    from pytorchltr_amd import _C, _ties
    from pytorchltr_amd.utils import rank_by_score, tie_breaking
    lib = _C.lib()
    L, B = 5000, 3
    s = torch.zeros(B, L, device=DEV)
    n = torch.tensor([L, 3000, 1], device=DEV)
    seed = 0x1234_5678_9ABC
    ws = torch.empty(lib.ltr_sort_workspace_bytes(0, B, L), dtype=torch.uint8, device=DEV)
    out = torch.empty(B, L, dtype=torch.int64, device=DEV)
    _direct(lib, "ltr_rank_by_score_long_f32", s.data_ptr(), n.data_ptr(), None, 1, seed, None, B, L, out.data_ptr(),
            ws.data_ptr(), ws.numel(), _C.stream_of(s))
    got = out.cpu().numpy()
    w = _ties.hash_words_long(seed, L)
    for b, nb in enumerate((L, 3000, 1)):
        assert np.array_equal(got[b, :nb], np.argsort(w[:nb], kind="stable"))
        assert np.array_equal(got[b, nb:], np.arange(nb, L))
    # the seed read from device memory (a device generator's draw) gives the same as passing it
    sdev = torch.tensor([seed], dtype=torch.int64, device=DEV)
    out2 = torch.empty_like(out)
    _direct(lib, "ltr_rank_by_score_long_f32", s.data_ptr(), n.data_ptr(), None, 1, 0, sdev.data_ptr(), B, L,
            out2.data_ptr(), ws.data_ptr(), ws.numel(), _C.stream_of(s))
    assert torch.equal(out, out2)
    g = torch.Generator(device=DEV).manual_seed(5)
    a = rank_by_score(s, n, generator=g)
    g2 = torch.Generator(device=DEV).manual_seed(5)
    assert torch.equal(a, rank_by_score(s, n, generator=g2))
    # torch.manual_seed reproduces a call of the package's default (random) mode -- the suite runs in index mode
    with tie_breaking("random"):
        torch.manual_seed(11)
        r1 = rank_by_score(s, n)
        torch.manual_seed(11)
        assert torch.equal(r1, rank_by_score(s, n))
        torch.manual_seed(12)
        assert not torch.equal(r1, rank_by_score(s, n))
        # over 200 seeds the first-ranked of 5000 tied documents is spread roughly uniformly (10 bins of 500)
        first = np.array([int(rank_by_score(s[:1], n[:1])[0, 0]) for _ in range(200)])
    counts = np.bincount(first // 500, minlength=10)
    assert counts.min() >= 5 and counts.max() <= 45, counts
    assert np.unique(first).size > 150


def test_golden_reference_vectors():
    """The reference's outputs (tests/golden/generate_long_list_golden.py) on inputs that generator's
    `batch()` remakes from integer arithmetic."""
    import json
    import os
    from pytorchltr_amd.evaluation import arp, dcg, ndcg
    from pytorchltr_amd.utils import rank_by_score
    from tests.golden.generate_long_list_golden import SHAPES, batch, curve_positions, rank_digest
    base = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "long_list_vectors")
    z = np.load(base + ".npz")
    manifest = json.load(open(base + ".json"))["shapes"]
    for B, L in SHAPES:
        tag = "L%d" % L
        s_np, y_np, n_np = batch(B, L)
        assert n_np.tolist() == manifest[tag]["n"]
        s, y, n = (torch.from_numpy(a).to(DEV) for a in (s_np, y_np, n_np))
        # (the reference orders the padded tail by its random tie-break too: the real documents are compared; the
        # padded labels are zero, so the metrics do not depend on that order)
        got = rank_by_score(s, n).cpu().numpy()
        if tag + "_rank" in z:
            for b, nb in enumerate(n_np):
                assert np.array_equal(got[b, :nb], z[tag + "_rank"][b, :nb])
        assert rank_digest(got, n_np) == manifest[tag]["rank_sha256"]
        for k in (1, 10, 100):
            assert np.allclose(dcg(s, y, n, k=k).cpu().numpy(), z["%s_dcg%d" % (tag, k)], rtol=2e-5, atol=1e-6)
            assert np.allclose(ndcg(s, y, n, k=k).cpu().numpy(), z["%s_ndcg%d" % (tag, k)], rtol=2e-5, atol=1e-6)
        assert np.allclose(arp(s, y, n).cpu().numpy(), z[tag + "_arp"], rtol=2e-5, atol=1e-6)
        if manifest[tag]["curves"]:
            pos = curve_positions(L)
            assert np.allclose(dcg(s, y, n).cpu().numpy()[:, pos], z[tag + "_dcg_curve"], rtol=5e-5, atol=1e-5)
            assert np.allclose(ndcg(s, y, n).cpu().numpy()[:, pos], z[tag + "_ndcg_curve"], rtol=5e-5, atol=1e-5)


def test_evaluation_loop_with_one_long_query():
    """The reference's evaluation loop (collate_fn, no sampler): one 6 000-document query among 50
    short ones pads the whole batch past 4096."""
    from pytorchltr_amd.datasets.ragged import RaggedQueries
    from pytorchltr_amd.evaluation import ndcg
    from pytorchltr_amd.fused import LinearScorer
    g = torch.Generator().manual_seed(3)
    counts = [int(c) for c in torch.randint(5, 60, (50,), generator=g)]
    counts.insert(17, 6000)
    F = 8
    N = sum(counts)
    X = torch.randn(N, F, generator=g)
    ys = torch.randint(0, 5, (N,), generator=g)
    offsets = torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int64)
    data = RaggedQueries(X, ys, offsets, device=DEV)
    batch = data.collate_fn()(list(range(len(counts))))
    assert batch.features.shape[1] == 6000
    torch.manual_seed(0)
    model = LinearScorer(F, lazy=False).to(DEV)
    with torch.no_grad(), _index():
        scores = model(batch.features)
        got = ndcg(scores, batch.relevance, batch.n, k=10).cpu().numpy()
    sc = scores.reshape(len(counts), -1).cpu().numpy()
    want = O.ndcg(sc, batch.relevance.cpu().numpy(), batch.n.cpu().numpy(), k=10)
    assert np.allclose(got, want, rtol=2e-5, atol=1e-6)


def test_plackettluce_on_a_long_list():
    from pytorchltr_amd import _C
    from pytorchltr_amd.utils.tensor_operations import _plackettluce_from_uniform
    L, B = 10000, 3
    g = torch.Generator().manual_seed(9)
    s = torch.randn(B, L, generator=g).to(DEV)
    u = torch.rand(B, L, generator=g).to(DEV)
    n = torch.tensor([L, 7000, 1], device=DEV)
    got = _plackettluce_from_uniform(s, n, u).cpu().numpy()
    keys = torch.empty_like(s)
    _direct(_C.lib(), "ltr_plackettluce_keys_f32", s.data_ptr(), n.data_ptr(), u.data_ptr(), B, L, keys.data_ptr(),
            _C.stream_of(s))
    k = keys.cpu().numpy()
    for b, nb in enumerate((L, 7000, 1)):
        assert np.array_equal(got[b, :nb], np.argsort(-k[b, :nb], kind="stable"))
        assert np.array_equal(got[b, nb:], np.arange(nb, L))


def test_many_queries_sampled_rows():
    from pytorchltr_amd.evaluation import arp, ndcg
    from pytorchltr_amd.utils import rank_by_score
    B, L = 2048, 4100
    s, y, n = synth(B, L, 41)
    n[:3] = torch.tensor([L, 0, 1])
    rows = np.array([0, 1, 2, 3, 500, 1023, 1500, 2047])
    with _index():
        r = rank_by_score(s.to(DEV), n.to(DEV)).cpu().numpy()[rows]
        m = ndcg(s.to(DEV), y.to(DEV), n.to(DEV), k=10).cpu().numpy()[rows]
        a = arp(s.to(DEV), y.to(DEV), n.to(DEV)).cpu().numpy()[rows]
    ss, yy, nn = s.numpy()[rows], y.numpy()[rows], n.numpy()[rows]
    assert np.array_equal(r, O.rank_by_score(ss, nn))
    assert np.allclose(m, O.ndcg(ss, yy, nn, k=10), rtol=2e-5, atol=1e-6)
    assert np.allclose(a, O.arp(ss, yy, nn), rtol=2e-5, atol=1e-6)


def test_one_query_of_four_million():
    from pytorchltr_amd.utils import rank_by_score
    L = 1 << 22
    s = torch.randn(1, L, generator=torch.Generator().manual_seed(4))
    s[0, ::7] = 0.5                                                        # some ties as well
    with _index():
        got = rank_by_score(s.to(DEV), torch.tensor([L], device=DEV)).cpu().numpy()
    assert np.array_equal(got[0], np.argsort(-s[0].numpy(), kind="stable"))


def test_identical_calls_are_bit_identical():
    from pytorchltr_amd.evaluation import arp, ndcg
    from pytorchltr_amd.utils import rank_by_score
    B, L = 16, 100000
    s, y, n = synth(B, L, 5)
    sd, yd, nd = s.to(DEV), y.to(DEV), n.to(DEV)
    with _index():
        for fn in (lambda: rank_by_score(sd, nd), lambda: ndcg(sd, yd, nd), lambda: ndcg(sd, yd, nd, k=10),
                   lambda: arp(sd, yd, nd)):
            assert torch.equal(fn(), fn())
    # the longest curves against the float64 statement: fp32 tile sums (4096 terms) plus a sum of tile sums
    with _index():
        got = ndcg(sd[:2], yd[:2], nd[:2]).cpu().numpy()
    assert np.allclose(got, _np_dcg(s.numpy()[:2], y.numpy()[:2], n.numpy()[:2], normalize=True), rtol=5e-5, atol=1e-5)


def test_graph_capture():
    from pytorchltr_amd.evaluation import ndcg
    B, L = 8, 6000
    s, y, n = synth(B, L, 77)
    sd, yd, nd = s.to(DEV), y.to(DEV), n.to(DEV)
    with _index():
        eager = ndcg(sd, yd, nd, k=10)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ndcg(sd, yd, nd, k=10)                                         # warm-up off the default stream
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = ndcg(sd, yd, nd, k=10)
        sd.copy_(s.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, eager)
