"""CPU tier of LambdaRankLoss (include/ltr_lambdarank.h; pytorchltr_amd/csrc/ltr_lambdarank.inc,
ltr_lambdarank_row.inc): the C ABI's table and exports, the return codes of both calls in the documented order, the
plan rule, the fp64 reference itself (tests/lambdarank_ref.py: its weights against NDCG@K swaps computed by the oracle,
its gradient against central differences), the loss names of pytorchltr_amd.fused and the new kernels' register use.
The library is built, nothing is launched."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import lambdarank_ref as R

NEW = ("ltr_lambdarank_f32", "ltr_linear_lambdarank_plan", "ltr_linear_lambdarank_partials_f32")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from pytorchltr_amd import _C
    from pytorchltr_amd.build import build_extension
    if not os.environ.get("LTR_HIP_LIB"):
        build_extension()
    return _C.lib()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltr_lambdarank.h")).read(), flags=re.S)


def test_header_table_and_exports(lib):
    from pytorchltr_amd import _C, build
    text = _header()
    declared = sorted(set(re.findall(r"\b(ltr_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW) == sorted(_C.LAMBDARANK_SIGNATURES)
    others = (set(_C.SIGNATURES) | set(_C.EVAL_SIGNATURES) | set(_C.LISTWISE_SIGNATURES) | set(_C.LONGPAIR_SIGNATURES)
              | set(_C.MLP_ROWS_SIGNATURES) | set(_C.MLP_WIDE_SIGNATURES) | set(_C.MLP_BF16_SIGNATURES)
              | set(_C.LINEAR_BF16_SIGNATURES) | set(_C.SCHED_SIGNATURES))
    for name in NEW:
        assert name not in others, name
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr), name
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(proto.split(",")) == len(_C.LAMBDARANK_SIGNATURES[name][1]), name
        assert getattr(lib, name).argtypes == _C.LAMBDARANK_SIGNATURES[name][1]         # bound as the other tables are
    # ltr_hip.h's table is still exactly ltr_hip.h, and the version did not move
    hip = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltr_hip.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(ltr_[a-z0-9_]+)\s*\(", hip))) == sorted(_C.SIGNATURES)
    assert lib.ltr_version() == 114
    assert _C.LISTWISE_LAMBDARANK not in (_C.LISTWISE_LISTNET, _C.LISTWISE_LISTMLE)
    assert os.path.join(ROOT, "include", "ltr_lambdarank.h") in build.DEPENDS


# ---- return codes (no case gets as far as a launch) ----
P = 256                                        # dummy non-NULL, 16-byte aligned device pointer: never dereferenced
KIND, SHAPE, TOO_LONG, NULL, CONFIG = -3, -2, -4, -1, -6
INF, NAN = float("inf"), float("nan")

_LOSS_ARGS = ["scores", "rel", "rel_dtype", "n", "k", "sigma", "B", "L", "loss", "dscores", "stream"]
_LOSS_VALID = dict(scores=P, rel=P, rel_dtype=0, n=P, k=10, sigma=1.0, B=2, L=16, loss=P, dscores=None, stream=None)
LOSS_CASES = [
    (dict(rel_dtype=7), KIND), (dict(rel_dtype=-1), KIND),
    (dict(B=-1), SHAPE), (dict(L=0), SHAPE), (dict(L=-3), SHAPE), (dict(sigma=INF), SHAPE), (dict(sigma=-INF), SHAPE),
    (dict(sigma=NAN), SHAPE),
    (dict(L=4097), TOO_LONG), (dict(L=1 << 20), TOO_LONG),
    (dict(B=0), 0), (dict(B=0, scores=None, loss=None), 0),
    (dict(scores=None), NULL), (dict(rel=None), NULL), (dict(n=None), NULL), (dict(loss=None), NULL),
    # two at once: the dtype, then the shape, then the length, then B == 0, then NULL
    (dict(rel_dtype=7, B=-1), KIND), (dict(rel_dtype=7, sigma=NAN), KIND), (dict(rel_dtype=7, L=5000), KIND),
    (dict(rel_dtype=7, scores=None), KIND), (dict(rel_dtype=7, B=0), KIND),
    (dict(B=-1, L=5000), SHAPE), (dict(sigma=NAN, L=5000), SHAPE), (dict(L=0, scores=None), SHAPE),
    (dict(sigma=INF, B=0), SHAPE),
    (dict(L=5000, scores=None), TOO_LONG), (dict(L=5000, B=0), TOO_LONG),
]

_STEP_ARGS = ["k", "sigma", "X", "W", "bias", "rel", "rel_dtype", "n", "B", "L", "F", "loss_out", "scores_out", "partials",
              "stream"]
_STEP_VALID = dict(k=0, sigma=1.0, X=P, W=P, bias=None, rel=P, rel_dtype=0, n=P, B=2, L=16, F=8, loss_out=P,
                   scores_out=None, partials=P, stream=None)
STEP_CASES = [
    (dict(rel_dtype=7), KIND), (dict(rel_dtype=-1), KIND),
    (dict(B=-1), SHAPE), (dict(L=0), SHAPE), (dict(L=-3), SHAPE), (dict(F=0), SHAPE), (dict(F=-4), SHAPE),
    (dict(sigma=INF), SHAPE), (dict(sigma=NAN), SHAPE),
    (dict(L=4097), TOO_LONG), (dict(L=1 << 20), TOO_LONG),
    (dict(B=0), 0), (dict(B=0, X=None, partials=None), 0), (dict(B=0, F=5), 0),
    (dict(X=None), NULL), (dict(W=None), NULL), (dict(rel=None), NULL), (dict(n=None), NULL), (dict(loss_out=None), NULL),
    (dict(partials=None), NULL),
    (dict(F=5), CONFIG), (dict(F=46), CONFIG), (dict(X=P + 4), CONFIG), (dict(partials=P + 8), CONFIG),
    (dict(L=4096, F=1 << 16), CONFIG),
    # two at once: the dtype, then the shape, then the length, then B == 0, then NULL, then the plan
    (dict(rel_dtype=7, B=-1), KIND), (dict(rel_dtype=7, L=0), KIND), (dict(rel_dtype=7, X=None), KIND),
    (dict(rel_dtype=7, L=5000), KIND), (dict(rel_dtype=7, sigma=NAN), KIND),
    (dict(B=-1, L=5000), SHAPE), (dict(F=0, X=None), SHAPE), (dict(L=0, F=5), SHAPE), (dict(sigma=NAN, F=5), SHAPE),
    (dict(sigma=INF, B=0), SHAPE),
    (dict(L=5000, X=None), TOO_LONG), (dict(L=5000, F=5), TOO_LONG), (dict(L=5000, B=0), TOO_LONG),
    (dict(X=None, F=5), NULL), (dict(n=None, X=P + 4), NULL),
]


@pytest.mark.parametrize("i", range(len(LOSS_CASES)))
def test_loss_return_codes_in_the_documented_order(lib, i):
    change, want = LOSS_CASES[i]
    args = dict(_LOSS_VALID, **change)
    assert lib.ltr_lambdarank_f32(*[args[a] for a in _LOSS_ARGS]) == want, change


@pytest.mark.parametrize("i", range(len(STEP_CASES)))
def test_step_return_codes_in_the_documented_order(lib, i):
    change, want = STEP_CASES[i]
    args = dict(_STEP_VALID, **change)
    assert lib.ltr_linear_lambdarank_partials_f32(*[args[a] for a in _STEP_ARGS]) == want, change


def test_header_states_the_order_of_the_errors():
    text = " ".join(open(os.path.join(ROOT, "include", "ltr_lambdarank.h")).read().replace("*", " ").split())
    words = ("LTR_ERR_KIND", "LTR_ERR_SHAPE", "LTR_ERR_LIST_TOO_LONG", "B == 0 is a no-op", "LTR_ERR_NULL")
    first = text[text.index("dscores may be NULL"):text.index("int ltr_lambdarank_f32(")]
    order = [first.index(w) for w in words]
    assert order == sorted(order)
    tail = text[text.index("ltr_linear_lambdarank_plan: 1 where"):]
    order = [tail.index(w) for w in words + ("LTR_ERR_CONFIG", "sticky device status")]
    assert order == sorted(order)
    assert "loss_out equals ltr_lambdarank_f32 on scores_out bit for bit" in text


# ---- the plan ----
def test_plan(lib):
    plan = lib.ltr_linear_lambdarank_plan
    assert lib.ltr_max_list_len() == 4096
    for shape in ((1024, 128, 136), (6, 4096, 700), (1, 1, 4), (7, 300, 8), (7, 1000, 700)):
        assert plan(*shape) == 1, shape
    assert plan(6, 4097, 136) == 0
    assert plan(6, 128, 5) == 0 and plan(6, 128, 46) == 0 and plan(6, 128, 6) == 0
    for bad in ((0, 128, 136), (-1, 128, 136), (6, 0, 136), (6, -2, 136), (6, 128, 0), (6, 128, -4)):
        assert plan(*bad) == 0, bad
    # a row whose weights alone are past the LDS left behind the longest ranked row
    assert plan(6, 4096, 1 << 16) == 0
    # the existing entry points do not know the Python-side code
    assert lib.ltr_linear_listwise_plan(2, 1024, 128, 136) == 0


# ---- the reference itself ----
def _separated(rng, L, spacing=0.25):
    """Tie-free scores at least `spacing` apart, in a random order."""
    s = (np.arange(L) * spacing + rng.uniform(0.0, spacing * 0.2, L)).astype(np.float32)
    return s[rng.permutation(L)]


@pytest.mark.parametrize("k", [None, 1, 3, 100])
def test_reference_weights_are_ndcg_swap_deltas(k):
    from oracle import ltr_oracle as O
    L = 7
    rng = np.random.default_rng(3 + (k or 0))
    for _ in range(4):
        s = _separated(rng, L)
        y = rng.integers(0, 5, L).astype(np.int64)
        if not y.any():
            y[0] = 3
        w, _ = R.pair_weights(s, y, k)
        K = R.cutoff(k, L)
        n = np.array([L], dtype=np.int64)
        base = O.ndcg(s[None, :].astype(np.float64), y[None, :], n, k=K)[0]
        for i in range(L):
            for j in range(i + 1, L):
                # swapping the ranks of i and j = swapping their labels under the same scores
                y2 = y.copy()
                y2[i], y2[j] = y[j], y[i]
                swapped = O.ndcg(s[None, :].astype(np.float64), y2[None, :], n, k=K)[0]
                assert abs(w[i, j] - abs(base - swapped)) <= 1e-12, (k, i, j)
                assert w[i, j] == w[j, i]


@pytest.mark.parametrize("k", [None, 1, 3, 100])
@pytest.mark.parametrize("sigma", [1.0, 2.5])
def test_reference_gradient_equals_central_differences(k, sigma):
    L = 7
    rng = np.random.default_rng(11 + (k or 0))
    s = _separated(rng, L, spacing=0.1 * 1.25).astype(np.float64)      # >= 0.1 apart: a step of 1e-6 moves no rank
    assert np.min(np.diff(np.sort(s))) >= 0.1
    y = rng.integers(0, 5, L).astype(np.int64)
    y[:2] = (4, 0)
    frozen = R.pair_weights(s.astype(np.float32), y, k)
    _, grad = R.row(s, y, k, sigma, frozen)
    h = 1e-6
    for j in range(L):
        up, dn = s.copy(), s.copy()
        up[j] += h
        dn[j] -= h
        # (the ranking is the same on both sides: the weights of either side equal the frozen ones)
        assert np.array_equal(R.ranks_by_score(up), R.ranks_by_score(s)) and np.array_equal(R.ranks_by_score(dn), R.ranks_by_score(s))
        fd = (R.row(up, y, k, sigma, frozen)[0] - R.row(dn, y, k, sigma, frozen)[0]) / (2 * h)
        assert abs(fd - grad[j]) <= 1e-7 * max(1.0, abs(grad[j])), (j, fd, grad[j])
    assert abs(grad.sum()) <= 1e-12                                    # every lambda is taken from one and given to another


def test_reference_edge_cases():
    # n <= 1, equal labels, no positive gain (maxDCG 0 -> 1), ties by index, a label of -1 (gain -0.5)
    assert R.row(np.zeros(0), np.zeros(0))[0] == 0.0 and R.row(np.ones(1), np.ones(1))[0] == 0.0
    loss, g = R.row(np.array([0.3, -1.0, 2.0]), np.array([2, 2, 2]))
    assert loss == 0.0 and not g.any()
    assert R.max_dcg(np.zeros(4), 4) == 1.0 and R.row(np.array([1.0, 2.0]), np.zeros(2))[0] == 0.0
    assert list(R.ranks_by_score(np.array([1.0, 2.0, 1.0, 2.0], dtype=np.float32))) == [2, 0, 3, 1]
    assert R.gains(np.array([-1.0]))[0] == -0.5
    loss, ds = R.batch(np.zeros((3, 4)), np.arange(12).reshape(3, 4) % 3, np.array([0, 1, 9]), k=2)
    assert loss[0] == 0.0 and loss[1] == 0.0 and loss[2] > 0.0 and not ds[:2].any()


# ---- pytorchltr_amd.fused and the module ----
def test_resolve_loss_takes_the_name_and_the_module():
    from pytorchltr_amd import _C, fused
    from pytorchltr_amd.loss import LambdaRankLoss
    import pytorchltr_amd.loss as Lm
    assert "LambdaRankLoss" in Lm.__all__ and LambdaRankLoss is Lm.pairwise_lambda.LambdaRankLoss
    kind, sigma = fused._resolve_loss("lambdarank")
    assert isinstance(kind, fused._ListwiseKind) and kind == (_C.LISTWISE_LAMBDARANK, None) and sigma == 1.0
    kind, sigma = fused._resolve_loss(LambdaRankLoss(sigma=2.5, k=10))
    assert isinstance(kind, fused._ListwiseKind) and kind == (_C.LISTWISE_LAMBDARANK, 10) and sigma == 2.5
    assert fused._resolve_loss(LambdaRankLoss())[0].k is None
    m = fused.FusedLinearLoss(8, loss=LambdaRankLoss(k=3, sigma=0.5))
    assert m.kind == (_C.LISTWISE_LAMBDARANK, 3) and m.sigma == 0.5
    assert fused.FusedLinearLoss(8, loss="lambdarank").kind.loss == _C.LISTWISE_LAMBDARANK
    # the MLP entry points have no kernel for it
    for make in (lambda: fused.FusedMLPLoss(8, loss="lambdarank"), lambda: fused.FusedMLPLoss(8, loss=LambdaRankLoss(k=5)),
                 lambda: fused.FusedMLPListwiseLoss(8, loss="lambdarank"),
                 lambda: fused.FusedMLPListwiseLoss(8, loss=LambdaRankLoss()),
                 lambda: fused.mlp_loss_step(None, None, None, None, loss="lambdarank"),
                 lambda: fused.mlp_loss_step(None, None, None, None, loss=LambdaRankLoss(k=5)),
                 lambda: fused.LazySGD(None, None, 0.1, loss="lambdarank")):
        with pytest.raises(TypeError):
            make()


def test_module_constructor_repr_and_state():
    import torch
    from pytorchltr_amd.loss import LambdaRankLoss
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            LambdaRankLoss(k=bad)
    m = LambdaRankLoss(sigma=2.5, k=10.0)
    assert m.k == 10 and isinstance(m.k, int) and m.sigma == 2.5
    assert "sigma=2.5" in repr(m) and "k=10" in repr(m) and "k=None" in repr(LambdaRankLoss())
    assert LambdaRankLoss().sigma == 1.0 and LambdaRankLoss().k is None
    assert len(m.state_dict()) == 0 and not list(m.parameters())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(2, 5), torch.zeros(2, 5, dtype=torch.long), torch.tensor([5, 3]))


# ---- the code object ----
def test_kernels_do_not_spill_and_are_counted():
    from pytorchltr_amd import _codeobj
    from pytorchltr_amd.build import LIB_PATH, build_extension
    build_extension()
    try:
        recs = _codeobj.kernel_records(LIB_PATH)
    except FileNotFoundError as exc:          # no llvm tools on this machine
        pytest.skip(str(exc))
    names = [r.get("demangled", r["name"]) for r in recs]
    ours = [(r, n) for r, n in zip(recs, names) if "lambdarank_kernel<" in n]
    # the six launch shapes of the ranked-row core, stand-alone and in the fused Linear step
    assert len(ours) == 12 and len([n for _, n in ours if "linear_lambdarank_kernel<" in n]) == 6, [n for _, n in ours]
    for r, n in ours:
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, n
        # up to 1024 threads, two workgroups per CU on the sort shapes (DPT <= 0): 64 VGPRs, 80 SGPRs; the counting-rank
        # shapes keep the core's budget of 128
        dpt = int(re.search(r"lambdarank_kernel<(-?\d+)>", n).group(1))
        assert r["vgpr_count"] <= (64 if dpt <= 0 else 128), n
        if dpt <= 0:
            assert r["sgpr_count"] <= 80, n
