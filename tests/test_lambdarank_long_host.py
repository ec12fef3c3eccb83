"""CPU tier of LambdaRankLoss on lists longer than ltr_max_list_len() documents (include/ltr_lambdarank_long.h;
pytorchltr_amd/csrc/ltr_lambdarank_long.inc): the blocked fp64 reference (tests/lambdarank_long_ref.py) against the
O(L^2) one, the header and its ctypes table, the workspace formula, the return codes in the documented order, the
Python bound and the new kernels' code-object notes.  The library is built, nothing is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import lambdarank_long_ref as RL
from tests import lambdarank_ref as R

NEW = ("ltr_lambdarank_long_workspace_bytes", "ltr_lambdarank_long_f32", "ltr_debug_lambdarank_long_all")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ltr_lambdarank_long.h")


@pytest.fixture(scope="module")
def lib():
    from pytorchltr_amd import _C
    from pytorchltr_amd.build import build_extension
    if not os.environ.get("LTR_HIP_LIB"):
        build_extension()
    return _C.lib()


# ---- the reference against tests/lambdarank_ref.py ----
def _close(got, want, what):
    """1e-12 relative to the largest magnitude of the expected values."""
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    assert got.shape == want.shape, what
    if want.size:
        assert float(np.max(np.abs(got - want))) <= 1e-12 * float(np.max(np.abs(want))), what


@pytest.mark.parametrize("L", [1, 2, 3, 17, 257, 1000])
@pytest.mark.parametrize("k", [None, 1, 10, 1 << 20])
def test_reference_equals_the_quadratic_one(L, k):
    rng = np.random.default_rng(100 * L + (k or 0) % 97)
    B = 5
    s = rng.standard_normal((B, L)).astype(np.float32)
    y = rng.integers(0, 5, (B, L)).astype(np.int64)
    kk = k if k not in (None, 1 << 20) else 10
    # duplicate scores straddling the cutoff of row 0; n_b in {0, 1, k, k + 1} on rows 1..4
    if L >= 3:
        top = np.argsort(-s[0], kind="stable")
        lo, hi = max(0, min(kk, L) - 2), min(L, min(kk, L) + 2)
        s[0, top[lo:hi]] = s[0, top[lo]]
    n = np.array([L, 0, 1, min(kk, L), min(kk + 1, L)], dtype=np.int64)
    for sigma in (1.0, 2.5):
        want_l, want_g = R.batch(s, y, n, k, sigma)
        for block in (RL.BLOCK, 7):                                    # (a block that divides nothing as well)
            got_l, got_g = RL.batch(s, y, n, k, sigma, block)
            for b in range(B):
                _close(got_l[b], want_l[b], (L, k, sigma, b, "loss"))
                _close(got_g[b], want_g[b], (L, k, sigma, b, "grad"))
            assert not got_g[1].any() and not got_g[2].any() and got_l[1] == 0.0 and got_l[2] == 0.0


def test_reference_edge_cases():
    assert RL.row(np.zeros(0), np.zeros(0))[0] == 0.0 and RL.row(np.ones(1), np.ones(1))[0] == 0.0
    loss, g = RL.row(np.array([0.3, -1.0, 2.0]), np.array([2, 2, 2]))
    assert loss == 0.0 and not g.any()
    assert RL.row(np.array([1.0, 2.0]), np.zeros(2))[0] == 0.0
    # ties by index: with all scores equal the ranks are the indices
    y = np.array([0, 3, 1, 2], dtype=np.int64)
    _close(RL.row(np.zeros(4), y, 2)[1], R.row(np.zeros(4), y, 2)[1], "ties")
    # a float label of -1 has the gain -0.5
    yf = np.array([-1.0, 2.0, 0.0], dtype=np.float32)
    _close(RL.row(np.array([0.1, 0.2, 0.3]), yf, 2)[0], R.row(np.array([0.1, 0.2, 0.3]), yf, 2)[0], "gain -0.5")


# ---- the header ----
def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_table_and_exports(lib):
    from pytorchltr_amd import _C, build
    text = _header()
    declared = sorted(set(re.findall(r"\b(ltr_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW) == sorted(_C.LAMBDARANK_LONG_SIGNATURES)
    others = (set(_C.SIGNATURES) | set(_C.EVAL_SIGNATURES) | set(_C.LISTWISE_SIGNATURES) | set(_C.LONGPAIR_SIGNATURES)
              | set(_C.LAMBDARANK_SIGNATURES) | set(_C.MLP_ROWS_SIGNATURES) | set(_C.MLP_WIDE_SIGNATURES)
              | set(_C.MLP_BF16_SIGNATURES) | set(_C.LINEAR_BF16_SIGNATURES) | set(_C.SCHED_SIGNATURES))
    hooks_hidden = os.environ.get("LTR_NO_DEBUG_HOOKS") == "1"
    for name in NEW:
        assert name not in others, name
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(proto.split(",")) == len(_C.LAMBDARANK_LONG_SIGNATURES[name][1]), name
        if name.startswith("ltr_debug_") and hooks_hidden:
            assert not hasattr(ctypes.CDLL(_C.LIB_PATH), name), "a production build exports %s" % name
            continue
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr), name
        assert getattr(lib, name).argtypes == _C.LAMBDARANK_LONG_SIGNATURES[name][1]   # bound as the other tables are
        assert getattr(lib, name).restype == _C.LAMBDARANK_LONG_SIGNATURES[name][0]
    assert re.search(r"LTR_DEBUG_HOOK\s+int\s+ltr_debug_lambdarank_long_all", text)
    assert HEADER in build.DEPENDS
    assert os.path.join(build.CSRC, "ltr_lambdarank_long.inc") in build.DEPENDS
    assert lib.ltr_version() == 114
    # the short entry points keep their bound
    assert lib.ltr_lambdarank_f32(256, 256, 0, 256, 10, 1.0, 2, 4097, 256, None, None) == -4
    assert lib.ltr_linear_lambdarank_plan(6, 4097, 136) == 0


def test_header_states_the_order_of_the_errors_and_the_formula():
    text = " ".join(open(HEADER).read().replace("*", " ").split())
    words = ("LTR_ERR_KIND", "LTR_ERR_SHAPE", "LTR_ERR_LIST_TOO_LONG", "B == 0 is a no-op", "LTR_ERR_NULL",
             "LTR_ERR_WORKSPACE", "sticky device status")
    tail = text[text.index("Errors, in this order"):]
    order = [tail.index(w) for w in words]
    assert order == sorted(order)
    assert "ltr_lambdarank_long_workspace_bytes(k, B, L) =" in text and "ltr_sort_workspace_bytes(1, B, L)" in text


# ---- the size query ----
def _al(x):
    return -(-x // 256) * 256


def _formula(lib, k, B, L):
    """The closed form of include/ltr_lambdarank_long.h."""
    T = -(-L // 1024)
    kc = k if 0 < k < L else 0
    return (lib.ltr_sort_workspace_bytes(1, B, L) + 2 * _al(8 * B * L) + 2 * _al(4 * B * L) + _al(4 * B * T)
            + _al(4 * B * kc * (T - kc // 1024)))


def test_workspace_bytes(lib):
    ws = lib.ltr_lambdarank_long_workspace_bytes
    for k in (0, 1, 10, 5000, 1 << 20):
        for L in (1, 64, 4095, 4096):
            assert ws(k, 3, L) == 0, (k, L)                            # the call is ltr_lambdarank_f32 there
        prev = 0
        for L in (4097, 5000, 8192, 8193, 12289, 40000, 65535, 65536):
            got = ws(k, 3, L)
            assert got == _formula(lib, k, 3, L) > 0, (k, L)
            assert got >= prev, (k, L)                                 # monotone in L
            prev = got
    for L in range(4097, 4200):                                        # ... also step by step
        assert ws(10, 2, L + 1) >= ws(10, 2, L) > 0
    for bad in [(10, -1, 5000), (10, 2, 0), (10, 2, -3), (10, 2, 65537), (0, 2, 1 << 20)]:
        assert ws(*bad) == 0, bad


def test_workspace_bytes_under_the_hook(lib):
    if os.environ.get("LTR_NO_DEBUG_HOOKS") == "1":
        return                                                         # a production build has no debug hooks
    ws = lib.ltr_lambdarank_long_workspace_bytes
    prev = lib.ltr_debug_lambdarank_long_all(1)
    try:
        for k in (0, 1, 10):
            for L in (1, 63, 1024, 1025, 4096):
                assert ws(k, 3, L) == _formula(lib, k, 3, L) > 0, (k, L)
        assert lib.ltr_debug_lambdarank_long_all(1) == 1               # returns the old value
    finally:
        lib.ltr_debug_lambdarank_long_all(prev)
    assert ws(10, 3, 64) == 0


# ---- return codes (no case gets as far as a launch) ----
P = 256                                        # dummy non-NULL device pointer: never dereferenced
KIND, SHAPE, TOO_LONG, NULL, WORKSPACE = -3, -2, -4, -1, -5
INF, NAN = float("inf"), float("nan")
_ARGS = ["scores", "rel", "rel_dtype", "n", "k", "sigma", "B", "L", "loss", "dscores", "workspace", "workspace_bytes",
         "stream"]
_VALID = dict(scores=P, rel=P, rel_dtype=0, n=P, k=10, sigma=1.0, B=2, L=5000, loss=P, dscores=None, workspace=P,
              workspace_bytes=1 << 40, stream=None)
CASES = [
    (dict(rel_dtype=7), KIND), (dict(rel_dtype=-1), KIND),
    (dict(B=-1), SHAPE), (dict(L=0), SHAPE), (dict(L=-3), SHAPE), (dict(sigma=INF), SHAPE), (dict(sigma=-INF), SHAPE),
    (dict(sigma=NAN), SHAPE),
    (dict(L=65537), TOO_LONG), (dict(L=1 << 24), TOO_LONG),
    (dict(B=0), 0), (dict(B=0, scores=None, loss=None, workspace=None), 0),
    (dict(scores=None), NULL), (dict(rel=None), NULL), (dict(n=None), NULL), (dict(loss=None), NULL),
    (dict(workspace=None), WORKSPACE), (dict(workspace_bytes=0), WORKSPACE), (dict(workspace_bytes=4096), WORKSPACE),
    (dict(L=65536, workspace_bytes=1 << 20), WORKSPACE),
    # two at once: the dtype, then the shape, then the length, then B == 0, then NULL, then the workspace
    (dict(rel_dtype=7, B=-1), KIND), (dict(rel_dtype=7, sigma=NAN), KIND), (dict(rel_dtype=7, L=65537), KIND),
    (dict(rel_dtype=7, scores=None), KIND), (dict(rel_dtype=7, B=0), KIND), (dict(rel_dtype=7, workspace=None), KIND),
    (dict(B=-1, L=65537), SHAPE), (dict(sigma=NAN, L=65537), SHAPE), (dict(L=0, scores=None), SHAPE),
    (dict(sigma=INF, B=0), SHAPE), (dict(sigma=INF, workspace=None), SHAPE),
    (dict(L=65537, scores=None), TOO_LONG), (dict(L=65537, B=0), TOO_LONG), (dict(L=65537, workspace=None), TOO_LONG),
    (dict(B=0, workspace_bytes=0), 0),
    (dict(workspace=None, n=None), NULL), (dict(workspace_bytes=0, loss=None), NULL),
    # at most ltr_max_list_len() documents the call is ltr_lambdarank_f32: its checks, no workspace
    (dict(L=16, scores=None, workspace=None), NULL), (dict(L=16, rel_dtype=9, workspace=None), KIND),
    (dict(L=4096, n=None, workspace=None, workspace_bytes=0), NULL),
]


@pytest.mark.parametrize("i", range(len(CASES)))
def test_return_codes_in_the_documented_order(lib, i):
    change, want = CASES[i]
    args = dict(_VALID, **change)
    assert lib.ltr_lambdarank_long_f32(*[args[a] for a in _ARGS]) == want, change


def test_workspace_one_byte_short(lib):
    need = lib.ltr_lambdarank_long_workspace_bytes(10, 2, 5000)
    args = dict(_VALID, workspace_bytes=need - 1)
    assert lib.ltr_lambdarank_long_f32(*[args[a] for a in _ARGS]) == WORKSPACE


# ---- the Python bound ----
def test_python_bound_is_host_logic(lib, monkeypatch):
    from pytorchltr_amd import _C, fused
    from pytorchltr_amd.loss import LambdaRankLoss
    monkeypatch.setattr(_C, "require_device", lambda t, what: None)
    too_long = _C.max_pair_list_len() + 1
    assert too_long == 65537
    y, n = torch.zeros(1, too_long, dtype=torch.int64), torch.tensor([too_long])
    with pytest.raises(ValueError, match=r"max_pair_list_len\(\) = 65536"):
        LambdaRankLoss(k=10)(torch.zeros(1, too_long), y, n)
    # no flag: the kind stays the two-field tuple
    assert fused._resolve_loss(LambdaRankLoss(k=10))[0] == (_C.LISTWISE_LAMBDARANK, 10)
    assert not hasattr(LambdaRankLoss(), "long_lists")
    assert "quadratic" in LambdaRankLoss.__doc__ and "65 536" in LambdaRankLoss.__doc__


# ---- the code object ----
def test_kernels_do_not_spill():
    from pytorchltr_amd import _codeobj
    from pytorchltr_amd.build import LIB_PATH, build_extension
    build_extension()
    try:
        recs = _codeobj.kernel_records(LIB_PATH)
    except FileNotFoundError as exc:          # no llvm tools on this machine
        pytest.skip(str(exc))
    ours = [(r, r.get("demangled", r["name"])) for r in recs if "lambdarank_long" in r.get("demangled", r["name"])]
    # the maxDCG partials, the by-rank epilogue, the pair pass without and with the anchors' share, the finish
    assert len(ours) == 5, [n for _, n in ours]
    for r, n in ours:
        assert "lambdarank_kernel<" not in n, n
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, n
