"""CPU tier of the pairwise losses on lists longer than ltr_max_list_len() documents (include/ltr_longpair.h,
``long_lists=True``): the workspace formula, the return codes, the Python limits and the module surface.  Nothing here
gets as far as a launch."""
import ctypes
import os
import re

import pytest
import torch

P = 256                                        # dummy non-NULL device pointer: never dereferenced below
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NDCG = (5, 6)                                  # LTR_NDCG1, LTR_NDCG2


@pytest.fixture(scope="module")
def lib():
    from pytorchltr_amd import _C
    from pytorchltr_amd.build import build_extension
    if not os.environ.get("LTR_HIP_LIB"):
        build_extension()
    return _C.lib()


def _al(x):
    return -(-x // 256) * 256


def _formula(lib, kind, B, L):
    """The closed form of include/ltr_longpair.h."""
    from pytorchltr_amd import _C
    own, _ = _C.long_pair_geometry()
    total = _al(4 * B * -(-L // own))
    if kind in NDCG:
        total += _al(8 * B * L) + _al(16 * B * L) + _al(4 * L) + 8 * B * -(-L // 4096)
    return total


def test_limits_and_geometry(lib):
    from pytorchltr_amd import _C
    assert lib.ltr_max_pair_list_len() == _C.max_pair_list_len() == 65536 > lib.ltr_max_list_len()
    own, ch = _C.long_pair_geometry()
    assert own > 0 and ch > 0 and own % 64 == 0 and ch % 8 == 0
    lib.ltr_long_pair_geometry(None, None)     # either pointer may be NULL


@pytest.mark.parametrize("B", [1, 24])
def test_workspace_formula(lib, B):
    from pytorchltr_amd import _C
    ws = lib.ltr_pairwise_loss_long_workspace_bytes
    own, _ = _C.long_pair_geometry()
    lengths = {4097, 5000, 65536}
    for mult in (5, 6, 20):
        lengths |= {mult * own - 1, mult * own, mult * own + 1}
    for kind in range(7):
        for L in (1, 64, 4095, 4096):
            assert ws(kind, B, L) == 0, (kind, L)                      # the call is ltr_pairwise_loss_f32 there
        for L in sorted(lengths):
            assert 4096 < L <= 65536
            assert ws(kind, B, L) == _formula(lib, kind, B, L), (kind, L)
            if kind in NDCG:                                           # ... stated through the sort's own size query
                assert ws(kind, B, L) == _al(4 * B * -(-L // own)) + _al(8 * B * L) + lib.ltr_sort_workspace_bytes(1, B, L)
    for bad in [(7, 2, 5000), (-1, 2, 5000), (0, -1, 5000), (0, 2, 0), (0, 2, -3), (0, 2, 65537), (6, 2, 1 << 20)]:
        assert ws(*bad) == 0, bad
    assert ws(0, 0, 5000) == 0                                         # an empty batch needs none


def test_workspace_formula_under_the_hook(lib):
    ws = lib.ltr_pairwise_loss_long_workspace_bytes
    prev = lib.ltr_debug_long_pairs_all(1)
    try:
        for kind in (0, 2, 5, 6):
            for L in (1, 63, 1024, 1025, 4096):
                assert ws(kind, 3, L) == _formula(lib, kind, 3, L) > 0, (kind, L)
        assert lib.ltr_debug_long_pairs_all(1) == 1                    # returns the old value
    finally:
        lib.ltr_debug_long_pairs_all(prev)
    assert ws(0, 3, 64) == 0


_ARGS = ["kind", "sigma", "scores", "rel", "rel_dtype", "n", "B", "L", "loss", "dscores", "workspace", "workspace_bytes",
         "stream"]
_VALID = dict(kind=0, sigma=1.0, scores=P, rel=P, rel_dtype=0, n=P, B=2, L=5000, loss=P, dscores=P, workspace=P,
              workspace_bytes=1 << 40, stream=None)
CASES = [
    (dict(scores=None), -1), (dict(rel=None), -1), (dict(n=None), -1), (dict(loss=None), -1),
    (dict(B=-1), -2), (dict(L=0), -2), (dict(L=-5), -2),
    (dict(kind=7), -3), (dict(kind=-1), -3), (dict(rel_dtype=7), -3),
    (dict(L=65537), -4), (dict(L=1 << 24), -4),
    (dict(workspace_bytes=1), -5), (dict(workspace=None), -5), (dict(workspace_bytes=0), -5),
    (dict(kind=6, workspace_bytes=4096), -5),                          # enough for the partials, not for the sort
    (dict(B=0), 0), (dict(B=0, scores=None, workspace=None), 0),
    # two at once: kind / dtype, then the lists, then NULL, then the workspace
    (dict(kind=7, B=-1), -3), (dict(rel_dtype=7, L=65537), -3), (dict(L=0, loss=None), -2),
    (dict(L=65537, scores=None), -4), (dict(workspace=None, n=None), -1),
    # at most ltr_max_list_len() documents the call is ltr_pairwise_loss_f32: its checks, no workspace
    (dict(L=16, scores=None, workspace=None), -1), (dict(L=16, kind=9, workspace=None), -3),
]


@pytest.mark.parametrize("i", range(len(CASES)))
def test_return_codes(lib, i):
    change, want = CASES[i]
    args = dict(_VALID, **change)
    assert lib.ltr_pairwise_loss_long_f32(*[args[a] for a in _ARGS]) == want, change


def test_header_matches_the_ctypes_table(lib):
    from pytorchltr_amd import _C
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltr_longpair.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(ltr_[a-z0-9_]+)\s*\(", text))) == sorted(_C.LONGPAIR_SIGNATURES)
    assert not set(_C.LONGPAIR_SIGNATURES) & (set(_C.SIGNATURES) | set(_C.EVAL_SIGNATURES) | set(_C.LISTWISE_SIGNATURES))
    for name in _C.LONGPAIR_SIGNATURES:                                # exported by the library
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr), name
    for name, (_, argtypes) in _C.LONGPAIR_SIGNATURES.items():        # as many arguments as the prototype
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1).strip()
        count = 0 if proto == "void" else len(proto.split(","))
        assert count == len(argtypes), name


def test_python_limits_are_host_logic(lib, monkeypatch):
    """The default module keeps failing fast past max_list_len(), and names the opt-in; the opt-in has a bound of its
    own; fp64 scores keep theirs.  Every case raises before a launch."""
    from pytorchltr_amd import _C, loss as losses
    from pytorchltr_amd._autograd import pairwise_loss_and_grad
    monkeypatch.setattr(_C, "require_device", lambda t, what: None)
    y, n = torch.zeros(1, 5000, dtype=torch.int64), torch.tensor([5000])
    for cls in (losses.PairwiseHingeLoss, losses.PairwiseLogisticLoss, losses.LambdaNDCGLoss2):
        with pytest.raises(ValueError, match="exceeds") as exc:
            cls()(torch.zeros(1, 5000), y, n)
        assert "long_lists=True" in str(exc.value)
    with pytest.raises(ValueError, match="exceeds"):
        pairwise_loss_and_grad(torch.zeros(1, 5000), y, n, _C.HINGE)
    too_long = _C.max_pair_list_len() + 1
    yl, nl = torch.zeros(1, too_long, dtype=torch.int64), torch.tensor([too_long])
    with pytest.raises(ValueError, match=r"max_pair_list_len\(\)"):
        losses.PairwiseHingeLoss(long_lists=True)(torch.zeros(1, too_long), yl, nl)
    with pytest.raises(ValueError, match=r"max_pair_list_len\(\)"):
        pairwise_loss_and_grad(torch.zeros(1, too_long), yl, nl, _C.HINGE, long_lists=True)
    with pytest.raises(ValueError, match="fp64"):                      # fp64 is not part of the long path
        losses.PairwiseHingeLoss(long_lists=True)(torch.zeros(1, 5000, dtype=torch.float64), y, n)
    with pytest.raises(ValueError, match="cfg"):
        pairwise_loss_and_grad(torch.zeros(1, 16), y[:, :16], torch.tensor([16]), _C.HINGE, cfg=(64, 1, 1), long_lists=True)


def test_module_surface():
    import inspect
    from pytorchltr_amd import fused, loss as losses
    from pytorchltr_amd._autograd import LongKind
    names = ("PairwiseHingeLoss", "PairwiseDCGHingeLoss", "PairwiseLogisticLoss", "LambdaARPLoss1", "LambdaARPLoss2",
             "LambdaNDCGLoss1", "LambdaNDCGLoss2")
    for kind, name in enumerate(names):
        cls = getattr(losses, name)
        p = inspect.signature(cls.__init__).parameters["long_lists"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False, name
        assert cls().long_lists is False and cls(long_lists=True).long_lists is True
        assert cls(long_lists=True).state_dict() == {} and list(cls(long_lists=True).parameters()) == []
        with pytest.raises(TypeError):
            cls(1.0, True) if "sigma" in inspect.signature(cls.__init__).parameters else cls(True)
        got, sigma = fused._resolve_loss(cls(long_lists=True))
        assert got == kind and isinstance(got, LongKind) and got.long_lists and sigma == 1.0
        got, _ = fused._resolve_loss(cls())
        assert got == kind and not getattr(got, "long_lists", False)
    # sigma stays the first positional parameter
    assert losses.PairwiseLogisticLoss(2.0, long_lists=True).sigma == 2.0
    assert losses.LambdaNDCGLoss2(0.5, long_lists=True).sigma == 0.5
    assert fused._resolve_loss(losses.LambdaARPLoss2(3.0, long_lists=True)) == (4, 3.0)
    assert not getattr(fused._resolve_loss("hinge")[0], "long_lists", False)
    assert fused._long_pair_shape(fused._resolve_loss(losses.PairwiseHingeLoss(long_lists=True))[0], 4097)
    assert not fused._long_pair_shape(fused._resolve_loss(losses.PairwiseHingeLoss(long_lists=True))[0], 4096)
    assert not fused._long_pair_shape(fused._resolve_loss(losses.PairwiseHingeLoss())[0], 5000)


def test_long_pair_kernels_do_not_spill():
    """tests/test_codeobj.py's rule for the new kernels: no VGPR spill, no scratch."""
    from pytorchltr_amd import _codeobj
    from pytorchltr_amd.build import LIB_PATH, build_extension
    build_extension()
    try:
        recs = _codeobj.kernel_records(LIB_PATH)
    except FileNotFoundError as exc:          # no llvm tools on this machine
        pytest.skip(str(exc))
    ours = [r for r in recs if "longpair_" in r.get("demangled", r["name"])]
    assert len(ours) == 16, [r.get("demangled") for r in ours]         # 7 tile, 7 finish, 2 preparation kernels
    for r in ours:
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, r.get("demangled")
