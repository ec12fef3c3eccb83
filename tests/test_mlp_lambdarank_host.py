"""CPU tier of the fused MLP step of LambdaRankLoss (include/ltr_mlp_lambdarank.h: ltr_mlp_lambdarank_plan,
ltr_mlp_lambdarank_f32; the slot: mlp_lambdarank_slot in pytorchltr_amd/csrc/ltr_mlp_listwise.inc): the C ABI's table,
the return codes in the documented order, the plan rule, the new kernels' register use and the names of
pytorchltr_amd.fused.  The library is built, nothing is launched."""
import ctypes
import os
import re

import pytest

NEW = ("ltr_mlp_lambdarank_plan", "ltr_mlp_lambdarank_f32")
KIND_LAMBDARANK = 18                           # the kernels' KIND value (csrc/ltr_common.inc), beside 16 and 17


@pytest.fixture(scope="module")
def lib():
    from pytorchltr_amd import _C
    from pytorchltr_amd.build import build_extension
    if not os.environ.get("LTR_HIP_LIB"):
        build_extension()
    return _C.lib()


def _root():
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(_root(), "include", "ltr_mlp_lambdarank.h")).read()


# ---- the ABI table ----
def test_header_table_and_exports(lib):
    from pytorchltr_amd import _C, build
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(ltr_[a-z0-9_]+)\s*\(", text))
    assert declared == set(_C.MLP_LAMBDARANK_SIGNATURES) == set(NEW)
    others = [v for k, v in vars(_C).items() if k.endswith("SIGNATURES") and k != "MLP_LAMBDARANK_SIGNATURES"]
    assert len(others) >= 10
    for name in NEW:
        assert not any(name in table for table in others), name
        fn = getattr(lib, name)
        assert isinstance(fn, ctypes._CFuncPtr), name
        restype, argtypes = _C.MLP_LAMBDARANK_SIGNATURES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(proto.split(",")) == len(argtypes), name
    # the parameters of ltr_mlp_pairwise_f32, with (k, sigma) for (kind, sigma)
    assert _C.MLP_LAMBDARANK_SIGNATURES["ltr_mlp_lambdarank_f32"][1] == _C.SIGNATURES["ltr_mlp_pairwise_f32"][1]
    assert lib.ltr_version() == 114
    assert os.path.join(_root(), "include", "ltr_mlp_lambdarank.h") in build.DEPENDS


# ---- return codes (no case gets as far as a launch) ----
P = 256                                        # dummy non-NULL, 16-byte aligned device pointer: never dereferenced
_ARGS = ["k", "sigma", "X", "W1", "b1", "W2", "b2", "W3", "b3", "rel", "rel_dtype", "n", "grad_out", "B", "L", "F", "H1",
         "H2", "loss_out", "scores_out", "grads", "loss_sum", "workspace", "workspace_bytes", "stream"]
_VALID = dict(k=10, sigma=1.0, X=P, W1=P, b1=P, W2=P, b2=P, W3=P, b3=P, rel=P, rel_dtype=0, n=P, grad_out=None, B=2,
              L=16, F=8, H1=5, H2=3, loss_out=P, scores_out=None, grads=P, loss_sum=None, workspace=P,
              workspace_bytes=1 << 30, stream=None)
KIND, SHAPE, TOO_LONG, NULL, WORKSPACE = -3, -2, -4, -1, -5
INF, NAN = float("inf"), float("nan")

CASES = [
    (dict(rel_dtype=7), KIND), (dict(rel_dtype=-1), KIND), (dict(rel_dtype=3), KIND),
    (dict(B=-1), SHAPE), (dict(L=0), SHAPE), (dict(F=0), SHAPE), (dict(F=6), SHAPE), (dict(F=228), SHAPE),
    (dict(H1=0), SHAPE), (dict(H1=65), SHAPE), (dict(H2=17), SHAPE), (dict(H2=-1), SHAPE),
    (dict(L=257), TOO_LONG), (dict(L=129, F=148), TOO_LONG), (dict(L=1 << 20), TOO_LONG),
    (dict(B=0), 0), (dict(B=0, X=None, grads=None, workspace=None, workspace_bytes=0), 0),
    (dict(X=None), NULL), (dict(W1=None), NULL), (dict(b1=None), NULL), (dict(W2=None), NULL), (dict(b2=None), NULL),
    (dict(W3=None), NULL), (dict(b3=None), NULL), (dict(rel=None), NULL), (dict(n=None), NULL), (dict(loss_out=None), NULL),
    (dict(grads=None), NULL),
    (dict(workspace=None), WORKSPACE), (dict(workspace_bytes=16), WORKSPACE),
    # two at once: the label dtype, then the shape, then the length, then B == 0, then NULL, then the workspace
    (dict(rel_dtype=7, B=-1), KIND), (dict(rel_dtype=7, L=0), KIND), (dict(rel_dtype=7, X=None), KIND),
    (dict(rel_dtype=7, L=5000), KIND), (dict(rel_dtype=7, sigma=NAN), KIND),
    (dict(B=-1, L=5000), SHAPE), (dict(F=6, X=None), SHAPE), (dict(H1=65, L=300), SHAPE), (dict(sigma=INF, L=300), SHAPE),
    (dict(L=300, X=None), TOO_LONG), (dict(L=300, B=0), TOO_LONG), (dict(L=300, workspace=None), TOO_LONG),
    (dict(X=None, workspace=None), NULL), (dict(n=None, workspace_bytes=0), NULL),
]


@pytest.mark.parametrize("i", range(len(CASES)))
def test_return_codes_in_the_documented_order(lib, i):
    change, want = CASES[i]
    args = dict(_VALID, **change)
    assert lib.ltr_mlp_lambdarank_f32(*[args[a] for a in _ARGS]) == want, change


@pytest.mark.parametrize("sigma", [INF, -INF, NAN, 0.0, -1.0])
def test_sigma_is_judged_as_the_stand_alone_entry_point_judges_it(lib, sigma):
    """A sigma ltr_lambdarank_f32 refuses is refused with its code; one it lets through (no launch here: B == 0) passes."""
    alone = lib.ltr_lambdarank_f32(P, P, 0, P, 10, sigma, 0, 16, P, None, None)
    assert lib.ltr_mlp_lambdarank_f32(*[dict(_VALID, sigma=sigma, B=0)[a] for a in _ARGS]) == alone
    assert alone == (0 if sigma in (0.0, -1.0) else SHAPE)
    if alone != 0:                                # ... and ahead of the NULL and workspace checks of a real batch
        assert lib.ltr_mlp_lambdarank_f32(*[dict(_VALID, sigma=sigma, X=None, workspace=None)[a] for a in _ARGS]) == alone


def test_return_codes_match_the_listwise_entry_point_on_shapes(lib):
    """The shape and length rules are those of ltr_mlp_listwise_f32."""
    for change in (dict(F=6), dict(F=228), dict(H1=65), dict(H2=17), dict(L=257), dict(L=129, F=148), dict(L=0), dict(B=-1)):
        a = dict(_VALID, **change)
        lw = lib.ltr_mlp_listwise_f32(1, 0, P, P, P, P, P, P, P, P, 0, P, None, 0, 0, None, None, a["B"], a["L"], a["F"],
                                      a["H1"], a["H2"], P, None, P, None, P, 1 << 30, None)
        assert lw == lib.ltr_mlp_lambdarank_f32(*[a[x] for x in _ARGS]) != 0, change


def test_header_states_the_order_of_the_errors():
    text = " ".join(_header().replace("*", " ").split())
    tail = text[text.index("ltr_mlp_lambdarank_plan: 1 where"):]
    order = [tail.index(w) for w in ("LTR_ERR_KIND", "LTR_ERR_SHAPE", "LTR_ERR_LIST_TOO_LONG", "B == 0 is a no-op",
                                     "LTR_ERR_NULL", "LTR_ERR_WORKSPACE", "LTR_ERR_CONFIG")]
    assert order == sorted(order)


# ---- the plan ----
def test_plan_grid(lib):
    """L <= 256 for F <= 144 (the tile layout), L <= 128 above, F <= 224: the rule of ltr_mlp_listwise_plan."""
    plan = lib.ltr_mlp_lambdarank_plan
    for F in (136, 144, 148, 224, 228):
        for L in (128, 129, 256, 257):
            want = 1 if (F <= 224 and L <= (256 if F <= 144 else 128)) else 0
            assert plan(4, L, F, 50, 10) == plan(4, L, F, 64, 16) == want, (L, F)
            assert want == lib.ltr_mlp_listwise_plan(1, 4, L, F, 50, 10), (L, F)          # ListMLE: the same row
    for F in (6, 135, 137, 138):
        assert plan(4, 128, F, 50, 10) == 0, F
    assert plan(4, 128, 136, 65, 10) == 0 and plan(4, 128, 136, 64, 17) == 0
    assert plan(1024, 128, 136, 50, 10) == 1 and plan(16384, 1, 4, 1, 1) == 1
    for bad in ((0, 128, 136, 50, 10), (-1, 128, 136, 50, 10), (1, 0, 136, 50, 10), (1, 128, 0, 50, 10),
                (1, 128, 136, 0, 10), (1, 128, 136, 50, 0)):
        assert plan(*bad) == 0, bad


def test_the_listwise_entry_points_still_refuse_loss_code_2(lib):
    assert lib.ltr_mlp_listwise_plan(2, 1024, 128, 136, 50, 10) == 0
    assert lib.ltr_mlp_listwise_plan(KIND_LAMBDARANK, 1024, 128, 136, 50, 10) == 0
    assert lib.ltr_mlp_listwise_f32(2, 0, P, P, P, P, P, P, P, P, 0, P, None, 0, 0, None, None, 2, 16, 8, 5, 3, P, None, P,
                                    None, P, 1 << 30, None) == KIND
    # ... and the pairwise one the internal kind
    assert lib.ltr_mlp_pairwise_f32(KIND_LAMBDARANK, 1.0, P, P, P, P, P, P, P, P, 0, P, None, 2, 16, 8, 5, 3, P, None, P,
                                    None, P, 1 << 30, None) == KIND


# ---- the code object ----
def test_kernels_are_present_and_do_not_spill():
    from pytorchltr_amd import _codeobj
    from pytorchltr_amd.build import LIB_PATH, build_extension
    build_extension()
    recs = _codeobj.kernel_records(LIB_PATH)     # (needs the llvm tools of the ROCm install: their absence is a failure)
    by_name = {r.get("demangled", r["name"]): r for r in recs}
    tile = [r for n, r in by_name.items() if re.match(r"void mlp_tile_kernel<%d, " % KIND_LAMBDARANK, n)]
    wide = [r for n, r in by_name.items() if re.match(r"void mlp_pairwise_kernel<%d, " % KIND_LAMBDARANK, n)]
    # feature buckets x list-length classes, as the other listwise kinds have them
    assert len(tile) == 8 and len(wide) == 4, sorted(by_name)
    for r in tile + wide:
        name = r.get("demangled")
        assert r.get("vgpr_spill_count", 0) == 0, name
        assert r.get("private_segment_fixed_size", 0) == 0, name
        assert r["vgpr_count"] + r.get("agpr_count", 0) <= 256, name
    # the tile kernel keeps two workgroups (of four waves) per CU
    assert all(r["max_flat_workgroup_size"] == 256 for r in tile)
    assert all(r["max_flat_workgroup_size"] == 512 for r in wide)
    # the pinned pairwise instantiation keeps its name (tests/test_codeobj.py)
    assert "void mlp_tile_kernel<0, 9, 34, 128, false, false>(MlpParams)" in by_name


# ---- pytorchltr_amd.fused ----
def test_the_class_takes_sigma_and_k_or_the_module():
    import inspect

    import torch
    from pytorchltr_amd import _C, fused
    from pytorchltr_amd.loss import LambdaRankLoss, ListMLELoss, PairwiseHingeLoss
    m = fused.FusedMLPLambdaRankLoss(8)
    assert isinstance(m.kind, fused._ListwiseKind) and m.kind == (_C.LISTWISE_LAMBDARANK, None) and m.sigma == 1.0
    m = fused.FusedMLPLambdaRankLoss(8, sigma=2.5, k=10.0, hidden=(7, 3), reduction="sum")
    assert m.kind == (_C.LISTWISE_LAMBDARANK, 10) and isinstance(m.kind.k, int) and m.sigma == 2.5 and m.reduction == "sum"
    by_module = fused.FusedMLPLambdaRankLoss(8, loss=LambdaRankLoss(sigma=0.5, k=3), sigma=9.0, k=99)
    assert by_module.kind == (_C.LISTWISE_LAMBDARANK, 3) and by_module.sigma == 0.5       # the module supplies both
    sig = inspect.signature(fused.FusedMLPLambdaRankLoss.__init__).parameters
    assert [(k, v.default) for k, v in list(sig.items())[2:]] == [("loss", None), ("sigma", 1.0), ("k", None),
                                                                  ("hidden", (50, 10)), ("reduction", "mean")]
    # k as LambdaRankLoss checks it, reduction as the base class does
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            fused.FusedMLPLambdaRankLoss(8, k=bad)
        with pytest.raises(ValueError):
            fused.mlp_lambdarank_step(None, None, None, None, k=bad)
    with pytest.raises(ValueError):
        fused.FusedMLPLambdaRankLoss(8, reduction="none")
    for bad in ("lambdarank", "hinge", "listmle", PairwiseHingeLoss(), ListMLELoss(k=3), 7):
        with pytest.raises(TypeError, match="FusedMLPLambdaRankLoss"):
            fused.FusedMLPLambdaRankLoss(8, loss=bad)
    # the same layers and state_dict as FusedMLPLoss, one shared base
    pair = fused.FusedMLPLoss(8, loss="hinge", hidden=(7, 3))
    assert list(m.state_dict()) == list(pair.state_dict()) == ["l1.weight", "l1.bias", "l2.weight", "l2.bias", "l3.weight", "l3.bias"]
    m.load_state_dict(pair.state_dict())
    assert type(m).__mro__[1] is type(pair).__mro__[1] is fused._FusedMLPBase is not torch.nn.Module
    assert type(m).score is type(pair).score and type(m).forward is type(pair).forward
    assert m.last_losses is None


def test_the_four_older_entry_points_still_refuse_lambdarank():
    from pytorchltr_amd import fused
    from pytorchltr_amd.loss import LambdaRankLoss
    for make in (lambda: fused.FusedMLPLoss(8, loss="lambdarank"), lambda: fused.FusedMLPLoss(8, loss=LambdaRankLoss(k=5)),
                 lambda: fused.FusedMLPListwiseLoss(8, loss="lambdarank"),
                 lambda: fused.FusedMLPListwiseLoss(8, loss=LambdaRankLoss()),
                 lambda: fused.mlp_loss_step(None, None, None, None, loss="lambdarank"),
                 lambda: fused.mlp_loss_step(None, None, None, None, loss=LambdaRankLoss(k=5)),
                 lambda: fused.LazySGD(None, None, 0.1, loss="lambdarank")):
        with pytest.raises(TypeError):
            make()
    # two of them name the new entry points
    with pytest.raises(TypeError, match="mlp_lambdarank_step"):
        fused.mlp_loss_step(None, None, None, None, loss="lambdarank")
    with pytest.raises(TypeError, match="FusedMLPLambdaRankLoss"):
        fused.FusedMLPListwiseLoss(8, loss="lambdarank")


def test_mlp_lambdarank_step_needs_a_device(lib):
    import torch
    from pytorchltr_amd import fused
    X = torch.zeros(2, 4, 8).double()
    params = [torch.zeros(3, 8), torch.zeros(3), torch.zeros(2, 3), torch.zeros(2), torch.zeros(1, 2), torch.zeros(1)]
    y, n = torch.zeros(2, 4, dtype=torch.int64), torch.tensor([4, 2])
    for kw in (dict(), dict(k=10), dict(sigma=2.5, k=1)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fused.mlp_lambdarank_step(X, params, y, n, **kw)
    m = fused.FusedMLPLambdaRankLoss(8, k=10, hidden=(3, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(X.float(), y, n)


def test_mlp_lambdarank_supported_follows_the_plan(lib):
    from pytorchltr_amd import fused
    assert fused.mlp_lambdarank_supported(4, 256, 80, 64, 16)
    assert fused.mlp_lambdarank_supported(4, 256, 144, 64, 16)
    assert fused.mlp_lambdarank_supported(4, 128, 224, 64, 16)
    assert fused.mlp_lambdarank_supported(0, 128, 136, 50, 10)                       # an empty batch
    assert not fused.mlp_lambdarank_supported(4, 300, 136, 50, 10)
    assert not fused.mlp_lambdarank_supported(4, 129, 148, 50, 10)
    assert not fused.mlp_lambdarank_supported(4, 128, 46, 50, 10)
    assert not fused.mlp_lambdarank_supported(4, 128, 136, 65, 10)
    assert not fused.mlp_lambdarank_supported(4, 128, 136, 50, 17)
    # the routes: the fused step on the plan, the rows off it
    kind = fused._ListwiseKind(2, 10)
    import torch
    args = ("step", torch.float32, 3, True, False, True, False)
    assert fused._mlp_route(*args, 128, 136, 50, 10, kind, True) is fused._FUSED
    assert fused._mlp_route(*args, 300, 136, 50, 10, kind, False) is fused._ROWS
