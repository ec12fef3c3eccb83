"""CPU tier of the fused MLP step of the listwise losses (include/ltr_listwise.h: ltr_mlp_listwise_plan,
ltr_mlp_listwise_f32; pytorchltr_amd/csrc/ltr_mlp_listwise.inc): the C ABI's table, the return codes in the documented
order, the plan rule, the loss names of pytorchltr_amd.fused and the new kernels' register use.  The library is built,
nothing is launched."""
import ctypes
import os
import re

import pytest

LISTNET, LISTMLE = 0, 1
NEW = ("ltr_mlp_listwise_plan", "ltr_mlp_listwise_f32")
KIND_LISTNET, KIND_LISTMLE = 16, 17            # the kernels' KIND values (csrc/ltr_common.inc), outside the pairwise 0..6


@pytest.fixture(scope="module")
def lib():
    from pytorchltr_amd import _C
    from pytorchltr_amd.build import build_extension
    if not os.environ.get("LTR_HIP_LIB"):
        build_extension()
    return _C.lib()


def _header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return open(os.path.join(root, "include", "ltr_listwise.h")).read()


def test_header_table_and_exports(lib):
    from pytorchltr_amd import _C
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(ltr_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared and name in _C.LISTWISE_SIGNATURES and name not in _C.SIGNATURES
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr), name
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(proto.split(",")) == len(_C.LISTWISE_SIGNATURES[name][1]), name
    # the same parameters as ltr_mlp_pairwise_f32, with (loss, k) for (kind, sigma) and the four tie arguments
    assert len(_C.LISTWISE_SIGNATURES["ltr_mlp_listwise_f32"][1]) == len(_C.SIGNATURES["ltr_mlp_pairwise_f32"][1]) + 4


# ---- return codes (no case gets as far as a launch) ----
P = 256                                        # dummy non-NULL, 16-byte aligned device pointer: never dereferenced
_ARGS = ["loss", "k", "X", "W1", "b1", "W2", "b2", "W3", "b3", "rel", "rel_dtype", "n", "tie", "use_seed", "seed",
         "seed_dev", "grad_out", "B", "L", "F", "H1", "H2", "loss_out", "scores_out", "grads", "loss_sum", "workspace",
         "workspace_bytes", "stream"]
_VALID = dict(loss=LISTMLE, k=0, X=P, W1=P, b1=P, W2=P, b2=P, W3=P, b3=P, rel=P, rel_dtype=0, n=P, tie=None, use_seed=0,
              seed=0, seed_dev=None, grad_out=None, B=2, L=16, F=8, H1=5, H2=3, loss_out=P, scores_out=None, grads=P,
              loss_sum=None, workspace=P, workspace_bytes=1 << 30, stream=None)
KIND, SHAPE, TOO_LONG, NULL, WORKSPACE = -3, -2, -4, -1, -5

CASES = [
    (dict(loss=2), KIND), (dict(loss=-1), KIND), (dict(loss=16), KIND), (dict(rel_dtype=7), KIND), (dict(rel_dtype=-1), KIND),
    (dict(B=-1), SHAPE), (dict(L=0), SHAPE), (dict(F=0), SHAPE), (dict(F=6), SHAPE), (dict(F=228), SHAPE),
    (dict(H1=0), SHAPE), (dict(H1=65), SHAPE), (dict(H2=17), SHAPE), (dict(H2=-1), SHAPE),
    (dict(L=257), TOO_LONG), (dict(L=129, F=148), TOO_LONG), (dict(L=1 << 20), TOO_LONG),
    (dict(B=0), 0), (dict(B=0, X=None, grads=None, workspace=None, workspace_bytes=0), 0),
    (dict(X=None), NULL), (dict(W1=None), NULL), (dict(b1=None), NULL), (dict(W2=None), NULL), (dict(b2=None), NULL),
    (dict(W3=None), NULL), (dict(b3=None), NULL), (dict(rel=None), NULL), (dict(n=None), NULL), (dict(loss_out=None), NULL),
    (dict(grads=None), NULL),
    (dict(workspace=None), WORKSPACE), (dict(workspace_bytes=16), WORKSPACE),
    # two at once: kind, then the shape, then the length, then B == 0, then NULL, then the workspace
    (dict(loss=9, B=-1), KIND), (dict(rel_dtype=7, L=0), KIND), (dict(loss=9, X=None), KIND), (dict(rel_dtype=7, L=5000), KIND),
    (dict(B=-1, L=5000), SHAPE), (dict(F=6, X=None), SHAPE), (dict(H1=65, L=300), SHAPE),
    (dict(L=300, X=None), TOO_LONG), (dict(L=300, B=0), TOO_LONG), (dict(L=300, workspace=None), TOO_LONG),
    (dict(X=None, workspace=None), NULL), (dict(n=None, workspace_bytes=0), NULL),
]


@pytest.mark.parametrize("i", range(len(CASES)))
def test_return_codes_in_the_documented_order(lib, i):
    change, want = CASES[i]
    args = dict(_VALID, **change)
    assert lib.ltr_mlp_listwise_f32(*[args[a] for a in _ARGS]) == want, change


def test_return_codes_match_the_pairwise_entry_point_on_shapes(lib):
    """The shape and length rules are those of ltr_mlp_pairwise_f32."""
    for change in (dict(F=6), dict(F=228), dict(H1=65), dict(H2=17), dict(L=257), dict(L=129, F=148), dict(L=0)):
        a = dict(_VALID, **change)
        pair = lib.ltr_mlp_pairwise_f32(0, 1.0, P, P, P, P, P, P, P, P, 0, P, None, a["B"], a["L"], a["F"], a["H1"], a["H2"],
                                        P, None, P, None, P, 1 << 30, None)
        assert pair == lib.ltr_mlp_listwise_f32(*[a[x] for x in _ARGS]) != 0, change


def test_header_states_the_order_of_the_errors():
    text = " ".join(_header().replace("*", " ").split())
    tail = text[text.index("ltr_mlp_listwise_plan: 1 where"):]
    order = [tail.index(w) for w in ("LTR_ERR_KIND", "LTR_ERR_SHAPE", "LTR_ERR_LIST_TOO_LONG", "B == 0 is a no-op",
                                     "LTR_ERR_NULL", "LTR_ERR_WORKSPACE", "LTR_ERR_CONFIG")]
    assert order == sorted(order)


# ---- the plan ----
@pytest.mark.parametrize("loss", [LISTNET, LISTMLE])
def test_plan_accepts_the_longest_list_of_each_layout(lib, loss):
    """The longest list of each layout at its widest row.  The 8-wave kernel at F = 224 keeps 155 792 B of LDS for the
    network; the ranked row of 128 documents is 32 * 128 + 384 = 4480 B: 160 272 of the 163 776 B a workgroup may
    take, so the plan accepts it (ListNet: 8 * 128 + 384 B)."""
    plan = lib.ltr_mlp_listwise_plan
    assert plan(loss, 1, 128, 224, 64, 16) == 1
    assert plan(loss, 1, 256, 144, 64, 16) == 1


@pytest.mark.parametrize("loss", [LISTNET, LISTMLE])
def test_plan(lib, loss):
    plan = lib.ltr_mlp_listwise_plan
    assert plan(loss, 1024, 128, 136, 50, 10) == 1 and plan(loss, 16384, 1, 4, 1, 1) == 1
    assert plan(loss, 1, 256, 80, 64, 16) == 1 and plan(loss, 1, 128, 144, 64, 16) == 1
    assert plan(loss, 1, 257, 136, 50, 10) == 0
    assert plan(loss, 1, 129, 148, 50, 10) == 0 and plan(loss, 1, 128, 148, 50, 10) == 1
    assert plan(loss, 1, 128, 6, 50, 10) == 0
    assert plan(loss, 1, 128, 136, 65, 10) == 0 and plan(loss, 1, 128, 136, 64, 17) == 0
    for bad in ((0, 128, 136, 50, 10), (-1, 128, 136, 50, 10), (1, 0, 136, 50, 10), (1, 128, 0, 50, 10),
                (1, 128, 228, 50, 10), (1, 128, 136, 0, 10), (1, 128, 136, 50, 0)):
        assert plan(loss, *bad) == 0, bad


def test_plan_bad_losses_and_workspace(lib):
    plan = lib.ltr_mlp_listwise_plan
    for loss in (-1, 2, KIND_LISTNET, KIND_LISTMLE):
        assert plan(loss, 1024, 128, 136, 50, 10) == 0
    # the workspace of the pairwise step serves (same grids, same partial vectors)
    assert lib.ltr_mlp_workspace_bytes(1024, 136, 50, 10) >= 4 * lib.ltr_mlp_param_count(136, 50, 10)


# ---- pytorchltr_amd.fused ----
def test_fused_names_and_modules():
    import inspect

    import torch
    from pytorchltr_amd import fused
    from pytorchltr_amd.loss import ListMLELoss, ListwiseSoftmaxLoss, PairwiseHingeLoss
    for name, loss in (("softmax", LISTNET), ("listnet", LISTNET), ("listmle", LISTMLE)):
        m = fused.FusedMLPListwiseLoss(8, loss=name)
        assert isinstance(m.kind, fused._ListwiseKind) and m.kind.loss == loss and m.kind.k is None
    assert fused.FusedMLPListwiseLoss(8).kind.loss == LISTNET                        # the default
    assert fused.FusedMLPListwiseLoss(8, loss=ListwiseSoftmaxLoss()).kind.loss == LISTNET
    m = fused.FusedMLPListwiseLoss(8, loss=ListMLELoss(k=10), hidden=(7, 3), reduction="sum")
    assert m.kind.loss == LISTMLE and m.kind.k == 10 and m.reduction == "sum"
    assert fused.FusedMLPListwiseLoss(8, loss=ListMLELoss()).kind.k is None
    # the same layers and state_dict as FusedMLPLoss, one shared base
    pair = fused.FusedMLPLoss(8, loss="hinge", hidden=(7, 3))
    assert list(m.state_dict()) == list(pair.state_dict()) == ["l1.weight", "l1.bias", "l2.weight", "l2.bias", "l3.weight", "l3.bias"]
    assert [tuple(v.shape) for v in m.state_dict().values()] == [tuple(v.shape) for v in pair.state_dict().values()]
    m.load_state_dict(pair.state_dict())
    assert type(m).__mro__[1] is type(pair).__mro__[1] is not torch.nn.Module
    assert type(m).score is type(pair).score and type(m).forward is type(pair).forward
    assert m.last_losses is None
    sig = inspect.signature(fused.FusedMLPListwiseLoss.__init__).parameters
    assert [(k, v.default) for k, v in list(sig.items())[2:]] == [("loss", "listnet"), ("hidden", (50, 10)), ("reduction", "mean")]
    with pytest.raises(ValueError):
        fused.FusedMLPListwiseLoss(8, reduction="none")
    # each class says where the other family of losses lives
    for bad in ("hinge", PairwiseHingeLoss()):
        with pytest.raises(TypeError, match="FusedMLPLoss"):
            fused.FusedMLPListwiseLoss(8, loss=bad)
    for bad in ("listmle", "listnet", ListMLELoss(k=3)):
        with pytest.raises(TypeError, match="FusedMLPListwiseLoss"):
            fused.FusedMLPLoss(8, loss=bad)
    with pytest.raises(KeyError):
        fused.FusedMLPListwiseLoss(8, loss="no_such_loss")


def test_mlp_listwise_supported_follows_the_plan(lib):
    from pytorchltr_amd import fused
    for loss in (LISTNET, LISTMLE):
        kind = fused._ListwiseKind(loss, 5)
        assert fused.mlp_listwise_supported(kind, 4, 256, 80, 64, 16)
        assert fused.mlp_listwise_supported(kind, 4, 256, 144, 64, 16)
        assert fused.mlp_listwise_supported(kind, 4, 128, 224, 64, 16)
        assert fused.mlp_listwise_supported(kind, 0, 128, 136, 50, 10)                   # an empty batch
        assert not fused.mlp_listwise_supported(kind, 4, 300, 136, 50, 10)
        assert not fused.mlp_listwise_supported(kind, 4, 129, 148, 50, 10)
        assert not fused.mlp_listwise_supported(kind, 4, 128, 46, 50, 10)
        assert not fused.mlp_listwise_supported(kind, 4, 128, 136, 65, 10)
        assert not fused.mlp_listwise_supported(kind, 4, 128, 136, 50, 17)


def test_mlp_loss_step_resolves_the_losses_before_it_needs_a_device():
    """mlp_loss_step takes the listwise names and modules: on CPU tensors the call gets as far as the device check
    (RuntimeError), where on the code before this entry point the loss name itself was refused (TypeError)."""
    import torch
    from pytorchltr_amd import fused
    from pytorchltr_amd.loss import ListMLELoss, ListwiseSoftmaxLoss
    X = torch.zeros(2, 4, 8).double()
    params = [torch.zeros(3, 8), torch.zeros(3), torch.zeros(2, 3), torch.zeros(2), torch.zeros(1, 2), torch.zeros(1)]
    y, n = torch.zeros(2, 4, dtype=torch.int64), torch.tensor([4, 2])
    for loss in ("listnet", "softmax", "listmle", ListwiseSoftmaxLoss(), ListMLELoss(k=2), "hinge"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fused.mlp_loss_step(X, params, y, n, loss=loss)
    with pytest.raises(KeyError):
        fused.mlp_loss_step(X, params, y, n, loss="no_such_loss")


# ---- the code object ----
def test_kernels_are_present_and_do_not_spill():
    from pytorchltr_amd import _codeobj
    from pytorchltr_amd.build import LIB_PATH, build_extension
    build_extension()
    recs = _codeobj.kernel_records(LIB_PATH)     # (needs the llvm tools of the ROCm install: their absence is a failure)
    by_name = {r.get("demangled", r["name"]): r for r in recs}
    tile = {k: [r for n, r in by_name.items() if re.match(r"void mlp_tile_kernel<%d, " % k, n)] for k in (KIND_LISTNET, KIND_LISTMLE, 2)}
    wide = {k: [r for n, r in by_name.items() if re.match(r"void mlp_pairwise_kernel<%d, " % k, n)] for k in (KIND_LISTNET, KIND_LISTMLE, 2)}
    for k in (KIND_LISTNET, KIND_LISTMLE):
        # as many instantiations as the pairwise logistic kind (2) has: feature buckets x list-length classes
        assert len(tile[k]) == len(tile[2]) == 8, sorted(by_name)
        assert len(wide[k]) == len(wide[2]) == 4
        for r in tile[k] + wide[k]:
            name = r.get("demangled")
            assert r.get("vgpr_spill_count", 0) == 0, name
            assert r.get("private_segment_fixed_size", 0) == 0, name
        # the tile kernel keeps two workgroups (of four waves) per CU: <= 256 registers per wave, arch + accumulation
        for r in tile[k]:
            assert r["vgpr_count"] + r.get("agpr_count", 0) <= 256, r.get("demangled")
            assert r["max_flat_workgroup_size"] == 256
        for r in wide[k]:
            assert r["vgpr_count"] + r.get("agpr_count", 0) <= 256 and r["max_flat_workgroup_size"] == 512, r.get("demangled")
    # the pinned pairwise instantiation keeps its name (tests/test_codeobj.py)
    assert "void mlp_tile_kernel<0, 9, 34, 128, false, false>(MlpParams)" in by_name
