"""CPU tier of the fused Linear step of the listwise losses (include/ltr_listwise.h: ltr_linear_listwise_plan,
ltr_linear_listwise_partials_f32; pytorchltr_amd/csrc/ltr_linear_listwise.inc): the C ABI's table, the return codes in
the documented order, the plan rule, the loss names of pytorchltr_amd.fused and the new kernels' register use.  The
library is built, nothing is launched."""
import ctypes
import os
import re

import pytest

LISTNET, LISTMLE = 0, 1
NEW = ("ltr_linear_listwise_plan", "ltr_linear_listwise_partials_f32")
N_KERNELS = 7                                  # ListNet: one instantiation; ListMLE: the six launch shapes of the core


@pytest.fixture(scope="module")
def lib():
    from pytorchltr_amd import _C
    from pytorchltr_amd.build import build_extension
    if not os.environ.get("LTR_HIP_LIB"):
        build_extension()
    return _C.lib()


def test_header_table_and_exports(lib):
    from pytorchltr_amd import _C
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "ltr_listwise.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ltr_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared and name in _C.LISTWISE_SIGNATURES and name not in _C.SIGNATURES
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr), name
    # the prototype's parameters, counted, against the ctypes table
    for name in NEW:
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(proto.split(",")) == len(_C.LISTWISE_SIGNATURES[name][1]), name
    assert re.search(r"LTR_LISTWISE_LISTNET\s*=\s*0\s*,\s*LTR_LISTWISE_LISTMLE\s*=\s*1", text)
    assert (_C.LISTWISE_LISTNET, _C.LISTWISE_LISTMLE) == (LISTNET, LISTMLE)


# ---- return codes (no case gets as far as a launch) ----
P = 256                                        # dummy non-NULL, 16-byte aligned device pointer: never dereferenced
_ARGS = ["loss", "k", "X", "W", "bias", "rel", "rel_dtype", "n", "tie", "use_seed", "seed", "seed_dev", "B", "L", "F",
         "loss_out", "scores_out", "partials", "stream"]
_VALID = dict(loss=LISTMLE, k=0, X=P, W=P, bias=None, rel=P, rel_dtype=0, n=P, tie=None, use_seed=0, seed=0,
              seed_dev=None, B=2, L=16, F=8, loss_out=P, scores_out=None, partials=P, stream=None)
KIND, SHAPE, TOO_LONG, NULL, CONFIG = -3, -2, -4, -1, -6

CASES = [
    (dict(loss=2), KIND), (dict(loss=-1), KIND), (dict(rel_dtype=7), KIND), (dict(rel_dtype=-1), KIND),
    (dict(B=-1), SHAPE), (dict(L=0), SHAPE), (dict(L=-3), SHAPE), (dict(F=0), SHAPE), (dict(F=-4), SHAPE),
    (dict(L=4097), TOO_LONG), (dict(L=1 << 20), TOO_LONG),
    (dict(B=0), 0), (dict(B=0, X=None, partials=None), 0), (dict(B=0, F=5), 0),
    (dict(X=None), NULL), (dict(W=None), NULL), (dict(rel=None), NULL), (dict(n=None), NULL), (dict(loss_out=None), NULL),
    (dict(partials=None), NULL),
    (dict(F=5), CONFIG), (dict(F=46), CONFIG), (dict(X=P + 4), CONFIG), (dict(partials=P + 8), CONFIG),
    (dict(loss=LISTNET, F=6), CONFIG),
    # two at once: kind, then the shape, then the length, then B == 0, then NULL, then the plan
    (dict(loss=9, B=-1), KIND), (dict(rel_dtype=7, L=0), KIND), (dict(loss=9, X=None), KIND), (dict(rel_dtype=7, L=5000), KIND),
    (dict(B=-1, L=5000), SHAPE), (dict(F=0, X=None), SHAPE), (dict(L=0, F=5), SHAPE),
    (dict(L=5000, X=None), TOO_LONG), (dict(L=5000, F=5), TOO_LONG), (dict(L=5000, B=0), TOO_LONG),
    (dict(X=None, F=5), NULL), (dict(n=None, X=P + 4), NULL),
]


@pytest.mark.parametrize("i", range(len(CASES)))
def test_return_codes_in_the_documented_order(lib, i):
    change, want = CASES[i]
    args = dict(_VALID, **change)
    assert lib.ltr_linear_listwise_partials_f32(*[args[a] for a in _ARGS]) == want, change


def test_header_states_the_order_of_the_errors():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = " ".join(open(os.path.join(root, "include", "ltr_listwise.h")).read().replace("*", " ").split())
    tail = text[text.index("ltr_linear_listwise_plan: 1 where"):]
    order = [tail.index(w) for w in ("LTR_ERR_KIND", "LTR_ERR_SHAPE", "LTR_ERR_LIST_TOO_LONG", "B == 0 is a no-op",
                                     "LTR_ERR_NULL", "LTR_ERR_CONFIG", "sticky device status")]
    assert order == sorted(order)


# ---- the plan ----
def test_plan(lib):
    plan = lib.ltr_linear_listwise_plan
    assert lib.ltr_max_list_len() == 4096
    for loss in (LISTNET, LISTMLE):
        for shape in ((1024, 128, 136), (6, 4096, 700), (1, 1, 4)):
            assert plan(loss, *shape) == 1, (loss, shape)
        assert plan(loss, 6, 4097, 136) == 0
        assert plan(loss, 6, 128, 5) == 0 and plan(loss, 6, 128, 46) == 0
        for bad in ((0, 128, 136), (-1, 128, 136), (6, 0, 136), (6, -2, 136), (6, 128, 0), (6, 128, -4)):
            assert plan(loss, *bad) == 0, bad
        # a row whose weights alone are past the LDS left behind the longest ranked row
        assert plan(loss, 6, 4096, 1 << 16) == 0
    for loss in (-1, 2, 100):
        assert plan(loss, 1024, 128, 136) == 0


def test_the_partial_rows_fit_the_linear_workspace(lib):
    for B, L, F in ((1, 1, 4), (6, 4096, 700), (1024, 128, 136), (16384, 100, 8)):
        assert lib.ltr_linear_workspace_bytes(B, L, F) >= 4 * B * ((F + 4) & ~3)


# ---- pytorchltr_amd.fused ----
def test_resolve_loss_takes_the_listwise_names_and_modules():
    import torch
    from pytorchltr_amd import fused
    from pytorchltr_amd.loss import ListMLELoss, ListwiseSoftmaxLoss, PairwiseHingeLoss
    for name, loss in (("softmax", LISTNET), ("listnet", LISTNET), ("listmle", LISTMLE)):
        kind, sigma = fused._resolve_loss(name)
        assert isinstance(kind, fused._ListwiseKind) and kind.loss == loss and kind.k is None and sigma == 1.0
    kind, _ = fused._resolve_loss(ListwiseSoftmaxLoss())
    assert isinstance(kind, fused._ListwiseKind) and kind.loss == LISTNET
    kind, _ = fused._resolve_loss(ListMLELoss(k=10))
    assert kind.loss == LISTMLE and kind.k == 10
    assert fused._resolve_loss(ListMLELoss())[0].k is None
    assert fused.FusedLinearLoss(8, loss=ListMLELoss(k=3)).kind.k == 3
    assert fused.FusedLinearLoss(8, loss="listnet").kind.loss == LISTNET
    # the pairwise kinds as before
    assert fused._resolve_loss("hinge") == (0, 1.0) and fused._resolve_loss(PairwiseHingeLoss())[0] == 0
    assert not isinstance(fused._resolve_loss("hinge")[0], fused._ListwiseKind)
    for bad in (3, None, torch.nn.MSELoss(), object()):
        with pytest.raises(TypeError):
            fused._resolve_loss(bad)
    with pytest.raises(KeyError):
        fused._resolve_loss("no_such_loss")
    # the entry points without a listwise kernel say so
    with pytest.raises(TypeError):
        fused.FusedMLPLoss(8, loss="listmle")


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
    ours = [r for r, n in zip(recs, names) if "linear_listwise_kernel" in n]
    assert len(ours) == N_KERNELS, [n for n in names if "linear_listwise" in n]
    for r in ours:
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, r.get("demangled")
        # launched with up to 1024 threads: two workgroups per CU need <= 64 VGPRs and <= 80 SGPRs on the sort shapes
        # and for ListNet (DPT <= 0); the counting-rank shapes keep the core's budget of 128
        dpt = int(re.search(r"linear_listwise_kernel<\d+, (-?\d+)>", r.get("demangled", r["name"])).group(1))
        assert r["vgpr_count"] <= (64 if dpt <= 0 else 128), r.get("demangled")
        if dpt <= 0:
            assert r["sgpr_count"] <= 80, r.get("demangled")
    # the twelve kernels of ListMLE are still the only ones named after it (tests/test_listmle_host.py counts them)
    listmle = [n for n in names if "listmle_" in n]
    assert len(listmle) == 11 and not [n for n in listmle if "linear_listwise" in n], listmle
