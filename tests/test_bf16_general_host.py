"""CPU tier of the general fused Linear step on bf16 batches (include/ltr_bf16_general.h; fused._linear_route's opt-in
route): the boundary, the plan, the order of the argument errors, the route on plain values, the code objects.  No launch."""
import ctypes
import os
import re

import pytest
import torch

P = 256                                        # dummy non-NULL, 16-byte aligned device pointer: never dereferenced below
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_NULL, ERR_SHAPE, ERR_KIND, ERR_TOO_LONG, ERR_CONFIG = 0, -1, -2, -3, -4, -6
KINDS = range(7)


@pytest.fixture(scope="module")
def lib():
    from pytorchltr_amd import _C
    from pytorchltr_amd.build import build_extension
    if not os.environ.get("LTR_HIP_LIB"):
        build_extension()
    return _C.lib()


def _partials(lib, kind=0, B=2, L=10, F=8, X=P, W=P, rel=P, rel_dtype=0, n=P, loss=P, part=P):
    return lib.ltr_bf16_general_linear_partials(kind, 1.0, X, W, P, rel, rel_dtype, n, B, L, F, loss, None, part, None)


def test_header_exports_and_ctypes_table_agree(lib):
    from pytorchltr_amd import _C
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltr_bf16_general.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(ltr_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_C.BF16_GENERAL_SIGNATURES) == ["ltr_bf16_general_linear_partials", "ltr_bf16_general_linear_plan"]
    for name, (_, argtypes) in _C.BF16_GENERAL_SIGNATURES.items():
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr), name          # exported by the library
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1).strip()
        assert len(proto.split(",")) == len(argtypes), name                     # as many arguments as the prototype
    # argument for argument the register tile's prototypes
    assert list(_C.BF16_GENERAL_SIGNATURES.values()) == [_C.LINEAR_BF16_SIGNATURES[k] for k in ("ltr_linear_bf16_plan", "ltr_linear_partials_bf16")]


@pytest.mark.parametrize("kind", KINDS)
def test_plan_on_each_side_of_each_limit(lib, kind):
    plan = lib.ltr_bf16_general_linear_plan
    assert [plan(kind, 4, 300, F) for F in (8, 12, 1024, 1032)] == [1, 0, 1, 0]
    # (LambdaNDCG2's pair pass keeps 36 bytes of LDS per document: its block ends at 4084 documents at F = 8, 3884 at 1024)
    top = 4084 if kind == 6 else 4096
    assert [plan(kind, 4, L, 8) for L in (0, 1, top, top + 1, 4097)] == [0, 1, 1, int(kind != 6) * int(top < 4096), 0]
    assert plan(kind, 4, 3884, 1024) == 1 and plan(kind, 4, 3885, 1024) == int(kind != 6)
    assert plan(kind, 0, 300, 8) == 0 and plan(7, 4, 300, 8) == 0 and plan(-1, 4, 300, 8) == 0
    # the shapes the register tile refuses, and the ones it takes as well
    assert all(plan(kind, 384, L, F) == 1 for L, F in ((257, 136), (81, 704), (1000, 224), (1251, 136), (5, 8), (128, 136)))


def test_return_codes_in_the_house_order(lib):
    every = dict(X=None, W=None, rel=None, n=None, loss=None, part=None)
    assert _partials(lib, kind=7, F=12, **every) == ERR_KIND                # the kind in front of the shape
    assert _partials(lib, rel_dtype=3, L=5000, **every) == ERR_KIND
    for bad in (dict(F=12), dict(F=1032), dict(F=0), dict(L=0), dict(B=-1), dict(B=1 << 20, L=1 << 12)):
        assert _partials(lib, **bad, **every) == ERR_SHAPE, bad
    assert _partials(lib, L=5000, F=12, **every) == ERR_SHAPE               # the shape in front of the length
    assert _partials(lib, L=4097, **every) == ERR_TOO_LONG                  # the length in front of the pointers
    # (off the plan by its LDS block alone: LambdaNDCG2's pair pass on the longest lists)
    assert _partials(lib, kind=6, B=0, L=4096, F=1024, **every) == ERR_CONFIG      # the plan in front of the empty batch
    assert _partials(lib, B=0, **every) == OK                               # the empty batch in front of the pointers
    for bad in (dict(X=None), dict(W=None), dict(rel=None), dict(n=None), dict(loss=None), dict(part=None)):
        assert _partials(lib, L=300, F=136, **bad) == ERR_NULL, bad


def test_the_flag_turns_the_refused_shapes_to_the_general_step(lib):
    from pytorchltr_amd import _C, fused
    from pytorchltr_amd._autograd import LongKind
    bf = torch.bfloat16
    route = fused._linear_route
    for kind in KINDS:
        for caller in ("step", "module"):
            # bf16-F136-L257 and bf16-F704-L81 of tests/test_linear_routes_host.py, and a feature count padded to 8
            for B, L, F in ((3, 257, 136), (3, 81, 704), (384, 1000, 220)):
                assert route(caller, bf, 3, True, False, False, kind, B, L, F, cus=1, bf16_general=True) \
                    == fused._LIN_BF16_GENERAL, (kind, caller, B, L, F)
            # what the register tile takes stays its own, a long list past max_list_len() the pieces'
            assert route(caller, bf, 3, True, False, False, kind, 3, 256, 136, cus=1, bf16_general=True) == fused._LIN_BF16_FUSED
            assert route(caller, bf, 3, True, False, False, LongKind(kind), 2, _C.max_list_len() + 4, 8, cus=1,
                         bf16_general=True) == fused._LIN_BF16_PIECES
    # the module callers keep the pieces where _prefer_pieces prefers them (a few long lists on a big device); the step does not
    assert route("module", bf, 3, True, False, False, 0, 32, 1000, 224, cus=256, bf16_general=True) == fused._LIN_BF16_PIECES
    assert route("step", bf, 3, True, False, False, 0, 32, 1000, 224, cus=256, bf16_general=True) == fused._LIN_BF16_GENERAL
    # the listwise kinds have no such kernel
    listnet = fused._ListwiseKind(_C.LISTWISE_LISTNET)
    assert route("step", bf, 3, True, False, False, listnet, 4, 300, 8, cus=1, bf16_general=True) == fused._LIN_BF16_PIECES
    assert fused._LIN_PARTIALS[fused._LIN_BF16_GENERAL] in _C.BF16_GENERAL_SIGNATURES
    assert fused.FusedLinearLoss(8, "hinge", bf16_general=True).bf16_general and not fused.FusedLinearLoss(8).bf16_general


def test_general_kernels_keep_their_occupancy_and_nothing_in_scratch():
    from pytorchltr_amd import _codeobj
    from pytorchltr_amd.build import build_extension
    try:
        recs = _codeobj.kernel_records(build_extension())
    except FileNotFoundError as exc:          # no llvm tools on this machine
        pytest.skip(str(exc))
    found = [(re.search(r"bf16_general_linear_kernel<(\d), (\d)>", r.get("demangled", r["name"])), r) for r in recs]
    ours = {(int(m.group(1)), int(m.group(2))): r for m, r in found if m}
    assert sorted(ours) == [(k, d) for k in KINDS for d in (0, 1, 4)]
    for (kind, dpt), r in ours.items():
        # csrc/ltr_linear_bf16_general.inc, lbg_waves, as VGPR caps: 512 / waves per SIMD, in eights
        cap = 128 if dpt == 4 else (96 if (kind, dpt) == (6, 1) else 80)
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, (kind, dpt, r)
        assert 0 < r["vgpr_count"] + r.get("agpr_count", 0) <= cap, (kind, dpt, r)
