"""CPU tier of the MLP scorer on wide bf16 rows (include/ltr_mlp_widebf16.h, fused.mlp_wide_scores_bf16 /
fused.mlp_wide_grad_bf16): the boundary, the argument errors (decided on the host, in front of any launch), the code
objects and the opt-in route.  Nothing here gets as far as a launch."""
import ctypes
import os
import re

import pytest
import torch

P = 256                                        # dummy non-NULL device pointer: never dereferenced below
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_NULL, ERR_SHAPE, ERR_WORKSPACE = 0, -1, -2, -5


@pytest.fixture(scope="module")
def lib():
    from pytorchltr_amd import _C
    from pytorchltr_amd.build import build_extension
    if not os.environ.get("LTR_HIP_LIB"):
        build_extension()
    return _C.lib()


def test_header_exports_and_ctypes_table_agree(lib):
    import subprocess
    from pytorchltr_amd import _C, _codeobj
    from pytorchltr_amd.build import LIB_PATH
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltr_mlp_widebf16.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(ltr_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_C.MLP_WIDEBF16_SIGNATURES) and len(declared) == 3
    out = subprocess.run([_codeobj._tool("llvm-readelf"), "--dyn-syms", "-W", LIB_PATH], check=True,
                         stdout=subprocess.PIPE).stdout.decode()
    defined = "\n".join(ln for ln in out.splitlines() if " FUNC " in ln and " GLOBAL " in ln and " UND " not in ln)
    assert sorted(set(re.findall(r"\b(ltr_mlp_widebf16_[a-z0-9_]+)\b", defined))) == declared
    wide = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltr_mlp_wide.h")).read(), flags=re.S)
    for ours, theirs in (("ltr_mlp_widebf16_scores", "ltr_mlp_wide_scores_f32"),
                         ("ltr_mlp_widebf16_grad", "ltr_mlp_wide_grad_f32"),
                         ("ltr_mlp_widebf16_grad_workspace_bytes", "ltr_mlp_wide_grad_workspace_bytes")):
        assert isinstance(getattr(lib, ours), ctypes._CFuncPtr)
        assert _C.MLP_WIDEBF16_SIGNATURES[ours] == _C.MLP_WIDE_SIGNATURES[theirs]
        # argument for argument the prototype of ltr_mlp_wide.h, X as bf16
        a = re.search(r"\b%s\s*\(([^)]*)\)" % ours, text).group(1).split()
        b = re.search(r"\b%s\s*\(([^)]*)\)" % theirs, wide).group(1).replace("const float *X", "const uint16_t *X").split()
        assert a == b, ours
    assert len(_C.SIGNATURES) == 80 and lib.ltr_version() == 114


def _scores(lib, B=2, L=10, F=8, H1=4, H2=4, X=P, W=P, out=P):
    return lib.ltr_mlp_widebf16_scores(X, W, P, P, P, P, P, P, B, L, F, H1, H2, out, None)


def _grad(lib, B=2, L=10, F=8, H1=4, H2=4, X=P, W=P, g=P, grads=P, ws=P, ws_bytes=1 << 40):
    return lib.ltr_mlp_widebf16_grad(X, W, P, P, P, P, P, g, P, B, L, F, H1, H2, grads, ws, ws_bytes, None)


@pytest.mark.parametrize("change", [dict(F=12), dict(F=712), dict(F=0), dict(H1=65), dict(H2=17), dict(L=0)])
def test_shape_errors_come_first(lib, change):
    # (every pointer NULL as well: the shape is judged first)
    assert _scores(lib, X=None, W=None, out=None, **change) == ERR_SHAPE
    assert _grad(lib, X=None, W=None, g=None, grads=None, ws=None, ws_bytes=0, **change) == ERR_SHAPE
    assert lib.ltr_mlp_widebf16_grad_workspace_bytes(2, change.get("L", 10), change.get("F", 8), change.get("H1", 4),
                                                     change.get("H2", 4)) == 0


@pytest.mark.parametrize("F", [8, 224, 232, 704])
def test_null_then_empty_then_null_then_workspace(lib, F):
    assert _scores(lib, F=F, W=None, X=None, out=None) == ERR_NULL
    assert _grad(lib, F=F, grads=None) == ERR_NULL
    assert _scores(lib, F=F, B=0, W=None) == ERR_NULL                       # a parameter in front of the empty batch
    assert _scores(lib, F=F, B=0, X=None, out=None) == OK                   # (the gradient call launches: GPU tier)
    assert _scores(lib, F=F, X=None) == ERR_NULL and _scores(lib, F=F, out=None) == ERR_NULL
    assert _grad(lib, F=F, X=None, ws=None, ws_bytes=0) == ERR_NULL         # NULL in front of the workspace
    assert _grad(lib, F=F, g=None, ws=None, ws_bytes=0) == ERR_NULL
    need = lib.ltr_mlp_widebf16_grad_workspace_bytes(2, 10, F, 4, 4)
    assert need >= 4 * lib.ltr_mlp_param_count(F, 4, 4) + 256 * 20
    assert _grad(lib, F=F, ws_bytes=need - 1) == ERR_WORKSPACE and _grad(lib, F=F, ws=None) == ERR_WORKSPACE
    assert lib.ltr_mlp_widebf16_grad_workspace_bytes(0, 10, F, 4, 4) == 0


def test_kernels_exist_and_do_not_spill():
    from pytorchltr_amd import _codeobj
    from pytorchltr_amd.build import LIB_PATH, build_extension
    build_extension()
    ours = {}
    for r in _codeobj.kernel_records(LIB_PATH):
        m = re.search(r"(mlp_widebf16_[a-z0-9_]+_kernel<[^>]*>)", r.get("demangled", r["name"]))
        if m:
            ours[m.group(1)] = r
    assert sorted(ours) == sorted(["mlp_widebf16_fwd_kernel<%d, %s>" % (c, gr) for c in (1, 2, 3) for gr in ("false", "true")]
                                  + ["mlp_widebf16_dw1_kernel<8>", "mlp_widebf16_dw1_kernel<11>"])
    for key, r in ours.items():
        print(key, r.get("vgpr_count"), r.get("agpr_count", 0), r.get("sgpr_count"), r.get("group_segment_fixed_size"))
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, (key, r)
        # two workgroups of four waves per CU: 256 registers a wave (AGPRs included)
        assert 0 < r.get("vgpr_count", 0) + r.get("agpr_count", 0) <= 256, (key, r)


def test_the_route_is_opt_in():
    from pytorchltr_amd import fused

    def route(caller, dtype, F, hidden=(50, 10), L=40, kind=None, **flags):
        return fused._mlp_route(caller, dtype, 3, True, False, True, False, L, F, *hidden, kind, True, **flags)
    bf, f32 = torch.bfloat16, torch.float32
    for caller, kind in (("scorer", None), ("score", None), ("loss", fused._C.HINGE), ("step", fused._C.HINGE)):
        for F in (232, 456, 704) + (() if caller == "step" else (225, 699, 700)):       # (the modules pad to 8)
            assert route(caller, bf, F, kind=kind, wide_bf16=True) is fused._WIDE_BF16, (caller, F)
            assert route(caller, bf, F, kind=kind, wide_bf16=True, fuse_bf16=True) is fused._WIDE_BF16
            assert route(caller, bf, F, kind=kind) is fused._BF16                       # (whose prepare step raises)
        # with the flag nothing else moves: narrow bf16 rows, rows and hidden sizes past the limits, fp32 batches
        for dtype, F, hidden in ((bf, 224, (50, 10)), (bf, 136, (50, 10)), (bf, 712, (50, 10)), (bf, 456, (65, 10)),
                                 (bf, 456, (50, 17)), (f32, 456, (50, 10)), (f32, 136, (50, 10)), (torch.float16, 456, (50, 10))):
            for L in (40, 300):
                assert route(caller, dtype, F, hidden, L, kind, wide_bf16=True) is route(caller, dtype, F, hidden, L, kind)
    assert route("step", bf, 700, kind=fused._C.HINGE, wide_bf16=True) is route("step", bf, 700, kind=fused._C.HINGE)
    assert fused._mlp_route("loss", bf, 3, True, True, True, False, 40, 456, 50, 10, fused._C.HINGE, True, False, True) \
        is fused._TORCH                                                                  # features that need a gradient
    assert fused._ROUTE_FAMILY[fused._WIDE_BF16] is fused._MLP_WIDE_BF16
    assert fused.MLPScorer.wide_bf16 is False and fused.FusedMLPLoss.wide_bf16 is False
    assert fused.MLPScorer(8, (4, 3), wide_bf16=True).wide_bf16 and fused.FusedMLPLoss(8, wide_bf16=True).wide_bf16
    params = [p.detach() for p in fused.MLPScorer(226, (5, 3)).parameters()]
    with pytest.raises(ValueError, match="224 < F <= 704"):                              # 8 features: the narrow family's
        fused.mlp_wide_scores_bf16(torch.zeros(2, 5, 8, dtype=torch.bfloat16), [torch.zeros(5, 8)] + params[1:])
    with pytest.raises(ValueError, match="bfloat16"):
        fused.mlp_wide_grad_bf16(torch.zeros(2, 5, 226), params, torch.zeros(2, 5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fused.mlp_wide_scores_bf16(torch.zeros(2, 5, 226, dtype=torch.bfloat16), params)
