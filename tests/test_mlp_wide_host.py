"""CPU tier of the wide-row MLP scorer (include/ltr_mlp_wide.h, fused.mlp_wide_scores / fused.mlp_wide_grad): the
boundary, the argument errors (decided on the host, in front of any launch), the code objects and the Python surface.
Nothing here gets as far as a launch."""
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


# ---- boundary ----
def test_header_exports_and_ctypes_table_agree(lib):
    from pytorchltr_amd import _C
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltr_mlp_wide.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(ltr_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_C.MLP_WIDE_SIGNATURES)
    assert len(declared) == 3
    for name, (_, argtypes) in _C.MLP_WIDE_SIGNATURES.items():
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr), name          # exported by the library
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1).strip()
        assert len(proto.split(",")) == len(argtypes), name                     # as many arguments as the prototype
        # word for word the prototypes of ltr_mlp_rows.h
        assert argtypes == _C.MLP_ROWS_SIGNATURES[name.replace("_wide_", "_rows_")][1], name
    others = (set(_C.SIGNATURES) | set(_C.EVAL_SIGNATURES) | set(_C.LISTWISE_SIGNATURES) | set(_C.LONGPAIR_SIGNATURES)
              | set(_C.MLP_ROWS_SIGNATURES))
    assert not set(_C.MLP_WIDE_SIGNATURES) & others


def test_exported_mlp_wide_symbols_are_the_declared_ones(lib):
    """Every ltr_mlp_wide_* symbol the library exports is declared in the header (and the other way round); the
    ltr_mlp_rows_* set and the version are what they were."""
    import subprocess
    from pytorchltr_amd import _C, _codeobj
    from pytorchltr_amd.build import LIB_PATH, build_extension
    build_extension()
    out = subprocess.run([_codeobj._tool("llvm-readelf"), "--dyn-syms", "-W", LIB_PATH], check=True,
                         stdout=subprocess.PIPE).stdout.decode()
    defined = "\n".join(ln for ln in out.splitlines() if " FUNC " in ln and " GLOBAL " in ln and " UND " not in ln)
    assert sorted(set(re.findall(r"\b(ltr_mlp_wide_[a-z0-9_]+)\b", defined))) == sorted(_C.MLP_WIDE_SIGNATURES)
    assert sorted(set(re.findall(r"\b(ltr_mlp_rows_[a-z0-9_]+)\b", defined))) == sorted(_C.MLP_ROWS_SIGNATURES)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltr_hip.h")).read(), flags=re.S)
    assert not [k for k in _C.SIGNATURES if "mlp_wide" in k] and "ltr_mlp_wide" not in main
    assert len(_C.SIGNATURES) == 80 and lib.ltr_version() == 114


# ---- argument errors ----
def _scores(lib, B=2, L=10, F=8, H1=4, H2=4, X=P, W=P, out=P):
    return lib.ltr_mlp_wide_scores_f32(X, W, P, P, P, P, P, P, B, L, F, H1, H2, out, None)


def _grad(lib, B=2, L=10, F=8, H1=4, H2=4, X=P, W=P, g=P, grads=P, ws=P, ws_bytes=1 << 40):
    return lib.ltr_mlp_wide_grad_f32(X, W, P, P, P, P, P, g, P, B, L, F, H1, H2, grads, ws, ws_bytes, None)


@pytest.mark.parametrize("change", [dict(F=6), dict(F=708), dict(F=0), dict(H1=65), dict(H1=0), dict(H2=17), dict(L=0),
                                    dict(B=-1), dict(B=1 << 20, L=1 << 12)])
def test_shape_errors_come_first(lib, change):
    # (every pointer NULL as well: the shape is judged first)
    assert _scores(lib, X=None, W=None, out=None, **change) == ERR_SHAPE
    assert _grad(lib, X=None, W=None, g=None, grads=None, ws=None, ws_bytes=0, **change) == ERR_SHAPE
    assert lib.ltr_mlp_wide_grad_workspace_bytes(change.get("B", 2), change.get("L", 10), change.get("F", 8),
                                                 change.get("H1", 4), change.get("H2", 4)) == 0


@pytest.mark.parametrize("F", [8, 224, 228, 704])
def test_feature_counts_up_to_704_reach_the_null_check(lib, F):
    assert _scores(lib, F=F, H1=64, H2=16, W=None, X=None, out=None) == ERR_NULL
    assert _scores(lib, F=F, H1=64, H2=16, X=None) == ERR_NULL
    assert _grad(lib, F=F, H1=64, H2=16, grads=None) == ERR_NULL
    assert _grad(lib, F=F, H1=64, H2=16, g=None) == ERR_NULL
    assert lib.ltr_mlp_wide_grad_workspace_bytes(2, 10, F, 64, 16) > 0


def test_the_row_kernels_keep_their_limit(lib):
    assert lib.ltr_mlp_rows_scores_f32(None, None, None, None, None, None, None, None, 2, 10, 228, 4, 4, None, None) \
        == ERR_SHAPE
    assert lib.ltr_mlp_rows_grad_workspace_bytes(2, 10, 228, 4, 4) == 0


def test_null_then_workspace(lib):
    assert _scores(lib, W=None) == ERR_NULL
    assert _scores(lib, X=None) == ERR_NULL
    assert _scores(lib, out=None) == ERR_NULL
    assert _grad(lib, W=None) == ERR_NULL
    assert _grad(lib, grads=None) == ERR_NULL
    assert _grad(lib, X=None, ws=None, ws_bytes=0) == ERR_NULL              # NULL in front of the workspace
    assert _grad(lib, g=None, ws=None, ws_bytes=0) == ERR_NULL
    for F in (8, 700):
        need = lib.ltr_mlp_wide_grad_workspace_bytes(2, 10, F, 4, 4)
        assert _grad(lib, F=F, ws_bytes=need - 1) == ERR_WORKSPACE
        assert _grad(lib, F=F, ws=None) == ERR_WORKSPACE
    # a long list is a shape like any other: accepted as far as the NULL check
    assert _scores(lib, L=100000, F=700, X=None) == ERR_NULL
    assert _grad(lib, L=100000, F=700, g=None) == ERR_NULL
    assert _grad(lib, L=100000, F=700,
                 ws_bytes=lib.ltr_mlp_wide_grad_workspace_bytes(2, 100000, 700, 4, 4) - 1) == ERR_WORKSPACE


def test_an_empty_batch_is_ok(lib):
    # (the gradient call launches its reduction to write the zero gradients: tests/test_gpu_mlp_wide.py)
    assert _scores(lib, B=0, X=None, out=None) == OK
    assert _scores(lib, B=0, F=700, X=None, out=None) == OK
    assert _scores(lib, B=0, W=None) == ERR_NULL
    assert lib.ltr_mlp_wide_grad_workspace_bytes(0, 10, 700, 4, 4) == 0


def test_workspace_bytes(lib):
    """At least one parameter vector, and non-decreasing in the number of flat rows.  The two-kernel gradient keeps
    256 bytes per flat row in the workspace, so unlike the row kernels' it does not level off at a full grid: the
    shapes are walked in the order of B * L, in which 256 x 1000 (256 000 rows) comes in front of 64 x 4096
    (262 144 rows)."""
    count = lib.ltr_mlp_param_count
    shapes = ((1, 1), (1, 32), (1, 33), (3, 37), (2, 300), (64, 4096), (256, 1000))
    for F, H1, H2 in ((228, 4, 4), (452, 50, 10), (704, 64, 16)):
        one = 4 * count(F, H1, H2)
        last = 0
        for B, L in sorted(shapes, key=lambda s: s[0] * s[1]):
            got = lib.ltr_mlp_wide_grad_workspace_bytes(B, L, F, H1, H2)
            # at least one parameter vector, and the d loss / d hidden-1 tile at 256 bytes per flat row
            assert got >= one + 256 * B * L and got >= last, (B, L, F)
            last = got
    assert lib.ltr_mlp_wide_grad_workspace_bytes(2, 10, 6, 4, 4) == 0
    assert lib.ltr_mlp_wide_grad_workspace_bytes(2, 0, 8, 4, 4) == 0
    assert lib.ltr_mlp_wide_grad_workspace_bytes(2, 10, 708, 4, 4) == 0
    assert lib.ltr_mlp_wide_grad_workspace_bytes(1 << 20, 1 << 12, 8, 4, 4) == 0


# ---- code object ----
def test_wide_kernels_exist_and_do_not_spill():
    from pytorchltr_amd import _codeobj
    from pytorchltr_amd.build import LIB_PATH, build_extension
    build_extension()
    recs = _codeobj.kernel_records(LIB_PATH)  # (no skip without the llvm tools: the no-spill rule is a requirement)
    ours = {}
    for r in recs:
        m = re.search(r"(mlp_wide_[a-z0-9_]+_kernel<[^>]*>)", r.get("demangled", r["name"]))
        if m:
            ours[m.group(1)] = r
    assert sorted(ours) == ["mlp_wide_dw1_kernel<11>", "mlp_wide_dw1_kernel<8>", "mlp_wide_fwd_kernel<false>",
                            "mlp_wide_fwd_kernel<true>"], sorted(ours)
    for key, r in ours.items():
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, (key, r)
        # every instantiation: two workgroups of four waves per CU, 256 registers a wave (AGPRs included)
        assert 0 < r.get("vgpr_count", 0) <= 256, (key, r)
    # the row kernels keep their records
    rows = [r for r in recs if "mlp_rows_kernel<" in r.get("demangled", r["name"])]
    assert len(rows) == 8 and not any(r.get("vgpr_spill_count", 0) for r in rows)


# ---- Python surface ----
def test_python_surface():
    from pytorchltr_amd import fused
    from pytorchltr_amd.fused import mlp_wide_grad, mlp_wide_scores                 # noqa: F401  (importable)
    assert fused.MLP_WIDE_MAX_FEATURES == 704 and fused.MLP_MAX_FEATURES == 224
    for key in ((228, 64, 16), (700, 50, 10), (704, 64, 16)):
        assert fused._mlp_wide_network(*key), key
    for key in ((224, 64, 16), (708, 64, 16), (700, 65, 16), (230, 64, 16), (700, 64, 17), (0, 4, 4)):
        assert not fused._mlp_wide_network(*key), key
    assert fused._mlp_rows_network(224, 64, 16) and not fused._mlp_rows_network(228, 64, 16)
    assert not fused._mlp_rows_network(6, 4, 4) and not fused._mlp_rows_network(8, 65, 4)


def test_cpu_tensors_are_refused():
    from pytorchltr_amd.fused import MLPScorer, mlp_wide_grad, mlp_wide_scores
    m = MLPScorer(228, (4, 3))
    params = [p.detach() for p in m.parameters()]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(2, 5, 228))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mlp_wide_scores(torch.zeros(2, 5, 228), params)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mlp_wide_grad(torch.zeros(2, 5, 228), params, torch.zeros(2, 5))
