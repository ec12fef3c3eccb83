"""CPU tier of the stand-alone MLP scorer (include/ltr_mlp_rows.h, fused.MLPScorer / fused.mlp_grad): the boundary, the
argument errors (decided on the host, in front of any launch), the code objects and the Python surface.  Nothing here
gets as far as a launch."""
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
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltr_mlp_rows.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(ltr_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_C.MLP_ROWS_SIGNATURES)
    assert len(declared) == 3
    for name, (_, argtypes) in _C.MLP_ROWS_SIGNATURES.items():
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr), name          # exported by the library
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1).strip()
        assert len(proto.split(",")) == len(argtypes), name                     # as many arguments as the prototype
    others = set(_C.SIGNATURES) | set(_C.EVAL_SIGNATURES) | set(_C.LISTWISE_SIGNATURES) | set(_C.LONGPAIR_SIGNATURES)
    assert not set(_C.MLP_ROWS_SIGNATURES) & others


def test_exported_mlp_rows_symbols_are_the_declared_ones():
    """Every ltr_mlp_rows_* symbol the library exports is declared in the header (and the other way round)."""
    import subprocess
    from pytorchltr_amd import _C, _codeobj
    from pytorchltr_amd.build import LIB_PATH, build_extension
    build_extension()
    # (llvm-readelf of the ROCm toolchain, which _codeobj needs anyway: a machine without it fails here, it does not skip)
    out = subprocess.run([_codeobj._tool("llvm-readelf"), "--dyn-syms", "-W", LIB_PATH], check=True,
                         stdout=subprocess.PIPE).stdout.decode()
    defined = [ln for ln in out.splitlines() if " FUNC " in ln and " GLOBAL " in ln and " UND " not in ln]
    exported = sorted(set(re.findall(r"\b(ltr_mlp_rows_[a-z0-9_]+)\b", "\n".join(defined))))
    assert exported == sorted(_C.MLP_ROWS_SIGNATURES)


def test_the_main_table_is_unchanged(lib):
    from pytorchltr_amd import _C
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltr_hip.h")).read(), flags=re.S)
    assert not [k for k in _C.SIGNATURES if "mlp_rows" in k] and "ltr_mlp_rows" not in text
    assert len(_C.SIGNATURES) == 80 and lib.ltr_version() == 114


# ---- argument errors ----
def _scores(lib, B=2, L=10, F=8, H1=4, H2=4, X=P, W=P, out=P):
    return lib.ltr_mlp_rows_scores_f32(X, W, P, P, P, P, P, P, B, L, F, H1, H2, out, None)


def _grad(lib, B=2, L=10, F=8, H1=4, H2=4, X=P, W=P, g=P, grads=P, ws=P, ws_bytes=1 << 40):
    return lib.ltr_mlp_rows_grad_f32(X, W, P, P, P, P, P, g, P, B, L, F, H1, H2, grads, ws, ws_bytes, None)


@pytest.mark.parametrize("change", [dict(F=6), dict(F=228), dict(F=0), dict(H1=65), dict(H2=17), dict(H1=0), dict(L=0),
                                    dict(B=-1), dict(B=1 << 20, L=1 << 12)])
def test_shape_errors_come_first(lib, change):
    # (every pointer NULL as well: the shape is judged first)
    assert _scores(lib, X=None, W=None, out=None, **change) == ERR_SHAPE
    assert _grad(lib, X=None, W=None, g=None, grads=None, ws=None, ws_bytes=0, **change) == ERR_SHAPE
    assert lib.ltr_mlp_rows_grad_workspace_bytes(change.get("B", 2), change.get("L", 10), change.get("F", 8),
                                                 change.get("H1", 4), change.get("H2", 4)) == 0


def test_null_then_workspace(lib):
    assert _scores(lib, W=None) == ERR_NULL
    assert _scores(lib, X=None) == ERR_NULL
    assert _scores(lib, out=None) == ERR_NULL
    assert _grad(lib, W=None) == ERR_NULL
    assert _grad(lib, grads=None) == ERR_NULL
    assert _grad(lib, X=None, ws=None, ws_bytes=0) == ERR_NULL              # NULL in front of the workspace
    assert _grad(lib, g=None, ws=None, ws_bytes=0) == ERR_NULL
    need = lib.ltr_mlp_rows_grad_workspace_bytes(2, 10, 8, 4, 4)
    assert _grad(lib, ws_bytes=need - 1) == ERR_WORKSPACE
    assert _grad(lib, ws=None) == ERR_WORKSPACE
    # a long list is a shape like any other: accepted as far as the NULL check
    assert _scores(lib, L=100000, X=None) == ERR_NULL
    assert _grad(lib, L=100000, g=None) == ERR_NULL
    assert _grad(lib, L=100000, ws_bytes=lib.ltr_mlp_rows_grad_workspace_bytes(2, 100000, 8, 4, 4) - 1) == ERR_WORKSPACE


def test_an_empty_batch_is_ok(lib):
    # (the gradient call launches its reduction to write the zero gradients: tests/test_gpu_mlp_rows.py)
    assert _scores(lib, B=0, X=None, out=None) == OK
    assert _scores(lib, B=0, W=None) == ERR_NULL
    assert lib.ltr_mlp_rows_grad_workspace_bytes(0, 10, 8, 4, 4) == 0


def test_workspace_bytes(lib):
    count = lib.ltr_mlp_param_count
    for F, H1, H2 in ((8, 4, 4), (136, 50, 10), (224, 64, 16)):
        one = 4 * count(F, H1, H2)
        last = 0
        for B, L in ((1, 1), (1, 32), (1, 33), (3, 37), (2, 300), (5, 300), (64, 4096), (256, 1000), (2047, 1 << 20)):
            got = lib.ltr_mlp_rows_grad_workspace_bytes(B, L, F, H1, H2)
            assert got >= one and got >= last, (B, L, F)
            last = got
    assert lib.ltr_mlp_rows_grad_workspace_bytes(2, 10, 6, 4, 4) == 0
    assert lib.ltr_mlp_rows_grad_workspace_bytes(2, 0, 8, 4, 4) == 0
    assert lib.ltr_mlp_rows_grad_workspace_bytes(1 << 20, 1 << 12, 8, 4, 4) == 0


# ---- code object ----
def test_row_kernels_exist_for_every_bucket_and_do_not_spill():
    from pytorchltr_amd import _codeobj
    from pytorchltr_amd.build import LIB_PATH, build_extension
    build_extension()
    recs = _codeobj.kernel_records(LIB_PATH)  # (no skip without the llvm tools: the no-spill rule is a requirement)
    ours = {}
    for r in recs:
        m = re.search(r"mlp_rows_kernel<(\d+), (true|false)>", r.get("demangled", r["name"]))
        if m:
            ours[(int(m.group(1)), m.group(2) == "true")] = r
    assert sorted(ours) == sorted((nt, grad) for nt in (3, 5, 9, 14) for grad in (False, True)), sorted(ours)
    for key, r in ours.items():
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, (key, r)
        # two workgroups of four waves per CU: 256 registers a wave; the widest gradient kernel runs one per CU
        assert r.get("vgpr_count", 0) <= (512 if key == (14, True) else 256), (key, r)


# ---- Python surface ----
def test_python_surface():
    from pytorchltr_amd import fused
    from pytorchltr_amd.fused import FusedMLPLoss, MLPScorer, mlp_grad            # noqa: F401  (importable)
    for F, hidden in ((136, (50, 10)), (46, (64, 16)), (8, (3, 2))):
        a = MLPScorer(F, hidden).state_dict()
        b = FusedMLPLoss(F, "hinge", hidden=hidden).state_dict()
        assert list(a) == list(b) == ["l1.weight", "l1.bias", "l2.weight", "l2.bias", "l3.weight", "l3.bias"]
        assert [tuple(v.shape) for v in a.values()] == [tuple(v.shape) for v in b.values()]
    assert MLPScorer(8).l1.out_features == 50 and MLPScorer(8).l2.out_features == 10
    assert fused._mlp_rows_network(224, 64, 16) and not fused._mlp_rows_network(228, 64, 16)
    assert not fused._mlp_rows_network(6, 4, 4) and not fused._mlp_rows_network(8, 65, 4)


def test_cpu_tensors_are_refused():
    from pytorchltr_amd.fused import MLPScorer, mlp_grad
    m = MLPScorer(8, (4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(2, 5, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mlp_grad(torch.zeros(2, 5, 8), [p.detach() for p in m.parameters()], torch.zeros(2, 5))
