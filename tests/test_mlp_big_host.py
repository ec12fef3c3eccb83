"""CPU tier of the MLP scorer with wide hidden layers (include/ltr_mlp_big.h, fused.mlp_big_scores / fused.mlp_big_grad,
the opt-in route `big_hidden`): the route table with and without the flag, the family's limits, the argument errors of
the C ABI (decided on the host, in front of any launch) and the code objects.  Nothing here gets as far as a launch."""
import itertools
import os
import re

import pytest
import torch

P = 256                                        # dummy non-NULL device pointer: never dereferenced below
OK, ERR_NULL, ERR_SHAPE, ERR_WORKSPACE = 0, -1, -2, -5
CALLERS = ("scorer", "score", "loss", "step", "scores")
HIDDEN = ((4, 3), (65, 3), (4, 17), (256, 64), (257, 3), (4, 65))


@pytest.fixture(scope="module")
def lib():
    from pytorchltr_amd import _C
    from pytorchltr_amd.build import build_extension
    if not os.environ.get("LTR_HIP_LIB"):
        build_extension()
    return _C.lib()


def _route(caller, dtype, L, F, H1, H2, big, grad=False, cuda=True, req=False, autocast=False, dim=3):
    from pytorchltr_amd import fused
    kind = fused._resolve_loss("hinge")[0] if caller in ("loss", "step") else None
    return fused._mlp_route(caller, dtype, dim, cuda, req, grad, autocast, L, F, H1, H2, kind, True, False, False, big)


@pytest.mark.parametrize("caller,dtype", list(itertools.product(CALLERS, (torch.float32, torch.bfloat16, torch.float64))))
def test_route_with_and_without_the_flag(caller, dtype):
    from pytorchltr_amd import fused
    module = caller in ("scorer", "score", "loss")
    for (H1, H2), F, L, grad in itertools.product(HIDDEN, (8, 136, 148, 228), (5, 300), (False, True)):
        off = _route(caller, dtype, L, F, H1, H2, False, grad)
        on = _route(caller, dtype, L, F, H1, H2, True, grad)
        big = (dtype is torch.float32 and (H1 > 64 or H2 > 16) and H1 <= 256 and H2 <= 64 and F <= 144)
        assert on == (fused._BIG if big else off), (caller, dtype, H1, H2, F, L, grad)
        if big:
            assert off is fused._TORCH                     # today's answer: torch layers / ValueError
    # the raw feature count for the functions, the padded one for the modules
    assert _route(caller, torch.float32, 5, 142, 256, 64, True) == (fused._BIG if module else fused._TORCH)
    # a batch that needs a gradient, autocast, the CPU, two dimensions: what they answer without the flag
    for kw in (dict(req=True), dict(autocast=True), dict(cuda=False), dict(dim=2)):
        assert _route(caller, torch.float32, 5, 136, 256, 64, True, **kw) == \
            _route(caller, torch.float32, 5, 136, 256, 64, False, **kw) != fused._BIG


def test_family_limits():                      # (the ValueError text needs a device batch: tests/test_gpu_mlp_big.py)
    from pytorchltr_amd import fused
    takes = fused._MLP_BIG.takes
    assert fused.MLP_BIG_MAX_FEATURES >= 144 and fused.MLP_BIG_MAX_HIDDEN == fused._MLP_BIG.hidden == (256, 64)
    assert all(takes(*key) for key in ((4, 1, 1), (144, 256, 64), (136, 50, 10), (8, 256, 1), (8, 1, 64)))
    assert not any(takes(*key) for key in ((148, 256, 64), (0, 4, 4), (6, 4, 4), (8, 257, 4), (8, 4, 65), (8, 0, 4)))
    assert fused._MLP_ROWS.takes(8, 64, 16) and not fused._MLP_ROWS.takes(8, 65, 16)


def _scores(lib, B=2, L=10, F=8, H1=256, H2=64, X=P, W=P, out=P):
    return lib.ltr_mlp_big_scores_f32(X, W, P, P, P, P, P, P, B, L, F, H1, H2, out, None)


def _grad(lib, B=2, L=10, F=8, H1=256, H2=64, X=P, W=P, g=P, grads=P, ws=P, ws_bytes=1 << 40):
    return lib.ltr_mlp_big_grad_f32(X, W, P, P, P, P, P, g, P, B, L, F, H1, H2, grads, ws, ws_bytes, None)


@pytest.mark.parametrize("change", [dict(F=6), dict(F=148), dict(F=0), dict(H1=257), dict(H1=0), dict(H2=65), dict(L=0),
                                    dict(B=-1), dict(B=1 << 20, L=1 << 12)])
def test_abi_shape_errors_come_first(lib, change):
    assert _scores(lib, X=None, W=None, out=None, **change) == ERR_SHAPE
    assert _grad(lib, X=None, W=None, g=None, grads=None, ws=None, ws_bytes=0, **change) == ERR_SHAPE
    assert lib.ltr_mlp_big_grad_workspace_bytes(*{**dict(B=2, L=10, F=8, H1=256, H2=64), **change}.values()) == 0


def test_abi_null_empty_workspace_order(lib):
    for F, H1, H2 in ((8, 256, 64), (144, 256, 64), (8, 4, 3)):
        kw = dict(F=F, H1=H1, H2=H2)
        assert _scores(lib, W=None, X=None, out=None, **kw) == _scores(lib, X=None, **kw) == _scores(lib, out=None, **kw) \
            == _grad(lib, grads=None, **kw) == _grad(lib, X=None, ws=None, **kw) == _grad(lib, g=None, ws=None, **kw) == ERR_NULL
        need = lib.ltr_mlp_big_grad_workspace_bytes(2, 10, F, H1, H2)
        assert need >= 4 * lib.ltr_mlp_param_count(F, H1, H2)
        assert _grad(lib, ws_bytes=need - 1, **kw) == _grad(lib, ws=None, **kw) == ERR_WORKSPACE
    assert _scores(lib, B=0, X=None, out=None) == OK and _scores(lib, B=0, W=None) == ERR_NULL


def test_big_kernels_exist_and_do_not_spill():
    from pytorchltr_amd import _codeobj
    from pytorchltr_amd.build import LIB_PATH, build_extension
    build_extension()
    ours = {m.group(1): r for r in _codeobj.kernel_records(LIB_PATH)
            for m in [re.search(r"(mlp_big_kernel<[^>]*>)", r.get("demangled", r["name"]))] if m}
    assert sorted(ours) == sorted("mlp_big_kernel<%d, %s>" % (nt, g) for nt in (3, 5, 9) for g in ("false", "true"))
    for key, r in ours.items():
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, (key, r)
        assert 0 < r.get("vgpr_count", 0) <= 256, (key, r)
