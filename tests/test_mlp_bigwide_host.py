"""CPU tier of the MLP scorer with wide hidden layers on wide rows (include/ltr_mlp_bigwide.h, fused.mlp_bigwide_scores /
fused.mlp_bigwide_grad, the opt-in route `big_hidden_wide`): the route table with and without the flag, the family's
limits, the argument errors of the C ABI (decided on the host, in front of any launch) and the code objects.  Nothing
here gets as far as a launch."""
import itertools
import os
import re

import pytest
import torch

P = 256                                        # dummy non-NULL device pointer: never dereferenced below
OK, ERR_NULL, ERR_SHAPE, ERR_WORKSPACE = 0, -1, -2, -5
CALLERS = ("scorer", "score", "loss", "step", "scores")
HIDDEN = ((4, 3), (64, 16), (65, 3), (4, 17), (256, 64), (257, 3), (4, 65))


@pytest.fixture(scope="module")
def lib():
    from pytorchltr_amd import _C
    from pytorchltr_amd.build import build_extension
    if not os.environ.get("LTR_HIP_LIB"):
        build_extension()
    return _C.lib()


def _route(caller, dtype, L, F, H1, H2, flags=(), grad=False, cuda=True, req=False, autocast=False, dim=3):
    from pytorchltr_amd import fused
    kind = fused._resolve_loss("hinge")[0] if caller in ("loss", "step") else None
    return fused._mlp_route(caller, dtype, dim, cuda, req, grad, autocast, L, F, H1, H2, kind, True,
                            **{name: True for name in flags})


@pytest.mark.parametrize("caller,dtype", list(itertools.product(CALLERS, (torch.float32, torch.bfloat16, torch.float64))))
def test_route_with_and_without_the_flag(caller, dtype):
    from pytorchltr_amd import fused
    module = caller in ("scorer", "score", "loss")
    others = ("fuse_bf16", "wide_bf16", "big_hidden", "big_hidden_bf16")
    for (H1, H2), F, L, grad in itertools.product(HIDDEN, (8, 136, 144, 148, 220, 700, 704, 708), (5, 300), (False, True)):
        off = _route(caller, dtype, L, F, H1, H2, (), grad)
        on = _route(caller, dtype, L, F, H1, H2, ("big_hidden_wide",), grad)
        taken = (dtype is torch.float32 and (H1 > 64 or H2 > 16) and H1 <= 256 and H2 <= 64 and 144 < F <= 704)
        assert on == (fused._BIG_WIDE if taken else off), (caller, dtype, H1, H2, F, L, grad)
        if taken:
            assert off is fused._TORCH                     # today's answer: torch layers / ValueError
        # every combination of the other flags answers what it answered, and never _BIG_WIDE
        for r in range(1, 3):
            for combo in itertools.combinations(others, r):
                was = _route(caller, dtype, L, F, H1, H2, combo, grad)
                assert was != fused._BIG_WIDE
                assert _route(caller, dtype, L, F, H1, H2, combo + ("big_hidden_wide",), grad) == \
                    (fused._BIG_WIDE if taken else was)
    # the raw feature count for the functions, the padded one for the modules (Yahoo: 699 -> 700)
    assert _route(caller, torch.float32, 5, 699, 256, 64, ("big_hidden_wide",)) == \
        (fused._BIG_WIDE if module else fused._TORCH)
    # a batch that needs a gradient, autocast, the CPU, two dimensions: what they answer without the flag
    for kw in (dict(req=True), dict(autocast=True), dict(cuda=False), dict(dim=2)):
        assert _route(caller, torch.float32, 5, 220, 256, 64, ("big_hidden_wide",), **kw) == \
            _route(caller, torch.float32, 5, 220, 256, 64, (), **kw) != fused._BIG_WIDE


def test_family_limits_and_the_flag_on_the_modules():
    from pytorchltr_amd import fused
    takes = fused._MLP_BIG_WIDE.takes
    assert fused.MLP_BIG_WIDE_MAX_FEATURES == 704 and fused.MLP_BIG_MAX_FEATURES == 144
    assert fused._ROUTE_FAMILY[fused._BIG_WIDE] is fused._MLP_BIG_WIDE and fused._MLP_BIG_WIDE.hidden == (256, 64)
    assert all(takes(*key) for key in ((148, 1, 1), (704, 256, 64), (220, 128, 32), (700, 50, 10)))
    assert not any(takes(*key) for key in ((144, 256, 64), (708, 256, 64), (150, 4, 4), (148, 257, 4), (148, 4, 65)))
    assert fused.MLPScorer(700, (256, 64), big_hidden_wide=True).big_hidden_wide is True
    assert fused.FusedMLPLoss(220, "hinge", (128, 32), big_hidden_wide=True).big_hidden_wide is True
    assert fused.MLPScorer(700, (256, 64)).big_hidden_wide is fused.FusedMLPListwiseLoss(220).big_hidden_wide is False


def _scores(lib, B=2, L=10, F=220, H1=256, H2=64, X=P, W=P, out=P):
    return lib.ltr_mlp_bigwide_scores_f32(X, W, P, P, P, P, P, P, B, L, F, H1, H2, out, None)


def _grad(lib, B=2, L=10, F=220, H1=256, H2=64, X=P, W=P, g=P, grads=P, ws=P, ws_bytes=1 << 40):
    return lib.ltr_mlp_bigwide_grad_f32(X, W, P, P, P, P, P, g, P, B, L, F, H1, H2, grads, ws, ws_bytes, None)


@pytest.mark.parametrize("change", [dict(F=222), dict(F=708), dict(F=0), dict(H1=257), dict(H1=0), dict(H2=65), dict(L=0),
                                    dict(B=-1), dict(B=1 << 20, L=1 << 12)])
def test_abi_shape_errors_come_first(lib, change):
    assert _scores(lib, X=None, W=None, out=None, **change) == ERR_SHAPE
    assert _grad(lib, X=None, W=None, g=None, grads=None, ws=None, ws_bytes=0, **change) == ERR_SHAPE
    assert lib.ltr_mlp_bigwide_grad_workspace_bytes(*{**dict(B=2, L=10, F=220, H1=256, H2=64), **change}.values()) == 0


def test_abi_null_empty_workspace_order(lib):
    for F, H1, H2 in ((220, 256, 64), (704, 256, 64), (8, 4, 3)):
        kw = dict(F=F, H1=H1, H2=H2)
        assert _scores(lib, W=None, X=None, out=None, **kw) == _scores(lib, X=None, **kw) == _scores(lib, out=None, **kw) \
            == _grad(lib, grads=None, **kw) == _grad(lib, X=None, ws=None, **kw) == _grad(lib, g=None, ws=None, **kw) == ERR_NULL
        need = lib.ltr_mlp_bigwide_grad_workspace_bytes(2, 10, F, H1, H2)
        # one partial dW1, one vector of the small sums, the d hidden-1 rows of the one tile
        assert need >= 4 * (lib.ltr_mlp_param_count(F, H1, H2) + 32 * H1)
        assert _grad(lib, ws_bytes=need - 1, **kw) == _grad(lib, ws=None, **kw) == ERR_WORKSPACE
    assert _scores(lib, B=0, X=None, out=None) == OK and _scores(lib, B=0, W=None) == ERR_NULL


def test_bigwide_kernels_exist_and_do_not_spill():
    from pytorchltr_amd import _codeobj
    from pytorchltr_amd.build import LIB_PATH, build_extension
    build_extension()
    ours = {m.group(1): r for r in _codeobj.kernel_records(LIB_PATH)
            for m in [re.search(r"(mlp_bigwide_\w+_kernel<[^>]*>)", r.get("demangled", r["name"]))] if m}
    assert sorted(ours) == ["mlp_bigwide_dw1_kernel<11>", "mlp_bigwide_dw1_kernel<8>", "mlp_bigwide_fwd_kernel<false>",
                            "mlp_bigwide_fwd_kernel<true>"]
    for key, r in ours.items():
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, (key, r)
        assert 0 < r.get("vgpr_count", 0) <= 256, (key, r)
