"""CPU tier of the wide-hidden MLP scorer on wide bf16 rows (include/ltr_mlp_bigwidebf16.h, the opt-in route
`big_hidden_wide_bf16`): route table, family limits, the C ABI's argument errors, header against ctypes table and
exported symbols, code objects.  No launch."""
import itertools
import os
import re
import subprocess

import pytest
import torch

from tests.test_mlp_big_host import CALLERS, ERR_NULL, ERR_SHAPE, ERR_WORKSPACE, HIDDEN, OK, P, lib  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLDER = ("fuse_bf16", "wide_bf16", "big_hidden", "big_hidden_bf16", "big_hidden_wide")


@pytest.mark.parametrize("caller,dtype", list(itertools.product(CALLERS, (torch.float32, torch.bfloat16, torch.float64))))
def test_route_with_and_without_the_flag(caller, dtype):
    from pytorchltr_amd import fused
    kind = fused._resolve_loss("hinge")[0] if caller in ("loss", "step") else None
    combos = [c for r in range(len(OLDER) + 1) for c in itertools.combinations(OLDER, r)]
    for (H1, H2), F, L, grad in itertools.product(HIDDEN, (8, 136, 160, 161, 168, 220, 699, 704, 705, 712), (5, 300),
                                                  (False, True)):
        args = (caller, dtype, 3, True, False, grad, False, L, F, H1, H2, kind, True)
        for combo in combos:
            kw = {name: True for name in combo}
            off = fused._mlp_route(*args, **kw)
            assert fused._mlp_route(*args, big_hidden_wide_bf16=False, **kw) == off != fused._BIG_WIDE_BF16
            ours = (off is fused._BF16 and (H1 > 64 or H2 > 16) and H1 <= 256 and H2 <= 64
                    and 160 < (F + 7) // 8 * 8 <= 704)
            assert fused._mlp_route(*args, big_hidden_wide_bf16=True, **kw) == (fused._BIG_WIDE_BF16 if ours else off), \
                (caller, dtype, H1, H2, F, L, grad, combo)
    # the modules pad 699 to 704, the step function takes whole 16-byte rows only, mlp_scores has no bf16 route
    on = fused._mlp_route(caller, torch.bfloat16, 3, True, False, False, False, 5, 699, 256, 64, kind, True,
                          big_hidden_wide_bf16=True)
    assert (on is fused._BIG_WIDE_BF16) == (caller in ("scorer", "score", "loss"))
    # a batch that needs a gradient, autocast, the CPU: what they answer without the flag
    for i, v in ((4, True), (6, True), (3, False)):
        base = (caller, torch.bfloat16, 3, True, False, False, False, 5, 224, 256, 64, kind, True)
        changed = base[:i] + (v,) + base[i + 1:]
        assert fused._mlp_route(*changed, big_hidden_wide_bf16=True) == fused._mlp_route(*changed) != fused._BIG_WIDE_BF16


def test_family_limits_and_the_flag_on_the_modules():
    from pytorchltr_amd import fused
    fam = fused._MLP_BIG_WIDE_BF16
    assert fused._ROUTE_FAMILY[fused._BIG_WIDE_BF16] is fam and fam.dtype is torch.bfloat16 and fam.align == 8
    assert fused.MLP_BIG_WIDE_BF16_MAX_FEATURES == 704 and fam.hidden == (256, 64) and (fam.f_min, fam.f_max) == (160, 704)
    assert "wide-hidden wide-row bf16" in fam.limits and fam.limits != fused._MLP_BIG_BF16.limits
    assert all(fam.takes(*key) for key in ((168, 1, 1), (704, 256, 64), (224, 128, 32), (704, 50, 10)))
    assert not any(fam.takes(*key) for key in ((160, 256, 64), (712, 256, 64), (172, 4, 4), (168, 257, 4), (168, 4, 65)))
    assert fused.MLPScorer(699, (256, 64), big_hidden_wide_bf16=True).big_hidden_wide_bf16 is True
    assert fused.FusedMLPLoss(220, "hinge", (128, 32), big_hidden_wide_bf16=True).big_hidden_wide_bf16 is True
    assert fused.MLPScorer(699, (256, 64)).big_hidden_wide_bf16 is fused.FusedMLPListwiseLoss(220).big_hidden_wide_bf16 \
        is fused.FusedMLPLambdaRankLoss(220).big_hidden_wide_bf16 is False


def _scores(lib, B=2, L=10, F=224, H1=256, H2=64, X=P, W=P, out=P):
    return lib.ltr_mlp_bigwidebf16_scores(X, W, P, P, P, P, P, P, B, L, F, H1, H2, out, None)


def _grad(lib, B=2, L=10, F=224, H1=256, H2=64, X=P, W=P, g=P, grads=P, ws=P, ws_bytes=1 << 40):
    return lib.ltr_mlp_bigwidebf16_grad(X, W, P, P, P, P, P, g, P, B, L, F, H1, H2, grads, ws, ws_bytes, None)


@pytest.mark.parametrize("change", [dict(F=220), dict(F=228), dict(F=712), dict(F=0), dict(H1=257), dict(H1=0),
                                    dict(H2=65), dict(L=0), dict(B=-1), dict(B=1 << 20, L=1 << 12)])
def test_abi_error_order(lib, change):                                     # shape, NULL, the empty batch, the workspace
    assert _scores(lib, X=None, W=None, out=None, **change) == ERR_SHAPE
    assert _grad(lib, X=None, W=None, g=None, grads=None, ws=None, ws_bytes=0, **change) == ERR_SHAPE
    assert lib.ltr_mlp_bigwidebf16_grad_workspace_bytes(*{**dict(B=2, L=10, F=224, H1=256, H2=64), **change}.values()) == 0
    for F, H1, H2 in ((224, 256, 64), (704, 256, 64), (8, 4, 3)):
        kw = dict(F=F, H1=H1, H2=H2)
        assert _scores(lib, W=None, X=None, out=None, **kw) == _scores(lib, X=None, **kw) == _scores(lib, out=None, **kw) \
            == _grad(lib, grads=None, **kw) == _grad(lib, X=None, ws=None, **kw) == _grad(lib, g=None, ws=None, **kw) == ERR_NULL
        need = lib.ltr_mlp_bigwidebf16_grad_workspace_bytes(2, 10, F, H1, H2)
        # one partial dW1, one vector of the small sums, the d hidden-1 rows of the one tile
        assert need >= 4 * (lib.ltr_mlp_param_count(F, H1, H2) + 32 * H1)
        assert _grad(lib, ws_bytes=need - 1, **kw) == _grad(lib, ws=None, **kw) == ERR_WORKSPACE
    assert _scores(lib, B=0, X=None, out=None) == OK and _scores(lib, B=0, W=None) == _grad(lib, B=0, grads=None) == ERR_NULL


def test_header_ctypes_table_and_exported_symbols_agree(lib):
    from pytorchltr_amd import _C, _codeobj
    from pytorchltr_amd.build import LIB_PATH
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltr_mlp_bigwidebf16.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(ltr_[a-z0-9_]+)\s*\(", text))) == sorted(_C.MLP_BIGWIDEBF16_SIGNATURES)
    for ours, theirs in (("ltr_mlp_bigwidebf16_scores", "ltr_mlp_bigwide_scores_f32"),
                         ("ltr_mlp_bigwidebf16_grad", "ltr_mlp_bigwide_grad_f32"),
                         ("ltr_mlp_bigwidebf16_grad_workspace_bytes", "ltr_mlp_bigwide_grad_workspace_bytes")):
        assert _C.MLP_BIGWIDEBF16_SIGNATURES[ours] == _C.MLP_BIGWIDE_SIGNATURES[theirs] and hasattr(lib, ours)
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % ours, text).group(1)
        assert len(proto.split(",")) == len(_C.MLP_BIGWIDEBF16_SIGNATURES[ours][1])
    out = subprocess.run([_codeobj._tool("llvm-readelf"), "--dyn-syms", "-W", LIB_PATH], check=True,
                         stdout=subprocess.PIPE).stdout.decode()
    defined = "\n".join(ln for ln in out.splitlines() if " FUNC " in ln and " GLOBAL " in ln and " UND " not in ln)
    assert sorted(set(re.findall(r"\b(ltr_mlp_bigwidebf16_[a-z0-9_]+)\b", defined))) == sorted(_C.MLP_BIGWIDEBF16_SIGNATURES)


def test_bigwidebf16_kernels_exist_and_do_not_spill():
    from pytorchltr_amd import _codeobj
    from pytorchltr_amd.build import LIB_PATH, build_extension
    build_extension()
    ours = {m.group(1): r for r in _codeobj.kernel_records(LIB_PATH)
            for m in [re.search(r"(mlp_bigwidebf16_\w+_kernel<[^>]*>)", r.get("demangled", r["name"]))] if m}
    assert sorted(ours) == ["mlp_bigwidebf16_dw1_kernel<15>", "mlp_bigwidebf16_dw1_kernel<8>",
                            "mlp_bigwidebf16_fwd_kernel<4, false>", "mlp_bigwidebf16_fwd_kernel<4, true>"]
    for key, r in ours.items():
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, (key, r)
        assert 0 < r.get("vgpr_count", 0) + r.get("agpr_count", 0) <= 256, (key, r)
