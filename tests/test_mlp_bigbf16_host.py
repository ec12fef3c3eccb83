"""CPU tier of the wide-hidden MLP scorer on bf16 batches (include/ltr_mlp_bigbf16.h, the opt-in route `big_hidden_bf16`):
route table, family limits, the C ABI's argument errors, header against ctypes table, code objects.  No launch."""
import itertools
import os
import re

import pytest
import torch

from tests.test_mlp_big_host import CALLERS, ERR_NULL, ERR_SHAPE, ERR_WORKSPACE, HIDDEN, OK, P, lib  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("caller,dtype", list(itertools.product(CALLERS, (torch.float32, torch.bfloat16, torch.float64))))
def test_route_with_and_without_the_flag(caller, dtype):
    from pytorchltr_amd import fused
    kind = fused._resolve_loss("hinge")[0] if caller in ("loss", "step") else None
    for (H1, H2), F, L, grad, big in itertools.product(HIDDEN, (8, 136, 148, 166, 228), (5, 300), (False, True), (False, True)):
        args = (caller, dtype, 3, True, False, grad, False, L, F, H1, H2, kind, True, False, False, big)
        off, on = fused._mlp_route(*args), fused._mlp_route(*args, True)
        assert fused._mlp_route(*args, False) == off != fused._BIG_BF16
        ours = off is fused._BF16 and (H1 > 64 or H2 > 16) and H1 <= 256 and H2 <= 64 and (F + 7) // 8 * 8 <= 160
        assert on == (fused._BIG_BF16 if ours else off), (caller, dtype, H1, H2, F, L, grad, big)
    base = (caller, torch.bfloat16, 3, True, False, False, False, 5, 136, 256, 64, kind, True, False, False)
    if caller != "scores":
        assert fused._mlp_route(*base, True) is fused._BF16 and fused._mlp_route(*base, False, True) is fused._BIG_BF16
    for i, v in ((4, True), (6, True), (3, False)):
        changed = base[:i] + (v,) + base[i + 1:]
        assert fused._mlp_route(*changed, False, True) == fused._mlp_route(*changed) != fused._BIG_BF16


def test_family_limits():
    from pytorchltr_amd import fused
    fam = fused._MLP_BIG_BF16
    assert fused._ROUTE_FAMILY[fused._BIG_BF16] is fam and fam.dtype is torch.bfloat16 and fam.align == 8
    assert fused.MLP_BIG_BF16_MAX_FEATURES >= 160 and fam.hidden == fused.MLP_BIG_MAX_HIDDEN == (256, 64)
    assert all(fam.takes(*key) for key in ((8, 1, 1), (160, 256, 64), (136, 50, 10), (136, 128, 32), (8, 256, 1), (8, 1, 64)))
    assert not any(fam.takes(*key) for key in ((fused.MLP_BIG_BF16_MAX_FEATURES + 8, 256, 64), (0, 4, 4), (12, 4, 4), (8, 257, 4), (8, 4, 65), (8, 0, 4)))


def _scores(lib, B=2, L=10, F=8, H1=256, H2=64, X=P, W=P, out=P):
    return lib.ltr_mlp_bigbf16_scores(X, W, P, P, P, P, P, P, B, L, F, H1, H2, out, None)


def _grad(lib, B=2, L=10, F=8, H1=256, H2=64, X=P, W=P, g=P, grads=P, ws=P, ws_bytes=1 << 40):
    return lib.ltr_mlp_bigbf16_grad(X, W, P, P, P, P, P, g, P, B, L, F, H1, H2, grads, ws, ws_bytes, None)


@pytest.mark.parametrize("change", [dict(F=12), dict(F=4), dict(F=0), dict(H1=257), dict(H1=0), dict(H2=65), dict(L=0),
                                    dict(B=-1), dict(B=1 << 20, L=1 << 12), "past the widest bucket"])
def test_abi_error_order(lib, change):                                     # shape, NULL, the empty batch, the workspace
    from pytorchltr_amd import fused
    if change == "past the widest bucket":
        change = dict(F=fused.MLP_BIG_BF16_MAX_FEATURES + 8)
    assert _scores(lib, X=None, W=None, out=None, **change) == ERR_SHAPE
    assert _grad(lib, X=None, W=None, g=None, grads=None, ws=None, ws_bytes=0, **change) == ERR_SHAPE
    assert lib.ltr_mlp_bigbf16_grad_workspace_bytes(*{**dict(B=2, L=10, F=8, H1=256, H2=64), **change}.values()) == 0
    for F, H1, H2 in ((8, 256, 64), (fused.MLP_BIG_BF16_MAX_FEATURES, 256, 64), (8, 4, 3)):
        kw = dict(F=F, H1=H1, H2=H2)
        assert _scores(lib, W=None, X=None, out=None, **kw) == _scores(lib, X=None, **kw) == _scores(lib, out=None, **kw) \
            == _grad(lib, grads=None, **kw) == _grad(lib, X=None, ws=None, **kw) == _grad(lib, g=None, ws=None, **kw) == ERR_NULL
        need = lib.ltr_mlp_bigbf16_grad_workspace_bytes(2, 10, F, H1, H2)
        assert need >= 4 * lib.ltr_mlp_param_count(F, H1, H2)
        assert _grad(lib, ws_bytes=need - 1, **kw) == _grad(lib, ws=None, **kw) == ERR_WORKSPACE
    assert _scores(lib, B=0, X=None, out=None) == OK and _scores(lib, B=0, W=None) == _grad(lib, B=0, grads=None) == ERR_NULL


def test_header_and_ctypes_table_agree(lib):
    from pytorchltr_amd import _C
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltr_mlp_bigbf16.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(ltr_[a-z0-9_]+)\s*\(", text))) == sorted(_C.MLP_BIGBF16_SIGNATURES)
    for ours, theirs in (("ltr_mlp_bigbf16_scores", "ltr_mlp_big_scores_f32"), ("ltr_mlp_bigbf16_grad", "ltr_mlp_big_grad_f32"),
                         ("ltr_mlp_bigbf16_grad_workspace_bytes", "ltr_mlp_big_grad_workspace_bytes")):
        assert _C.MLP_BIGBF16_SIGNATURES[ours] == _C.MLP_BIG_SIGNATURES[theirs] and hasattr(lib, ours)
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % ours, text).group(1)
        assert len(proto.split(",")) == len(_C.MLP_BIGBF16_SIGNATURES[ours][1])


def test_bigbf16_kernels_exist_and_do_not_spill():
    from pytorchltr_amd import _codeobj, fused
    from pytorchltr_amd.build import LIB_PATH, build_extension
    build_extension()
    ours = {m.group(1): r for r in _codeobj.kernel_records(LIB_PATH)
            for m in [re.search(r"(mlp_bigbf16_kernel<[^>]*>)", r.get("demangled", r["name"]))] if m}
    buckets = sorted({int(k.split("<")[1].split(",")[0]) for k in ours})
    assert 1 <= len(buckets) <= 3 and 32 * buckets[-1] == fused.MLP_BIG_BF16_MAX_FEATURES
    assert sorted(ours) == sorted("mlp_bigbf16_kernel<%d, %s>" % (ks, g) for ks in buckets for g in ("false", "true"))
    for key, r in ours.items():
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, (key, r)
        assert 0 < r.get("vgpr_count", 0) + r.get("agpr_count", 0) <= 256, (key, r)
