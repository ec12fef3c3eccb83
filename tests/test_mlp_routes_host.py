"""The route table of the MLP scorer: which kernel family a batch reaches from each public caller.

CASES varies one axis at a time off the base (fp32, F = 8, L = 5, hidden (4, 3), no input gradient, no autocast), plus
the crossings on each side of every limit of the table; every batch is B = 2 with n = [L, L // 2 + 1].  EXPECTED is what
tests/test_gpu_mlp_routes.py recorded on an MI355X at commit e6eba4d (the parent of the commit that introduced
``fused._mlp_route``): per case and caller, the ``ltr_mlp_*`` entry points in the order they were called, "torch" where
the three ``nn.Linear`` layers ran, "raises <class>" where the call raised.  The GPU test proves that the callers obey
the table; the test below proves, without a GPU, that the one pure route function states it.
"""
import pytest
import torch

BASE = dict(dtype="float32", F=8, L=5, hidden=(4, 3), xgrad=False, autocast=False)


def _vary(**kw):
    return dict(BASE, **kw)


CASES = {
    "base": _vary(),
    "bf16": _vary(dtype="bfloat16"), "fp16": _vary(dtype="float16"), "fp64": _vary(dtype="float64"),
    "F46": _vary(F=46), "F148": _vary(F=148), "F224": _vary(F=224), "F228": _vary(F=228), "F700": _vary(F=700),
    "F708": _vary(F=708),
    "L130": _vary(L=130), "L260": _vary(L=260),                     # (also the crossings L = 130 / 260 at F = 8)
    "H65x3": _vary(hidden=(65, 3)), "H4x17": _vary(hidden=(4, 17)),
    "xgrad": _vary(xgrad=True), "autocast": _vary(autocast=True),
    "L130-F148": _vary(L=130, F=148),
    "bf16-F12": _vary(dtype="bfloat16", F=12), "bf16-F228": _vary(dtype="bfloat16", F=228),
    "bf16-L260": _vary(dtype="bfloat16", L=260),
    "F700-L260": _vary(F=700, L=260),
}

# caller -> (the route function's caller, grad mode, loss)
CALLERS = {
    "scorer": ("scorer", True, None), "scorer-nograd": ("scorer", False, None),
    "score": ("score", True, None), "score-nograd": ("score", False, None),
    "hinge": ("loss", True, "hinge"), "listnet": ("loss", True, "listnet"), "listmle": ("loss", True, "listmle"),
    "mlp_loss_step": ("step", True, "hinge"), "mlp_scores": ("scores", True, None),
}

EXPECTED = {
    "base": {
        "scorer": ["ltr_mlp_rows_scores_f32", "ltr_mlp_rows_grad_f32"],
        "scorer-nograd": ["ltr_mlp_rows_scores_f32"],
        "score": ["ltr_mlp_rows_scores_f32", "ltr_mlp_rows_grad_f32"],
        "score-nograd": ["ltr_mlp_scores_f32"],
        "hinge": ["ltr_mlp_pairwise_f32"],
        "listnet": ["ltr_mlp_listwise_f32"],
        "listmle": ["ltr_mlp_listwise_f32"],
        "mlp_loss_step": ["ltr_mlp_pairwise_f32"],
        "mlp_scores": ["ltr_mlp_scores_f32"],
    },
    "bf16": {
        "scorer": ["ltr_mlp_bf16_scores", "ltr_mlp_bf16_grad"],
        "scorer-nograd": ["ltr_mlp_bf16_scores"],
        "score": ["ltr_mlp_bf16_scores", "ltr_mlp_bf16_grad"],
        "score-nograd": ["ltr_mlp_bf16_scores"],
        "hinge": ["ltr_mlp_bf16_scores", "ltr_mlp_bf16_grad"],
        "listnet": ["ltr_mlp_bf16_scores", "ltr_mlp_bf16_grad"],
        "listmle": ["ltr_mlp_bf16_scores", "ltr_mlp_bf16_grad"],
        "mlp_loss_step": ["ltr_mlp_bf16_scores", "ltr_mlp_bf16_grad"],
        "mlp_scores": ["ltr_mlp_scores_f32"],
    },
    "fp16": {
        "scorer": ["raises RuntimeError"],
        "scorer-nograd": ["raises RuntimeError"],
        "score": ["raises RuntimeError"],
        "score-nograd": ["ltr_mlp_scores_f32"],
        "hinge": ["ltr_mlp_pairwise_f32"],
        "listnet": ["ltr_mlp_listwise_f32"],
        "listmle": ["ltr_mlp_listwise_f32"],
        "mlp_loss_step": ["ltr_mlp_pairwise_f32"],
        "mlp_scores": ["ltr_mlp_scores_f32"],
    },
    "fp64": {
        "scorer": ["raises RuntimeError"],
        "scorer-nograd": ["raises RuntimeError"],
        "score": ["raises RuntimeError"],
        "score-nograd": ["ltr_mlp_scores_f32"],
        "hinge": ["ltr_mlp_pairwise_f32"],
        "listnet": ["ltr_mlp_listwise_f32"],
        "listmle": ["ltr_mlp_listwise_f32"],
        "mlp_loss_step": ["ltr_mlp_pairwise_f32"],
        "mlp_scores": ["ltr_mlp_scores_f32"],
    },
    "F46": {
        "scorer": ["ltr_mlp_rows_scores_f32", "ltr_mlp_rows_grad_f32"],
        "scorer-nograd": ["ltr_mlp_rows_scores_f32"],
        "score": ["ltr_mlp_rows_scores_f32", "ltr_mlp_rows_grad_f32"],
        "score-nograd": ["ltr_mlp_scores_f32"],
        "hinge": ["ltr_mlp_pairwise_f32"],
        "listnet": ["ltr_mlp_listwise_f32"],
        "listmle": ["ltr_mlp_listwise_f32"],
        "mlp_loss_step": ["raises ValueError"],
        "mlp_scores": ["raises ValueError"],
    },
    "F148": {
        "scorer": ["ltr_mlp_rows_scores_f32", "ltr_mlp_rows_grad_f32"],
        "scorer-nograd": ["ltr_mlp_rows_scores_f32"],
        "score": ["ltr_mlp_rows_scores_f32", "ltr_mlp_rows_grad_f32"],
        "score-nograd": ["ltr_mlp_scores_f32"],
        "hinge": ["ltr_mlp_pairwise_f32"],
        "listnet": ["ltr_mlp_listwise_f32"],
        "listmle": ["ltr_mlp_listwise_f32"],
        "mlp_loss_step": ["ltr_mlp_pairwise_f32"],
        "mlp_scores": ["ltr_mlp_scores_f32"],
    },
    "F224": {
        "scorer": ["ltr_mlp_rows_scores_f32", "ltr_mlp_rows_grad_f32"],
        "scorer-nograd": ["ltr_mlp_rows_scores_f32"],
        "score": ["ltr_mlp_rows_scores_f32", "ltr_mlp_rows_grad_f32"],
        "score-nograd": ["ltr_mlp_scores_f32"],
        "hinge": ["ltr_mlp_pairwise_f32"],
        "listnet": ["ltr_mlp_listwise_f32"],
        "listmle": ["ltr_mlp_listwise_f32"],
        "mlp_loss_step": ["ltr_mlp_pairwise_f32"],
        "mlp_scores": ["ltr_mlp_scores_f32"],
    },
    "F228": {
        "scorer": ["ltr_mlp_wide_scores_f32", "ltr_mlp_wide_grad_f32"],
        "scorer-nograd": ["ltr_mlp_wide_scores_f32"],
        "score": ["ltr_mlp_wide_scores_f32", "ltr_mlp_wide_grad_f32"],
        "score-nograd": ["ltr_mlp_wide_scores_f32"],
        "hinge": ["ltr_mlp_wide_scores_f32", "ltr_mlp_wide_grad_f32"],
        "listnet": ["ltr_mlp_wide_scores_f32", "ltr_mlp_wide_grad_f32"],
        "listmle": ["ltr_mlp_wide_scores_f32", "ltr_mlp_wide_grad_f32"],
        "mlp_loss_step": ["raises ValueError"],
        "mlp_scores": ["raises ValueError"],
    },
    "F700": {
        "scorer": ["ltr_mlp_wide_scores_f32", "ltr_mlp_wide_grad_f32"],
        "scorer-nograd": ["ltr_mlp_wide_scores_f32"],
        "score": ["ltr_mlp_wide_scores_f32", "ltr_mlp_wide_grad_f32"],
        "score-nograd": ["ltr_mlp_wide_scores_f32"],
        "hinge": ["ltr_mlp_wide_scores_f32", "ltr_mlp_wide_grad_f32"],
        "listnet": ["ltr_mlp_wide_scores_f32", "ltr_mlp_wide_grad_f32"],
        "listmle": ["ltr_mlp_wide_scores_f32", "ltr_mlp_wide_grad_f32"],
        "mlp_loss_step": ["raises ValueError"],
        "mlp_scores": ["raises ValueError"],
    },
    "F708": {
        "scorer": ["torch"],
        "scorer-nograd": ["torch"],
        "score": ["torch"],
        "score-nograd": ["torch"],
        "hinge": ["torch"],
        "listnet": ["torch"],
        "listmle": ["torch"],
        "mlp_loss_step": ["raises ValueError"],
        "mlp_scores": ["raises ValueError"],
    },
    "L130": {
        "scorer": ["ltr_mlp_rows_scores_f32", "ltr_mlp_rows_grad_f32"],
        "scorer-nograd": ["ltr_mlp_rows_scores_f32"],
        "score": ["ltr_mlp_rows_scores_f32", "ltr_mlp_rows_grad_f32"],
        "score-nograd": ["ltr_mlp_scores_f32"],
        "hinge": ["ltr_mlp_pairwise_f32"],
        "listnet": ["ltr_mlp_listwise_f32"],
        "listmle": ["ltr_mlp_listwise_f32"],
        "mlp_loss_step": ["ltr_mlp_pairwise_f32"],
        "mlp_scores": ["ltr_mlp_scores_f32"],
    },
    "L260": {
        "scorer": ["ltr_mlp_rows_scores_f32", "ltr_mlp_rows_grad_f32"],
        "scorer-nograd": ["ltr_mlp_rows_scores_f32"],
        "score": ["ltr_mlp_rows_scores_f32", "ltr_mlp_rows_grad_f32"],
        "score-nograd": ["ltr_mlp_rows_scores_f32"],
        "hinge": ["ltr_mlp_rows_scores_f32", "ltr_mlp_rows_grad_f32"],
        "listnet": ["ltr_mlp_rows_scores_f32", "ltr_mlp_rows_grad_f32"],
        "listmle": ["ltr_mlp_rows_scores_f32", "ltr_mlp_rows_grad_f32"],
        "mlp_loss_step": ["ltr_mlp_rows_scores_f32", "ltr_mlp_rows_grad_f32"],
        "mlp_scores": ["ltr_mlp_rows_scores_f32"],
    },
    "H65x3": {
        "scorer": ["torch"],
        "scorer-nograd": ["torch"],
        "score": ["torch"],
        "score-nograd": ["torch"],
        "hinge": ["torch"],
        "listnet": ["torch"],
        "listmle": ["torch"],
        "mlp_loss_step": ["raises ValueError"],
        "mlp_scores": ["raises ValueError"],
    },
    "H4x17": {
        "scorer": ["torch"],
        "scorer-nograd": ["torch"],
        "score": ["torch"],
        "score-nograd": ["torch"],
        "hinge": ["torch"],
        "listnet": ["torch"],
        "listmle": ["torch"],
        "mlp_loss_step": ["raises ValueError"],
        "mlp_scores": ["raises ValueError"],
    },
    "xgrad": {
        "scorer": ["torch"],
        "scorer-nograd": ["torch"],
        "score": ["torch"],
        "score-nograd": ["ltr_mlp_scores_f32"],
        "hinge": ["ltr_mlp_pairwise_f32"],
        "listnet": ["ltr_mlp_listwise_f32"],
        "listmle": ["ltr_mlp_listwise_f32"],
        "mlp_loss_step": ["ltr_mlp_pairwise_f32"],
        "mlp_scores": ["ltr_mlp_scores_f32"],
    },
    "autocast": {
        "scorer": ["torch"],
        "scorer-nograd": ["torch"],
        "score": ["torch"],
        "score-nograd": ["ltr_mlp_scores_f32"],
        "hinge": ["ltr_mlp_pairwise_f32"],
        "listnet": ["ltr_mlp_listwise_f32"],
        "listmle": ["ltr_mlp_listwise_f32"],
        "mlp_loss_step": ["ltr_mlp_pairwise_f32"],
        "mlp_scores": ["ltr_mlp_scores_f32"],
    },
    "L130-F148": {
        "scorer": ["ltr_mlp_rows_scores_f32", "ltr_mlp_rows_grad_f32"],
        "scorer-nograd": ["ltr_mlp_rows_scores_f32"],
        "score": ["ltr_mlp_rows_scores_f32", "ltr_mlp_rows_grad_f32"],
        "score-nograd": ["ltr_mlp_rows_scores_f32"],
        "hinge": ["ltr_mlp_rows_scores_f32", "ltr_mlp_rows_grad_f32"],
        "listnet": ["ltr_mlp_rows_scores_f32", "ltr_mlp_rows_grad_f32"],
        "listmle": ["ltr_mlp_rows_scores_f32", "ltr_mlp_rows_grad_f32"],
        "mlp_loss_step": ["ltr_mlp_rows_scores_f32", "ltr_mlp_rows_grad_f32"],
        "mlp_scores": ["ltr_mlp_rows_scores_f32"],
    },
    "bf16-F12": {
        "scorer": ["ltr_mlp_bf16_scores", "ltr_mlp_bf16_grad"],
        "scorer-nograd": ["ltr_mlp_bf16_scores"],
        "score": ["ltr_mlp_bf16_scores", "ltr_mlp_bf16_grad"],
        "score-nograd": ["ltr_mlp_bf16_scores"],
        "hinge": ["ltr_mlp_bf16_scores", "ltr_mlp_bf16_grad"],
        "listnet": ["ltr_mlp_bf16_scores", "ltr_mlp_bf16_grad"],
        "listmle": ["ltr_mlp_bf16_scores", "ltr_mlp_bf16_grad"],
        "mlp_loss_step": ["ltr_mlp_pairwise_f32"],
        "mlp_scores": ["ltr_mlp_scores_f32"],
    },
    "bf16-F228": {
        "scorer": ["raises ValueError"],
        "scorer-nograd": ["raises ValueError"],
        "score": ["raises ValueError"],
        "score-nograd": ["raises ValueError"],
        "hinge": ["raises ValueError"],
        "listnet": ["raises ValueError"],
        "listmle": ["raises ValueError"],
        "mlp_loss_step": ["raises ValueError"],
        "mlp_scores": ["raises ValueError"],
    },
    "bf16-L260": {
        "scorer": ["ltr_mlp_bf16_scores", "ltr_mlp_bf16_grad"],
        "scorer-nograd": ["ltr_mlp_bf16_scores"],
        "score": ["ltr_mlp_bf16_scores", "ltr_mlp_bf16_grad"],
        "score-nograd": ["ltr_mlp_bf16_scores"],
        "hinge": ["ltr_mlp_bf16_scores", "ltr_mlp_bf16_grad"],
        "listnet": ["ltr_mlp_bf16_scores", "ltr_mlp_bf16_grad"],
        "listmle": ["ltr_mlp_bf16_scores", "ltr_mlp_bf16_grad"],
        "mlp_loss_step": ["ltr_mlp_bf16_scores", "ltr_mlp_bf16_grad"],
        "mlp_scores": ["ltr_mlp_rows_scores_f32"],
    },
    "F700-L260": {
        "scorer": ["ltr_mlp_wide_scores_f32", "ltr_mlp_wide_grad_f32"],
        "scorer-nograd": ["ltr_mlp_wide_scores_f32"],
        "score": ["ltr_mlp_wide_scores_f32", "ltr_mlp_wide_grad_f32"],
        "score-nograd": ["ltr_mlp_wide_scores_f32"],
        "hinge": ["ltr_mlp_wide_scores_f32", "ltr_mlp_wide_grad_f32"],
        "listnet": ["ltr_mlp_wide_scores_f32", "ltr_mlp_wide_grad_f32"],
        "listmle": ["ltr_mlp_wide_scores_f32", "ltr_mlp_wide_grad_f32"],
        "mlp_loss_step": ["raises ValueError"],
        "mlp_scores": ["raises ValueError"],
    },
}


def _predicted(fused, caller, case, route):
    """What EXPECTED holds for a caller whose route function answers `route`."""
    kind, grad, loss = CALLERS[caller]
    F, (H1, H2) = case["F"], case["hidden"]
    module = kind in ("scorer", "score", "loss")
    if route == fused._TORCH:
        if not module:
            return ["raises ValueError"]            # the functions have no torch layers
        # (the layers' fp32 weights meet the batch as it is: another dtype raises outside autocast)
        return ["torch"] if case["dtype"] == "float32" else ["raises RuntimeError"]
    if route == fused._FUSED:
        return ["ltr_mlp_pairwise_f32" if loss == "hinge" else "ltr_mlp_listwise_f32"]
    if route == fused._PER_QUERY:
        return ["ltr_mlp_scores_f32"]
    family = fused._ROUTE_FAMILY[route]
    if route == fused._BF16 and not family.takes((F + 7) & ~7, H1, H2):
        return ["raises ValueError"]                # no fallback from the bf16 kernels
    backward = kind in ("loss", "step") or (module and grad)
    return [family.scores, family.grad] if backward else [family.scores]


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_route_function_states_the_recorded_table(name):
    from pytorchltr_amd import fused
    case = CASES[name]
    F, L, (H1, H2) = case["F"], case["L"], case["hidden"]
    for caller, (kind, grad, loss) in CALLERS.items():
        lkind = fused._resolve_loss(loss)[0] if loss else None
        plan = True
        if isinstance(lkind, fused._ListwiseKind):
            plan = fused.mlp_listwise_supported(lkind, 2, L, fused._f4(F) if kind == "loss" else F, H1, H2)
        route = fused._mlp_route(kind, getattr(torch, case["dtype"]), 3, True, case["xgrad"], grad, case["autocast"],
                                 L, F, H1, H2, lkind, plan)
        assert _predicted(fused, caller, case, route) == EXPECTED[name][caller], (caller, route)


def test_what_is_no_batch_on_the_device_takes_the_torch_route():
    from pytorchltr_amd import fused
    for caller in ("scorer", "score", "loss", "step", "scores"):
        for dim, cuda, L in ((2, True, 5), (3, False, 5), (3, True, 0)):
            assert fused._mlp_route(caller, torch.float32, dim, cuda, False, True, False, L, 8, 4, 3, fused._C.HINGE) \
                == fused._TORCH
