"""CPU tier of the fused MLP step on a bf16 feature batch (include/ltr_mlp_step_bf16.h): where `fused._mlp_route` answers
_FUSED_BF16, that ltr_mlp_step_bf16_plan states the same limits, and the code-object records of mlp_tile_bf16_kernel
(no spill, two workgroups per CU)."""
import re

import pytest
import torch


def _route(caller="step", dtype=torch.bfloat16, L=128, F=160, hidden=(64, 16), kind=0, fuse=True, xgrad=False,
           autocast=False):
    from pytorchltr_amd import fused
    return fused._mlp_route(caller, dtype, 3, True, xgrad, True, autocast, L, F, *hidden, kind, True, fuse)


@pytest.mark.parametrize("change,taken", [
    ({}, True), ({"caller": "loss"}, True), ({"caller": "loss", "F": 154}, True),       # (the modules pad 154 to 160)
    ({"L": 129}, False), ({"F": 168}, False), ({"caller": "loss", "F": 161}, False), ({"hidden": (65, 16)}, False),
    ({"hidden": (64, 17)}, False), ({"fuse": False}, False), ({"xgrad": True}, False), ({"autocast": True}, False),
    ({"dtype": torch.float32}, False), ({"kind": None}, False), ({"caller": "score"}, False), ({"caller": "scorer"}, False),
])
def test_route_takes_the_fused_bf16_step_exactly_inside_its_limits(change, taken):
    from pytorchltr_amd import fused
    got = _route(**change)
    assert (got is fused._FUSED_BF16) == taken, (change, got)
    # off the route, and with the flag off everywhere, the answer is the one without the flag
    assert taken or got == _route(**dict(change, fuse=False))
    assert fused._ROUTE_FAMILY[fused._FUSED_BF16] is fused._MLP_BF16


def test_plan_agrees_with_the_routes_limits():
    from pytorchltr_amd import _C, fused
    from pytorchltr_amd.build import build_extension
    build_extension()
    lib = _C.lib()
    slots = [(_C.MLP_TRAIN_PAIRWISE, kind) for kind in range(7)] + [(_C.MLP_TRAIN_LISTWISE, _C.LISTWISE_LISTNET),
                                                                  (_C.MLP_TRAIN_LISTWISE, _C.LISTWISE_LISTMLE),
                                                                  (_C.MLP_TRAIN_LAMBDARANK, 0)]
    for L, F, H1, H2 in ((128, 160, 64, 16), (129, 160, 64, 16), (128, 168, 64, 16), (128, 224, 64, 16), (1, 8, 1, 1),
                         (128, 12, 4, 4), (128, 64, 65, 16), (128, 72, 64, 17), (33, 136, 50, 10), (0, 8, 4, 4)):
        for family, code in slots:
            assert lib.ltr_mlp_step_bf16_plan(family, code, 5, L, F, H1, H2) == \
                int(fused.mlp_step_bf16_supported(L, F, H1, H2)), (family, code, L, F, H1, H2)
    # an unknown code or family, an empty batch: off the plan
    assert not any(lib.ltr_mlp_step_bf16_plan(*head, 33, 136, 50, 10) for head in ((0, 7, 5), (3, 0, 5), (0, 0, 0)))
    assert lib.ltr_mlp_step_bf16_workspace_bytes(3, 136, 50, 10) == lib.ltr_mlp_workspace_bytes(3, 136, 50, 10) > 0


def test_kernels_do_not_spill_and_run_two_workgroups_per_cu():
    from pytorchltr_amd import _codeobj
    from pytorchltr_amd.build import LIB_PATH, build_extension
    build_extension()
    ours = {}
    for r in _codeobj.kernel_records(LIB_PATH):
        m = re.search(r"mlp_tile_bf16_kernel<(\d+), (\d+)>", r.get("demangled", r["name"]))
        if m:
            ours[(int(m.group(1)), int(m.group(2)))] = r
    # the seven pairwise kinds and the three row slots (16, 17, 18), two K-step buckets each
    assert sorted(ours) == sorted((kind, ks) for kind in list(range(7)) + [16, 17, 18] for ks in (2, 5))
    for key, r in ours.items():
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, (key, r)
        assert 0 < r.get("vgpr_count", 0) + r.get("agpr_count", 0) <= 256, (key, r)       # 512 a SIMD, two waves on it
