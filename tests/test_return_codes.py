"""CPU tier: the return code of every exported entry point for a grid of invalid arguments.

Each entry point checks its arguments on the host, in an order of its own, before anything is launched; the order
decides which code a caller sees when several arguments are wrong.  The grid below takes the declarations of
include/ltr_hip.h, starts from valid arguments with dummy non-NULL device pointers, and breaks one argument
(a NULL pointer, B = -1 or 0, L = 0, 4097 or 2^24 + 1, an unknown loss kind or label dtype, k = -1, a one-byte
workspace) or two of them at once.  EXPECTED holds the codes, one character per call in the order of _cases():
'0'..'7' for 0 .. -7, and for the size queries '0' or '+' (non-zero).  A '.' marks a call that gets past every
check and would launch (recorded without a GPU, where the launch fails); it is not made.  Left out: the debug
hooks, functions without arguments, and the overlap / mailbox handle functions (a dummy handle cannot stand in
for one; handle arguments are NULL everywhere else).  The table was recorded from the library before its entry
points shared their checks (metric_entry, check_kind, check_lists in csrc/).
"""
import itertools
import os
import re

import pytest

P = 256                                       # dummy non-NULL device pointer: no call below dereferences it
_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ltr_hip.h")
_SKIP = re.compile(r"^ltr_(debug_|overlap_|mailbox_)")
_HANDLES = {"stream", "overlap", "mailbox", "comm", "handle", "allreduce_fn"}       # always NULL
# valid values of the integer / float arguments by name (anything else: 1)
_VALID = {"kind": 0, "rel_dtype": 0, "B": 2, "L": 16, "F": 8, "k": 10, "H1": 4, "H2": 2, "Q": 4, "n_probs": 5,
          "elem_bytes": 4, "owners": 64, "dpt": 1, "msplit": 1, "op": 1, "use_seed": 0, "seed": 0, "slot": 0,
          "pending_B": 0, "workspace_bytes": 1 << 40, "pending_scale_stride": 0}
_BAD = {"B": (-1, 0), "L": (0, 4097, (1 << 24) + 1), "kind": (7,), "rel_dtype": (7,), "k": (-1,),
        "workspace_bytes": (1,)}


def _declarations():
    with open(_HEADER) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    out = []
    for ret, name, params in re.findall(r"\b(int|size_t)\s+(ltr_\w+)\s*\(([^)]*)\)\s*;", text):
        params = [p.strip() for p in params.split(",")]
        if params == ["void"] or _SKIP.match(name):
            continue
        args = []
        for p in params:
            pname = re.findall(r"\w+", p)[-1]
            args.append((pname, "*" in p, re.sub(r"\b(const|unsigned)\b", "", p).split()[0]))
        if _cases(args):
            out.append((name, ret, args))
    return out


def _cases(args):
    """Each case: {argument index: value} over the valid arguments -- single breaks, then pairs."""
    single = []
    for i, (name, is_ptr, _) in enumerate(args):
        if is_ptr and name not in _HANDLES:
            single.append((i, None))
        for v in _BAD.get(name, ()):
            single.append((i, v))
    cases = [dict([c]) for c in single]
    cases += [dict([a, b]) for a, b in itertools.combinations(single, 2) if a[0] != b[0]]
    return cases


def _call(fn, args, case):
    vals = []
    for i, (name, is_ptr, ctype) in enumerate(args):
        if i in case:
            vals.append(case[i])
        elif is_ptr:
            vals.append(None if name in _HANDLES else P)
        elif ctype in ("float", "double"):
            vals.append(1.0)
        else:
            vals.append(_VALID.get(name, 1))
    return fn(*vals)


def _code(ret, rc):
    if ret == "size_t":                       # the workspace / size queries: 0 for invalid arguments
        return "0" if rc == 0 else "+"
    return "." if rc > 0 else str(-rc)


EXPECTED = {
    "ltr_pairwise_loss_f32": "31131202441.33332323333131202441131202441132323333202441122222244002244441",
    "ltr_pairwise_loss_f32_cfg": "31131202441.33333333333131202441131202441133333333202441122222244002244441",
    "ltr_pairwise_loss_workspace_bytes": "00000000000000000",
    "ltr_pairwise_loss_ws_f32":
        "31131202441...3333333333333131202441111312024411113333333333202441111222222224400002222444444441"
        "11...",
    "ltr_scale_rows_f32": "11202..1120211120211122222000211",
    "ltr_scale_rows_uniform_f32": "11202..1120211120211122222000211",
    "ltr_pairwise_loss_f64": "31131202441.33333333333131202441131202441133333333202441122222244002244441",
    "ltr_scale_rows_f64": "11202..1120211120211122222000211",
    "ltr_rank_by_score_f32": "11202441120244120244122222440244",
    "ltr_dcg_f32": "11312024421131202442131202442133333333202442122222244202224242",
    "ltr_arp_f32": "113120244113120244131202441333333320244122222440244",
    "ltr_rank_by_score_tie_f32": "11.20244111202441120244120244122222440244",
    "ltr_dcg_tie_f32": "1131.202442113112024421311202442133333333312024421202442122222244202224242",
    "ltr_arp_tie_f32": "1131.202441131120244131120244133333333120244120244122222440244",
    "ltr_rank_by_score_seed_f32": "11.20244111202441120244120244122222440244",
    "ltr_dcg_seed_f32": "1131.202442113112024421311202442133333333312024421202442122222244202224242",
    "ltr_arp_seed_f32": "1131.202441131120244131120244133333333120244120244122222440244",
    "ltr_sort_workspace_bytes": "0+0+00000+0",
    "ltr_rank_by_score_long_f32": "11..202.41..111202141111120214111.202.41..202.41..22222220400022215544411.",
    "ltr_dcg_long_f32":
        "1131..202.421..13111202142111311120214211133333333333311202142111.202.421..202.421..222222220420"
        "0022222155244422211.",
    "ltr_arp_long_f32":
        "1131..202.41..1311120214111311120214111333333333331120214111.202.41..202.41..2222222040002221554"
        "4411.",
    "ltr_listwise_softmax_f32": "1131202..1.13120211113120211113333333320211112222220000221.1.1",
    "ltr_mask_padded_values_f32": "11202..1120211120211122222000211",
    "ltr_batch_pairs": "1202..120211122222000211",
    "ltr_plackettluce_keys_f32": "111202..111202111120211120211122222000211",
    "ltr_pbm_clicks": "11111202..1111112021111111202111111202111112021111202111122222200002211111",
    "ltr_collate_pad_f32": "1111.202..111111120211111111202111111120211111120211111202..111222222200000222111111111",
    "ltr_collate_pad_csr_f32":
        "111111.202..111111111202111111111120211111111120211111111202111111120211111120211111202..1112222"
        "22200000222111111111",
    "ltr_linear_workspace_bytes": "00+++000000",
    "ltr_linear_fused_plan": "00000000000000000",
    "ltr_linear_pairwise_f32":
        "311.131.2.2441.11553333333232333311551113112.244111155113112.244111155131.2.2441.11553112.244111"
        "155332323333115512.2441111552.2441.1155222222222244..11..222222441155441155111551155111115",
    "ltr_linear_partials_f32":
        "311.131202441.1333333333333331113120244111113120244111131202441.13120244111333333333202441112222"
        "22244000222444444111",
    "ltr_linear_reduce_f32": "1.2.1112.112.1122111",
    "ltr_linear_reduce_bcast_f32": "112.1112.11211122111",
    "ltr_linear_reduce_loss_f32": "1.12.11.112.11112.11.2.11.22211.111",
    "ltr_linear_reduce_accum_f32": "1.12.11.112.11112.11.2.11.22211.111",
    "ltr_linear_step_f32":
        "311.131.2.244115533333332323331551113112.2441155113112.2441155131.2.24411553112.2441155332323331"
        "5512.24411552.24411552222222244.1..222241554155155115",
    "ltr_linear_sgd_step_f32":
        "311.131.2.244115531333332323331551113112.244115511111212111111131.2.24411553112.2441155332323331"
        "5512.24411552.24411552222222244.1..222241554155155115",
    "ltr_linear_sgd_lazy_step_f32":
        "311.13120244115531333320233115511131202441155111121211111113120244115531202441155320233115520244"
        "115522222222001100222211551155111115",
    "ltr_linear_sgd_flush_f32": "000200000002000000200000200000222000000000",
    "ltr_linear_sgd_lazy_step_dp_f32":
        "311.131202441155.313333202331155311131202441155111112121111111131202441155.312024411551320233115"
        "53202441155122222222200110002222211554115541111111555",
    "ltr_linear_sgd_flush_dp_f32": "0002000000002000000020000002000000222200000000000000",
    "ltr_linear_lazy_rows_reduce_f32": "020000002000000222200000000000000",
    "ltr_mlp_workspace_bytes": "00",
    "ltr_mlp_pairwise_f32":
        "31111111131.2.2441.1.55333333333332324433333311111113112.244111111111111311212441111111111131121"
        "2441111111111311212441111111113112124411111111311212441111111311212441111113112.2441111113323244"
        "33333312.2441111112.2441.1.55222222222244..1...222222444444444444111111.55111555",
    "ltr_mlp_scores_f32":
        "111111112024411111111202441111111212441111112124411111212441111212441112124411212441202441222224"
        "40244",
    "ltr_linear_scores_f32": "11..202..111120211111202111.202..1202..122222000211",
    "ltr_linear_grad_workspace_bytes": "000++000000",
    "ltr_linear_grad_f32": "11.2.2..155112.21111112.2111112.2..1552222222..1..222155155115",
}


@pytest.fixture(scope="module")
def lib():
    from pytorchltr_amd import _C
    from pytorchltr_amd.build import build_extension
    if not os.environ.get("LTR_HIP_LIB"):
        build_extension()
    return _C.lib()


def test_every_entry_point_is_pinned():
    assert sorted(name for name, _, _ in _declarations()) == sorted(EXPECTED)


def _lazy_step(lib, B, pending_B, ws_for, dp, L=72, F=136):
    """The lazy step with dummy pointers, a batch of B queries, pending_B pending and a workspace sized for `ws_for` queries."""
    ws_bytes = lib.ltr_linear_workspace_bytes(ws_for, L, F)
    head = (0, 1.0, P, P, P, P, 0, P, B, L, F, 0.05, P, P, P, ws_bytes, pending_B)
    if dp:
        return lib.ltr_linear_sgd_lazy_step_dp_f32(*head, 0.0, None, 0, None, None)
    return lib.ltr_linear_sgd_lazy_step_f32(*head, None)


@pytest.mark.parametrize("dp", [False, True], ids=["lazy_step", "lazy_step_dp"])
def test_lazy_step_checks_the_pending_batch_too(lib, dp):
    """The pending batch may have another size than this call's: a negative pending_B is LTR_ERR_SHAPE, and the ONE workspace
    has to take the larger of the two batches -- LTR_ERR_WORKSPACE whichever of them it is too small for (before any launch:
    every pointer here is a dummy)."""
    ERR_SHAPE, ERR_WORKSPACE = -2, -5
    assert lib.ltr_linear_workspace_bytes(300, 72, 136) > lib.ltr_linear_workspace_bytes(77, 72, 136) > 0
    assert _lazy_step(lib, 77, -1, 300, dp) == ERR_SHAPE
    assert _lazy_step(lib, 77, 300, 77, dp) == ERR_WORKSPACE          # large enough for B, not for the larger pending batch
    assert _lazy_step(lib, 300, 77, 77, dp) == ERR_WORKSPACE          # ... and with B and pending_B swapped
    assert _lazy_step(lib, 0, 300, 77, dp) == ERR_WORKSPACE           # the empty batch that only applies the pending update


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_return_codes(lib, name):
    decl = {n: (r, a) for n, r, a in _declarations()}
    ret, args = decl[name]
    fn = getattr(lib, name)
    want = EXPECTED[name]
    cases = _cases(args)
    assert len(want) == len(cases), name
    got = []
    for case, w in zip(cases, want):
        if w == ".":
            got.append(".")
            continue
        got.append(_code(ret, _call(fn, args, case)))
    assert "".join(got) == want
