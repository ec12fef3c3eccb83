"""CPU tier of the Linear(F, 1) scorer on bf16 feature batches (include/ltr_linear_bf16.h; fused._linear_route): the
boundary, the argument errors (decided on the host, in front of any launch), the plan of the fused step, the route
function on plain values and the code objects.  Nothing here gets as far as a launch."""
import ctypes
import os
import re

import pytest
import torch

P = 256                                        # dummy non-NULL, 16-byte aligned device pointer: never dereferenced below
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_NULL, ERR_SHAPE, ERR_KIND, ERR_TOO_LONG, ERR_WORKSPACE = 0, -1, -2, -3, -4, -5
KINDS = range(7)


@pytest.fixture(scope="module")
def lib():
    from pytorchltr_amd import _C
    from pytorchltr_amd.build import build_extension
    if not os.environ.get("LTR_HIP_LIB"):
        build_extension()
    return _C.lib()


# ---- boundary ----
def test_error_codes_are_the_headers(lib):
    text = open(os.path.join(ROOT, "include", "ltr_hip.h")).read()
    for name, code in (("LTR_ERR_NULL", ERR_NULL), ("LTR_ERR_SHAPE", ERR_SHAPE), ("LTR_ERR_KIND", ERR_KIND),
                       ("LTR_ERR_LIST_TOO_LONG", ERR_TOO_LONG), ("LTR_ERR_WORKSPACE", ERR_WORKSPACE)):
        assert re.search(r"#define %s \(%d\)" % (name, code), text), name


def test_header_exports_and_ctypes_table_agree(lib):
    import subprocess
    from pytorchltr_amd import _C, _codeobj
    from pytorchltr_amd.build import LIB_PATH
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltr_linear_bf16.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(ltr_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_C.LINEAR_BF16_SIGNATURES)
    assert len(declared) == 6
    for name, (_, argtypes) in _C.LINEAR_BF16_SIGNATURES.items():
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr), name          # exported by the library
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1).strip()
        assert len(proto.split(",")) == len(argtypes), name                     # as many arguments as the prototype
    # argument for argument the fp32 prototypes
    for ours, theirs in (("ltr_linear_scores_bf16", "ltr_linear_scores_f32"), ("ltr_linear_grad_bf16", "ltr_linear_grad_f32"),
                         ("ltr_linear_grad_workspace_bytes_bf16", "ltr_linear_grad_workspace_bytes"),
                         ("ltr_linear_bf16_plan", "ltr_linear_fused_plan"), ("ltr_linear_partials_bf16", "ltr_linear_partials_f32"),
                         ("ltr_collate_pad_bf16", "ltr_collate_pad_f32")):
        assert _C.LINEAR_BF16_SIGNATURES[ours] == _C.SIGNATURES[theirs]
    others = (set(_C.SIGNATURES) | set(_C.EVAL_SIGNATURES) | set(_C.LISTWISE_SIGNATURES) | set(_C.LONGPAIR_SIGNATURES)
              | set(_C.MLP_ROWS_SIGNATURES) | set(_C.MLP_WIDE_SIGNATURES) | set(_C.MLP_BF16_SIGNATURES) | set(_C.SCHED_SIGNATURES))
    assert not set(_C.LINEAR_BF16_SIGNATURES) & others
    # the library's exports: the bf16 Linear symbols are the declared ones; nothing internal leaks
    try:
        tool = _codeobj._tool("llvm-readelf")
    except FileNotFoundError as exc:
        pytest.skip(str(exc))
    out = subprocess.run([tool, "--dyn-syms", "-W", LIB_PATH], check=True, stdout=subprocess.PIPE).stdout.decode()
    defined = "\n".join(ln for ln in out.splitlines() if " FUNC " in ln and " GLOBAL " in ln and " UND " not in ln)
    exported = set(re.findall(r"\b(ltr_[a-z0-9_]+)\b", defined))
    ours = {s for s in exported if re.search(r"linear_.*bf16|collate_pad_bf16", s)}
    assert sorted(ours) == sorted(_C.LINEAR_BF16_SIGNATURES)
    assert not [s for s in exported if s.startswith("ltr_internal_")]


def test_the_main_header_and_the_version_are_untouched(lib):
    from pytorchltr_amd import _C
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltr_hip.h")).read(), flags=re.S)
    assert "bf16" not in main
    assert not [k for k in _C.SIGNATURES if "bf16" in k]
    assert len(_C.SIGNATURES) == 80 and lib.ltr_version() == 114


# ---- argument errors, no launch ----
def _scores(lib, B=2, L=10, F=8, X=P, W=P, out=P):
    return lib.ltr_linear_scores_bf16(X, W, P, P, B, L, F, out, None)


def _grad(lib, B=2, L=10, F=8, X=P, g=P, out=P, ws=P, ws_bytes=1 << 40):
    return lib.ltr_linear_grad_bf16(X, g, P, B, L, F, out, ws, ws_bytes, None)


def _partials(lib, kind=0, B=2, L=10, F=8, X=P, W=P, rel=P, rel_dtype=0, n=P, loss=P, part=P):
    return lib.ltr_linear_partials_bf16(kind, 1.0, X, W, P, rel, rel_dtype, n, B, L, F, loss, None, part, None)


def _collate(lib, Q=3, B=2, L=10, F=8, xs=P, out=P):
    return lib.ltr_collate_pad_bf16(xs, P, P, P, None, Q, B, L, F, out, P, P, None)


@pytest.mark.parametrize("change", [dict(F=12), dict(F=4), dict(F=1032), dict(F=0), dict(L=0), dict(L=-3), dict(B=-1),
                                    dict(B=1 << 20, L=1 << 12)])
def test_shape_errors_come_first(lib, change):
    # (every pointer NULL as well: the shape is judged first)
    assert _scores(lib, X=None, W=None, out=None, **change) == ERR_SHAPE
    assert _grad(lib, X=None, g=None, out=None, ws=None, ws_bytes=0, **change) == ERR_SHAPE
    assert _partials(lib, X=None, W=None, rel=None, n=None, loss=None, part=None, **change) == ERR_SHAPE
    assert lib.ltr_linear_grad_workspace_bytes_bf16(change.get("B", 2), change.get("L", 10), change.get("F", 8)) == 0
    for kind in KINDS:
        assert lib.ltr_linear_bf16_plan(kind, change.get("B", 2), change.get("L", 10), change.get("F", 8)) == 0


def test_null_empty_and_workspace(lib):
    for bad in (dict(X=None), dict(W=None), dict(out=None)):
        assert _scores(lib, **bad) == ERR_NULL
    assert _scores(lib, B=0, X=None, W=None, out=None) == OK
    assert _grad(lib, out=None) == ERR_NULL
    assert _grad(lib, B=0, out=None) == ERR_NULL                            # dW_db in front of the empty batch
    assert _grad(lib, X=None, ws=None, ws_bytes=0) == ERR_NULL              # NULL in front of the workspace
    assert _grad(lib, g=None, ws=None, ws_bytes=0) == ERR_NULL
    need = lib.ltr_linear_grad_workspace_bytes_bf16(2, 10, 8)
    assert need == 2 * 12 * 4                                               # one partial vector [dW | db | pad] per query
    assert lib.ltr_linear_grad_workspace_bytes_bf16(2, 257, 136) == 2 * 2 * 140 * 4
    assert _grad(lib, ws_bytes=need - 1) == ERR_WORKSPACE
    assert _grad(lib, ws=None) == ERR_WORKSPACE
    assert lib.ltr_linear_grad_workspace_bytes_bf16(0, 10, 8) == 0
    for bad in (dict(X=None), dict(W=None), dict(rel=None), dict(n=None), dict(loss=None), dict(part=None)):
        assert _partials(lib, **bad) == ERR_NULL
    assert _partials(lib, B=0, X=None, W=None, rel=None, n=None, loss=None, part=None) == OK
    assert _partials(lib, kind=7) == ERR_KIND and _partials(lib, kind=-1) == ERR_KIND
    assert _partials(lib, rel_dtype=3) == ERR_KIND
    assert _partials(lib, kind=7, F=12) == ERR_KIND                         # the kind in front of the shape
    # the collate: a copy, any F
    assert _collate(lib, F=5, B=0) == OK and _collate(lib, B=0, xs=None, out=None) == OK
    assert _collate(lib, xs=None) == ERR_NULL and _collate(lib, out=None) == ERR_NULL
    for bad in (dict(F=0), dict(L=0), dict(B=-1), dict(Q=0)):
        assert _collate(lib, **bad) == ERR_SHAPE


@pytest.mark.parametrize("kind", KINDS)
def test_partials_off_the_plan(lib, kind):
    assert _partials(lib, kind=kind, L=257, F=136) == ERR_TOO_LONG
    assert _partials(lib, kind=kind, L=4100, F=8) == ERR_TOO_LONG
    assert _partials(lib, kind=kind, L=200, F=704) == ERR_SHAPE             # 88 column vectors: 5 rows a sweep, 80 rows
    assert _partials(lib, kind=kind, L=65, F=1024) == ERR_SHAPE
    assert _partials(lib, kind=kind, L=300, F=12) == ERR_SHAPE              # the shape in front of the length
    # ... and on it: as far as the NULL check
    for L, F in ((256, 224), (128, 512), (64, 1024), (80, 704), (1, 8)):
        assert lib.ltr_linear_bf16_plan(kind, 2, L, F) == 1
        assert _partials(lib, kind=kind, L=L, F=F, X=None) == ERR_NULL


# ---- the plan ----
def _reach(F):
    """Longest list the tile takes at F features by its sweeps alone: 16 sweeps of floor(512 / (F / 8)) rows."""
    return min(256, 16 * (512 // (F // 8)))


@pytest.mark.parametrize("kind", KINDS)
def test_plan(lib, kind):
    plan = lib.ltr_linear_bf16_plan
    for F in range(8, 1025, 8):
        taken = [L for L in range(1, 258) if plan(kind, 4, L, F) == 1]
        assert taken == list(range(1, len(taken) + 1)), F                   # (L, F) on the plan: (L - 1, F) too
        top = len(taken)
        assert top == _reach(F), (F, top)                                   # the documented rule, and no LDS surprise
        if F <= 224:
            assert top == 256, F
        if F <= 512:
            assert top >= 128, F
    for F in (1, 4, 12, 44, 100, 220, 700):                                 # never F % 8 != 0
        assert not any(plan(kind, 4, L, F) for L in (1, 8, 64, 256)), F
    assert plan(kind, 0, 10, 8) == 0 and plan(kind, 4, 10, 1032) == 0
    assert plan(7, 4, 10, 8) == 0 and plan(-1, 4, 10, 8) == 0
    # it does not depend on the batch size
    assert plan(kind, 1, 256, 136) == plan(kind, 1 << 20, 256, 136) == 1


# ---- the route ----
def test_route_on_plain_values(lib):
    from pytorchltr_amd import _C, fused
    from pytorchltr_amd._autograd import LongKind
    bf, f32 = torch.bfloat16, torch.float32
    route = fused._linear_route
    FUSED, PIECES, TODAY = fused._LIN_BF16_FUSED, fused._LIN_BF16_PIECES, fused._LIN_F32
    assert (FUSED, PIECES, TODAY) == ("bf16 fused", "bf16 pieces", "f32 fused")
    for kind in KINDS:
        for caller in ("step", "module"):
            # on the plan (F = 220 counts as its padded 224)
            for B, L, F in ((1024, 128, 136), (3, 1, 8), (4, 256, 224), (4, 128, 512), (300, 200, 220), (0, 10, 8)):
                assert route(caller, bf, 3, True, False, False, kind, B, L, F, cus=256) == FUSED, (kind, B, L, F)
            # off the plan
            for B, L, F in ((3, 257, 136), (2, 300, 704), (2, 1000, 224), (2, 200, 700)):
                assert route(caller, bf, 3, True, False, False, kind, B, L, F, cus=256) == PIECES, (kind, B, L, F)
            # long lists, opted in, past max_list_len()
            assert route(caller, bf, 3, True, False, False, LongKind(kind), 2, _C.max_list_len() + 4, 8, cus=256) == PIECES
            assert route(caller, bf, 3, True, False, False, LongKind(kind), 2, 100, 8, cus=256) == FUSED
            # everything that is not a bf16 data batch on the device: today's answers
            for args in ((f32, 3, True, False, False), (bf, 3, True, False, True), (bf, 3, True, True, False),
                         (bf, 3, False, False, False), (bf, 2, True, False, False), (torch.float16, 3, True, False, False),
                         (torch.float64, 3, True, False, False)):
                assert route(caller, *args, kind, 1024, 128, 136, cus=256) == TODAY, args
    # the listwise kinds have no bf16 fused step: on the plan of the fp32 one they cast, off it the bf16 scorer runs
    listnet = fused._ListwiseKind(_C.LISTWISE_LISTNET)
    assert route("step", bf, 3, True, False, False, listnet, 4, 10, 8, cus=256, listwise_plan=True) == fused._LIN_LISTWISE
    assert route("step", bf, 3, True, False, False, listnet, 4, 10, 8, cus=256, listwise_plan=False) == PIECES


def test_prefer_pieces_bf16_is_the_fp32_rule_without_the_exemptions(lib):
    from pytorchltr_amd import _C, fused
    # where the stand-alone loss has no split-query form the fused step stays, whatever the batch size
    for kind in KINDS:
        small = lib.ltr_pairwise_loss_workspace_bytes(kind, 4, 128) != 0
        assert fused._prefer_pieces(kind, 4, 128, 8, cus=256, exempt=False) == small
        assert not fused._prefer_pieces(kind, 0, 128, 8, cus=256, exempt=False)
        assert not fused._prefer_pieces(kind, 1024, 128, 8, cus=256, exempt=False)
        # ... and the fp32 rule is the same one behind the exemptions: the cluster / parts kernels keep the fused step
        assert fused._prefer_pieces(kind, 4, 128, 8, cus=256, plan=_C.PLAN_GENERAL) == small
        assert not fused._prefer_pieces(kind, 4, 128, 8, cus=256, plan=_C.PLAN_CLUSTER)
        assert not fused._prefer_pieces(kind, 4, 128, 8, cus=256, plan=_C.PLAN_PARTS)


def test_a_bf16_batch_is_judged_without_a_device():
    from pytorchltr_amd import fused
    x = torch.zeros(2, 3, 8, dtype=torch.bfloat16)
    assert not fused._bf16_batch(x)                                         # on the host
    assert fused._linear_route_of("step", x, 0) == fused._LIN_F32
    assert fused._padded_rows(x) is None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fused.linear_loss_step(x, torch.zeros(8), torch.zeros(1), torch.zeros(2, 3, dtype=torch.int64),
                               torch.tensor([3, 2]))


def test_ragged_queries_feature_dtype_arguments():
    from pytorchltr_amd.datasets.ragged import RaggedQueries
    x = torch.zeros(5, 6)
    y = torch.zeros(5, dtype=torch.int64)
    off = torch.tensor([0, 2, 5])
    with pytest.raises(ValueError, match="feature_dtype"):
        RaggedQueries(x, y, off, device="cpu", feature_dtype=torch.float16)
    with pytest.raises(ValueError, match="pad_features_to"):
        RaggedQueries(x, y, off, device="cpu", feature_dtype=torch.bfloat16, pad_features_to=4)
    with pytest.raises(ValueError, match="pad_features_to"):
        RaggedQueries(x, y, off, device="cpu", pad_features_to=8)
    with pytest.raises(ValueError, match="csr"):
        RaggedQueries(None, y, off, device="cpu", feature_dtype=torch.bfloat16,
                      csr=(torch.tensor([0, 1, 1, 2, 2, 3]), torch.tensor([0, 1, 2], dtype=torch.int32), torch.ones(3)))


# ---- code objects ----
def test_bf16_linear_kernels_keep_their_occupancy_and_nothing_in_scratch():
    from pytorchltr_amd import _codeobj
    from pytorchltr_amd.build import LIB_PATH, build_extension
    build_extension()
    try:
        recs = _codeobj.kernel_records(LIB_PATH)
    except FileNotFoundError as exc:          # no llvm tools on this machine
        pytest.skip(str(exc))
    ours = {}
    for r in recs:
        n = r.get("demangled", r["name"]).replace("(anonymous namespace)::", "")
        m = re.search(r"(linear_bf16_\w+?_kernel(?:<[^>]*>)?)", n)
        if m:
            ours[m.group(1)] = r
    # the declared occupancies (streaming kernels: csrc/ltr_scorer.inc; tile: csrc/ltr_linear_bf16.inc), as VGPR caps:
    # 512 / waves per SIMD, in eights
    caps = {"linear_bf16_scores_kernel<1>": 64, "linear_bf16_scores_kernel<2>": 80, "linear_bf16_grad_kernel": 64}
    for kind in KINDS:
        for ni, cap in ((5, 64), (10, 80), (16, 128)):
            caps["linear_bf16_tile_kernel<%d, %d>" % (kind, ni)] = cap
    assert sorted(ours) == sorted(caps)
    assert len(ours) == 24
    for key, r in ours.items():
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, (key, r)
        assert 0 < r["vgpr_count"] + r.get("agpr_count", 0) <= caps[key], (key, r)
        # eight waves per SIMD need <= 80 SGPRs as well
        if caps[key] == 64:
            assert r["sgpr_count"] <= 80, (key, r)
    # none of the names falls under the substring filters of tests/test_codeobj.py
    for key in ours:
        assert not any(k in key for k in ("linear_regtile", "linear_pairwise_kernel", "linear_parts_kernel", "linear_cluster_kernel"))
