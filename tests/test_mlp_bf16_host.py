"""CPU tier of the MLP scorer on bf16 feature batches (include/ltr_mlp_bf16.h, fused.mlp_scores_bf16 /
fused.mlp_grad_bf16): the boundary, the argument errors (decided on the host, in front of any launch), the code
objects, the Python surface, and a numpy emulation of the kernels' arithmetic against the reference the GPU tier uses.
Nothing here gets as far as a launch.

Reference (`_case`, shared with tests/test_gpu_mlp_bf16.py): the three layers in torch float64 on the CPU, loss =
(s * g).sum(), autograd, as tests/test_gpu_mlp_rows.py::_case, on X rounded once to bf16 and on W1 rounded to bf16; the
gradient with respect to that rounded W1 is dW1.  Tolerances, those of that file: scores rtol 1e-5 / atol 2e-6, every
gradient tensor <= 2e-5 * max(max|that tensor|, max|any gradient| / 4) + 1e-6."""
import ctypes
import functools
import os
import re

import numpy as np
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


# ---- the reference and the emulation ----
def bf16_round(a):
    """float32 array -> the nearest bf16 values (ties to even) as float32: what v_cvt_pk_bf16_f32 and torch give."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    r = ((u >> 16) & 1) + np.uint32(0x7FFF)
    return ((u + r) & np.uint32(0xFFFF0000)).view(np.float32)


def _params(F, H1, H2, rng):
    def u(*shape, fan):
        return ((rng.random(shape) * 2 - 1) / np.sqrt(fan)).astype(np.float32)
    return [u(H1, F, fan=F), u(H1, fan=F), u(H2, H1, fan=H1), u(H2, fan=H1), u(1, H2, fan=H2), u(1, fan=H2)]


@functools.lru_cache(maxsize=None)
def _case(B, L, F, H1, H2, lengths="ragged", every=1):
    """tests/test_gpu_mlp_rows.py::_case with the batch rounded once to bf16 (X: the rounded values as float32) and the
    float64 reference on the rounded X and the rounded W1 (params: the fp32 master weights, unrounded).  Cached and
    shared: never written to."""
    rng = np.random.default_rng(100000 * every + 1000 * L + 10 * F + B)
    X = torch.from_numpy(rng.normal(0.0, 1.0, (B, L, F)).astype(np.float32)).bfloat16().float().numpy()
    params = _params(F, H1, H2, rng)
    if lengths is None:
        n = None
        real = np.ones((B, L), dtype=bool)
    else:
        if lengths == "ragged":
            n = rng.integers(2, L + 1, B).astype(np.int64)
            for i, v in enumerate((0, 1, L, L + 5)):
                if i < B:
                    n[i] = v
        else:
            n = np.asarray(lengths, dtype=np.int64)
        real = np.arange(L)[None, :] < np.clip(n, 0, L)[:, None]
    g = ((rng.random((B, L)) + 0.5) * rng.choice([-1.0, 1.0], (B, L))).astype(np.float32)
    if every > 1:
        order = np.cumsum(real.reshape(-1)).reshape(B, L)            # 1-based index among the real rows
        g = np.where(order % every == 0, g, np.float32(0.0))
    g = np.where(real, g, np.float32(0.0))
    rounded = [torch.from_numpy(params[0]).bfloat16().float().numpy()] + params[1:]
    leaves = [torch.from_numpy(p.astype(np.float64)).requires_grad_() for p in rounded]
    x = torch.from_numpy(X.astype(np.float64))
    h = torch.relu(torch.relu(x @ leaves[0].T + leaves[1]) @ leaves[2].T + leaves[3])
    s = (h @ leaves[4].T + leaves[5]).squeeze(-1)
    (s * torch.from_numpy(g.astype(np.float64))).sum().backward()
    return dict(X=X, params=params, n=n, g=g, real=real, scores=s.detach().numpy(),
                grads=[t.grad.numpy() for t in leaves])


def _errors(case, scores, grads):
    """[(name, error, tolerance)] of the scores (real rows; atol + rtol * |want| at the worst row) and the six
    gradients."""
    real = case["real"]
    out = []
    if real.any():
        d = np.abs(scores[real] - case["scores"][real]) - 1e-5 * np.abs(case["scores"][real])
        out.append(("scores", float(d.max()), 2e-6))
    scale = max(np.abs(w).max() for w in case["grads"])
    for key, got, w in zip(("W1", "b1", "W2", "b2", "W3", "b3"), grads, case["grads"]):
        tol = 2e-5 * max(np.abs(w).max(), 0.25 * scale) + 1e-6
        out.append((key, float(np.abs(np.asarray(got, dtype=np.float64).reshape(w.shape) - w).max()), tol))
    return out


def _emulate(case, split):
    """The kernels' arithmetic in numpy float32: bf16 X, bf16 W1, exact products accumulated in float32, everything
    behind layer 1 in float32; dW1 = dH1^T . X with dH1 as hi + lo in bf16 (`split`) or as hi alone."""
    f32 = np.float32
    W1, b1, W2, b2, W3, b3 = case["params"]
    X = case["X"].reshape(-1, case["X"].shape[2])
    real = case["real"].reshape(-1)
    g = case["g"].reshape(-1, 1)
    W1b = bf16_round(W1)
    z1 = (X @ W1b.T + b1).astype(f32)
    h1 = np.maximum(z1, f32(0))
    z2 = (h1 @ W2.T + b2).astype(f32)
    h2 = np.maximum(z2, f32(0))
    s = np.where(real, (h2 @ W3.T + b3).astype(f32).reshape(-1), f32(0))
    d2 = ((g @ W3) * (z2 > 0)).astype(f32)
    d1 = ((d2 @ W2) * (z1 > 0)).astype(f32)
    hi = bf16_round(d1)
    dW1 = (hi.T @ X).astype(f32)
    if split:
        dW1 = dW1 + (bf16_round(d1 - hi).T @ X).astype(f32)
    grads = [dW1, d1.sum(0), (d2.T @ h1).astype(f32), d2.sum(0), (g.T @ h2).astype(f32), g.sum(0)]
    return s.reshape(case["real"].shape), grads


EMULATED = (3, 70, 136, 64, 16)


def test_the_emulated_arithmetic_meets_the_reference():
    case = _case(*EMULATED)
    for name, err, tol in _errors(case, *_emulate(case, split=True)):
        print("%s err %.3g tol %.3g" % (name, err, tol))
        assert err <= tol, (name, err, tol)


def test_a_single_bf16_term_of_dh1_does_not():
    case = _case(*EMULATED)
    errs = {name: (err, tol) for name, err, tol in _errors(case, *_emulate(case, split=False))}
    print("W1 err %.3g tol %.3g" % errs["W1"])
    assert errs["W1"][0] > errs["W1"][1]
    # (and nothing but dW1 feels it)
    assert all(err <= tol for name, (err, tol) in errs.items() if name != "W1")


def test_bf16_round_is_torch_s():
    a = np.random.default_rng(0).normal(0, 3, 4096).astype(np.float32)
    a[:4] = np.array([1.00390625, 1.01171875, -1.00390625, 0.0], dtype=np.float32)        # ties: to even
    assert np.array_equal(bf16_round(a), torch.from_numpy(a).bfloat16().float().numpy())


# ---- boundary ----
def test_header_exports_and_ctypes_table_agree(lib):
    from pytorchltr_amd import _C
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltr_mlp_bf16.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(ltr_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_C.MLP_BF16_SIGNATURES)
    assert len(declared) == 3
    for name, (_, argtypes) in _C.MLP_BF16_SIGNATURES.items():
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr), name          # exported by the library
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1).strip()
        assert len(proto.split(",")) == len(argtypes), name                     # as many arguments as the prototype
    # argument for argument the prototypes of ltr_mlp_rows.h
    for ours, theirs in (("ltr_mlp_bf16_scores", "ltr_mlp_rows_scores_f32"), ("ltr_mlp_bf16_grad", "ltr_mlp_rows_grad_f32"),
                         ("ltr_mlp_bf16_grad_workspace_bytes", "ltr_mlp_rows_grad_workspace_bytes")):
        assert _C.MLP_BF16_SIGNATURES[ours] == _C.MLP_ROWS_SIGNATURES[theirs]
    others = (set(_C.SIGNATURES) | set(_C.EVAL_SIGNATURES) | set(_C.LISTWISE_SIGNATURES) | set(_C.LONGPAIR_SIGNATURES)
              | set(_C.MLP_ROWS_SIGNATURES) | set(_C.MLP_WIDE_SIGNATURES))
    assert not set(_C.MLP_BF16_SIGNATURES) & others


def test_exported_mlp_bf16_symbols_are_the_declared_ones(lib):
    import subprocess
    from pytorchltr_amd import _C, _codeobj
    from pytorchltr_amd.build import LIB_PATH, build_extension
    build_extension()
    out = subprocess.run([_codeobj._tool("llvm-readelf"), "--dyn-syms", "-W", LIB_PATH], check=True,
                         stdout=subprocess.PIPE).stdout.decode()
    defined = "\n".join(ln for ln in out.splitlines() if " FUNC " in ln and " GLOBAL " in ln and " UND " not in ln)
    assert sorted(set(re.findall(r"\b(ltr_mlp_bf16_[a-z0-9_]+)\b", defined))) == sorted(_C.MLP_BF16_SIGNATURES)
    assert len(_C.MLP_BF16_SIGNATURES) == 3
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltr_hip.h")).read(), flags=re.S)
    assert not [k for k in _C.SIGNATURES if "mlp_bf16" in k] and "ltr_mlp_bf16" not in main
    assert len(_C.SIGNATURES) == 80 and lib.ltr_version() == 114


# ---- argument errors ----
def _scores(lib, B=2, L=10, F=8, H1=4, H2=4, X=P, W=P, out=P):
    return lib.ltr_mlp_bf16_scores(X, W, P, P, P, P, P, P, B, L, F, H1, H2, out, None)


def _grad(lib, B=2, L=10, F=8, H1=4, H2=4, X=P, W=P, g=P, grads=P, ws=P, ws_bytes=1 << 40):
    return lib.ltr_mlp_bf16_grad(X, W, P, P, P, P, P, g, P, B, L, F, H1, H2, grads, ws, ws_bytes, None)


@pytest.mark.parametrize("change", [dict(F=12), dict(F=232), dict(F=4), dict(F=0), dict(H1=65), dict(H1=0), dict(H2=17),
                                    dict(L=0), dict(B=-1), dict(B=1 << 20, L=1 << 12)])
def test_shape_errors_come_first(lib, change):
    # (every pointer NULL as well: the shape is judged first)
    assert _scores(lib, X=None, W=None, out=None, **change) == ERR_SHAPE
    assert _grad(lib, X=None, W=None, g=None, grads=None, ws=None, ws_bytes=0, **change) == ERR_SHAPE
    assert lib.ltr_mlp_bf16_grad_workspace_bytes(change.get("B", 2), change.get("L", 10), change.get("F", 8),
                                                 change.get("H1", 4), change.get("H2", 4)) == 0


@pytest.mark.parametrize("F", [8, 136, 224])
def test_every_feature_count_up_to_224_reaches_the_null_check(lib, F):
    assert _scores(lib, F=F, H1=64, H2=16, W=None, X=None, out=None) == ERR_NULL
    assert _scores(lib, F=F, H1=64, H2=16, X=None) == ERR_NULL
    assert _grad(lib, F=F, H1=64, H2=16, grads=None) == ERR_NULL
    assert _grad(lib, F=F, H1=64, H2=16, g=None) == ERR_NULL
    count = lib.ltr_mlp_param_count(F, 64, 16)
    assert lib.ltr_mlp_bf16_grad_workspace_bytes(2, 10, F, 64, 16) >= 4 * count


def test_null_then_empty_then_null_then_workspace(lib):
    assert _scores(lib, W=None) == ERR_NULL
    assert _grad(lib, W=None) == ERR_NULL
    assert _grad(lib, grads=None) == ERR_NULL
    assert _scores(lib, B=0, W=None) == ERR_NULL                            # a parameter in front of the empty batch
    assert _grad(lib, B=0, grads=None) == ERR_NULL
    assert _scores(lib, B=0, X=None, out=None) == OK                        # (the gradient call launches: GPU tier)
    assert _scores(lib, X=None) == ERR_NULL
    assert _scores(lib, out=None) == ERR_NULL
    assert _grad(lib, X=None, ws=None, ws_bytes=0) == ERR_NULL              # NULL in front of the workspace
    assert _grad(lib, g=None, ws=None, ws_bytes=0) == ERR_NULL
    need = lib.ltr_mlp_bf16_grad_workspace_bytes(2, 10, 8, 4, 4)
    assert need > 0
    assert _grad(lib, ws_bytes=need - 1) == ERR_WORKSPACE
    assert _grad(lib, ws=None) == ERR_WORKSPACE
    assert lib.ltr_mlp_bf16_grad_workspace_bytes(0, 10, 8, 4, 4) == 0


# ---- code object ----
def test_bf16_kernels_exist_and_do_not_spill():
    from pytorchltr_amd import _codeobj
    from pytorchltr_amd.build import LIB_PATH, build_extension
    build_extension()
    recs = _codeobj.kernel_records(LIB_PATH)  # (no skip without the llvm tools: the no-spill rule is a requirement)
    ours = {}
    for r in recs:
        m = re.search(r"(mlp_bf16_kernel<[^>]*>)", r.get("demangled", r["name"]))
        if m:
            ours[m.group(1)] = r
    assert sorted(ours) == sorted("mlp_bf16_kernel<%d, %s>" % (ks, gr) for ks in range(1, 8) for gr in ("false", "true"))
    for key, r in ours.items():
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, (key, r)
        # two workgroups of four waves per CU: 256 registers a wave (AGPRs included)
        assert 0 < r.get("vgpr_count", 0) + r.get("agpr_count", 0) <= 256, (key, r)
    # the fp32 row kernels keep their records
    rows = [r for r in recs if "mlp_rows_kernel<" in r.get("demangled", r["name"])]
    assert len(rows) == 8 and not any(r.get("vgpr_spill_count", 0) for r in rows)


# ---- Python surface ----
def test_python_surface():
    from pytorchltr_amd import fused
    for key in ((8, 1, 1), (136, 50, 10), (224, 64, 16)):
        assert fused._mlp_bf16_network(*key), key
    for key in ((12, 4, 4), (220, 64, 16), (232, 64, 16), (8, 65, 16), (8, 64, 17), (0, 4, 4)):
        assert not fused._mlp_bf16_network(*key), key
    m = fused.MLPScorer(16, (5, 3))
    params = [p.detach() for p in m.parameters()]
    bf = torch.zeros(2, 5, 16, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="bfloat16"):                       # an fp32 batch
        fused.mlp_scores_bf16(torch.zeros(2, 5, 16), params)
    with pytest.raises(ValueError, match="bfloat16"):
        fused.mlp_grad_bf16(torch.zeros(2, 5, 16), params, torch.zeros(2, 5))
    with pytest.raises(ValueError, match="Linear"):                         # a wrong parameter shape
        fused.mlp_scores_bf16(torch.zeros(2, 5, 24, dtype=torch.bfloat16), params)
    with pytest.raises(ValueError, match="Linear"):
        fused.mlp_grad_bf16(bf, params[:2] + [torch.zeros(3, 6)] + params[3:], torch.zeros(2, 5))
    with pytest.raises(ValueError, match="L >= 1"):                         # L == 0
        fused.mlp_scores_bf16(torch.zeros(2, 0, 16, dtype=torch.bfloat16), params)
    with pytest.raises(ValueError, match="L >= 1"):
        fused.mlp_grad_bf16(torch.zeros(2, 0, 16, dtype=torch.bfloat16), params, torch.zeros(2, 0))
    wide = [p.detach() for p in fused.MLPScorer(226, (5, 3)).parameters()]
    with pytest.raises(ValueError, match="224"):                            # 226 -> 232 features
        fused.mlp_scores_bf16(torch.zeros(2, 5, 226, dtype=torch.bfloat16), wide)
    big = [p.detach() for p in fused.MLPScorer(16, (65, 3)).parameters()]
    with pytest.raises(ValueError, match="hidden"):
        fused.mlp_scores_bf16(bf, big)


def test_cpu_tensors_are_refused():
    from pytorchltr_amd import fused
    m = fused.MLPScorer(16, (4, 3))
    params = [p.detach() for p in m.parameters()]
    bf = torch.zeros(2, 5, 16, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(bf)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fused.mlp_scores_bf16(bf, params)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fused.mlp_grad_bf16(bf, params, torch.zeros(2, 5))
