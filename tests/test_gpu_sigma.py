"""GPU tier of the loss-steepness parity (run with `-m gpu` on an MI355X): sigma != 1 through every kernel path.

The five log-sigmoid kinds (PairwiseLogistic, LambdaARP1/2, LambdaNDCG1/2) take a steepness sigma, which enters twice:
as c1 = sigma * log2(e) inside the pair term and as the gradient scale sigma / ln 2, applied once per document at the end.
That second rule is written once per kernel family, each copy behind another exchange of partial sums.  The batches
are tests/degenerate.py's (exact grid scores: W = e_0, b = 0.25, no row is excused as a rank flip; the degenerate
flavours stay in: `maxDCG == 0 -> 1` meets the sigma scale), the shapes the degenerate sweep's, sigma is 0.7 and 2.0.

Per path, every check of every kind is run before the case fails (_Errors), and the worst excess is printed:
  (a) parity with the fp64 oracle at that sigma (tests/test_sigma_host.py, and the golden vectors at sigma = 2, pin it),
      at the neighbouring tests' own bounds as tests/test_gpu_degenerate.py's header lists them, unwidened;
  (b) sigma = 2.0, no tolerance: loss(sigma = 2; s) is bit-identical to loss(sigma = 1; 2 s), its gradient to twice the
      other side's.  Scaling by a power of two is exact in fp32: t = (s_k - s_m) c1 has the same bits whether the 2 sits
      in c1 or in the scores, 2 / ln 2 is twice 1 / ln 2, the ranks do not move and the build has no fast-math.  For the
      fused Linear step the 2 goes into W and b (W = e_0: the dot products scale exactly), for the MLP step into W3, b3
      (dW3, db3 come out doubled, the gradients of the layers below bit-identical: d h2 = ds (x) W3 has the 2 on either
      side).  EVERY path below holds the identity; none needed the fallback to the bounds of (a);
  (c) the hinge kinds ignore sigma: through the C ABI with sigma = 2.0 bit-identical to sigma = 1.0;
  (d) the host paths that carry sigma from call to call: pytorchltr_amd.optim.SGD when the loss module changes between
      two steps, the lazy step of the C ABI, GraphedStep.

Which case reaches which sigma site (each case asserts its plan, workspace or hook):
  ltr_common.inc pairwise_core        test_loss_only_default_launch (24 x 37: one document per thread),
                                      test_loss_only_explicit_launch_shapes (64,1,1) and (128,2,4), test_loss_only_narrow_workgroups,
                                      test_step_general_kernel[scalar_rows]
  ltr_common.inc pairwise_core_sym    test_loss_only_default_launch (128, 300), the (64,0,8) launch shape, test_loss_only_label_dtypes,
                                      test_step_register_tiles (8-, 19-, 24-sweep tile), test_step_general_kernel[scores_out],
                                      test_mlp_step (ltr_mlp.inc and ltr_mlp2.inc call it)
  ltr_kernels.hip split finisher      test_loss_only_split_query_launch (24 x 1000, 12 x 1025: several workgroups per query)
  ltr_cluster.inc                     test_step_cluster_kernel; ltr_debug_cluster_mode(2) only switches the hinge kinds'
                                      sorted runs off (`kRuns` is compiled for them alone), mode 1 replaces every member's
                                      plain stores of pair sums and gradient shares by write-through ones for ALL kinds: the
                                      log-sigmoid kinds run in modes 0 and 1, the hinge kinds in 0, 1 and 2
  ltr_parts.inc parts_finish          its P == 1 call: 24 x 257 x 16 under ltr_debug_parts_all (one part per query); its call in
                                      `combine` (the last part of a query adds the parked shares): 24 x 420 x 16 under the hook
                                      and the two shapes that plan the parts kernel WITHOUT the hook, 24 x 512 x 448 (NDCG
                                      kinds) and 24 x 1025 x 448 (the others) -- the smallest such lists at 24 queries of 112
                                      float4, the narrowest rows the planner calls wide
  ltr_parts.inc parts_pair_pass       three groups of call sites: the NDCG kinds' (ndcg1, ndcg2 on every parts shape up to 1024
                                      documents), the plain one (logistic, arp1, arp2 on every parts shape) and the polling one
                                      (kPollInPass: the hinge kinds in the one-sided kernel on lists of several parts,
                                      24 x 420 x 16 -- sigma is handed over and must be ignored, check (c))
  ltr_longpair.inc c1 and finisher    test_loss_only_forced_long_pair_path (both ids), test_loss_only_long_pair_path_past_the_limit
  ltr_f64.inc                         test_loss_only_fp64_scores
  past the fused MLP limit            test_mlp_step_past_the_fused_limit: the stand-alone loss kernel between the row kernels
"""
import copy
import functools

import numpy as np
import pytest
import torch

from oracle import ltr_oracle as O
from tests.degenerate import exact_scores, zero_rows
from tests.test_gpu_degenerate import HINGES, PARTS_SHAPES, _Errors, _Hooks, _batch, _check_rows, _code, _dev, _loss_excess

pytestmark = pytest.mark.gpu

LOGISTIC_KINDS = ("logistic", "arp1", "arp2", "ndcg1", "ndcg2")
SIGMAS = (0.7, 2.0)
MODE = "grid"
ZERO_Q = 11                 # the query whose upstream gradient is exactly 0: the first `control` query of a batch


def _module(kind):
    from tests.test_gpu_parity import _loss_cls
    return _loss_cls(kind)


def _bits(errs, what, name, got, want):
    """got and want bit for bit (as numbers: -0.0 == 0.0); the figure of a miss is the largest difference."""
    got, want = np.asarray(got), np.asarray(want)
    same = np.array_equal(got, want)
    errs.expect(same, what, name, "not bit-identical: max |diff| %.3e of max %.3e"
                % (0.0 if same else float(np.max(np.abs(got.astype(np.float64) - want))), float(np.max(np.abs(want), initial=0.0))))


def _grad_excess(ds, want_g, long_path):
    """Worst |ds - want| minus the bound of tests/test_gpu_parity.py::_check_grad (the long-pair path:
    tests/test_gpu_long_pairs.py::_check_grad_vs_oracle) over the entries: <= 0 is inside."""
    scale = np.max(np.abs(want_g), axis=1, keepdims=True)
    bound = 2e-4 * scale + 1e-5 if long_path else 1e-5 * scale + 1e-6
    return float(np.max(np.abs(ds - want_g) - bound))


# ---------------------------------------------------------------------------------------------------------------------
# the loss-only kernels
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _want_loss(kind, B, L, sigma):
    X, W, b, y, n, fl = _batch(B, L, 1, MODE)
    return O.pairwise_loss(kind, exact_scores(X), y.numpy(), n.numpy(), sigma=sigma)


def _run_loss_only(kind, B, L, sigma, scale=1.0, labels="int64", cfg=None, long_lists=False):
    """(loss, dscores) as the kernel wrote them (fp32) on `scale` times the batch's scores."""
    from pytorchltr_amd._autograd import pairwise_loss_and_grad
    X, W, b, y, n, fl = _batch(B, L, 1, MODE, labels)
    dev = _dev()
    s = ((X[:, :, 0] + b[0]) * scale).contiguous()
    loss, ds = pairwise_loss_and_grad(s.to(dev), y.to(dev), n.to(dev), _code(kind), sigma, cfg=cfg, long_lists=long_lists)
    return loss.cpu().numpy(), ds.cpu().numpy()


def _loss_only_case(B, L, labels="int64", cfg=None, long_lists=False, sigmas=SIGMAS, kinds=LOGISTIC_KINDS, tag=""):
    X, W, b, y, n, fl = _batch(B, L, 1, MODE)
    errs = _Errors()
    run = functools.partial(_run_loss_only, B=B, L=L, labels=labels, cfg=cfg, long_lists=long_lists)
    for kind in kinds:
        for sigma in sigmas:
            what = "%s %s sigma %.1f %dx%d %s" % (tag, kind, sigma, B, L, labels)
            loss, ds = run(kind, sigma=sigma)
            want_l, want_g = _want_loss(kind, B, L, sigma)
            print("%s: gradient worst excess %.3e" % (what, _grad_excess(ds.astype(np.float64), want_g, long_lists)))
            _check_rows(errs, kind, loss, ds.astype(np.float64), want_l, want_g, y.numpy(), n.numpy(), fl, L, what,
                        long_path=long_lists)
            if sigma == 2.0:
                loss1, ds1 = run(kind, sigma=1.0, scale=2.0)
                _bits(errs, what, "loss vs loss(sigma = 1; 2 s)", loss, loss1)
                _bits(errs, what, "dscores vs 2 dscores(sigma = 1; 2 s)", ds, 2.0 * ds1)
    for kind in HINGES:
        what = "%s %s %dx%d %s" % (tag, kind, B, L, labels)
        loss1, ds1 = run(kind, sigma=1.0)
        loss2, ds2 = run(kind, sigma=2.0)
        _bits(errs, what, "loss at sigma = 2 vs sigma = 1", loss2, loss1)
        _bits(errs, what, "dscores at sigma = 2 vs sigma = 1", ds2, ds1)
    errs.done()


@pytest.mark.parametrize("L", [37, 128, 300])
def test_loss_only_default_launch(L):
    """ltr_pairwise_loss_f32 with the launch shape it picks (the entry point IS the path): one wave tile, two, a long list."""
    _loss_only_case(24, L, tag="default")


@pytest.mark.parametrize("cfg", [(64, 1, 1), (128, 2, 4), (64, 0, 8)], ids=lambda c: "%d-%d-%d" % c)
def test_loss_only_explicit_launch_shapes(cfg):
    """One document per thread on one wave, the widest split of the pair loop (pairwise_core), and the symmetric pair
    pass (dpt 0: pairwise_core_sym)."""
    _loss_only_case(24, 300, cfg=cfg, tag="cfg%s" % (cfg,))


@pytest.mark.parametrize("B,L", [(24, 1000), (12, 1025)])
def test_loss_only_split_query_launch(B, L):
    """Several workgroups per query through the workspace entry point: the finisher of ltr_kernels.hip scales the summed
    shares.  12 x 1025 also as one workgroup."""
    from pytorchltr_amd import _C
    assert all(_C.lib().ltr_pairwise_loss_workspace_bytes(_code(k), B, L) > 0 for k in LOGISTIC_KINDS + HINGES)
    _loss_only_case(B, L, cfg="split", tag="split")
    if L == 1025:
        _loss_only_case(B, L, tag="one workgroup")


def test_loss_only_narrow_workgroups():
    """4096 queries of 64 documents: a query on one or two waves (choose_loss_shape), no split-query workspace."""
    from pytorchltr_amd import _C
    assert all(_C.lib().ltr_pairwise_loss_workspace_bytes(_code(k), 4096, 64) == 0 for k in LOGISTIC_KINDS + HINGES)
    _loss_only_case(4096, 64, tag="narrow")


@pytest.mark.parametrize("sorted_preparation", [False, True], ids=["prepare_kernel", "sorted_preparation"])
def test_loss_only_forced_long_pair_path(sorted_preparation):
    """ltr_pairwise_loss_long_f32 forced onto lists of 300 documents (ltr_longpair.inc: its own c1 in the tile kernel, its
    own sigma / ln 2 in the finisher), behind the two sorts -- the long path's one preparation, so both ids run it, the
    second with ltr_debug_long_sort_all set as well."""
    from pytorchltr_amd import _C
    lib = _C.lib()
    prev = lib.ltr_debug_long_pairs_all(1)
    prev_sort = lib.ltr_debug_long_sort_all(1) if sorted_preparation else None
    try:
        assert lib.ltr_debug_long_pairs_all(1) == 1
        assert lib.ltr_pairwise_loss_long_workspace_bytes(_code("ndcg2"), 24, 300) > 0
        _loss_only_case(24, 300, long_lists=True, tag="forced long")
    finally:
        if sorted_preparation:
            lib.ltr_debug_long_sort_all(prev_sort)
        lib.ltr_debug_long_pairs_all(prev)


@pytest.mark.parametrize("kind", LOGISTIC_KINDS)
def test_loss_only_long_pair_path_past_the_limit(kind):
    """... and for real: 4097 documents, one past ltr_max_list_len(), sigma = 2.0 only (the oracle's pair loop takes a
    few seconds per kind and sigma there); the hinge kinds ride along with the first kind."""
    from pytorchltr_amd import _C
    assert 4097 > _C.max_list_len()
    X, W, b, y, n, fl = _batch(12, 4097, 1, MODE)
    errs = _Errors()
    what = "long %s sigma 2.0 12x4097" % kind
    loss, ds = _run_loss_only(kind, 12, 4097, 2.0, long_lists=True)
    want_l, want_g = _want_loss(kind, 12, 4097, 2.0)
    print("%s: gradient worst excess %.3e" % (what, _grad_excess(ds.astype(np.float64), want_g, True)))
    _check_rows(errs, kind, loss, ds.astype(np.float64), want_l, want_g, y.numpy(), n.numpy(), fl, 4097, what, long_path=True)
    loss1, ds1 = _run_loss_only(kind, 12, 4097, 1.0, scale=2.0, long_lists=True)
    _bits(errs, what, "loss vs loss(sigma = 1; 2 s)", loss, loss1)
    _bits(errs, what, "dscores vs 2 dscores(sigma = 1; 2 s)", ds, 2.0 * ds1)
    if kind == LOGISTIC_KINDS[0]:
        for hk in HINGES:
            loss1, ds1 = _run_loss_only(hk, 12, 4097, 1.0, long_lists=True)
            loss2, ds2 = _run_loss_only(hk, 12, 4097, 2.0, long_lists=True)
            _bits(errs, "long %s 12x4097" % hk, "loss at sigma = 2 vs sigma = 1", loss2, loss1)
            _bits(errs, "long %s 12x4097" % hk, "dscores at sigma = 2 vs sigma = 1", ds2, ds1)
    errs.done()


def _run_f64(kind, s, y, n, sigma):
    """ltr_pairwise_loss_f64 through the C ABI (the hinge modules have no sigma to hand over)."""
    from pytorchltr_amd import _C
    dev = _dev()
    sd, yd, nd = torch.from_numpy(s).to(dev), y.to(dev), n.to(dev)
    B, L = s.shape
    loss = torch.empty(B, dtype=torch.float64, device=dev)
    ds = torch.empty(B, L, dtype=torch.float64, device=dev)
    _C.check(_C.lib().ltr_pairwise_loss_f64(_code(kind), float(sigma), sd.data_ptr(), yd.data_ptr(), _C.label_dtype(yd),
                                            nd.data_ptr(), B, L, loss.data_ptr(), ds.data_ptr(), _C.stream_of(sd)))
    return loss.cpu().numpy(), ds.cpu().numpy()


@pytest.mark.parametrize("L", [37, 300])
def test_loss_only_fp64_scores(L):
    """fp64 scores take the fp64 kernels (ltr_f64.inc: `sig` in the exponent, sig / ln 2 at the end), through the modules
    and autograd: bounds of tests/test_gpu_parity.py::test_fp64_scores_give_fp64_arithmetic.  The identity holds in fp64
    for the same reasons as in fp32."""
    dev = _dev()
    X, W, b, y, n, fl = _batch(24, L, 1, MODE)
    s = exact_scores(X)
    errs = _Errors()

    def run(kind, sigma, scale):
        sc = torch.from_numpy(s * scale).to(dev).requires_grad_(True)
        out = _module(kind)(sigma=sigma)(sc, y.to(dev), n.to(dev))
        assert out.dtype == torch.float64
        out.sum().backward()
        return out.detach().cpu().numpy(), sc.grad.cpu().numpy()

    for kind in LOGISTIC_KINDS:
        for sigma in SIGMAS:
            what = "fp64 %s sigma %.1f 24x%d" % (kind, sigma, L)
            loss, ds = run(kind, sigma, 1.0)
            want_l, want_g = _want_loss(kind, 24, L, sigma)
            scale = np.max(np.abs(want_g), axis=1, keepdims=True) + 1e-300
            e_l = float(np.max(np.abs(loss - want_l) - (1e-12 + 1e-11 * np.abs(want_l))))
            e_g = float(np.max(np.abs(ds - want_g) - (1e-11 * scale + 1e-13)))
            print("%s: loss worst excess %.3e gradient worst excess %.3e" % (what, e_l, e_g))
            errs.expect(np.allclose(loss, want_l, rtol=1e-11, atol=1e-12), what, "loss err", np.abs(loss - want_l).max())
            errs.expect(np.all(np.abs(ds - want_g) <= 1e-11 * scale + 1e-13), what, "grad err", np.abs(ds - want_g).max())
            rows = zero_rows(kind, y.numpy(), n.numpy())
            errs.expect(not loss[rows].any() and not ds[rows].any(), what, "pair-free rows not exactly 0")
            if sigma == 2.0:
                loss1, ds1 = run(kind, 1.0, 2.0)
                _bits(errs, what, "loss vs loss(sigma = 1; 2 s)", loss, loss1)
                _bits(errs, what, "dscores vs 2 dscores(sigma = 1; 2 s)", ds, 2.0 * ds1)
    for kind in HINGES:
        loss1, ds1 = _run_f64(kind, s, y, n, 1.0)
        loss2, ds2 = _run_f64(kind, s, y, n, 2.0)
        _bits(errs, "fp64 %s 24x%d" % (kind, L), "loss at sigma = 2 vs sigma = 1", loss2, loss1)
        _bits(errs, "fp64 %s 24x%d" % (kind, L), "dscores at sigma = 2 vs sigma = 1", ds2, ds1)
    errs.done()


@pytest.mark.parametrize("labels", ["int32", "float32"])
def test_loss_only_label_dtypes(labels):
    """The same values as int32 and float32 labels (float labels switch off the integer-label shortcuts)."""
    for L in (128, 300):
        _loss_only_case(24, L, labels=labels, tag="default")


# ---------------------------------------------------------------------------------------------------------------------
# the fused Linear step
# ---------------------------------------------------------------------------------------------------------------------
def _grad_out(B):
    """The per-query upstream gradient: a negative, a zero and non-uniform weights."""
    go = torch.linspace(-0.5, 1.5, B)
    go[min(ZERO_Q, B - 1)] = 0.0
    assert float(go.min()) < 0.0 and not go.all()
    return go


@functools.lru_cache(maxsize=None)
def _want_step(kind, B, L, F, sigma, weighted):
    X, W, b, y, n, fl = _batch(B, L, F, MODE)
    gout = _grad_out(B).double().numpy() if weighted else np.full(B, 1.0 / B)
    return O.linear_pairwise(kind, X.numpy(), W.numpy(), float(b[0]), y.numpy(), n.numpy(), gout, sigma=sigma)


def _loss_arg(kind, sigma):
    """A loss module built with that sigma; the hinge modules have none: (kind, sigma) as the C ABI takes them."""
    from pytorchltr_amd.fused import _KindProxy
    if kind in HINGES:
        return _KindProxy(_code(kind), sigma)
    return _module(kind)(sigma)


def _step_case(B, L, F, plan, weighted, kinds=LOGISTIC_KINDS, hinges=HINGES, return_scores=False, parts_all=False,
               cluster_mode=0, tag=""):
    from pytorchltr_amd import _C
    from pytorchltr_amd.fused import linear_loss_step
    dev = _dev()
    lib = _C.lib()
    X, W, b, y, n, fl = _batch(B, L, F, MODE)
    assert fl[ZERO_Q] == "control" and int(n[ZERO_Q]) >= 3
    Xd, Wd, bd, yd, nd = X.to(dev), W.to(dev), b.to(dev), y.to(dev), n.to(dev)
    W2d, b2d = (2.0 * W).to(dev), (2.0 * b).to(dev)
    go = _grad_out(B).to(dev) if weighted else None
    n0 = n.clone()
    n0[ZERO_Q] = 0
    n0d = n0.to(dev)
    errs = _Errors()
    multi = plan in (_C.PLAN_CLUSTER, _C.PLAN_PARTS)

    def step(kind, sigma, Wt=Wd, bt=bd, nt=nd):
        out = linear_loss_step(Xd, Wt, bt, yd, nt, loss=_loss_arg(kind, sigma), grad_out=go, return_scores=return_scores)
        torch.cuda.synchronize()
        if multi:
            _C.device_status()
        return [t.cpu().numpy() for t in out]

    with _Hooks(parts_all, cluster_mode):
        for kind in kinds:
            assert lib.ltr_linear_fused_plan(_code(kind), B, L, F) == plan, (tag, kind)
            for sigma in SIGMAS:
                what = "%s %s sigma %.1f %dx%dx%d %s" % (tag, kind, sigma, B, L, F, "weighted" if weighted else "uniform")
                out = step(kind, sigma)
                loss, dW, db = out[0], out[1], out[2]
                want_l, want_s, want_dW, want_db = _want_step(kind, B, L, F, sigma, weighted)
                errs.expect(np.all(np.isfinite(loss)) and np.all(np.isfinite(dW)), what, "not finite")
                ex, r = _loss_excess(loss, want_l, L)
                tol = 2e-5 * max(1.0, float(np.max(np.abs(want_dW)))) * (10 if L > 256 else 1)     # tests/test_gpu_fused.py::_check
                e_w, e_b = float(np.max(np.abs(dW.astype(np.float64) - want_dW))), abs(float(db[0]) - want_db)
                print("%s: loss worst excess %.3e (row %d, %s); dW err %.3e db err %.3e tol %.3e"
                      % (what, ex, r, fl[r], e_w, e_b, tol))
                errs.expect(ex <= 0, what, "loss row %d (%s): got %r want %r" % (r, fl[r], loss[r], want_l[r]))
                errs.expect(e_w < tol and e_b < tol, what, "dW err %.3e db err %.3e tol %.3e" % (e_w, e_b, tol))
                rows = zero_rows(kind, y.numpy(), n.numpy())
                errs.expect(not loss[rows].any(), what, "loss of pair-free rows not exactly 0:", loss[rows])
                if return_scores:
                    rl = (torch.arange(L)[None, :] < n[:, None]).numpy()
                    errs.expect(np.array_equal(out[3][rl].astype(np.float64), exact_scores(X)[rl]), what, "scores not exact")
                if sigma == 2.0:
                    loss1, dW1, db1 = step(kind, 1.0, W2d, b2d)[:3]
                    _bits(errs, what, "loss vs loss(sigma = 1; 2 W, 2 b)", loss, loss1)
                    _bits(errs, what, "dW vs 2 dW(sigma = 1; 2 W, 2 b)", dW, 2.0 * dW1)
                    _bits(errs, what, "db vs 2 db(sigma = 1; 2 W, 2 b)", db, 2.0 * db1)
                if weighted:
                    # the query of weight 0 contributes exactly nothing: the same batch without it
                    loss0, dW0, db0 = step(kind, sigma, nt=n0d)[:3]
                    _bits(errs, what, "dW vs the batch with the zero-weight query emptied", dW, dW0)
                    _bits(errs, what, "db vs the batch with the zero-weight query emptied", db, db0)
                    keep = np.arange(B) != ZERO_Q
                    _bits(errs, what, "the other queries' losses", loss[keep], loss0[keep])
        for kind in hinges:
            assert lib.ltr_linear_fused_plan(_code(kind), B, L, F) == plan, (tag, kind)
            what = "%s %s %dx%dx%d %s" % (tag, kind, B, L, F, "weighted" if weighted else "uniform")
            one, two = step(kind, 1.0), step(kind, 2.0)
            for name, a, c in zip(("loss", "dW", "db"), two, one):
                _bits(errs, what, "%s at sigma = 2 vs sigma = 1" % name, a, c)
    errs.done()


WEIGHTED = pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])


@WEIGHTED
@pytest.mark.parametrize("shape", [(24, 128, 136), (64, 129, 220), (64, 216, 220)], ids=lambda s: "%dx%dx%d" % s)
def test_step_register_tiles(shape, weighted):
    """The 8-sweep register tile, the 19-sweep and the 24-sweep tile (pairwise_core_sym with the deferred scale)."""
    from pytorchltr_amd import _C
    _step_case(*shape, _C.PLAN_REGISTER_TILE, weighted, tag="tile")


@WEIGHTED
@pytest.mark.parametrize("shape", [(24, 128, 136, True), (24, 128, 6, False)], ids=["scores_out", "scalar_rows"])
def test_step_general_kernel(shape, weighted):
    """The general (re-read) kernel: what a register-tile shape takes once the scores are asked for, and rows that are not
    whole float4 (F = 6, the scalar path)."""
    from pytorchltr_amd import _C
    B, L, F, scores_out = shape
    _step_case(B, L, F, _C.PLAN_REGISTER_TILE if scores_out else _C.PLAN_GENERAL, weighted, return_scores=True, tag="general")


@WEIGHTED
@pytest.mark.parametrize("shape", [(33, 1000, 220), (64, 300, 64)], ids=lambda s: "%dx%dx%d" % s)
def test_step_cluster_kernel(shape, weighted):
    """A query spread over a cluster of workgroups: the members' pair sums and gradient shares meet before ltr_cluster.inc
    applies sigma / ln 2.  ltr_debug_cluster_mode(1) -- the write-through exchange -- changes the stores of every kind, so
    the log-sigmoid kinds run under it too; mode 2 (the pair pass instead of the sorted runs) exists for the hinge kinds
    only, which run in all three modes."""
    from pytorchltr_amd import _C
    _step_case(*shape, _C.PLAN_CLUSTER, weighted, tag="cluster")
    _step_case(*shape, _C.PLAN_CLUSTER, weighted, cluster_mode=1, tag="cluster write-through")
    _step_case(*shape, _C.PLAN_CLUSTER, weighted, kinds=(), cluster_mode=2, tag="cluster pair pass")


@WEIGHTED
@pytest.mark.parametrize("shape", PARTS_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_step_parts_kernel(shape, weighted):
    """The parts kernel under ltr_debug_parts_all(1): one part per query (parts_finish's P == 1 call) at 24 x 257 x 16, lists
    of two parts (parts_finish in `combine`; the hinge kinds' polling pair pass) at 24 x 420 x 16."""
    from pytorchltr_amd import _C
    B, L, F = shape
    assert _C.lib().ltr_linear_fused_plan(_C.LOGISTIC, B, L, F) != _C.PLAN_PARTS          # (not without the hook)
    _step_case(B, L, F, _C.PLAN_PARTS, weighted, parts_all=True, tag="parts")


# the smallest lists that plan the parts kernel on their own at 24 queries of 112 float4 (F = 448, the narrowest rows its
# planner calls wide): 512 documents for the NDCG kinds, one past the symmetric pass for the others
PARTS_PLANNED = {(24, 512, 448): (("ndcg1", "ndcg2"), ()), (24, 1025, 448): (("logistic", "arp1", "arp2"), HINGES)}


@WEIGHTED
@pytest.mark.parametrize("shape", list(PARTS_PLANNED), ids=lambda s: "%dx%dx%d" % s)
def test_step_parts_kernel_as_planned(shape, weighted):
    """... and where ltr_linear_fused_plan picks the parts kernel WITHOUT the hook (the cluster kernel, which comes first
    in the dispatcher's chain, declines): wide rows, several parts per query."""
    from pytorchltr_amd import _C
    lib = _C.lib()
    B, L, F = shape
    kinds, hinges = PARTS_PLANNED[shape]
    for kind in kinds + hinges:                  # one document shorter and another kernel takes the shape
        assert lib.ltr_linear_fused_plan(_code(kind), B, L - 1, F) != _C.PLAN_PARTS, kind
    _step_case(B, L, F, _C.PLAN_PARTS, weighted, kinds=kinds, hinges=hinges, tag="parts as planned")


# ---------------------------------------------------------------------------------------------------------------------
# the fused MLP step
# ---------------------------------------------------------------------------------------------------------------------
def _mlp_case(B, L, F, seed, weighted):
    """tests/test_gpu_mlp.py::_check at both sigmas, then the identity: sigma = 2 on (W3, b3) against sigma = 1 on
    (2 W3, 2 b3) -- loss, dW1, db1, dW2, db2 bit-identical, dW3 and db3 doubled."""
    from pytorchltr_amd import fused
    from tests.test_gpu_mlp import _check, _mlp_params
    dev = _dev()
    X, W, b, y, n, fl = _batch(B, L, F, MODE)
    params = _mlp_params(F, 50, 10, seed)
    go = _grad_out(B) if weighted else None
    errs = _Errors()
    Xd, yd, nd = X.to(dev), y.to(dev), n.to(dev)
    god = None if go is None else go.to(dev)

    def step(kind, sigma, prm):
        lossv, grads = fused.mlp_loss_step(Xd, [p.to(dev) for p in prm], yd, nd, loss=_loss_arg(kind, sigma), grad_out=god)
        torch.cuda.synchronize()
        return lossv.cpu().numpy(), [g.cpu().numpy() for g in grads]

    doubled = params[:4] + [2.0 * params[4], 2.0 * params[5]]
    for kind in LOGISTIC_KINDS:
        for sigma in SIGMAS:
            what = "mlp %s sigma %.1f %dx%dx%d %s" % (kind, sigma, B, L, F, "weighted" if weighted else "uniform")
            try:
                _check(kind, X, y, n, params, grad_out=go, sigma=sigma)
                print("%s: inside the bounds of tests/test_gpu_mlp.py::_check" % what)
            except AssertionError as e:
                errs.append("%s: %s" % (what, str(e)[:300]))
        what = "mlp %s sigma 2.0 %dx%dx%d" % (kind, B, L, F)
        loss, grads = step(kind, 2.0, params)
        loss1, grads1 = step(kind, 1.0, doubled)
        _bits(errs, what, "loss vs loss(sigma = 1; 2 W3, 2 b3)", loss, loss1)
        for key, g, g1 in zip(("dW1", "db1", "dW2", "db2"), grads[:4], grads1[:4]):
            _bits(errs, what, "%s vs the other side's" % key, g, g1)
        for key, g, g1 in zip(("dW3", "db3"), grads[4:], grads1[4:]):
            _bits(errs, what, "%s vs twice the other side's" % key, g, 2.0 * g1)
    for kind in HINGES:
        what = "mlp %s %dx%dx%d" % (kind, B, L, F)
        (loss1, grads1), (loss2, grads2) = step(kind, 1.0, params), step(kind, 2.0, params)
        _bits(errs, what, "loss at sigma = 2 vs sigma = 1", loss2, loss1)
        for i, (g2, g1) in enumerate(zip(grads2, grads1)):
            _bits(errs, what, "gradient %d at sigma = 2 vs sigma = 1" % i, g2, g1)
    errs.done()


@WEIGHTED
@pytest.mark.parametrize("L", [100, 200])
@pytest.mark.parametrize("layout", ["tile", "wide"])
def test_mlp_step(layout, L, weighted):
    """mlp_loss_step on the guide's 136-50-10-1 network, both kernel layouts (ltr_debug_mlp_layout 2 and 1: ltr_mlp2.inc and
    ltr_mlp.inc each hand p.sigma to pairwise_core_sym), one fill of the tile and the 129 .. 256 class."""
    from pytorchltr_amd import _C, fused
    assert fused.mlp_supported(L, 136, 50, 10)
    lib = _C.lib()
    lib.ltr_debug_mlp_layout(1 if layout == "wide" else 2)
    try:
        _mlp_case(24, L, 136, 31 + L, weighted)
    finally:
        lib.ltr_debug_mlp_layout(0)


@WEIGHTED
def test_mlp_step_past_the_fused_limit(weighted):
    """300 documents: no fused MLP kernel holds the list; the row score kernel, the stand-alone loss kernel (which gets the
    module's sigma from _mlp_step_pieces), the row gradient kernel."""
    from pytorchltr_amd import fused
    assert not fused.mlp_supported(300, 24, 50, 10)
    _mlp_case(6, 300, 24, 331, weighted)


# ---------------------------------------------------------------------------------------------------------------------
# host paths that carry sigma from call to call
# ---------------------------------------------------------------------------------------------------------------------
def test_training_loop_changes_module_and_sigma_between_steps():
    """The reference's loop body with pytorchltr_amd.optim.SGD on use_linear_scorer(nn.Linear(136, 1)), 64 x 100 x 136: three
    steps with LambdaNDCGLoss2(sigma=2.0), then on the same model and optimizer three with PairwiseLogisticLoss(sigma=0.7),
    against torch.optim.SGD on a plain nn.Linear with the same modules, at tests/test_gpu_optim.py's bounds
    (test_same_training_as_torch_sgd).  The fourth step's launch applies the third's pending update (NDCG2 rows) and
    computes with the new module's kind and sigma: every step's loss is compared, so the change must take effect at once.
    The learning rate changes with the module (both optimizers' param_groups): LambdaNDCG2 is normalised by maxDCG, the
    logistic loss is a plain sum over the ~L^2 / 4 pairs of a query, so its gradient is some 10^3 times larger -- at the
    first phase's 0.03 it takes steps of many times the weights and the run diverges (losses 1.5e3, 8.5e3, 1.6e4), which
    amplifies the two paths' rounding past any bound on the weights; 1e-5 keeps its steps at the first phase's size."""
    from pytorchltr_amd import loss as L_
    from pytorchltr_amd.optim import SGD, LazyGrad
    from tests.test_gpu_optim import _data, _loop, _models
    dev = _dev()
    B, L, F = 64, 100, 136
    data = _data(6, B, L, F, 500, dev)
    lin, _, m_lazy = _models(F, dev)
    m_ref = copy.deepcopy(lin)
    assert type(m_ref) is torch.nn.Linear
    o_ref = torch.optim.SGD(m_ref.parameters(), lr=0.03)
    o_lazy = SGD(m_lazy.parameters(), lr=0.03)
    first, second = L_.LambdaNDCGLoss2(sigma=2.0), L_.PairwiseLogisticLoss(sigma=0.7)

    def train(model, opt):
        head = _loop(model, opt, first, data[:3])
        for group in opt.param_groups:
            group["lr"] = 1e-5
        return torch.cat([head, _loop(model, opt, second, data[3:])])

    l_ref, l_lazy = train(m_ref, o_ref), train(m_lazy, o_lazy)
    print("losses lazy %s\nlosses ref  %s" % (l_lazy.tolist(), l_ref.tolist()))
    assert torch.allclose(l_lazy, l_ref, rtol=2e-5, atol=1e-6)
    # the steps were the lazy ones (the last update still pending), and sigma mattered: the same step at sigma = 1 is another
    st = m_lazy.weight._ltr_lazy
    assert st.pending is not None and isinstance(m_lazy.weight.grad, LazyGrad)
    with torch.no_grad():
        xs, ys, n = data[3]
        at_one = L_.PairwiseLogisticLoss()(torch.nn.functional.linear(xs, m_ref.weight, m_ref.bias), ys, n).mean()
        at_07 = second(torch.nn.functional.linear(xs, m_ref.weight, m_ref.bias), ys, n).mean()
    assert not torch.allclose(at_one, at_07, rtol=1e-2)
    w = m_lazy.weight.detach().clone()
    assert st.pending is None
    assert torch.allclose(w, m_ref.weight.detach(), rtol=1e-5, atol=1e-6)
    assert torch.allclose(m_lazy.bias.detach(), m_ref.bias.detach(), rtol=1e-5, atol=1e-6)
    assert torch.allclose(m_lazy.weight.grad, m_ref.weight.grad, rtol=1e-4, atol=1e-5 * max(1.0, float(m_ref.weight.grad.abs().max())))


@pytest.mark.parametrize("kind", LOGISTIC_KINDS)
def test_lazy_step_at_sigma_2(kind):
    """ltr_linear_sgd_lazy_step_f32 at sigma = 2.0 against the two-launch ltr_linear_sgd_step_f32 at 24 x 128 x 136: weights,
    buckets and losses bit-identical after three steps -- and the two-launch step's first gradient is the oracle's at
    sigma = 2 (bound of tests/test_gpu_step.py::test_sgd_step_follows_the_oracles_trajectory), so neither drops it."""
    from pytorchltr_amd import _C
    from tests.conftest import synth
    lib = _C.lib()
    dev = _dev()
    B, L, F = 24, 128, 136
    kind_id, sigma, lr = _code(kind), 2.0, 0.05
    batches = []
    for i in range(3):
        s, y, n, X, W, b = synth(B, L, 11 + i, F=F)
        batches.append((X, y, n))
    _, _, _, _, W0, b0 = synth(B, L, 11, F=F)
    dbatches = [[t.to(dev) for t in bt] for bt in batches]
    st = _C.stream_of(dbatches[0][0])
    nws = lib.ltr_linear_workspace_bytes(B, L, F)

    def run(lazy):
        Wd, bd = W0.clone().to(dev), b0.clone().to(dev)
        ws = torch.full((nws // 4 + 64,), float("nan"), device=dev)
        loss = torch.empty(B, device=dev)
        bucket = torch.zeros(F + 2, device=dev)
        out = []
        pending = 0
        for k in range(3):
            Xd, yd, nd = dbatches[k]
            if lazy:
                _C.check(lib.ltr_linear_sgd_lazy_step_f32(kind_id, sigma, Xd.data_ptr(), Wd.data_ptr(), bd.data_ptr(), yd.data_ptr(),
                                                          _C.LABEL_I64, nd.data_ptr(), B, L, F, lr, loss.data_ptr(), bucket.data_ptr(),
                                                          ws.data_ptr(), ws.numel() * 4, pending, st))
                pending = B
            else:
                _C.check(lib.ltr_linear_sgd_step_f32(kind_id, sigma, Xd.data_ptr(), Wd.data_ptr(), bd.data_ptr(), yd.data_ptr(),
                                                     _C.LABEL_I64, nd.data_ptr(), None, B, L, F, lr, loss.data_ptr(),
                                                     bucket.data_ptr(), ws.data_ptr(), ws.numel() * 4, None, st))
                if k == 0:
                    out.append(bucket.clone())
            out.append(loss.clone())
        if lazy:
            _C.check(lib.ltr_linear_sgd_flush_f32(kind_id, Wd.data_ptr(), bd.data_ptr(), pending, L, F, lr, loss.data_ptr(),
                                                  bucket.data_ptr(), ws.data_ptr(), st))
        torch.cuda.synchronize()
        _C.device_status()
        return Wd.cpu().numpy(), bd.cpu().numpy(), bucket.cpu().numpy(), [t.cpu().numpy() for t in out]

    We, be, bucket_e, out_e = run(False)
    Wl, bl, bucket_l, out_l = run(True)
    first = out_e.pop(0)
    X, y, n = batches[0]
    want_l, _, want_dW, want_db = O.linear_pairwise(kind, X.numpy(), W0.numpy(), float(b0[0]), y.numpy(), n.numpy(),
                                                    np.full(B, 1.0 / B), sigma=sigma)
    tol = 5e-5 * max(1.0, float(np.max(np.abs(want_dW)))) + 1e-6
    err = float(np.max(np.abs(first[:F] - want_dW)))
    print("%s: first step's dW err %.3e tol %.3e" % (kind, err, tol))
    assert err < tol and abs(float(first[F]) - want_db) < tol
    assert np.isclose(float(first[F + 1]), float(want_l.sum()), rtol=2e-5, atol=1e-4)
    assert np.all(np.isfinite(We)) and np.array_equal(We, Wl) and np.array_equal(be, bl)
    assert np.array_equal(bucket_e, bucket_l)
    for a, c in zip(out_e, out_l):
        assert np.array_equal(a, c)


@pytest.mark.parametrize("which", ["dropin", "fused_linear", "fused_mlp"])
def test_graphed_step_with_a_sigma_2_loss(which):
    """GraphedStep with PairwiseLogisticLoss(sigma=2.0): the replay equals the eager step at tests/test_gpu_graphed.py's
    bounds; the eager loss of the first step is the oracle's at sigma = 2 (loss bound of tests/test_gpu_fused.py /
    tests/test_gpu_mlp.py)."""
    from pytorchltr_amd.fused import FusedLinearLoss, FusedMLPLoss
    from pytorchltr_amd.graphed import GraphedStep
    from pytorchltr_amd.loss import PairwiseLogisticLoss
    from tests.test_gpu_graphed import _batches
    dev = _dev()
    B, L, F = 32, 40, 24
    host = _batches(8, B, L, F, 100)
    data = [tuple(t.to(dev) for t in bt) for bt in host]

    def make():
        torch.manual_seed(7)
        loss_fn = PairwiseLogisticLoss(sigma=2.0)
        if which == "dropin":
            model = torch.nn.Linear(F, 1).to(dev)
            return model, (lambda xs, ys, n: loss_fn(model(xs), ys, n).mean())
        if which == "fused_linear":
            model = FusedLinearLoss(F, loss_fn).to(dev)
            return model, (lambda xs, ys, n: model(xs, ys, n).mean())
        model = FusedMLPLoss(F, loss_fn, hidden=(16, 4)).to(dev)
        return model, (lambda xs, ys, n: model(xs, ys, n))

    model_e, closure_e = make()
    start = [p.detach().cpu().double().numpy() for p in model_e.parameters()]
    opt_e = torch.optim.SGD(model_e.parameters(), lr=0.05)
    losses_e = []
    for batch in [data[0]] * 3 + data:
        opt_e.zero_grad(set_to_none=True)
        loss = closure_e(*batch)
        loss.backward()
        opt_e.step()
        losses_e.append(float(loss))
    X, y, n = host[0]
    if which == "fused_mlp":
        want = O.mlp_pairwise("logistic", X.numpy(), start, y.numpy(), n.numpy(), np.full(B, 1.0 / B), sigma=2.0)[0]
    else:
        want = O.linear_pairwise("logistic", X.numpy(), start[0].reshape(-1), float(start[1][0]), y.numpy(), n.numpy(),
                                 np.full(B, 1.0 / B), sigma=2.0)[0]
    assert losses_e[0] == pytest.approx(float(want.mean()), rel=2e-5, abs=1e-5)

    model_g, closure_g = make()
    opt_g = torch.optim.SGD(model_g.parameters(), lr=0.05)
    step = GraphedStep(model_g, opt_g, closure_g, example_batch=data[0], warmup=3)
    losses_g = [float(step(*batch)) for batch in data]
    assert losses_g == pytest.approx(losses_e[3:], rel=1e-5, abs=1e-6)
    for a, c in zip(model_g.parameters(), model_e.parameters()):
        assert torch.allclose(a, c, rtol=1e-5, atol=1e-6)
