"""GPU tier of the fused MLP step on a bf16 feature batch (include/ltr_mlp_step_bf16.h; run with `-m gpu`).  The
reference is the fp64 one the fp32 step is held to, on the bf16-rounded X and W1: oracle.ltr_oracle.mlp_pairwise, and
for the row slots the fp64 network and loss references of tests/test_gpu_mlp_listwise.py / _lambdarank.py (LambdaRank
on the returned scores, as there).  Tolerances: tests/test_gpu_mlp.py::_check's."""
import numpy as np
import pytest
import torch

from oracle import ltr_oracle as O
from tests import lambdarank_ref as R
from tests import mlp_train_ref as ref
from tests.test_gpu_mlp import KINDS
from tests.test_gpu_mlp_listwise import LISTMLE, LISTNET, _loss64, _network64, _params

pytestmark = pytest.mark.gpu
LAMBDARANK, NAMES = "lambdarank", ("W1", "b1", "W2", "b2", "W3", "b3")
DEV = torch.device("cuda:0")


def _round(a):
    return torch.from_numpy(a).bfloat16().float().numpy()


def _case(B, L, F, H1, H2, lengths=None):
    rng = np.random.default_rng(1000 * L + 10 * F + B)
    X = _round(rng.normal(0.0, 1.0, (B, L, F)).astype(np.float32))
    y = rng.integers(0, 5, (B, L)).astype(np.int64)
    n = rng.integers(0, L + 1, B).astype(np.int64) if lengths is None else np.array(lengths, dtype=np.int64)
    return X, y, n, _params(F, H1, H2, rng)


def _step(slot, case, k=None, sigma=1.0, go=None, fuse=True, X=None):
    from pytorchltr_amd import fused
    from pytorchltr_amd import loss as Lmod
    dev = DEV
    X0, y, n, params = case
    args = (torch.from_numpy(X0 if X is None else X).to(dev).bfloat16(), [torch.from_numpy(p).to(dev) for p in params],
            torch.from_numpy(y).to(dev), torch.from_numpy(n).to(dev))
    kw = dict(grad_out=None if go is None else torch.from_numpy(go).to(dev), return_scores=True, return_loss_sum=True,
              fuse_bf16=fuse)
    if slot == LAMBDARANK:
        out = fused.mlp_lambdarank_step(*args, sigma=sigma, k=k, **kw)
    else:
        obj = Lmod.ListMLELoss(k) if slot == LISTMLE and k is not None else slot
        if sigma != 1.0:
            obj = Lmod.PairwiseLogisticLoss(sigma=sigma)
        out = fused.mlp_loss_step(*args, loss=obj, **kw)
    torch.cuda.synchronize()
    return out


def _check(slot, case, got, k=None, sigma=1.0, go=None):
    X, y, n, params = case
    B, L = y.shape
    lossv, grads, scores, lsum = got
    got_l, got_s = lossv.cpu().numpy().astype(np.float64), scores.cpu().numpy()
    rounded = [_round(params[0])] + list(params[1:])
    w = np.full(B, 1.0 / B) if go is None else go.astype(np.float64)
    valid = np.arange(L)[None, :] < np.clip(n, 0, L)[:, None]
    if slot in KINDS:
        want_l, want_s, g = O.mlp_pairwise(slot, X, rounded, y, n, w, sigma=sigma)
        want_g = [g[key] for key in NAMES]
        ds = O.pairwise_loss(slot, want_s, y, n, sigma=sigma)[1]
    else:
        s64, leaves = _network64(X, rounded)
        want_s = s64.detach().numpy()
        if slot == LAMBDARANK:                     # (the ranking is decided on the scores the kernel ranked)
            want_l, ds = R.batch(got_s, y, n, k=k, sigma=sigma)
        else:
            want_l, ds = _loss64(slot, want_s, y, n, k)
        s64.backward(torch.from_numpy(np.where(valid, ds, 0.0) * w[:, None]))
        want_g = [t.grad.numpy() for t in leaves]
    print("%s loss err %.3g" % (slot, np.abs(got_l - want_l).max()))
    assert np.allclose(got_l, want_l, rtol=2e-5, atol=1e-5), (slot, np.abs(got_l - want_l).max())
    assert np.allclose(float(lsum), want_l.sum(), rtol=2e-5, atol=1e-4)
    assert np.allclose(got_s[valid], want_s[valid], rtol=1e-5, atol=2e-6)
    assert np.all(got_s[~valid] == 0.0)
    scale = max(max(np.abs(g).max() for g in want_g), float((np.abs(np.where(valid, ds, 0.0)) * w[:, None]).sum()))
    for key, g, want in zip(NAMES, grads, want_g):
        tol = 2e-5 * max(np.abs(want).max(), 0.25 * scale) + 1e-6
        err = np.abs(g.cpu().numpy().reshape(want.shape).astype(np.float64) - want).max()
        print("  d%s err %.3g tol %.3g" % (key, err, tol))
        assert err <= tol, (slot, key, err, tol)


@pytest.mark.parametrize("slot,k", [(kind, None) for kind in KINDS] + [
    (LISTNET, None), (LISTMLE, None), (LISTMLE, 10), (LAMBDARANK, None), (LAMBDARANK, 10)])
def test_every_loss_slot(slot, k):
    from pytorchltr_amd.utils import tie_breaking
    case = _case(5, 33, 136, 50, 10, lengths=(0, 1, 33, 38, 17))
    with tie_breaking("index"):
        _check(slot, case, _step(slot, case, k=k), k=k)


@pytest.mark.parametrize("slot", ["hinge", "ndcg2"])
@pytest.mark.parametrize("F,hidden", [(8, (1, 1))] + [(F, (64, 16)) for F in (8, 32, 40, 64, 72, 136, 160, 168, 224)])
def test_every_k_step_count_its_zero_padding_and_the_declined_widths(F, hidden, slot):
    from pytorchltr_amd import fused
    case = _case(4, 50, F, *hidden)
    got = _step(slot, case)
    if F > 160:                                    # off the plan (the bucket would spill): the pieces' own result
        off = _step(slot, case, fuse=False)
        assert not fused.mlp_step_bf16_supported(50, F, *hidden)
        assert torch.equal(got[0], off[0]) and all(torch.equal(a, b) for a, b in zip(got[1], off[1]))
    _check(slot, case, got)


FILLS = (7, 128, 24, 13, 5, (128, 97, 96, 33, 32, 1, 0))                   # every fill count in one batch


@pytest.mark.parametrize("slot,k,sigma,weighted,shape", [
    ("hinge", None, 1.0, False, FILLS), (LAMBDARANK, 10, 1.0, False, FILLS),
    ("hinge", None, 1.0, False, (1100, 8, 8, 4, 3)),                       # more queries than workgroups, two scheduling blocks
    ("logistic", None, 2.5, True, (5, 33, 136, 50, 10, (0, 1, 33, 38, 17)))])  # explicit grad_out, sigma
def test_fill_counts_scheduling_weights_and_sigma(slot, k, sigma, weighted, shape):
    case = _case(*shape)
    go = (np.random.default_rng(3).random(shape[0]) + 0.1).astype(np.float32) if weighted else None
    _check(slot, case, _step(slot, case, k=k, sigma=sigma, go=go), k=k, sigma=sigma, go=go)


def test_padding_is_never_read_runs_are_bit_identical_and_a_replay_equals_eager():
    from pytorchltr_amd import fused
    dev, case = DEV, _case(6, 40, 24, 13, 5, lengths=(40, 0, 1, 33, 17, 32))
    X, y, n, params = case
    dirty = X.copy()
    dirty[np.arange(40)[None, :] >= n[:, None]] = np.nan
    a, b, c = _step("hinge", case), _step("hinge", case), _step("hinge", case, X=dirty)
    for other in (b, c):
        assert torch.equal(a[0], other[0]) and torch.equal(a[2], other[2]) and torch.equal(a[3], other[3])
        assert all(torch.equal(g, h) for g, h in zip(a[1], other[1]))
    # one capture, replayed on changed inputs
    P = [torch.from_numpy(p).to(dev) for p in params]
    sx, sy, sn = (torch.zeros(*shape, dtype=t, device=dev) for shape, t in
                  (((6, 40, 24), torch.bfloat16), ((6, 40), torch.int64), ((6,), torch.int64)))
    out = torch.empty(a[1][0]._base.numel(), device=dev)
    graph = torch.cuda.CUDAGraph()             # (the eager calls above were the warm-up)
    with torch.cuda.graph(graph):
        lossv, grads = fused.mlp_loss_step(sx, P, sy, sn, "hinge", out=out, fuse_bf16=True)
    sx.copy_(torch.from_numpy(X)), sy.copy_(torch.from_numpy(y)), sn.copy_(torch.from_numpy(n))
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(lossv, a[0]) and all(torch.equal(g, h) for g, h in zip(grads, a[1]))


@pytest.mark.parametrize("which,F,L", [("pairwise", 136, 33), ("pairwise", 46, 20), ("listnet", 24, 20),
                                      ("lambdarank", 24, 20), ("pairwise", 24, 300)])
def test_modules_make_one_call_and_their_backward_meets_the_tolerances(which, F, L, monkeypatch):
    from pytorchltr_amd import _C, fused
    dev, lib, called = DEV, _C.lib(), []
    for name in ("ltr_mlp_step_bf16", "ltr_mlp_bf16_scores", "ltr_mlp_bf16_grad"):
        monkeypatch.setattr(lib, name, lambda *args, _n=name, _f=getattr(lib, name): called.append(_n) or _f(*args))
    torch.manual_seed(2)
    if which == "pairwise":
        model, slot, k = fused.FusedMLPLoss(F, "hinge", fuse_bf16=True), "hinge", None
    elif which == "listnet":
        model, slot, k = fused.FusedMLPListwiseLoss(F, "listnet"), LISTNET, None
    else:
        model, slot, k = fused.FusedMLPLambdaRankLoss(F, k=10), LAMBDARANK, 10
    model.fuse_bf16 = True                         # (the two row-slot classes keep their constructors: the attribute)
    model = model.to(dev)
    X, y, n, _ = _case(5, L, F, 50, 10)
    total = model(torch.from_numpy(X).to(dev).bfloat16(), torch.from_numpy(y).to(dev), torch.from_numpy(n).to(dev))
    total.backward()
    fits = L <= fused.MLP_STEP_BF16_MAX_LIST_LEN   # past the plan: the pieces, as without the flag
    assert called == (["ltr_mlp_step_bf16"] if fits else ["ltr_mlp_bf16_scores", "ltr_mlp_bf16_grad"])
    if fits:
        params = [p.detach().cpu().numpy() for p in model._params()]
        grads = [p.grad for p in model._params()]
        scores = model.score(torch.from_numpy(X).to(dev).bfloat16(), torch.from_numpy(n).to(dev)).detach().squeeze(-1)
        _check(slot, (X, y, n, params), (model.last_losses, grads, scores, total.detach() * 5), k=k)


def test_trainer_takes_two_steps_on_the_rounded_network(monkeypatch):
    from pytorchltr_amd import _C, fused
    dev, lib, called = DEV, _C.lib(), []
    monkeypatch.setattr(lib, "ltr_mlp_train_step_bf16",
                        lambda *args, _f=lib.ltr_mlp_train_step_bf16: called.append(1) or _f(*args))
    torch.manual_seed(5)
    model = fused.FusedMLPLoss(24, "hinge", fuse_bf16=True).to(dev)
    trainer = fused.MLPTrainer(model, "adagrad", lr=0.05)
    hyper = dict(trainer.hyper, lr=trainer.lr)
    for step in range(2):
        X, y, n, _ = _case(6 + step, 33, 24, 50, 10)
        batch = (torch.from_numpy(X).to(dev).bfloat16(), torch.from_numpy(y).to(dev), torch.from_numpy(n).to(dev))
        params0 = [p.detach().clone() for p in model._params()]
        state0 = trainer.state_dict()["state"]
        grads = [g.clone() for g in trainer.step(*batch, return_grads=True)[1]]
        # the update consumed the fused step's gradient (held to the rounded network above) by the reference's rule
        want = fused.mlp_loss_step(batch[0], params0, *batch[1:], "hinge", fuse_bf16=True)[1]
        assert all(torch.equal(g, h.reshape(g.shape)) for g, h in zip(grads, want))
        for i, (p0, g, p1) in enumerate(zip(params0, grads, model._params())):
            st = {key: v.cpu().numpy() for key, v in state0.get(i, {}).items() if key != "step"} \
                or ref.initial_state("adagrad", hyper, p0.cpu().numpy())
            want_p, _, bound = ref.step("adagrad", hyper, p0.cpu().numpy(), g.cpu().numpy(), st, step)
            assert (np.abs(p1.detach().cpu().numpy().astype(np.float64) - want_p) <= bound["p"]).all(), (step, i)
    assert called == [1, 1] and trainer.steps == 2
