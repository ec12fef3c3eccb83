"""GPU tier of the MLP trainer (run with `-m gpu` on an MI355X): pytorchltr_amd.fused.MLPTrainer -- the fused MLP step
with the optimizer update inside the reduction launch (ltr_mlp_train_step_f32) and, off the fused route, the pieces plus
one update launch (ltr_mlp_apply_update_f32).

The reference is tests/mlp_train_ref.py: the fp64 rule applied to the fp32 gradient the EXISTING step
(mlp_loss_step / mlp_lambdarank_step) computes on the pre-step parameters, and its derived bound -- roundings on the
chain x 2^-24 x the magnitudes of its terms + half an ulp; nothing here is a measured tolerance.  Every step is checked
against its own pre-step snapshot, so nothing compounds."""
import copy

import numpy as np
import pytest
import torch

from tests import mlp_train_ref as ref

pytestmark = pytest.mark.gpu

HIDDEN = (50, 10)
# name -> (B, L, F, hidden, dtype, what it exercises)
SHAPES = {
    "3x5x8": (3, 5, 8, (5, 3), torch.float32),            # P = 67: every segment boundary misaligned, a float4 tail, grid 3
    "40x20x136": (40, 20, 136, HIDDEN, torch.float32),    # the guide's network, P = 7371
    "520x4x12": (520, 4, 12, HIDDEN, torch.float32),      # B >= 2 x CUs: the tile layout's full grid
    "6x9x5": (6, 9, 5, HIDDEN, torch.float32),            # F % 4 != 0: w1_pitch < the gradient's row width
    "1x7x8": (1, 7, 8, (5, 3), torch.float32),            # a single-query grid
    "5x6x8-degenerate": (5, 6, 8, (5, 3), torch.float32),  # n holds 0 and 1
    "4x300x136": (4, 300, 136, HIDDEN, torch.float32),    # off the fused route: the row kernels + apply
    "4x40x452": (4, 40, 452, HIDDEN, torch.float32),      # wide rows + apply
    "6x20x136-bf16": (6, 20, 136, HIDDEN, torch.bfloat16),  # the bf16 kernels + apply
    # the padded routes: w1_pitch < the gradient's row width, so the update meets columns that are no parameters
    "2x300x46": (2, 300, 46, HIDDEN, torch.float32),      # the row kernels + apply, pad 2
    "2x20x699": (2, 20, 699, HIDDEN, torch.float32),      # wide rows + apply, pad 1
    "3x20x44-bf16": (3, 20, 44, HIDDEN, torch.bfloat16),  # bf16 pads to 8: a whole float4 of every W1 row is padding
    "3x20x46-bf16": (3, 20, 46, HIDDEN, torch.bfloat16),  # pad 2
    "3x9x46": (3, 9, 46, HIDDEN, torch.float32),          # fused, pad 2
}
PADDED = ("2x300x46", "2x20x699", "3x20x44-bf16", "3x20x46-bf16", "3x9x46")
FUSED = ("3x5x8", "40x20x136", "520x4x12", "6x9x5", "1x7x8", "5x6x8-degenerate", "3x9x46")
# batches of the tests that bring their own network (hidden sizes: the test's)
OTHER = {
    "3x9x44": (3, 9, 44, (5, 3), torch.float32),          # fused, Fp = 44
    "3x9x44-bf16": (3, 9, 44, (5, 3), torch.bfloat16),    # the bf16 kernels + apply, Fp = 48
    "4x6x8": (4, 6, 8, None, torch.float32),
}
OPTIMS = {
    "sgd": dict(lr=0.05, momentum=0.9, dampening=0.3, weight_decay=0.02),
    "sgd-nesterov": dict(lr=0.05, momentum=0.8, nesterov=True, weight_decay=0.01),
    "sgd-plain": dict(lr=0.05),
    "adagrad": dict(lr=0.1, lr_decay=0.05, weight_decay=0.01, initial_accumulator_value=0.5, eps=1e-6),
    "adam": dict(lr=0.01, betas=(0.7, 0.95), eps=1e-5, weight_decay=0.03),
}
_TORCH = {"sgd": torch.optim.SGD, "adagrad": torch.optim.Adagrad, "adam": torch.optim.Adam}


def _algo(name):
    return name.split("-")[0]


def _dev():
    assert torch.cuda.is_available(), "GPU tier needs a ROCm device"
    return torch.device("cuda:0")


class _Layout:
    """A kernel layout of the training step through ltr_debug_mlp_layout (reset afterwards)."""

    def __init__(self, name):
        self.code = {"auto": 0, "tile": 2, "wide": 1}[name]

    def __enter__(self):
        from pytorchltr_amd import _C
        _C.lib().ltr_debug_mlp_layout(self.code)

    def __exit__(self, *exc):
        from pytorchltr_amd import _C
        _C.lib().ltr_debug_mlp_layout(0)
        return False


def _model(family, F, hidden, reduction="mean", seed=5):
    from pytorchltr_amd import fused
    torch.manual_seed(seed)
    if family == "pairwise":
        m = fused.FusedMLPLoss(F, loss="hinge", hidden=hidden, reduction=reduction)
    elif family == "logistic":
        m = fused.FusedMLPLoss(F, loss="logistic", hidden=hidden, reduction=reduction)
    elif family == "listnet":
        m = fused.FusedMLPListwiseLoss(F, loss="listnet", hidden=hidden, reduction=reduction)
    elif family == "listmle":
        m = fused.FusedMLPListwiseLoss(F, loss="listmle", hidden=hidden, reduction=reduction)
    else:
        m = fused.FusedMLPLambdaRankLoss(F, sigma=1.5, k=3, hidden=hidden, reduction=reduction)
    return m.to(_dev())


def _batches(shape, count, seed=0):
    B, L, F, _, dtype = SHAPES[shape] if shape in SHAPES else OTHER[shape]
    rng = np.random.default_rng(100 * B + L + seed)
    out = []
    for _ in range(count):
        xs = torch.from_numpy(rng.normal(0, 1, (B, L, F)).astype(np.float32)).to(_dev()).to(dtype)
        ys = torch.from_numpy(rng.integers(0, 5, (B, L))).to(_dev())
        n = rng.integers(2, L + 1, B)
        if shape.endswith("degenerate"):
            n[:3] = (0, 1, L)
        out.append((xs, ys, torch.from_numpy(n.astype(np.int64)).to(_dev())))
    return out


def _existing_step(model, xs, ys, n):
    """(per-query loss, the six gradients in the parameters' shapes, loss_sum) of the library's existing step on the
    model's present parameters: what the parent's loop body hands to the optimizer (the module's zero-padding of a
    feature count that is no multiple of 4 included)."""
    from pytorchltr_amd import fused
    params = [p.detach() for p in model._params()]
    B = xs.shape[0]
    go = None if model.reduction == "mean" else torch.ones(B, device=xs.device)
    xp, w1, extra = fused._zero_pad(xs, params[0], 8 if xs.dtype is torch.bfloat16 else 4)
    padded = [w1] + params[1:]
    kind = model.kind
    if xp.shape[2] > fused.MLP_MAX_FEATURES:
        # (the functions have no wide route: the module's pieces, as its forward composes them)
        X, flat, H1, H2, _, _ = fused._mlp_prepare(xp, padded, fused._MLP_WIDE, pad=False)
        lossv, grads, lsum = fused._mlp_step_pieces(X, flat, H1, H2, ys, n, kind, model.sigma, go, False, True, None)
    elif isinstance(kind, fused._ListwiseKind) and kind.loss == 2:
        lossv, grads, lsum = fused.mlp_lambdarank_step(xp, padded, ys, n, sigma=model.sigma, k=kind.k, grad_out=go,
                                                       return_loss_sum=True)
    else:
        lossv, grads, lsum = fused.mlp_loss_step(xp, padded, ys, n, loss=fused._KindProxy(kind, model.sigma), grad_out=go,
                                                 return_loss_sum=True)
    grads = fused._crop_grads(grads, extra, [p.shape for p in params])
    return lossv.clone(), [g.clone() for g in grads], lsum.clone()


def _snapshot(trainer):
    params = [p.detach().cpu().numpy().copy() for p in trainer.model._params()]
    return params, trainer.state_dict()["state"], trainer.steps


def _check_against_reference(name, before, grads, trainer, factor=1.0, after=None):
    """Every parameter and state element within `factor` x the reference's bound of the fp64 rule applied to the
    fp32 gradient, from the pre-step snapshot `before`."""
    algo, hyper = _algo(name), dict(OPTIMS[name], lr=trainer.lr)
    params0, state0, t = before
    params1 = after if after is not None else [p.detach().cpu().numpy() for p in trainer.model._params()]
    state1 = trainer.state_dict()["state"] if after is None else None
    for i, (p0, g) in enumerate(zip(params0, grads)):
        st = {k: v.cpu().numpy() for k, v in state0.get(i, {}).items() if k != "step" and v is not None}
        if not st:
            st = ref.initial_state(algo, hyper, p0)
        want_p, want_state, bound = ref.step(algo, hyper, p0, g.cpu().numpy(), st, t)
        err = np.abs(params1[i].astype(np.float64) - want_p)
        assert (err <= factor * bound["p"]).all(), (name, i, float((err / bound["p"]).max()))
        if state1 is None:
            continue
        for key, want in want_state.items():
            got = state1[i][key].cpu().numpy().astype(np.float64)
            err = np.abs(got - want)
            assert (err <= factor * bound[key]).all(), (name, i, key, float((err / bound[key]).max()))


def _trainer(model, name):
    from pytorchltr_amd import fused
    return fused.MLPTrainer(model, _algo(name), **OPTIMS[name])


# ---- 1. one step against the reference, 2. the same gradient ----
@pytest.mark.parametrize("layout", ["tile", "wide"])
@pytest.mark.parametrize("family", ["pairwise", "listnet", "lambdarank"])
@pytest.mark.parametrize("name", ["sgd", "adagrad", "adam"])
@pytest.mark.parametrize("shape", ["3x5x8", "40x20x136"])
def test_one_step_against_the_reference_and_the_same_gradient(shape, name, family, layout):
    B, L, F, hidden, _ = SHAPES[shape]
    model = _model(family, F, hidden)
    (batch,) = _batches(shape, 1)
    trainer = _trainer(model, name)
    with _Layout(layout):
        lossv, grads, lsum = _existing_step(model, *batch)
        before = _snapshot(trainer)
        total, got = trainer.step(*batch, return_grads=True)
        # the gradient the update consumed, the per-query losses and their sum: bit for bit the existing step's
        for g, w in zip(got, grads):
            assert g.shape == w.shape and torch.equal(g, w)
        assert torch.equal(model.last_losses, lossv)
        assert total.dim() == 0 and torch.equal(total, (lsum / B).reshape(()))
    _check_against_reference(name, before, grads, trainer)
    assert trainer.steps == 1
    assert all(p.grad is None for p in model.parameters())


def test_sum_reduction_listmle_and_the_other_sgd_forms():
    """reduction='sum' (grad_out of ones), ListMLE in index tie order, logistic; SGD with nesterov and without momentum."""
    from pytorchltr_amd.utils import tie_breaking
    B, L, F, hidden, _ = SHAPES["40x20x136"]
    (batch,) = _batches("40x20x136", 1)
    with tie_breaking("index"):
        for family, name in (("listmle", "sgd-nesterov"), ("logistic", "sgd-plain"), ("pairwise", "adam")):
            model = _model(family, F, hidden, reduction="sum")
            trainer = _trainer(model, name)
            lossv, grads, lsum = _existing_step(model, *batch)
            before = _snapshot(trainer)
            total, got = trainer.step(*batch, return_grads=True)
            assert all(torch.equal(g, w) for g, w in zip(got, grads)) and torch.equal(total, lsum.reshape(()))
            _check_against_reference(name, before, grads, trainer)
            if name == "sgd-plain":
                assert trainer.state_dict()["state"] == {}


# ---- 3. ten consecutive steps on every shape ----
@pytest.mark.parametrize("name", ["sgd", "adagrad", "adam"])
@pytest.mark.parametrize("shape", [s for s in SHAPES if s not in PADDED])
def test_ten_consecutive_steps(shape, name):
    B, L, F, hidden, _ = SHAPES[shape]
    family = {"sgd": "pairwise", "adagrad": "lambdarank", "adam": "listnet"}[name]
    model = _model(family, F, hidden)
    trainer = _trainer(model, name)
    if name == "sgd" and shape not in FUSED:
        trainer.lr = 2e-4               # (300 documents or 452 features: pair sums in the hundreds; a plain attribute)
    for step, batch in enumerate(_batches(shape, 10)):
        _, grads, _ = _existing_step(model, *batch)
        assert all(torch.isfinite(g).all() for g in grads)
        before = _snapshot(trainer)
        if shape in FUSED:
            loss = trainer.step(*batch)
        else:                                           # off the fused route the gradient is rebuilt from pieces:
            loss, got = trainer.step(*batch, return_grads=True)
            assert all(torch.equal(g, w) for g, w in zip(got, grads))        # the same pieces, the same bits
        assert torch.isfinite(loss)
        _check_against_reference(name, before, grads, trainer)
        assert trainer.steps == step + 1
    state = trainer.state_dict()["state"]
    if _algo(name) != "sgd":
        assert all(float(state[i]["step"]) == 10.0 for i in range(6))


def test_scalar_kernel_on_a_workspace_off_16_bytes():
    """The C ABI with a workspace that is not 16-byte aligned: ltr_mlp_train_step_f32 runs mlp_reduce_update_kernel, as
    ltr_mlp_pairwise_f32 runs mlp_reduce_kernel there -- the same gradient bit for bit, the update within the bound,
    the header counted and the ticket back at 0."""
    import ctypes

    from pytorchltr_amd import _C, fused
    B, L, F, hidden, _ = SHAPES["3x5x8"]
    H1, H2 = hidden
    lib, dev = _C.lib(), _dev()
    model = _model("pairwise", F, hidden)
    xs, ys, n = _batches("3x5x8", 1)[0]
    params = [p.detach().clone() for p in model._params()]
    before = [p.cpu().numpy().copy() for p in params]
    P, ws_bytes = fused._mlp_sizes_for(B, F, H1, H2)
    ws = torch.empty(ws_bytes // 4 + 4, device=dev)[1:]
    assert ws.data_ptr() % 16 == 4
    loss, want_loss = torch.empty(B, device=dev), torch.empty(B, device=dev)
    lsum, want_lsum = torch.empty(1, device=dev), torch.empty(1, device=dev)
    grads, want_grads = torch.empty(P, device=dev), torch.empty(P, device=dev)
    st = _C.stream_of(xs)
    _C.check(lib.ltr_mlp_pairwise_f32(0, 1.0, xs.data_ptr(), *[p.data_ptr() for p in params], ys.data_ptr(), 0, n.data_ptr(),
                                      None, B, L, F, H1, H2, want_loss.data_ptr(), None, want_grads.data_ptr(),
                                      want_lsum.data_ptr(), ws.data_ptr(), ws_bytes, st))
    hyper = OPTIMS["adam"]
    optim = _C.MLPOptim(algo=_C.OPT_ADAM, lr=hyper["lr"], weight_decay=hyper["weight_decay"], eps=hyper["eps"],
                        beta1=hyper["betas"][0], beta2=hyper["betas"][1])
    state = torch.zeros(lib.ltr_mlp_train_state_floats(_C.OPT_ADAM, F, H1, H2), device=dev)
    _C.check(lib.ltr_mlp_train_step_f32(
        _C.MLP_TRAIN_PAIRWISE, 0, 0, 1.0, xs.data_ptr(), *[p.data_ptr() for p in params], F, None, ys.data_ptr(), 0,
        n.data_ptr(), None, 0, 0, None, None, B, L, F, H1, H2, loss.data_ptr(), None, lsum.data_ptr(), state.data_ptr(),
        ctypes.byref(optim), grads.data_ptr(), ws.data_ptr(), ws_bytes, st))
    torch.cuda.synchronize()
    assert torch.equal(grads, want_grads) and torch.equal(loss, want_loss) and torch.equal(lsum, want_lsum)
    assert state[-4:].view(torch.int32).tolist() == [1, 0, 0, 0]
    got_state = fused.mlp_train_state_to_torch("adam", state.cpu(), 1, F, H1, H2)
    for i, g in enumerate(fused._split_grads(want_grads, F, H1, H2)):
        p0 = before[i]
        want_p, want_state, bound = ref.step("adam", hyper, p0, g.reshape(p0.shape).cpu().numpy(),
                                             ref.initial_state("adam", hyper, p0), 0)
        assert (np.abs(params[i].cpu().numpy() - want_p) <= bound["p"]).all(), i
        for key, want in want_state.items():
            assert (np.abs(got_state[i][key].numpy().reshape(p0.shape) - want) <= bound[key]).all(), (i, key)


# ---- 4. one step against torch.optim itself, 8. resume ----
def _torch_step(name, model, grads, state_dict=None):
    """One step of the matching torch.optim optimizer (foreach=False) on copies of the parameters, .grad = `grads`."""
    params = [torch.nn.Parameter(p.detach().clone()) for p in model._params()]
    opt = _TORCH[_algo(name)](params, foreach=False, **OPTIMS[name])
    if state_dict is not None:
        opt.load_state_dict(state_dict)
    for p, g in zip(params, grads):
        p.grad = g.clone()
    opt.step()
    return [p.detach().cpu().numpy() for p in params]


@pytest.mark.parametrize("name", list(OPTIMS))
@pytest.mark.parametrize("shape", ["3x5x8", "6x9x5"])
def test_one_step_against_torch_optim_itself(shape, name):
    B, L, F, hidden, _ = SHAPES[shape]
    model = _model("pairwise", F, hidden)
    (batch,) = _batches(shape, 1)
    trainer = _trainer(model, name)
    _, grads, _ = _existing_step(model, *batch)
    theirs = _torch_step(name, model, grads)
    before = _snapshot(trainer)
    trainer.step(*batch)
    _check_against_reference(name, before, grads, trainer)
    _check_against_reference(name, before, grads, trainer, factor=2.0, after=theirs)


@pytest.mark.parametrize("name", ["sgd", "adagrad", "adam"])
def test_resume(name):
    from pytorchltr_amd import fused
    shape = "6x9x5"
    B, L, F, hidden, _ = SHAPES[shape]
    model = _model("pairwise", F, hidden)
    batches = _batches(shape, 6)
    trainer = _trainer(model, name)
    for batch in batches[:3]:
        trainer.step(*batch)
    saved = trainer.state_dict()
    twin = copy.deepcopy(model)
    resumed = fused.MLPTrainer(twin, _algo(name), lr=123.0)              # (its hyper-parameters come from the dict)
    resumed.load_state_dict(saved)
    # (torch's SGD state has no step count: a loaded momentum buffer means "not the first step", counted as 1)
    assert resumed.steps == (1 if name == "sgd" else trainer.steps) and resumed.lr == trainer.lr
    # torch takes the same dict: one torch step on the library's gradient, within twice the bound
    _, grads, _ = _existing_step(model, *batches[3])
    theirs = _torch_step(name, model, grads, saved)
    before = _snapshot(trainer)
    for batch in batches[3:5]:
        a, b = trainer.step(*batch), resumed.step(*batch)
        assert torch.equal(a, b)
        for p, q in zip(model.parameters(), twin.parameters()):
            assert torch.equal(p, q)
        if batch is batches[3]:
            after = [p.detach().cpu().numpy().copy() for p in model._params()]
    _check_against_reference(name, before, grads, trainer, factor=2.0, after=theirs)
    _check_against_reference(name, before, grads, trainer, after=after)
    mine, theirs_state = trainer.state_dict()["state"], resumed.state_dict()["state"]
    for i in mine:
        for key in mine[i]:
            assert torch.equal(mine[i][key], theirs_state[i][key]), (i, key)


# ---- 5. write-through ----
def test_write_through_to_the_unpadded_w1():
    B, L, F, hidden, _ = SHAPES["6x9x5"]
    model = _model("pairwise", F, hidden)
    (batch,) = _batches("6x9x5", 1)
    weight = model.l1.weight
    ptr, before = weight.data_ptr(), weight.detach().clone()
    tensors = [id(p) for p in model.parameters()]
    _trainer(model, "adagrad").step(*batch)
    assert model.l1.weight is weight and weight.data_ptr() == ptr and weight.shape == (50, 5)
    assert [id(p) for p in model.parameters()] == tensors
    assert not torch.equal(weight.detach(), before) and (weight.detach() != before).float().mean() > 0.5
    xs, _, n = batch
    with torch.no_grad():
        got = model.score(xs, n).squeeze(-1)
        h = torch.relu(torch.relu(xs.double() @ model.l1.weight.double().T + model.l1.bias.double())
                       @ model.l2.weight.double().T + model.l2.bias.double())
        want = (h @ model.l3.weight.double().T + model.l3.bias.double()).squeeze(-1)
        old = torch.relu(torch.relu(xs.double() @ before.double().T + model.l1.bias.double())
                         @ model.l2.weight.double().T + model.l2.bias.double())
        old = (old @ model.l3.weight.double().T + model.l3.bias.double()).squeeze(-1)
    real = torch.arange(L, device=xs.device)[None, :] < n[:, None]
    assert torch.allclose(got[real].double(), want[real], rtol=1e-4, atol=1e-5)
    assert not torch.allclose(got[real].double(), old[real], rtol=1e-4, atol=1e-5)


# ---- 6. determinism ----
@pytest.mark.parametrize("shape", ["40x20x136", "4x300x136"])
def test_two_trainers_stay_bit_identical(shape):
    B, L, F, hidden, _ = SHAPES[shape]
    a, b = _model("lambdarank", F, hidden), _model("lambdarank", F, hidden)
    ta, tb = _trainer(a, "adam"), _trainer(b, "adam")
    for batch in _batches(shape, 5):
        la, lb = ta.step(*batch), tb.step(*batch)
        assert torch.equal(la, lb)
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)
    sa, sb = ta.state_dict()["state"], tb.state_dict()["state"]
    assert all(torch.equal(sa[i][k], sb[i][k]) for i in sa for k in sa[i])


# ---- 7. capture ----
@pytest.mark.parametrize("name", ["adam", "sgd", "adagrad"])
def test_graphed_replays_equal_eager_steps(name):
    """(Adagrad with lr_decay: its clr is the one factor linear in t, read from the device header on replay.)"""
    _graphed_replays_equal_eager_steps(name, "pairwise")


def test_graphed_listmle_in_index_tie_order():
    from pytorchltr_amd.utils import tie_breaking
    with tie_breaking("index"):
        _graphed_replays_equal_eager_steps("adam", "listmle")


def _graphed_replays_equal_eager_steps(name, family):
    shape = "40x20x136"
    B, L, F, hidden, _ = SHAPES[shape]
    batches = _batches(shape, 7)
    _trainer(_model(family, F, hidden), name).step(*batches[0])           # one-time launch set-up, outside any capture
    torch.cuda.synchronize()
    a, b = _model(family, F, hidden), _model(family, F, hidden)
    graphed_trainer, eager = _trainer(a, name), _trainer(b, name)
    call = graphed_trainer.graphed(batches[0], warmup=0)                    # so that the first REPLAY is the step t = 0
    assert graphed_trainer.steps == 0
    for batch in batches[1:]:
        lg = call(*batch).clone()
        le = eager.step(*batch)
        assert torch.equal(lg, le)
    assert graphed_trainer.steps == eager.steps == 6
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)
    sa, sb = graphed_trainer.state_dict()["state"], eager.state_dict()["state"]
    assert all(torch.equal(sa[i][k], sb[i][k]) for i in sa for k in sa[i])
    with pytest.raises(ValueError, match="captured shape"):
        call(batches[0][0][:2], batches[0][1][:2], batches[0][2][:2])


# ---- 9. empty batch and bad input ----
def test_empty_batch_changes_nothing():
    B, L, F, hidden, _ = SHAPES["3x5x8"]
    model = _model("pairwise", F, hidden)
    trainer = _trainer(model, "adam")
    (batch,) = _batches("3x5x8", 1)
    trainer.step(*batch)
    before = [p.detach().clone() for p in model.parameters()]
    state = trainer.state_dict()["state"]
    loss = trainer.step(batch[0][:0], batch[1][:0], batch[2][:0])
    assert loss.dim() == 0 and float(loss) == 0.0 and trainer.steps == 1 and model.last_losses.numel() == 0
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), before))
    after = trainer.state_dict()["state"]
    assert all(torch.equal(state[i][k], after[i][k]) for i in state for k in state[i])


def test_bad_input():
    from pytorchltr_amd import fused
    B, L, F, hidden, _ = SHAPES["3x5x8"]
    model = _model("pairwise", F, hidden)
    trainer = _trainer(model, "sgd")
    xs, ys, n = _batches("3x5x8", 1)[0]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        trainer.step(xs.cpu(), ys.cpu(), n.cpu())
    with pytest.raises(ValueError, match="features"):
        trainer.step(xs[..., :4], ys, n)
    # a network no kernel takes: the ValueError of mlp_loss_step
    big = _model("pairwise", 8, (65, 10))
    with pytest.raises(ValueError) as theirs:
        fused.mlp_loss_step(xs, [p.detach() for p in big._params()], ys, n)
    with pytest.raises(ValueError) as ours:
        _trainer(big, "sgd").step(xs, ys, n)
    assert str(ours.value) == str(theirs.value)
    assert trainer.steps == 0


# ---- 10. the padded routes: the update meets gradient columns that are no parameters ----
@pytest.mark.parametrize("name", ["sgd", "adagrad", "adam"])
@pytest.mark.parametrize("shape", PADDED)
def test_three_steps_on_the_padded_routes(shape, name):
    B, L, F, hidden, _ = SHAPES[shape]
    family = {"sgd": "pairwise", "adagrad": "lambdarank", "adam": "listnet"}[name]
    model = _model(family, F, hidden)
    weight = model.l1.weight
    ptr = weight.data_ptr()
    trainer = _trainer(model, name)
    if name == "sgd" and shape not in FUSED:
        trainer.lr = 2e-4               # (as test_ten_consecutive_steps: pair sums in the hundreds)
    for step, batch in enumerate(_batches(shape, 3)):
        _, grads, _ = _existing_step(model, *batch)
        assert all(torch.isfinite(g).all() for g in grads)
        before = _snapshot(trainer)
        loss, got = trainer.step(*batch, return_grads=True)
        for g, w, p in zip(got, grads, model._params()):
            assert g.shape == w.shape == p.shape and torch.equal(g, w)
        assert torch.isfinite(loss)
        _check_against_reference(name, before, grads, trainer)
        assert trainer.steps == step + 1
        assert model.l1.weight is weight and weight.data_ptr() == ptr and weight.shape == (hidden[0], F)


# ---- 11. one trainer, two row widths: the state re-laid through torch's form ----
@pytest.mark.parametrize("name", ["adagrad", "adam", "sgd"])
def test_one_trainer_two_row_widths(name):
    """F = 44: an fp32 batch has rows of 44 floats, a bf16 batch (padded to 8) of 48, and the trainer re-lays its flat
    state at each change.  Two fp32 steps, two bf16 steps, two fp32 steps, each within the bound from its snapshot;
    the state after a change is the state before it bit for bit on the real columns, zero on the padding.  The step
    count runs on for Adagrad and Adam; SGD's restarts at 1 (MLPTrainer.steps says why)."""
    F, hidden = 44, (5, 3)
    model = _model("pairwise", F, hidden)
    trainer = _trainer(model, name)
    plan = [("3x9x44", 0), ("3x9x44", 1), ("3x9x44-bf16", 0), ("3x9x44-bf16", 1), ("3x9x44", 2), ("3x9x44", 3)]
    want_steps = [1, 2, 2, 3, 2, 3] if name == "sgd" else [1, 2, 3, 4, 5, 6]
    width = None
    for step, (shape, which) in enumerate(plan):
        batch = _batches(shape, 4)[which]
        if width is not None and width != shape:
            params0, state0, t0 = _snapshot(trainer)
            trainer._prime(batch[0])                      # (what graphed() calls ahead of a capture: the re-lay alone)
            Fp = 48 if shape.endswith("bf16") else 44
            assert trainer._state_Fp == Fp
            state1 = trainer.state_dict()["state"]
            assert sorted(state1) == sorted(state0) == list(range(6))
            for i in state0:
                for key in state0[i]:
                    assert state1[i][key].shape == state0[i][key].shape and torch.equal(state1[i][key], state0[i][key])
            rows = trainer._state[:hidden[0] * Fp].view(hidden[0], Fp)
            assert Fp == F or (rows[:, F:] == 0).all()
            assert trainer.steps == (1 if name == "sgd" else t0)
        width = shape
        _, grads, _ = _existing_step(model, *batch)
        before = _snapshot(trainer)
        _, got = trainer.step(*batch, return_grads=True)
        assert all(torch.equal(g, w) for g, w in zip(got, grads))
        _check_against_reference(name, before, grads, trainer)
        assert trainer.steps == want_steps[step]


# ---- 12. hidden sizes on the fused route ----
@pytest.mark.parametrize("layout", ["tile", "wide"])
@pytest.mark.parametrize("name", ["sgd", "adagrad", "adam"])
@pytest.mark.parametrize("hidden", [(1, 1), (17, 5), (64, 16)], ids=["1x1", "17x5", "64x16"])
def test_hidden_sizes_on_the_fused_route(hidden, name, layout):
    B, L, F, _, _ = OTHER["4x6x8"]
    model = _model("pairwise", F, hidden)
    (batch,) = _batches("4x6x8", 1)
    trainer = _trainer(model, name)
    with _Layout(layout):
        _, grads, _ = _existing_step(model, *batch)
        before = _snapshot(trainer)
        _, got = trainer.step(*batch, return_grads=True)
        for g, w in zip(got, grads):
            assert g.shape == w.shape and torch.equal(g, w)
    _check_against_reference(name, before, grads, trainer)
    assert trainer.steps == 1


# ---- 13. from torch to the trainer ----
@pytest.mark.parametrize("name", list(OPTIMS))
def test_load_a_torch_optimizers_state(name):
    """torch.optim on the model's own parameters takes three steps on the library's gradients; its state_dict goes
    into a fresh MLPTrainer on a copy of the model; step 4 of both against the reference of that step from the loaded
    state -- the trainer at factor 1, torch at factor 2."""
    from pytorchltr_amd import fused
    shape = "6x9x5"
    B, L, F, hidden, _ = SHAPES[shape]
    model = _model("pairwise", F, hidden)
    batches = _batches(shape, 4)
    params = list(model._params())
    opt = _TORCH[_algo(name)](params, foreach=False, **OPTIMS[name])

    def torch_step(batch):
        _, grads, _ = _existing_step(model, *batch)
        for p, g in zip(params, grads):
            p.grad = g.clone()
        opt.step()
        return grads

    for batch in batches[:3]:
        torch_step(batch)
    twin = copy.deepcopy(model)
    for p in twin.parameters():
        p.grad = None
    trainer = fused.MLPTrainer(twin, _algo(name), lr=123.0)
    trainer.load_state_dict(opt.state_dict())
    # (torch's SGD keeps no count: a momentum buffer reads as 1, none -- plain SGD has no state at all -- as 0)
    assert trainer.steps == {"sgd": 1, "sgd-nesterov": 1, "sgd-plain": 0}.get(name, 3)
    assert trainer.lr == OPTIMS[name]["lr"]
    before = _snapshot(trainer)
    assert all(np.array_equal(a, p.detach().cpu().numpy()) for a, p in zip(before[0], params))
    grads = torch_step(batches[3])
    theirs = [p.detach().cpu().numpy() for p in params]
    trainer.step(*batches[3])
    _check_against_reference(name, before, grads, trainer)
    _check_against_reference(name, before, grads, trainer, factor=2.0, after=theirs)
    for p in params:
        p.grad = None


def test_load_a_torch_sgd_that_never_stepped():
    """Its state is empty: the trainer's first step takes the t == 0 rule (the buffer becomes g, not 0.7 g)."""
    from pytorchltr_amd import fused
    shape, name = "6x9x5", "sgd"
    B, L, F, hidden, _ = SHAPES[shape]
    model = _model("pairwise", F, hidden)
    (batch,) = _batches(shape, 1)
    opt = torch.optim.SGD(list(model._params()), **OPTIMS[name])
    trainer = fused.MLPTrainer(model, "sgd", lr=123.0)
    trainer.load_state_dict(opt.state_dict())
    assert trainer.steps == 0 and trainer.state_dict()["state"] == {}
    _, grads, _ = _existing_step(model, *batch)
    before = _snapshot(trainer)
    assert before[2] == 0
    trainer.step(*batch)
    _check_against_reference(name, before, grads, trainer)
    assert trainer.steps == 1


# ---- 14. a learning-rate schedule ----
@pytest.mark.parametrize("name", ["adagrad", "sgd-nesterov"])
def test_a_schedule_set_through_lr(name):
    """trainer.lr = lr0 * 0.5 ** (step // 2) before each of six eager steps, against torch.optim under LambdaLR with
    the same factor: per step, from the trainer's snapshot (parameters and state go into the torch optimizer, its
    learning rate stays the scheduler's), torch at factor 2 and the trainer at factor 1 of the reference."""
    shape = "3x5x8"
    B, L, F, hidden, _ = SHAPES[shape]
    model = _model("pairwise", F, hidden)
    trainer = _trainer(model, name)
    lr0 = OPTIMS[name]["lr"]
    params = [torch.nn.Parameter(p.detach().clone()) for p in model._params()]
    opt = _TORCH[_algo(name)](params, foreach=False, **OPTIMS[name])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda epoch: 0.5 ** (epoch // 2))
    for step, batch in enumerate(_batches(shape, 6)):
        trainer.lr = lr0 * 0.5 ** (step // 2)
        assert opt.param_groups[0]["lr"] == trainer.lr
        _, grads, _ = _existing_step(model, *batch)
        before = _snapshot(trainer)
        sd = opt.state_dict()
        sd["state"] = copy.deepcopy(before[1])            # (torch keeps and steps the tensors it loads, in place)
        opt.load_state_dict(sd)
        with torch.no_grad():
            for p, q, g in zip(params, model._params(), grads):
                p.copy_(q)
                p.grad = g.clone()
        opt.step()
        sched.step()
        theirs = [p.detach().cpu().numpy() for p in params]
        trainer.step(*batch)
        _check_against_reference(name, before, grads, trainer)
        _check_against_reference(name, before, grads, trainer, factor=2.0, after=theirs)
    assert trainer.lr == lr0 * 0.25 and trainer.steps == 6
