"""GPU tier: pytorchltr_amd.optim.SGD against torch.optim.SGD through everything a training script does with an optimizer
besides stepping it -- resume, load_state_dict, schedulers attached late, param groups, reads and writes of the parameters,
`.grad` handling, closures, GradScaler, freezing, pickling (tests/test_optim_host.py is the CPU tier).

Every scenario is ONE script of events applied in lock step to four trainings that start from one nn.Linear(F, 1):

    (a)  "lazy":  pytorchltr_amd.optim.SGD on a use_linear_scorer copy, lr 0.05      -- the code under test
    (b)  "fused": torch.optim.SGD on a use_linear_scorer copy, lr 0.05               -- the reference
    (b') "fused": the same at lr 0.002
    (c)  "plain": torch.optim.SGD on the nn.Linear itself, lr 0.002

An event is a callable ``ev(t)`` on a training ``t`` (``t.model``, ``t.opt``, ``t.state``; an event may replace the model and
the optimizer, which is why it gets the holder; every lr in a script is a multiple of ``t.lr``).  (a) is compared with (b),
(b') with (c), at tests/test_gpu_optim.py's bounds: weights and bias rtol 1e-5 / atol 1e-6, per-step mean losses rtol 2e-5 /
atol 1e-6, gradients rtol 1e-4 / atol 1e-5 max(1, |g|max).

Why (c) runs at a lower lr: (b) and (c) compute one gradient by two fp32 routes (the fused kernel's rows; rocBLAS scores and
autograd) that agree to about 1e-6 of its size, and a step puts lr x that into the weights whatever the optimizer.  Measured
on an MI355X at lr 0.05, (b) from (c) is 1.2 to 1.9 x the weight bound after three to eight plain steps and up to 9.5e-6 with
momentum 0.9: no reference at that lr.  At lr 0.002 it stays below 0.5 x the bound.  (a) and (b) share the kernel and are held
to the bound at lr 0.05.

Two reading disciplines: `quiet` -- nothing reads a parameter or gradient value of (a) until the end, except what the event
itself is about, so pending updates span the events (where the bugs live); `look` -- the weights are compared after every
event, and every comparison applies the pending update.

Every scenario asserts that (a) really had an update pending after a plain step (else it would pass on the ordinary path), and
one that changes a hyper-parameter also runs (b) on the "bug trajectory" -- the change not applied -- and asserts that its
final weights differ from (b)'s by more than 100 x the weight bound: the scenario can tell right from wrong.

Shapes: 32 x 64 x 136 hinge and 24 x 50 x 136 logistic, the smallest of test_gpu_optim.py that take the register tile and so
the lazy launch; six to eight steps per scenario.
"""
import collections
import copy
import functools
import io
import pickle

import pytest
import torch
import torch.nn.functional as F_

from tests.test_gpu_optim import _data, _loop, _models

pytestmark = pytest.mark.gpu

W_RTOL, W_ATOL = 1e-5, 1e-6
L_RTOL, L_ATOL = 2e-5, 1e-6
LR = 0.05                               # (a) and (b)
LR_PLAIN = 0.002                        # (b') and (c): the module docstring
WORKLOADS = {"hinge": (32, 64, 136), "logistic": (24, 50, 136)}
both_workloads = pytest.mark.parametrize("workload", sorted(WORKLOADS))
both_disciplines = pytest.mark.parametrize("discipline", ["quiet", "look"])


@functools.lru_cache(maxsize=None)
def _batches(workload):
    """Eight batches of the workload, made once and never written to."""
    B, L, F = WORKLOADS[workload]
    return tuple(_data(8, B, L, F, 4200 + B, torch.device("cuda")))


def _loss_fn(workload):
    from pytorchltr_amd import loss as L_
    return {"hinge": L_.PairwiseHingeLoss, "logistic": L_.PairwiseLogisticLoss}[workload]()


def _scorers(model):
    return [model] if hasattr(model, "weight") else list(model)


def _params(model):
    return [p for m in _scorers(model) for p in (m.weight, m.bias)]


def _one_group(cls, model, lr, **kw):
    return cls(model.parameters(), lr=lr, **kw)


class _Training:
    def __init__(self, role, model, build_opt, workload, lr):
        from pytorchltr_amd.optim import SGD
        self.role = role
        self.cls = SGD if role == "lazy" else torch.optim.SGD
        self.lr = lr
        self.model = model
        self.opt = build_opt(self.cls, model, lr)
        self.loss_fn = _loss_fn(workload)
        self.data = _batches(workload)
        self.F = WORKLOADS[workload][2]
        self.losses = []
        self.state = {}
        self.discipline = "quiet"

    def expect_pending(self):
        """Under `quiet` the steps before this event have left an update of (a) pending (under `look` the comparison after
        them applied it)."""
        if self.role == "lazy" and self.discipline == "quiet":
            assert self.lazy_state().pending is not None

    def fresh_model(self, seed):
        """A new model of this training's kind with other initial weights."""
        from pytorchltr_amd.fused import use_linear_scorer
        torch.manual_seed(seed)
        lin = torch.nn.Linear(self.F, 1).to("cuda")
        return lin if self.role == "plain" else use_linear_scorer(lin)

    def lazy_state(self, i=0):
        return _scorers(self.model)[i].weight._ltr_lazy

    def note_pending(self):
        if self.role == "lazy" and self.lazy_state().pending is not None:
            self.state["saw_pending"] = True


def _trainings(workload, build_opt=_one_group, scorers=1):
    """[(b), (a), (b'), (c)] -- a reference runs every event before the training that is compared with it (ReduceLROnPlateau
    is fed ITS losses in both)."""
    dev = torch.device("cuda")
    F = WORKLOADS[workload][2]

    def models():                           # (lin, a use_linear_scorer copy, another) per scorer: the same in every call
        sets = [_models(F, dev, seed=3 + i) for i in range(scorers)]
        return (lambda k: sets[0][k]) if scorers == 1 else (lambda k: torch.nn.ModuleList([s[k] for s in sets]))
    hi, lo = models(), models()
    return [_Training("fused", hi(1), build_opt, workload, LR), _Training("lazy", hi(2), build_opt, workload, LR),
            _Training("fused", lo(1), build_opt, workload, LR_PLAIN), _Training("plain", lo(0), build_opt, workload, LR_PLAIN)]


def _weights_close(t, ref, what):
    for i, (p, q) in enumerate(zip(_params(t.model), _params(ref.model))):
        p, q = p.detach(), q.detach()
        ratio = float(((p - q).abs() / (W_ATOL + W_RTOL * q.abs())).max())
        print("%s: %s vs %s, parameter %d: max |d| %.3e, %.2f x the bound" % (
            what, t.role, ref.role, i, float((p - q).abs().max()), ratio))
        assert torch.allclose(p, q, rtol=W_RTOL, atol=W_ATOL), \
            "%s: %s vs %s, parameter %d: max |d| %.3e" % (what, t.role, ref.role, i, float((p - q).abs().max()))


def _grad_close(g, want):
    return torch.allclose(g, want, rtol=1e-4, atol=1e-5 * max(1.0, float(want.abs().max())))


Played = collections.namedtuple("Played", "lazy ref pairs")         # pairs: ((a), (b)) and ((b'), (c))


def _play(workload, discipline, events, build_opt=_one_group, scorers=1, must_go_lazy=True):
    """Applies the script to the four trainings in lock step and compares (a) with (b) and (b') with (c)."""
    ref, lazy, ref_lo, plain = ts = _trainings(workload, build_opt, scorers)
    pairs = ((lazy, ref), (ref_lo, plain))
    for t in ts:
        t.discipline = discipline
    for k, ev in enumerate(events):
        for t in ts:
            ev(t)
        if discipline == "look":
            for t, r in pairs:
                _weights_close(t, r, "after event %d (%s)" % (k, getattr(ev, "__qualname__", ev)))
    assert lazy.state.get("saw_pending") or not must_go_lazy, \
        "no update of (a) was ever pending: the scenario ran on the ordinary path"
    for t, r in pairs:
        l_t, l_r = torch.cat(t.losses), torch.cat(r.losses)
        print("losses: %s vs %s %.3e (of %.3e)" % (t.role, r.role, float((l_t - l_r).abs().max()), float(l_r.abs().max())))
        assert torch.allclose(l_t, l_r, rtol=L_RTOL, atol=L_ATOL), (t.role, r.role, float((l_t - l_r).abs().max()))
        _weights_close(t, r, "at the end")
    for st in lazy.opt._lazy:
        assert st.pending is None                                        # (the comparison read the weights)
    return Played(lazy, ref, pairs)


def _control(workload, right, wrong, build_opt=_one_group, scorers=1):
    """The reference on the script and on its bug trajectory: the final weights are further apart than 100 x the weight bound."""
    finals = []
    for events in (right, wrong):
        t = _trainings(workload, build_opt, scorers)[0]
        for ev in events:
            ev(t)
        finals.append(torch.cat([p.detach().reshape(-1) for p in _params(t.model)]))
    good, bad = finals
    ratio = float(((good - bad).abs() / (W_ATOL + W_RTOL * good.abs())).max())
    print("control %s: bug trajectory is %.0f x the weight bound away" % (workload, ratio))
    assert ratio > 100.0, ratio


# ---- events ----
def steps(i, j):
    def steps_(t):
        models = _scorers(t.model)
        if len(models) == 1:
            t.losses.append(_loop(t.model, t.opt, t.loss_fn, t.data[i:j]))
        else:
            for xs, ys, n in t.data[i:j]:
                loss = t.loss_fn(models[0](xs), ys, n).mean() + t.loss_fn(models[1](xs), ys, n).mean()
                t.opt.zero_grad()
                loss.backward()
                t.opt.step()
                t.losses.append(loss.detach().reshape(1))
        t.note_pending()
    return steps_


def _round_trip(obj):
    buf = io.BytesIO()
    torch.save(obj, buf)
    buf.seek(0)
    return torch.load(buf)


def save(t):
    t.state["ckpt"] = _round_trip({"model": t.model.state_dict(), "opt": t.opt.state_dict()})


def load_opt(change=None, pending=True):
    """In-place optimizer.load_state_dict of the saved state with `change(state_dict)` applied; `pending`: the steps since
    the save have left an update of (a) pending."""
    def load_opt_(t):
        if pending:
            t.expect_pending()
        sd = copy.deepcopy(t.state["ckpt"]["opt"])
        if change is not None:
            change(sd, t)
        t.opt.load_state_dict(sd)
    return load_opt_


def set_groups(lr_times=None, **kw):
    def change(sd, t):
        for g in sd["param_groups"]:
            g.update(kw)
            if lr_times is not None:
                g["lr"] = t.lr * lr_times
    return change


def left_the_lazy_path(t):
    if t.role == "lazy":
        for st in t.opt._lazy:
            assert st.pending is None and not st.plain_sgd()


# ---- resume ----
def resume(ctor_lr_times, load_optimizer=True):
    def resume_(t):
        ckpt = t.state["ckpt"]
        t.model = t.fresh_model(seed=77)
        t.model.load_state_dict(ckpt["model"])
        t.opt = t.cls(t.model.parameters(), lr=t.lr * ctor_lr_times)
        if load_optimizer:
            t.opt.load_state_dict(ckpt["opt"])
    return resume_


@both_disciplines
@both_workloads
def test_resume_into_fresh_objects(workload, discipline):
    def script(bug=False):
        return [steps(0, 3), save, resume(0.1, load_optimizer=not bug), steps(3, 6)]
    lazy = _play(workload, discipline, script()).lazy
    assert lazy.lazy_state().group is lazy.opt.param_groups[0] and lazy.opt.param_groups[0]["lr"] == LR
    _control(workload, script(), script(bug=True))


@both_disciplines
@both_workloads
def test_load_state_dict_in_place_with_an_update_pending_and_another_lr(workload, discipline):
    """The pending step is applied with the lr of the step that recorded it, the later ones use the loaded lr."""
    def script(bug=False):
        return [steps(0, 2), save, steps(2, 4), load_opt(None if bug else set_groups(lr_times=0.1)), steps(4, 7)]
    _play(workload, discipline, script())
    _control(workload, script(), script(bug=True))


def _momentum_buffers(sd, t):
    g = torch.Generator().manual_seed(9)
    sd["state"] = {i: {"momentum_buffer": (torch.randn(p.shape, generator=g) * 0.1).to(p.device)}
                   for i, p in enumerate(_params(t.model))}


def _with_buffers(sd, t):
    set_groups(momentum=0.9)(sd, t)
    _momentum_buffers(sd, t)


NOT_PLAIN = {"momentum": set_groups(momentum=0.9), "momentum with buffers": _with_buffers,
             "weight decay": set_groups(weight_decay=0.01), "nesterov": set_groups(momentum=0.9, nesterov=True)}


@pytest.mark.parametrize("case", sorted(NOT_PLAIN))
@both_disciplines
@both_workloads
def test_a_loaded_state_that_is_no_longer_plain_sgd(workload, discipline, case):
    def script(bug=False):
        return [steps(0, 1), save, steps(1, 2), load_opt(None if bug else NOT_PLAIN[case]), steps(2, 8), left_the_lazy_path]
    _play(workload, discipline, script())
    _control(workload, script()[:-1], script(bug=True)[:-1])


@both_disciplines
@both_workloads
def test_a_plain_state_loaded_into_a_momentum_optimizer(workload, discipline):
    def plain(sd, t):
        set_groups(momentum=0)(sd, t)
        sd["state"] = {}

    def script(bug=False):
        return [steps(0, 2), save, steps(2, 3), load_opt(None if bug else plain, pending=False), steps(3, 7)]
    build = functools.partial(_one_group, momentum=0.9)
    _play(workload, discipline, script(), build, must_go_lazy=False)     # (parity is asked, the lazy path is not)
    _control(workload, script(), script(bug=True), build)


# ---- schedulers and assignments after a load ----
def attach(make):
    def attach_(t):
        t.state["sched"] = make(t.opt)
    return attach_


def sched_step(t):
    t.state["sched"].step()


def plateau_step(shared):
    """ReduceLROnPlateau fed the same Python floats in both trainings of a pair: the reference's losses (it runs every event
    first)."""
    def plateau_step_(t):
        k = (t.lr, sum(len(x) for x in t.losses))
        if t.role == "fused":
            shared[k] = float(t.losses[-1][-1])
        t.state["sched"].step(shared[k])
    return plateau_step_


def scale_lr(t):
    for g in t.opt.param_groups:
        g["lr"] *= 0.1


def set_momentum(t):
    t.expect_pending()
    t.opt.param_groups[0]["momentum"] = 0.9


def _after_a_load(case, bug=False):
    head = [steps(0, 2), save, steps(2, 3), load_opt(set_groups(lr_times=0.4))]
    sched = torch.optim.lr_scheduler
    if case in ("StepLR", "LambdaLR", "ReduceLROnPlateau"):
        make = {"StepLR": lambda o: sched.StepLR(o, 1, gamma=0.5),
                "LambdaLR": lambda o: sched.LambdaLR(o, lambda epoch: 1.0 / (1 + 2 * epoch)),
                # (mode="max" on a falling loss with no patience: every step but the first is a plateau and halves the lr)
                "ReduceLROnPlateau": lambda o: sched.ReduceLROnPlateau(o, mode="max", factor=0.5, patience=0)}[case]
        tick = plateau_step({}) if case == "ReduceLROnPlateau" else sched_step
        tail = []
        for k in range(3, 7):
            tail += [steps(k, k + 1)] + ([] if bug else [tick])
        return head + [attach(make)] + tail + [steps(7, 8)]
    head += [steps(3, 4)]
    if case == "assignment":
        return head + ([] if bug else [scale_lr]) + [steps(4, 8)]
    assert case == "momentum"
    return head + ([] if bug else [set_momentum]) + [steps(4, 8)] + ([] if bug else [left_the_lazy_path])


@pytest.mark.parametrize("case", ["StepLR", "LambdaLR", "ReduceLROnPlateau", "assignment", "momentum"])
@both_disciplines
@both_workloads
def test_schedulers_and_assignments_after_a_load(workload, discipline, case):
    lazy = _play(workload, discipline, _after_a_load(case)).lazy
    assert lazy.lazy_state().group is lazy.opt.param_groups[0]
    _control(workload, _after_a_load(case), _after_a_load(case, bug=True))


# ---- groups ----
def _two_groups(cls, model, lr):
    return cls([{"params": list(m.parameters()), "lr": x} for m, x in zip(model, (lr, lr / 10))], lr=1.0)


def _first_only(cls, model, lr):
    return cls(model[0].parameters(), lr=lr)


def add_second(t):
    t.opt.add_param_group({"params": list(t.model[1].parameters()), "lr": t.lr / 10})


def swap_lrs(sd, t):
    a, b = sd["param_groups"]
    a["lr"], b["lr"] = b["lr"], a["lr"]


@pytest.mark.parametrize("case", ["two groups", "add_param_group", "load swaps the lrs"])
@both_disciplines
@both_workloads
def test_two_scorers_in_two_groups(workload, discipline, case):
    if case == "two groups":
        build, script = _two_groups, lambda bug=False: [steps(0, 6)]
    elif case == "add_param_group":
        build, script = _first_only, lambda bug=False: [steps(0, 2), add_second, steps(2, 7)]
    else:
        build = _two_groups

        def script(bug=False):
            return [steps(0, 2), save, steps(2, 3), load_opt(None if bug else swap_lrs), steps(3, 7)]
    lazy = _play(workload, discipline, script(), build, scorers=2).lazy
    assert len(lazy.opt._lazy) == 2                                      # both scorers are updated lazily
    for st, group in zip(lazy.opt._lazy, lazy.opt.param_groups):
        assert st.group is group
    if case == "load swaps the lrs":
        _control(workload, script(), script(bug=True), build, scorers=2)


# ---- reads and writes while an update is pending ----
def _nested_cat(groups):
    """A torch-function-aware library function whose argument nests tensors two levels deep: a tuple inside a list."""
    flat = [v for g in groups for v in g]
    if torch.overrides.has_torch_function(flat):
        return torch.overrides.handle_torch_function(_nested_cat, flat, groups)
    return torch.cat([v.reshape(-1) for v in flat])


def _param_bound(v):
    return W_ATOL + W_RTOL * v.abs()


# read(x, w, b) -> value, and bound(x, w, b) -> how far two values may be apart when w and b agree within the weight bound:
# the weight bound pushed through the (linear) read, plus -- where the read sums -- two fp32 dot-product roundings F eps |x|.|w|
READS = {
    "F.linear(x, weight=w, bias=b)": (
        lambda x, w, b: F_.linear(x, weight=w, bias=b),
        lambda x, w, b: (x.abs() @ _param_bound(w).T + _param_bound(b)
                         + 2 * x.shape[-1] * 2.0 ** -24 * (x.abs() @ w.abs().T + b.abs()))),
    "torch.mul(x, other=w)": (
        lambda x, w, b: torch.mul(x, other=w),
        lambda x, w, b: x.abs() * _param_bound(w) + 2.0 ** -23 * (x * w).abs()),
    "torch.cat(tensors=[w, w])": (
        lambda x, w, b: torch.cat(tensors=[w, w]), lambda x, w, b: _param_bound(torch.cat([w, w]))),
    "a tuple inside a list": (
        lambda x, w, b: _nested_cat([(w, b)]), lambda x, w, b: _param_bound(torch.cat([w.reshape(-1), b]))),
    "parameters_to_vector": (
        lambda x, w, b: torch.nn.utils.parameters_to_vector([w, b]),
        lambda x, w, b: _param_bound(torch.cat([w.reshape(-1), b]))),
}


def read(how):
    def read_(t):
        t.expect_pending()
        x = t.data[0][0][0]
        with torch.no_grad():
            t.state["read"] = READS[how][0](x, t.model.weight, t.model.bias).clone()
            t.state["bound"] = READS[how][1](x, t.model.weight.detach(), t.model.bias.detach())     # (from |w| as read)
        assert t.role != "lazy" or t.lazy_state().pending is None
    return read_


@pytest.mark.parametrize("how", sorted(READS))
@both_disciplines
@both_workloads
def test_reads_while_an_update_is_pending(workload, discipline, how):
    for t, r in _play(workload, discipline, [steps(0, 3), read(how), steps(3, 6)]).pairs:
        d, bound = (t.state["read"] - r.state["read"]).abs(), r.state["bound"]
        assert bool((d <= bound).all()), "%s vs %s: %.3e over the bound" % (t.role, r.role, float((d - bound).max()))


def _other_weights(t):
    g = torch.Generator().manual_seed(21)
    return {"weight": torch.randn(1, t.F, generator=g) * 0.05, "bias": torch.randn(1, generator=g) * 0.05}


def _write_load(t):
    t.model.load_state_dict(_other_weights(t))


def _write_mul(t):
    with torch.no_grad():
        t.model.weight.mul_(0.5)


def _write_data_mul(t):
    t.model.weight.data.mul_(0.5)


WRITES = {"model.load_state_dict": _write_load, "no_grad mul_": _write_mul, "data.mul_": _write_data_mul}


def write(how):
    def write_(t):
        t.expect_pending()
        WRITES[how](t)
        assert t.role != "lazy" or t.lazy_state().pending is None       # it landed BEFORE the write, and only once
    return write_


@pytest.mark.parametrize("how", sorted(WRITES))
@both_disciplines
@both_workloads
def test_writes_while_an_update_is_pending(workload, discipline, how):
    _play(workload, discipline, [steps(0, 3), write(how), steps(3, 6)])


# ---- `.grad` ----
CLIP = 0.5


def clipped_step(clone):
    def clipped_step_(t):
        xs, ys, n = t.data[2]
        loss = t.loss_fn(t.model(xs), ys, n).mean()
        t.opt.zero_grad()
        loss.backward()
        params = _params(t.model)
        t.state["saved"] = [clone(p.grad) for p in params]
        t.state["alias"] = [p.grad.detach() for p in params]
        t.state["norm"] = torch.nn.utils.clip_grad_norm_(params, CLIP)
        t.opt.step()
        t.losses.append(loss.detach().reshape(1))
        t.state["grad"] = [p.grad for p in params]
    return clipped_step_


def _dispatch_clone(g):
    with torch._C.DisableTorchFunctionSubclass():                       # (as C++ callers reach it: __torch_dispatch__ only)
        return torch.ops.aten.clone.default(g)


@pytest.mark.parametrize("clone", ["Tensor.clone", "aten.clone", "aten.clone below the Python API"])
@both_disciplines
@both_workloads
def test_grad_clone_clip_and_step(workload, discipline, clone):
    fn = {"Tensor.clone": lambda g: g.clone(), "aten.clone": torch.ops.aten.clone.default}.get(clone, _dispatch_clone)
    for t, r in _play(workload, discipline, [steps(0, 2), clipped_step(fn), steps(3, 6)]).pairs:
        assert float(r.state["norm"]) > 4 * CLIP                        # (it clipped)
        assert torch.allclose(t.state["norm"], r.state["norm"], rtol=1e-4)
        for i in range(2):
            assert _grad_close(t.state["saved"][i], r.state["saved"][i]), i            # unclipped, untouched by the clipping
            assert _grad_close(t.state["grad"][i], r.state["grad"][i]), i              # clipped
            assert torch.equal(t.state["alias"][i], t.state["grad"][i]), i             # detach() is an alias, as in torch
        assert not torch.allclose(t.state["saved"][0], t.state["grad"][0], rtol=0.5, atol=0)


# ---- step twice, step without a backward, closure ----
def step_again(t):
    t.opt.step()


def step_with_nothing(t):
    t.opt.zero_grad()
    t.opt.step()


@both_disciplines
@both_workloads
def test_stepping_twice_and_stepping_without_a_backward(workload, discipline):
    def script(bug=False):
        return [step_with_nothing, steps(0, 2)] + ([] if bug else [step_again]) + [step_with_nothing, steps(2, 4),
                                                                                 step_with_nothing, steps(4, 6)]
    _play(workload, discipline, script())
    _control(workload, script(), script(bug=True))                       # (the second step applied the gradient again)


def closure_steps(i, j):
    def closure_steps_(t):
        for xs, ys, n in t.data[i:j]:
            def closure():
                t.opt.zero_grad()
                loss = t.loss_fn(t.model(xs), ys, n).mean()
                loss.backward()
                return loss
            t.losses.append(t.opt.step(closure).detach().reshape(1))
        t.note_pending()
    return closure_steps_


@both_disciplines
@both_workloads
def test_step_with_a_closure(workload, discipline):
    _play(workload, discipline, [closure_steps(0, 3), steps(3, 5), closure_steps(5, 7)])


# ---- GradScaler ----
def scaler_steps(i, j):
    def scaler_steps_(t):
        scaler = t.state.setdefault("scaler", torch.amp.GradScaler("cuda", init_scale=1024.))
        for xs, ys, n in t.data[i:j]:
            loss = t.loss_fn(t.model(xs), ys, n).mean()
            t.opt.zero_grad()
            scaler.scale(loss).backward()
            scaler.unscale_(t.opt)
            torch.nn.utils.clip_grad_norm_(_params(t.model), 50.0)
            scaler.step(t.opt)
            scaler.update()
            t.losses.append(loss.detach().reshape(1))
    return scaler_steps_


@both_disciplines
@both_workloads
def test_grad_scaler_on_the_fp32_loop(workload, discipline):
    lazy, ref, _ = _play(workload, discipline, [steps(0, 2), scaler_steps(2, 6), steps(6, 7)])
    assert lazy.state["scaler"].get_scale() == ref.state["scaler"].get_scale() == 1024.


# ---- freeze / unfreeze ----
def frozen_passes(t):
    t.model.requires_grad_(False)
    for xs, ys, n in t.data[6:8]:
        t.losses.append(t.loss_fn(t.model(xs), ys, n).mean().detach().reshape(1))
    t.model.requires_grad_(True)


@both_disciplines
@both_workloads
def test_freeze_and_unfreeze_between_steps(workload, discipline):
    _play(workload, discipline, [steps(0, 3), frozen_passes, steps(3, 6)])


# ---- serialisation with an update pending ----
def _flat(model):
    return torch.cat([p.detach().reshape(-1) for p in _params(model)]).clone()


def save_whole_model(t):
    """torch.save(model) / torch.load: the loaded weights, and the loaded model trained on under a fresh optimizer of either
    class."""
    from pytorchltr_amd.optim import SGD
    t.expect_pending()
    buf = io.BytesIO()
    torch.save(t.model, buf)
    twins = []
    for cls in (t.cls, SGD if t.role == "fused" else torch.optim.SGD):
        buf.seek(0)
        twin = torch.load(buf, weights_only=False)
        assert all(type(p) is torch.nn.Parameter and not hasattr(p, "_ltr_lazy") for p in twin.parameters())
        twins.append(_flat(twin))
        losses = _loop(twin, cls(twin.parameters(), lr=t.lr), t.loss_fn, t.data[6:8])
        twins += [_flat(twin), losses]
    t.state["twins"] = twins


def deepcopy_model(t):
    t.expect_pending()
    twin = copy.deepcopy(t.model)
    assert all(type(p) is torch.nn.Parameter and not hasattr(p, "_ltr_lazy") for p in twin.parameters())
    t.state["copy"] = _flat(twin)


def _by_pickle(obj):
    return pickle.loads(pickle.dumps(obj))


def copy_optimizer(t):
    """copy.deepcopy and a pickle round trip of the optimizer: alone (its parameters are copies without gradients: step() has
    nothing to do), and together with the model, which the copy then trains for a step."""
    t.expect_pending()
    groups = t.opt.state_dict()["param_groups"]
    mine = {p.data_ptr() for p in _params(t.model)}
    for twin_of in (copy.deepcopy, _by_pickle):
        twin = twin_of(t.opt)
        model, opt = twin_of((t.model, t.opt))
        for o in (twin, opt):
            assert type(o) is type(t.opt)
            o.step()
            if hasattr(o, "flush"):
                o.flush()
            assert o.state_dict()["param_groups"] == groups and groups[0]["lr"] == t.lr
            copies = [p for g in o.param_groups for p in g["params"]]
            assert not {p.data_ptr() for p in copies} & mine
            t.state.setdefault("opt copies", []).append(torch.cat([p.detach().reshape(-1) for p in copies]))
        assert all(p is q for p, q in zip(_params(model), copies))       # (the copy's optimizer holds the copy's parameters)
        losses = _loop(model, opt, t.loss_fn, t.data[7:8])
        t.state["opt copies"] += [_flat(model), losses]


@both_disciplines
@both_workloads
def test_serialisation_with_an_update_pending(workload, discipline):
    lazy, _, pairs = _play(workload, discipline, [steps(0, 3), save_whole_model, steps(3, 4), deepcopy_model, steps(4, 5),
                                                  copy_optimizer, steps(5, 7)])
    for t, r in pairs:
        for got, want in zip(t.state["twins"] + [t.state["copy"]] + t.state["opt copies"],
                             r.state["twins"] + [r.state["copy"]] + r.state["opt copies"]):
            close = torch.allclose(got, want, rtol=L_RTOL if got.numel() <= 2 else W_RTOL, atol=W_ATOL)
            assert close, (t.role, r.role, got.numel(), float((got - want).abs().max()))
    # the loaded scorer pairs its parameters up again: under a fresh optim.SGD it is back on the lazy path
    buf = io.BytesIO()
    torch.save(lazy.model, buf)
    buf.seek(0)
    twin = torch.load(buf, weights_only=False)
    opt = lazy.cls(twin.parameters(), lr=LR)
    _loop(twin, opt, lazy.loss_fn, lazy.data[:2])
    assert len(opt._lazy) == 1 and opt._lazy[0].pending is not None


# ---- a second optimizer over the same scorer ----
def second_optimizer(t):
    if t.role == "lazy":
        with pytest.raises(ValueError, match="already belong to another"):
            t.cls(t.model.parameters(), lr=LR)
        assert t.lazy_state() is t.opt._lazy[0]
        t.expect_pending()


@both_disciplines
@both_workloads
def test_a_second_optimizer_over_the_same_scorer_is_refused(workload, discipline):
    _play(workload, discipline, [steps(0, 3), second_optimizer, steps(3, 6)])
