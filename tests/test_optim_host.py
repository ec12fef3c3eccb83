"""CPU tier of the optimizer-protocol parity (tests/test_gpu_optim_protocol.py is the GPU tier): the host rules of
pytorchltr_amd.optim that need no device, on small stubs.

  - a _LazyParameter applies its pending update before ANY torch function that could show its values, wherever the parameter
    sits in the call (positional, keyword, nested containers), and before none of the metadata questions in _PARAM_NO_FLUSH;
  - a LazyGrad's clone is a copy at the function level and at the dispatch level, its detach / alias stay aliases;
  - pickle, torch.save and copy.deepcopy of a _LazyParameter apply the update and give a plain nn.Parameter without lazy state;
    a copied or unpickled LinearScorer pairs its new parameters up again;
  - optim.SGD on CPU parameters adopts nothing and is torch.optim.SGD bit for bit through deepcopy, pickle and load_state_dict;
  - after load_state_dict the per-scorer state answers from the optimizer's CURRENT group (lr, plain SGD or not), and an update
    that was pending is applied before the groups change.
"""
import copy
import io
import pickle
import weakref

import pytest
import torch
import torch.nn.functional as F_

from pytorchltr_amd import optim as O_


class _StubState:
    """Stands for optim._LazyLinear behind a parameter: counts the updates it applied; an update adds 1 to the values."""

    def __init__(self, *params):
        self.params = params
        self.owner = weakref.ref(params[0])          # (the real state holds weak references: what pickle chokes on)
        self.flushes = 0
        self.pending = None
        for p in params:
            p.__class__ = O_._LazyParameter
            p._ltr_lazy = self

    def arm(self):
        self.pending = object()
        return self

    def flush(self):
        if self.pending is None:
            return
        self.pending = None
        self.flushes += 1
        with torch._C.DisableTorchFunctionSubclass(), torch.no_grad():
            for p in self.params:
                p.data.add_(1.0)


def _scorer_params(F=6, seed=0):
    g = torch.Generator().manual_seed(seed)
    w = torch.nn.Parameter(torch.randn(1, F, generator=g))
    b = torch.nn.Parameter(torch.randn(1, generator=g))
    w._ltr_scorer_bias = b
    return w, b


def _nested_sum(groups):
    """A torch-function-aware library function whose argument nests tensors two levels deep (a tuple inside a list)."""
    flat = [t for g in groups for t in g]
    if torch.overrides.has_torch_function(flat):
        return torch.overrides.handle_torch_function(_nested_sum, flat, groups)
    return torch.stack([t.sum() for t in flat]).sum()


_READS = {
    "positional": lambda x, w, b: F_.linear(x, w, b),
    "keyword": lambda x, w, b: F_.linear(x, weight=w, bias=b),
    "all keywords": lambda x, w, b: F_.linear(input=x, weight=w, bias=b),
    "keyword other": lambda x, w, b: torch.mul(x, other=w),
    "list": lambda x, w, b: torch.cat([w, w]),
    "keyword list": lambda x, w, b: torch.cat(tensors=[w, w]),
    "keyword tuple": lambda x, w, b: torch.cat(tensors=(w, w)),
    "tuple in a list": lambda x, w, b: _nested_sum([(x, w)]),
    "tuple in a list by keyword": lambda x, w, b: _nested_sum(groups=[(x, w)]),
    "dict in a tuple": lambda x, w, b: O_._LazyParameter.__torch_function__(
        lambda a: a[0]["w"] * 1.0, (O_._LazyParameter,), (({"w": w},),)),
    "parameters_to_vector": lambda x, w, b: torch.nn.utils.parameters_to_vector([w, b]),
    "method": lambda x, w, b: w.sum(),
    "out=": lambda x, w, b: torch.mul(x, 2.0, out=w),
}


@pytest.mark.parametrize("how", sorted(_READS))
def test_every_read_applies_the_pending_update_first(how):
    w, b = _scorer_params()
    st = _StubState(w, b)
    with torch._C.DisableTorchFunctionSubclass():
        w0, b0 = w.detach().clone(), b.detach().clone()
    x = torch.ones(1, 6) if how == "out=" else torch.randn(3, 6, generator=torch.Generator().manual_seed(1))
    st.arm()
    with torch.no_grad():
        got = _READS[how](x, w, b)
    assert st.flushes == 1 and st.pending is None, how
    # ... and what was read is the updated value
    if how != "out=":
        plain_w, plain_b = torch.nn.Parameter(w0 + 1.0), torch.nn.Parameter(b0 + 1.0)
        with torch.no_grad():
            want = _READS[how](x, plain_w, plain_b) if how != "dict in a tuple" else plain_w * 1.0
        assert torch.equal(got, want), how
    # nothing pending: nothing to apply
    with torch.no_grad():
        _READS[how](x, w, b)
    assert st.flushes == 1, how


def test_no_metadata_question_applies_the_update():
    w, b = _scorer_params()
    st = _StubState(w, b)
    extra = {torch.Tensor.requires_grad.__set__: (True,), torch.Tensor.grad.__set__: (None,),
             torch.Tensor.register_hook: (lambda g: g,)}
    assert len(O_._PARAM_NO_FLUSH) >= 30
    for func in O_._PARAM_NO_FLUSH:
        st.arm()
        O_._LazyParameter.__torch_function__(func, (O_._LazyParameter,), (w,) + extra.get(func, ()), {})
        assert st.flushes == 0 and st.pending is not None, func
    # the same through the attribute syntax a training loop uses
    st.arm()
    w.grad = torch.zeros(1, 6)
    assert w.shape == (1, 6) and w.dtype is torch.float32 and w.requires_grad and w.is_leaf and w.grad is not None
    assert w.numel() == 6 and w.dim() == 2 and w.is_contiguous() and not w.is_cuda and hash(w) == id(w)
    w.grad = None
    w.requires_grad_(False)
    w.requires_grad_(True)
    assert st.flushes == 0 and st.pending is not None


class _StubPendingGrad:
    """Stands for optim._PendingGrad: the values appear when somebody asks."""

    def __init__(self, F=6):
        self.real = None
        self.asked = 0
        g = torch.Generator().manual_seed(5)
        self.values = {"w": torch.randn(1, F, generator=g), "b": torch.randn(1, generator=g)}

    def materialize(self):
        if self.real is None:
            self.asked += 1
            self.real = {k: v.clone() for k, v in self.values.items()}
        return self.real


def _lazy_grad(which="w"):
    pg = _StubPendingGrad()
    return pg, O_.LazyGrad(pg, which, pg.values[which].shape, torch.device("cpu"))


def _below_the_python_api(op, g):
    """The op as autograd's C++ calls it: no __torch_function__, straight to __torch_dispatch__."""
    with torch._C.DisableTorchFunctionSubclass():
        return op(g)


@pytest.mark.parametrize("level", ["function", "dispatch"])
@pytest.mark.parametrize("materialised_first", [False, True])
def test_clone_of_a_lazy_gradient_is_a_copy(level, materialised_first):
    pg, g = _lazy_grad()
    if materialised_first:
        g.materialize()
    c = g.clone() if level == "function" else _below_the_python_api(torch.ops.aten.clone.default, g)
    assert not isinstance(c, O_.LazyGrad) and torch.equal(c, pg.values["w"])
    g.mul_(0.5)                                      # what clip_grad_norm_ / GradScaler.unscale_ do to `.grad`
    assert torch.equal(c, pg.values["w"])
    assert torch.equal(g.materialize(), pg.values["w"] * 0.5)
    c.add_(1.0)
    assert torch.equal(g.materialize(), pg.values["w"] * 0.5)


@pytest.mark.parametrize("op", ["aten.detach", "aten.alias", "Tensor.detach"])
def test_detach_and_alias_of_a_lazy_gradient_stay_aliases(op):
    pg, g = _lazy_grad()
    if op == "Tensor.detach":
        a = g.detach()
    else:
        a = _below_the_python_api(getattr(torch.ops.aten, op.split(".")[1]).default, g)
        assert isinstance(a, O_.LazyGrad) and pg.asked == 0          # (what autograd does when it stores `.grad`: no launch)
        assert a.shape == g.shape and a.dtype is torch.float32
    g.mul_(0.5)
    assert pg.asked == 1
    assert torch.equal(a + 0.0, pg.values["w"] * 0.5)
    a.mul_(4.0)
    assert torch.equal(g + 0.0, pg.values["w"] * 2.0)


def _copies():
    def by_pickle(obj):
        return pickle.loads(pickle.dumps(obj))

    def by_torch_save(obj):
        buf = io.BytesIO()
        torch.save(obj, buf)
        buf.seek(0)
        return torch.load(buf, weights_only=False)
    return {"pickle": by_pickle, "torch.save": by_torch_save, "deepcopy": copy.deepcopy}


@pytest.mark.parametrize("how", ["pickle", "torch.save", "deepcopy"])
def test_a_lazy_parameter_serialises_as_a_plain_updated_parameter(how):
    w, b = _scorer_params()
    st = _StubState(w, b)
    with torch._C.DisableTorchFunctionSubclass():
        w0, b0 = w.detach().clone(), b.detach().clone()
    b.requires_grad_(False)
    st.arm()
    w2, b2 = _copies()[how]((w, b))
    assert st.flushes == 1 and st.pending is None
    for q, want, rg in ((w2, w0 + 1.0, True), (b2, b0 + 1.0, False)):
        assert type(q) is torch.nn.Parameter and q.requires_grad is rg
        assert not [k for k in q.__dict__ if k.startswith("_ltr_")]
        assert torch.equal(q.detach(), want)
    # a copy, not an alias: the original moves on alone, and is still what it was
    assert isinstance(w, O_._LazyParameter) and w._ltr_lazy is st and w._ltr_scorer_bias is b
    st.arm()
    assert torch.equal(w.detach(), w0 + 2.0) and torch.equal(w2.detach(), w0 + 1.0)
    # loadable where only weights are allowed
    buf = io.BytesIO()
    torch.save({"weight": w2, "lazy": w}, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=True)
    assert type(back["lazy"]) is torch.nn.Parameter and torch.equal(back["lazy"].detach(), w0 + 2.0)


@pytest.mark.parametrize("how", ["pickle", "torch.save", "deepcopy"])
def test_a_copied_scorer_pairs_its_parameters_up_again(how):
    from pytorchltr_amd.fused import LinearScorer, use_linear_scorer
    model = torch.nn.Sequential(torch.nn.Identity(), use_linear_scorer(torch.nn.Linear(6, 1)))
    st = _StubState(model[1].weight, model[1].bias).arm()
    twin = _copies()[how](model)
    assert st.flushes == 1
    sc = twin[1]
    assert isinstance(sc, LinearScorer) and type(sc.weight) is torch.nn.Parameter and type(sc.bias) is torch.nn.Parameter
    assert sc.weight._ltr_scorer_bias is sc.bias and not hasattr(sc.weight, "_ltr_lazy")
    assert torch.equal(sc.weight.detach(), model[1].weight.detach()) and sc.weight.data_ptr() != model[1].weight.data_ptr()
    no_bias = _copies()[how](LinearScorer(6, bias=False))
    assert no_bias.bias is None and not hasattr(no_bias.weight, "_ltr_scorer_bias")


def _cpu_training(cls, events):
    from pytorchltr_amd.fused import use_linear_scorer
    torch.manual_seed(11)
    model = use_linear_scorer(torch.nn.Linear(5, 1))
    opt = cls(model.parameters(), lr=0.1, momentum=0.9)
    g = torch.Generator().manual_seed(12)
    trace = []
    for ev in events:
        if ev == "step":
            x, y = torch.randn(7, 5, generator=g), torch.randn(7, 1, generator=g)
            opt.zero_grad()
            F_.mse_loss(model(x), y).backward()
            opt.step()
        elif ev == "deepcopy":
            model, opt = copy.deepcopy((model, opt))
        elif ev == "pickle":
            model, opt = pickle.loads(pickle.dumps((model, opt)))
        elif ev == "load":
            other = torch.optim.SGD([torch.nn.Parameter(p.detach().clone()) for p in model.parameters()], lr=0.01,
                                    momentum=0.5, weight_decay=0.1)
            sd = other.state_dict()
            sd["state"] = copy.deepcopy(opt.state_dict()["state"])
            opt.load_state_dict(sd)
        trace.append(torch.cat([p.detach().reshape(-1).clone() for p in model.parameters()]))
    return model, opt, torch.stack(trace)


def test_on_cpu_parameters_it_is_torch_sgd_through_deepcopy_pickle_and_load():
    events = ["step", "step", "deepcopy", "step", "pickle", "step", "step", "load", "step", "step"]
    m_ref, o_ref, t_ref = _cpu_training(torch.optim.SGD, events)
    m, o, t = _cpu_training(O_.SGD, events)
    assert type(o) is O_.SGD and o._lazy == []                       # CPU parameters: nothing to adopt
    assert type(m.weight) is torch.nn.Parameter
    assert torch.equal(t, t_ref)
    assert len({tuple(r.tolist()) for r in t}) == 7                  # (every step moved the weights)
    o.flush()
    sd, sd_ref = o.state_dict(), o_ref.state_dict()
    assert sd["param_groups"] == sd_ref["param_groups"] and sd["param_groups"][0]["lr"] == 0.01
    for k in sd_ref["state"]:
        assert torch.equal(sd["state"][k]["momentum_buffer"], sd_ref["state"][k]["momentum_buffer"])


def test_the_scorer_state_follows_the_optimizers_current_group():
    w, b = _scorer_params()
    x = torch.nn.Parameter(torch.zeros(3))
    opt = O_.SGD([{"params": [x], "lr": 0.3}, {"params": [w, b]}], lr=0.1)
    assert opt._lazy == []
    st = O_._LazyLinear(w, b, opt.param_groups[1])                    # (what _adopt() builds for device parameters)
    opt._lazy.append(st)
    assert st.plain_sgd() and st.group["lr"] == 0.1
    # an update is pending when the state is loaded: it is applied first, while the old group still stands
    old_group, seen = opt.param_groups[1], []
    st.pending = object()

    def flush():
        if st.pending is not None:
            seen.append(st.group is old_group and opt.param_groups[1] is old_group)
            st.pending = None
    st.flush = flush
    other = torch.optim.SGD([{"params": [torch.nn.Parameter(torch.zeros(3))], "lr": 0.2},
                             {"params": [torch.nn.Parameter(torch.zeros(1, 6)), torch.nn.Parameter(torch.zeros(1))],
                              "lr": 0.01, "momentum": 0.9}], lr=0.5)
    opt.load_state_dict(other.state_dict())
    assert seen == [True]
    assert opt.param_groups[1] is not old_group                      # (torch replaces the dicts: what the state must follow)
    assert st.group is opt.param_groups[1] and st.group["lr"] == 0.01 and not st.plain_sgd()
    # a scheduler attached after the load, and plain assignment, reach the scorer's state
    opt.param_groups[1]["momentum"] = 0
    assert st.plain_sgd()
    sched = torch.optim.lr_scheduler.StepLR(opt, 1, gamma=0.5)
    opt.step()
    sched.step()
    assert st.group["lr"] == pytest.approx(0.005) and opt.param_groups[0]["lr"] == pytest.approx(0.1)
    for g in opt.param_groups:
        g["lr"] *= 0.1
    assert st.group["lr"] == pytest.approx(0.0005)
    # in-place __setstate__ (what load_state_dict ends in) with the groups swapped
    sd = opt.state_dict()
    sd["param_groups"][1]["lr"] = 0.7
    opt.load_state_dict(sd)
    assert st.group is opt.param_groups[1] and st.group["lr"] == 0.7
