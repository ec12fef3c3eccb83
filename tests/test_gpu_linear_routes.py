"""GPU tier of the Linear scorer's route table (run with `-m gpu` on an MI355X): every public caller, on every case of
tests/test_linear_routes_host.py::CASES, reaches the entry points (or ``torch.nn.functional.linear``, or the exception)
that the same caller reached at commit e49dee3, before the routes were folded into ``fused._linear_route``.  Public
modules and functions only: the file runs unchanged at that commit, where EXPECTED and ANSWERS were recorded."""
import pytest
import torch

from tests.test_linear_routes_host import ANSWERS, CALLERS, CASES, EXPECTED, LOSSES, f4, rows_in_memory

pytestmark = pytest.mark.gpu

ENTRY_POINTS = ("ltr_linear_partials_f32", "ltr_linear_partials_bf16", "ltr_linear_listwise_partials_f32",
                "ltr_linear_reduce_f32", "ltr_linear_reduce_bcast_f32", "ltr_linear_reduce_loss_f32",
                "ltr_linear_scores_f32", "ltr_linear_scores_bf16", "ltr_linear_grad_f32", "ltr_linear_grad_bf16",
                "ltr_linear_sgd_lazy_step_dp_f32", "ltr_linear_sgd_flush_dp_f32", "ltr_linear_lazy_rows_reduce_f32",
                "ltr_pairwise_loss_f32", "ltr_pairwise_loss_ws_f32", "ltr_pairwise_loss_long_f32",
                "ltr_listwise_softmax_f32", "ltr_listmle_f32")


def _spy(monkeypatch, called):
    from pytorchltr_amd import _C
    lib = _C.lib()
    for name in ENTRY_POINTS:
        def wrapper(*args, _fn=getattr(lib, name), _name=name):
            called.append(_name)
            return _fn(*args)
        monkeypatch.setattr(lib, name, wrapper)
    # (looked up as torch.nn.functional.linear at every call: what LinearScorer falls back to)
    monkeypatch.setattr(torch.nn.functional, "linear",
                        lambda *a, _fn=torch.nn.functional.linear, **kw: (called.append("torch"), _fn(*a, **kw))[1])


def _loss_module(name, long_lists=False):
    from pytorchltr_amd import loss as L
    if name == "listnet":
        return L.ListwiseSoftmaxLoss()
    if name == "listmle":
        return L.ListMLELoss()
    cls = {"hinge": L.PairwiseHingeLoss, "logistic": L.PairwiseLogisticLoss, "ndcg2": L.LambdaNDCGLoss2}[name]
    return cls(long_lists=True) if long_lists else cls()


def batch(case, dev):
    """(xs, y, n) of a case: B lists of L documents, n = [L, L // 2 + 1, ...]."""
    from pytorchltr_amd.datasets.ragged import RaggedQueries
    B, L, F = case["B"], case["L"], case["F"]
    dtype = getattr(torch, case["dtype"])
    g = torch.Generator().manual_seed(0)
    n = torch.tensor([L if b % 2 == 0 else L // 2 + 1 for b in range(B)], dtype=torch.int64)
    y = torch.randint(0, 3, (B, L), generator=g)
    view = case["view"]
    if view == "ragged":                         # what the collate of this package makes: a marked view of zero-padded rows
        counts = n.tolist()
        off = torch.tensor([0] + counts).cumsum(0)
        rq = RaggedQueries(torch.randn(sum(counts), F, generator=g), torch.randint(0, 3, (sum(counts),), generator=g), off,
                           device=dev, pad_features_to=8 if dtype is torch.bfloat16 else 4, feature_dtype=dtype)
        b = rq.collate(list(range(B)))
        assert b.features.shape == (B, L, F) and not b.features.is_contiguous() and b.features._ltr_zero_padded_rows
        return b.features, b.relevance, b.n
    x = torch.randn(B, L, F, generator=g)
    if view == "strided":                        # a user's view with the same strides and no mark
        xs = torch.zeros(B, L, f4(F)).to(dev)[:, :, :F]
        xs.copy_(x)
        assert not xs.is_contiguous()
    elif view == "offset":                       # contiguous, one element into its storage: not 16-byte aligned
        flat = torch.zeros(B * L * F + 1, dtype=dtype, device=dev)
        xs = flat[1:].view(B, L, F)
        xs.copy_(x)
        assert xs.is_contiguous() and xs.data_ptr() % 16 != 0
    else:
        xs = x.to(dtype)
        if not case["cpu"]:
            xs = xs.to(dev)
    if case["xgrad"]:
        xs.requires_grad_()
    if not case["cpu"]:
        y, n = y.to(dev), n.to(dev)
    return xs, y, n


def observe(monkeypatch, case):
    """caller -> what it did on `case`: entry points in call order, "torch" for F.linear, "raises <class>"."""
    from pytorchltr_amd import fused
    from pytorchltr_amd.optim import SGD
    assert torch.cuda.is_available(), "GPU tier needs a ROCm device"
    dev = torch.device("cuda:0")
    called = []
    _spy(monkeypatch, called)
    xs, y, n = batch(case, dev)
    F = case["F"] + (1 if case["wrong_weight"] else 0)          # the parameters' feature count
    bias = case["bias"]

    def run(fn):
        del called[:]
        try:
            with torch.autocast("cuda", enabled=case["autocast"]):
                fn()
            torch.cuda.synchronize()
        except (ValueError, RuntimeError, TypeError) as e:
            # a device fault is no route (the runtime's "HIP error: ..."; this library's own errors speak of "HIP kernels")
            assert "HIP error" not in str(e) and "illegal memory" not in str(e), e
            called.append("raises " + type(e).__name__)
        return list(called)

    def backward(out):
        if out.requires_grad:
            out.mean().backward()

    def module(loss, long_lists=False, return_scores=False):
        m = fused.FusedLinearLoss(F, _loss_module(loss, long_lists), bias=bias).to(dev)
        if return_scores:
            return lambda: backward(m(xs, y, n, return_scores=True)[0])
        return lambda: backward(m(xs, y, n))

    def scorer(loss, lazy=True, long_lists=False):
        m = fused.LinearScorer(F, bias=bias, lazy=lazy).to(dev)
        loss_fn = _loss_module(loss, long_lists)
        return lambda: backward(loss_fn(m(xs, n), y, n))

    def nograd():
        m = fused.LinearScorer(F, bias=bias).to(dev)
        with torch.no_grad():
            m(xs, n)

    def step(loss, long_lists=False):
        m = fused.LinearScorer(F, bias=bias).to(dev)
        W, b = m.weight.detach().reshape(-1), None if m.bias is None else m.bias.detach()
        return lambda: fused.linear_loss_step(xs, W, b, y, n, loss=_loss_module(loss, long_lists))

    def lazysgd():
        m = fused.LinearScorer(F, bias=bias).to(dev)
        opt = fused.LazySGD(m.weight.detach().reshape(-1), None if m.bias is None else m.bias.detach(), 0.01, loss="hinge")
        opt.step(xs, y, n)
        opt.step(xs, y, n)
        opt.flush()

    def loop():
        model = fused.use_linear_scorer(torch.nn.Linear(F, 1, bias=bias).to(dev))
        opt = SGD(model.parameters(), lr=0.01)
        loss_fn = _loss_module("hinge")
        for _ in range(2):
            loss = loss_fn(model(xs), y, n).mean()
            opt.zero_grad()
            loss.backward()
            opt.step()
        if hasattr(opt, "flush"):
            opt.flush()

    got = {}
    for caller, (kind, loss) in CALLERS.items():
        if kind == "module":
            fn = module(loss, return_scores=caller.endswith("+scores"))
        elif kind == "lazy":
            fn = scorer(loss)
        elif kind == "eager":
            fn = scorer(loss, lazy=False)
        elif kind == "step":
            fn = step(loss)
        elif kind in ("module-long", "lazy-long", "step-long"):
            fn = {"module-long": module, "lazy-long": scorer, "step-long": step}[kind](loss, long_lists=True)
        else:
            fn = {"nograd": nograd, "lazysgd": lazysgd, "loop": loop}[kind]
        got[caller] = run(fn)
    return got


def answers(case):
    """What the library answers on this device where `fused._linear_route` takes the answer as a plain value."""
    from pytorchltr_amd import _C
    lib = _C.lib()
    B, L, F = case["B"], case["L"], case["F"]
    codes = {"hinge": _C.HINGE, "logistic": _C.LOGISTIC, "ndcg2": _C.NDCG2}
    return {"cus": torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count,
            "fused_plan": {k: [int(lib.ltr_linear_fused_plan(codes[k], B, L, F)),
                               int(lib.ltr_linear_fused_plan(codes[k], B, L, f4(F)))] for k in LOSSES if k in codes},
            "listwise_plan": {k: int(lib.ltr_linear_listwise_plan(code, B, L, rows_in_memory(case)))
                              for k, code in (("listnet", _C.LISTWISE_LISTNET), ("listmle", _C.LISTWISE_LISTMLE))}}


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_caller_takes_the_recorded_route(monkeypatch, name):
    from pytorchltr_amd import _C
    assert answers(CASES[name]) == ANSWERS[name]            # still the library's: the host tier feeds them to the route
    got = observe(monkeypatch, CASES[name])
    for caller in CALLERS:
        print(name, caller, got[caller])
    assert got == EXPECTED[name]


def test_the_cases_lie_where_their_names_say():
    """The device and the library put the cases on the sides of the limits they were chosen for."""
    from pytorchltr_amd import _C
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    assert 2 * 2 <= cus < 2 * 160                           # B = 2: a few lists; B = 160: past the few-lists rule
    assert 160 <= cus                                       # ... and inside the heavy-pairs rule (B <= CUs, L > 768)
    assert ANSWERS["cluster"]["fused_plan"]["logistic"][0] == _C.PLAN_CLUSTER
    assert ANSWERS["parts"]["fused_plan"]["ndcg2"][0] == _C.PLAN_PARTS
    assert ANSWERS["B80-L500-F512"]["fused_plan"]["logistic"][0] == _C.PLAN_CLUSTER
    assert ANSWERS["B80-L500-F512"]["fused_plan"]["ndcg2"][0] not in (_C.PLAN_CLUSTER, _C.PLAN_PARTS)
    assert CASES["long"]["L"] == CASES["bf16-long"]["L"] == _C.max_list_len() + 4
    assert ANSWERS["F5"]["listwise_plan"] == {"listnet": 0, "listmle": 0}     # rows that are no whole float4
    assert ANSWERS["base"]["listwise_plan"] == {"listnet": 1, "listmle": 1}
