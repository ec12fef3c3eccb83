"""GPU tier of the MLP scorer's route table (run with `-m gpu` on an MI355X): every public caller, on every case of
tests/test_mlp_routes_host.py::CASES, reaches the ``ltr_mlp_*`` entry points (or the torch layers, or the exception)
that the same caller reached at commit e6eba4d, before the routes were folded into ``fused._mlp_route``.  Public
modules and functions only: the file runs unchanged at that commit, where EXPECTED was recorded."""
import pytest
import torch

from tests.test_mlp_routes_host import CALLERS, CASES, EXPECTED

pytestmark = pytest.mark.gpu

ENTRY_POINTS = ("ltr_mlp_pairwise_f32", "ltr_mlp_listwise_f32", "ltr_mlp_scores_f32",
                "ltr_mlp_rows_scores_f32", "ltr_mlp_rows_grad_f32", "ltr_mlp_wide_scores_f32", "ltr_mlp_wide_grad_f32",
                "ltr_mlp_bf16_scores", "ltr_mlp_bf16_grad")


def _spy(monkeypatch, called):
    from pytorchltr_amd import _C
    lib = _C.lib()
    for name in ENTRY_POINTS:
        def wrapper(*args, _fn=getattr(lib, name), _name=name):
            called.append(_name)
            return _fn(*args)
        monkeypatch.setattr(lib, name, wrapper)


def observe(monkeypatch, case):
    """caller -> what it did on `case`: entry points in call order, "torch" for the layers, "raises <class>"."""
    from pytorchltr_amd import fused
    assert torch.cuda.is_available(), "GPU tier needs a ROCm device"
    dev = torch.device("cuda:0")
    called = []
    _spy(monkeypatch, called)
    F, L = case["F"], case["L"]
    torch.manual_seed(0)
    X = torch.randn(2, L, F, device=dev).to(getattr(torch, case["dtype"]))
    if case["xgrad"]:
        X.requires_grad_()
    y = torch.randint(0, 3, (2, L), device=dev)
    n = torch.tensor([L, L // 2 + 1], device=dev)

    def backward(out):
        if out.requires_grad:
            out.float().sum().backward()

    def run(module, fn, grad):
        del called[:]
        hook = module.l1.register_forward_hook(lambda *a: called.append("torch"))
        try:
            with torch.set_grad_enabled(grad), torch.autocast("cuda", enabled=case["autocast"]):
                fn()
            torch.cuda.synchronize()
        except (ValueError, RuntimeError, TypeError) as e:
            assert "HIP" not in str(e) and "illegal memory" not in str(e), e        # a device fault is no route
            called.append("raises " + type(e).__name__)
        finally:
            hook.remove()
        return list(called)

    got = {}
    for caller, (kind, grad, loss) in CALLERS.items():
        if kind == "scorer":
            m = fused.MLPScorer(F, case["hidden"]).to(dev)
            got[caller] = run(m, lambda: backward(m(X, n)), grad)
        elif kind == "score":
            m = fused.FusedMLPLoss(F, "hinge", hidden=case["hidden"]).to(dev)
            got[caller] = run(m, lambda: backward(m.score(X, n)), grad)
        elif kind == "loss":
            cls = fused.FusedMLPLoss if loss == "hinge" else fused.FusedMLPListwiseLoss
            m = cls(F, loss, hidden=case["hidden"]).to(dev)
            got[caller] = run(m, lambda: m(X, y, n).backward(), grad)
        else:
            m = fused.MLPScorer(F, case["hidden"]).to(dev)
            params = [p.detach() for p in m.parameters()]
            fn = (lambda: fused.mlp_loss_step(X, params, y, n, loss=loss)) if kind == "step" \
                else (lambda: fused.mlp_scores(X, params, n))
            got[caller] = run(m, fn, grad)
    return got


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_caller_takes_the_recorded_route(monkeypatch, name):
    got = observe(monkeypatch, CASES[name])
    for caller in CALLERS:
        print(name, caller, got[caller])
    assert got == EXPECTED[name]
