"""CPU tier of the MLP trainer (include/ltr_mlp_train.h: ltr_mlp_train_state_floats, ltr_mlp_train_step_f32,
ltr_mlp_apply_update_f32; pytorchltr_amd.fused.MLPTrainer): the C ABI's table, the host-side return codes, the
reference rules of tests/mlp_train_ref.py against torch.optim in float64, the state_dict conversion against real
torch.optim optimizers, the constructor's refusals and the new kernels' register use.  The library is built, nothing
is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import mlp_train_ref as ref

NEW = ("ltr_mlp_train_state_floats", "ltr_mlp_train_step_f32", "ltr_mlp_apply_update_f32")


@pytest.fixture(scope="module")
def lib():
    from pytorchltr_amd import _C
    from pytorchltr_amd.build import build_extension
    if not os.environ.get("LTR_HIP_LIB"):
        build_extension()
    return _C.lib()


def _root():
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(_root(), "include", "ltr_mlp_train.h")).read()


# ---- the ABI table ----
def test_header_table_and_exports(lib):
    from pytorchltr_amd import _C, build
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(ltr_[a-z0-9_]+)\s*\(", text))
    assert declared == set(_C.MLP_TRAIN_SIGNATURES) == set(NEW)
    others = [v for k, v in vars(_C).items() if k.endswith("SIGNATURES") and k != "MLP_TRAIN_SIGNATURES"]
    assert len(others) >= 11
    for name in NEW:
        assert not any(name in table for table in others), name
        fn = getattr(lib, name)
        assert isinstance(fn, ctypes._CFuncPtr), name
        restype, argtypes = _C.MLP_TRAIN_SIGNATURES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(proto.split(",")) == len(argtypes), name
    assert lib.ltr_version() == 114                                      # (ltr_hip.h and its version stay)
    assert os.path.join(_root(), "include", "ltr_mlp_train.h") in build.DEPENDS
    # the struct as the header declares it: two ints, then eight doubles in this order
    fields = re.search(r"struct ltr_mlp_optim \{(.*?)\};", text, flags=re.S).group(1)
    names = re.findall(r"\b(?:int|double)\s+(\w+);", fields)
    assert names == [f[0] for f in _C.MLPOptim._fields_]
    assert [f[1] for f in _C.MLPOptim._fields_] == [ctypes.c_int] * 2 + [ctypes.c_double] * 8
    for macro, value in (("LTR_OPT_SGD", _C.OPT_SGD), ("LTR_OPT_ADAGRAD", _C.OPT_ADAGRAD), ("LTR_OPT_ADAM", _C.OPT_ADAM),
                         ("LTR_MLP_TRAIN_PAIRWISE", _C.MLP_TRAIN_PAIRWISE), ("LTR_MLP_TRAIN_LISTWISE", _C.MLP_TRAIN_LISTWISE),
                         ("LTR_MLP_TRAIN_LAMBDARANK", _C.MLP_TRAIN_LAMBDARANK)):
        assert int(re.search(r"#define %s (\d+)" % macro, text).group(1)) == value


def test_state_floats(lib):
    count = lib.ltr_mlp_train_state_floats
    for F, H1, H2 in ((8, 5, 3), (136, 50, 10), (452, 50, 10), (4, 1, 1)):
        P = lib.ltr_mlp_param_count(F, H1, H2)
        assert P == H1 * F + H1 + H2 * H1 + H2 + H2 + 1
        for algo, nbuf in ((0, 1), (1, 1), (2, 2)):
            want = (nbuf * P + 3) // 4 * 4 + 4              # the buffers, then the 16-byte aligned header of four words
            assert count(algo, F, H1, H2) == want and want % 4 == 0
    for bad in ((3, 8, 5, 3), (-1, 8, 5, 3), (0, 0, 5, 3), (0, 8, 0, 3), (0, 8, 5, -1)):
        assert count(*bad) == 0, bad


# ---- return codes (no case gets as far as a launch) ----
P = 256                                        # dummy non-NULL, 16-byte aligned device pointer: never dereferenced
_ARGS = ["family", "code", "k", "sigma", "X", "W1", "b1", "W2", "b2", "W3", "b3", "w1_pitch", "W1_rows", "rel", "rel_dtype",
         "n", "tie", "use_seed", "seed", "seed_dev", "grad_out", "B", "L", "F", "H1", "H2", "loss", "scores_out", "loss_sum",
         "state", "optim", "grads_out", "workspace", "workspace_bytes", "stream"]
_VALID = dict(family=0, code=0, k=0, sigma=1.0, X=P, W1=P, b1=P, W2=P, b2=P, W3=P, b3=P, w1_pitch=8, W1_rows=None, rel=P,
              rel_dtype=0, n=P, tie=None, use_seed=0, seed=0, seed_dev=None, grad_out=None, B=2, L=16, F=8, H1=5, H2=3,
              loss=P, scores_out=None, loss_sum=None, state=P, optim="adagrad", grads_out=None, workspace=P,
              workspace_bytes=1 << 30, stream=None)
KIND, SHAPE, TOO_LONG, NULL, WORKSPACE = -3, -2, -4, -1, -5
INF, NAN = float("inf"), float("nan")


def _optim(algo="adagrad", **over):
    from pytorchltr_amd import _C
    o = _C.MLPOptim(algo={"sgd": 0, "adagrad": 1, "adam": 2}.get(algo, algo), nesterov=0, lr=0.1, weight_decay=0.0,
                    momentum=0.0, dampening=0.0, lr_decay=0.0, eps=1e-10, beta1=0.9, beta2=0.999)
    for k, v in over.items():
        setattr(o, k, v)
    return o


_BAD_HYPER = [
    dict(lr=-0.1), dict(lr=NAN), dict(lr=INF), dict(weight_decay=-1.0), dict(weight_decay=NAN),
    dict(algo="sgd", momentum=-0.5), dict(algo="sgd", momentum=INF), dict(algo="sgd", dampening=NAN),
    dict(algo="sgd", nesterov=1), dict(algo="sgd", nesterov=1, momentum=0.9, dampening=0.1),
    dict(algo="adagrad", eps=-1.0), dict(algo="adagrad", lr_decay=-0.1), dict(algo="adagrad", lr_decay=NAN),
    dict(algo="adam", beta1=1.0), dict(algo="adam", beta1=-0.1), dict(algo="adam", beta2=1.0), dict(algo="adam", beta2=NAN),
    dict(algo="adam", eps=-1e-8),
]

CASES = [
    (dict(optim=None), NULL),
    (dict(family=3), KIND), (dict(family=-1), KIND), (dict(code=7), KIND), (dict(family=1, code=2), KIND),
    (dict(rel_dtype=3), KIND), (dict(optim=_optim(3)), KIND), (dict(optim=_optim(-1)), KIND),
    (dict(B=-1), SHAPE), (dict(L=0), SHAPE), (dict(F=6, w1_pitch=6), SHAPE), (dict(F=228), SHAPE), (dict(H1=65), SHAPE),
    (dict(H2=17), SHAPE), (dict(w1_pitch=0), SHAPE), (dict(w1_pitch=9), SHAPE), (dict(family=2, sigma=NAN), SHAPE),
] + [(dict(optim=_optim(**h)), SHAPE) for h in _BAD_HYPER] + [
    (dict(L=257), TOO_LONG), (dict(L=129, F=148, w1_pitch=148), TOO_LONG),
    (dict(B=0), 0), (dict(B=0, X=None, W1=None, state=None, workspace=None, workspace_bytes=0), 0),
    (dict(X=None), NULL), (dict(W1=None), NULL), (dict(b1=None), NULL), (dict(W2=None), NULL), (dict(b2=None), NULL),
    (dict(W3=None), NULL), (dict(b3=None), NULL), (dict(rel=None), NULL), (dict(n=None), NULL), (dict(loss=None), NULL),
    (dict(state=None), NULL), (dict(state=None, optim=_optim("adam")), NULL),
    (dict(state=None, optim=_optim("sgd", momentum=0.9)), NULL),
    (dict(w1_pitch=5), NULL),                                        # a narrower W1 needs its padded image
    (dict(workspace=None), WORKSPACE), (dict(workspace_bytes=16), WORKSPACE),
    (dict(state=None, optim=_optim("sgd"), workspace=None), WORKSPACE),          # SGD without momentum needs no state
    # two at once: the documented order
    (dict(family=3, B=-1), KIND), (dict(optim=_optim(3), L=300), KIND), (dict(B=-1, L=300), SHAPE),
    (dict(optim=_optim(lr=-1.0), L=300), SHAPE), (dict(L=300, X=None), TOO_LONG), (dict(L=300, B=0), TOO_LONG),
    (dict(X=None, workspace=None), NULL),
]


@pytest.mark.parametrize("i", range(len(CASES)))
def test_train_step_return_codes(lib, i):
    change, want = CASES[i]
    args = dict(_VALID, **change)
    if args["optim"] == "adagrad":
        args["optim"] = _optim()
    args["optim"] = None if args["optim"] is None else ctypes.byref(args["optim"])
    assert lib.ltr_mlp_train_step_f32(*[args[a] for a in _ARGS]) == want, change


def test_train_step_shape_rules_are_the_entry_points(lib):
    """The network, list and label rules answer as the family's existing entry point does."""
    for change in (dict(F=6), dict(F=228), dict(H1=65), dict(H2=17), dict(L=257), dict(L=129, F=148), dict(L=0), dict(B=-1),
                   dict(rel_dtype=5), dict(code=9)):
        a = dict(_VALID, **change)
        a["w1_pitch"] = a["F"]
        a["optim"] = ctypes.byref(_optim())
        pw = lib.ltr_mlp_pairwise_f32(a["code"], 1.0, P, P, P, P, P, P, P, P, a["rel_dtype"], P, None, a["B"], a["L"],
                                      a["F"], a["H1"], a["H2"], P, None, P, None, P, 1 << 30, None)
        assert pw == lib.ltr_mlp_train_step_f32(*[a[x] for x in _ARGS]) != 0, change


# One bad argument through all four entry points of the fused step.  The expected codes are the answers of the build
# before the four shared one launch path, as literals: (change, the pairwise entry point's code, the code of the listwise
# and the LambdaRank entry points).  One bad argument at a time: where two are wrong the orders differ (the pairwise entry
# point answers SHAPE and LIST_TOO_LONG ahead of KIND, the other three KIND first), which the tables above and those of
# test_mlp_listwise_host.py and test_mlp_lambdarank_host.py pin.  No legal shape makes ltr_mlp_listwise_plan or ltr_mlp_lambdarank_plan
# answer 0 at a list length ltr_mlp_max_list_len allows (every F <= 224 in steps of 4 was asked at L = 16, 64, 128, 129,
# 200, 256), so LTR_ERR_CONFIG has no case here: no argument reaches it.
SAME_BAD_ARGUMENT = [
    (dict(F=6), SHAPE, SHAPE), (dict(F=228), SHAPE, SHAPE), (dict(H1=65), SHAPE, SHAPE), (dict(H2=17), SHAPE, SHAPE),
    (dict(L=257), TOO_LONG, TOO_LONG), (dict(L=129, F=148), TOO_LONG, TOO_LONG),
    (dict(rel_dtype=3), KIND, KIND),
    (dict(workspace_bytes=16), WORKSPACE, WORKSPACE), (dict(workspace=None), WORKSPACE, WORKSPACE),
]


def _four_entry_points(lib, change):
    """{name: code} of the change on ltr_mlp_pairwise_f32, ltr_mlp_listwise_f32 (ListNet, ListMLE), ltr_mlp_lambdarank_f32
    and on ltr_mlp_train_step_f32 in each of the three families."""
    a = dict(_VALID, **change)
    a["w1_pitch"] = a["F"]
    a["optim"] = ctypes.byref(_optim())
    net = [a[x] for x in ("X", "W1", "b1", "W2", "b2", "W3", "b3")]
    dims = [a[x] for x in ("B", "L", "F", "H1", "H2")]
    tail = [a["loss"], None, P, None, a["workspace"], a["workspace_bytes"], None]      # loss, scores, grads, loss_sum, ...
    got = {"pairwise": lib.ltr_mlp_pairwise_f32(0, 1.0, *net, a["rel"], a["rel_dtype"], a["n"], None, *dims, *tail),
           "lambdarank": lib.ltr_mlp_lambdarank_f32(10, 1.0, *net, a["rel"], a["rel_dtype"], a["n"], None, *dims, *tail)}
    for name, code in (("listnet", 0), ("listmle", 1)):
        got[name] = lib.ltr_mlp_listwise_f32(code, 0, *net, a["rel"], a["rel_dtype"], a["n"], None, 0, 0, None, None,
                                             *dims, *tail)
    for name, family, code in (("train-pairwise", 0, 0), ("train-listnet", 1, 0), ("train-listmle", 1, 1),
                               ("train-lambdarank", 2, 0)):
        got[name] = lib.ltr_mlp_train_step_f32(*[dict(a, family=family, code=code, k=10)[x] for x in _ARGS])
    return got


@pytest.mark.parametrize("i", range(len(SAME_BAD_ARGUMENT)))
def test_one_bad_argument_through_all_four_entry_points(lib, i):
    change, pairwise, rows = SAME_BAD_ARGUMENT[i]
    got = _four_entry_points(lib, change)
    # the trainer's code for a family is that family's own entry point's
    assert got["train-pairwise"] == got["pairwise"] == pairwise, (change, got)
    assert got["train-listnet"] == got["listnet"] and got["train-listmle"] == got["listmle"], (change, got)
    assert got["train-lambdarank"] == got["lambdarank"], (change, got)
    # the three entry points that are not the pairwise one give one code
    assert {got[name] for name in got if "pairwise" not in name} == {rows}, (change, got)


_APPLY = ["grads", "W1", "b1", "W2", "b2", "W3", "b3", "w1_pitch", "state", "optim", "F", "H1", "H2", "stream"]
_APPLY_VALID = dict(grads=P, W1=P, b1=P, W2=P, b2=P, W3=P, b3=P, w1_pitch=8, state=P, optim="adagrad", F=8, H1=5, H2=3,
                    stream=None)
APPLY_CASES = [
    (dict(optim=None), NULL), (dict(optim=_optim(3)), KIND), (dict(optim=_optim(-2)), KIND),
    (dict(F=0), SHAPE), (dict(H1=0), SHAPE), (dict(H2=-1), SHAPE), (dict(w1_pitch=0), SHAPE), (dict(w1_pitch=9), SHAPE),
] + [(dict(optim=_optim(**h)), SHAPE) for h in _BAD_HYPER] + [
    (dict(grads=None), NULL), (dict(W1=None), NULL), (dict(b1=None), NULL), (dict(W2=None), NULL), (dict(b2=None), NULL),
    (dict(W3=None), NULL), (dict(b3=None), NULL), (dict(state=None), NULL), (dict(state=None, optim=_optim("adam")), NULL),
    (dict(optim=_optim(3), F=0), KIND), (dict(F=0, grads=None), SHAPE),
]


@pytest.mark.parametrize("i", range(len(APPLY_CASES)))
def test_apply_update_return_codes(lib, i):
    change, want = APPLY_CASES[i]
    args = dict(_APPLY_VALID, **change)
    if args["optim"] == "adagrad":
        args["optim"] = _optim()
    args["optim"] = None if args["optim"] is None else ctypes.byref(args["optim"])
    assert lib.ltr_mlp_apply_update_f32(*[args[a] for a in _APPLY]) == want, change


# ---- the reference rules are torch.optim's ----
CONFIGS = [
    ("sgd", dict(lr=0.05)),
    ("sgd", dict(lr=0.05, weight_decay=0.01)),
    ("sgd", dict(lr=0.05, momentum=0.9, dampening=0.3, weight_decay=0.02)),
    ("sgd", dict(lr=0.05, momentum=0.8, nesterov=True, weight_decay=0.01)),
    ("adagrad", dict(lr=0.1)),
    ("adagrad", dict(lr=0.1, lr_decay=0.05, weight_decay=0.01, initial_accumulator_value=0.5, eps=1e-6)),
    ("adam", dict(lr=0.01)),
    ("adam", dict(lr=0.01, betas=(0.7, 0.95), eps=1e-5, weight_decay=0.03)),
]
_TORCH = {"sgd": torch.optim.SGD, "adagrad": torch.optim.Adagrad, "adam": torch.optim.Adam}


def test_the_corner_grid_holds_the_earlier_configurations():
    grid = [(algo, hyper) for _, algo, hyper in ref.CORNERS]
    assert all(c in grid for c in CONFIGS) and len({name for name, _, _ in ref.CORNERS}) == len(grid) == 16


# (the eight earlier configurations keep their ids; the corners they do not hold follow under their own names)
_NEW_CORNERS = [c for c in ref.CORNERS if c[1:] not in CONFIGS]


@pytest.mark.parametrize("algo, hyper", CONFIGS + [c[1:] for c in _NEW_CORNERS],
                         ids=["%s-%d" % (a, i) for i, (a, _) in enumerate(CONFIGS)] + [c[0] for c in _NEW_CORNERS])
def test_reference_rules_are_torch_optims_in_float64(algo, hyper):
    gen = torch.Generator().manual_seed(7)
    p = torch.randn(6, 7, dtype=torch.float64, generator=gen).requires_grad_(True)
    opt = _TORCH[algo]([p], foreach=False, **hyper)
    mine, state = p.detach().numpy().copy(), ref.initial_state(algo, hyper, p.detach().numpy())
    for t in range(5):
        g = torch.randn(6, 7, dtype=torch.float64, generator=gen)
        p.grad = g.clone()
        opt.step()
        mine, new, bound = ref.step(algo, hyper, mine, g.numpy(), state, t)
        state.update(new)
        np.testing.assert_allclose(mine, p.detach().numpy(), rtol=1e-12, atol=0)
        for name, value in new.items():
            np.testing.assert_allclose(value, opt.state[p][name].numpy(), rtol=1e-12, atol=0)
            assert (bound[name] > 0).all()
        assert (bound["p"] > 0).all() and bound["p"].shape == mine.shape


def test_the_bound_counts_roundings_and_sees_cancellation():
    """Plain SGD: one scalar and two operations -> 3 u (|p| + lr |g|) + half an ulp; a weight decay that cancels the
    gradient leaves the magnitudes of what cancelled in the bound."""
    p, g = np.float32([1.0]), np.float32([0.5])
    _, _, b = ref.step("sgd", dict(lr=0.25), p, g, {}, 0)
    assert b["p"][0] == pytest.approx(3 * ref.U * (1.0 + 0.125) * (1 + 2.0 ** -10) + 0.5 * np.spacing(np.float32(0.875)))
    q, _, b = ref.step("sgd", dict(lr=0.25, weight_decay=0.5), p, np.float32([-0.5]), {}, 0)
    assert q[0] == 1.0 and b["p"][0] > 5 * ref.U * (1.0 + 0.25 * 1.0)


STEP_COUNTS = (0, 1, 7, 999, 10 ** 6)


@pytest.mark.parametrize("name", [c[0] for c in ref.CORNERS])
def test_an_fp32_evaluation_stays_within_the_bound_at_every_corner(name):
    """ref.step_f32 -- the header's chain in np.float32, operation by operation -- against ref.step at factor 1, on the
    inputs the GPU tier uses: gradients log-uniform in [1e-3, 10] with one exact zero in eight, parameters N(0, 1), a
    random state (and, from t = 0, also the state torch starts from: a zero accumulator under a zero gradient).  No
    corner needed narrower inputs.  Prints the worst error / bound per corner (a record, not a threshold)."""
    algo, hyper = ref.CORNER[name]
    rng = np.random.default_rng(sum(name.encode()))
    count, worst = 4096, 0.0
    for t in STEP_COUNTS:
        p = rng.normal(0.0, 1.0, count).astype(np.float32)
        g = ref.synthetic_gradient(rng, count)
        assert (g == 0).sum() == count // 8 and np.abs(g[g != 0]).min() >= 1e-3 * (1 - 1e-6) and np.abs(g).max() <= 10.0
        states = [ref.random_state(rng, algo, count)]
        if t == 0:
            states.append({k: v.astype(np.float32) for k, v in ref.initial_state(algo, hyper, p).items()})
        for state in states:
            want_p, want_state, bound = ref.step(algo, hyper, p, g, state, t)
            got_p, got_state = ref.step_f32(algo, hyper, p, g, state, t)
            assert sorted(got_state) == sorted(want_state)
            for key, got, want in [("p", got_p, want_p)] + [(k, got_state[k], want_state[k]) for k in want_state]:
                err = np.abs(got.astype(np.float64) - want)
                assert np.isfinite(want).all() and np.isfinite(bound[key]).all(), (name, t, key)
                ratio = float((err / bound[key]).max())
                assert (err <= bound[key]).all(), (name, t, key, ratio)
                worst = max(worst, ratio)
    print("%s: worst error / bound %.3f" % (name, worst))


# ---- the state_dict conversion ----
def _model(F=5, hidden=(7, 3)):
    from pytorchltr_amd import fused
    torch.manual_seed(3)
    return fused.FusedMLPLoss(F, hidden=hidden)


def _assert_same_state(a, b):
    assert sorted(a) == sorted(b)
    for i in a:
        assert sorted(a[i]) == sorted(b[i]), i
        for name in a[i]:
            x, y = a[i][name], b[i][name]
            assert torch.is_tensor(x) == torch.is_tensor(y)
            assert x.shape == y.shape and x.dtype == y.dtype, (i, name)
            assert torch.equal(x, y), (i, name)


@pytest.mark.parametrize("algo, hyper", [c for c in CONFIGS if c[0] != "sgd" or "momentum" in c[1]],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_state_dict_round_trips_with_torch(algo, hyper):
    from pytorchltr_amd import fused
    model = _model()
    opt = _TORCH[algo](model.parameters(), **hyper)
    gen = torch.Generator().manual_seed(11)
    for _ in range(3):
        for p in model.parameters():
            p.grad = torch.randn(p.shape, generator=gen)
        opt.step()
    theirs = opt.state_dict()
    # torch -> trainer -> torch: the same dict
    trainer = fused.MLPTrainer(model, algo, **hyper)
    trainer.load_state_dict(theirs)
    ours = trainer.state_dict()
    assert ours["param_groups"] == theirs["param_groups"]
    _assert_same_state(ours["state"], theirs["state"])
    assert trainer.steps == (1 if algo == "sgd" else 3)
    # ... and torch loads ours
    again = _TORCH[algo](model.parameters(), **hyper)
    again.load_state_dict(ours)
    _assert_same_state(again.state_dict()["state"], theirs["state"])
    # the pure functions, through a flat buffer with zero-padded W1 rows (F = 5 -> 8) and back
    flat, t = fused.mlp_train_state_from_torch(algo, theirs["state"], 8, 7, 3, w1_cols=5)
    nbuf = 2 if algo == "adam" else 1
    assert flat.shape == (nbuf * (7 * 8 + 7 + 3 * 7 + 3 + 3 + 1),) and flat.dtype == torch.float32
    assert torch.equal(flat[:56].view(7, 8)[:, 5:], torch.zeros(7, 3))
    _assert_same_state(fused.mlp_train_state_to_torch(algo, flat, 3 if algo != "sgd" else t, 8, 7, 3, w1_cols=5),
                       theirs["state"])


@pytest.mark.parametrize("algo, hyper", CONFIGS, ids=["%s-%d" % (a, i) for i, (a, _) in enumerate(CONFIGS)])
def test_a_fresh_trainers_state_dict_is_a_fresh_torch_optimizers(algo, hyper):
    from pytorchltr_amd import fused
    model = _model()
    theirs = _TORCH[algo](model.parameters(), **hyper).state_dict()
    ours = fused.MLPTrainer(model, algo, **hyper).state_dict()
    assert ours["param_groups"] == theirs["param_groups"]
    _assert_same_state(ours["state"], theirs["state"])


def test_load_state_dict_takes_the_groups_hyper_parameters():
    from pytorchltr_amd import fused
    model = _model()
    opt = torch.optim.Adam(model.parameters(), lr=0.02, betas=(0.8, 0.9), weight_decay=0.1)
    trainer = fused.MLPTrainer(model, "adam")
    trainer.load_state_dict(opt.state_dict())
    assert trainer.lr == 0.02 and trainer.hyper["betas"] == (0.8, 0.9) and trainer.hyper["weight_decay"] == 0.1
    assert trainer.steps == 0 and trainer.state_dict()["state"] == {}
    with pytest.raises(ValueError):
        trainer.load_state_dict({"state": {}, "param_groups": [dict(opt.state_dict()["param_groups"][0], params=[0, 1])]})
    with pytest.raises(NotImplementedError):
        trainer.load_state_dict(torch.optim.Adam(model.parameters(), amsgrad=True).state_dict())


def test_load_state_dict_refuses_a_partial_state():
    """One to five per-parameter entries are no state of the six parameters: a ValueError that names the count, and the
    trainer as it was.  None (no step taken) and six load as before."""
    from pytorchltr_amd import fused
    model = _model()
    opt = torch.optim.Adam(model.parameters(), lr=0.02)
    for p in model.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    full = opt.state_dict()
    trainer = fused.MLPTrainer(model, "adam", lr=0.5)
    for count in (1, 3, 5):
        part = {"state": {k: full["state"][k] for k in range(count)}, "param_groups": full["param_groups"]}
        with pytest.raises(ValueError, match=r"\b%d per-parameter entries" % count):
            trainer.load_state_dict(part)
        assert trainer.lr == 0.5 and trainer.steps == 0 and trainer.state_dict()["state"] == {}
    trainer.load_state_dict({"state": {}, "param_groups": full["param_groups"]})
    assert trainer.lr == 0.02 and trainer.steps == 0 and trainer.state_dict()["state"] == {}
    trainer.load_state_dict(full)
    assert trainer.steps == 1
    _assert_same_state(trainer.state_dict()["state"], full["state"])


# ---- the constructor ----
def test_constructor_defaults_are_torch_optims():
    from pytorchltr_amd import fused
    model = _model()
    for algo, cls in _TORCH.items():
        trainer = fused.MLPTrainer(model, algo, lr=0.1)
        want = {k: v for k, v in cls(model.parameters(), lr=0.1).defaults.items()
                if k not in ("maximize", "amsgrad", "differentiable", "foreach", "capturable", "fused")}
        assert trainer.lr == want.pop("lr") == 0.1 and trainer.hyper == want, algo
    assert fused.MLPTrainer(model, "adagrad").lr == torch.optim.Adagrad(model.parameters()).defaults["lr"]
    assert fused.MLPTrainer(model).optimizer == "adagrad"
    trainer = fused.MLPTrainer(model, "sgd", lr=0.5)
    trainer.lr = 0.25                                      # a plain attribute: what a scheduler sets
    assert trainer.state_dict()["param_groups"][0]["lr"] == 0.25


@pytest.mark.parametrize("algo, hyper", [
    ("sgd", dict(lr=-0.1)), ("sgd", dict(lr=0.1, momentum=-1.0)), ("sgd", dict(lr=0.1, weight_decay=-1.0)),
    ("sgd", dict(lr=0.1, nesterov=True)), ("sgd", dict(lr=0.1, nesterov=True, momentum=0.9, dampening=0.5)),
    ("adagrad", dict(lr=-1.0)), ("adagrad", dict(lr_decay=-0.5)), ("adagrad", dict(weight_decay=-0.5)),
    ("adagrad", dict(initial_accumulator_value=-1.0)), ("adagrad", dict(eps=-1.0)),
    ("adam", dict(lr=-1.0)), ("adam", dict(eps=-1.0)), ("adam", dict(betas=(1.0, 0.9))), ("adam", dict(betas=(0.9, -0.1))),
    ("adam", dict(weight_decay=-1.0)),
])
def test_constructor_refuses_what_torch_refuses(algo, hyper):
    from pytorchltr_amd import fused
    model = _model()
    with pytest.raises(ValueError) as theirs:
        _TORCH[algo](model.parameters(), **hyper)
    with pytest.raises(ValueError) as ours:
        fused.MLPTrainer(model, algo, **hyper)
    assert str(ours.value) == str(theirs.value)


def test_constructor_refuses_the_rest():
    from pytorchltr_amd import fused
    model = _model()
    for algo, name in (("sgd", "maximize"), ("adagrad", "maximize"), ("adam", "amsgrad"), ("adam", "maximize"),
                       ("sgd", "differentiable"), ("adam", "differentiable")):
        with pytest.raises(NotImplementedError, match=name):
            fused.MLPTrainer(model, algo, **{name: True})
        fused.MLPTrainer(model, algo, **{name: False})
    with pytest.raises(ValueError, match="optimizer must be"):
        fused.MLPTrainer(model, "rmsprop")
    with pytest.raises(TypeError, match="FusedMLPLoss"):
        fused.MLPTrainer(torch.nn.Linear(5, 1), "sgd", lr=0.1)
    with pytest.raises(TypeError):
        fused.MLPTrainer(model, "adam", no_such_option=1)
    fused.MLPTrainer(model, "adam", foreach=False, capturable=True, fused=None)       # torch's execution switches: ignored


def test_step_needs_a_device(lib):
    from pytorchltr_amd import fused
    model = _model(8)
    trainer = fused.MLPTrainer(model, "sgd", lr=0.1)
    X, y, n = torch.zeros(2, 4, 8), torch.zeros(2, 4, dtype=torch.int64), torch.tensor([4, 2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        trainer.step(X, y, n)


# ---- the code object ----
def test_kernels_are_present_and_do_not_spill():
    from pytorchltr_amd import _codeobj
    from pytorchltr_amd.build import LIB_PATH, build_extension
    build_extension()
    recs = _codeobj.kernel_records(LIB_PATH)     # (needs the llvm tools of the ROCm install: their absence is a failure)
    by_name = {r.get("demangled", r["name"]): r for r in recs}
    new = [r for n, r in by_name.items() if re.match(
        r"(void )?(mlp_reduce_update4_kernel<16>|mlp_reduce_update_kernel|mlp_apply_update_kernel)\(", n)]
    assert len(new) == 3, sorted(n for n in by_name if "update" in n)
    for r in new:
        name = r.get("demangled")
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, name
        assert r["vgpr_count"] + r.get("agpr_count", 0) <= 128, name          # 1024 threads: four waves per SIMD
    # the reductions they repeat are still there, unchanged in name
    assert any(n.startswith("void mlp_reduce4_kernel<16>(") for n in by_name)
    assert any(n.startswith("mlp_reduce_kernel(") for n in by_name)
