"""GPU tier of the MLP trainer's update launches on their own (run with `-m gpu` on an MI355X), through the C ABI of
include/ltr_mlp_train.h: ltr_mlp_apply_update_f32 (mlp_apply_update_kernel) on synthetic flat gradients -- no scorer
launch, so every network, row pitch, alignment and step count is reachable with a few thousand floats -- and
ltr_mlp_train_step_f32's two reduce-and-update kernels behind the pairwise MFMA launch.

The reference is tests/mlp_train_ref.py: the fp64 rule and its derived per-element bound at factor 1, on every element
of every parameter and state tensor; nothing here is a measured tolerance.  The hyper-parameter sets are ref.CORNERS,
the gradients ref.synthetic_gradient (log-uniform magnitudes, one exact zero in eight), the parameters N(0, 1), the
state random (`sum` and `exp_avg_sq` positive).  The gradient columns of W1's zero padding hold NaN: they must reach
neither a parameter nor a state element.  Every device buffer lies between guard floats of a fixed bit pattern that
must be there afterwards: what catches a float4 written over a tail, a padded column or a neighbouring tensor."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import mlp_train_ref as ref

pytestmark = pytest.mark.gpu

NETWORKS = [(3, 2, 1), (8, 5, 3), (8, 64, 16), (136, 50, 10), (224, 64, 16)]        # (F, H1, H2); P = 13, 67, ...
FULL = {"sgd": "sgd-mu-damp-wd", "adagrad": "adagrad-full", "adam": "adam-full"}    # the corner that uses all its state
LONG_RUN = ("adagrad-decay", "adagrad-full", "adam-beta1-0", "adam-beta2-0")        # also from t = 999 and 10**6
GUARD = 8
PATTERN = 0x7FE5C3E1                             # (a quiet NaN's bits: a guard that is read poisons what reads it)
WORST = {}                                       # rule -> the worst error / bound seen (a record, printed per test)


def _pitches(F):
    """w1_pitch: F, F - 1, and on the wider rows a whole float4 of padding (F - 3, F - 4) and bf16's pad-to-8 (F - 7)."""
    return [F, F - 1] + ([F - 3, F - 4, F - 7] if F >= 8 else [])


def _dev():
    assert torch.cuda.is_available(), "GPU tier needs a ROCm device"
    return torch.device("cuda:0")


def _sizes(net):
    F, H1, H2 = net
    return (H1 * F, H1, H2 * H1, H2, H2, 1)


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


class _Guarded:
    """`payload` (float32) on the device, `offset` floats behind a 16-byte line, GUARD pattern floats on either side."""

    def __init__(self, payload, offset=0):
        payload = np.ascontiguousarray(payload, dtype=np.float32).reshape(-1)
        self.lo, self.n = GUARD + offset, payload.size
        host = np.full(self.lo + self.n + GUARD + (-(offset + self.n)) % 4, PATTERN, dtype=np.int32)
        host[self.lo:self.lo + self.n] = payload.view(np.int32)
        self.base = torch.from_numpy(host).to(_dev())
        assert self.base.data_ptr() % 16 == 0
        self.ptr = self.base.data_ptr() + 4 * self.lo

    def read(self):
        """The payload as it is now; asserts the guards."""
        host = self.base.cpu().numpy()
        outside = np.concatenate([host[:self.lo], host[self.lo + self.n:]])
        assert (outside == PATTERN).all(), "a guard float was overwritten"
        return host[self.lo:self.lo + self.n].view(np.float32).copy()


def _optim(name, lr=None):
    from pytorchltr_amd import _C
    algo, hyper = ref.CORNER[name]
    b1, b2 = hyper.get("betas", (0.9, 0.999))
    return _C.MLPOptim(algo={"sgd": _C.OPT_SGD, "adagrad": _C.OPT_ADAGRAD, "adam": _C.OPT_ADAM}[algo],
                       nesterov=1 if hyper.get("nesterov") else 0, lr=hyper["lr"] if lr is None else lr,
                       weight_decay=hyper.get("weight_decay", 0.0), momentum=hyper.get("momentum", 0.0),
                       dampening=hyper.get("dampening", 0.0), lr_decay=hyper.get("lr_decay", 0.0),
                       eps=hyper.get("eps", 1e-10 if algo == "adagrad" else 1e-8), beta1=b1, beta2=b2)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _real(net, pitch):
    """The flat layout's elements that are parameters: all but W1's columns >= pitch."""
    F, H1, _ = net
    mask = np.ones(sum(_sizes(net)), dtype=bool)
    mask[:H1 * F].reshape(H1, F)[:, pitch:] = False
    return _frozen(mask)[0]


@functools.lru_cache(maxsize=None)
def _inputs(net, pitch, algo, seed=0):
    """(p, g, state) of a case, flat in the gradient's layout (rows of F floats): p N(0, 1) (its padded columns are
    not parameters and go nowhere), g synthetic with NaN in the padded columns, state (nbuf, P) random."""
    P = sum(_sizes(net))
    rng = np.random.default_rng(100000 * net[0] + 1000 * net[1] + 10 * pitch + len(algo) + 7919 * seed)
    p = rng.normal(0.0, 1.0, P).astype(np.float32)
    g = ref.synthetic_gradient(rng, P)
    g[~_real(net, pitch)] = np.nan
    state = ref.random_state(rng, algo, P)
    return _frozen(p, g, np.stack([state[k] for k in ref.STATE_NAMES[algo]]))


def _initial(net, name):
    algo, hyper = ref.CORNER[name]
    P = sum(_sizes(net))
    fill = float(hyper.get("initial_accumulator_value", 0.0)) if algo == "adagrad" else 0.0
    return np.full((len(ref.STATE_NAMES[algo]), P), fill, dtype=np.float32)


def _state_words(net, algo, state, t):
    """The state as include/ltr_mlp_train.h lays it out: the buffers, zeros up to a multiple of 4, {t, 0, 0, 0}."""
    from pytorchltr_amd import _C
    F, H1, H2 = net
    code = {"sgd": _C.OPT_SGD, "adagrad": _C.OPT_ADAGRAD, "adam": _C.OPT_ADAM}[algo]
    count = int(_C.lib().ltr_mlp_train_state_floats(code, F, H1, H2))
    assert count == (state.size + 3) // 4 * 4 + 4
    words = np.zeros(count, dtype=np.float32)
    words[:state.size] = state.reshape(-1)
    words.view(np.int32)[count - 4] = t
    return words


class _Params:
    """The six parameters on the device.  layout "sep": six guarded buffers of their own, 16-byte aligned; ("flat", k):
    consecutive views of ONE guarded buffer entered k floats behind a 16-byte line, with one guard float between W1 and
    b1 (so a float4 across W1's end has somewhere wrong to land) -- the addresses fall where the sizes put them, and
    over k = 0 .. 3 every tensor starts at every residue."""

    def __init__(self, net, pitch, p, layout):
        F, H1, H2 = net
        sizes = _sizes(net)
        parts = list(np.split(p, np.cumsum(sizes)[:-1]))
        parts[0] = np.ascontiguousarray(parts[0].reshape(H1, F)[:, :pitch]).reshape(-1)
        self.net, self.pitch, self.lengths = net, pitch, [x.size for x in parts]
        if layout == "sep":
            self.bufs = [_Guarded(x) for x in parts]
            self.ptrs = [b.ptr for b in self.bufs]
        else:
            gap = np.array([PATTERN], dtype=np.int32).view(np.float32)
            self.bufs = [_Guarded(np.concatenate([parts[0], gap] + parts[1:]), layout[1])]
            starts = np.concatenate([[0], np.cumsum(self.lengths)[:-1]]) + np.array([0, 1, 1, 1, 1, 1])
            self.starts = [int(s) for s in starts]
            self.ptrs = [self.bufs[0].ptr + 4 * s for s in self.starts]

    def read(self, before):
        """The parameters in the flat layout of rows of F floats (the padded columns: `before`'s, as they were)."""
        F, H1, H2 = self.net
        if len(self.bufs) == 6:
            parts = [b.read() for b in self.bufs]
        else:
            whole = self.bufs[0].read()
            assert _bits(whole)[self.lengths[0]] == PATTERN, "the float between W1 and b1 was overwritten"
            parts = [whole[s:s + n] for s, n in zip(self.starts, self.lengths)]
        w1 = before[:H1 * F].reshape(H1, F).copy()
        w1[:, :self.pitch] = parts[0].reshape(H1, self.pitch)
        return np.concatenate([w1.reshape(-1)] + parts[1:])


def _apply(net, pitch, name, t, p, g, state, params="sep", state_offset=0, grads_offset=0):
    """One ltr_mlp_apply_update_f32 launch from (p, g, state, t): (p', state' or None, the header's four words)."""
    from pytorchltr_amd import _C
    algo = ref.CORNER[name][0]
    F, H1, H2 = net
    pars = _Params(net, pitch, p, params)
    gbuf = _Guarded(g, grads_offset)
    sbuf = None if state is None else _Guarded(_state_words(net, algo, state, t), state_offset)
    optim = _optim(name)
    _C.check(_C.lib().ltr_mlp_apply_update_f32(gbuf.ptr, *pars.ptrs, pitch, None if sbuf is None else sbuf.ptr,
                                               ctypes.byref(optim), F, H1, H2, _C.stream_of(gbuf.base)))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(gbuf.read()), _bits(g)), "the gradient is an input"
    if sbuf is None:
        return pars.read(p), None, None
    words = sbuf.read()
    return pars.read(p), words[:state.size].reshape(state.shape), [int(w) for w in _bits(words)[-4:]]


def _check(net, pitch, name, t, p, g, state, got):
    """Every parameter and state element within the bound of ref.step from (p, g, state, t); the state of the padded
    columns, and of a rule that keeps none, bit for bit what it was; the header counted.  Returns the worst ratio."""
    algo, hyper = ref.CORNER[name]
    real = _real(net, pitch)
    got_p, got_state, header = got
    names = ref.STATE_NAMES[algo]
    before = {k: state[b][real] for b, k in enumerate(names)} if state is not None else ref.initial_state(algo, hyper, p[real])
    want_p, want_state, bound = ref.step(algo, hyper, p[real], g[real], before, t)
    err = np.abs(got_p[real].astype(np.float64) - want_p)
    worst = float((err / bound["p"]).max())
    assert (err <= bound["p"]).all(), (net, pitch, name, t, "p", worst)
    assert np.array_equal(_bits(got_p[~real]), _bits(p[~real]))
    if state is not None:
        for b, key in enumerate(names):
            assert np.array_equal(_bits(got_state[b][~real]), _bits(state[b][~real])), (net, pitch, name, t, key, "padding")
            if key in want_state:
                err = np.abs(got_state[b][real].astype(np.float64) - want_state[key])
                ratio = float((err / bound[key]).max())
                assert (err <= bound[key]).all(), (net, pitch, name, t, key, ratio)
                worst = max(worst, ratio)
            else:                                                   # SGD without momentum: the buffer is never touched
                assert np.array_equal(_bits(got_state[b]), _bits(state[b])), (net, pitch, name, t, key)
        assert header == [t + 1, 0, 0, 0], (net, pitch, name, t, header)
    WORST[algo] = max(WORST.get(algo, 0.0), worst)
    return worst


def _same(a, b):
    """Two launches' results, bit for bit."""
    return (np.array_equal(_bits(a[0]), _bits(b[0])) and a[2] == b[2]
            and (a[1] is None) == (b[1] is None) and (a[1] is None or np.array_equal(_bits(a[1]), _bits(b[1]))))


def _report(what):
    print("%s: worst error / bound so far %s" % (what, {k: round(v, 3) for k, v in sorted(WORST.items())}))


# ---- one step, every corner ----
@pytest.mark.parametrize("name", [c[0] for c in ref.CORNERS])
def test_one_step_at_every_corner(name):
    """(8, 5, 3) at every pitch (P = 67: every segment start misaligned, a float4 tail) and (136, 50, 10) at pitch F
    (eight blocks), from t = 0 and t = 7 on a random state, from t = 0 also on the state a caller starts from (a zero
    accumulator under a zero gradient), and for the rules whose t-dependent factor has a long run from t = 999 and
    10**6.  A rule without state runs with a state (the header is counted, the buffer untouched) and with NULL."""
    algo, hyper = ref.CORNER[name]
    for net, pitches in (((8, 5, 3), _pitches(8)), ((136, 50, 10), [136])):
        for pitch in pitches:
            p, g, state = _inputs(net, pitch, algo)
            for t in (0, 7) + ((999, 10 ** 6) if name in LONG_RUN else ()):
                _check(net, pitch, name, t, p, g, state, _apply(net, pitch, name, t, p, g, state))
            first = _initial(net, name)
            _check(net, pitch, name, 0, p, g, first, _apply(net, pitch, name, 0, p, g, first))
            if algo == "sgd" and not hyper.get("momentum"):
                _check(net, pitch, name, 0, p, g, None, _apply(net, pitch, name, 0, p, g, None))
    _report(name)


def test_sgd_first_step_rule_reads_the_header():
    """With momentum, t = 0 overwrites a non-zero buffer with g (no decay, no dampening: g's own bits); t = 1 folds
    the buffer in."""
    net, pitch, name = (8, 5, 3), 7, "sgd-mu"
    real = _real(net, pitch)
    p, g, state = _inputs(net, pitch, "sgd")
    assert (state[0][real] != 0).all()
    first = _apply(net, pitch, name, 0, p, g, state)
    _check(net, pitch, name, 0, p, g, state, first)
    assert np.array_equal(_bits(first[1][0][real]), _bits(g[real])) and first[2][0] == 1
    second = _apply(net, pitch, name, 1, p, g, state)
    _check(net, pitch, name, 1, p, g, state, second)
    assert (second[1][0][real] != g[real]).all() and second[2][0] == 2


# ---- five consecutive launches ----
@pytest.mark.parametrize("algo", list(FULL))
@pytest.mark.parametrize("net", [(224, 64, 16), (3, 2, 1)], ids=["224x64x16", "3x2x1"])
def test_five_consecutive_launches(net, algo):
    """Five launches on ONE set of device buffers, a new gradient each, from the state a caller starts with; each step
    is checked from its own snapshot and the header counts 1 .. 5."""
    from pytorchltr_amd import _C
    name = FULL[algo]
    F, H1, H2 = net
    p, _, _ = _inputs(net, F, algo)
    state = _initial(net, name)
    pars = _Params(net, F, p, "sep")
    sbuf = _Guarded(_state_words(net, algo, state, 0))
    optim = _optim(name)
    for t in range(5):
        g = _inputs(net, F, algo, seed=t + 1)[1]
        gbuf = _Guarded(g)
        _C.check(_C.lib().ltr_mlp_apply_update_f32(gbuf.ptr, *pars.ptrs, F, sbuf.ptr, ctypes.byref(optim), F, H1, H2,
                                                   _C.stream_of(gbuf.base)))
        torch.cuda.synchronize()
        words = sbuf.read()
        got = (pars.read(p), words[:state.size].reshape(state.shape), [int(w) for w in _bits(words)[-4:]])
        _check(net, F, name, t, p, g, state, got)
        p, state = got[0], got[1]
    _report("five launches, %s" % name)


# ---- layouts ----
LAYOUTS = {
    "a": dict(),                                                 # separate aligned tensors
    "b": dict(params=("flat", 0)),                               # six views of one flat buffer
    "c1": dict(params=("flat", 1)), "c2": dict(params=("flat", 2)), "c3": dict(params=("flat", 3)),
    "d": dict(state_offset=1),                                   # P % 4 != 0: vec0 != vec1, both ways over (a) and (d)
    "e": dict(grads_offset=1),
}


@pytest.mark.parametrize("algo", list(FULL))
@pytest.mark.parametrize("net", NETWORKS, ids=["x".join(map(str, n)) for n in NETWORKS])
def test_layouts_give_the_same_bits(net, algo):
    """The same step under every layout of parameters, state and gradient, at every pitch: within the bound, the guards
    intact, and BIT-IDENTICAL across the layouts -- the arithmetic of an element does not depend on how it was loaded.
    Layout (a) runs twice: the same bits run to run."""
    name = FULL[algo]
    for pitch in _pitches(net[0]):
        p, g, state = _inputs(net, pitch, algo)
        first = _apply(net, pitch, name, 3, p, g, state)
        _check(net, pitch, name, 3, p, g, state, first)
        assert _same(first, _apply(net, pitch, name, 3, p, g, state)), (net, pitch, name, "run to run")
        for key, layout in LAYOUTS.items():
            if key != "a":
                assert _same(first, _apply(net, pitch, name, 3, p, g, state, **layout)), (net, pitch, name, key)
    _report("layouts, %s" % name)


# ---- the two reduce-and-update kernels ----
@functools.lru_cache(maxsize=None)
def _batch():
    B, L, F = 3, 5, 8
    rng = np.random.default_rng(31)
    dev = _dev()
    xs = torch.from_numpy(rng.normal(0, 1, (B, L, F)).astype(np.float32)).to(dev)
    ys = torch.from_numpy(rng.integers(0, 5, (B, L))).to(dev)
    n = torch.tensor([5, 2, 4], dtype=torch.int64, device=dev)
    return xs, ys, n


@pytest.mark.parametrize("algo", list(FULL))
@pytest.mark.parametrize("pitch", [8, 5])
@pytest.mark.parametrize("workspace", ["aligned", "offset-1"])
def test_reduce_and_update_kernels(workspace, pitch, algo):
    """ltr_mlp_train_step_f32 (pairwise hinge, B = 3, L = 5, F = 8, hidden (5, 3)) with the workspace 16-byte aligned
    (mlp_reduce_update4_kernel) and one float off (mlp_reduce_update_kernel), W1 at pitch 8 and at pitch 5 behind its
    zero-padded image W1_rows; the parameters as separate tensors and as views of a flat buffer at offsets 1 .. 3,
    `grads_out` aligned and one float off.  The gradient is ltr_mlp_pairwise_f32's bit for bit (same workspace, the
    scorer reading the same W1 image), the update within the bound of ref.step on that gradient, the guards intact;
    each kernel gives the same bits under every layout, and the two kernels agree within the bound.
    (Off the separate layout the MFMA launch reads W1 through an aligned W1_rows copy: the scorer's own alignment
    rules are not what this test is about.)"""
    from pytorchltr_amd import _C, fused
    name = FULL[algo]
    net = (8, 5, 3)
    F, H1, H2 = net
    B, L = 3, 5
    lib, dev = _C.lib(), _dev()
    xs, ys, n = _batch()
    st = _C.stream_of(xs)
    P, ws_bytes = fused._mlp_sizes_for(B, F, H1, H2)
    off = 0 if workspace == "aligned" else 1
    ws = torch.empty(ws_bytes // 4 + 4, device=dev)[off:]
    assert ws.data_ptr() % 16 == 4 * off
    p, _, state = _inputs(net, pitch, algo, seed=9)
    p = p * np.float32(0.3)                                        # (a scorer's weights: keep the hidden units alive)
    real = _real(net, pitch)
    image = p[:H1 * F].reshape(H1, F).copy()
    image[:, pitch:] = 0.0                                         # what the MFMA launch reads as W1
    rows = torch.from_numpy(image).to(dev)
    small = [torch.from_numpy(x.copy()).to(dev) for x in np.split(p, np.cumsum(_sizes(net))[:-1])[1:]]
    want_loss, want_lsum, want_grads = torch.empty(B, device=dev), torch.empty(1, device=dev), torch.empty(P, device=dev)
    _C.check(lib.ltr_mlp_pairwise_f32(0, 1.0, xs.data_ptr(), rows.data_ptr(), *[t.data_ptr() for t in small], ys.data_ptr(),
                                      0, n.data_ptr(), None, B, L, F, H1, H2, want_loss.data_ptr(), None,
                                      want_grads.data_ptr(), want_lsum.data_ptr(), ws.data_ptr(), ws_bytes, st))
    torch.cuda.synchronize()
    g = want_grads.cpu().numpy()
    assert np.isfinite(g).all() and (g != 0).mean() > 0.25
    if pitch < F:
        assert (g[~real] != 0).any()                               # the dropped columns do carry a gradient
    optim = _optim(name)
    first = None
    for layout in ("sep", ("flat", 1), ("flat", 2), ("flat", 3)):
        for grads_offset in (0, 1):
            pars = _Params(net, pitch, p, layout)
            sbuf = _Guarded(_state_words(net, algo, state, 2))
            gout = _Guarded(np.zeros(P, dtype=np.float32), grads_offset)
            loss, lsum = torch.empty(B, device=dev), torch.empty(1, device=dev)
            w1_rows = rows.data_ptr() if pitch < F or layout != "sep" else None
            _C.check(lib.ltr_mlp_train_step_f32(
                _C.MLP_TRAIN_PAIRWISE, 0, 0, 1.0, xs.data_ptr(), *pars.ptrs, pitch, w1_rows, ys.data_ptr(), 0, n.data_ptr(),
                None, 0, 0, None, None, B, L, F, H1, H2, loss.data_ptr(), None, lsum.data_ptr(), sbuf.ptr,
                ctypes.byref(optim), gout.ptr, ws.data_ptr(), ws_bytes, st))
            torch.cuda.synchronize()
            assert np.array_equal(_bits(gout.read()), _bits(g)), (layout, grads_offset)
            assert torch.equal(loss, want_loss) and torch.equal(lsum, want_lsum)
            words = sbuf.read()
            got = (pars.read(p), words[:state.size].reshape(state.shape), [int(w) for w in _bits(words)[-4:]])
            _check(net, pitch, name, 2, p, g, state, got)
            if first is None:
                first = got
            assert _same(first, got), (layout, grads_offset)
    # the update alone on the same gradient: the third kernel, within the bound of the same reference
    _check(net, pitch, name, 2, p, g, state, _apply(net, pitch, name, 2, p, g, state))
    _report("reduce and update, %s, workspace %s" % (name, workspace))
