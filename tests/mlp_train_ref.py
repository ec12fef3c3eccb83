"""The three update rules of include/ltr_mlp_train.h (torch.optim's SGD, Adagrad, Adam) restated in fp64 numpy, with the
bound a correct fp32 evaluation of the same chain stays within.  tests/test_mlp_train_host.py pins the rules to
torch.optim on float64 tensors and holds `step_f32` (the chain in np.float32) to the bound on every corner of `CORNERS`;
tests/test_gpu_mlp_train.py and tests/test_gpu_mlp_update.py hold the kernels to it.

``step(algo, hyper, p, g, state, t)`` takes one tensor's parameters `p`, gradient `g`, state (a dict of arrays by torch's
names) and the number of steps already taken `t`, all as they are in memory (fp32 on the device; any float dtype works),
and returns ``(p', state', bound)``: fp64 results, and ``bound["p"]`` / ``bound[name]`` per element.

The bound, derived, not measured.  Every intermediate x of the chain carries (v, M, N): its fp64 value, a magnitude
M >= |v| -- the same expression evaluated on the magnitudes of its terms, so that a cancellation does not hide the
error of what cancelled --, and the number N of fp32 roundings on its chain, such that an fp32 evaluation x^ has
|x^ - v| <= N * u * M to first order in u = 2^-24:

    an input                   (v, |v|, 0)                       it is exact
    c * x, c a scalar          (c v, |c| M, N + 2)               c is rounded to fp32 from the double, the product rounds
    a + b                      (a + b, Ma + Mb, max(Na, Nb) + 1) Na u Ma + Nb u Mb + u |a + b| <= (max + 1) u (Ma + Mb)
    a * b                      (a b, Ma Mb, Na + Nb + 1)
    a / b, b > 0               (a / b, (Ma / b) (Mb / b), Na + Nb + 1)     b's relative error is Nb u Mb / b
    sqrt(a), a > 0             (sqrt a, sqrt(a) Ma / a, Na + 1)            half a's relative error, and one rounding

A fused multiply-add only removes a rounding.  The scalars that depend on t (clr, lr / (1 - beta1^t), sqrt(1 - beta2^t))
are evaluated in fp64 and rounded once: scalars like any other.  The chain is the one the header documents; torch's own
kernels order two of its sums differently (lerp for exp_avg), which is why a comparison with torch.optim itself gets
twice the bound.  On top comes half an ulp of the fp32 result for the final store, and a factor 1 + 2^-10 for the
second-order terms (N^2 u^2, below 2^-40 here)."""
import numpy as np

U = 2.0 ** -24


class _V:
    """(value, magnitude, roundings) of one intermediate; arrays of one shape."""

    def __init__(self, v, m=None, n=0):
        self.v = np.asarray(v, dtype=np.float64)
        self.m = np.abs(self.v) if m is None else np.asarray(m, dtype=np.float64)
        self.n = n

    def scaled(self, c):
        return _V(c * self.v, abs(c) * self.m, self.n + 2)

    def __add__(self, o):
        return _V(self.v + o.v, self.m + o.m, max(self.n, o.n) + 1)

    def __sub__(self, o):
        return _V(self.v - o.v, self.m + o.m, max(self.n, o.n) + 1)

    def __mul__(self, o):
        return _V(self.v * o.v, self.m * o.m, self.n + o.n + 1)

    def __truediv__(self, o):
        with np.errstate(divide="ignore", invalid="ignore"):
            return _V(self.v / o.v, (self.m / o.v) * (o.m / o.v), self.n + o.n + 1)

    def sqrt(self):
        r = np.sqrt(self.v)
        with np.errstate(divide="ignore", invalid="ignore"):
            amp = np.where(self.v > 0, self.m / self.v, 1.0)
        return _V(r, r * amp, self.n + 1)

    def bound(self):
        """N u M (1 + 2^-10) + half an ulp of the fp32 result."""
        half_ulp = 0.5 * np.spacing(np.abs(self.v).astype(np.float32)).astype(np.float64)
        return self.n * U * self.m * (1.0 + 2.0 ** -10) + half_ulp


def step(algo, hyper, p, g, state, t):
    """One step of `algo` ("sgd", "adagrad", "adam") on one tensor; `t` = steps taken before this one."""
    p, g = _V(p), _V(g)
    wd = float(hyper.get("weight_decay", 0.0))
    lr = float(hyper["lr"])
    if wd != 0.0:
        g = g + p.scaled(wd)
    new, out = {}, {}
    if algo == "sgd":
        mu = float(hyper.get("momentum", 0.0))
        if mu != 0.0:
            if t == 0:
                buf = g
            else:
                buf = _V(state["momentum_buffer"]).scaled(mu) + g.scaled(1.0 - float(hyper.get("dampening", 0.0)))
            new["momentum_buffer"] = buf
            g = g + buf.scaled(mu) if hyper.get("nesterov") else buf
        p = p - g.scaled(lr)
    elif algo == "adagrad":
        clr = lr / (1.0 + t * float(hyper.get("lr_decay", 0.0)))
        s = _V(state["sum"]) + g * g
        new["sum"] = s
        eps = _V(np.full_like(s.v, float(hyper.get("eps", 1e-10))), n=1)
        p = p - (g / (s.sqrt() + eps)).scaled(clr)
    elif algo == "adam":
        b1, b2 = [float(b) for b in hyper.get("betas", (0.9, 0.999))]
        m = _V(state["exp_avg"]).scaled(b1) + g.scaled(1.0 - b1)
        v = _V(state["exp_avg_sq"]).scaled(b2) + (g * g).scaled(1.0 - b2)
        new["exp_avg"], new["exp_avg_sq"] = m, v
        step_size = lr / (1.0 - b1 ** (t + 1))
        bc2_sqrt = (1.0 - b2 ** (t + 1)) ** 0.5
        eps = _V(np.full_like(v.v, float(hyper.get("eps", 1e-8))), n=1)
        p = p - (m / (v.sqrt().scaled(1.0 / bc2_sqrt) + eps)).scaled(step_size)
    else:
        raise ValueError(algo)
    bound = {"p": p.bound()}
    for name, x in new.items():
        out[name] = x.v
        bound[name] = x.bound()
    return p.v, out, bound


def step_f32(algo, hyper, p, g, state, t):
    """The chain of `step` evaluated operation by operation in np.float32, as include/ltr_mlp_train.h words it: wd, lr,
    mu, 1 - dampening, eps, the betas and 1 - beta rounded to fp32 from the double, the scalars that depend on t
    evaluated in fp64 and rounded once, no fused multiply-add.  Returns ``(p', state')`` as float32 arrays: one correct
    fp32 evaluation, which `step`'s bound must hold (tests/test_mlp_train_host.py)."""
    f = np.float32
    p, g = np.asarray(p, dtype=f), np.asarray(g, dtype=f)
    wd, lr = f(hyper.get("weight_decay", 0.0)), f(hyper["lr"])
    if wd != 0:
        g = g + wd * p
    new = {}
    if algo == "sgd":
        mu = f(hyper.get("momentum", 0.0))
        if mu != 0:
            if t == 0:
                buf = g
            else:
                omd = f(1.0 - float(hyper.get("dampening", 0.0)))
                buf = mu * np.asarray(state["momentum_buffer"], dtype=f) + omd * g
            new["momentum_buffer"] = buf
            g = g + mu * buf if hyper.get("nesterov") else buf
        p = p - lr * g
    elif algo == "adagrad":
        clr = f(float(hyper["lr"]) / (1.0 + t * float(hyper.get("lr_decay", 0.0))))
        s = np.asarray(state["sum"], dtype=f) + g * g
        new["sum"] = s
        p = p - clr * (g / (np.sqrt(s) + f(hyper.get("eps", 1e-10))))
    elif algo == "adam":
        b1, b2 = [float(b) for b in hyper.get("betas", (0.9, 0.999))]
        m = f(b1) * np.asarray(state["exp_avg"], dtype=f) + f(1.0 - b1) * g
        v = f(b2) * np.asarray(state["exp_avg_sq"], dtype=f) + f(1.0 - b2) * (g * g)
        new["exp_avg"], new["exp_avg_sq"] = m, v
        step_size = f(float(hyper["lr"]) / (1.0 - b1 ** (t + 1)))
        bc2_sqrt = f((1.0 - b2 ** (t + 1)) ** 0.5)
        p = p - step_size * (m / (np.sqrt(v) / bc2_sqrt + f(hyper.get("eps", 1e-8))))
    else:
        raise ValueError(algo)
    assert p.dtype == f and all(x.dtype == f for x in new.values())
    return p, new


# The corner grid of the update rules: every zero-coefficient short cut of the kernels taken and not taken, one full
# set per rule.  (id, algo, torch.optim's keyword arguments); CPU and GPU tiers share it.
CORNERS = [
    ("sgd-plain", "sgd", dict(lr=0.05)),
    ("sgd-wd", "sgd", dict(lr=0.05, weight_decay=0.01)),
    ("sgd-mu", "sgd", dict(lr=0.05, momentum=0.9)),
    ("sgd-mu-damp-wd", "sgd", dict(lr=0.05, momentum=0.9, dampening=0.3, weight_decay=0.02)),
    ("sgd-nesterov-wd", "sgd", dict(lr=0.05, momentum=0.8, nesterov=True, weight_decay=0.01)),
    ("sgd-lr0-mu", "sgd", dict(lr=0.0, momentum=0.9)),
    ("adagrad-defaults", "adagrad", dict(lr=0.1)),
    ("adagrad-decay", "adagrad", dict(lr=0.1, lr_decay=0.05)),
    ("adagrad-wd", "adagrad", dict(lr=0.1, weight_decay=0.01)),
    ("adagrad-init", "adagrad", dict(lr=0.1, initial_accumulator_value=0.5)),
    ("adagrad-full", "adagrad", dict(lr=0.1, lr_decay=0.05, weight_decay=0.01, initial_accumulator_value=0.5, eps=1e-6)),
    ("adam-defaults", "adam", dict(lr=0.01)),
    ("adam-wd", "adam", dict(lr=0.01, weight_decay=0.03)),
    ("adam-beta1-0", "adam", dict(lr=0.01, betas=(0.0, 0.999))),
    ("adam-beta2-0", "adam", dict(lr=0.01, betas=(0.9, 0.0))),
    ("adam-full", "adam", dict(lr=0.01, betas=(0.7, 0.95), eps=1e-5, weight_decay=0.03)),
]
CORNER = {name: (algo, hyper) for name, algo, hyper in CORNERS}
STATE_NAMES = {"sgd": ("momentum_buffer",), "adagrad": ("sum",), "adam": ("exp_avg", "exp_avg_sq")}
POSITIVE_STATE = ("sum", "exp_avg_sq")


def synthetic_gradient(rng, count):
    """`count` float32 gradients: magnitudes log-uniform in [1e-3, 10], random signs, one element in eight exactly 0."""
    g = np.exp(rng.uniform(np.log(1e-3), np.log(10.0), count)) * rng.choice([-1.0, 1.0], count)
    g[rng.permutation(count)[:max(1, count // 8)]] = 0.0
    return g.astype(np.float32)


def random_state(rng, algo, count):
    """Random float32 state buffers by torch's names; `sum` and `exp_avg_sq` positive."""
    out = {}
    for name in STATE_NAMES[algo]:
        x = rng.normal(0.0, 1.0, count)
        out[name] = (np.abs(x) + 1e-3 if name in POSITIVE_STATE else x).astype(np.float32)
    return out


def initial_state(algo, hyper, like):
    """The state torch starts from: zeros (Adagrad: its initial accumulator value)."""
    z = np.zeros_like(np.asarray(like, dtype=np.float64))
    if algo == "sgd":
        return {"momentum_buffer": z} if float(hyper.get("momentum", 0.0)) != 0.0 else {}
    if algo == "adagrad":
        return {"sum": z + float(hyper.get("initial_accumulator_value", 0.0))}
    return {"exp_avg": z, "exp_avg_sq": z.copy()}
