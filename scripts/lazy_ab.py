"""A/B of the LAZY step (one launch per step + the flush) between library builds, in one process:
python scripts/lazy_ab.py parent.so new.so [--workload c2 | --case hinge:600x128x136] [--steps 2000] [--regions 7] [--hold 0:8,1:8,...]

Regions of `steps` lazy steps over the workload's rotating batches + the flush, timed on the wall clock like bench.py's
lazy_sgd_step_us, the libraries taking turns region by region (A B A B ...): per library the median and its own min - max, in us
per step.  --hold: further contestants -- the LAST library with ltr_debug_lazy_holdback(everybody's | quiet << 8) set to each
`everybody:quiet` pair, in the same rotation."""
import argparse
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import bench  # noqa: E402
from pytorchltr_amd import _C  # noqa: E402


def load(path):
    lib = ctypes.CDLL(path)
    for name, (res, argt) in list(_C.SIGNATURES.items()) + list(_C.SCHED_SIGNATURES.items()):
        if hasattr(lib, name):
            getattr(lib, name).restype = res
            getattr(lib, name).argtypes = argt
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+")
    ap.add_argument("--workload", default="c2")
    ap.add_argument("--case", default="", help="kind:BxLxF instead of a bench.py workload")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--hold", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, L, F, kind = bench.WORKLOADS[args.workload]
    if args.case:
        kind, shape = args.case.split(":")
        B, L, F = (int(v) for v in shape.split("x"))
        args.workload = args.case
    nbuf = bench.nbuf_for(B, L, F)
    bat = bench.make_batches(B, L, F, nbuf, 0, dev)
    runs = []                                       # (label, FusedStep, hold-back word or None)
    for path in args.libs:
        fs = bench.FusedStep(kind, B, L, F, dev)
        fs.lib = load(path)
        runs.append((os.path.basename(path), fs, None))
    for pair in [h for h in args.hold.split(",") if h]:
        every, quiet = (int(v) for v in pair.split(":"))
        runs.append(("%s hold %d:%d" % (runs[len(args.libs) - 1][0], every, quiet), runs[len(args.libs) - 1][1], every | quiet << 8))

    def region(fs, hold):
        if hold is not None:
            fs.lib.ltr_debug_lazy_holdback(hold)
        t0 = time.perf_counter()
        for i in range(args.steps):
            fs.lazy_step(bat[i % nbuf])
        fs.lazy_flush()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.steps * 1e6
        if hold is not None:
            fs.lib.ltr_debug_lazy_holdback(-1)
        return dt

    for _, fs, hold in runs:                        # warm-up: every contestant once
        region(fs, hold)
    per = [[] for _ in runs]
    for _ in range(args.regions):
        for k, (_, fs, hold) in enumerate(runs):
            per[k].append(region(fs, hold))
    print("%s %dx%dx%d %s: lazy step + flush, us per step over %d regions of %d steps" % (args.workload, B, L, F, kind, args.regions, args.steps))
    for (label, fs, _), ts in zip(runs, per):
        s = sorted(ts)
        print("%-40s median %.3f  min %.3f  max %.3f  spread %.3f" % (label, s[len(s) // 2], s[0], s[-1], s[-1] - s[0]), flush=True)
    sig = [(float(fs.W.double().sum()), float(fs.flat.double().sum())) for _, fs, _ in runs[:len(args.libs)]]
    print("weights / bucket sums per library:", sig, "SAME" if all(v == sig[0] for v in sig) else "(step counts differ between libraries with --hold)")


if __name__ == "__main__":
    main()
