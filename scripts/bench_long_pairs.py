"""The pairwise losses on lists longer than 4096 documents (long_lists=True, ltr_pairwise_loss_long_f32): loss and
gradient in one call.

Prints one JSON line: per shape (queries x list size, ragged n, int64 labels in [0, 5)) and kind, the median time in us
of one call that returns loss[B] and dscores[B, L].
  long shapes   -- the long path: owner tiles against the streamed query, a finish kernel (LambdaNDCG2: two key sorts
                   and their epilogues in front);
  the --compare shape (64x4096, the longest list the one-workgroup kernels take) -- `existing`: ltr_pairwise_loss_f32;
                   `long`: the long path forced onto the same batches by ltr_debug_long_pairs_all; `long_over_existing`.
                   The long path evaluates every unordered pair twice, so about 2x is what the design costs.
Nobody else has a number for the long shapes: the reference's (B, L, L) pair tensors do not fit at 20 000 documents.
Each region is one call per batch of a rotating set (at most --max-batches: the calls are compute bound, milliseconds
each at the largest shape), timed by device events around a synchronised region; the median of --regions regions after
--warmup untimed ones.

    python scripts/bench_long_pairs.py [--regions 5] [--warmup 1] [--shapes 64x5000,16x20000,4x65536]
                                       [--compare 64x4096] [--kinds hinge,logistic,ndcg2]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorchltr_amd import _C  # noqa: E402
from pytorchltr_amd._autograd import pairwise_loss_and_grad  # noqa: E402

CACHE_BYTES = 256 << 20


def batches(B, L, dev, max_batches, seed=0):
    """(scores, labels, n) batches: more than the last-level cache holds, capped at max_batches."""
    per = B * L * (4 + 8) + B * 8
    count = min(max_batches, max(2, -(-(CACHE_BYTES + (32 << 20)) // per)))
    g = torch.Generator(device=dev).manual_seed(seed)
    out = []
    for _ in range(count):
        s = torch.randn(B, L, device=dev, generator=g)
        y = torch.randint(0, 5, (B, L), device=dev, generator=g)
        n = torch.randint(1, L + 1, (B,), device=dev, generator=g)
        out.append((s, y, n))
    return out


def time_region(fn, data, regions, warmup):
    """Median us per call of fn on one batch, from `regions` event-timed regions of len(data) calls each."""
    times = []
    for r in range(warmup + regions):
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for s, y, n in data:
            fn(s, y, n)
        stop.record()
        torch.cuda.synchronize()
        if r >= warmup:
            times.append(start.elapsed_time(stop) * 1000.0 / len(data))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-batches", type=int, default=16)
    ap.add_argument("--shapes", default="64x5000,16x20000,4x65536")
    ap.add_argument("--compare", default="64x4096")
    ap.add_argument("--kinds", default="hinge,logistic,ndcg2")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _C.lib()
    kinds = [(k, _C.__dict__[k.upper()]) for k in args.kinds.split(",")]
    own, ch = _C.long_pair_geometry()
    result = {"unit": "us per call (loss and gradient)", "owner_docs": own, "chunk_docs": ch, "shapes": {}, "compare": {}}

    def long_call(code):
        return lambda s, y, n: pairwise_loss_and_grad(s, y, n, code, long_lists=True)

    for shape in [v for v in args.shapes.split(",") if v]:
        B, L = (int(v) for v in shape.split("x"))
        data = batches(B, L, dev, args.max_batches)
        row = {name: round(time_region(long_call(code), data, args.regions, args.warmup), 1) for name, code in kinds}
        row["batches"] = len(data)
        result["shapes"][shape] = row
        del data
        torch.cuda.empty_cache()

    for shape in [v for v in args.compare.split(",") if v]:
        B, L = (int(v) for v in shape.split("x"))
        data = batches(B, L, dev, args.max_batches)
        row = {}
        for name, code in kinds:
            existing = time_region(lambda s, y, n: pairwise_loss_and_grad(s, y, n, code), data, args.regions, args.warmup)
            prev = lib.ltr_debug_long_pairs_all(1)
            try:
                forced = time_region(long_call(code), data, args.regions, args.warmup)
            finally:
                lib.ltr_debug_long_pairs_all(prev)
            row[name] = {"existing": round(existing, 1), "long": round(forced, 1),
                         "long_over_existing": round(forced / existing, 2)}
        row["batches"] = len(data)
        result["compare"][shape] = row
        del data
        torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
