"""evaluate() with nine metrics against the separate calls a validation pass makes without it.

Prints one JSON line: per shape (queries x list size, ragged n, int64 labels in [0, 5)), the median time in us of
  evaluate   -- evaluate(metrics=ndcg@1, @3, @5, @10, map, mrr, p@10, recall@10, err@10), one call;
  separate   -- ndcg(k=1), ndcg(k=3), ndcg(k=5), ndcg(k=10) and arp(): five calls;
  ndcg10_x2  -- two ndcg(k=10) calls (the target: evaluate below this).
Each region is R calls, one per batch of a rotating set larger than the 256 MiB last-level cache, timed by device
events around a synchronised region; the median of --regions regions after --warmup untimed ones.  Default tie
mode ("random"): every call draws its seed on the host, as a user's call does.

    python scripts/bench_eval.py [--regions 7] [--warmup 2] [--shapes 1024x128,16384x1000,64x20000]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytorchltr_amd.evaluation as ev  # noqa: E402

NINE = ("ndcg@1", "ndcg@3", "ndcg@5", "ndcg@10", "map", "mrr", "p@10", "recall@10", "err@10")
CACHE_BYTES = 256 << 20


def batches(B, L, dev, seed=0):
    """Enough (scores, labels, n) batches that one pass over them streams more than the last-level cache."""
    per = B * L * (4 + 8) + B * 8
    count = max(2, -(-(CACHE_BYTES + (32 << 20)) // per))
    g = torch.Generator(device=dev).manual_seed(seed)
    out = []
    for _ in range(count):
        s = torch.randn(B, L, device=dev, generator=g)
        y = torch.randint(0, 5, (B, L), device=dev, generator=g)
        n = torch.randint(1, L + 1, (B,), device=dev, generator=g)
        out.append((s, y, n))
    return out


def time_region(fn, data, regions, warmup):
    """Median us per pass of fn over one batch, from `regions` event-timed regions of len(data) passes each."""
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


def separate(s, y, n):
    for k in (1, 3, 5, 10):
        ev.ndcg(s, y, n, k=k)
    ev.arp(s, y, n)


def ndcg10_x2(s, y, n):
    ev.ndcg(s, y, n, k=10)
    ev.ndcg(s, y, n, k=10)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="1024x128,16384x1000,64x20000")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    result = {"metrics": list(NINE), "unit": "us per batch", "shapes": {}}
    for shape in args.shapes.split(","):
        B, L = (int(v) for v in shape.split("x"))
        data = batches(B, L, dev)
        row = {
            "evaluate": time_region(lambda s, y, n: ev.evaluate(s, y, n, metrics=NINE), data, args.regions, args.warmup),
            "separate": time_region(separate, data, args.regions, args.warmup),
            "ndcg10_x2": time_region(ndcg10_x2, data, args.regions, args.warmup),
            "batches": len(data),
        }
        row["evaluate_below_ndcg10_x2"] = row["evaluate"] < row["ndcg10_x2"]
        result["shapes"][shape] = row
        del data
        torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
