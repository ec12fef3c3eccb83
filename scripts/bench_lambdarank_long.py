"""ltr_lambdarank_long_f32 (LambdaRank past 4096 documents) with NDCG@10 and without a cutoff, next to
ltr_pairwise_loss_long_f32(LTR_NDCG2) on the same batches -- the other NDCG-weighted loss at these lengths -- and, at
the hand-over point, the long path forced onto 4096 documents against ltr_lambdarank_f32.  The method of
scripts/bench_lambdarank.py.

Prints one JSON line: per shape (queries x list size, ragged n, int64 labels in [0, 5)), the median time in us of one
entry-point call with loss, dscores and workspace allocated once:
  long_k10  -- ltr_lambdarank_long_f32, k = 10: two sorts, the by-rank arrays, about K n pair evaluations;
  long      -- the same without a cutoff: n^2 pair evaluations;
  ndcg2     -- ltr_pairwise_loss_long_f32(LTR_NDCG2): n^2 pair evaluations, every pair twice;
and for --handover (queries x list size <= 4096):
  forced_k10 -- ltr_lambdarank_long_f32 under ltr_debug_lambdarank_long_all, k = 10;
  short_k10  -- ltr_lambdarank_f32, k = 10.
Each region is one pass over a rotating set of batches larger than the 256 MiB last-level cache (cold batches), timed
by device events around a synchronised region; the median of --regions regions after --warmup untimed ones.  Run it
twice and compare the two lines before relying on a number.

    python scripts/bench_lambdarank_long.py [--regions 5] [--warmup 1] [--shapes 64x8192,16x65536,256x5000]
                                            [--handover 1024x4096] [--only long_k10] [--warm-seconds 1]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorchltr_amd import _C  # noqa: E402

CACHE_BYTES = 256 << 20


def batches(B, L, dev, seed=0):
    """Enough (scores, labels, n) batches that one pass over them streams more than the last-level cache."""
    per = B * L * 12 + B * 8
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


def lambdarank_long(k, B, L, dev):
    lib = _C.lib()
    loss = torch.empty(B, dtype=torch.float32, device=dev)
    ds = torch.empty(B, L, dtype=torch.float32, device=dev)
    ws, nbytes = _C.workspace(lib.ltr_lambdarank_long_workspace_bytes(k, B, L), dev)

    def run(s, y, n):
        _C.check(lib.ltr_lambdarank_long_f32(s.data_ptr(), y.data_ptr(), _C.LABEL_I64, n.data_ptr(), k, 1.0, B, L,
                                             loss.data_ptr(), ds.data_ptr(), _C.ptr(ws), nbytes, _C.stream_of(s)))
    return run


def lambdarank_short(k, B, L, dev):
    lib = _C.lib()
    loss = torch.empty(B, dtype=torch.float32, device=dev)
    ds = torch.empty(B, L, dtype=torch.float32, device=dev)

    def run(s, y, n):
        _C.check(lib.ltr_lambdarank_f32(s.data_ptr(), y.data_ptr(), _C.LABEL_I64, n.data_ptr(), k, 1.0, B, L,
                                        loss.data_ptr(), ds.data_ptr(), _C.stream_of(s)))
    return run


def ndcg2_long(B, L, dev):
    lib = _C.lib()
    loss = torch.empty(B, dtype=torch.float32, device=dev)
    ds = torch.empty(B, L, dtype=torch.float32, device=dev)
    ws, nbytes = _C.workspace(lib.ltr_pairwise_loss_long_workspace_bytes(_C.NDCG2, B, L), dev)

    def run(s, y, n):
        _C.check(lib.ltr_pairwise_loss_long_f32(_C.NDCG2, 1.0, s.data_ptr(), y.data_ptr(), _C.LABEL_I64, n.data_ptr(), B, L,
                                                loss.data_ptr(), ds.data_ptr(), _C.ptr(ws), nbytes, _C.stream_of(s)))
    return run


def warm_up(dev, seconds=1.0):
    """Device work for about `seconds` before anything is timed (clocks, allocator, code objects)."""
    data = batches(8, 8192, dev)[:4]
    fn = lambdarank_long(10, 8, 8192, dev)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for s, y, n in data:
            fn(s, y, n)
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default="64x8192,16x65536,256x5000")
    ap.add_argument("--handover", default="1024x4096")
    ap.add_argument("--only", default="", help="comma-separated row names; the others are left out (a profiler run)")
    ap.add_argument("--warm-seconds", type=float, default=1.0, help="device work before anything is timed (0: a profiler run)")
    args = ap.parse_args()
    only = {v for v in args.only.split(",") if v}
    dev = torch.device("cuda:0")
    result = {"unit": "us per entry-point call (loss and dscores, preallocated outputs and workspace)", "shapes": {},
              "handover": {}}
    if args.warm_seconds > 0:
        warm_up(dev, args.warm_seconds)
    for shape in [s for s in args.shapes.split(",") if s]:
        B, L = (int(v) for v in shape.split("x"))
        data = batches(B, L, dev)
        row = {}
        for name, make in (("long_k10", lambda: lambdarank_long(10, B, L, dev)), ("long", lambda: lambdarank_long(0, B, L, dev)),
                           ("ndcg2", lambda: ndcg2_long(B, L, dev))):
            if not only or name in only:
                row[name] = time_region(make(), data, args.regions, args.warmup)
        row["batches"] = len(data)
        if "long_k10" in row and "ndcg2" in row:
            row["ndcg2_over_long_k10"] = round(row["ndcg2"] / row["long_k10"], 1)
        result["shapes"][shape] = row
        del data
        torch.cuda.empty_cache()

    if args.handover and not only:
        B, L = (int(v) for v in args.handover.split("x"))
        data = batches(B, L, dev)
        lib = _C.lib()
        row = {"short_k10": time_region(lambdarank_short(10, B, L, dev), data, args.regions, args.warmup)}
        prev = lib.ltr_debug_lambdarank_long_all(1)
        try:
            row["forced_k10"] = time_region(lambdarank_long(10, B, L, dev), data, args.regions, args.warmup)
        finally:
            lib.ltr_debug_lambdarank_long_all(prev)
        row["batches"] = len(data)
        row["forced_over_short"] = round(row["forced_k10"] / row["short_k10"], 2)
        result["handover"][args.handover] = row
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
