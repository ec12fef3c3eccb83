"""The fused Linear step of the listwise losses against the three kernels it replaces.

Prints one JSON line: per shape (queries x list size x features, ragged n, int64 labels in [0, 5)) and loss (ListNet,
ListMLE), the median time in us of one training step's forward + backward, `loss.mean().backward()`:
  fused   -- FusedLinearLoss(F, loss=...): ltr_linear_listwise_partials_f32 (scores, loss row, weight-gradient row in
             one launch) and the cross-query reduction;
  pieces  -- LinearScorer(F, lazy=False) + the loss module: the streaming scorer, the listwise kernel, the row scale and
             the streaming weight gradient, with autograd between them -- the step before the fused kernel existed.
Each region is one call per batch of a rotating set larger than the 256 MiB last-level cache, timed by device events
around a synchronised region; the median of --regions regions after --warmup untimed ones.  Tie mode "index".

The kernel times of both come from a profiler run of this script, in a run of its own:
    rocprofv3 --kernel-trace --stats -- python scripts/bench_listwise_fused.py --regions 3
    python scripts/bench_listwise_fused.py [--regions 7] [--warmup 2] [--shapes 1024x128x136,...] [--max-batches 64]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorchltr_amd.fused import FusedLinearLoss, LinearScorer  # noqa: E402
from pytorchltr_amd.loss import ListMLELoss, ListwiseSoftmaxLoss  # noqa: E402
from pytorchltr_amd.utils import tie_breaking  # noqa: E402

CACHE_BYTES = 256 << 20


def batches(B, L, F, dev, max_batches, seed=0):
    """Enough (features, labels, n) batches that one pass over them streams more than the last-level cache."""
    per = B * L * (4 * F + 8) + B * 8
    count = min(max_batches, max(2, -(-(CACHE_BYTES + (32 << 20)) // per)))
    g = torch.Generator(device=dev).manual_seed(seed)
    out = []
    for _ in range(count):
        xs = torch.randn(B, L, F, device=dev, generator=g)
        y = torch.randint(0, 5, (B, L), device=dev, generator=g)
        n = torch.randint(1, L + 1, (B,), device=dev, generator=g)
        out.append((xs, y, n))
    return out


def time_region(fn, data, regions, warmup):
    """Median us per call of fn on one batch, from `regions` event-timed regions of len(data) calls each."""
    times = []
    for r in range(warmup + regions):
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for xs, y, n in data:
            fn(xs, y, n)
        stop.record()
        torch.cuda.synchronize()
        if r >= warmup:
            times.append(start.elapsed_time(stop) * 1000.0 / len(data))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="1024x128x136,16384x128x136,256x1000x220,64x4096x136")
    ap.add_argument("--max-batches", type=int, default=64)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    losses = {"listnet": ListwiseSoftmaxLoss(), "listmle": ListMLELoss()}
    result = {"unit": "us per step (forward + backward of loss.mean())", "shapes": {}}
    with tie_breaking("index"):
        for shape in args.shapes.split(","):
            B, L, F = (int(v) for v in shape.split("x"))
            data = batches(B, L, F, dev, args.max_batches)
            row = {"batches": len(data)}
            for name, loss_fn in losses.items():
                fused = FusedLinearLoss(F, loss=loss_fn).to(dev)
                scorer = LinearScorer(F, lazy=False).to(dev)

                def step_fused(xs, y, n):
                    fused(xs, y, n).mean().backward()
                    fused.weight.grad = fused.bias.grad = None

                def step_pieces(xs, y, n):
                    loss_fn(scorer(xs, n), y, n).mean().backward()
                    scorer.weight.grad = scorer.bias.grad = None

                row[name] = {"fused": round(time_region(step_fused, data, args.regions, args.warmup), 2),
                             "pieces": round(time_region(step_pieces, data, args.regions, args.warmup), 2)}
            result["shapes"][shape] = row
            del data
            torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
