"""ListMLELoss forward + backward against a torch composition of the same definition, ListNet and ndcg@10.

Prints one JSON line: per shape (queries x list size, ragged n, int64 labels in [0, 5)), the median time in us of
  listmle       -- ListMLELoss()(s, y, n).sum().backward(): one HIP launch forward (two past 4096 documents: the sort
                   and its epilogues), one row scale backward;
  listmle_fwd   -- the forward alone, on scores that require grad: loss AND dscores, the same kernel work as above;
  torch         -- the same loss as a torch program: stable argsort of the labels, gather, logcumsumexp on the flipped
                   list, masking, autograd;
  listnet       -- ListwiseSoftmaxLoss forward + backward;
  ndcg10        -- ndcg(k=10), one ranking and an O(n) pass: what the one-workgroup path is expected to stay within
                   about 1.5x of.
Each region is R calls, one per batch of a rotating set larger than the 256 MiB last-level cache, timed by device
events around a synchronised region; the median of --regions regions after --warmup untimed ones.  Default tie mode
("random"): every call draws its seed on the host, as a user's call does.

    python scripts/bench_listmle.py [--regions 7] [--warmup 2] [--shapes 1024x128,16384x128,256x1000,64x20000,4x200000]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytorchltr_amd.evaluation as ev  # noqa: E402
from pytorchltr_amd.loss import ListMLELoss, ListwiseSoftmaxLoss  # noqa: E402

CACHE_BYTES = 256 << 20


def batches(B, L, dev, seed=0):
    """Enough (scores, labels, n) batches that one pass over them streams more than the last-level cache."""
    per = B * L * (4 + 8) + B * 8
    count = max(2, -(-(CACHE_BYTES + (32 << 20)) // per))
    g = torch.Generator(device=dev).manual_seed(seed)
    out = []
    for _ in range(count):
        s = torch.randn(B, L, device=dev, generator=g).requires_grad_(True)
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


def torch_listmle(s, y, n):
    """ListMLE as plain torch (index ties among equal labels): the reference point a user would otherwise write."""
    L = s.shape[1]
    pos = torch.arange(L, device=s.device).unsqueeze(0)
    real = pos < n.unsqueeze(1)
    key = torch.where(real, y.float(), torch.full_like(s, -math.inf))
    pi = torch.sort(key, dim=1, descending=True, stable=True).indices
    x = torch.where(real, torch.gather(s, 1, pi), torch.full_like(s, -math.inf))
    lse = torch.flip(torch.logcumsumexp(torch.flip(x, [1]), 1), [1])
    return torch.where(real, lse - torch.where(real, x, torch.zeros_like(x)), torch.zeros_like(x)).sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="1024x128,16384x128,256x1000,64x20000,4x200000")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    mle, listnet = ListMLELoss(), ListwiseSoftmaxLoss()
    result = {"unit": "us per batch (forward + backward; ndcg10 forward)", "shapes": {}}

    def fwd_bwd(fn):
        def run(s, y, n):
            fn(s, y, n).sum().backward()
            s.grad = None
        return run

    for shape in args.shapes.split(","):
        B, L = (int(v) for v in shape.split("x"))
        data = batches(B, L, dev)
        row = {
            "listmle": time_region(fwd_bwd(mle), data, args.regions, args.warmup),
            "listmle_fwd": time_region(mle, data, args.regions, args.warmup),
            "torch": time_region(fwd_bwd(torch_listmle), data, args.regions, args.warmup),
            "listnet": time_region(fwd_bwd(listnet), data, args.regions, args.warmup),
            "ndcg10": time_region(lambda s, y, n: ev.ndcg(s.detach(), y, n, k=10), data, args.regions, args.warmup),
            "batches": len(data),
        }
        row["listmle_fwd_over_ndcg10"] = round(row["listmle_fwd"] / row["ndcg10"], 2)
        row["torch_over_listmle"] = round(row["torch"] / row["listmle"], 2)
        result["shapes"][shape] = row
        del data
        torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
