"""LambdaRankLoss forward + backward with and without a cutoff against LambdaNDCGLoss2, and the fused Linear step of
LambdaRankLoss against its three pieces.  The method of scripts/bench_listmle.py.

Prints one JSON line: per shape (queries x list size, ragged n, int64 labels in [0, 5)), the median time in us of
  lambdarank_k10 -- LambdaRankLoss(k=10)(s, y, n).sum().backward(): one HIP launch forward (ranking, the anchors' pairs),
                    one row scale backward;
  lambdarank     -- LambdaRankLoss(): the same kernel without a cutoff, every pair;
  ndcg2          -- LambdaNDCGLoss2(): the pairwise kernel of the reference's loss (every pair, no cutoff);
  call_k10, call -- ltr_lambdarank_f32 itself (loss and dscores into preallocated outputs, no autograd) with k = 10 and
                    without a cutoff: what is left of the rows above once the host's share is taken out;
and for the shape of --linear (queries x list size x features):
  fused          -- FusedLinearLoss(F, loss=LambdaRankLoss(k=10)) forward + backward: the one-launch step and the
                    cross-query reduction;
  pieces         -- LinearScorer(F, lazy=False) + LambdaRankLoss(k=10) + autograd: scorer, loss kernel, row scale,
                    weight-gradient kernel.
Each region is one pass over a rotating set of batches larger than the 256 MiB last-level cache (cold batches), timed
by device events around a synchronised region; the median of --regions regions after --warmup untimed ones.

    python scripts/bench_lambdarank.py [--regions 7] [--warmup 2] [--shapes 1024x128,256x1000,16384x128] [--linear 1024x128x136]
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
from pytorchltr_amd.fused import FusedLinearLoss, LinearScorer  # noqa: E402
from pytorchltr_amd.loss import LambdaNDCGLoss2, LambdaRankLoss  # noqa: E402

CACHE_BYTES = 256 << 20


def batches(B, L, dev, F=None, seed=0):
    """Enough (scores or features, labels, n) batches that one pass over them streams more than the last-level cache."""
    per = B * L * (4 * (F or 1) + 8) + B * 8
    count = max(2, -(-(CACHE_BYTES + (32 << 20)) // per))
    g = torch.Generator(device=dev).manual_seed(seed)
    out = []
    for _ in range(count):
        if F is None:
            x = torch.randn(B, L, device=dev, generator=g).requires_grad_(True)
        else:
            x = torch.randn(B, L, F, device=dev, generator=g)
        y = torch.randint(0, 5, (B, L), device=dev, generator=g)
        n = torch.randint(1, L + 1, (B,), device=dev, generator=g)
        out.append((x, y, n))
    return out


def time_region(fn, data, regions, warmup):
    """Median us per pass of fn over one batch, from `regions` event-timed regions of len(data) passes each."""
    times = []
    for r in range(warmup + regions):
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for x, y, n in data:
            fn(x, y, n)
        stop.record()
        torch.cuda.synchronize()
        if r >= warmup:
            times.append(start.elapsed_time(stop) * 1000.0 / len(data))
    return statistics.median(times)


def entry_point(k, B, L, dev):
    """ltr_lambdarank_f32 on a batch, outputs allocated once."""
    lib = _C.lib()
    loss = torch.empty(B, dtype=torch.float32, device=dev)
    ds = torch.empty(B, L, dtype=torch.float32, device=dev)

    def run(s, y, n):
        _C.check(lib.ltr_lambdarank_f32(s.data_ptr(), y.data_ptr(), _C.LABEL_I64, n.data_ptr(), k, 1.0, B, L,
                                        loss.data_ptr(), ds.data_ptr(), _C.stream_of(s)))
    return run


def warm_up(dev, seconds=1.0):
    """Device work for about `seconds` before anything is timed (clocks, allocator, code objects)."""
    data = batches(1024, 128, dev)[:8]
    fn = LambdaRankLoss(k=10)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for s, y, n in data:
            fn(s, y, n).sum().backward()
            s.grad = None
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="1024x128,256x1000,16384x128")
    ap.add_argument("--linear", default="1024x128x136")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    result = {"unit": "us per batch (forward + backward; call_*: one entry-point call)", "shapes": {}, "linear": {}}

    def fwd_bwd(fn):
        def run(s, y, n):
            fn(s, y, n).sum().backward()
            s.grad = None
        return run

    warm_up(dev)
    losses = (("lambdarank_k10", LambdaRankLoss(k=10)), ("lambdarank", LambdaRankLoss()), ("ndcg2", LambdaNDCGLoss2()))
    for shape in [s for s in args.shapes.split(",") if s]:
        B, L = (int(v) for v in shape.split("x"))
        data = batches(B, L, dev)
        row = {name: time_region(fwd_bwd(fn), data, args.regions, args.warmup) for name, fn in losses}
        row["call_k10"] = time_region(entry_point(10, B, L, dev), data, args.regions, args.warmup)
        row["call"] = time_region(entry_point(0, B, L, dev), data, args.regions, args.warmup)
        row["batches"] = len(data)
        row["lambdarank_over_k10"] = round(row["lambdarank"] / row["lambdarank_k10"], 2)
        row["ndcg2_over_k10"] = round(row["ndcg2"] / row["lambdarank_k10"], 2)
        result["shapes"][shape] = row
        del data
        torch.cuda.empty_cache()

    if args.linear:
        B, L, F = (int(v) for v in args.linear.split("x"))
        data = batches(B, L, dev, F=F)
        loss_fn = LambdaRankLoss(k=10)
        fused = FusedLinearLoss(F, loss=loss_fn).to(dev)
        scorer = LinearScorer(F, lazy=False).to(dev)
        scorer.load_state_dict(fused.state_dict())

        def run_fused(x, y, n):
            fused(x, y, n).sum().backward()
            fused.zero_grad(set_to_none=True)

        def run_pieces(x, y, n):
            loss_fn(scorer(x, n), y, n).sum().backward()
            scorer.zero_grad(set_to_none=True)

        row = {"fused": time_region(run_fused, data, args.regions, args.warmup),
               "pieces": time_region(run_pieces, data, args.regions, args.warmup), "batches": len(data)}
        row["pieces_over_fused"] = round(row["pieces"] / row["fused"], 2)
        result["linear"][args.linear] = row
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
