"""The fused MLP step of LambdaRankLoss against the path it replaces.

Prints one JSON line: per shape (queries x list size x features, ragged n, int64 labels in [0, 5)) and cutoff, the
median time in us of one training step's forward + backward, `loss.backward()` of the mean loss, of the guide's network
Linear(F, 50) / ReLU / Linear(50, 10) / ReLU / Linear(10, 1):
  fused   -- FusedMLPLambdaRankLoss(F, k=...): ltr_mlp_lambdarank_f32 (network, LambdaRank row and backward in one
             launch) and the cross-workgroup reduction; `fused_path` says whether the plan took the shape (else the
             module itself runs the pieces);
  pieces  -- what users ran before it: MLPScorer(F) (the row score kernel), LambdaRankLoss(k) (the stand-alone kernel)
             and autograd (the row gradient kernel), on the same parameters and the same batches.
Each region is one call per batch of a rotating set larger than the 256 MiB last-level cache, timed by device events
around a synchronised region; the median of --regions regions after --warmup untimed ones.  The first shape runs at
k = 10 and without a cutoff ("none"), the others at k = 10.

The kernel times come from a profiler run of this script, in a run of its own:
    rocprofv3 --kernel-trace --stats -- python scripts/bench_mlp_lambdarank.py --regions 3 --cutoffs 10 --shapes 1024x128x136
    python scripts/bench_mlp_lambdarank.py [--regions 7] [--warmup 2] [--shapes 1024x128x136,...] [--max-batches 64]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_listwise_fused import batches, time_region  # noqa: E402
from pytorchltr_amd.fused import FusedMLPLambdaRankLoss, MLPScorer  # noqa: E402
from pytorchltr_amd.loss import LambdaRankLoss  # noqa: E402

HIDDEN = (50, 10)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="1024x128x136,16384x128x136,1024x256x136,1024x128x220")
    ap.add_argument("--max-batches", type=int, default=64)
    ap.add_argument("--cutoffs", default=None, help="e.g. 10 or 10,none for every shape (a profiler run of one cutoff)")
    args = ap.parse_args()
    cutoffs = None if args.cutoffs is None else [None if c == "none" else int(c) for c in args.cutoffs.split(",")]
    dev = torch.device("cuda:0")
    result = {"unit": "us per step (forward + backward of the mean loss)", "hidden": list(HIDDEN), "shapes": {}}
    for i, shape in enumerate(args.shapes.split(",")):
        B, L, F = (int(v) for v in shape.split("x"))
        data = batches(B, L, F, dev, args.max_batches)
        row = {"batches": len(data)}
        for k in (cutoffs if cutoffs is not None else (10, None) if i == 0 else (10,)):
            fused = FusedMLPLambdaRankLoss(F, k=k, hidden=HIDDEN).to(dev)
            scorer = MLPScorer(F, hidden=HIDDEN).to(dev)
            scorer.load_state_dict(fused.state_dict())
            loss_fn = LambdaRankLoss(k=k)

            def step_fused(xs, y, n):
                fused(xs, y, n).backward()
                for p in fused.parameters():
                    p.grad = None

            def step_pieces(xs, y, n):
                loss_fn(scorer(xs, n), y, n).mean().backward()
                for p in scorer.parameters():
                    p.grad = None

            row["k=%s" % (k or "none")] = {
                "fused": round(time_region(step_fused, data, args.regions, args.warmup), 2),
                "pieces": round(time_region(step_pieces, data, args.regions, args.warmup), 2),
                "fused_path": bool(fused._fused_shape(B, L, (F + 3) & ~3))}
        result["shapes"][shape] = row
        del data
        torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
