"""The fused MLP step on a bf16 feature batch (include/ltr_mlp_step_bf16.h) against what it replaces, in one process,
by the method of scripts/bench_mlp_bf16.py.

Prints one JSON line: per shape (queries x list size x features, n ~ U[1, L], random features, int64 labels in [0, 5))
and per loss (hinge; LambdaRank k = 10), with the guide's network Linear(F, 50) / ReLU / Linear(50, 10) / ReLU /
Linear(10, 1), the median time in us of one `mlp_loss_step` / `mlp_lambdarank_step` call in three modes:
  fused_bf16 -- fuse_bf16=True on the bf16 batch: one bf16-MFMA launch plus the reduction (ltr_mlp_step_bf16);
  pieces     -- the same call without the flag on the same bf16 batch: the bf16 score kernel, the stand-alone loss
                kernel with autograd, the bf16 gradient kernel -- the baseline the flag replaces;
  f32        -- the fp32 one-launch step on the same batch upcast beforehand (outside the timed region).
Each region is one call per batch of a rotating set whose bf16 copy alone is larger than the 256 MiB last-level cache,
timed by device events around a synchronised region; the median of --regions regions after --warmup untimed ones.

    python scripts/bench_mlp_bf16_step.py [--regions 7] [--warmup 2] [--shapes 1024x128x136,16384x128x136]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_listwise_fused import time_region  # noqa: E402
from bench_mlp_bf16 import HIDDEN, batches  # noqa: E402
from pytorchltr_amd import fused  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="1024x128x136,16384x128x136")
    ap.add_argument("--max-batches", type=int, default=64)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    result = {"unit": "us, median", "hidden": list(HIDDEN), "shapes": {}}
    for shape in args.shapes.split(","):
        B, L, F = (int(v) for v in shape.split("x"))
        data = batches(B, L, F, dev, args.max_batches)
        params = [p.detach() for p in fused.FusedMLPLoss(F, "hinge", hidden=HIDDEN).to(dev)._params()]
        steps = {
            "hinge": lambda xs, y, n, **kw: fused.mlp_loss_step(xs, params, y, n, "hinge", **kw),
            "lambdarank_k10": lambda xs, y, n, **kw: fused.mlp_lambdarank_step(xs, params, y, n, k=10, **kw),
        }
        row = {"batches": len(data)}
        for name, step in steps.items():
            bf16 = [(xb, y, n) for xb, _, y, n in data]
            f32 = [(xf, y, n) for _, xf, y, n in data]
            t = {
                "fused_bf16": time_region(lambda xs, y, n: step(xs, y, n, fuse_bf16=True), bf16, args.regions, args.warmup),
                "pieces": time_region(step, bf16, args.regions, args.warmup),
                "f32": time_region(step, f32, args.regions, args.warmup),
            }
            row[name] = {k: round(v, 2) for k, v in t.items()}
            row[name]["pieces_over_fused"] = round(t["pieces"] / t["fused_bf16"], 2)
            row[name]["f32_over_fused"] = round(t["f32"] / t["fused_bf16"], 2)
        result["shapes"][shape] = row
        del data
        torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
