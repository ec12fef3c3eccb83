"""The fused MLP step of the listwise losses against the pieces it replaces.

Prints one JSON line: per shape (queries x list size x features, ragged n, int64 labels in [0, 5)) and loss (ListNet,
ListMLE), the median time in us of one training step's forward + backward, `loss.backward()` of the mean loss, of the
guide's network Linear(F, 50) / ReLU / Linear(50, 10) / ReLU / Linear(10, 1):
  fused   -- FusedMLPListwiseLoss(F, loss=...): ltr_mlp_listwise_f32 (network, loss row and backward in one launch) and
             the cross-workgroup reduction; `fused_path` says whether the plan took the shape (else the module itself
             runs the pieces);
  pieces  -- the three nn.Linear layers (rocBLAS), the stand-alone listwise loss kernel and torch's autograd.
Each region is one call per batch of a rotating set larger than the 256 MiB last-level cache, timed by device events
around a synchronised region; the median of --regions regions after --warmup untimed ones.  Tie mode "index".
--pairwise adds FusedMLPLoss(F, "logistic") on the same batches, the pairwise instantiation of the same kernels.

The kernel times come from a profiler run of this script, in a run of its own:
    rocprofv3 --kernel-trace --stats -- python scripts/bench_mlp_listwise.py --regions 3 --pairwise
    python scripts/bench_mlp_listwise.py [--regions 7] [--warmup 2] [--shapes 1024x128x136,...] [--max-batches 64]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_listwise_fused import batches, time_region  # noqa: E402
from pytorchltr_amd.fused import FusedMLPListwiseLoss, FusedMLPLoss  # noqa: E402
from pytorchltr_amd.loss import ListMLELoss, ListwiseSoftmaxLoss  # noqa: E402
from pytorchltr_amd.utils import tie_breaking  # noqa: E402

HIDDEN = (50, 10)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="1024x128x136,16384x128x136,1024x256x136,1024x128x220")
    ap.add_argument("--max-batches", type=int, default=64)
    ap.add_argument("--pairwise", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    losses = {"listnet": ListwiseSoftmaxLoss(), "listmle": ListMLELoss()}
    result = {"unit": "us per step (forward + backward of the mean loss)", "hidden": list(HIDDEN), "shapes": {}}
    with tie_breaking("index"):
        for shape in args.shapes.split(","):
            B, L, F = (int(v) for v in shape.split("x"))
            data = batches(B, L, F, dev, args.max_batches)
            row = {"batches": len(data)}

            def timed(module):
                def step(xs, y, n):
                    module(xs, y, n).backward()
                    for p in module.parameters():
                        p.grad = None
                return round(time_region(step, data, args.regions, args.warmup), 2)

            for name, loss_fn in losses.items():
                fused = FusedMLPListwiseLoss(F, loss=loss_fn, hidden=HIDDEN).to(dev)

                def step_pieces(xs, y, n):
                    loss_fn(fused.score(xs), y, n).mean().backward()
                    for p in fused.parameters():
                        p.grad = None

                row[name] = {"fused": timed(fused),
                             "pieces": round(time_region(step_pieces, data, args.regions, args.warmup), 2),
                             "fused_path": bool(fused._fused_shape(B, L, (F + 3) & ~3))}
            if args.pairwise:
                row["logistic"] = {"fused": timed(FusedMLPLoss(F, "logistic", hidden=HIDDEN).to(dev))}
            result["shapes"][shape] = row
            del data
            torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
