"""MLPTrainer.step against the loop body it replaces.

Prints one JSON line: per shape (queries x list size x features, ragged n, int64 labels in [0, 5)) and loss (hinge:
FusedMLPLoss; lambdarank: FusedMLPLambdaRankLoss(k = 10)), the median time in us of one WHOLE training step of the
guide's network Linear(F, 50) / ReLU / Linear(50, 10) / ReLU / Linear(10, 1) with Adagrad (lr 0.1), four ways in one
process, each on a model of its own with the same initial parameters:
  a_eager_autograd    -- the loop body of examples/02_mlp_getting_started.py: loss = model(xs, ys, n); zero_grad();
                         loss.backward(); torch.optim.Adagrad.step()
  b_graphed_autograd  -- the same under pytorchltr_amd.graphed.GraphedStep (capturable=True where this torch's Adagrad
                         has the switch; without it the step count stays on the host, which lr_decay = 0 never reads)
  c_trainer_eager     -- MLPTrainer.step: the MFMA launch and the reduce-and-update launch, no autograd
  d_trainer_graphed   -- MLPTrainer.graphed: those two launches replayed
The two graphed modes copy every batch into their static buffers, as GraphedStep does; that copy is inside their time.
Each region is one call per batch of a rotating set larger than the 256 MiB last-level cache, timed by device events
around a synchronised region; the median of --regions regions after --warmup untimed ones.

The kernel times and the launches per step come from a profiler run of this script, in a run of its own:
    rocprofv3 --kernel-trace --stats -- python scripts/bench_mlp_train.py --regions 2 --warmup 1 --shapes 1024x128x136 --losses hinge
    python scripts/bench_mlp_train.py [--regions 7] [--warmup 2] [--shapes 1024x128x136,16384x128x136] [--losses hinge,lambdarank]
"""
import argparse
import inspect
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_listwise_fused import batches, time_region  # noqa: E402
from pytorchltr_amd.fused import FusedMLPLambdaRankLoss, FusedMLPLoss, MLPTrainer  # noqa: E402
from pytorchltr_amd.graphed import GraphedStep  # noqa: E402

HIDDEN = (50, 10)
LR = 0.1


def make_model(loss, F, dev, like=None):
    model = (FusedMLPLoss(F, "hinge", hidden=HIDDEN) if loss == "hinge"
             else FusedMLPLambdaRankLoss(F, k=10, hidden=HIDDEN)).to(dev)
    if like is not None:
        model.load_state_dict(like.state_dict())
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="1024x128x136,16384x128x136")
    ap.add_argument("--losses", default="hinge,lambdarank")
    ap.add_argument("--max-batches", type=int, default=64)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    result = {"unit": "us per training step (loss, gradients and the Adagrad update)", "hidden": list(HIDDEN),
              "optimizer": "adagrad lr=%g" % LR,
              "adagrad_capturable": "capturable" in inspect.signature(torch.optim.Adagrad.__init__).parameters, "shapes": {}}
    for shape in args.shapes.split(","):
        B, L, F = (int(v) for v in shape.split("x"))
        data = batches(B, L, F, dev, args.max_batches)
        row = {"batches": len(data)}
        for loss in args.losses.split(","):
            first = make_model(loss, F, dev)
            # (a) the parent's loop body, eager
            model_a = make_model(loss, F, dev, first)
            opt_a = torch.optim.Adagrad(model_a.parameters(), lr=LR)

            def step_a(xs, y, n):
                out = model_a(xs, y, n)
                opt_a.zero_grad()
                out.backward()
                opt_a.step()

            times = {"a_eager_autograd": time_region(step_a, data, args.regions, args.warmup)}
            # (b) the same, captured
            model_b = make_model(loss, F, dev, first)
            capturable = "capturable" in inspect.signature(torch.optim.Adagrad.__init__).parameters
            opt_b = torch.optim.Adagrad(model_b.parameters(), lr=LR, **({"capturable": True} if capturable else {}))
            step_b = GraphedStep(model_b, opt_b, lambda xs, y, n: model_b(xs, y, n), example_batch=data[0])
            times["b_graphed_autograd"] = time_region(lambda xs, y, n: step_b(xs, y, n), data, args.regions, args.warmup)
            del step_b
            # (c) the trainer, eager
            trainer_c = MLPTrainer(make_model(loss, F, dev, first), "adagrad", lr=LR)
            times["c_trainer_eager"] = time_region(lambda xs, y, n: trainer_c.step(xs, y, n), data, args.regions,
                                                   args.warmup)
            # (d) the trainer, captured
            trainer_d = MLPTrainer(make_model(loss, F, dev, first), "adagrad", lr=LR)
            step_d = trainer_d.graphed(data[0])
            times["d_trainer_graphed"] = time_region(lambda xs, y, n: step_d(xs, y, n), data, args.regions, args.warmup)
            del step_d
            row[loss] = {k: round(v, 2) for k, v in times.items()}
            row[loss]["fused_path"] = bool(first._fused_shape(B, L, (F + 3) & ~3))
            torch.cuda.empty_cache()
        result["shapes"][shape] = row
        del data
        torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
