"""The general fused Linear step on a bf16 feature batch (include/ltr_bf16_general.h; linear_loss_step(...,
bf16_general=True)) against what such a batch takes without the flag, in one process.

Prints one JSON line: per shape (queries x list size x features; n ~ U[1, L], random bf16 features, int64 labels in
[0, 5)) and loss kind, median times in us per call of fused.linear_loss_step (launch or pieces + the cross-query
reduction):
  general   -- bf16_general=True on the bf16 batch (`route`: what the flag reaches -- the shapes here are all off the
               register tile's plan);
  pieces    -- the same batch without the flag: ltr_linear_scores_bf16, the stand-alone loss, ltr_linear_grad_bf16;
  f32       -- the fp32 step on the batch upcast beforehand (the fp32 general / cluster / parts kernel);
  cast_f32  -- xs.float() and the fp32 step, the cast counted.
Cold, as scripts/bench_linear_bf16.py measures (its `batches` and `time_rotating`): one hipGraph replay per timed
region over a rotating set of batches whose bf16 copies alone exceed the last-level cache, between one pair of device
events; the median of --regions regions after --warmup untimed replays.  `graph`: false where a route could not be
captured and its calls were issued eagerly (host-bound on the small shapes).

    python scripts/bench_linear_bf16_general.py [--regions 9] [--warmup 2] [--shapes 1024x300x136,...] [--kinds hinge,...]
"""
import argparse
import json

import torch

from bench_linear_bf16 import batches, time_rotating
from pytorchltr_amd import fused

SHAPES = "1024x300x136,384x1000x224,2048x128x704,512x512x704,32x1000x224"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--kinds", default="hinge,logistic,ndcg2")
    ap.add_argument("--max-batches", type=int, default=32)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_linear_bf16_general: no GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    result = {"unit": "us per call, median of %d cold regions" % args.regions, "shapes": {}}
    for shape in args.shapes.split(","):
        B, L, F = (int(v) for v in shape.split("x"))
        data = batches(B, L, F, False, dev, args.max_batches)
        nbuf = len(data)
        F8 = data[0][0].shape[2]
        g = torch.Generator(device=dev).manual_seed(1)
        W = (torch.rand(F8, device=dev, generator=g) * 2 - 1) / F8 ** 0.5
        b = torch.zeros(1, device=dev)
        rec = {"batches": nbuf}
        for kind in args.kinds.split(","):
            code = fused._resolve_loss(kind)[0]
            step = {"route": fused._linear_routed("step", data[0][0], code, bf16_general=True)[0], "graph": {}}

            def call(i, col=0, cast=False, **kw):
                xs = data[i][col].float() if cast else data[i][col]
                return fused.linear_loss_step(xs, W, b, data[i][2], data[i][3], loss=kind, **kw)

            for name, fn in (("general", lambda i: call(i, bf16_general=True)), ("pieces", call),
                             ("f32", lambda i: call(i, col=1)), ("cast_f32", lambda i: call(i, cast=True))):
                step[name], step["graph"][name] = time_rotating(fn, nbuf, args.regions, args.warmup)
            for other in ("pieces", "f32", "cast_f32"):
                step[other + "_over_general"] = round(step[other] / step["general"], 2)
            rec[kind] = step
        result["shapes"][shape] = rec
        del data
        torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
