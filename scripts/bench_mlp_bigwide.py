"""The K-streamed MLP scorer kernels for wide hidden layers on wide rows (include/ltr_mlp_bigwide.h) against the torch
layers they replace, at hidden sizes (128, 32) and (256, 64) on Istella's and Yahoo's widths.

Prints one JSON line: per hidden size and shape (queries x list size x features, ragged n ~ U[1, L], int64 labels in
[0, 5)), times in us, one process, cold batches:
  scores      -- `model.score(xs, n)` under torch.no_grad(): `bigwide` = the module with big_hidden_wide=True
                 (ltr_mlp_bigwide_scores_f32), `torch` = the same module with the flag off (the three nn.Linear layers);
  hinge_step  -- FusedMLPLoss(F, "hinge") forward + backward of the mean loss: `bigwide` = the scores, the stand-alone
                 loss kernel, the two gradient kernels + reductions; `torch` = flag off: the torch layers, the same loss
                 kernel, autograd; medians, and `torch_max` = the slowest region of the torch side;
  kernels     -- the entry points on their own (fused.mlp_bigwide_scores; fused.mlp_bigwide_grad) and their share of the
                 155 TFLOP/s f32 MFMA peak, counting the FLOPs of the real rows at the network's own sizes.
Regions, batches and the interleaving (on, off, on, off, ...) are those of scripts/bench_mlp_big.py.

    python scripts/bench_mlp_bigwide.py [--regions 7] [--warmup 2] [--shapes 1024x200x220,...] [--max-batches 64]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_listwise_fused import batches, time_region  # noqa: E402
from bench_mlp_big import row_flops  # noqa: E402
from bench_mlp_rows import PEAK_F32_MFMA  # noqa: E402
from pytorchltr_amd import fused  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="1024x200x220,512x512x700")
    ap.add_argument("--hidden", default="128x32,256x64")
    ap.add_argument("--max-batches", type=int, default=64)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    result = {"unit": "us, median", "shapes": {}}
    for shape in args.shapes.split(","):
        B, L, F = (int(v) for v in shape.split("x"))
        data = batches(B, L, F, dev, args.max_batches)
        real = sum(int(n.clamp(0, L).sum()) for _, _, n in data) / len(data)
        gs = [torch.randn(B, L, device=dev) for _ in data]
        for hidden in args.hidden.split(","):
            H1, H2 = (int(v) for v in hidden.split("x"))
            module = fused.FusedMLPLoss(F, "hinge", hidden=(H1, H2)).to(dev)
            params = [p.detach() for p in module._params()]

            def score(xs, y, n):
                with torch.no_grad():
                    module.score(xs, n)

            def step(xs, y, n):
                module(xs, y, n).backward()
                for p in module.parameters():
                    p.grad = None

            row = {"batches": len(data), "real_rows": round(real)}
            for name, fn in (("scores", score), ("hinge_step", step)):
                times = {True: [], False: []}
                for r in range(args.warmup + args.regions):        # one region a side, alternating
                    for flag in (True, False):
                        module.big_hidden_wide = flag
                        t = time_region(fn, data, 1, 0)
                        if r >= args.warmup:
                            times[flag].append(t)
                row[name] = {"bigwide": round(statistics.median(times[True]), 2),
                             "torch": round(statistics.median(times[False]), 2), "torch_max": round(max(times[False]), 2)}
            it = iter(range(1 << 30))
            k_scores = round(time_region(lambda xs, y, n: fused.mlp_bigwide_scores(xs, params, n), data, args.regions,
                                         args.warmup), 2)
            k_grad = round(time_region(lambda xs, y, n: fused.mlp_bigwide_grad(xs, params, gs[next(it) % len(gs)], n),
                                       data, args.regions, args.warmup), 2)
            f_fwd, f_grad = row_flops(F, H1, H2)
            row["kernels"] = {"scores": k_scores, "grad_and_reduce": k_grad,
                              "scores_share_of_peak": round(real * f_fwd / (k_scores * 1e-6) / PEAK_F32_MFMA, 3),
                              "grad_share_of_peak": round(real * f_grad / (k_grad * 1e-6) / PEAK_F32_MFMA, 3)}
            result["shapes"]["%s h%s" % (shape, hidden)] = row
        del data, gs
        torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
