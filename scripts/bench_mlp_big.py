"""The MLP scorer kernels for wide hidden layers (include/ltr_mlp_big.h) against the torch layers they replace, at hidden
sizes (128, 32) and (256, 64).

Prints one JSON line: per hidden size and shape (queries x list size x features, ragged n ~ U[1, L], int64 labels in
[0, 5)), median times in us, one process, cold batches:
  scores      -- `model.score(xs, n)` under torch.no_grad(): `big` = the module built with big_hidden=True
                 (ltr_mlp_big_scores_f32), `torch` = the same module with the flag off (the three nn.Linear layers);
  hinge_step  -- FusedMLPLoss(F, "hinge") forward + backward of the mean loss: `big` = big scores, the stand-alone loss
                 kernel, the big gradient + reduction; `torch` = flag off: the torch layers, the same loss kernel, autograd;
  kernels     -- the entry points on their own (fused.mlp_big_scores; fused.mlp_big_grad) and their share of the
                 155 TFLOP/s f32 MFMA peak, counting the FLOPs of the real rows at the network's own sizes.
Each region is one call per batch of a rotating set larger than the 256 MiB last-level cache, timed by device events
around a synchronised region; the median of --regions regions after --warmup untimed ones.  Flag on and flag off are
interleaved region by region (on, off, on, off, ...), so clock and thermal drift fall on both sides alike.

    python scripts/bench_mlp_big.py [--regions 7] [--warmup 2] [--shapes 1024x128x136,...] [--max-batches 64]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_listwise_fused import batches, time_region  # noqa: E402
from bench_mlp_rows import PEAK_F32_MFMA  # noqa: E402
from pytorchltr_amd import fused  # noqa: E402


def row_flops(F, H1, H2):
    """(forward, forward + backward) FLOPs of one row: the backward recomputes the forward and adds dW1, dH1, dW2."""
    fwd = 2 * (F * H1 + H1 * H2 + H2)
    return fwd, fwd + 2 * (F * H1 + 2 * H1 * H2 + H2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="1024x128x136,16384x128x136,256x1000x136")
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

            def timed(fn):
                return round(time_region(fn, data, args.regions, args.warmup), 2)

            def score(xs, y, n):
                with torch.no_grad():
                    module.score(xs, n)

            def step(xs, y, n):
                module(xs, y, n).backward()
                for p in module.parameters():
                    p.grad = None

            row = {"batches": len(data), "real_rows": round(real), "scores": {}, "hinge_step": {}}
            for name, fn in (("scores", score), ("hinge_step", step)):
                times = {True: [], False: []}
                for r in range(args.warmup + args.regions):        # one region a side, alternating
                    for flag in (True, False):
                        module.big_hidden = flag
                        t = time_region(fn, data, 1, 0)
                        if r >= args.warmup:
                            times[flag].append(t)
                row[name] = {"big": round(statistics.median(times[True]), 2),
                             "torch": round(statistics.median(times[False]), 2)}
            it = iter(range(1 << 30))
            k_scores = timed(lambda xs, y, n: fused.mlp_big_scores(xs, params, n))
            k_grad = timed(lambda xs, y, n: fused.mlp_big_grad(xs, params, gs[next(it) % len(gs)], n))
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
