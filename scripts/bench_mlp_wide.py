"""The wide-row MLP scorer kernels (include/ltr_mlp_wide.h) against the torch layers they replace at 228 .. 704 features.

Prints one JSON line: per shape (queries x list size x features, ragged n ~ U[1, L], int64 labels in [0, 5)), with the
guide's network Linear(F, 50) / ReLU / Linear(50, 10) / ReLU / Linear(10, 1), median times in us:
  scores      -- (a) `model.score(xs, n)` under torch.no_grad(): `wide` = ltr_mlp_wide_scores_f32, `torch` = the three
                 nn.Linear layers (rocBLAS), the route before the wide kernels;
  hinge_step  -- (b) FusedMLPLoss(F, "hinge") forward + backward of the mean loss: `wide` = wide scores, the stand-alone
                 loss kernel, the wide gradient (two kernels + two reductions); `torch` = the torch layers, the same
                 loss kernel and torch's autograd, written out: `bench_mlp_rows.torch_step`;
  kernels     -- (c) the entry points on their own (fused.mlp_wide_scores; fused.mlp_wide_grad) and their share of the
                 155 TFLOP/s f32 MFMA peak, counting the FLOPs of the real rows at the padded tile sizes
                 (16-feature steps x 64 x 16), and the score kernel's feature bytes per second.
Each region is one call per batch of a rotating set larger than the 256 MiB last-level cache, timed by device events
around a synchronised region; the median of --regions regions after --warmup untimed ones.

    python scripts/bench_mlp_wide.py [--regions 7] [--warmup 2] [--shapes 512x512x700,...] [--max-batches 64]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_listwise_fused import batches, time_region  # noqa: E402
from bench_mlp_rows import HIDDEN, PEAK_F32_MFMA, row_flops, torch_scores, torch_step  # noqa: E402
from pytorchltr_amd import fused  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="512x512x700,256x1000x700,1024x128x700,1024x300x452")
    ap.add_argument("--max-batches", type=int, default=64)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    result = {"unit": "us, median", "hidden": list(HIDDEN), "shapes": {}}
    for shape in args.shapes.split(","):
        B, L, F = (int(v) for v in shape.split("x"))
        if not fused._mlp_wide_network(F, *HIDDEN):
            raise SystemExit("%s: the wide kernels are routed 228 .. 704 features, a multiple of 4" % shape)
        data = batches(B, L, F, dev, args.max_batches)
        real = sum(int(n.clamp(0, L).sum()) for _, _, n in data) / len(data)
        module = fused.FusedMLPLoss(F, "hinge", hidden=HIDDEN).to(dev)
        params = [p.detach() for p in module._params()]
        gs = [torch.randn(B, L, device=dev) for _ in data]

        def timed(fn):
            return round(time_region(fn, data, args.regions, args.warmup), 2)

        def score(xs, y, n):
            with torch.no_grad():
                module.score(xs, n)

        def score_torch(xs, y, n):
            with torch.no_grad():
                torch_scores(module, xs)

        def step(xs, y, n):
            module(xs, y, n).backward()
            for p in module.parameters():
                p.grad = None

        row = {"batches": len(data), "real_rows": round(real)}
        # (a) scores under no_grad, (b) the training step of FusedMLPLoss("hinge"): the module's route, the torch route
        row["scores"] = {"wide": timed(score), "torch": timed(score_torch)}
        row["hinge_step"] = {"wide": timed(step), "torch": timed(lambda xs, y, n: torch_step(module, xs, y, n))}
        # (c) the entry points and their share of the MFMA peak
        it = iter(range(1 << 30))
        k_scores = timed(lambda xs, y, n: fused.mlp_wide_scores(xs, params, n))
        k_grad = timed(lambda xs, y, n: fused.mlp_wide_grad(xs, params, gs[next(it) % len(gs)], n))
        f_fwd, f_grad = row_flops(F)
        row["kernels"] = {"scores": k_scores, "grad_and_reduce": k_grad,
                          "scores_share_of_peak": round(real * f_fwd / (k_scores * 1e-6) / PEAK_F32_MFMA, 3),
                          "grad_share_of_peak": round(real * f_grad / (k_grad * 1e-6) / PEAK_F32_MFMA, 3),
                          "scores_GBps": round(real * F * 4 / (k_scores * 1e-6) / 1e9, 1)}
        result["shapes"][shape] = row
        del data, gs
        torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
