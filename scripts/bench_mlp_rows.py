"""The stand-alone MLP scorer kernels (include/ltr_mlp_rows.h) against the routes they replace.

Prints one JSON line: per shape (queries x list size x features, ragged n, int64 labels in [0, 5)), with the guide's
network Linear(F, 50) / ReLU / Linear(50, 10) / ReLU / Linear(10, 1), median times in us:
  scores      -- (a) `model.score(xs, n)` under torch.no_grad(): `rows` = ltr_mlp_rows_scores_f32, `torch` = the three
                 nn.Linear layers (rocBLAS), which is what ran past the fused kernels' list lengths before the row
                 kernels; `fused` = ltr_mlp_scores_f32 where that kernel takes the shape;
  hinge_step  -- (b) FusedMLPLoss(F, "hinge") forward + backward of the mean loss: `rows` = row scores, the stand-alone
                 loss kernel, the row gradient kernel; `torch` = the torch layers, the same loss kernel and torch's
                 autograd (the route before, written out here: `torch_step` below, at
                 every shape); `fused_path` says whether the one-launch fused step takes the shape (then `rows` is it);
  kernels     -- (c) the two row kernels on their own (fused._mlp_rows_scores; fused.mlp_grad = gradient kernel + the
                 reduction of the partial vectors) and their share of the 155 TFLOP/s f32 MFMA peak, counting the
                 FLOPs of the real rows at the padded tile sizes (16-feature chunks x 64 x 16).
Each region is one call per batch of a rotating set larger than the 256 MiB last-level cache, timed by device events
around a synchronised region; the median of --regions regions after --warmup untimed ones.

    python scripts/bench_mlp_rows.py [--regions 7] [--warmup 2] [--shapes 256x1000x136,...] [--max-batches 64]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_listwise_fused import batches, time_region  # noqa: E402
from pytorchltr_amd import fused  # noqa: E402

HIDDEN = (50, 10)
PEAK_F32_MFMA = 155e12


def row_flops(F):
    """(forward, forward + backward) FLOPs of one row at the padded tile sizes."""
    Fp = 16 * ((F + 15) // 16)
    fwd = 2 * (Fp * 64 + 64 * 16 + 16)
    return fwd, fwd + 2 * (Fp * 64 + 64 * 16 + 64 * 16 + 16)


def torch_scores(module, xs):
    """The route before the kernels: the module's three nn.Linear layers."""
    return module.l3(torch.relu(module.l2(torch.relu(module.l1(xs)))))


def torch_step(module, xs, y, n):
    module._pieces(torch_scores(module, xs), y, n).mean().backward()
    for p in module.parameters():
        p.grad = None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="256x1000x136,1024x300x220,64x4096x136,1024x128x136")
    ap.add_argument("--max-batches", type=int, default=64)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    result = {"unit": "us, median", "hidden": list(HIDDEN), "shapes": {}}
    for shape in args.shapes.split(","):
        B, L, F = (int(v) for v in shape.split("x"))
        data = batches(B, L, F, dev, args.max_batches)
        real = sum(int(n.clamp(0, L).sum()) for _, _, n in data) / len(data)
        module = fused.FusedMLPLoss(F, "hinge", hidden=HIDDEN).to(dev)
        params = [p.detach() for p in module._params()]
        gs = [torch.randn(B, L, device=dev) for _ in data]
        fused_path = bool(module._fused_shape(B, L, (F + 3) & ~3))

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

        row = {"batches": len(data), "real_rows": round(real), "fused_path": fused_path}
        # (a) scores.  Where the per-query kernel takes the shape, score() is that kernel: the row kernel is called directly
        k_scores = timed(lambda xs, y, n: fused._mlp_rows_scores(xs, params, HIDDEN[0], HIDDEN[1], n))
        row["scores"] = {"rows": k_scores, "torch": timed(score_torch)}
        if fused.mlp_supported(L, F, *HIDDEN):
            row["scores"]["fused"] = timed(score)
        # (b) the training step of FusedMLPLoss("hinge")
        row["hinge_step"] = {"rows": timed(step), "torch": timed(lambda xs, y, n: torch_step(module, xs, y, n))}
        # (c) the kernels and their share of the MFMA peak
        it = iter(range(1 << 30))
        k_grad = timed(lambda xs, y, n: fused.mlp_grad(xs, params, gs[next(it) % len(gs)], n))
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
