"""The MLP scorer kernels on wide bf16 rows (include/ltr_mlp_widebf16.h) against the fp32 wide-row kernels
(include/ltr_mlp_wide.h) on the same values, in one process.

Prints one JSON line: per shape (queries x list size x features, n ~ U[1, L], random features, int64 labels in
[0, 5)), with the guide's network Linear(F, 50) / ReLU / Linear(50, 10) / ReLU / Linear(10, 1), times in us as
[median, min, max] over the regions:
  kernels     -- the score call and the gradient call (both gradient kernels + the reductions of the partial vectors)
                 of both families: `bf16` = fused.mlp_wide_scores_bf16 / fused.mlp_wide_grad_bf16 on the bf16 batch,
                 `f32` = fused.mlp_wide_scores / fused.mlp_wide_grad on the same batch upcast beforehand; `ratio` =
                 f32 / bf16 of the medians; `*_share_of_8TBps` = the bytes that must move once (the feature rows of the
                 real documents at 2 or 4 bytes a feature, plus 4 bytes of score or of d loss / d score) over the median,
                 as a share of 8 TB/s; `*_wins` = the bf16 median is not above the fp32 median by more than the fp32
                 call's own min-max spread in this run;
  hinge_step  -- FusedMLPLoss(F, "hinge") forward + backward of the mean loss: the bf16 batch with `wide_bf16=True`
                 against the fp32 batch (score kernel, loss kernel, gradient kernels on both sides: no one-launch step
                 exists at these widths).
A feature count that is not a multiple of 8 (700, 452) is padded ONCE, outside the timed regions, as a user stores the
split (`features_bf16` is the padded width; the bf16 module is built with that many inputs); the fp32 side keeps its
width.  Each region is one call per batch of a rotating set whose bf16 copy alone is larger than the 256 MiB last-level
cache, timed by device events around a synchronised region; --regions regions after --warmup untimed ones.

    python scripts/bench_mlp_widebf16.py [--regions 7] [--warmup 2] [--shapes 512x512x700,...] [--max-batches 64]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_mlp_bf16 import HBM_BYTES_PER_S, HIDDEN, batches  # noqa: E402
from pytorchltr_amd import fused  # noqa: E402


def regions_us(fn, data, regions, warmup):
    """[median, min, max] us per call of fn on one batch, from `regions` event-timed regions of len(data) calls each."""
    times = []
    for r in range(warmup + regions):
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for xs, y, n in data:
            fn(xs, y, n)
        stop.record()
        torch.cuda.synchronize()
        if r >= warmup:
            times.append(start.elapsed_time(stop) * 1000.0 / len(data))
    return [round(statistics.median(times), 2), round(min(times), 2), round(max(times), 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="512x512x700,256x1000x700,1024x128x700,1024x300x452")
    ap.add_argument("--max-batches", type=int, default=64)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    result = {"unit": "us, [median, min, max]", "hidden": list(HIDDEN), "shapes": {}}
    for shape in args.shapes.split(","):
        B, L, F = (int(v) for v in shape.split("x"))
        F8 = (F + 7) & ~7
        data = batches(B, L, F, dev, args.max_batches)
        real = sum(int(n.clamp(0, L).sum()) for _, _, _, n in data) / len(data)
        m32 = fused.FusedMLPLoss(F, "hinge", hidden=HIDDEN).to(dev)
        m16 = fused.FusedMLPLoss(F8, "hinge", hidden=HIDDEN, wide_bf16=True).to(dev)
        with torch.no_grad():
            m16.l1.weight.zero_()
            m16.l1.weight[:, :F].copy_(m32.l1.weight)
            for a, b in zip(list(m16.parameters())[1:], list(m32.parameters())[1:]):
                a.copy_(b)
        p32 = [p.detach() for p in m32._params()]
        p16 = [p.detach() for p in m16._params()]
        gs = [torch.randn(B, L, device=dev) for _ in data]
        it = iter(range(1 << 30))

        def g_next():
            return gs[next(it) % len(gs)]

        def timed(fn, which):
            view = [((xb if which == "bf16" else xf), y, n) for xb, xf, y, n in data]
            return regions_us(fn, view, args.regions, args.warmup)

        def step(module):
            def run(xs, y, n):
                module(xs, y, n).backward()
                for p in module.parameters():
                    p.grad = None
            return run

        k = {
            "scores_bf16": timed(lambda xs, y, n: fused.mlp_wide_scores_bf16(xs, p16, n), "bf16"),
            "scores_f32": timed(lambda xs, y, n: fused.mlp_wide_scores(xs, p32, n), "f32"),
            "grad_bf16": timed(lambda xs, y, n: fused.mlp_wide_grad_bf16(xs, p16, g_next(), n), "bf16"),
            "grad_f32": timed(lambda xs, y, n: fused.mlp_wide_grad(xs, p32, g_next(), n), "f32"),
        }
        for what in ("scores", "grad"):
            bf, f32 = k[what + "_bf16"], k[what + "_f32"]
            k[what + "_ratio"] = round(f32[0] / bf[0], 2)
            k[what + "_wins"] = bf[0] <= f32[0] + (f32[2] - f32[1])
            for tag, width in (("bf16", 2 * F8), ("f32", 4 * F)):
                k["%s_%s_share_of_8TBps" % (what, tag)] = round(
                    real * (width + 4) / (k["%s_%s" % (what, tag)][0] * 1e-6) / HBM_BYTES_PER_S, 3)
        s16, s32 = timed(step(m16), "bf16"), timed(step(m32), "f32")
        result["shapes"][shape] = {
            "batches": len(data), "real_rows": round(real), "features_bf16": F8, "kernels": k,
            "hinge_step": {"bf16": s16, "f32": s32, "ratio": round(s32[0] / s16[0], 2)}}
        del data, gs
        torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
