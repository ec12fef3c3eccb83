"""The MLP scorer kernels on a bf16 feature batch (include/ltr_mlp_bf16.h) against the fp32 row kernels
(include/ltr_mlp_rows.h) on the same batch, in one process.

Prints one JSON line: per shape (queries x list size x features, n ~ U[1, L], random features, int64 labels in
[0, 5)), with the guide's network Linear(F, 50) / ReLU / Linear(50, 10) / ReLU / Linear(10, 1), median times in us:
  kernels     -- the score call and the gradient call (gradient kernel + the reduction of the partial vectors) of both
                 families: `bf16` = fused.mlp_scores_bf16 / fused.mlp_grad_bf16 on the bf16 batch, `f32` =
                 fused._mlp_rows_scores / fused.mlp_grad on the same batch upcast beforehand; `ratio` = f32 / bf16;
                 `*_share_of_8TBps` = the bytes that must move (the feature rows of the real documents at 2 or 4 bytes
                 a feature, plus 4 bytes of score or of d loss / d score) over the time, as a share of 8 TB/s;
  hinge_step  -- FusedMLPLoss(F, "hinge") forward + backward of the mean loss on both dtypes (`f32_fused_path` says
                 whether the fp32 batch takes the one-launch fused step; a bf16 batch always runs score kernel, loss
                 kernel, gradient kernel).
A feature count that is not a multiple of 8 (220) is padded ONCE, outside the timed regions, as a user stores the split
(`features_bf16` is the padded width; the bf16 module is built with that many inputs); the fp32 side keeps its width.
Each region is one call per batch of a rotating set whose bf16 copy alone is larger than the 256 MiB last-level cache,
timed by device events around a synchronised region; the median of --regions regions after --warmup untimed ones.

    python scripts/bench_mlp_bf16.py [--regions 7] [--warmup 2] [--shapes 256x1000x136,...] [--max-batches 64]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_listwise_fused import CACHE_BYTES, time_region  # noqa: E402
from pytorchltr_amd import fused  # noqa: E402

HIDDEN = (50, 10)
HBM_BYTES_PER_S = 8e12


def batches(B, L, F, dev, max_batches, seed=0):
    """(bf16 features padded to 8, fp32 features, labels, n) batches; the bf16 copies alone exceed the cache."""
    F8 = (F + 7) & ~7
    count = min(max_batches, max(2, -(-(CACHE_BYTES + (32 << 20)) // (B * L * 2 * F8))))
    g = torch.Generator(device=dev).manual_seed(seed)
    out = []
    for _ in range(count):
        xb = torch.randn(B, L, F, device=dev, generator=g).bfloat16()
        y = torch.randint(0, 5, (B, L), device=dev, generator=g)
        n = torch.randint(1, L + 1, (B,), device=dev, generator=g)
        out.append((torch.nn.functional.pad(xb, (0, F8 - F)).contiguous(), xb.float(), y, n))
    return out


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
        F8 = (F + 7) & ~7
        data = batches(B, L, F, dev, args.max_batches)
        real = sum(int(n.clamp(0, L).sum()) for _, _, _, n in data) / len(data)
        m32 = fused.FusedMLPLoss(F, "hinge", hidden=HIDDEN).to(dev)
        m16 = fused.FusedMLPLoss(F8, "hinge", hidden=HIDDEN).to(dev)
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
            return round(time_region(fn, view, args.regions, args.warmup), 2)

        def step(module):
            def run(xs, y, n):
                module(xs, y, n).backward()
                for p in module.parameters():
                    p.grad = None
            return run

        k = {
            "scores_bf16": timed(lambda xs, y, n: fused.mlp_scores_bf16(xs, p16, n), "bf16"),
            "scores_f32": timed(lambda xs, y, n: fused._mlp_rows_scores(xs, p32, HIDDEN[0], HIDDEN[1], n), "f32"),
            "grad_bf16": timed(lambda xs, y, n: fused.mlp_grad_bf16(xs, p16, g_next(), n), "bf16"),
            "grad_f32": timed(lambda xs, y, n: fused.mlp_grad(xs, p32, g_next(), n), "f32"),
        }
        for what in ("scores", "grad"):
            k[what + "_ratio"] = round(k[what + "_f32"] / k[what + "_bf16"], 2)
            for tag, width in (("bf16", 2 * F8), ("f32", 4 * F)):
                k["%s_%s_share_of_8TBps" % (what, tag)] = round(
                    real * (width + 4) / (k["%s_%s" % (what, tag)] * 1e-6) / HBM_BYTES_PER_S, 3)
        s16, s32 = timed(step(m16), "bf16"), timed(step(m32), "f32")
        result["shapes"][shape] = {
            "batches": len(data), "real_rows": round(real), "features_bf16": F8, "kernels": k,
            "hinge_step": {"bf16": s16, "f32": s32, "ratio": round(s32 / s16, 2),
                           "f32_fused_path": bool(m32._fused_shape(B, L, (F + 3) & ~3))}}
        del data, gs
        torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
