"""The K-streamed wide-hidden MLP scorer kernels on a wide bf16 batch (include/ltr_mlp_bigwidebf16.h) against the fp32
K-streamed wide-hidden kernels (include/ltr_mlp_bigwide.h) on `xs.float()` of the same values, at hidden sizes (128, 32)
and (256, 64).  The shapes are those of scripts/bench_mlp_bigwide.py with the rows padded to whole 16-byte pieces of
bf16, as the modules pad them: Istella 220 -> 224 features, Yahoo 699 -> 704.

Prints one JSON line: per hidden size and shape (queries x list size x features, ragged n ~ U[1, L]), times in us, one
process, cold batches:
  scores / grad  -- the entry points on their own: `bf16` = fused.mlp_bigwide_scores_bf16 / mlp_bigwide_grad_bf16 on the
                    bf16 batch, `f32` = fused.mlp_bigwide_scores / mlp_bigwide_grad on the fp32 copy made beforehand (the
                    cast is not in the time); medians, the fp32 side's own spread over its regions (min, max), `ratio` =
                    f32 / bf16, `wins` = the bf16 median lies below the fp32 side's FASTEST region, and `slower` = it
                    lies above the fp32 side's slowest region (neither: level);
  cast           -- `xs.float()` of one batch: what a bf16 user pays per call today on top of `f32`;
  share_of_peak  -- FLOPs of the real rows at the network's own sizes over the time, against the 155 TFLOP/s f32 MFMA peak
                    (for the bf16 side a yardstick only: two thirds of its arithmetic run on the bf16 instruction).
Each region is one call per batch of a rotating set larger than the 256 MiB last-level cache, timed by device events
around a synchronised region; --regions regions after --warmup untimed ones, both sides interleaved region by region
(bf16, f32, bf16, f32, ...), so clock and thermal drift fall on both sides alike.

    python scripts/bench_mlp_bigwidebf16.py [--regions 7] [--warmup 2] [--shapes 1024x200x224,...] [--max-batches 64]
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
from bench_mlp_bigbf16 import interleaved  # noqa: E402
from bench_mlp_rows import PEAK_F32_MFMA  # noqa: E402
from pytorchltr_amd import fused  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="1024x200x224,512x512x704")
    ap.add_argument("--hidden", default="128x32,256x64")
    ap.add_argument("--max-batches", type=int, default=64)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    result = {"unit": "us", "shapes": {}}
    for shape in args.shapes.split(","):
        B, L, F = (int(v) for v in shape.split("x"))
        if not fused._MLP_BIG_WIDE_BF16.takes(F, 256, 64):
            raise SystemExit(fused._MLP_BIG_WIDE_BF16.limits)
        data16 = [(xs.bfloat16(), y, n) for xs, y, n in batches(B, L, F, dev, args.max_batches)]
        datas = {"bf16": data16, "f32": [(xs.float(), y, n) for xs, y, n in data16]}        # the same values
        real = sum(int(n.clamp(0, L).sum()) for _, _, n in data16) / len(data16)
        gs = [torch.randn(B, L, device=dev) for _ in data16]
        cast = round(time_region(lambda xs, y, n: xs.float(), data16, args.regions, args.warmup), 2)
        for hidden in args.hidden.split(","):
            H1, H2 = (int(v) for v in hidden.split("x"))
            params = [p.detach() for p in fused.MLPScorer(F, hidden=(H1, H2)).to(dev)._params()]
            it = iter(range(1 << 30))
            calls = {"scores": {"bf16": lambda xs, y, n: fused.mlp_bigwide_scores_bf16(xs, params, n),
                                "f32": lambda xs, y, n: fused.mlp_bigwide_scores(xs, params, n)},
                     "grad": {"bf16": lambda xs, y, n: fused.mlp_bigwide_grad_bf16(xs, params, gs[next(it) % len(gs)], n),
                              "f32": lambda xs, y, n: fused.mlp_bigwide_grad(xs, params, gs[next(it) % len(gs)], n)}}
            row = {"batches": len(data16), "real_rows": round(real), "cast": cast}
            for name, flops in zip(("scores", "grad"), row_flops(F, H1, H2)):
                times = interleaved(calls[name], datas, args.regions, args.warmup)
                med = {side: statistics.median(v) for side, v in times.items()}
                row[name] = {"bf16": round(med["bf16"], 2), "f32": round(med["f32"], 2),
                             "f32_spread": [round(min(times["f32"]), 2), round(max(times["f32"]), 2)],
                             "ratio": round(med["f32"] / med["bf16"], 3), "wins": med["bf16"] < min(times["f32"]),
                             "slower": med["bf16"] > max(times["f32"]),
                             "share_of_peak": {side: round(real * flops / (med[side] * 1e-6) / PEAK_F32_MFMA, 3)
                                               for side in ("bf16", "f32")}}
            result["shapes"]["%s h%s" % (shape, hidden)] = row
        del datas, data16, gs
        torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
