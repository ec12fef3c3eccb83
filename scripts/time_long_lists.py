"""Time the long-list path (include/ltr_hip.h: ltr_*_long_f32) against a plain torch composition, graph-batched
event timing as scripts/time_metrics.py.  One JSON line per (shape, op):

    python scripts/time_long_lists.py [--shapes 1024x5000,256x8192] > profiles/long_lists.jsonl

`us`: per call.  `GBps` (= bytes per us / 1000): the call's compulsory traffic -- scores (4 B) and labels (8 B,
int64) read once, the output written once (ranking 8 B, curve 4 B per document) -- over its time.  `sort_GBps`:
the traffic the sort path itself moves -- 8 B key read + 8 B written per document by the chunk sort and by every
merge pass -- over the same time (about 5-6 TB/s is the achievable stream rate).  The torch composition
(written here, not the reference's code): mask, torch.sort(masked, descending=True, stable=True), gather, gains,
discounts, cumsum (or the top-k sum), and a second sort of the labels for the ideal DCG."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from _benchutil import time_launches  # noqa: E402
from pytorchltr_amd import _C  # noqa: E402

SHAPES = [(1024, 5000), (256, 8192), (64, 20000), (16, 100000), (1, 1 << 22)]


def torch_rank(s, n):
    L = s.shape[1]
    pad = torch.arange(L, device=s.device)[None, :] >= n[:, None]
    return torch.sort(s.masked_fill(pad, -math.inf), dim=1, descending=True, stable=True).indices, pad


def torch_dcg(s, y, n, k, normalize):
    L = s.shape[1]
    r, pad = torch_rank(s, n)
    disc = 1.0 / torch.log2(torch.arange(L, device=s.device, dtype=torch.float32) + 2.0)
    t = (torch.exp2(y.gather(1, r).float()) - 1.0) * disc
    out = t[:, :k].sum(1) if k else t.cumsum(1)
    if normalize:
        yi = torch.sort(y.float().masked_fill(pad, -1.0), dim=1, descending=True).values
        yi = torch.where(pad, y.float(), yi)
        it = (torch.exp2(yi) - 1.0) * disc
        ideal = it[:, :k].sum(1) if k else it.cumsum(1)
        out = out / torch.where(ideal == 0, torch.ones_like(ideal), ideal)
    return out


def torch_arp(s, y, n):
    L = s.shape[1]
    r, pad = torch_rank(s, n)
    yr = y.gather(1, r).float().masked_fill(pad, 0.0)
    pos = torch.arange(1, L + 1, device=s.device, dtype=torch.float32)
    num, den = (yr * pos).sum(1), yr.sum(1)
    return num / torch.where(den == 0, torch.ones_like(den), den)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join("%dx%d" % s for s in SHAPES))
    ap.add_argument("--replays", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _C.lib()
    for shape in args.shapes.split(","):
        B, L = (int(x) for x in shape.split("x"))
        g = torch.Generator(device=dev).manual_seed(B + L)
        s = torch.randn(B, L, device=dev, generator=g)
        y = torch.randint(0, 5, (B, L), device=dev, generator=g)
        n = torch.randint(L // 2, L + 1, (B,), device=dev, generator=g)
        n[0] = L
        ws = [torch.empty(lib.ltr_sort_workspace_bytes(op, B, L), dtype=torch.uint8, device=dev) for op in range(3)]
        rk = torch.empty(B, L, dtype=torch.int64, device=dev)
        curve = torch.empty(B, L, device=dev)
        vec = torch.empty(B, device=dev)

        def cs():
            return torch.cuda.current_stream().cuda_stream

        def dcg_call(k, out):
            return lambda: _C.check(lib.ltr_dcg_long_f32(s.data_ptr(), y.data_ptr(), 0, n.data_ptr(), None, 0, 0, None, B, L,
                                                         k, 1, 1, out.data_ptr(), ws[1].data_ptr(), ws[1].numel(), cs()))
        hip = {
            "ndcg@10": dcg_call(10, vec),
            "ndcg curve": dcg_call(0, curve),
            "arp": lambda: _C.check(lib.ltr_arp_long_f32(s.data_ptr(), y.data_ptr(), 0, n.data_ptr(), None, 0, 0, None, B, L,
                                                         vec.data_ptr(), ws[2].data_ptr(), ws[2].numel(), cs())),
            "rank_by_score": lambda: _C.check(lib.ltr_rank_by_score_long_f32(s.data_ptr(), n.data_ptr(), None, 0, 0, None, B,
                                                                             L, rk.data_ptr(), ws[0].data_ptr(),
                                                                             ws[0].numel(), cs())),
        }
        ref = {
            "ndcg@10": lambda: torch_dcg(s, y, n, 10, True),
            "ndcg curve": lambda: torch_dcg(s, y, n, 0, True),
            "arp": lambda: torch_arp(s, y, n),
            "rank_by_score": lambda: torch_rank(s, n)[0],
        }
        out_bytes = {"ndcg@10": 0, "ndcg curve": 4, "arp": 0, "rank_by_score": 8}
        sorts = {"ndcg@10": 2, "ndcg curve": 2, "arp": 1, "rank_by_score": 1}
        passes = 1 + max(0, math.ceil(math.log2(L / 8192))) if L > 8192 else 1
        docs = B * L
        for name in hip:
            for _ in range(3):
                hip[name]()
                ref[name]()
            per = 10 if docs <= 1 << 23 else 4
            t_hip, _ = time_launches(hip[name], per_graph=per, replays=args.replays)
            t_ref, _ = time_launches(ref[name], per_graph=per, replays=args.replays)
            nbytes = docs * (4 + (8 if name != "rank_by_score" else 0) + out_bytes[name])
            print(json.dumps({
                "B": B, "L": L, "op": name, "us": round(t_hip, 2), "torch_us": round(t_ref, 2),
                "speedup": round(t_ref / t_hip, 2), "GBps": round(nbytes / t_hip / 1e3, 1),
                "sort_GBps": round(sorts[name] * passes * 16 * docs / t_hip / 1e3, 1),
            }), flush=True)


if __name__ == "__main__":
    main()
