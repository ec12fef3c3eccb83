"""The Linear(F, 1) scorer on a bf16 feature batch (include/ltr_linear_bf16.h) against the fp32 kernels on the same
values, in one process.

Prints one JSON line: per shape (queries x list size x features; n ~ U[1, L], or full lists with an `f` behind the
shape; random bf16 features, int64 labels in [0, 5)), median times in us per call:
  scores / grad -- ltr_linear_scores_bf16 / ltr_linear_grad_bf16 (gradient kernel + the reduction of the partial
                   vectors) against ltr_linear_scores_f32 / ltr_linear_grad_f32 on the batch upcast beforehand;
                   `*_share_of_8TBps`: the bytes that must move (the real documents' feature rows at 2 or 4 bytes a
                   feature plus 4 bytes of score or of d loss / d score) over the time, as a share of 8 TB/s;
  step          -- fused.linear_loss_step per loss kind (fused launch + cross-query reduction): `bf16` on the bf16 batch
                   (`bf16_route`: the fused launch or the pieces), `f32` on the upcast batch, `cast_f32` = xs.float()
                   and the fp32 step, which is what a bf16 batch cost before there were bf16 kernels.
A feature count that is not a multiple of 8 is padded ONCE, outside the timed regions, as a user stores the split.
Cold: every timed region is one replay of a hipGraph that holds one call per batch of a rotating set whose bf16
copies alone exceed the 256 MiB last-level cache (as bench.py rotates), between one pair of device events: no host
or event overhead inside; the median of --regions regions after --warmup untimed replays.  Without graph capture the
calls are issued eagerly and `graph` says false (the small shapes are then bound by the host).

    python scripts/bench_linear_bf16.py [--regions 9] [--warmup 2] [--shapes 1024x128x136,16384x128x136f,...]
"""
import argparse
import json
import statistics

import torch

import _benchutil
from pytorchltr_amd import _C, fused

CACHE_BYTES = 256 << 20
HBM_BYTES_PER_S = 8e12


def batches(B, L, F, full, dev, max_batches, seed=0):
    """(bf16 features padded to 8, the same values as fp32, labels, n) batches; the bf16 copies alone exceed the cache."""
    F8 = (F + 7) & ~7
    count = min(max_batches, max(2, -(-(CACHE_BYTES + (32 << 20)) // (B * L * 2 * F8))))
    g = torch.Generator(device=dev).manual_seed(seed)
    out = []
    for _ in range(count):
        xb = torch.nn.functional.pad(torch.randn(B, L, F, device=dev, generator=g).bfloat16(), (0, F8 - F)).contiguous()
        y = torch.randint(0, 5, (B, L), device=dev, generator=g)
        n = torch.full((B,), L, device=dev) if full else torch.randint(1, L + 1, (B,), device=dev, generator=g)
        out.append((xb, xb.float(), y, n))
    return out


def time_rotating(fn, nbuf, regions, warmup):
    """Median us per call of fn(i), i over the nbuf batches: one hipGraph of nbuf calls, one replay per timed region."""
    def many():
        for i in range(nbuf):
            fn(i)
    replay = _benchutil.try_graph(many, warm=1)
    run = replay if replay is not None else many
    times = []
    for r in range(warmup + regions):
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        run()
        stop.record()
        torch.cuda.synchronize()
        if r >= warmup:
            times.append(start.elapsed_time(stop) * 1e3 / nbuf)
    return round(statistics.median(times), 2), replay is not None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="1024x128x136,16384x128x136f,1024x200x224,4096x128x136")
    ap.add_argument("--kinds", default="hinge,logistic,ndcg2")
    ap.add_argument("--max-batches", type=int, default=32)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_linear_bf16: no GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    lib = _C.lib()
    result = {"unit": "us per call, median of %d cold regions" % args.regions, "shapes": {}}
    for shape in args.shapes.split(","):
        full = shape.endswith("f")
        B, L, F = (int(v) for v in shape.rstrip("f").split("x"))
        F8 = (F + 7) & ~7
        data = batches(B, L, F, full, dev, args.max_batches)
        nbuf = len(data)
        real = sum(int(n.sum()) for _, _, _, n in data) / nbuf
        g = torch.Generator(device=dev).manual_seed(1)
        W = (torch.rand(F8, device=dev, generator=g) * 2 - 1) / F8 ** 0.5
        b = torch.zeros(1, device=dev)
        gs = torch.randn(B, L, device=dev, generator=g)
        scores = torch.empty(B, L, device=dev)
        out = torch.empty(F8 + 1, device=dev)
        ws16, nb16 = _C.workspace(lib.ltr_linear_grad_workspace_bytes_bf16(B, L, F8), dev)
        ws32, nb32 = _C.workspace(lib.ltr_linear_grad_workspace_bytes(B, L, F8), dev)

        def sc16(i):
            _C.check(lib.ltr_linear_scores_bf16(_C.ptr(data[i][0]), _C.ptr(W), _C.ptr(b), _C.ptr(data[i][3]), B, L, F8,
                                                _C.ptr(scores), _C.stream_of(scores)))

        def sc32(i):
            _C.check(lib.ltr_linear_scores_f32(_C.ptr(data[i][1]), _C.ptr(W), _C.ptr(b), _C.ptr(data[i][3]), B, L, F8,
                                               _C.ptr(scores), _C.stream_of(scores)))

        def gr16(i):
            _C.check(lib.ltr_linear_grad_bf16(_C.ptr(data[i][0]), _C.ptr(gs), _C.ptr(data[i][3]), B, L, F8, _C.ptr(out),
                                              _C.ptr(ws16), nb16, _C.stream_of(scores)))

        def gr32(i):
            _C.check(lib.ltr_linear_grad_f32(_C.ptr(data[i][1]), _C.ptr(gs), _C.ptr(data[i][3]), B, L, F8, _C.ptr(out),
                                             _C.ptr(ws32), nb32, _C.stream_of(scores)))

        rec = {"batches": nbuf, "real_rows": round(real), "features_in_memory": F8}
        for name, fn in (("scores_bf16", sc16), ("scores_f32", sc32), ("grad_bf16", gr16), ("grad_f32", gr32)):
            rec[name], rec["graph"] = time_rotating(fn, nbuf, args.regions, args.warmup)
        for what in ("scores", "grad"):
            rec[what + "_ratio"] = round(rec[what + "_f32"] / rec[what + "_bf16"], 2)
            for tag, width in (("bf16", 2 * F8), ("f32", 4 * F8)):
                rec["%s_%s_share_of_8TBps" % (what, tag)] = round(
                    real * (width + 4) / (rec["%s_%s" % (what, tag)] * 1e-6) / HBM_BYTES_PER_S, 3)
        rec["step"] = {}
        for kind in args.kinds.split(","):
            code = fused._resolve_loss(kind)[0]
            step = {"bf16_route": fused._linear_route_of("step", data[0][0], code)}
            for name, fn in (
                    ("bf16", lambda i: fused.linear_loss_step(data[i][0], W, b, data[i][2], data[i][3], loss=kind)),
                    ("f32", lambda i: fused.linear_loss_step(data[i][1], W, b, data[i][2], data[i][3], loss=kind)),
                    ("cast_f32", lambda i: fused.linear_loss_step(data[i][0].float(), W, b, data[i][2], data[i][3], loss=kind))):
                step[name], _ = time_rotating(fn, nbuf, args.regions, args.warmup)
            step["f32_over_bf16"] = round(step["f32"] / step["bf16"], 2)
            step["cast_f32_over_bf16"] = round(step["cast_f32"] / step["bf16"], 2)
            # the real documents' feature rows, once, over the step's time
            step["bf16_share_of_8TBps"] = round(real * 2 * F8 / (step["bf16"] * 1e-6) / HBM_BYTES_PER_S, 3)
            step["f32_share_of_8TBps"] = round(real * 4 * F8 / (step["f32"] * 1e-6) / HBM_BYTES_PER_S, 3)
            rec["step"][kind] = step
        result["shapes"][shape] = rec
        del data, gs, scores
        torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
