#!/usr/bin/env python
"""Golden vectors for the degenerate queries of tests/degenerate.py from the REAL reference
(rjagerman/pytorchltr), which runs on the CPU here:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/generate_degenerate_golden.py

Writes tests/golden/degenerate_vectors.npz: DATA only -- the reference's per-query losses and score
gradients (`loss.sum().backward()`), computed in fp64 on the builder's exact scores, for all seven
pairwise losses, at 24 x 37 and 24 x 300, for both score modes ("grid", "constant") and for int64 and
float32 labels of the same values.  Keys: `<L>/<scores>/<labels>/<kind>/loss` and `.../grad`; the
builder's scores, labels and list lengths are stored once per shape and score mode, so that the host
test also pins the builder (`<L>/<scores>/scores`, `/y`, `/n`).

Float32-label gradients equal the int64-label ones bit for bit on every query without a negative label
(asserted here); only the rows of the `negative` flavour are stored for them (`.../grad_negative`).

Ties.  The reference breaks score ties by a random permutation (utils/tensor_operations.py:
tiebreak_argsort draws torch.randperm and calls an unstable torch.argsort).  While the reference runs,
this script hands it the identity permutation and a stable argsort -- one of the draws it can make, and
the index tie rule the oracle and the parity tests use.  On the grid scores nothing is tied and the
patch changes nothing there but the order of equal labels inside maxDCG, which has no effect.

The archive is written with fixed zip timestamps: running this script again reproduces it byte for byte.
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("PYTORCHLTR_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, REFERENCE)
sys.path.insert(0, ROOT)
from pytorchltr.loss import (LambdaARPLoss1, LambdaARPLoss2, LambdaNDCGLoss1, LambdaNDCGLoss2,  # noqa: E402
                             PairwiseDCGHingeLoss, PairwiseHingeLoss, PairwiseLogisticLoss)
from tests.degenerate import degenerate_batch, exact_scores, rows_of  # noqa: E402

LOSSES = {"hinge": PairwiseHingeLoss, "dcg_hinge": PairwiseDCGHingeLoss, "logistic": PairwiseLogisticLoss,
          "arp1": LambdaARPLoss1, "arp2": LambdaARPLoss2, "ndcg1": LambdaNDCGLoss1, "ndcg2": LambdaNDCGLoss2}
SHAPES = [(24, 37), (24, 300)]
MODES = ("grid", "constant")
LABELS = {"i64": torch.int64, "f32": torch.float32}
F = 4
SEED = 20261019


class index_ties:
    """The reference's random tie-break with the identity draw, and a stable sort behind it."""

    def __enter__(self):
        self.randperm, self.argsort = torch.randperm, torch.argsort
        torch.randperm = lambda k, device=None, generator=None: torch.arange(k, device=device)
        torch.argsort = lambda x, dim=-1, descending=False, **kw: self.argsort(x, dim=dim, descending=descending, stable=True)
        return self

    def __exit__(self, *exc):
        torch.randperm, torch.argsort = self.randperm, self.argsort
        return False


def reference_loss(kind, scores64, y, n):
    s = torch.from_numpy(scores64).clone().requires_grad_(True)
    with index_ties():
        loss = LOSSES[kind]()(s, y, n)
        loss.sum().backward()
    return loss.detach().numpy().copy(), s.grad.numpy().copy()


def save_fixed(path, arrays):
    """np.savez_compressed with constant member timestamps (numpy stamps the current time)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    out = {}
    for B, L in SHAPES:
        for mode in MODES:
            tag = "%d/%s" % (L, mode)
            grads = {}
            for lname, dtype in LABELS.items():
                X, W, b, y, n, flavours = degenerate_batch(B, L, F, SEED + L, scores=mode, label_dtype=dtype)
                s64 = exact_scores(X)
                if lname == "i64":
                    out[tag + "/scores"] = s64.astype(np.float32)
                    out[tag + "/y"] = y.numpy().astype(np.int8)
                    out[tag + "/n"] = n.numpy().astype(np.int32)
                    assert np.array_equal(out[tag + "/scores"].astype(np.float64), s64)
                neg = rows_of(flavours, ("negative",))
                for kind in LOSSES:
                    loss, grad = reference_loss(kind, s64, y, n)
                    assert loss.dtype == np.float64 and grad.dtype == np.float64
                    out["%s/%s/%s/loss" % (tag, lname, kind)] = loss
                    if lname == "i64":
                        out["%s/%s/%s/grad" % (tag, lname, kind)] = grad
                        grads[kind] = grad
                    else:
                        other = np.setdiff1d(np.arange(B), neg)
                        assert np.array_equal(grad[other], grads[kind][other]), (tag, kind)
                        out["%s/%s/%s/grad_negative" % (tag, lname, kind)] = grad[neg]
    path = os.path.join(HERE, "degenerate_vectors.npz")
    save_fixed(path, out)
    print("wrote %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
