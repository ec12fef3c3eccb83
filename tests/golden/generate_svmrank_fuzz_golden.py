#!/usr/bin/env python
"""Reference outputs for the seeded random / mutated SVMrank files and the large file of
tests/test_svmrank_parser.py, so that those tests need neither the reference sources nor a
compiled reference parser.

The reference's C parser is compiled from where it lies by oracle/build_ref.py
(oracle/_ref/libsvmrank_ref.so, LTR_REFERENCE_ROOT) and run on every file the tests generate;
per file the status and the sha256 of the text and of (xs, ys, qids) are stored.

    python tests/golden/generate_svmrank_fuzz_golden.py

Writes tests/golden/svmrank_fuzz_digests.npz.  Data only.
"""
import hashlib
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
from oracle import build_ref  # noqa: E402
from tests.test_svmrank_parser import FUZZ_CASES, _digest, fuzz_cases, write_large_file  # noqa: E402

OUT = os.path.join(HERE, "svmrank_fuzz_digests.npz")


def main():
    if build_ref.build() is None:
        raise SystemExit("the reference parser is not available (oracle/build_ref.py)")
    status = np.full(FUZZ_CASES, -1, dtype=np.int32)
    text_sha = np.zeros((FUZZ_CASES, 32), dtype=np.uint8)
    out_sha = np.zeros((FUZZ_CASES, 32), dtype=np.uint8)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "f.txt")

        def status_of(it, text):
            with open(path, "wb") as f:
                f.write(text.encode())
            rc, X, Y, Q = build_ref.parse_svmrank_file(path)
            status[it] = rc
            text_sha[it] = np.frombuffer(hashlib.sha256(text.encode()).digest(), np.uint8)
            if rc == 0:
                out_sha[it] = np.frombuffer(_digest(X, Y, Q), np.uint8)
            return rc

        for _ in fuzz_cases(status_of):
            pass
        big = os.path.join(tmp, "big.txt")
        write_large_file(big)
        rc, X, Y, Q = build_ref.parse_svmrank_file(big)
        assert rc == 0
        large_text = np.frombuffer(hashlib.sha256(open(big, "rb").read()).digest(), np.uint8)
        large_out = np.frombuffer(_digest(X, Y, Q), np.uint8)
    assert (status >= 0).all()
    np.savez_compressed(OUT, status=status, text_sha256=text_sha, out_sha256=out_sha,
                        large_text_sha256=large_text, large_out_sha256=large_out)
    print("wrote %s: %d files, %d accepted" % (OUT, FUZZ_CASES, int((status == 0).sum())))


if __name__ == "__main__":
    main()
