"""Generates tests/golden/foreign_blocks.npz from the REFERENCE codec.

Run where the reference build exists (oracle/_ref, `make -C oracle ref`):

    python tests/golden/make_golden_blocks.py

For the seeded block sets of tests/test_gpu_foreign_blocks.py (tests/
lz4_blocks.py: set_a, set_b's extra blocks, set_c, set_d's extra block,
set_e and the service's cases) the file holds the reference's
LZ4_decompress_safe_partial return code and the CRC32C of its output, once
with the full size as the target and once with the partial target the GPU
tests give that case -- and nothing else: the blocks are regenerated from
the seed.  A machine without the reference is pinned to it by these.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lz4_blocks as L  # noqa: E402
import oracle  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "foreign_blocks.npz")


def main() -> None:
    ref = oracle.Reference()
    arrs = {}
    for name, cases in L.stored_sets().items():
        for k, v in L.results(ref, cases).items():
            arrs["%s_%s" % (name, k)] = v
        print(name, len(cases), "blocks,", int((arrs[name + "_ret"] <= 0).sum()), "errors or empty")
    np.savez_compressed(OUT, **arrs)
    print("written", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
