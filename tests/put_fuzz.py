"""Seeded ragged puts for the put path's fuzz -- TEST INFRASTRUCTURE ONLY.

stream(orc, seed) draws about 200 (key, value, chunks) with the shapes of
tests/test_gpu_flush.py: db_bench text, random bytes and a random tail after
a compressible head, in sizes on both sides of every threshold of the put
policy (the 64-byte and 512-byte entry kernels, the 64 KiB parts, the padding
step at 65536), cut into chunks in eight styles.  tests/test_gpu_put_ragged.py
runs the same streams through the GPU and tests/test_write_path.py through the
reference, so the oracle that judges the GPU is pinned on the very values.
"""
from __future__ import annotations

import numpy as np

SEEDS = (2, 3)          # picked on the CPU: each reaches every class of put_policy_model.CLASSES
NVALUES = 200
SIZES = ((0, 65), (64, 601), (1000, 9001), (60000, 70001), (65536, 110001))
STYLES = ("single", "parts64k", "cuts", "empty_first", "empty_middle", "empty_last", "one_byte", "tail8")


def stream(orc, seed: int, nvalues: int = NVALUES):
    """[(key, value, chunks)], under 8 MB of values."""
    rng = np.random.default_rng(seed)
    pool = orc.g1_pieces(12000).tobytes()
    puts = []
    for j in range(nvalues):
        lo, hi = SIZES[int(rng.choice(len(SIZES), p=(0.26, 0.26, 0.26, 0.12, 0.10)))]
        n = int(rng.integers(lo, hi))
        style = STYLES[int(rng.integers(0, len(STYLES)))]
        if style == "one_byte" and n >= 64:
            n = int(rng.integers(1, 64))
        content = int(rng.integers(0, 3))
        a = int(rng.integers(0, len(pool) - n))
        v = bytearray(pool[a:a + n])                                 # G1 text
        if content == 1 or style == "tail8":
            v[:] = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        elif content == 2 and n:                                     # a random tail after a compressible head
            b = int(rng.integers(0, n))
            v[b:] = rng.integers(0, 256, n - b, dtype=np.uint8).tobytes()
        v = bytes(v)
        key = b"%d-" % j + rng.integers(0, 256, int(rng.integers(0, 88)), dtype=np.uint8).tobytes()
        key = key[:90]
        parts64k = [min(65536, n - o) for o in range(0, n, 65536)] or [0]
        if style == "single" or n == 0:
            ch = [n]
        elif style == "parts64k":
            ch = parts64k
        elif style == "cuts":
            cuts = sorted(set(int(x) for x in rng.integers(0, n + 1, int(rng.integers(1, 7)))))
            ch = [q - p for p, q in zip([0] + cuts, cuts + [n])]
        elif style == "empty_first":
            ch = [0] + parts64k
        elif style == "empty_middle":
            c = int(rng.integers(1, n)) if n > 1 else 1
            ch = [c, 0, n - c] if n > 1 else [1, 0, 0]
        elif style == "empty_last":
            c = int(rng.integers(1, n + 1))
            ch = ([c, n - c] if c < n else [n]) + [0]
        elif style == "one_byte":
            ch = [1] * n
        else:                                                        # V - 8 random bytes, then 8
            ch = [n - 8, 8] if n > 8 else [n]
        assert sum(ch) == n and 1 <= len(key) <= 90
        puts.append((key, v, ch))
    assert sum(len(v) for _, v, _ in puts) < 8 << 20
    return puts
