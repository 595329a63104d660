#!/usr/bin/env python3
"""Golden fixture for Get and scan with keys of every length: two put streams,
the HSTable files the REFERENCE writes for them, what the reference's own
Database::Get returns for every key and how many entries its iterator visits.

Runs oracle/_ref/ref_db (built by __graft_entry__.build()) on each stream and
`ref_db --verify` on a COPY of the directory (make_golden_getkeys.run_ref_verified
with its raise_hstable_size step).  Exit 0 is the reference confirming that
Database::Get, its iterator and MultipartReader return the last value put for
every key; only then is anything stored.  Neither stream had to be shrunk.
What --verify printed:

    xx      (348 puts, 3 files):
            verify 113 found 0 missing 0 bad 113 iterated 0 iterator_bad 0 multipart_bad
    murmur  (218 puts, 2 files):
            verify 112 found 0 missing 0 bad 112 iterated 0 iterator_bad 0 multipart_bad

    python tests/golden/make_golden_keylens.py      -> tests/golden/key_lengths.npz

Layout: get_keys.npz's arrays per stream (`__stream`, `__opts`, `__files`,
`__file_*`, `__len`, `__crc`) and scan.npz's (`__iterated`, `__iterator_bad`);
the distinct keys, sorted, as one byte array `__keys` with `__key_off` (n + 1
offsets); `__twins`: rows of (index of A, index of B, position of the one
byte in which they differ); `__hot`: indices of the hot keys.

Both streams: 64 KiB HSTables, 32 KiB parts.  Keys are seeded random bytes:
  * one of every length 1..80 (every MurmurHash3 tail 0..15 behind 0..4 blocks;
    xxHash-64 below and from 32 bytes with every 8/4/1-byte remainder);
  * 127, 128, 129, 252..260, 300, 511..516 and 1000 bytes;
  * a twin of the same length, one byte different, for 16 (byte 0), 67 (last),
    255 (last), 256 (byte 255, last), 257 (byte 256, last), 259 (byte 255),
    260 (byte 256), 513 (last) and 1000 (byte klen - 2), and for 66 and 514
    (last; lengths of 2 mod 4, which the list above does not hold);
  * a hot key of 19 bytes put 70 times and, in `xx`, one of 258 bytes put 130
    times, the overwrites spread through the stream and so through the files;
  * a third of the other keys overwritten once, later in the stream.
Values of 0, 1, 13, 100 and 300..2000 bytes, G1 (compressible) and G3
(incompressible), one of them sent in two PutPart chunks.  The empty key is
not in the streams (index_live_kernel takes a valid entry's key as non-empty).
"""
from __future__ import annotations

import contextlib
import io
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import oracle  # noqa: E402
from make_golden_getkeys import HSTABLE_SIZE, PART_SIZE, run_ref_verified  # noqa: E402
from make_golden_put import encode_stream  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "key_lengths.npz")

LENGTHS = list(range(1, 81)) + [127, 128, 129] + list(range(252, 261)) + [300] + list(range(511, 517)) + [1000]
# length -> position of the byte in which the twin differs
TWINS = {16: 0, 67: 66, 255: 254, 256: 255, 257: 256, 259: 255, 260: 256, 513: 512, 1000: 998, 66: 65, 514: 513}
HOT = {"xx": [(19, 70), (258, 130)], "murmur": [(19, 70)]}


def streams(orc, ref):
    pool = oracle.g1_pool(orc, 1 << 20)
    g3 = ref.g3(65536, 1).tobytes()
    out = {}
    for name, ht, seed in (("xx", 1, 31), ("murmur", 0, 32)):
        rng = np.random.default_rng(seed)
        pos = [int(rng.integers(0, 1 << 19))]

        def value(n: int, incompressible: bool) -> bytes:
            if incompressible:
                o = int(rng.integers(0, len(g3) - n))
                return g3[o:o + n]
            if pos[0] + n > len(pool):
                pos[0] = 0
            v = pool[pos[0]:pos[0] + n].tobytes()
            pos[0] += n
            return v

        def size() -> int:
            c = int(rng.integers(0, 10))
            return (0, 1, 13, 100)[c] if c < 4 else int(rng.integers(300, 2001))

        keys, seen = [], set()
        for n in LENGTHS:
            while True:
                k = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
                if k not in seen:
                    break
            seen.add(k)
            keys.append(k)
        twins = []
        for n, at in TWINS.items():
            a = keys[LENGTHS.index(n)]
            b = bytearray(a)
            b[at] ^= int(rng.integers(1, 256))
            b = bytes(b)
            assert b not in seen
            seen.add(b)
            keys.append(b)
            twins.append((a, b, at))
        hot = []
        for n, _ in HOT[name]:
            k = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            assert k not in seen
            seen.add(k)
            hot.append(k)
        # every key once in a shuffled order, then a third of them once more
        order = [keys[i] for i in rng.permutation(len(keys))]
        again = [keys[i] for i in rng.permutation(len(keys))[:len(keys) // 3]]
        plain = order + again
        puts = [(k, value(size(), i % 4 == 3), None) for i, k in enumerate(plain)]
        # one value in two PutPart chunks (an overwrite, so late in the stream)
        i = len(order) + 5
        puts[i] = (puts[i][0], value(1500, False), [700, 800])
        # the hot keys' puts, evenly through the stream
        for k, (_, times) in zip(hot, HOT[name]):
            total = len(puts) + times
            at = sorted({int(x) for x in np.linspace(0, total - 1, times)})
            assert len(at) == times
            vals = [value((13, 100, int(rng.integers(300, 901)))[j % 3], j % 5 == 4) for j in range(times)]
            assert len(set(vals)) == times                 # different values: the newest is told from the others
            for a, v in zip(at, vals):
                puts.insert(a, (k, v, None))
        out[name] = (puts, ht, keys + hot, twins, hot)
    return out


def main() -> None:
    orc, ref = oracle.Oracle(), oracle.Reference()
    arrs, names = {}, []
    for name, (puts, ht, keys, twins, hot) in streams(orc, ref).items():
        s = encode_stream(puts)
        print(f"{name}: {len(puts)} puts")
        printed = io.StringIO()
        with contextlib.redirect_stdout(printed):
            files = run_ref_verified(orc, s, ht)          # raises unless --verify exits 0
        print("  ", printed.getvalue().strip())
        m = re.search(r"(\d+) iterated (\d+) iterator_bad", printed.getvalue())
        if not m:
            raise SystemExit(f"{name}: no iterator counts in {printed.getvalue()!r}")
        iterated, bad = int(m.group(1)), int(m.group(2))
        last = {}
        for k, v, _ in puts:
            last[k] = v
        skeys = sorted(last)
        assert set(skeys) == set(keys)
        if bad != 0 or iterated != len(skeys):
            raise SystemExit(f"{name}: the reference's iterator did not visit exactly the distinct keys")
        names.append(name)
        arrs[f"{name}__stream"] = np.frombuffer(s, np.uint8)
        arrs[f"{name}__opts"] = np.array([HSTABLE_SIZE, ht, PART_SIZE], np.uint64)
        arrs[f"{name}__files"] = np.array(list(files), dtype="U16")
        for f, b in files.items():
            arrs[f"{name}__file_{f}"] = np.frombuffer(b, np.uint8)
        arrs[f"{name}__keys"] = np.frombuffer(b"".join(skeys), np.uint8)
        arrs[f"{name}__key_off"] = np.cumsum([0] + [len(k) for k in skeys]).astype(np.uint64)
        arrs[f"{name}__len"] = np.array([len(last[k]) for k in skeys], np.uint64)
        arrs[f"{name}__crc"] = np.array([orc.crc32c(last[k]) for k in skeys], np.uint32)
        arrs[f"{name}__twins"] = np.array([(skeys.index(a), skeys.index(b), at) for a, b, at in twins], np.uint32)
        arrs[f"{name}__hot"] = np.array([skeys.index(k) for k in hot], np.uint32)
        arrs[f"{name}__iterated"] = np.array([iterated], np.uint64)
        arrs[f"{name}__iterator_bad"] = np.array([bad], np.uint64)
        print(f"   {len(skeys)} keys, {len(files)} file(s), {sum(map(len, files.values()))} bytes")
    arrs["names"] = np.array(names, dtype="U16")
    np.savez_compressed(OUT, **arrs)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
