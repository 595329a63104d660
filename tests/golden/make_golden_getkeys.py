#!/usr/bin/env python3
"""Golden fixture for Get by key: put streams with overwritten keys, the
HSTable files the REFERENCE writes for them, and what the reference's own
Database::Get returns for every key.

Runs oracle/_ref/ref_db (built by __graft_entry__.build()) on each stream,
reads the files it leaves, then runs `ref_db --verify` on a COPY of the
directory: exit 0 is the reference confirming that Database::Get (and its
iterator and MultipartReader) return the last value put for every key.  Only
then is the expectation stored: per distinct key, the length and CRC32C of
the last value put.  The files stored are the ones from before the verify
run.  Neither stream had to be shrunk: --verify exits 0 on both as written.

One step the verify run needs: Database::Open replaces the caller's options
with the 48-byte db_options file (interface/database.h:112-115), which does not
hold maximum_part_size, and then refuses maximum_part_size (now the 1 MiB
default) >= hstable_size (:152).  So the reference cannot reopen any database
it wrote with hstable_size <= 1 MiB, whatever the stream.  hstable_size is used
by the write path only (hstable_manager.h:90, write_buffer.cc:170), so in the
COPY the db_options file's hstable_size field is raised to 32 MiB (CRC
redone) before --verify; the HSTable files are not touched.

    python tests/golden/make_golden_getkeys.py      -> tests/golden/get_keys.npz

Streams:
  xx      400 puts over 150 distinct 16-byte keys (most keys overwritten, many
          overwrites in a later file), values of 100 B .. 4 KiB, G1
          (compressible) and G3 (incompressible), three values sent in 2-3
          PutPart chunks; 64 KiB HSTables, 32 KiB parts, xxHash-64
  murmur  60 puts over 40 keys, MurmurHash3-64, same options
"""
from __future__ import annotations

import os
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import oracle  # noqa: E402
from make_golden_put import REF_DB, encode_stream  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "get_keys.npz")
HSTABLE_SIZE, PART_SIZE = 64 << 10, 32 << 10     # make_golden_put's `rollover` options


def raise_hstable_size(orc, path: str) -> None:
    """hstable_size := 32 MiB in a db_options file (DatabaseOptionEncoder, format.h:317-331)."""
    with open(path, "rb") as f:
        b = bytearray(f.read())
    assert len(b) == 48 and struct.unpack_from("<Q", b, 28)[0] == HSTABLE_SIZE
    struct.pack_into("<Q", b, 28, 32 << 20)
    struct.pack_into("<I", b, 0, orc.crc32c(bytes(b[4:48])))
    with open(path, "wb") as f:
        f.write(b)


def run_ref_verified(orc, stream: bytes, hash_type: int) -> dict[str, bytes]:
    d = tempfile.mkdtemp(prefix="kdbgetk")
    try:
        sp = os.path.join(d, "stream.bin")
        with open(sp, "wb") as f:
            f.write(stream)
        db = os.path.join(d, "db")
        opts = [str(PART_SIZE), str(HSTABLE_SIZE), str(hash_type)]
        subprocess.run([REF_DB, db, sp] + opts, check=True, capture_output=True)
        files = {}
        for name in sorted(os.listdir(db)):
            if len(name) == 8 and all(c in "0123456789abcdef" for c in name):
                with open(os.path.join(db, name), "rb") as f:
                    files[name] = f.read()
        copy = os.path.join(d, "copy")
        shutil.copytree(db, copy)
        raise_hstable_size(orc, os.path.join(copy, "db_options"))
        v = subprocess.run([REF_DB, "--verify", copy, sp] + opts, capture_output=True, text=True)
        if v.returncode != 0:
            raise SystemExit(f"ref_db --verify exit {v.returncode}: {v.stdout} {v.stderr[-2000:]}")
        print("  ", v.stdout.strip())
        return files
    finally:
        shutil.rmtree(d, ignore_errors=True)


def streams(orc, ref):
    pool = oracle.g1_pool(orc, 1 << 20)
    g3 = ref.g3(65536, 1).tobytes()
    rng = np.random.default_rng(11)
    pos = [0]

    def value(n: int, incompressible: bool) -> bytes:
        if incompressible:
            o = int(rng.integers(0, len(g3) - n))
            return g3[o:o + n]
        if pos[0] + n > len(pool):
            pos[0] = 0
        v = pool[pos[0]:pos[0] + n].tobytes()
        pos[0] += n
        return v

    def make(nputs: int, nkeys: int, chunked: dict):
        puts = []
        sizes = rng.choice([100, 150, 300, 700, 1000, 2000, 4096], nputs, p=[.25, .15, .2, .15, .1, .1, .05])
        for i in range(nputs):
            # every key once, then overwrites of random keys
            k = i if i < nkeys else int(rng.integers(0, nkeys))
            v = value(int(sizes[i]), i % 4 == 3)
            puts.append((b"key%013d" % k, v, chunked.get(i)))
        return puts

    out = {}
    xx = make(400, 150, {})
    # three values sent in parts, one of them overwriting an earlier key late in the stream
    for i, ch in ((20, [1024, 976]), (200, [1000, 1000, 1000]), (390, [2048, 2048])):
        k = xx[i][0]
        xx[i] = (k, value(sum(ch), i == 200), ch)
    out["xx"] = (xx, 1)
    out["murmur"] = (make(60, 40, {}), 0)
    return out


def main() -> None:
    orc, ref = oracle.Oracle(), oracle.Reference()
    arrs, names = {}, []
    for name, (puts, ht) in streams(orc, ref).items():
        s = encode_stream(puts)
        print(f"{name}: {len(puts)} puts")
        files = run_ref_verified(orc, s, ht)
        last = {}
        for k, v, _ in puts:
            last[k] = v
        keys = sorted(last)
        names.append(name)
        arrs[f"{name}__stream"] = np.frombuffer(s, np.uint8)
        arrs[f"{name}__opts"] = np.array([HSTABLE_SIZE, ht, PART_SIZE], np.uint64)
        arrs[f"{name}__files"] = np.array(list(files), dtype="U16")
        for f, b in files.items():
            arrs[f"{name}__file_{f}"] = np.frombuffer(b, np.uint8)
        arrs[f"{name}__keys"] = np.frombuffer(b"".join(keys), np.uint8).reshape(len(keys), 16)
        arrs[f"{name}__len"] = np.array([len(last[k]) for k in keys], np.uint64)
        arrs[f"{name}__crc"] = np.array([orc.crc32c(last[k]) for k in keys], np.uint32)
        print(f"   {len(keys)} keys, {len(files)} file(s), {sum(map(len, files.values()))} bytes")
    arrs["names"] = np.array(names, dtype="U16")
    np.savez_compressed(OUT, **arrs)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
