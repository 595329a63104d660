#!/usr/bin/env python3
"""Golden fixture of ragged puts: values cut into chunks the way no tidy client
cuts them, and the HSTable files the REFERENCE writes for them.

Like make_golden_put.py (whose stream format and ref_db runner it reuses) this
runs oracle/_ref/ref_db on each stream and stores the stream and the files it
leaves.  hstable_streams.npz reaches six classes of put
(tests/put_policy_model.py OLD_CLASSES); these streams reach the rest:

    python tests/golden/make_golden_ragged.py   -> tests/golden/hstable_ragged.npz

Streams (all xxHash):
  ragged_ok   32 MiB files: chunkings the reference reads back -- the disable
              rule on the first and on a middle chunk of several, empty chunks
              in the middle and at the end, sizes on both sides of 65536 (the
              padding goes from 8 to 16).  `ref_db --verify` must return 0.
  ragged_odd  32 MiB files: what the reference leaves unreadable or refuses --
              later chunks dropped behind a first or middle chunk that looks
              last, entries never finished, an empty first chunk (the next call
              starts the value again), a refused empty chunk behind a disable,
              one key put twice with the first put left unfinished.  Run with
              KDB_DB_KEEP_GOING=1; a plain 100-byte put follows every value.
  ragged_cut  64 KiB files: multipart entries whose reserved region crosses
              the file cut, finished, finished twice and never finished.
Every stream also stores `<name>__refused`, the (record, chunk) pairs of the
calls ref_db reported as refused.
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import oracle  # noqa: E402
from make_golden_put import REF_DB, encode_stream  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "hstable_ragged.npz")
ODD = {"self_contained_chunks_dropped", "early_last_chunks_dropped", "multipart_unfinished", "refused",
       "dropped_bytes_zero_filled", "empty_chunk_first"}


def run_ref_keep_going(stream: bytes, hstable_size: int, hash_type: int, part_size: int, verify: bool):
    """(files, refused (record, chunk) pairs) of ref_db over the stream with
    KDB_DB_KEEP_GOING=1; with verify, `ref_db --verify` must then return 0."""
    d = tempfile.mkdtemp(prefix="kdbgold")
    try:
        sp = os.path.join(d, "stream.bin")
        open(sp, "wb").write(stream)
        db = os.path.join(d, "db")
        args = [str(part_size), str(hstable_size), str(hash_type)]
        r = subprocess.run([REF_DB, db, sp] + args, capture_output=True, env=dict(os.environ, KDB_DB_KEEP_GOING="1"))
        refused = [(int(a), int(b)) for a, b in re.findall(rb"^put (\d+) chunk (\d+):", r.stderr, re.M)]
        if r.returncode != (3 if refused else 0):
            raise RuntimeError("ref_db: exit status %d\n%s" % (r.returncode, r.stderr.decode(errors="replace")[-2000:]))
        files = {f: open(os.path.join(db, f), "rb").read() for f in sorted(os.listdir(db))
                 if len(f) == 8 and all(c in "0123456789abcdef" for c in f)}
        if verify:
            subprocess.run([REF_DB, "--verify", db, sp] + args, check=True, capture_output=True)
        return files, refused
    finally:
        shutil.rmtree(d, ignore_errors=True)


def exact_fit(orc, rnd, size: int, c0: int):
    """A value of `size` bytes and chunks [c0, c1, r] whose first two frames
    end exactly at `size` with compression still on: the middle call then looks
    like a last part (util/order.h:52-55) and the last r bytes are dropped.
    The middle chunk is random bytes followed by zeros, the random stretch
    tuned until its frame has the length that is needed; None if no stretch
    does.  (The disable rule leaves room for this only where the padding is
    16, size >= 65536, and r <= 8: database.cc:197-200.)"""
    head = rnd(c0)
    f0 = len(orc.frame(head))
    body = rnd(size)
    for r in range(1, 9):
        c1 = size - c0 - r
        lo, hi = 0, c1
        while lo < hi:                          # frame length grows with the random stretch
            x = (lo + hi) // 2
            if f0 + len(orc.frame(body[:x] + bytes(c1 - x))) < size:
                lo = x + 1
            else:
                hi = x
        for x in range(max(lo - 3, 0), min(lo + 4, c1 + 1)):
            mid = body[:x] + bytes(c1 - x)
            if f0 + len(orc.frame(mid)) == size:
                return head + mid + rnd(r), [c0, c1, r]
    return None


def streams(orc):
    pool = oracle.g1_pool(orc, 1 << 20).tobytes()
    rng = np.random.default_rng(20)
    pos = [0]

    def G(n):                                   # db_bench text
        if pos[0] + n > len(pool):
            pos[0] = 0
        pos[0] += n
        return pool[pos[0] - n:pos[0]]

    def R(n):                                   # incompressible
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    def A(n):
        return (b"abcdefgh" * (n // 8 + 1))[:n]

    # (value, chunks, classes it must reach).  The file has to stay under 1 MiB
    # and random bytes do not shrink, so only the values that need the
    # 16-byte padding (size >= 65536) are large; big compressible values are
    # runs of "abcdefgh".
    cand = []

    def add(v, ch, *must):
        cand.append((v, ch, set(must)))

    # a first chunk that looks last: [V - 8, 8] of random bytes, under and at 65536
    for v in (2000, 65535, 65536):
        add(R(v), [v - 8, 8], "self_contained_chunks_dropped")
    # the disable rule on a middle chunk, the value finished by its real last part:
    # padding 16 takes one stored frame and the second fires; padding 8 fires
    # as soon as the frames so far are longer than the bytes so far
    add(R(40000) + A(25536), [20000, 20000, 12000, 13536], "disable_middle", "multipart_finished_svc")
    add(b"a" * 20 + R(500) + G(300), [20, 500, 300], "disable_middle", "multipart_finished_svc")
    add(b"a" * 20 + R(300) + A(65215), [20, 300, 65215], "disable_middle", "multipart_finished_svc")
    # ... on the first of three
    add(R(1000) + A(1000), [1000, 600, 400], "disable_first_of_several", "multipart_finished_svc")
    add(R(200) + G(200), [200, 100, 100], "disable_first_of_several")
    # ... on a middle chunk, then a chunk that ends at V before the last one
    add(R(65536), [30000, 20000, 15520, 16], "disable_middle", "early_last_chunks_dropped",
        "multipart_finished_svc0", "dropped_bytes_zero_filled")
    add(R(3000), [1000, 1000, 992, 8], "disable_first_of_several", "early_last_chunks_dropped",
        "dropped_bytes_zero_filled")
    # one-byte chunks: disabled at once, the raw bytes reach V eight calls early
    add(A(40), [1] * 40, "early_last_chunks_dropped")
    add(G(63), [1] * 63, "early_last_chunks_dropped")
    # empty chunks in the middle, first and last
    add(A(5000), [3000, 0, 2000], "empty_chunk_middle", "multipart_finished_svc")
    add(G(300), [100, 0, 200], "empty_chunk_middle")
    add(R(300), [100, 0, 200], "empty_chunk_middle", "disable_first_of_several")
    add(A(65536), [65535, 0, 1], "empty_chunk_middle")
    add(A(70000), [0, 65536, 4464], "empty_chunk_first", "multipart_unfinished")
    add(A(65535), [0, 65535], "empty_chunk_first")
    add(A(65536), [0, 0, 30000, 35536], "empty_chunk_first")
    add(A(5000), [3000, 2000, 0], "empty_chunk_last", "last_part_twice")
    add(A(100000), [65536, 34464, 0], "empty_chunk_last", "last_part_twice")
    add(A(65535), [65000, 535, 0], "last_part_twice")
    add(A(65536), [65000, 536, 0, 0], "last_part_twice")
    add(G(7000), [3000, 4000, 0], "last_part_twice")
    add(A(100), [0, 100, 0], "empty_chunk_first", "empty_chunk_last")
    add(A(100), [0, 100], "empty_chunk_first")
    add(A(100), [100, 0], "empty_chunk_last", "self_contained_chunks_dropped")
    add(A(100), [0, 60, 40], "empty_chunk_first")
    add(b"", [0, 0], "empty_chunk_first")
    add(b"", [0], "empty_value_one_chunk")
    # a trailing empty chunk after a disable: refused
    add(R(3000), [2000, 1000, 0], "refused")
    add(b"a" * 20 + R(3000), [20, 3000, 0], "refused", "disable_middle")
    add(R(500), [500, 0], "refused")
    # the disable rule on the last chunk: svc is 8 short of the chunk's end, never finished
    add(b"a" * 20 + R(3000), [20, 3000], "disable_last_chunk", "multipart_unfinished")
    # frames that end exactly at V while compression is on
    ef = exact_fit(orc, R, 65536, 30000)
    if ef is None:
        raise RuntimeError("no exact fit found")
    add(ef[0], ef[1], "early_last_chunks_dropped", "multipart_finished_svc0", "dropped_bytes_zero_filled")
    # compressible multiparts in tidy parts, for the read-back
    add(A(110000), [65536, 44464], "multipart_finished_svc")
    add(G(9000), [4096, 4096, 808], "multipart_finished_svc")

    from put_policy_model import classify_put
    ok, odd = [], []
    for i, (v, ch, must) in enumerate(cand):
        assert sum(ch) == len(v) and len(v) <= 110000
        tags, calls = classify_put(orc, b"k", v, ch)
        assert must <= tags, (i, ch, sorted(must - tags))
        if "disable_middle" in must or "exact" in must:
            assert calls[0]["mode"] == 0
        key = b"rg%03d-" % i + b"k" * (i % 19)      # 6 .. 24 bytes
        if tags & ODD:
            odd.append((key, v, ch))
            odd.append((b"plain%03d" % i, G(100), None))
        else:
            ok.append((key, v, ch))
            if i % 2:
                ok.append((b"plain%03d" % i, G(100), None))
    # one key twice, the first put left unfinished (the disable rule on its last chunk)
    odd.append((b"twice", b"a" * 20 + R(2000), [20, 2000]))
    odd.append((b"twice", G(5000), [2500, 2500]))
    odd.append((b"plain-end", G(100), None))
    # ... and in the readable stream a key put twice, both finished
    ok.append((b"again", G(5000), [2500, 2500]))
    ok.append((b"again", A(3000), [1000, 0, 2000]))

    def fill(lo, hi):                           # ~ 1 KiB entries, each its own bytes
        return [(b"%016d" % i, b"%06d" % i + A(1000 - 6), None) for i in range(lo, hi)]

    cut = fill(0, 50)                                                   # ~ 52 KiB of entries
    cut.append((b"cross-finished", A(30000), [10000, 10000, 10000]))    # reserved region crosses 64 KiB
    cut += fill(50, 105)
    cut.append((b"cross-twice", A(40000), [20000, 20000, 0]))
    cut += fill(105, 155)
    cut.append((b"cross-unfinished", b"a" * 20 + R(12000), [20, 12000]))
    cut += fill(155, 170)
    # (maximum_part_size must stay under the file size; no chunk of ragged_cut reaches it)
    return {"ragged_ok": (ok, 32 << 20, 1, 1 << 20, True), "ragged_odd": (odd, 32 << 20, 1, 1 << 20, False),
            "ragged_cut": (cut, 64 << 10, 1, 32 << 10, False)}


def main() -> None:
    orc = oracle.Oracle()
    arrs, names = {}, []
    for name, (puts, hs, ht, mps, verify) in streams(orc).items():
        s = encode_stream(puts)
        files, refused = run_ref_keep_going(s, hs, ht, mps, verify)
        names.append(name)
        arrs[f"{name}__stream"] = np.frombuffer(s, np.uint8)
        arrs[f"{name}__opts"] = np.array([hs, ht, mps], np.uint64)
        arrs[f"{name}__files"] = np.array(list(files), dtype="U16")
        arrs[f"{name}__refused"] = np.array(refused, np.int64).reshape(-1, 2)
        for f, b in files.items():
            arrs[f"{name}__file_{f}"] = np.frombuffer(b, np.uint8)
        print(f"{name}: {len(puts)} puts, {len(files)} file(s), {sum(map(len, files.values()))} bytes, "
              f"refused {refused}")
    arrs["names"] = np.array(names, dtype="U16")
    np.savez_compressed(OUT, **arrs)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
