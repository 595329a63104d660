#!/usr/bin/env python3
"""Golden fixture for deletes: op streams of puts and Database::Delete calls,
the HSTable files the REFERENCE writes for them, and the status code its own
Database::Get returns for every key, before and after a crash recovery.

Compiles tests/cpp/ref_ops_main.cc (our own driver) with g++ -std=c++11 -O2
against the reference objects `make -C oracle ref` leaves in oracle/_ref/obj/
(__graft_entry__.build() makes them) into oracle/_ref/ref_ops, runs it on each
stream, reads the files it leaves, and runs `ref_ops --get` on a COPY of the
directory whose db_options file has its hstable_size raised
(make_golden_getkeys.raise_hstable_size explains why; the HSTable files are
not touched).

    python tests/golden/make_golden_deletes.py      -> tests/golden/deletes.npz

A reference delete entry is EntryHeader || key with flags 0x9 and every other
field 0 -- but size_padding and hash are 0 only because the reference never
assigns them (EntryHeader() sets flags alone, storage/format.h:46) and the
stack happened to hold 0.  This script ABORTS if any delete entry of any file
has a nonzero size_padding or hash: such a fixture would pin garbage.

Streams, all with 64 KiB HSTables and 16 KiB parts:
  mixed    300 ops over 100 sixteen-byte keys, xxHash-64: a delete as the very
           first op; deletes of keys put earlier in the same file and in an
           earlier file; a delete of a key never put; deletes followed by a
           new put of the key; a delete of a key whose value came in three chunks
  lengths  a put and then a delete for keys of 1, 2, 127, 128, 129, 511, 512,
           513, 1000 and 16384 bytes (the size_key varint at 1, 2 and 3 bytes;
           both sides of put.hip's kSmallEntry = 512)
  cuts     3000 deletes of 16-byte keys with a few puts between them: a file
           that holds only deletes, a file whose first entry is a delete, and a
           file whose last entry -- the one that takes the file past its size
           -- is a delete (all three asserted)
  murmur   60 ops with MurmurHash3-64
  torn     the `mixed` database's last file cut right after a delete entry,
           inside that entry's key and inside its header, each reopened by the
           reference (the procedure of make_golden_recover.py): the recovered
           file and the Get codes after the recovery.  The delete that
           survives the first cut is filed under its header's hash, 0, so the
           key it deleted is back.

Per stream NAME: NAME__stream (ops.bin, the format ref_ops_main.cc documents),
NAME__opts (hstable_size, hash type, part size), NAME__files and NAME__file_F,
NAME__keys / NAME__key_len (the distinct keys in order of first appearance,
concatenated), NAME__code (util/status.h: 0 OK, 1 NotFound, 2 DeleteOrder),
NAME__len and NAME__crc (length and CRC32C of the value, code 0 only).
torn__cut, torn__file_I, torn__code_I, torn__len_I, torn__crc_I for cut I.
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
from kingdb_amd import get as G  # noqa: E402
from make_golden_getkeys import raise_hstable_size  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "deletes.npz")
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
REF_OPS = os.path.join(REF_DIR, "ref_ops")
DRIVER = os.path.join(ROOT, "tests", "cpp", "ref_ops_main.cc")
REF = os.environ.get("REF", "/root/reference")
HSTABLE_SIZE, PART_SIZE = 64 << 10, 16 << 10
DELETE = None                                   # an op is (key, value bytes | DELETE, chunks | None)
DELETE_MARK = (1 << 64) - 1
# oracle/Makefile's REF_OBJS and REF_DB_OBJS
OBJS = ["lz4", "compressor", "crc32c", "coding", "endian", "logger", "status", "debug", "database", "write_buffer",
        "hash", "xxhash", "murmurhash3"]


def build_driver() -> None:
    objs = [os.path.join(REF_DIR, "obj", o + ".o") for o in OBJS]
    missing = [o for o in objs if not os.path.exists(o)]
    if missing:
        raise SystemExit(f"run `make -C oracle ref` first: missing {missing}")
    subprocess.run(["g++", "-std=c++11", "-O2", "-w", f"-I{REF}", f"-I{REF}/include", "-o", REF_OPS, DRIVER] + objs +
                   ["-lpthread"], check=True)


def encode_ops(ops) -> bytes:
    out = bytearray()
    for k, v, ch in ops:
        if v is DELETE:
            out += struct.pack("<I", len(k)) + k + struct.pack("<QI", DELETE_MARK, 0)
            continue
        ch = [len(v)] if ch is None else ch
        out += struct.pack("<I", len(k)) + k + struct.pack("<QI", len(v), len(ch))
        o = 0
        for c in ch:
            out += struct.pack("<I", c) + v[o:o + c]
            o += c
    return bytes(out)


def decode_ops(b: bytes):
    """The ops of a stream: [(key, value | None for a delete, chunks)]."""
    ops, i = [], 0
    while i < len(b):
        (kl,) = struct.unpack_from("<I", b, i)
        k = b[i + 4:i + 4 + kl]
        i += 4 + kl
        size, nch = struct.unpack_from("<QI", b, i)
        i += 12
        if size == DELETE_MARK:
            assert nch == 0
            ops.append((k, None, None))
            continue
        v, ch = bytearray(), []
        for _ in range(nch):
            (cl,) = struct.unpack_from("<I", b, i)
            v += b[i + 4:i + 4 + cl]
            i += 4 + cl
            ch.append(cl)
        assert len(v) == size
        ops.append((k, bytes(v), ch))
    return ops


def read_files(db: str) -> dict[str, bytes]:
    out = {}
    for name in sorted(os.listdir(db)):
        if len(name) == 8 and all(c in "0123456789abcdef" for c in name):
            with open(os.path.join(db, name), "rb") as f:
                out[name] = f.read()
    return out


def decode_gets(b: bytes):
    """ref_ops --get's output: [(key, code, value)]."""
    out, i = [], 0
    while i < len(b):
        (kl,) = struct.unpack_from("<I", b, i)
        k = b[i + 4:i + 4 + kl]
        i += 4 + kl
        code, vl = struct.unpack_from("<iQ", b, i)
        i += 12
        out.append((k, code, b[i:i + vl]))
        i += vl
    return out


def ref_get(orc, db: str, sp: str, tmp: str, damage=None):
    """Database::Get of every key on a copy of `db` (one file optionally
    replaced first): ([(key, code, value)], the copy's files after the run)."""
    copy = os.path.join(tmp, "copy")
    shutil.copytree(db, copy)
    try:
        raise_hstable_size(orc, os.path.join(copy, "db_options"))
        if damage is not None:
            with open(os.path.join(copy, damage[0]), "wb") as f:
                f.write(damage[1])
        out = os.path.join(tmp, "gets.bin")
        subprocess.run([REF_OPS, "--get", copy, sp, out], check=True, capture_output=True)
        with open(out, "rb") as f:
            return decode_gets(f.read()), read_files(copy)
    finally:
        shutil.rmtree(copy, ignore_errors=True)


def expected(ops):
    """{key: value | None} in order of first appearance: the last op wins."""
    last = {}
    for k, v, _ in ops:
        last[k] = v
    return last


def check_gets(gets, ops, name: str) -> None:
    want = expected(ops)
    assert [k for k, _, _ in gets] == list(want), name
    for k, code, val in gets:
        if want[k] is DELETE:
            # a delete entry in a file answers kDeleteOrder whether or not the key was ever put
            assert code == 2 and val == b"", (name, k, code)
        else:
            assert code == 0 and val == want[k], (name, k, code, len(val))


def check_delete_entries(files: dict[str, bytes], name: str) -> int:
    """ABORTS on a delete entry that carries the uninitialised pair."""
    n = 0
    for fname, f in files.items():
        # the other bytes the reference never writes: its write buffer's header block past the 72 encoded
        # bytes (zero as long as the driver has not used the heap before Database::Open)
        if any(f[72:G.HEADER_SIZE]):
            raise SystemExit(f"{name}/{fname}: the header block holds heap garbage past byte 72")
        for e in G.read_hstable(f):
            if e.flags & 0x1:
                n += 1
                if e.size_padding != 0 or e.hashed != 0:
                    raise SystemExit(f"{name}/{fname} offset {e.offset}: delete entry with size_padding "
                                     f"{e.size_padding}, hash {e.hashed:#x}: the reference's uninitialised fields are "
                                     "not 0 in this build; refusing to write a fixture of stack garbage")
                assert e.flags == 0x9 and e.checksum == 0 and e.size_value == 0 and e.size_value_compressed == 0, \
                    (name, fname, e)
    return n


def run_stream(orc, name: str, ops, hash_type: int, tmp: str):
    sp = os.path.join(tmp, f"{name}.bin")
    stream = encode_ops(ops)
    assert [(k, v, c) for k, v, c in decode_ops(stream)] == \
        [(k, v, None if v is DELETE else (c or [len(v)])) for k, v, c in ops]
    with open(sp, "wb") as f:
        f.write(stream)
    db = os.path.join(tmp, f"db_{name}")
    subprocess.run([REF_OPS, db, sp, str(PART_SIZE), str(HSTABLE_SIZE), str(hash_type)], check=True,
                   capture_output=True)
    files = read_files(db)
    ndel = check_delete_entries(files, name)
    assert ndel == sum(1 for _, v, _ in ops if v is DELETE), name
    assert sum(len(G.read_hstable(f)) for f in files.values()) == len(ops), name     # one entry per op
    gets, after = ref_get(orc, db, sp, tmp)
    assert after == files, name                  # an untouched reopen changes nothing
    check_gets(gets, ops, name)
    return stream, files, gets, db, sp


def make_streams(orc, ref):
    pool = oracle.g1_pool(orc, 1 << 20)
    g3 = ref.g3(65536, 1).tobytes()
    rng = np.random.default_rng(29)
    pos = [0]

    def value(n: int, incompressible: bool = False) -> bytes:
        if incompressible:
            o = int(rng.integers(0, len(g3) - n))
            return g3[o:o + n]
        if pos[0] + n > len(pool):
            pos[0] = 0
        v = pool[pos[0]:pos[0] + n].tobytes()
        pos[0] += n
        return v

    def mix(nops: int, nkeys: int, tag: bytes):
        """A delete first, then puts of fresh keys, overwrites and deletes of random keys."""
        key = lambda i: tag + b"%013d" % i                                   # noqa: E731
        ops = [(key(0), DELETE, None)]
        sizes = rng.choice([100, 150, 300, 700, 1000, 2000, 4096], nops, p=[.2, .15, .2, .15, .1, .1, .1])
        fresh = 1
        for i in range(1, nops):
            r = rng.random()
            if fresh < nkeys and (r < 0.4 or fresh < 8):
                ops.append((key(fresh), value(int(sizes[i]), i % 6 == 5), None))
                fresh += 1
            elif r < 0.7:
                ops.append((key(int(rng.integers(0, fresh))), DELETE, None))
            else:
                ops.append((key(int(rng.integers(0, fresh))), value(int(sizes[i]), i % 6 == 5), None))
        return ops

    out = {}
    mixed = mix(300, 100, b"key")
    # a value in three chunks, deleted later; a key that is never put; a delete followed by a put
    mixed[40] = (b"key-three-chunks", value(3000), [1000, 1000, 1000])
    mixed[120] = (b"key-three-chunks", DELETE, None)
    mixed[60] = (b"key-never-put---", DELETE, None)
    mixed[200] = (b"key-back-again--", value(300), None)
    mixed[230] = (b"key-back-again--", DELETE, None)
    mixed[260] = (b"key-back-again--", value(150, True), None)
    out["mixed"] = (mixed, 1)

    lengths = []
    for i, n in enumerate([1, 2, 127, 128, 129, 511, 512, 513, 1000, 16384]):
        k = (b"L%d-" % n + bytes(rng.integers(97, 123, n, dtype=np.uint8)))[:n]
        lengths.append((k, value(50 + i), None))
        lengths.append((k, DELETE, None))
    out["lengths"] = (lengths, 1)

    cuts = []
    for i in range(3000):
        cuts.append((b"cut%013d" % (i % 2500), DELETE, None))
        if i in (5, 700, 2950, 2990):           # (a file takes about 1400 deletes: the second holds nothing else)
            cuts.append((b"cut%013d" % (i + 1), value(200), None))
    out["cuts"] = (cuts, 1)
    out["murmur"] = (mix(60, 25, b"mur"), 0)
    return out


def check_mixed(ops, files) -> None:
    """The situations the `mixed` stream is there for."""
    assert ops[0][1] is DELETE
    ever_put = {k for k, v, _ in ops if v is not DELETE}
    assert any(v is DELETE and k not in ever_put for k, v, _ in ops)
    state, seen_del_then_put, three = {}, False, False
    for k, v, ch in ops:
        if v is not DELETE and state.get(k, 0) is DELETE:
            seen_del_then_put = True
        if v is DELETE and state.get(k) == 3:
            three = True
        state[k] = DELETE if v is DELETE else (len(ch) if ch else 1)
    assert seen_del_then_put and three
    # where the put a delete removes lies: the same file, and an earlier one
    where, same, earlier = {}, False, False
    for fname in sorted(files):
        for e in G.read_hstable(files[fname]):
            if e.flags & 0x1:
                if where.get(e.key) == fname:
                    same = True
                elif where.get(e.key) is not None:
                    earlier = True
                where[e.key] = None
            else:
                where[e.key] = fname
    assert same and earlier and len(files) >= 3, (same, earlier, len(files))


def check_cuts(files) -> None:
    names = sorted(files)
    ents = {f: G.read_hstable(files[f]) for f in names}
    assert len(names) >= 3
    assert any(all(e.flags & 0x1 for e in ents[f]) for f in names), "no file holds only deletes"
    assert any(ents[f][0].flags & 0x1 for f in names[1:]), "no later file starts with a delete"
    # every file but the last was closed by the entry that took offset_end_ past size_block_
    assert any(ents[f][-1].flags & 0x1 for f in names[:-1]), "no file was closed by a delete"


def main() -> None:
    build_driver()
    orc, ref = oracle.Oracle(), oracle.Reference()
    tmp = tempfile.mkdtemp(prefix="kdbdeletes")
    arrs, names = {}, []
    try:
        for name, (ops, ht) in make_streams(orc, ref).items():
            stream, files, gets, db, sp = run_stream(orc, name, ops, ht, tmp)
            if name == "mixed":
                check_mixed(ops, files)
                mixed = (ops, files, db, sp)
            if name == "cuts":
                check_cuts(files)
            names.append(name)
            arrs[f"{name}__stream"] = np.frombuffer(stream, np.uint8)
            arrs[f"{name}__opts"] = np.array([HSTABLE_SIZE, ht, PART_SIZE], np.uint64)
            arrs[f"{name}__files"] = np.array(list(files), dtype="U16")
            for f, b in files.items():
                arrs[f"{name}__file_{f}"] = np.frombuffer(b, np.uint8)
            arrs[f"{name}__keys"] = np.frombuffer(b"".join(k for k, _, _ in gets), np.uint8)
            arrs[f"{name}__key_len"] = np.array([len(k) for k, _, _ in gets], np.uint32)
            arrs[f"{name}__code"] = np.array([c for _, c, _ in gets], np.int32)
            arrs[f"{name}__len"] = np.array([len(v) for _, _, v in gets], np.uint64)
            arrs[f"{name}__crc"] = np.array([orc.crc32c(v) for _, _, v in gets], np.uint32)
            ndel = sum(1 for _, v, _ in ops if v is DELETE)
            print(f"{name}: {len(ops)} ops ({ndel} deletes), {len(gets)} keys, {len(files)} file(s), "
                  f"{sum(map(len, files.values()))} bytes")

        # torn: the last file of `mixed`, cut at a delete whose key is live before it
        ops, files, db, sp = mixed
        last = sorted(files)[-1]
        ents = G.read_hstable(files[last])
        assert not any(e.flags & 0x2 for e in ents), "a multipart entry in the last file: recovery would drop it"
        before = sum(len(G.read_hstable(files[f])) for f in sorted(files)[:-1])
        pick = None
        for j, e in enumerate(ents):
            if e.flags & 0x1 and j >= len(ents) // 3 and expected(ops[:before + j]).get(e.key, DELETE) is not DELETE:
                pick = (j, e)
                break
        assert pick is not None
        j, e = pick
        cut_at = [e.value_at, e.offset + e.header_size + len(e.key) // 2, e.offset + 10]
        arrs["torn__cut"] = np.array(cut_at, np.uint64)
        arrs["torn__base"] = np.array([last], dtype="U16")
        for i, cut in enumerate(cut_at):
            damaged = files[last][:cut]
            gets, after = ref_get(orc, db, sp, tmp, (last, damaged))
            assert {k: v for k, v in after.items() if k != last} == {k: v for k, v in files.items() if k != last}
            got = after[last]
            _, _, oi, num, magic, _ = struct.unpack_from("<IIQQQI", got, len(got) - 36)
            survive = j + 1 if i == 0 else j
            assert magic == G.MAGIC and oi == (e.value_at if i == 0 else e.offset) and num == survive
            assert got[:oi] == damaged[:oi]
            # what a recovery that kept every surviving op reachable would answer, and where the reference differs
            want = expected(ops[:before + survive])
            differs = []
            for k, code, val in gets:
                w = want.get(k, "absent")
                wcode = 1 if w == "absent" else 2 if w is DELETE else 0
                if code != wcode:
                    differs.append((k, code, wcode))
                else:
                    assert w in ("absent", DELETE) or val == w
            # only deletes of the recovered file go missing (filed under hash 0): the key is back, or not found
            assert all(w == 2 and c in (0, 1) for _, c, w in differs), differs
            if i == 0:
                assert (e.key, 0, 2) in differs, differs
            arrs[f"torn__file_{i}"] = np.frombuffer(got, np.uint8)
            arrs[f"torn__code_{i}"] = np.array([c for _, c, _ in gets], np.int32)
            arrs[f"torn__len_{i}"] = np.array([len(v) for _, _, v in gets], np.uint64)
            arrs[f"torn__crc_{i}"] = np.array([orc.crc32c(v) for _, _, v in gets], np.uint32)
            print(f"torn {i}: {last} cut at {cut} -> {len(got)} bytes, {num} rows; keys back after their delete: "
                  f"{[d[0] for d in differs]}")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    arrs["names"] = np.array(names, dtype="U16")
    np.savez_compressed(OUT, **arrs)
    size = os.path.getsize(OUT)
    print("wrote", OUT, size, "bytes")
    assert size < 400_000


if __name__ == "__main__":
    main()
