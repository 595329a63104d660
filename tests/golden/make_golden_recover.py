#!/usr/bin/env python3
"""Golden fixture for file recovery: damaged HSTable files and what the
REFERENCE's own Database::Open (HSTableManager::LoadDatabase -> RecoverFile,
storage/hstable_manager.h:1024-1039, 1101-1185) leaves on disk for them.

Runs oracle/_ref/ref_db (built by __graft_entry__.build()) with its default
options: a database reopened takes its options from the db_options file, which
does not hold maximum_part_size, so only the defaults can be reopened.  Each
ref_db run on the same directory is one write session and adds one file; a run
with an empty stream opens, recovers and closes.

Two databases:
  sessions   three sessions of 120 puts: keys of 1-40 bytes, values of 1-400
             bytes, half of them incompressible, keys overwritten across
             sessions
  multipart  two sessions of 30 puts; every fifth is a 6000-byte value sent as
             chunks [2500, 2500, 1000]
For each case the directory is copied, one file damaged by a recipe
(recover_model.apply_ops), `ref_db <copy> <empty stream>` run, and recorded:
whether the file was removed; if kept, its size, CRC32C, offset_indexes and
every byte from there on.  The bytes before offset_indexes must be the damaged
input's (asserted here), so they are not stored.  The base files are stored
once.  A recipe whose input makes some uncompacted entry's CRC range leave
the file is undefined in the reference and is listed in `undefined`, not
recorded (none with the recipes below).

    python tests/golden/make_golden_recover.py      -> tests/golden/recover.npz
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle  # noqa: E402
import recover_model as R  # noqa: E402
from kingdb_amd import get as G  # noqa: E402
from make_golden_put import REF_DB, encode_stream  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "recover.npz")
HEXNAME = "0123456789abcdef"


def read_files(db: str) -> dict[str, bytes]:
    out = {}
    for name in sorted(os.listdir(db)):
        if len(name) == 8 and all(c in HEXNAME for c in name):
            with open(os.path.join(db, name), "rb") as f:
                out[name] = f.read()
    return out


def run_session(db: str, puts, tmp: str) -> None:
    sp = os.path.join(tmp, "stream.bin")
    with open(sp, "wb") as f:
        f.write(encode_stream(puts))
    subprocess.run([REF_DB, db, sp], check=True, capture_output=True)


def databases(orc, ref):
    pool = oracle.g1_pool(orc, 1 << 20)
    g3 = ref.g3(65536, 1).tobytes()
    rng = np.random.default_rng(23)
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

    keys = []
    for i in range(200):
        n = int(rng.integers(1, 41))
        keys.append((b"k%d-" % i + bytes(rng.integers(97, 123, 40, dtype=np.uint8)))[:n] if n > 4 else
                    bytes(rng.integers(0, 256, n, dtype=np.uint8)))
    keys = list(dict.fromkeys(keys))
    sessions = []
    for s in range(3):
        puts = []
        for i in range(120):
            k = keys[(s * 70 + i) % len(keys)]             # later sessions overwrite earlier keys
            puts.append((k, value(int(rng.integers(1, 401)), i % 2 == 1), None))
        sessions.append(puts)
    multipart = []
    for s in range(2):
        puts = []
        for i in range(30):
            k = b"mp%02d-%03d" % (s, i)
            if i % 5 == 2:
                puts.append((k, value(6000, i % 10 == 7), [2500, 2500, 1000]))
            else:
                puts.append((k, value(int(rng.integers(1, 401)), i % 2 == 1), None))
        multipart.append(puts)
    return {"sessions": sessions, "multipart": multipart}


def recipes(f: bytes, orc, rng, blob: bytearray):
    """[(name, ops)] for one intact file."""
    _, _, oi, num, magic, _ = struct.unpack_from("<IIQQQI", f, len(f) - 36)
    assert magic == R.MAGIC
    ents = G.read_hstable(f)
    assert len(ents) == num and num >= 20
    size = len(f)
    mid = ents[num // 2]
    plain = [e for e in ents if not e.flags & R.UNCOMPACTED and e.stored_len >= 4]
    multi = [e for e in ents if e.flags & R.UNCOMPACTED]
    longkey = max(ents[3:], key=lambda e: len(e.key))

    def append(data: bytes):
        at = len(blob)
        blob.extend(data)
        return (R.OP_APPEND, at, len(data))

    out = [(f"torn{n}", [(R.OP_TRUNC, size - n, 0)]) for n in (1, 4, 35)]
    out += [("cut_at_offset_indexes", [(R.OP_TRUNC, oi, 0)]),
            ("cut_mid_row", [(R.OP_TRUNC, oi + (size - 36 - oi) // 2 + 1, 0)]),
            ("cut_header3", [(R.OP_TRUNC, mid.offset + 3, 0)]),
            ("cut_header24", [(R.OP_TRUNC, mid.offset + 24, 0)]),
            ("cut_in_key", [(R.OP_TRUNC, longkey.offset + longkey.header_size + len(longkey.key) // 2, 0)]),
            ("cut_in_value", [(R.OP_TRUNC, plain[len(plain) // 2].value_at + plain[len(plain) // 2].stored_len // 2, 0)]),
            ("cut_on_boundary", [(R.OP_TRUNC, mid.offset, 0)]),
            ("cut_8202", [(R.OP_TRUNC, 8192 + 10, 0)]),
            ("footer_crc_flipped", [(R.OP_FLIP, size - 2, 3)]),
            # (a flip alone leaves the footer intact and the file is loaded, not recovered: tear 4 bytes too)
            ("flip_entry_header", [(R.OP_FLIP, mid.offset + 6, 1), (R.OP_TRUNC, size - 4, 0)]),
            ("flip_plain_value", [(R.OP_FLIP, plain[len(plain) // 3].value_at + 1, 5), (R.OP_TRUNC, size - 4, 0)])]
    if multi:
        e = multi[len(multi) // 2]
        out.append(("flip_multipart_value", [(R.OP_FLIP, e.value_at + e.stored_len // 2, 2), (R.OP_TRUNC, size - 4, 0)]))
        # (an incompressible multipart value fills its space to the last byte: take one that leaves room)
        e = max(multi, key=lambda m: m.size_value + m.size_padding - m.stored_len)
        room = e.size_value + e.size_padding - e.stored_len
        assert room > 0
        out.append(("flip_multipart_padding", [(R.OP_FLIP, e.value_at + e.stored_len + room // 2, 6),
                                               (R.OP_TRUNC, size - 4, 0)]))
    out += [("zeros50", [(R.OP_TRUNC, oi, 0), append(bytes(50))]),
            ("zeros5000", [(R.OP_TRUNC, oi, 0), append(bytes(5000))]),
            ("random64", [(R.OP_TRUNC, oi, 0), append(bytes(rng.integers(0, 256, 64, dtype=np.uint8)))])]
    # filetype 4 (kCompactedLargeType) with the header CRC redone; the footer torn so that the file is recovered at all
    hdr = bytearray(f[:24])
    struct.pack_into("<I", hdr, 12, 4)
    struct.pack_into("<I", hdr, 0, orc.crc32c(bytes(hdr[4:24])))
    a = len(blob)
    blob.extend(hdr[12:16])
    blob.extend(hdr[0:4])
    out.append(("large_type_torn4", [(R.OP_PATCH, 12, a), (R.OP_PATCH, 0, a + 4), (R.OP_TRUNC, size - 4, 0)]))
    return out


def main() -> None:
    orc, ref = oracle.Oracle(), oracle.Reference()
    rng = np.random.default_rng(5)
    tmp = tempfile.mkdtemp(prefix="kdbrecover")
    arrs = {}
    base_names, case_names, case_base, case_ops, ops, expect, undefined = [], [], [], [], [], [], []
    blob, tails = bytearray(), bytearray()
    try:
        empty = os.path.join(tmp, "empty.bin")
        open(empty, "wb").close()
        for dbname, sessions in databases(orc, ref).items():
            db = os.path.join(tmp, dbname)
            for puts in sessions:
                run_session(db, puts, tmp)
            files = read_files(db)
            assert len(files) == len(sessions), (dbname, list(files))
            print(f"{dbname}: {len(files)} files, {sum(map(len, files.values()))} bytes")
            # an untouched reopen changes nothing
            copy = os.path.join(tmp, "copy")
            shutil.copytree(db, copy)
            subprocess.run([REF_DB, copy, empty], check=True, capture_output=True)
            assert read_files(copy) == files
            shutil.rmtree(copy)
            picked = sorted(files) if dbname == "multipart" else [sorted(files)[0], sorted(files)[-1]]
            for fname in sorted(files):
                base_names.append(f"{dbname}_{fname}")
                arrs[f"base__{dbname}_{fname}"] = np.frombuffer(files[fname], np.uint8)
            for fname in picked:
                for rname, rops in recipes(files[fname], orc, rng, blob):
                    name = f"{dbname}/{fname}/{rname}"
                    damaged = R.apply_ops(files[fname], rops, bytes(blob))
                    if R.walk(damaged, orc)[2]:
                        undefined.append(name)
                        continue
                    shutil.copytree(db, copy)
                    with open(os.path.join(copy, fname), "wb") as f:
                        f.write(damaged)
                    subprocess.run([REF_DB, copy, empty], check=True, capture_output=True)
                    after = read_files(copy)
                    shutil.rmtree(copy)
                    assert {k: v for k, v in after.items() if k != fname} == \
                        {k: v for k, v in files.items() if k != fname}, name
                    case_names.append(name)
                    case_base.append(f"{dbname}_{fname}")
                    case_ops.append((len(ops), len(ops) + len(rops)))
                    ops.extend(rops)
                    if fname not in after:
                        expect.append((1, 0, 0, 0, 0, 0))
                        print(f"   {name}: removed")
                        continue
                    got = after[fname]
                    _, fl, oi, num, magic, _ = struct.unpack_from("<IIQQQI", got, len(got) - 36)
                    assert magic == R.MAGIC and got[:oi] == damaged[:oi], name
                    expect.append((0, len(got), orc.crc32c(got), oi, len(tails), len(tails) + len(got) - oi))
                    tails.extend(got[oi:])
                    print(f"   {name}: {len(damaged)} -> {len(got)} bytes, offset_indexes {oi}, {num} rows, flags {fl}")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert len(undefined) * 20 <= len(case_names) + len(undefined), undefined
    arrs["base_names"] = np.array(base_names, dtype="U32")
    arrs["case_names"] = np.array(case_names, dtype="U64")
    arrs["case_base"] = np.array(case_base, dtype="U32")
    arrs["case_ops"] = np.array(case_ops, np.int64).reshape(-1, 2)
    arrs["ops"] = np.array(ops, np.int64).reshape(-1, 3)
    arrs["expect"] = np.array(expect, np.int64).reshape(-1, 6)
    arrs["blob"] = np.frombuffer(bytes(blob), np.uint8)
    arrs["tails"] = np.frombuffer(bytes(tails), np.uint8)
    arrs["undefined"] = np.array(undefined, dtype="U64")
    np.savez_compressed(OUT, **arrs)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(case_names)} cases, {len(undefined)} undefined")


if __name__ == "__main__":
    main()
