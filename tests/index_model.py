"""A Python model of Get by key, for the index tests (not a test module):
HSTableManager::LoadDatabase / LoadFile (storage/hstable_manager.h:906-1099),
StorageEngine::GetWithIndex / GetEntry (storage/storage_engine.h:424-521) and
Database::GetRaw's status mapping (interface/database.cc:9-75), with the
bounds rules of csrc/hstable_decode.h: an offset or a header that reaches past
the file is a decode error for that candidate, and sums of sizes do not wrap.

tests/test_index_model.py pins it to what the reference's own Database::Get
returned (tests/golden/get_keys.npz); after that it is the checker for
mutated files.  Also the helpers that build those mutations.
"""
from __future__ import annotations

import struct

from kingdb_amd import get as G

NOTFOUND, DELETED, MULTIPART = -3, -4, -5
HEADER, FOOTER, MAGIC = 8192, 36, 0x4D454F57
DECODE_ERROR, DECODE_CHECKSUM, DECODE_INVALID = -1, -2, -3


def varint(b: bytes, i: int, end: int, max_bytes: int, bits: int):
    """GetVarint32 / GetVarint64 (algorithm/coding.cc:143-188): (value, next) or None."""
    v = 0
    for n in range(max_bytes):
        if i + n >= end:
            return None
        c = b[i + n]
        v |= (c & 127) << (7 * n)
        if c < 128:
            return v & ((1 << bits) - 1), i + n + 1
    return None


def put_varint(v: int) -> bytes:
    out = bytearray()
    while v >= 128:
        out.append((v & 127) | 128)
        v >>= 7
    out.append(v)
    return bytes(out)


def locate_entry(f: bytes, off: int, verify: bool, orc):
    """(rc, fields): hstable_decode.h locate_entry.  fields = dict of the header."""
    size = len(f)
    if off >= size:
        return DECODE_ERROR, None
    if size - off < 5:
        return DECODE_ERROR, None
    h = {"checksum_header": f[off], "checksum": struct.unpack_from("<I", f, off + 1)[0]}
    i = off + 5
    for name, mb, bits in (("flags", 5, 32), ("size_key", 10, 64), ("size_value", 10, 64)):
        r = varint(f, i, size, mb, bits)
        if r is None:
            return DECODE_ERROR, None
        h[name], i = r
    if size - i < 8:
        return DECODE_ERROR, None
    h["svc"] = struct.unpack_from("<Q", f, i)[0]
    i += 8
    r = varint(f, i, size, 10, 64)
    if r is None:
        return DECODE_ERROR, None
    h["padding"], i = r
    if size - i < 8:
        return DECODE_ERROR, None
    h["hash"] = struct.unpack_from("<Q", f, i)[0]
    i += 8
    h["size_header"] = i - off
    if verify and orc.crc8(f[off + 1:i]) != h["checksum_header"]:
        return DECODE_CHECKSUM, h
    # AreSizesValid && IsEntryFull (format.h:105-108, storage_engine.h:491-495)
    if h["svc"] == 0 or (h["flags"] & 0x2):
        svo = h["size_value"] + h["padding"]
        if svo >= 1 << 64:
            return DECODE_INVALID, h
    else:
        svo = h["svc"]
    h["svo"] = svo
    if h["size_key"] == 0 or not (h["flags"] & 0x8) or i + h["size_key"] + svo > size:
        return DECODE_INVALID, h
    return 0, h


def footer(f: bytes):
    return struct.unpack_from("<IIQQQI", f, len(f) - FOOTER)


def parse_rows(f: bytes):
    """The rows of a file with a usable footer: [(hash, offset)]."""
    _, _, oi, num, _, _ = footer(f)
    rows, i, end = [], oi, len(f) - FOOTER
    for _ in range(num):
        a = varint(f, i, end, 10, 64)
        if a is None:
            return None
        b = varint(f, a[1], end, 5, 32)
        if b is None:
            return None
        rows.append((a[0], b[0]))
        i = b[1]
    return rows


def load_file(f: bytes, orc):
    """(status, rows, timestamp): the per-file status of kdb_index_load_files."""
    if len(f) <= HEADER:
        return -2, [], 0
    crc, major, minor, _ftype, ts = struct.unpack_from("<IIIIQ", f, 0)
    if (major, minor) != (1, 0) or orc.crc32c(f[4:24]) != crc:
        return -2, [], 0
    if len(f) < HEADER + FOOTER:
        return -1, [], ts
    _, _, oi, num, magic, fcrc = footer(f)
    if magic != MAGIC or not (HEADER <= oi <= len(f) - FOOTER):
        return -1, [], ts
    if orc.crc32c(f[oi:len(f) - 4]) != fcrc:
        return -1, [], ts
    if num > (len(f) - FOOTER - oi) // 2:
        return -3, [], ts
    rows = parse_rows(f)
    if rows is None:
        return -3, [], ts
    return 0, rows, ts


class Model:
    def __init__(self, files: dict, orc, hash_type: int = 1):
        self.files, self.orc = files, orc
        self.hash = orc.xxh64 if hash_type == 1 else orc.murmur3_64
        self.file_status, loaded = {}, []
        for name, f in files.items():
            st, rows, ts = load_file(f, orc)
            self.file_status[name] = st
            if st == 0:
                loaded.append((ts, int(name, 16), name, rows))
        loaded.sort()                       # LoadDatabase: by (timestamp, fileid)
        self.rows = [(h, name, off) for _, _, name, rows in loaded for h, off in rows]   # sequence order

    def pairs(self):
        return [(h, (int(name, 16) << 32) | off) for h, name, off in self.rows]

    def get(self, key: bytes, verify: int = 0, multipart_required: int = 1 << 20):
        """(status, value bytes, location)."""
        hk = self.hash(key)
        for h, name, off in reversed(self.rows):          # newest first
            if h != hk:
                continue
            f = self.files[name]
            rc, e = locate_entry(f, off, verify != 0, self.orc)
            if rc != 0:
                continue                                    # GetWithIndex:446 skips it
            at = off + e["size_header"]
            if f[at:at + e["size_key"]] != key:
                continue
            loc = (int(name, 16) << 32) | off
            if e["flags"] & 0x1:
                return DELETED, b"", loc
            if e["svc"] and e["size_value"] > multipart_required:
                return MULTIPART, b"", loc
            va = at + e["size_key"]
            st, val = self.orc.get_value(f[va:va + e["svo"]], e["svc"], e["size_value"], e["checksum"],
                                         self.orc.crc32c(key), verify)
            return st, val, loc
        return NOTFOUND, b"", 0


# ------------------------------------------------------------------ mutations
def with_rows(f: bytes, rows, orc, body: bytes | None = None) -> bytes:
    """The file with its offset array replaced by `rows` (and optionally the
    bytes before it by `body`), footer rebuilt with a valid CRC."""
    ftype, flags, oi, _, magic, _ = footer(f)
    body = f[:oi] if body is None else body
    arr = b"".join(put_varint(h) + put_varint(o) for h, o in rows)
    out = body + arr + struct.pack("<IIQQQ", ftype, flags, len(body), len(rows), magic)
    return out + struct.pack("<I", orc.crc32c((arr + out[-32:])))


def refooter(f: bytes, orc, num: int | None = None) -> bytes:
    """The file's footer CRC recomputed over what the file now holds."""
    ftype, flags, oi, n, magic, _ = footer(f)
    head = f[:len(f) - FOOTER] + struct.pack("<IIQQQ", ftype, flags, oi, n if num is None else num, magic)
    return head + struct.pack("<I", orc.crc32c(head[oi:]))


def entry_of(f: bytes, off: int) -> G.Entry:
    return G.decode_entry(f, off)


def hardened_set(files: dict, orc):
    """A copy of `files` whose newest file has five rows made hostile: offsets
    filesize, filesize - 3 and 0xFFFFFFF0, one into the middle of a value, and
    one entry whose size_key varint says 2^32 (its header CRC-8 left as it
    was, so wrong).  Returns (files, the keys of those five entries)."""
    name = sorted(files)[-1]
    f = files[name]
    rows = parse_rows(f)
    assert len(rows) >= 8
    pick = [1, 2, 3, 4, 5]
    ents = [entry_of(f, rows[i][1]) for i in pick]
    body = bytearray(f[:footer(f)[2]])
    e = ents[4]                                   # flags is one byte (0x8): size_key follows it
    assert body[e.offset + 5] < 128
    body[e.offset + 6:e.offset + 11] = bytes([0x80, 0x80, 0x80, 0x80, 0x10])
    size = len(f)
    for _ in range(4):                            # the file's size depends on the rows' varint lengths
        new = list(rows)
        new[pick[0]] = (rows[pick[0]][0], size)
        new[pick[1]] = (rows[pick[1]][0], size - 3)
        new[pick[2]] = (rows[pick[2]][0], 0xFFFFFFF0)
        new[pick[3]] = (rows[pick[3]][0], ents[3].value_at + max(ents[3].stored_len // 2, 1))
        out = with_rows(f, new, orc, bytes(body))
        if len(out) == size:
            break
        size = len(out)
    assert len(out) == size
    res = dict(files)
    res[name] = out
    return res, [e.key for e in ents]


def with_recovered_footer(f: bytes, orc) -> bytes:
    """A file the reference left without an offset array (a multipart value's
    last part never registered, hstable_manager.h:361-378), with the array and
    footer its recovery would append: one row per entry, walked from the
    header block (get.read_hstable)."""
    assert footer(f)[4] != MAGIC
    rows = [(e.hashed, e.offset) for e in G.read_hstable(f)]
    arr = b"".join(put_varint(h) + put_varint(o) for h, o in rows)
    out = f + arr + struct.pack("<IIQQQ", 1, 0, len(f), len(rows), MAGIC)
    return out + struct.pack("<I", orc.crc32c(arr + out[-32:]))
