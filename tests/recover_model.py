"""A Python model of file recovery, for the recovery tests (not a test module):
HSTableManager::RecoverFile (storage/hstable_manager.h:1101-1185) with
WriteOffsetArray (:381-428), under the bounds rules of csrc/hstable_decode.h.

  walk(f, orc, scope)     the entry walk from byte 8192: (entries, stop offset)
  recover(f, orc, scope)  (status, recovered bytes or None, report)

scope "reference" is RecoverFile's CRC range [offset + 5, end of the used
value), which never equals checksum_content (CRC32C over key || stored value,
interface/database.cc:250-257): the reference drops every uncompacted entry.
scope "content" checks what PutPartValidSize computed.

tests/test_recover_model.py pins it to what the reference's own Database::Open
left on disk (tests/golden/recover.npz); after that it is the checker for the
files the GPU tests build.  Also the fixture's recipes (apply_ops).
"""
from __future__ import annotations

import struct

import index_model as M

HEADER, FOOTER, MAGIC = M.HEADER, M.FOOTER, M.MAGIC
NOENTRY, LARGE, BADHEADER = -6, -7, -8       # KDB_RECOVER_NOENTRY, KDB_RECOVER_LARGE, KDB_RECOVER_BADHEADER
UNCOMPACTED, PADDING = 0x2, 0x4
OP_TRUNC, OP_FLIP, OP_APPEND, OP_PATCH = 0, 1, 2, 3


def step(f: bytes, off: int, orc):
    """hstable_recover.h recover_step: (header fields, next offset) or None (the walk stops)."""
    size = len(f)
    if off >= size or size - off < 5:
        return None
    h = {"checksum_header": f[off], "checksum": struct.unpack_from("<I", f, off + 1)[0]}
    i = off + 5
    for name, mb, bits in (("flags", 5, 32), ("size_key", 10, 64), ("size_value", 10, 64)):
        r = M.varint(f, i, size, mb, bits)
        if r is None:
            return None
        h[name], i = r
    if size - i < 8:
        return None
    h["svc"] = struct.unpack_from("<Q", f, i)[0]
    i += 8
    r = M.varint(f, i, size, 10, 64)
    if r is None:
        return None
    h["padding"], i = r
    if size - i < 8:
        return None
    h["hash"] = struct.unpack_from("<Q", f, i)[0]
    i += 8
    h["size_header"] = i - off
    if orc.crc8(f[off + 1:i]) != h["checksum_header"]:
        return None
    svo = h["size_value"] + h["padding"] if (h["svc"] == 0 or h["flags"] & UNCOMPACTED) else h["svc"]
    if svo >= 1 << 64 or h["size_key"] == 0 or i + h["size_key"] + svo > size:      # AreSizesValid, no wrap
        return None
    h["svu"] = h["svc"] if h["svc"] else h["size_value"]
    return h, i + h["size_key"] + svo


def crc_range(h: dict, off: int, scope: str):
    """(begin, length) of the bytes the content CRC covers."""
    if scope == "reference":
        return off + 5, h["size_header"] - 5 + h["size_key"] + h["svu"]
    return off + h["size_header"], h["size_key"] + h["svu"]


def walk(f: bytes, orc, scope: str = "reference"):
    """([(offset, header fields, kept)], stop offset, some CRC range left the file)."""
    out, off, undefined = [], HEADER, False
    while True:
        r = step(f, off, orc)
        if r is None:
            return out, off, undefined
        h, nxt = r
        kept = True
        if h["flags"] & UNCOMPACTED:
            a, n = crc_range(h, off, scope)
            if a + n > len(f):
                kept, undefined = False, True
            else:
                kept = orc.crc32c(f[a:a + n]) == h["checksum"]
        out.append((off, h, kept))
        off = nxt


def footer_filetype(filetype: int) -> int:
    """HSTableHeader::GetFileType (format.h:362-371)."""
    for t in (4, 2, 1):
        if filetype & t:
            return t
    return 0


def bound(size: int) -> int:
    """kdb_hstable_recover_bound."""
    n = size + 15 * ((size - HEADER) // 26 if size > HEADER else 0) + FOOTER
    return (n + 63) & ~63


def recover(f: bytes, orc, scope: str = "reference"):
    """(status, bytes | None, report): 0 and the recovered file, NOENTRY or
    LARGE (the reference removes the file), or BADHEADER (it skips the file
    and leaves it as it is)."""
    report = {"walked": 0, "kept": 0, "invalid": 0, "offset": 0, "flags": 0}
    if len(f) <= HEADER:
        return BADHEADER, None, report       # LoadDatabase skips it (hstable_manager.h:1000-1005): left on disk
    crc, major, minor, ftype, _ = struct.unpack_from("<IIIIQ", f, 0)
    if (major, minor) != (1, 0) or orc.crc32c(f[4:24]) != crc:
        return BADHEADER, None, report
    if ftype & 4:
        return LARGE, None, report
    ents, stop, _ = walk(f, orc, scope)
    rows = [(h["hash"], off) for off, h, kept in ents if kept]
    flags = (1 if any(h["flags"] & PADDING for _, h, _ in ents) else 0) | (2 if len(rows) < len(ents) else 0)
    report = {"walked": len(ents), "kept": len(rows), "invalid": len(ents) - len(rows), "offset": stop,
              "flags": flags}
    if stop <= HEADER:
        return NOENTRY, None, report
    arr = b"".join(M.put_varint(h) + M.put_varint(o) for h, o in rows)
    tail = arr + struct.pack("<IIQQQ", footer_filetype(ftype), flags, stop, len(rows), MAGIC)
    return 0, f[:stop] + tail + struct.pack("<I", orc.crc32c(tail)), report


def apply_ops(f: bytes, ops, blob: bytes) -> bytes:
    """The fixture's recipes: rows of (op, a, b) applied in order.  OP_TRUNC:
    cut to a bytes; OP_FLIP: flip bit b of byte a; OP_APPEND: append
    blob[a:a + b]; OP_PATCH: overwrite from byte a with blob[b:b + 4]."""
    b_ = bytearray(f)
    for op, a, b in ops:
        op, a, b = int(op), int(a), int(b)
        if op == OP_TRUNC:
            del b_[a:]
        elif op == OP_FLIP:
            b_[a] ^= 1 << b
        elif op == OP_APPEND:
            b_ += blob[a:a + b]
        elif op == OP_PATCH:
            b_[a:a + 4] = blob[b:b + 4]
        else:
            raise ValueError(op)
    return bytes(b_)


def load_cases(z):
    """The cases of tests/golden/recover.npz: [(name, damaged bytes, expected)]
    with expected = None (the reference removed the file) or (size, crc32c,
    offset_indexes, tail bytes)."""
    blob = z["blob"].tobytes()
    tails = z["tails"].tobytes()
    base = {str(n): z[f"base__{n}"].tobytes() for n in z["base_names"]}
    out = []
    for i, name in enumerate(str(n) for n in z["case_names"]):
        lo, hi = (int(x) for x in z["case_ops"][i])
        f = apply_ops(base[str(z["case_base"][i])], z["ops"][lo:hi], blob)
        removed, size, crc, oi, t0, t1 = (int(x) for x in z["expect"][i])
        out.append((name, f, None if removed else (size, crc, oi, tails[t0:t1])))
    return out
