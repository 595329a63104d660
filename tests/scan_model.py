"""A Python model of the scan (include/kdb_scan.h), for the scan tests (not a
test module), built on index_model.Model.

Row r (sequence number r of Model.rows) is live iff Model.get, run on the key
stored in r's entry, selects row r with status 0 or MULTIPART: liveness is by
sequence number, not by location.  The scan returns the live rows ordered by
(file rank in sequence order, offset ascending).

tests/test_scan_model.py pins it to the reference: on the files the reference
wrote it returns exactly the distinct keys with their last values, as many as
the reference's own iterator visited (tests/golden/scan.npz).
"""
from __future__ import annotations

import index_model as M


def select(model: M.Model, key: bytes, verify: int):
    """The sequence number Model.get(key) selects, with the entry's header, or (None, None)."""
    hk = model.hash(key)
    for r in range(len(model.rows) - 1, -1, -1):          # newest first
        h, name, off = model.rows[r]
        if h != hk:
            continue
        f = model.files[name]
        rc, e = M.locate_entry(f, off, verify != 0, model.orc)
        if rc != 0:
            continue
        at = off + e["size_header"]
        if f[at:at + e["size_key"]] != key:
            continue
        return r, e
    return None, None


def live_rows(model: M.Model, verify: int = 0):
    """[(file rank, offset, name, key)] of the live rows, in iterator order."""
    rank, out = {}, []
    for _, name, _ in model.rows:
        rank.setdefault(name, len(rank))                   # rows are in sequence order, file by file
    for r, (_, name, off) in enumerate(model.rows):
        f = model.files[name]
        rc, e = M.locate_entry(f, off, verify != 0, model.orc)
        if rc != 0 or e["flags"] & 0x1:
            continue
        at = off + e["size_header"]
        key = f[at:at + e["size_key"]]
        sel, _ = select(model, key, verify)
        if sel == r:
            out.append((rank[name], off, name, key))
    out.sort(key=lambda x: (x[0], x[1]))
    return out


def scan(model: M.Model, verify: int = 0, multipart_required: int = 1 << 20):
    """[(key, status, value)] in iterator order."""
    res = []
    for _, off, name, key in live_rows(model, verify):
        st, val, loc = model.get(key, verify, multipart_required)
        assert loc == (int(name, 16) << 32) | off
        res.append((key, st, val))
    return res


def prepare(model: M.Model, verify: int = 0):
    """(live, key bytes, max key length): what kdb_index_scan_prepare reports."""
    keys = [k for _, _, _, k in live_rows(model, verify)]
    return len(keys), sum(map(len, keys)), max(map(len, keys), default=0)
