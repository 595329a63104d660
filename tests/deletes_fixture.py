"""Loader of tests/golden/deletes.npz for the delete tests (not a test module):
the op streams, the files the reference wrote for them and the codes its own
Database::Get returned (tests/golden/make_golden_deletes.py).
"""
from __future__ import annotations

import os
import sys

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_golden_deletes import decode_ops  # noqa: E402

import index_model as M  # noqa: E402

REF_OK, REF_NOTFOUND, REF_DELETE_ORDER = 0, 1, 2         # util/status.h's codes
STATUS_OF_CODE = {REF_NOTFOUND: M.NOTFOUND, REF_DELETE_ORDER: M.DELETED}


def _keys(z, name):
    blob, out, o = z[f"{name}__keys"].tobytes(), [], 0
    for n in z[f"{name}__key_len"]:
        out.append(blob[o:o + int(n)])
        o += int(n)
    return out


def load():
    """{stream name: dict(ops, items, files, hash_type, hstable_size, keys, code, len, crc)} and the torn cases.
    ops are (key, value | None, chunks); items are the same for kingdb_amd.put."""
    from kingdb_amd import put
    z = load_golden("deletes.npz")
    sets = {}
    for name in (str(n) for n in z["names"]):
        ops = decode_ops(z[f"{name}__stream"].tobytes())
        sets[name] = dict(
            ops=ops, items=[(k, put.DELETE) if v is None else (k, v, ch) for k, v, ch in ops],
            files={str(f): z[f"{name}__file_{f}"].tobytes() for f in z[f"{name}__files"]},
            hstable_size=int(z[f"{name}__opts"][0]), hash_type=int(z[f"{name}__opts"][1]), keys=_keys(z, name),
            code=[int(c) for c in z[f"{name}__code"]], len=[int(c) for c in z[f"{name}__len"]],
            crc=[int(c) for c in z[f"{name}__crc"]])
    base = str(z["torn__base"][0])
    torn = [dict(base=base, cut=int(c), recovered=z[f"torn__file_{i}"].tobytes(),
                 code=[int(x) for x in z[f"torn__code_{i}"]], len=[int(x) for x in z[f"torn__len_{i}"]],
                 crc=[int(x) for x in z[f"torn__crc_{i}"]]) for i, c in enumerate(z["torn__cut"])]
    return sets, torn


def assert_codes(got, keys, code, length, crc, orc, what=""):
    """got = [(status, value)] per key against the reference's Get codes:
    DeleteOrder <-> DELETED, NotFound <-> NOTFOUND, OK <-> length and CRC32C."""
    assert len(got) == len(keys)
    for k, (st, val), c, n, w in zip(keys, got, code, length, crc):
        if c == REF_OK:
            assert st == 0 and len(val) == n and orc.crc32c(val) == w, (what, k, st, len(val), n)
        else:
            assert st == STATUS_OF_CODE[c] and val == b"", (what, k, st, c)


def last_ops(ops):
    """{key: value | None}: the last op of every key."""
    last = {}
    for k, v, _ in ops:
        last[k] = v
    return last


def delete_entries(f: bytes):
    """[(row hash, get.Entry)] of the delete entries a file's offset array lists."""
    from kingdb_amd import get as G
    return [(h, e) for (h, _), e in zip(M.parse_rows(f), G.read_hstable(f)) if e.is_delete]
