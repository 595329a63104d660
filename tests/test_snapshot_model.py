"""CPU: snapshots of a loaded index (include/kdb_snapshot.h), without a GPU.

  * the header declares exactly the kdb_snapshot_* functions, the library
    exports them, _lib.SIGNATURES has them with their twins' argument lists,
    kdb_put.h includes the header;
  * the argument checks made before any device work: a null snapshot, the scan
    calls before a prepare, and the lifetime rule (load and destroy of the
    handle refused while a snapshot is open, accepted after its release), on a
    handle created without a GPU.  The two checks that need a prepared list --
    a window past `live`, keys_cap one byte short -- are made in
    tests/test_gpu_snapshot.py::test_independence;
  * the expectation the GPU tests of tests/test_gpu_snapshot.py rest on: the
    scan model of tests/scan_model.py over a PREFIX of a database's files, in
    (timestamp, fileid) order, lists exactly the keys whose last entry among
    those files is a put, each once with that entry's value.  This passes
    without the feature and is here so that the GPU tests compare against a
    checked model.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import deletes_fixture as D
import index_model as M
import scan_model as S
from conftest import ROOT
from kingdb_amd import get as G
from test_index_add_model import file_order, fixture_streams

FUNCTIONS = ["kdb_snapshot_create", "kdb_snapshot_entry_count", "kdb_snapshot_file_count", "kdb_snapshot_get_batch",
             "kdb_snapshot_release", "kdb_snapshot_scan_batch", "kdb_snapshot_scan_prepare",
             "kdb_snapshot_scan_sort_steps"]
STREAMS = ["get_keys_xx", "get_keys_murmur", "key_lengths_xx", "key_lengths_murmur"]


def all_streams() -> dict:
    """{stream: dict(files, hash_type, keys, order)}: the fixture streams of the
    add tests and the multi-file streams of tests/golden/deletes.npz."""
    out = {}
    for name, (files, ht, keys) in fixture_streams().items():
        out[name] = {"files": files, "hash_type": ht, "keys": keys, "order": file_order(files)}
    for name, s in D.load()[0].items():
        if len(s["files"]) > 1:
            out["deletes_" + name] = {"files": s["files"], "hash_type": s["hash_type"], "keys": s["keys"],
                                      "order": file_order(s["files"])}
    return out


def last_entries(files: dict, names) -> dict:
    """{key: (file name, get.Entry)}: every key's last entry among the files `names`, read in that order."""
    last = {}
    for name in names:
        for e in G.read_hstable(files[name]):
            last[e.key] = (name, e)
    return last


def value_of(files: dict, name: str, e, orc) -> bytes:
    f = files[name]
    st, val = orc.get_value(f[e.value_at:e.value_at + e.stored_len], e.size_value_compressed, e.size_value,
                            e.checksum, orc.crc32c(e.key), 0)
    assert st == 0
    return val


def test_header_symbols_and_signatures():
    from kingdb_amd import _lib, index
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "kdb_snapshot.h")).read()
    assert "database.cc:301-327" in text and "snapshot.h" in text       # the reference rows it stands for
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(kdb_\w+)\s*\(", code))) == FUNCTIONS
    for s in FUNCTIONS:
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    assert '#include "kdb_snapshot.h"' in open(os.path.join(ROOT, "include", "kdb_put.h")).read()
    for twin in ("get_batch", "scan_prepare", "scan_sort_steps", "scan_batch"):
        assert _lib.SIGNATURES["kdb_snapshot_" + twin] == _lib.SIGNATURES["kdb_index_" + twin], twin
    assert callable(index.HSTableIndex.snapshot)
    for method in ("locate", "get", "scan_prepare", "scan_sort_steps", "scan", "items", "compacted",
                   "compacted_device", "close", "__enter__", "__exit__"):
        assert callable(getattr(index.HSTableSnapshot, method)), method
        if not method.startswith("__") and method != "close":                # shared with the index, not copied
            assert getattr(index.HSTableSnapshot, method) is getattr(index.HSTableIndex, method), method


def _get_args(summary=None):
    one64, one32 = np.zeros(8, np.uint64), np.zeros(8, np.uint32)
    p64, p32 = one64.ctypes.data, one32.ctypes.data
    keep = (one64, one32)
    # stream, keys, key_off, key_len, n, verify, multipart, scratch, scratch_bytes, 9 outputs, summary
    return keep, [None, p64, p64, p32, 0, 0, 0, p64, 256, p64, p64, p64, p64, p32, p32, p64, p64, p32,
                  p64 if summary is None else summary]


def _scan_args(first=0, n=0):
    one64, one32 = np.zeros(8, np.uint64), np.zeros(8, np.uint32)
    p64, p32 = one64.ctypes.data, one32.ctypes.data
    keep = (one64, one32)
    # stream, first, n, multipart, scratch, scratch_bytes, keys_out, keys_cap, key_off, key_len, 9 outputs, summary
    return keep, [None, first, n, 0, p64, 512, p64, 64, p64, p32, p64, p64, p64, p64, p32, p32, p64, p64, p32, p64]


def test_null_snapshot_and_scan_before_prepare():
    """KDB_PUT_EINVAL before any device work."""
    from kingdb_amd import _lib
    lib = _lib.load()
    n64, n32 = ctypes.c_uint64(7), ctypes.c_uint32(7)
    snap = ctypes.c_void_p()
    assert lib.kdb_snapshot_create(None, ctypes.byref(snap)) == _lib.EINVAL
    assert lib.kdb_snapshot_release(None) == _lib.EINVAL
    assert lib.kdb_snapshot_entry_count(None, ctypes.byref(n64)) == _lib.EINVAL
    assert lib.kdb_snapshot_file_count(None, ctypes.byref(n32)) == _lib.EINVAL
    keep, a = _get_args()
    assert lib.kdb_snapshot_get_batch(None, *a) == _lib.EINVAL
    assert lib.kdb_snapshot_scan_prepare(None, None, 0, None, None, None) == _lib.EINVAL
    assert lib.kdb_snapshot_scan_sort_steps(None, ctypes.byref(n32)) == _lib.EINVAL
    keep2, b = _scan_args()
    assert lib.kdb_snapshot_scan_batch(None, *b) == _lib.EINVAL
    h = ctypes.c_void_p()
    assert lib.kdb_index_create(1, ctypes.byref(h)) == 0
    try:
        assert lib.kdb_snapshot_create(h, None) == _lib.EINVAL
        assert lib.kdb_snapshot_create(h, ctypes.byref(snap)) == 0 and snap.value
        try:
            # an empty handle gives a valid empty snapshot
            assert lib.kdb_snapshot_entry_count(snap, ctypes.byref(n64)) == 0 and n64.value == 0
            assert lib.kdb_snapshot_file_count(snap, ctypes.byref(n32)) == 0 and n32.value == 0
            assert lib.kdb_snapshot_entry_count(snap, None) == _lib.EINVAL
            assert lib.kdb_snapshot_file_count(snap, None) == _lib.EINVAL
            # the scan calls before a prepare
            assert lib.kdb_snapshot_scan_sort_steps(snap, ctypes.byref(n32)) == _lib.EINVAL
            assert lib.kdb_snapshot_scan_batch(snap, *b) == _lib.EINVAL
            assert lib.kdb_snapshot_scan_prepare(snap, None, 2, None, None, None) == _lib.EINVAL    # verify_header
            # the lookup's own checks: no summary, a verify_header that does not exist, scratch one byte short
            keep3, c = _get_args()
            c[-1] = None
            assert lib.kdb_snapshot_get_batch(snap, *c) == _lib.EINVAL
            keep4, c = _get_args()
            c[5] = 2
            assert lib.kdb_snapshot_get_batch(snap, *c) == _lib.EINVAL
            keep5, c = _get_args()
            c[8] = int(lib.kdb_index_get_scratch_bytes(0)) - 1
            assert lib.kdb_snapshot_get_batch(snap, *c) == _lib.EINVAL
        finally:
            assert lib.kdb_snapshot_release(snap) == 0
    finally:
        assert lib.kdb_index_destroy(h) == 0
    del keep, keep2


def test_load_and_destroy_refused_while_a_snapshot_is_open():
    from kingdb_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.kdb_index_create(1, ctypes.byref(h)) == 0
    s1, s2 = ctypes.c_void_p(), ctypes.c_void_p()
    entries = ctypes.c_uint64(9)
    load = (None, None, None, None, None, 0, None, ctypes.byref(entries))     # no files: nothing for the device to do
    assert lib.kdb_snapshot_create(h, ctypes.byref(s1)) == 0
    assert lib.kdb_snapshot_create(h, ctypes.byref(s2)) == 0                  # several may be open at once
    assert s1.value != s2.value
    for left in (s1, s2):
        assert lib.kdb_index_load_files(h, *load) == _lib.EINVAL and entries.value == 9
        assert lib.kdb_index_destroy(h) == _lib.EINVAL
        n = ctypes.c_uint64(5)
        assert lib.kdb_index_entry_count(h, ctypes.byref(n)) == 0 and n.value == 0        # the handle is still there
        assert lib.kdb_snapshot_release(left) == 0
    # both released: the load passes the argument checks again (0 with a device;
    # without one it gets as far as the device and reports that, never EINVAL)
    assert lib.kdb_index_load_files(h, *load) in (0, _lib.EHIP, _lib.ENODEV)
    assert lib.kdb_index_destroy(h) == 0


@pytest.mark.parametrize("stream", STREAMS + ["deletes"])
def test_scan_model_over_a_prefix(orc, stream):
    """S.scan over the first k files = the keys whose last entry among them is a put, each with that value."""
    streams = all_streams()
    names = [n for n in streams if n.startswith("deletes_")] if stream == "deletes" else [stream]
    assert names
    deletes_seen = 0
    for name in names:
        s = streams[name]
        files, order = s["files"], s["order"]
        assert order == sorted(files)
        for k in range(len(order) + 1):
            prefix = {f: files[f] for f in order[:k]}
            m = M.Model(prefix, orc, s["hash_type"])
            last = last_entries(files, order[:k])
            want = {key: value_of(files, f, e, orc) for key, (f, e) in last.items() if not e.is_delete}
            deletes_seen += sum(1 for _, e in last.values() if e.is_delete)
            got = S.scan(m)
            assert all(st == 0 for _, st, _ in got)
            assert len(got) == len(want) and {key: v for key, _, v in got} == want, (name, k)
            assert S.prepare(m) == (len(want), sum(map(len, want)), max(map(len, want), default=0))
            # iterator order: files in order, offsets ascending
            where = [(order.index(last[key][0]), last[key][1].offset) for key, _, _ in got]
            assert where == sorted(where)
    if stream == "deletes":
        assert deletes_seen > 0
