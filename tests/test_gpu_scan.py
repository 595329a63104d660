"""GPU: the scan (csrc/index.hip, include/kdb_scan.h, HSTableIndex.scan) --
every live entry of a database in iterator order, then decoded by
kdb_get_values_batch.

Expectations come from the Python model in tests/scan_model.py, which
tests/test_scan_model.py pins to what the reference's own Database::Get and
iterator returned, and from the put streams themselves (the last value put
per key).
"""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

import index_model as M
import scan_model as S
from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_golden_put import decode_stream  # noqa: E402

pytestmark = pytest.mark.gpu


def _sets(npz, with_keys):
    z = load_golden(npz)
    out = {}
    for name in (str(n) for n in z["names"]):
        files = {str(f): z[f"{name}__file_{f}"].tobytes() for f in z[f"{name}__files"]}
        d = {"files": files, "hash_type": int(z[f"{name}__opts"][1]), "hstable_size": int(z[f"{name}__opts"][0]),
             "puts": decode_stream(z[f"{name}__stream"].tobytes())}
        if with_keys:
            d["keys"] = [k.tobytes() for k in z[f"{name}__keys"]]
        d["last"] = {k: v for k, v, _ in d["puts"]}
        out[name] = d
    return out


@pytest.fixture(scope="module")
def getkeys():
    return _sets("get_keys.npz", True)


@pytest.fixture(scope="module")
def streams():
    return _sets("hstable_streams.npz", False)


@pytest.fixture(scope="module")
def xx_scan(getkeys, orc):
    """The model's scan of `xx` at verify 0, computed once and left unchanged."""
    s = getkeys["xx"]
    return tuple(S.scan(M.Model(s["files"], orc, s["hash_type"])))


def open_index(gpu, files, hash_type=1):
    from kingdb_amd.index import HSTableIndex
    return HSTableIndex(files, hash_type)


def prepare_raw(ix, verify=0):
    from kingdb_amd import _lib
    live, kbytes, kmax = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
    rc = _lib.load().kdb_index_scan_prepare(ix.h, None, verify, ctypes.byref(live), ctypes.byref(kbytes),
                                            ctypes.byref(kmax))
    return rc, (live.value, kbytes.value, kmax.value)


def batch_raw(ix, first, n, keys_cap):
    """kdb_index_scan_batch on fresh buffers: its return code."""
    from kingdb_amd import _lib
    from kingdb_amd.index import _Lookup
    L = _Lookup(max(n, 1), keys_cap)
    try:
        return _lib.load().kdb_index_scan_batch(
            ix.h, None, first, n, 0, L.scratch.ptr, L.scratch_bytes, L.keys.ptr, keys_cap, L.p("key_off"),
            L.p("key_len"), L.p("stored_off"), L.p("avail"), L.p("svc"), L.p("size"), L.p("checksum"),
            L.p("checksum_initial"), L.p("out_off"), L.p("location"), L.p("status"), L.p("summary"))
    finally:
        L.free()


@pytest.mark.parametrize("verify", [0, 1, 2])
@pytest.mark.parametrize("name,rows,live", [("xx", 400, 150), ("murmur", 60, 40)])
def test_fixture_scan(gpu, getkeys, orc, name, rows, live, verify):
    """verify 0 and 1 as kdb_index_scan_prepare takes them (1: every header's
    CRC-8).  The Python `verify` also goes to the value decoder, where 1 is the
    reference's own value check with its double-streamed CRC (get.py): on these
    files it reports -2 for some values, in the model (the oracle's
    restatement) as here, so at 1 the value set is asserted for the entries of
    status 0 and the rest must be the model's -2; 2 (headers verified as at 1,
    the corrected value check) is run as well and returns every value."""
    s = getkeys[name]
    m = M.Model(s["files"], orc, s["hash_type"])
    want = S.scan(m, verify)
    ix = open_index(gpu, s["files"], s["hash_type"])
    try:
        assert ix.entries == rows
        rc, got_prep = prepare_raw(ix, 1 if verify else 0)
        assert rc == 0 and got_prep == S.prepare(m, verify) and got_prep[0] == live
        assert ix.scan_prepare(verify) == live and ix.scan_sort_steps() == 0
        got = ix.scan(verify=verify)
        assert got == want                                        # order included
        assert {k for k, _, _ in got} == set(s["last"]) and len(got) == len(s["last"])
        if verify != 1:
            assert {(k, v) for k, _, v in got} == set(s["last"].items())
        else:
            assert {st for _, st, _ in got} <= {0, -2}
            assert all(v == s["last"][k] for k, st, v in got if st == 0)
    finally:
        ix.close()


def test_windows(gpu, getkeys, xx_scan):
    from kingdb_amd import _lib
    s = getkeys["xx"]
    want = list(xx_scan)
    ix = open_index(gpu, s["files"], s["hash_type"])
    try:
        assert batch_raw(ix, 0, 1, 64) == _lib.EINVAL             # before prepare
        live = ix.scan_prepare()
        assert live == len(want)
        for w in (1, 7, 64, 65, live):
            got = []
            for first in range(0, live, w):
                got += ix.scan(first, min(w, live - first))
            assert got == want, w
        assert list(ix.items(batch=64)) == want
        assert ix.scan(live, 0) == []
        assert batch_raw(ix, live, 0, 0) == 0
        assert batch_raw(ix, live, 1, 64) == _lib.EINVAL          # first + n > live
        assert batch_raw(ix, live - 3, 4, 256) == _lib.EINVAL
        with pytest.raises(_lib.HipError):
            ix.scan(live - 3, 4)
        need = sum(len(k) for k, _, _ in want[10:75])
        assert batch_raw(ix, 10, 65, need) == 0
        assert batch_raw(ix, 10, 65, need - 1) == _lib.EINVAL     # keys_cap one byte short
    finally:
        ix.close()


def test_deletes(gpu, getkeys, orc):
    """test_gpu_index.py::test_delete_entry's files.  The delete row newest:
    the key is absent and so is the delete entry; every other key is there.
    The delete row oldest: the key's put is live."""
    from kingdb_amd import get as G
    s = getkeys["xx"]
    last = s["last"]
    name = sorted(s["files"])[-1]
    f = s["files"][name]
    key = G.read_hstable(f)[-1].key
    oi = M.footer(f)[2]
    entry = orc.entry_header(0, 0x1 | 0x8, len(key), 0, 0, 0, orc.xxh64(key)) + key
    rows = M.parse_rows(f)
    files = dict(s["files"])
    for newest in (True, False):
        r = rows + [(orc.xxh64(key), oi)] if newest else [(orc.xxh64(key), oi)] + rows
        files[name] = M.with_rows(f, r, orc, f[:oi] + entry)
        m = M.Model(files, orc, 1)
        ix = open_index(gpu, files, 1)
        try:
            assert set(ix.file_status.values()) == {0}
            got = ix.scan()
            assert got == S.scan(m)
            want = dict(last)
            if newest:
                del want[key]
            assert {k: v for k, _, v in got} == want and len(got) == len(want)
            assert all(st == 0 for _, st, _ in got)
            # the delete row sits below / above the others: the sort ran only where offsets do not ascend
            assert (ix.scan_sort_steps() > 0) == (not newest)
        finally:
            ix.close()


@pytest.mark.parametrize("how", ["reversed", "shuffled"])
def test_non_ascending_rows(gpu, getkeys, orc, how):
    """One file's offset array reversed, or shuffled: the output is still by
    offset, liveness follows the new sequence order, and the sort ran."""
    s = getkeys["xx"]
    name = sorted(s["files"])[1]
    rows = M.parse_rows(s["files"][name])
    if how == "reversed":
        rows = rows[::-1]
    else:
        random.Random(20).shuffle(rows)
    files = dict(s["files"])
    files[name] = M.with_rows(s["files"][name], rows, orc)
    m = M.Model(files, orc, 1)
    want = S.scan(m)
    order = [(rank, off) for rank, off, _, _ in S.live_rows(m)]
    assert order == sorted(order)
    ix = open_index(gpu, files, 1)
    try:
        live = ix.scan_prepare()
        assert ix.scan_sort_steps() > 0
        assert live == len(want) == S.prepare(m)[0]
        assert ix.scan() == want
        assert ix.scan(3, 70) == want[3:73]
    finally:
        ix.close()


def test_forged_hash(gpu, getkeys, orc):
    """test_gpu_index.py::test_candidate_walk's files: B's row carries A's
    hash.  Get cannot reach B, so B is not in the scan; A is."""
    from kingdb_amd import get as G
    s = getkeys["xx"]
    count = {}
    for k, _, _ in s["puts"]:
        count[k] = count.get(k, 0) + 1
    once = {k for k, c in count.items() if c == 1}
    for name, f in sorted(s["files"].items()):
        ents = G.read_hstable(f)
        idx = [i for i, e in enumerate(ents) if e.key in once]
        if len(idx) >= 2:
            break
    ia, ib = idx[0], idx[1]
    a, b = ents[ia].key, ents[ib].key
    rows = M.parse_rows(f)
    rows[ib] = (rows[ia][0], rows[ib][1])
    files = dict(s["files"])
    files[name] = M.with_rows(f, rows, orc)
    m = M.Model(files, orc, 1)
    ix = open_index(gpu, files, 1)
    try:
        got = ix.scan()
        assert got == S.scan(m)
        keys = [k for k, _, _ in got]
        assert a in keys and b not in keys and len(keys) == len(s["last"]) - 1
    finally:
        ix.close()


@pytest.mark.parametrize("verify", [0, 1])
def test_hostile_rows(gpu, getkeys, orc, verify):
    """index_model.hardened_set: the five hostile rows are skipped, every
    other live entry is returned."""
    s = getkeys["xx"]
    files, hostile = M.hardened_set(s["files"], orc)
    m = M.Model(files, orc, 1)
    want = S.scan(m, verify)
    ix = open_index(gpu, files, 1)
    try:
        assert set(ix.file_status.values()) == {0}
        got = ix.scan(verify=verify)
        assert got == want
        rc, prep = prepare_raw(ix, verify)
        assert rc == 0 and prep == S.prepare(m, verify)
        # a hostile row's key is in the scan only through an older, intact entry of that key
        base = {k for k, _, _ in S.scan(M.Model(s["files"], orc, 1), verify)}
        keys = {k for k, _, _ in got}
        assert base - keys <= set(hostile) and keys <= base
        assert len(keys) >= len(base) - 5
    finally:
        ix.close()


def test_multipart_required_1000(gpu, getkeys, orc):
    from kingdb_amd.index import MULTIPART
    s = getkeys["xx"]
    ix = open_index(gpu, s["files"], 1)
    try:
        got = ix.scan(multipart_required=1000)
        assert got == S.scan(M.Model(s["files"], orc, 1), 0, 1000)
        assert len(got) == len(s["last"])
        big = 0
        for k, st, v in got:
            if len(s["last"][k]) > 1000:
                assert (st, v) == (MULTIPART, b"")
                big += 1
            else:
                assert (st, v) == (0, s["last"][k])
        assert 0 < big < len(got)
    finally:
        ix.close()


def test_multipart_stream(gpu, streams, orc):
    """The `multipart` stream with the footer recovery would append: values
    of several frames, up to 115 536 bytes."""
    s = streams["multipart"]
    name, f = next(iter(s["files"].items()))
    files = {name: M.with_recovered_footer(f, orc)}
    m = M.Model(files, orc, s["hash_type"])
    want = S.scan(m)
    assert max(len(v) for _, _, v in want) == 115536
    ix = open_index(gpu, files, s["hash_type"])
    try:
        assert ix.file_status == {name: 0}
        assert ix.scan() == want
        assert list(ix.items(batch=5)) == want
    finally:
        ix.close()


def test_empty(gpu, getkeys, orc):
    s = getkeys["xx"]
    name = sorted(s["files"])[0]
    f = bytearray(s["files"][name])
    f[len(f) - 12:len(f) - 4] = bytes(8)                          # no magic: status -1, no rows
    for files in ({}, {name: bytes(f)}):
        ix = open_index(gpu, files, 1)
        try:
            assert ix.entries == 0 and set(ix.file_status.values()) <= {-1}
            assert prepare_raw(ix) == (0, (0, 0, 0))
            assert ix.scan_prepare() == 0 and ix.scan() == [] and list(ix.items()) == []
        finally:
            ix.close()


def test_compacted(gpu, getkeys, orc, xx_scan):
    s = getkeys["xx"]
    ix = open_index(gpu, s["files"], 1)
    try:
        before = ix.get(s["keys"])
        new_files = ix.compacted(s["hstable_size"], batch=64)
    finally:
        ix.close()
    assert len(new_files) >= 1
    ix = open_index(gpu, new_files, 1)
    try:
        assert set(ix.file_status.values()) == {0}
        assert ix.entries == len(xx_scan) == ix.scan_prepare()
        assert ix.get(s["keys"]) == before
        assert {(k, v) for k, _, v in ix.scan()} == {(k, v) for k, _, v in xx_scan}
    finally:
        ix.close()


def test_project_written_files(gpu, getkeys, orc):
    from kingdb_amd import put
    s = getkeys["xx"]
    files = put.write_hstables(s["puts"], s["hstable_size"], s["hash_type"], batch=50)
    assert len(files) > 1
    ix = open_index(gpu, files, s["hash_type"])
    try:
        for verify in (0, 2):
            got = ix.scan(verify=verify)
            assert all(st == 0 for _, st, _ in got)
            assert {k: v for k, _, v in got} == s["last"] and len(got) == len(s["last"])
        assert ix.scan_sort_steps() == 0
        assert got == S.scan(M.Model(files, orc, s["hash_type"]), 2)
    finally:
        ix.close()
