"""GPU: newly closed files added to a loaded index (include/kdb_index_add.h,
csrc/index.hip, HSTableIndex.refresh / .add_files).

The contract under test: after an add the handle is indistinguishable, through
entries, file_status, pairs(), Get and the scan, from an HSTableIndex made
fresh over the same files.  Expectations are that fresh index and the Python
model of tests/index_model.py (pinned to the reference's own Database::Get by
tests/test_index_model.py, and over prefixes of a database's files by
tests/test_index_add_model.py); every comparison is exact.

Rows per file of the fixture streams (their footers): get_keys xx
131 / 104 / 127 / 38, get_keys murmur 60, key_lengths xx 111 / 123 / 114,
key_lengths murmur 130 / 88.  B, the bucket count, is the smallest power of
two >= 2 x rows: the adds below cross 256 -> 512 -> 1024 and stay inside
512 and 1024.
"""
import ctypes
import struct

import numpy as np
import pytest

import index_model as M
import scan_model as S
from test_index_add_model import file_order, fixture_streams

pytestmark = pytest.mark.gpu

STREAMS = ["get_keys_xx", "get_keys_murmur", "key_lengths_xx", "key_lengths_murmur"]
REBUILD = 1                                              # KDB_INDEX_ADD_REBUILD


@pytest.fixture(scope="module")
def streams():
    out = {}
    for name, (files, ht, keys) in fixture_streams().items():
        out[name] = {"files": files, "hash_type": ht, "keys": keys, "order": file_order(files)}
    return out


def flipped(k, at, x=0x40):
    b = bytearray(k)
    b[at] ^= x
    return bytes(b)


def queries(keys):
    """Every key and its near-misses: a byte flipped, one byte shorter, one longer, the empty key."""
    q = list(keys)
    q += [flipped(k, len(k) // 2) for k in keys] + [k[:-1] for k in keys] + [k + b"\0" for k in keys] + [b""]
    return q


def buckets(rows: int) -> int:
    b = 2
    while b < 2 * rows:
        b <<= 1
    return b


def rows_of(f: bytes) -> int:
    return M.footer(f)[3]


def snapshot(ix, q):
    """What the public interface shows of an index: entries, file_status, pairs, Get and locate of `q`."""
    h, loc = ix.pairs()
    where, st = ix.locate(q)
    return {"entries": ix.entries, "file_status": dict(ix.file_status), "hash": [int(x) for x in h],
            "loc": [int(x) for x in loc], "get": ix.get(q), "where": [int(x) for x in where],
            "status": [int(x) for x in st]}


def assert_model(snap, m, q):
    assert snap["file_status"] == m.file_status
    want = m.pairs()
    assert snap["entries"] == len(want)
    assert snap["hash"] == [w[0] for w in want] and snap["loc"] == [w[1] for w in want]
    for k, (st, val), where in zip(q, snap["get"], snap["where"]):
        wst, wval, wloc = m.get(k)
        assert (st, val, where) == (wst, wval, wloc), (k, st, wst)


@pytest.fixture(scope="module")
def fresh(gpu, streams, orc):
    """The snapshot of an HSTableIndex made fresh over the first n files of a
    stream, checked against the model once and then shared."""
    from kingdb_amd.index import HSTableIndex
    cache = {}

    def get(stream, n):
        if (stream, n) not in cache:
            s = streams[stream]
            files = {f: s["files"][f] for f in s["order"][:n]}
            q = queries(s["keys"])
            ix = HSTableIndex(files, s["hash_type"])
            try:
                snap = snapshot(ix, q)
            finally:
                ix.close()
            assert_model(snap, M.Model(files, orc, s["hash_type"]), q)
            cache[stream, n] = snap
        return cache[stream, n]
    return get


def room(files, names) -> int:
    return sum((len(files[f]) + 63) & ~63 for f in names) + 64


def place(ix, files, names):
    """Uploads files[names] behind what the index holds, in the order given:
    (file_off, file_size, fileid) for kdb_index_add_files, and the end."""
    at = (ix._used + 63) & ~63
    off = []
    for f in names:
        off.append(at)
        ix.files.upload(np.frombuffer(files[f], np.uint8), at)
        at = (at + len(files[f]) + 63) & ~63
    end = off[-1] + len(files[names[-1]])
    assert end + 64 <= ix.files.nbytes
    return (np.array(off, np.uint64), np.array([len(files[f]) for f in names], np.uint64),
            np.array([int(f[:8], 16) for f in names], np.uint32), end)


def add_in_order(ix, files, names, flags=0):
    """One kdb_index_add_files call with the files in exactly this argument order."""
    off, size, fid, end = place(ix, files, names)
    res = ix._add(None, off, size, fid, flags)
    ix._used = end
    return res


def add_rc(ix, off, size, fid, flags=0, d_files=None):
    """The raw call: (rc, statuses, entries added); the Python object is not updated."""
    from kingdb_amd import _lib
    n = len(fid)
    status = np.full(max(n, 1), 99, np.int32)
    added = ctypes.c_uint64(0)
    rc = _lib.load().kdb_index_add_files(ix.h, None, ix.files.ptr if d_files is None else d_files, off.ctypes.data,
                                         size.ctypes.data, fid.ctypes.data, n, flags, status.ctypes.data,
                                         ctypes.byref(added))
    return rc, [int(x) for x in status[:n]], added.value


# ------------------------------------------------------------- 1. add equals load
@pytest.mark.parametrize("stream", STREAMS)
def test_add_equals_load(gpu, streams, fresh, stream):
    from kingdb_amd.index import HSTableIndex
    s = streams[stream]
    files, order, q = s["files"], s["order"], queries(s["keys"])
    for k in range(len(order)):
        rest = order[k:]
        # one call per file
        ix = HSTableIndex({f: files[f] for f in order[:k]}, s["hash_type"], reserve=room(files, rest))
        try:
            assert snapshot(ix, q) == fresh(stream, k)
            for n, f in enumerate(rest, k + 1):
                assert ix.add_files({f: files[f]}) == {f: 0}
                assert ix.names == order[:n]
                assert snapshot(ix, q) == fresh(stream, n), (k, n)
        finally:
            ix.close()
        # the rest in one call, newest first in the arguments
        ix = HSTableIndex({f: files[f] for f in order[:k]}, s["hash_type"], reserve=room(files, rest))
        try:
            assert add_in_order(ix, files, rest[::-1]) == {f: 0 for f in rest}
            snap = snapshot(ix, q)
            want = fresh(stream, len(order))
            assert snap == want, k
        finally:
            ix.close()


# ------------------------------------------------------------- 2. the bucket count, and the hot key on both sides
def test_bucket_count_and_hot_key_across_the_boundary(gpu, streams, fresh, orc):
    """Files 1..k loaded, file k + 1 added, where B stays (235 and 400 rows of
    get_keys xx, 218 of key_lengths murmur) and where it doubles: the add
    reports the B a load picks and the rows it parsed.  In key_lengths murmur
    the 70-fold hot key has rows on both sides of the boundary.  (A second
    bucket path for the adds where B stays was measured and not kept, DESIGN.md
    section 4.8; KDB_INDEX_ADD_REBUILD is accepted and changes nothing.)"""
    from kingdb_amd.index import HSTableIndex
    stays = {}
    for stream, k in (("get_keys_xx", 1), ("get_keys_xx", 2), ("get_keys_xx", 3), ("key_lengths_murmur", 1),
                      ("key_lengths_xx", 1), ("key_lengths_xx", 2)):
        s = streams[stream]
        files, order, q = s["files"], s["order"], queries(s["keys"])
        old = sum(rows_of(files[f]) for f in order[:k])
        new = rows_of(files[order[k]])
        stays[stream, k] = buckets(old) == buckets(old + new)
        for flags in (0, REBUILD):
            ix = HSTableIndex({f: files[f] for f in order[:k]}, s["hash_type"], reserve=room(files, order[k:k + 1]))
            try:
                add_in_order(ix, files, order[k:k + 1], flags)
                assert ix.add_stats() == (0, buckets(old + new), new), (stream, k)
                assert snapshot(ix, q) == fresh(stream, k + 1), (stream, k, flags)
            finally:
                ix.close()
    # what the row counts in the module docstring say
    assert stays == {("get_keys_xx", 1): True, ("get_keys_xx", 2): False, ("get_keys_xx", 3): True,
                     ("key_lengths_murmur", 1): True, ("key_lengths_xx", 1): False, ("key_lengths_xx", 2): False}
    s = streams["key_lengths_murmur"]
    h = orc.murmur3_64
    per_file = [[hh for hh, _ in M.parse_rows(s["files"][f])] for f in s["order"]]
    hot = [k for k in s["keys"] if sum(rows.count(h(k)) for rows in per_file) == 70]
    assert len(hot) == 1 and all(rows.count(h(hot[0])) > 0 for rows in per_file)


# ------------------------------------------------------------- 3. a crowded bucket across the boundary
def crowded_pair(s, orc):
    """Files 1 and 2 of get_keys xx with 70 rows each re-pointed at the hash of
    K, a key with an entry in both: (file 1', file 2', K, the keys whose rows
    were taken).  The row counts stay 131 + 104, so B stays 512."""
    from kingdb_amd import get as G
    a, b = s["order"][:2]
    ents = {f: G.read_hstable(s["files"][f]) for f in (a, b)}
    both = [e.key for e in ents[a] if any(x.key == e.key for x in ents[b])]
    assert both
    key = both[0]
    hk = orc.xxh64(key)
    out, taken = {}, []
    for f in (a, b):
        rows = M.parse_rows(s["files"][f])
        idx = [i for i, e in enumerate(ents[f]) if e.key != key][:70]
        assert len(idx) == 70
        for i in idx:
            rows[i] = (hk, rows[i][1])
            taken.append(ents[f][i].key)
        out[f] = M.with_rows(s["files"][f], rows, orc)
        assert sum(1 for h, _ in rows if h == hk) >= 65 + 1
    return out, key, taken


def test_crowded_bucket_across_the_boundary(gpu, streams, orc):
    from kingdb_amd import get as G
    from kingdb_amd.index import HSTableIndex, NOTFOUND
    s = streams["get_keys_xx"]
    files, key, taken = crowded_pair(s, orc)
    a, b = s["order"][:2]
    m = M.Model(files, orc, 1)
    q = queries([key] + taken)
    newest = [e for e in G.read_hstable(files[b]) if e.key == key][-1]
    assert m.get(key)[2] == (int(b, 16) << 32 | newest.offset)          # the newest same-key row, in the added file
    assert [m.get(k)[0] for k in taken].count(NOTFOUND) >= 65            # a differing key of that hash is not found
    want = None
    for flags in (0, REBUILD):
        ix = HSTableIndex({a: files[a]}, 1, reserve=room(files, [b]))
        try:
            add_in_order(ix, files, [b], flags)
            assert ix.add_stats() == (0, 512, 104)
            snap = snapshot(ix, q)
            assert_model(snap, m, q)
            assert snap["get"][0][0] == 0 and snap["where"][0] == m.get(key)[2]
            if want is None:
                fr = HSTableIndex(files, 1)
                try:
                    want = snapshot(fr, q)
                finally:
                    fr.close()
            assert snap == want
        finally:
            ix.close()


# ------------------------------------------------------------- 4. overwrite and delete in the added file
def test_overwrite_and_delete_in_the_added_file(gpu, streams, orc):
    from kingdb_amd import get as G
    from kingdb_amd.index import DELETED, HSTableIndex
    s = streams["get_keys_xx"]
    order = s["order"]
    name = order[-1]
    f = s["files"][name]
    older = {e.key for g in order[:-1] for e in G.read_hstable(s["files"][g])}
    key = [e.key for e in G.read_hstable(f) if e.key in older][-1]
    oi = M.footer(f)[2]
    entry = orc.entry_header(0, 0x1 | 0x8, len(key), 0, 0, 0, orc.xxh64(key)) + key
    files = dict(s["files"])
    files[name] = M.with_rows(f, M.parse_rows(f) + [(orc.xxh64(key), oi)], orc, f[:oi] + entry)
    before = M.Model({g: files[g] for g in order[:-1]}, orc, 1)
    after = M.Model(files, orc, 1)
    assert before.get(key)[0] == 0 and after.get(key)[0] == DELETED
    q = queries([key] + s["keys"][:20])
    ix = HSTableIndex({g: files[g] for g in order[:-1]}, 1, reserve=room(files, [name]))
    try:
        assert_model(snapshot(ix, q), before, q)
        assert ix.add_files({name: files[name]}) == {name: 0}
        snap = snapshot(ix, q)
        assert_model(snap, after, q)
        assert snap["get"][0] == (DELETED, b"")
    finally:
        ix.close()
    # a put that overwrites, added after the file holding the old value
    a, b = order[:2]
    ents_a, ents_b = G.read_hstable(s["files"][a]), G.read_hstable(s["files"][b])
    key = next(e.key for e in ents_a if any(x.key == e.key for x in ents_b))
    m_a = M.Model({a: s["files"][a]}, orc, 1)
    m_ab = M.Model({g: s["files"][g] for g in (a, b)}, orc, 1)
    assert m_a.get(key)[0] == 0 and m_ab.get(key)[0] == 0 and m_a.get(key)[2] >> 32 != m_ab.get(key)[2] >> 32
    ix = HSTableIndex({a: s["files"][a]}, 1, reserve=room(s["files"], [b]))
    try:
        assert ix.get([key]) == [m_a.get(key)[:2]]
        ix.add_files({b: s["files"][b]})
        assert ix.get([key]) == [m_ab.get(key)[:2]]
        where, _ = ix.locate([key])
        assert int(where[0]) == m_ab.get(key)[2]
    finally:
        ix.close()


# ------------------------------------------------------------- 5. refusals
def _zero_magic(f):
    b = bytearray(f)
    b[len(f) - 12:len(f) - 4] = bytes(8)
    return bytes(b)


def _short_one_varint(f, orc):
    ftype, flags, oi, num, magic, _ = M.footer(f)
    arr = f[oi:len(f) - M.FOOTER]
    end = len(arr) - 1                            # drop the last varint (the last row's offset)
    while end > 0 and arr[end - 1] & 0x80:
        end -= 1
    head = f[:oi] + arr[:end] + struct.pack("<IIQQQ", ftype, flags, oi, num, magic)
    return head + struct.pack("<I", orc.crc32c(head[oi:]))


def test_files_that_do_not_load_among_good_ones(gpu, streams, orc):
    """Added in one call: two good files, one with a malformed offset array
    (-3, found by the parse, so the rows are numbered a second time), one
    without a footer magic (-1) and one cut at 8192 bytes (-2)."""
    from kingdb_amd.index import HSTableIndex
    s = streams["get_keys_xx"]
    f1, f2, f3, f4 = (s["files"][f] for f in s["order"])
    n1, n2, n3, n4 = s["order"]
    files = {n1: f1, n2: f2, n3: _short_one_varint(f3, orc), n4: f4, "00000005": _zero_magic(f4), "00000006": f4[:8192]}
    want_status = {n1: 0, n2: 0, n3: -3, n4: 0, "00000005": -1, "00000006": -2}
    m = M.Model(files, orc, 1)
    assert m.file_status == want_status
    q = queries(s["keys"])
    added = [f for f in files if f != n1]
    ix = HSTableIndex({n1: f1}, 1, reserve=room(files, added))
    fr = HSTableIndex(files, 1)
    try:
        assert ix.add_files({f: files[f] for f in added}) == {f: want_status[f] for f in added}
        good = rows_of(f2) + rows_of(f4)
        assert ix.add_stats() == (0, buckets(rows_of(f1) + good), good + rows_of(f3) + good)
        snap = snapshot(ix, q)
        assert_model(snap, m, q)
        assert snap == snapshot(fr, q)
    finally:
        ix.close()
        fr.close()


def test_refused_adds_leave_the_index_as_it_was(gpu, streams, orc):
    from kingdb_amd import _lib
    from kingdb_amd.index import FILE_ORDER, HSTableIndex
    s = streams["get_keys_xx"]
    files, q = s["files"], queries(s["keys"])
    n1, n2, n3, n4 = s["order"]
    held = {n1: files[n1], n3: files[n3]}
    m = M.Model(held, orc, 1)
    ix = HSTableIndex(held, 1, reserve=room(files, [n2, n4, n3]))
    try:
        before = snapshot(ix, q)
        assert_model(before, m, q)
        # an older file after a newer one, alone and beside a good one; then a file the index holds
        off, size, fid, _ = place(ix, files, [n2, n4, n3])
        for pick, want in (([0], [FILE_ORDER]), ([0, 1], [FILE_ORDER, 0]), ([1, 0], [0, FILE_ORDER]),
                           ([2], [FILE_ORDER]), ([2, 1], [FILE_ORDER, 0])):
            rc, status, added = add_rc(ix, off[pick].copy(), size[pick].copy(), fid[pick].copy())
            assert (rc, status, added) == (_lib.EINVAL, want, 0), pick
            assert snapshot(ix, q) == before, pick
        # another buffer than the handle's
        rc, status, added = add_rc(ix, off[1:2].copy(), size[1:2].copy(), fid[1:2].copy(), d_files=ix.files.ptr + 64)
        assert (rc, added) == (_lib.EINVAL, 0)
        assert snapshot(ix, q) == before
        assert _lib.load().kdb_index_add_stats(ix.h, None, None, None) == _lib.EINVAL     # no add has succeeded
        # the index is usable: the newer file goes in
        assert ix._add(None, off[1:2], size[1:2], fid[1:2]) == {n4: 0}
        want = {n1: files[n1], n3: files[n3], n4: files[n4]}
        snap = snapshot(ix, q)
        assert_model(snap, M.Model(want, orc, 1), q)
        fr = HSTableIndex(want, 1)
        try:
            assert snap == snapshot(fr, q)
        finally:
            fr.close()
    finally:
        ix.close()


# ------------------------------------------------------------- 6. scan
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


@pytest.mark.parametrize("stream", ["get_keys_xx", "key_lengths_xx"])
def test_scan_after_an_add(gpu, streams, orc, stream):
    from kingdb_amd import _lib
    from kingdb_amd.index import HSTableIndex
    s = streams[stream]
    files, order = s["files"], s["order"]
    want = S.scan(M.Model(files, orc, s["hash_type"]))
    ix = HSTableIndex({f: files[f] for f in order[:-1]}, s["hash_type"], reserve=room(files, order[-1:]))
    fr = HSTableIndex(files, s["hash_type"])
    try:
        live = ix.scan_prepare()
        assert live > 0 and batch_raw(ix, 0, 1, 1000) == 0
        assert list(ix.items()) == S.scan(M.Model({f: files[f] for f in order[:-1]}, orc, s["hash_type"]))
        ix.add_files({order[-1]: files[order[-1]]})
        assert batch_raw(ix, 0, 1, 1000) == _lib.EINVAL            # the prepared list is gone
        assert _lib.load().kdb_index_scan_sort_steps(ix.h, ctypes.byref(ctypes.c_uint32(0))) == _lib.EINVAL
        got = list(ix.items())                                     # prepares again
        assert got == list(fr.items()) == want
        assert ix.scan_prepare() == len(want) and batch_raw(ix, 0, 1, 1000) == 0
        if stream == "key_lengths_xx":
            assert {len(k) for k, _, _ in got} >= {1, 1000}
    finally:
        ix.close()
        fr.close()


# ------------------------------------------------------------- 7. the writer loop
def test_writer_refresh_loop(gpu, orc):
    """write -> refresh -> Get on a DeviceHSTableWriter with 64 KiB files."""
    import oracle
    from kingdb_amd import _lib, put
    from kingdb_amd import get as G
    from kingdb_amd.index import HSTableIndex, NOTFOUND
    rng = np.random.default_rng(1234)
    pool = oracle.g1_pool(orc)
    batches, known = [], []
    for b in range(6):
        puts = []
        for i in range(150):
            if known and i % 3 == 0:
                k = known[int(rng.integers(0, len(known)))]             # an overwrite
            else:
                k = rng.integers(0, 256, int(rng.integers(8, 41)), dtype=np.uint8).tobytes()
                known.append(k)
            n, at = int(rng.integers(100, 601)), int(rng.integers(0, len(pool) - 600))
            puts.append((k, pool[at:at + n].tobytes()))
        batches.append(puts)
    every = [p for puts in batches for p in puts]
    hs = 64 << 10
    w = put.DeviceHSTableWriter(hs, 1, put.DeviceHSTableWriter.arena_bytes(
        hs, sum(put.entries_bound(p) for p in batches), len(every)))
    ix = HSTableIndex.from_resident(w)
    try:
        assert ix.entries == 0 and ix.refresh() == 0
        so_far, last, open_only_seen = [], {}, 0
        for step, puts in enumerate(batches + [None]):
            if puts is None:
                w.close()                                               # Database::Close: the open file closes
            else:
                b, n = put.put_entries_device(puts, 1)
                try:
                    w.append_batch(b, n)
                    _lib.check(_lib.load().kdb_lz4_stream_sync(None), "sync")
                finally:
                    b.free()
                for k, v in puts:
                    last[k] = v
                    if k not in so_far:
                        so_far.append(k)
            held = len(ix.names)
            added = ix.refresh()
            closed = w.files()
            assert ix.names == sorted(closed) and set(ix.file_status.values()) <= {0}
            assert added == sum(rows_of(closed[f]) for f in ix.names[held:])
            fr = HSTableIndex.from_resident(w)
            try:
                assert ix.entries == fr.entries
                for x, y in zip(ix.pairs(), fr.pairs()):
                    assert np.array_equal(x, y)
                got = ix.get(so_far)
                assert got == fr.get(so_far)
            finally:
                fr.close()
            # a key whose only entries are in the still open file cannot be read yet
            in_closed = {e.key for f in closed.values() for e in G.read_hstable(f)}
            for k, g in zip(so_far, got):
                if k not in in_closed:
                    assert g == (NOTFOUND, b"")
                    open_only_seen += 1
                else:
                    assert g[0] == 0
            assert ix.refresh() == 0 and len(ix.names) == len(closed)    # nothing new: nothing changes
            assert ix.get(so_far) == got
        assert open_only_seen > 0 and len(ix.names) >= 5
        assert ix.get(so_far) == [(0, last[k]) for k in so_far]
        assert ix.entries == len(every)
        assert sorted(k for k, _, _ in ix.items()) == sorted(last)
    finally:
        ix.close()
        w.free()


# ------------------------------------------------------------- 8. add_files with a reserve
def test_add_files_with_a_reserve(gpu, streams, fresh):
    from kingdb_amd.index import HSTableIndex
    s = streams["get_keys_xx"]
    files, order, q = s["files"], s["order"], queries(s["keys"])
    ix = HSTableIndex({order[0]: files[order[0]]}, s["hash_type"], reserve=room(files, order[1:2]))
    try:
        assert ix.add_files({order[1]: files[order[1]]}) == {order[1]: 0}
        assert snapshot(ix, q) == fresh("get_keys_xx", 2)
        with pytest.raises(ValueError):
            ix.add_files({order[2]: files[order[2]]})                   # one more than the reserve holds
        with pytest.raises(ValueError):
            ix.add_files({order[1]: files[order[1]]})                   # a name already held
        assert ix.names == order[:2]
        assert snapshot(ix, q) == fresh("get_keys_xx", 2)
    finally:
        ix.close()
    owned = HSTableIndex({}, 1)                                          # refresh() is the borrowed index's way
    try:
        with pytest.raises(ValueError):
            owned.refresh()
    finally:
        owned.close()
