"""GPU: Get by key, the scan, the writers and compaction on keys of every
length (csrc/index.hip, hash_device.h, hstable_dev.hip, kingdb_amd/index.py).

The fixture tests/golden/key_lengths.npz holds keys of 1..80, 127..129,
252..260, 300, 511..516 and 1000 bytes, twin keys that differ in one byte, and
hot keys put 70 and 130 times, in files the reference wrote.  Expectations
come from that fixture (the last value put per key, confirmed by the
reference's own Database::Get and iterator) and, for mutated files, from the
Python models of tests/index_model.py and tests/scan_model.py, which
tests/test_key_lengths_model.py pins to the fixture.  Every comparison is
exact: status, value bytes, key bytes, order.

What only these cases run: the key compare's byte tail and its second and
later strides (keys over 256 bytes), against a candidate of the same hash and
the same length; keys hashed from global memory (over 256 bytes) as queries
and as stored keys; the scan's key lengths through the sort and the prefix
with lengths that differ; the packed key copy's tail; crc32c(key) over more
than one 64-lane chunk; and a bucket scan of more than one stride.
"""
import random

import numpy as np
import pytest

import index_model as M
import keylens
import scan_model as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sets():
    return keylens.load()


@pytest.fixture(scope="module")
def models(sets, orc):
    return {name: M.Model(s["files"], orc, s["hash_type"]) for name, s in sets.items()}


@pytest.fixture(scope="module")
def scans(models):
    """The models' scans of the files as written, computed once per (stream,
    verify) and left unchanged."""
    cache = {}

    def scan(name, verify=0):
        if (name, verify) not in cache:
            cache[name, verify] = tuple(S.scan(models[name], verify))
        return list(cache[name, verify])
    return scan


def open_index(gpu, files, hash_type):
    from kingdb_amd.index import HSTableIndex
    return HSTableIndex(files, hash_type)


def assert_gets(ix, model, keys, verify=0):
    got = ix.get(keys, verify=verify)
    assert len(got) == len(keys)
    for k, (st, val) in zip(keys, got):
        wst, wval, _ = model.get(k, verify)
        assert (st, val) == (wst, wval), (len(k), verify, st, wst, len(val), len(wval))
    return got


def assert_same_files(got, want):
    assert sorted(got) == sorted(want)
    for f in want:
        assert len(got[f]) == len(want[f]), f
        assert got[f] == want[f], f                      # header block included, as in test_write_path.py


def hasher(orc, s):
    return orc.xxh64 if s["hash_type"] == 1 else orc.murmur3_64


def newest_file(files):
    """The last file in sequence order: the writers' timestamps and ids ascend together."""
    return sorted(files)[-1]


# ------------------------------------------------------------- the reference's files, read back
@pytest.mark.parametrize("verify", [0, 1, 2])
@pytest.mark.parametrize("name", ["xx", "murmur"])
def test_reference_files_read_back(gpu, sets, models, scans, orc, name, verify):
    """verify 1 as tests/test_gpu_scan.py::test_fixture_scan handles it: the
    reference's own value check reports -2 for some values, in the model as
    here, so there the values are asserted for the entries of status 0."""
    from kingdb_amd import _lib
    import ctypes
    s, m = sets[name], models[name]
    keys = s["keys"]
    want = scans(name, verify)
    ix = open_index(gpu, s["files"], s["hash_type"])
    try:
        assert set(ix.file_status.values()) == {0}
        assert ix.entries == len(s["puts"])
        got = assert_gets(ix, m, keys, verify)
        if verify != 1:
            assert got == [(0, s["last"][k]) for k in keys]
            for k, n, c, (st, val) in zip(keys, s["lens"], s["crcs"], got):
                assert (len(val), orc.crc32c(val)) == (int(n), int(c)), len(k)
        else:
            assert {st for st, _ in got} <= {0, -2}
            assert all(val == s["last"][k] for k, (st, val) in zip(keys, got) if st == 0)
        loc, st = ix.locate(keys, verify_header=1 if verify else 0)
        assert list(st) == [0] * len(keys)
        assert [int(x) for x in loc] == [m.get(k, verify)[2] for k in keys]
        # the scan
        live, kbytes, kmax = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
        rc = _lib.load().kdb_index_scan_prepare(ix.h, None, 1 if verify else 0, ctypes.byref(live),
                                                ctypes.byref(kbytes), ctypes.byref(kmax))
        assert rc == 0
        assert (live.value, kbytes.value, kmax.value) == S.prepare(m, verify)
        assert (live.value, kbytes.value, kmax.value) == (len(keys), sum(map(len, keys)), 1000)
        assert ix.scan_prepare(verify) == len(keys) == s["iterated"] and ix.scan_sort_steps() == 0
        got = ix.scan(verify=verify)
        assert got == want                                          # order and key bytes included
        assert sorted(k for k, _, _ in got) == keys
        if verify != 1:
            assert all(st == 0 and v == s["last"][k] for k, st, v in got)
        else:
            assert {st for _, st, _ in got} <= {0, -2}
            assert all(v == s["last"][k] for k, st, v in got if st == 0)
    finally:
        ix.close()


# ------------------------------------------------------------- absent near-misses
def flipped(k, at, x=0x40):
    b = bytearray(k)
    b[at] ^= x
    return bytes(b)


@pytest.mark.parametrize("name", ["xx", "murmur"])
def test_absent_near_misses(gpu, sets, name):
    from kingdb_amd.index import NOTFOUND
    s = sets[name]
    stored = set(s["keys"])
    rng = np.random.default_rng(5)
    absent = []
    for a, b, at in s["twins"]:                          # one more byte flipped, next to and far from the first
        n = len(a)
        for k in (a, b):
            absent += [flipped(k, (at + 1) % n), flipped(k, (at + n // 2) % n), flipped(k, at, 0x81)]
    absent += [k[:-1] for k in s["keys"]] + [k + b"\0" for k in s["keys"]] + [k + k[-1:] for k in s["keys"]]
    absent.insert(len(absent) // 2, b"")                 # the empty key, between others
    absent += [rng.integers(0, 256, 257, dtype=np.uint8).tobytes(), rng.integers(0, 256, 5000, dtype=np.uint8).tobytes()]
    absent = [k for k in absent if k not in stored]      # (a key minus its last byte may be a stored key)
    assert b"" in absent and len(absent) > 3 * len(s["keys"])
    ix = open_index(gpu, s["files"], s["hash_type"])
    try:
        for verify in (0, 2):
            # stored keys in between: a batch of hits and misses
            keys = absent[:50] + s["keys"][:20] + absent[50:]
            got = ix.get(keys, verify=verify)
            want = [(0, s["last"][k]) if k in stored else (NOTFOUND, b"") for k in keys]
            assert got == want
        loc, st = ix.locate(absent)
        assert list(st) == [NOTFOUND] * len(absent)
        assert all(int(x) == 0 for x in loc)
        assert ix.get([b""]) == [(NOTFOUND, b"")]          # a batch with no key byte at all
    finally:
        ix.close()


# ------------------------------------------------------------- forged same-hash, same-length candidates
def forged_twins(s, orc):
    """For each twin pair (A, B): the row of A's newest entry carries
    hash(B'), B' = A with the byte at the pair's position changed to a value
    neither A nor B has there, so B' is not stored.  (files, [(A, B', position)])."""
    h = hasher(orc, s)
    from kingdb_amd import get as G
    files = dict(s["files"])
    rows = {f: M.parse_rows(b) for f, b in files.items()}
    ents = {f: G.read_hstable(b) for f, b in files.items()}
    stored = set(s["keys"])
    out = []
    for a, b, at in s["twins"]:
        bp = bytearray(a)
        bp[at] = next(x for x in range(256) if x not in (a[at], b[at]))
        bp = bytes(bp)
        assert bp not in stored and len(bp) == len(a)
        f, i = max((f, i) for f in files for i, e in enumerate(ents[f]) if e.key == a)     # A's newest entry
        rows[f][i] = (h(bp), rows[f][i][1])
        out.append((a, bp, at))
    for f in files:
        files[f] = M.with_rows(files[f], rows[f], orc)
    return files, out


@pytest.mark.parametrize("verify", [0, 1])
@pytest.mark.parametrize("name", ["xx", "murmur"])
def test_forged_same_hash_same_length(gpu, sets, orc, name, verify):
    """The one case that reaches the key compare with a key that differs: a
    candidate of the query's hash and the query's length."""
    from kingdb_amd.index import NOTFOUND
    s = sets[name]
    files, pairs = forged_twins(s, orc)
    spots = {(len(a), at) for a, _, at in pairs}
    # byte 0; the last byte for klen % 4 = 1, 2, 3 (the byte tail); bytes 255 and 256 (the LDS stage's
    # edge and the second stride's first word); byte klen - 2 of the 1000-byte key (the fourth stride)
    assert (16, 0) in spots and (1000, 998) in spots
    assert {n % 4 for n, at in spots if at == n - 1} >= {1, 2, 3}
    assert {255, 256} <= {at for _, at in spots}
    assert {(259, 255), (260, 256)} <= spots               # and those two not as the last byte
    m = M.Model(files, orc, s["hash_type"])
    want_scan = S.scan(m, verify)
    ix = open_index(gpu, files, s["hash_type"])
    try:
        assert set(ix.file_status.values()) == {0}
        for a, bp, at in pairs:
            assert m.get(bp, verify)[0] == NOTFOUND        # the model, for the record
        got = ix.get([bp for _, bp, _ in pairs], verify=verify)
        assert got == [(NOTFOUND, b"")] * len(pairs), [(len(a), at) for (a, _, at), g in zip(pairs, got)
                                                       if g != (NOTFOUND, b"")]
        got_a = assert_gets(ix, m, [a for a, _, _ in pairs], verify)   # an older A, or NotFound
        assert {st for st, _ in got_a} <= {0, -2, NOTFOUND} and NOTFOUND in {st for st, _ in got_a}
        assert_gets(ix, m, s["keys"], verify)
        assert ix.scan(verify=verify) == want_scan
        # A's forged row is dead: A is in the scan only through an older entry
        in_scan = {k for k, _, _ in want_scan}
        for (a, _, _), (st, _) in zip(pairs, got_a):
            assert (a in in_scan) == (st != NOTFOUND)
    finally:
        ix.close()


# ------------------------------------------------------------- crowded buckets
@pytest.mark.parametrize("name", ["xx", "murmur"])
def test_hot_keys_as_written(gpu, sets, scans, orc, name):
    s = sets[name]
    h = hasher(orc, s)
    ix = open_index(gpu, s["files"], s["hash_type"])
    try:
        assert ix.entries == len(s["puts"])                # every row counted, the overwritten ones too
        hashes, _ = ix.pairs()
        for k, times in zip(s["hot"], (70, 130)):
            vals = [v for kk, v, _ in s["puts"] if kk == k]
            assert len(vals) == times and len(set(vals)) == times
            assert int((hashes == np.uint64(h(k))).sum()) == times
            for verify in (0, 2):
                assert ix.get([k], verify=verify) == [(0, vals[-1])]
            got = [(st, v) for kk, st, v in ix.scan() if kk == k]
            assert got == [(0, vals[-1])]                   # once, with the newest value
        assert ix.scan() == scans(name)
    finally:
        ix.close()


@pytest.mark.parametrize("name", ["xx", "murmur"])
def test_crowded_bucket_of_other_keys(gpu, sets, orc, name):
    """100 entries of other 19-byte keys, appended to the newest file, whose
    rows carry the hot key's hash and are newer than every row of the hot key:
    get(hot) walks past all 100 rejections to the hot key's newest entry, and
    the 100 keys cannot be reached."""
    from kingdb_amd import get as G
    from kingdb_amd import put
    from kingdb_amd.index import NOTFOUND
    s = sets[name]
    h = hasher(orc, s)
    hot = s["hot"][0]
    assert len(hot) == 19
    rng = np.random.default_rng(77)
    others = [rng.integers(0, 256, 19, dtype=np.uint8).tobytes() for _ in range(100)]
    assert len(set(others) | set(s["keys"])) == 100 + len(s["keys"])
    (donor,) = put.write_hstables([(k, b"crowd %03d" % i * 3) for i, k in enumerate(others)], 32 << 20,
                                  s["hash_type"]).values()
    d_oi = M.footer(donor)[2]
    d_ents = G.read_hstable(donor)
    assert [e.key for e in d_ents] == others
    fname = newest_file(s["files"])
    f = s["files"][fname]
    oi = M.footer(f)[2]
    rows = M.parse_rows(f) + [(h(hot), oi + e.offset - M.HEADER) for e in d_ents]
    files = dict(s["files"])
    files[fname] = M.with_rows(f, rows, orc, f[:oi] + donor[M.HEADER:d_oi])
    m = M.Model(files, orc, s["hash_type"])
    assert m.file_status[fname] == 0
    want_scan = S.scan(m)
    ix = open_index(gpu, files, s["hash_type"])
    try:
        assert set(ix.file_status.values()) == {0}
        assert ix.entries == len(s["puts"]) + 100
        hashes, _ = ix.pairs()
        assert int((hashes == np.uint64(h(hot))).sum()) == 170 > 128   # equal hashes share a bucket: three strides
        for verify in (0, 2):
            got = assert_gets(ix, m, [hot] + others + s["keys"], verify)
            assert got[0] == (0, s["last"][hot])
            assert got[1:101] == [(NOTFOUND, b"")] * 100
        got = ix.scan()
        assert got == want_scan
        assert sorted(k for k, _, _ in got) == s["keys"]    # the hot key once, none of the 100
    finally:
        ix.close()


@pytest.mark.parametrize("hash_type", [1, 0])
def test_crowded_bucket_of_reachable_keys(gpu, orc, hash_type):
    """80 keys of six lengths whose hashes agree in their low 10 bits, alone in
    one file: 80 rows make at most 1024 buckets of hash & (B - 1), so all 80
    share one, and every one of them has to be found there -- whatever order
    the bucket's slots are in, 16 of them lie beyond the first 64."""
    from kingdb_amd import put
    h = orc.xxh64 if hash_type == 1 else orc.murmur3_64
    blob = np.random.default_rng(90 + hash_type).integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()
    lengths = (5, 19, 67, 255, 257, 300)
    keys, low = [], h(blob[:5]) & 1023
    for at in range(0, len(blob) - 300, 5):                 # windows of the blob: some 80 in 80 x 1024 match
        k = blob[at:at + lengths[len(keys) % 6]]
        if h(k) & 1023 == low and k not in keys:
            keys.append(k)
            if len(keys) == 80:
                break
    assert len(keys) == 80
    puts = [(k, b"value %02d of the crowd " % i * (1 + i % 5)) for i, k in enumerate(keys)]
    files = put.write_hstables(puts, 32 << 20, hash_type)
    assert len(files) == 1
    m = M.Model(files, orc, hash_type)
    want_scan = S.scan(m)
    assert [(k, v) for k, _, v in want_scan] == puts
    ix = open_index(gpu, files, hash_type)
    try:
        hashes, _ = ix.pairs()
        assert ix.entries == 80 and 2 * ix.entries <= 1024
        assert {int(x) & 1023 for x in hashes} == {low} and len({int(x) for x in hashes}) == 80
        for verify in (0, 2):
            assert ix.get(keys, verify=verify) == [(0, v) for _, v in puts]
        assert_gets(ix, m, [k[:-1] for k in keys] + [flipped(k, len(k) - 1) for k in keys])
        assert ix.scan() == want_scan
    finally:
        ix.close()


# ------------------------------------------------------------- the sort, with lengths that differ
@pytest.mark.parametrize("how", ["reversed", "shuffled"])
@pytest.mark.parametrize("name", ["xx", "murmur"])
def test_sort_with_mixed_lengths(gpu, sets, orc, name, how):
    s = sets[name]
    fname = sorted(s["files"])[1]
    rows = M.parse_rows(s["files"][fname])
    if how == "reversed":
        rows = rows[::-1]
    else:
        random.Random(20).shuffle(rows)
    files = dict(s["files"])
    files[fname] = M.with_rows(s["files"][fname], rows, orc)
    m = M.Model(files, orc, s["hash_type"])
    want = S.scan(m)
    in_file = [len(k) for _, _, n, k in S.live_rows(m) if n == fname]
    assert len(set(in_file)) > 20 and max(in_file) > 256   # the rows that move carry many lengths
    assert len(want) & (len(want) - 1) != 0                # no power of two: the network is padded
    ix = open_index(gpu, files, s["hash_type"])
    try:
        live = ix.scan_prepare()
        assert ix.scan_sort_steps() > 0
        assert live == len(want) == S.prepare(m)[0]
        assert ix.scan() == want
        assert ix.scan(3, 70) == want[3:73]
        assert_gets(ix, m, s["keys"])
    finally:
        ix.close()


# ------------------------------------------------------------- windows and keys_cap
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


@pytest.mark.parametrize("name", ["xx", "murmur"])
def test_windows_and_keys_cap(gpu, sets, scans, name):
    from kingdb_amd import _lib
    s = sets[name]
    want = scans(name)
    ix = open_index(gpu, s["files"], s["hash_type"])
    try:
        live = ix.scan_prepare()
        assert live == len(want) > 65
        for w in (1, 7, 64, 65, live):
            got = []
            for first in range(0, live, w):
                got += ix.scan(first, min(w, live - first))
            assert got == want, w
        assert list(ix.items(batch=7)) == want
        at = next(i for i, (k, _, _) in enumerate(want) if len(k) == 1000)
        first = max(at - 3, 0)
        n = min(9, live - first)
        lens = [len(k) for k, _, _ in want[first:first + n]]
        need = sum(lens)
        assert 1000 in lens and len(set(lens)) > 3
        assert batch_raw(ix, first, n, need) == 0
        assert batch_raw(ix, first, n, need - 1) == _lib.EINVAL   # keys_cap one byte short
        assert batch_raw(ix, at, 1, 1000) == 0
        assert batch_raw(ix, at, 1, 999) == _lib.EINVAL
    finally:
        ix.close()


# ------------------------------------------------------------- this project's writers
@pytest.mark.parametrize("name", ["xx", "murmur"])
def test_project_writers(gpu, sets, name):
    from kingdb_amd import put
    from kingdb_amd.index import HSTableIndex
    s = sets[name]
    puts, hs, ht = s["puts"], s["hstable_size"], s["hash_type"]
    assert_same_files(put.write_hstables(puts, hs, ht), s["files"])
    assert_same_files(put.write_hstables_device(puts, hs, ht), s["files"])
    keys = s["keys"] + [b"", s["keys"][-1] + b"x"]
    ref = HSTableIndex(s["files"], ht)
    try:
        want_get, want_scan = ref.get(keys), ref.scan()
    finally:
        ref.close()
    assert want_get[:len(s["keys"])] == [(0, s["last"][k]) for k in s["keys"]]
    w = put.DeviceHSTableWriter(hs, ht, put.DeviceHSTableWriter.arena_bytes(hs, put.entries_bound(puts), len(puts)))
    try:
        b, n = put.put_entries_device(puts, ht)
        try:
            w.append_batch(b, n)
        finally:
            b.free()
        w.close()
        assert_same_files(w.files(), s["files"])
        ix = HSTableIndex.from_resident(w)
        try:
            assert ix.file_status == {f: 0 for f in s["files"]}
            assert ix.entries == len(puts)
            assert ix.get(keys) == want_get
            assert ix.scan() == want_scan
        finally:
            ix.close()
    finally:
        w.free()


# ------------------------------------------------------------- compaction
@pytest.mark.parametrize("batch", [16, 65536])
@pytest.mark.parametrize("name", ["xx", "murmur"])
def test_compaction(gpu, sets, scans, orc, name, batch):
    from kingdb_amd.index import HSTableIndex
    s = sets[name]
    hs, ht = s["hstable_size"], s["hash_type"]
    live = scans(name)
    src = HSTableIndex(s["files"], ht)
    w = None
    try:
        before = src.get(s["keys"])
        assert before == [(0, s["last"][k]) for k in s["keys"]]
        want = src.compacted(hs, batch)
        w = src.compacted_device(hs, batch)
        assert len(want) >= 1
        assert_same_files(w.files(), want)
        for ix in (HSTableIndex(want, ht), HSTableIndex.from_resident(w)):
            try:
                assert set(ix.file_status.values()) == {0}
                assert ix.entries == len(live) == ix.scan_prepare()        # exactly the live set
                got = ix.scan()
                assert got == S.scan(M.Model(want, orc, ht))
                assert sorted(got) == sorted(live)                          # the same (key, status, value)
                assert [k for k, _, _ in got] == [k for k, _, _ in live]   # written in scan order
                assert ix.get(s["keys"]) == before
            finally:
                ix.close()
    finally:
        src.close()
        if w is not None:
            w.free()
