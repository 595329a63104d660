"""GPU: read your writes -- the open file's tail of an index
(include/kdb_index_tail.h, csrc/index.hip, HSTableIndex.refresh(tail=True)).

The contract under test: after refresh(tail=True) the index is
indistinguishable, through entries, pairs(), Get, locate and the scan, from an
HSTableIndex made fresh over the files the writer would hold if it closed now.
The expectation for a prefix of batches is exactly that: a second writer fed
the same batches and closed, a fresh HSTableIndex over its files, and the
Python model of tests/index_model.py over the same files (the device writer's
files are pinned byte for byte to the host writer and the reference by
tests/test_gpu_hstable_dev.py).  Every comparison is exact.

The put stream is made here: 600 items over 200 keys of every length 1..80 and
127-129, 255-257, 1000; values of 0..300 bytes and a few of 5 000; one item in
twenty a delete.  It is fed in uneven batches (1, 7, 64, 65, 129, ...), one of
them split where the file it is writing reaches hstable_size, so that one
refresh falls exactly on a close; hstable_size gives about nine files, so the
batches of 129 and 130 items open and close whole files between two refreshes.
"""
import ctypes

import numpy as np
import pytest

import index_model as M

pytestmark = pytest.mark.gpu

SIZES = [1, 7, 64, 65, 129, 3, 40, 1, 90, 2, 130, 68]
KEY_LENGTHS = list(range(1, 81)) + [127, 128, 129, 255, 256, 257, 1000]
HEADER = 8192


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
    if rows == 0:
        return 0
    b = 2
    while b < 2 * rows:
        b <<= 1
    return b


def snapshot(ix, q):
    """What the public interface shows of an index's rows: entries, pairs, Get and locate of `q`."""
    h, loc = ix.pairs()
    where, st = ix.locate(q)
    return {"entries": ix.entries, "hash": [int(x) for x in h], "loc": [int(x) for x in loc], "get": ix.get(q),
            "where": [int(x) for x in where], "status": [int(x) for x in st]}


def assert_model(snap, m, q):
    want = m.pairs()
    assert snap["entries"] == len(want)
    assert snap["hash"] == [w[0] for w in want] and snap["loc"] == [w[1] for w in want]
    for k, (st, val), where in zip(q, snap["get"], snap["where"]):
        wst, wval, wloc = m.get(k)
        assert (st, val, where) == (wst, wval, wloc), (k, st, wst)


def make_stream(orc, seed):
    """(items, keys): the seeded put stream of the module docstring."""
    import oracle
    from kingdb_amd import put
    rng = np.random.default_rng(seed)
    pool = oracle.g1_pool(orc)
    keys, seen = [], set()
    for i in range(200):
        n = KEY_LENGTHS[i % len(KEY_LENGTHS)]
        k = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        while k in seen:
            k = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        seen.add(k)
        keys.append(k)
    order = rng.permutation(np.concatenate([np.arange(200), rng.integers(0, 200, 400)]))
    big = set(int(x) for x in rng.choice(600, 6, replace=False))
    items = []
    for i, ki in enumerate(order):
        if rng.random() < 0.05:
            items.append((keys[int(ki)], put.DELETE))
            continue
        n = 5000 if i in big else int(rng.integers(0, 301))
        at = int(rng.integers(0, len(pool) - n))
        items.append((keys[int(ki)], pool[at:at + n].tobytes()))
    assert sum(1 for it in items if put.is_delete(it)) >= 10
    return items, keys


def simulate(entry_len, sb, bounds):
    """The cut rule of csrc/hstable_cut.h over entries without marks: for each
    batch [a, b) the indices before which a file closed, and whether the file
    closed at the batch's end."""
    out = []
    fsize = 0
    for a, b in bounds:
        mid = []
        for i in range(a, b):
            if fsize > sb:
                mid.append(i)
                fsize = 0
            if fsize == 0:
                fsize = HEADER
            fsize += int(entry_len[i])
        end = fsize >= sb
        if end:
            fsize = 0
        out.append((mid, end))
    return out


def plan_batches(items, ht):
    """(hstable_size, batches): SIZES, with the first batch of three or more
    items that closes a file between two of its entries -- after the start of
    the stream -- split there, so that its first part ends exactly on the close."""
    from kingdb_amd import put
    r = put.put_entries(items, ht)
    assert all(int(s) == 0 for s in r.status)
    entry_len = [int(x) for x in r.entry_len]
    sb = HEADER + sum(entry_len) // 9
    bounds, at = [], 0
    for n in SIZES:
        bounds.append((at, at + n))
        at += n
    assert at == len(items)
    sim = simulate(entry_len, sb, bounds)
    for bi in range(3, len(bounds)):
        (a, b), (mid, _) = bounds[bi], sim[bi]
        cut = [j for j in mid if j > a]
        if cut:
            bounds[bi:bi + 1] = [(a, cut[0]), (cut[0], b)]
            break
    else:
        raise AssertionError("no batch closes a file between two entries")
    return sb, [items[a:b] for a, b in bounds]


def feed(w, puts, ht):
    from kingdb_amd import _lib, put
    b, n = put.put_entries_device(puts, ht)
    try:
        w.append_batch(b, n)
        _lib.check(_lib.load().kdb_lz4_stream_sync(None), "sync")
    finally:
        b.free()


def new_writer(sb, ht, batches, closes=0):
    """A writer whose arena holds the batches, and the files `closes` calls of close() cut short."""
    from kingdb_amd import put
    n = sum(len(b) for b in batches)
    return put.DeviceHSTableWriter(sb, ht, put.DeviceHSTableWriter.arena_bytes(
        sb, sum(put.entries_bound(b) for b in batches), max(n, 1)) + closes * (HEADER + 36 + 2 * 64))


def closed_form(sb, ht, batches, upto):
    """The files a writer fed batches[:upto] holds once closed."""
    w = new_writer(sb, ht, batches)
    try:
        for puts in batches[:upto]:
            feed(w, puts, ht)
        w.close()
        return w.files()
    finally:
        w.free()


def open_record(w):
    f = w.open_file()
    return None if f is None else {n: int(getattr(f, n)) for n, _ in f._fields_}


def tail_of(record):
    """What HSTableIndex.tail shows of an open_file() record."""
    if record is None or record["incomplete"]:
        return None
    return {"fileid": record["fileid"], "rows": record["rows"], "bytes": record["bytes"]}


class Run:
    """One writer driven through the batches, refresh(tail=True) after each,
    with a second index refreshed with reparse=True: what every step showed,
    and the expectation for it."""


@pytest.fixture(scope="module")
def runs(gpu, orc):
    from kingdb_amd.index import HSTableIndex
    cache = {}

    def get(ht):
        if ht in cache:
            return cache[ht]
        items, keys = make_stream(orc, 20260 + ht)
        sb, batches = plan_batches(items, ht)
        q = queries(keys)
        r = Run()
        r.ht, r.sb, r.batches, r.keys, r.q, r.steps = ht, sb, batches, keys, q, []
        w = new_writer(sb, ht, batches)
        ix = HSTableIndex.from_resident(w)
        rp = HSTableIndex.from_resident(w)
        try:
            for step, puts in enumerate(batches, 1):
                feed(w, puts, ht)
                before = ix.entries
                added = ix.refresh(tail=True)
                rp.refresh(tail=True, reparse=True)
                files = closed_form(sb, ht, batches, step)
                fr = HSTableIndex(files, ht)
                try:
                    want = snapshot(fr, q)
                    want_items = list(fr.items())
                    want_sort = fr.scan_sort_steps()
                finally:
                    fr.close()
                r.steps.append({
                    "got": snapshot(ix, q), "reparse": snapshot(rp, q), "want": want, "files": files,
                    "added": added, "before": before, "tail": ix.tail, "open": open_record(w),
                    "stats": ix.tail_stats(), "reparse_stats": rp.tail_stats(), "names": list(ix.names),
                    "file_status": dict(ix.file_status), "closed": sorted("%08x" % int(f) for f in w.resident()[3]),
                    "items": list(ix.items()), "sort": ix.scan_sort_steps(), "want_items": want_items,
                    "want_sort": want_sort})
        finally:
            ix.close()
            rp.close()
            w.free()
        cache[ht] = r
        return r
    return get


# ------------------------------------------------------------- 1. read your writes, every step
@pytest.mark.parametrize("ht", [1, 0], ids=["xxhash64", "murmur3"])
def test_read_your_writes_every_step(gpu, runs, orc, ht):
    r = runs(ht)
    closes, mid_file, on_a_close, whole_file = 0, 0, 0, 0
    was_open, held = False, 0
    for step, s in enumerate(r.steps, 1):
        assert s["got"] == s["want"], step
        assert_model(s["want"], M.Model(s["files"], orc, ht), r.q)
        assert s["tail"] == tail_of(s["open"]), step
        assert s["names"] == s["closed"] and set(s["file_status"].values()) <= {0}
        assert s["added"] == s["got"]["entries"] - s["before"]
        assert s["got"]["entries"] == sum(len(b) for b in r.batches[:step])
        grew = len(s["closed"]) - held
        closes += grew
        mid_file += s["open"] is not None and s["open"]["rows"] > 0
        on_a_close += s["open"] is None and grew > 0
        whole_file += grew - (1 if was_open else 0) >= 1      # a file this batch opened is closed already
        was_open, held = s["open"] is not None, len(s["closed"])
    # what the module docstring says of the batches
    assert closes >= 4 and mid_file >= 4 and on_a_close >= 1 and whole_file >= 1, (closes, mid_file, on_a_close,
                                                                                    whole_file)
    # every put of the stream is readable at the end, the last version of each key
    from kingdb_amd import put
    from kingdb_amd.index import DELETED
    last = {}
    for puts in r.batches:
        for it in puts:
            last[it[0]] = it[1]
    final = dict(zip(r.q, r.steps[-1]["got"]["get"]))
    for k, v in last.items():
        assert final[k] == ((DELETED, b"") if v is put.DELETE else (0, v)), k


# ------------------------------------------------------------- 2. versions across the boundary
def test_versions_across_the_boundary(gpu, orc):
    from kingdb_amd import put
    from kingdb_amd.index import DELETED, NOTFOUND, HSTableIndex
    A, B, C, D, E, F = (b"key-" + c * 9 for c in (b"a", b"b", b"c", b"d", b"e", b"f"))
    v = {n: bytes([65 + n]) * (40 + n) for n in range(12)}
    batches = [[(A, v[0]), (B, v[1]), (C, v[2]), (D, v[3])],
               [(A, v[4]), (B, put.DELETE), (E, v[5]), (E, v[6]), (F, v[7]), (D, put.DELETE)],
               [(F, v[8]), (D, v[9])]]
    keys = [A, B, C, D, E, F]
    sb = 1 << 20
    w = new_writer(sb, 1, batches, closes=2)
    ix = HSTableIndex.from_resident(w)
    try:
        feed(w, batches[0], 1)
        w.close()                                             # file 1 is closed; what follows stays open
        assert ix.refresh(tail=True) == 4 and ix.tail is None and ix.names == ["00000001"]
        assert ix.get(keys) == [(0, v[0]), (0, v[1]), (0, v[2]), (0, v[3]), (NOTFOUND, b""), (NOTFOUND, b"")]
        feed(w, batches[1], 1)
        assert ix.refresh() == 0                              # without tail=True nothing of the open file is read
        assert ix.get([A, E]) == [(0, v[0]), (NOTFOUND, b"")]
        assert ix.refresh(tail=True) == 6
        assert ix.tail == {"fileid": 2, "rows": 6, "bytes": w.open_bytes()} and ix.entries == 10
        # overwritten in the tail, deleted in the tail, untouched, deleted, put twice in one batch, new
        assert ix.get(keys) == [(0, v[4]), (DELETED, b""), (0, v[2]), (DELETED, b""), (0, v[6]), (0, v[7])]
        where, st = ix.locate(keys)
        assert [int(x) >> 32 for x in where] == [2, 2, 1, 2, 2, 2] and [int(x) for x in st] == [0, DELETED, 0, DELETED, 0, 0]
        feed(w, batches[2], 1)
        assert ix.refresh(tail=True) == 2 and ix.tail["rows"] == 8 and ix.names == ["00000001"]
        # put again in a second batch of the tail; deleted in the tail and then put again
        assert ix.get(keys) == [(0, v[4]), (DELETED, b""), (0, v[2]), (0, v[9]), (0, v[6]), (0, v[8])]
        want = closed_form_two(sb, batches)
        fr = HSTableIndex(want, 1)
        try:
            q = queries(keys)
            assert snapshot(ix, q) == snapshot(fr, q)
            assert_model(snapshot(ix, q), M.Model(want, orc, 1), q)
        finally:
            fr.close()
    finally:
        ix.close()
        w.free()


def closed_form_two(sb, batches):
    """closed_form() with a close after the first batch, as the test above drives its writer."""
    w = new_writer(sb, 1, batches, closes=2)
    try:
        feed(w, batches[0], 1)
        w.close()
        for puts in batches[1:]:
            feed(w, puts, 1)
        w.close()
        return w.files()
    finally:
        w.free()


# ------------------------------------------------------------- 3. the incremental parse
def test_incremental_parse_and_buckets(gpu, runs):
    r = runs(1)
    prev = None
    doubled = stayed = 0
    for step, s in enumerate(r.steps, 1):
        held, fid, rows, nbytes, parsed, nb = s["stats"]
        tail = s["tail"]
        assert (held, fid, rows, nbytes) == ((1, tail["fileid"], tail["rows"], tail["bytes"]) if tail else (0, 0, 0, 0))
        same = bool(tail and prev and prev["tail"] and prev["tail"]["fileid"] == tail["fileid"])
        # only the rows registered since the previous set_tail on the same file
        assert parsed == (rows - prev["tail"]["rows"] if same else rows), step
        assert nb == buckets(s["got"]["entries"])
        # the handle driven with KDB_INDEX_TAIL_REPARSE: everything parsed again, the same handle
        assert s["reparse"] == s["got"], step
        assert s["reparse_stats"] == (held, fid, rows, nbytes, rows, nb), step
        if same:
            doubled += nb > prev["stats"][5]
            stayed += nb == prev["stats"][5]
        prev = s
    assert doubled >= 1 and stayed >= 1, (doubled, stayed)


def test_refresh_with_nothing_appended_parses_nothing(gpu, orc):
    from kingdb_amd.index import HSTableIndex
    puts = [(b"k%03d" % i, b"v" * i) for i in range(30)]
    w = new_writer(1 << 20, 1, [puts, puts])
    ix = HSTableIndex.from_resident(w)
    try:
        feed(w, puts, 1)
        assert ix.refresh(tail=True) == 30 and ix.tail_stats()[4] == 30
        live = ix.scan_prepare()
        assert live == 30
        assert ix.refresh(tail=True) == 0 and ix.tail_stats()[4] == 0 and ix.entries == 30
        assert ix.refresh(tail=True, reparse=True) == 0 and ix.tail_stats()[4] == 30 and ix.entries == 30
        feed(w, puts[:5], 1)
        assert ix.refresh(tail=True) == 5 and ix.tail_stats()[4] == 5 and ix.tail["rows"] == 35
        assert ix.get([p[0] for p in puts]) == [(0, p[1]) for p in puts]
        ix.drop_tail()
        assert ix.tail is None and ix.entries == 0 and ix.tail_stats()[5] == 0
        assert ix.get([puts[3][0]]) == [(M.NOTFOUND, b"")]
        assert ix.refresh(tail=True) == 35 and ix.tail_stats()[4] == 35
        assert ix.get([p[0] for p in puts]) == [(0, p[1]) for p in puts]
    finally:
        ix.close()
        w.free()


# ------------------------------------------------------------- 4. the close
def test_the_close_keeps_every_row_in_its_place(gpu, runs):
    r = runs(1)
    prev = None
    closes = 0
    for step, s in enumerate(r.steps, 1):
        if prev is not None:
            # rows only ever come in behind the rows held: tail growth, the close, the next file's tail
            n = prev["got"]["entries"]
            assert s["got"]["hash"][:n] == prev["got"]["hash"] and s["got"]["loc"][:n] == prev["got"]["loc"], step
            if prev["tail"] and prev["tail"]["fileid"] in [int(f, 16) for f in s["names"]]:
                closes += 1                                   # the file that was the tail has closed
                assert s["tail"] is None or s["tail"]["fileid"] > prev["tail"]["fileid"]
                assert s["got"] == s["want"]
        prev = s
    assert closes >= 4


# ------------------------------------------------------------- 5. snapshots stand still
def test_snapshots_stand_still(gpu, orc):
    from kingdb_amd.index import HSTableIndex, NOTFOUND
    A, C, T = b"key-in-a-closed-file", b"another", b"tail-only"
    old, new = b"o" * 100, b"n" * 77
    more = [[(b"m%d-%d" % (j, i), b"x" * (i + j)) for i in range(20)] for j in range(3)]
    batches = [[(A, old), (C, b"c" * 10)], [(T, b"t" * 50), (A, new)]] + more
    w = new_writer(1 << 20, 1, batches, closes=4)
    ix = HSTableIndex.from_resident(w)
    try:
        feed(w, batches[0], 1)
        w.close()
        feed(w, batches[1], 1)
        ix.refresh(tail=True)
        assert ix.entries == 4 and ix.tail["rows"] == 2
        assert ix.get([T, A]) == [(0, b"t" * 50), (0, new)]
        snap = ix.snapshot()

        def view():
            return {"entries": snap.entries, "get": snap.get([T, A, C] + [p[0] for b in more for p in b]),
                    "where": [int(x) for x in snap.locate([T, A, C])[0]], "items": list(snap.items()),
                    "names": list(snap.names)}
        first = view()
        assert first["entries"] == 2 and first["names"] == ["00000001"]
        assert first["get"][:3] == [(NOTFOUND, b""), (0, old), (0, b"c" * 10)]
        assert first["items"] == [(A, 0, old), (C, 0, b"c" * 10)]
        feed(w, more[0], 1)                                   # the tail grows
        ix.refresh(tail=True)
        assert ix.tail["rows"] == 22 and view() == first
        ix.drop_tail()
        assert view() == first
        ix.refresh(tail=True)
        w.close()                                             # the file closes and is refreshed
        ix.refresh(tail=True)
        assert ix.tail is None and ix.names == ["00000001", "00000002"] and view() == first
        for puts in more[1:]:                                 # two more files
            feed(w, puts, 1)
            ix.refresh(tail=True)
            assert view() == first
            w.close()
            ix.refresh()
            assert view() == first
        assert len(ix.names) == 4 and ix.entries == 2 + 2 + 60
        assert ix.get([T, A]) == [(0, b"t" * 50), (0, new)]
        later = ix.snapshot()
        assert later.entries == ix.entries and later.get([T, A]) == [(0, b"t" * 50), (0, new)]
        later.close()
        snap.close()
    finally:
        ix.close()
        w.free()


# ------------------------------------------------------------- 6. scan
def test_scan_and_compaction_over_a_tail(gpu, runs):
    from kingdb_amd.index import HSTableIndex
    r = runs(1)
    some_tail = 0
    for step, s in enumerate(r.steps, 1):
        assert s["items"] == s["want_items"], step
        assert s["sort"] == s["want_sort"], step
        some_tail += s["tail"] is not None and len(s["names"]) > 0
    assert some_tail >= 3
    # compaction over a handle with closed files and a tail: the files of the fresh index's
    step = next(i for i, s in enumerate(r.steps, 1) if s["tail"] and s["tail"]["rows"] > 5 and len(s["names"]) >= 2)
    w = new_writer(r.sb, 1, r.batches)
    ix = HSTableIndex.from_resident(w)
    fr = HSTableIndex(r.steps[step - 1]["files"], 1)
    outs = []
    try:
        for puts in r.batches[:step]:
            feed(w, puts, 1)
        ix.refresh(tail=True)
        assert ix.tail == r.steps[step - 1]["tail"]
        for x in (ix, fr):
            for make in (lambda y: y.compacted_device(64 << 10, 100), lambda y: y.compact_copy(64 << 10, 100)):
                o = make(x)
                outs.append(o)
        assert outs[0].files() == outs[2].files() and len(outs[0].files()) >= 1
        assert outs[1].files() == outs[3].files()
    finally:
        for o in outs:
            o.free()
        ix.close()
        fr.close()
        w.free()


# ------------------------------------------------------------- 7. refusals change nothing
def set_tail_rc(ix, rec, flags=0, d_files=None):
    from kingdb_amd import _lib
    f = _lib.OpenFile(**rec)
    gained = ctypes.c_uint64(99)
    rc = _lib.load().kdb_index_set_tail(ix.h, None, ix.files.ptr if d_files is None else d_files, ctypes.byref(f),
                                        flags, ctypes.byref(gained))
    return rc, gained.value


def test_refusals_change_nothing(gpu, orc):
    from kingdb_amd import _lib
    from kingdb_amd.index import TAIL_REPARSE, HSTableIndex
    puts = [[(b"first-%02d" % i, b"a" * (3 * i)) for i in range(25)],
            [(b"second-%02d" % i, b"b" * (200 + i)) for i in range(25)],
            [(b"third-%02d" % i, b"c" * (5 * i)) for i in range(25)]]
    keys = [p[0] for b in puts for p in b]
    q = queries(keys)
    w = new_writer(1 << 20, 1, puts, closes=2)
    ix = HSTableIndex.from_resident(w)
    try:
        feed(w, puts[0], 1)
        w.close()
        ix.refresh()
        feed(w, puts[1], 1)
        rec = open_record(w)
        assert rec["open"] == 1 and rec["fileid"] == 2 and rec["rows"] == 25 and rec["rows_last"] == w.arena - 1

        def refused(cases, label):
            before = (snapshot(ix, q), ix.tail_stats())
            for what, r, flags, d_files in cases:
                assert set_tail_rc(ix, r, flags, d_files) == (_lib.EINVAL, 0), (label, what)
                ix._sync_tail()
                assert (snapshot(ix, q), ix.tail_stats()) == before, (label, what)

        # no tail held: the whole staging is parsed
        refused([("another buffer", rec, 0, ix.files.ptr + 64),
                 ("the id of a loaded file", dict(rec, fileid=1, timestamp=1), 0, None),
                 ("an older timestamp", dict(rec, timestamp=0), 0, None),
                 ("a row too many for the bytes", dict(rec, rows=26), 0, None),
                 ("a row too few for the bytes", dict(rec, rows=24), 0, None),
                 ("bytes cut inside the last row", dict(rec, row_bytes=rec["row_bytes"] - 1), 0, None),
                 ("more than 2^30 rows", dict(rec, rows=(1 << 30) + 1), 0, None),
                 ("a staging larger than what lies before its end", dict(rec, rows_last=rec["row_bytes"] - 2), 0, None),
                 ("a flag that does not exist", rec, 2, None)], "no tail")
        assert ix.tail is None and ix.entries == 25
        # a tail held: its growth is parsed alone, or everything with the flag
        assert ix.refresh(tail=True) == 25
        feed(w, puts[2], 1)
        grown = open_record(w)
        assert grown["rows"] == 50 and grown["fileid"] == 2
        for flags in (0, TAIL_REPARSE):
            refused([("fewer rows than held", dict(grown, rows=24), flags, None),
                     ("fewer bytes than held", dict(grown, row_bytes=rec["row_bytes"] - 1), flags, None),
                     ("a smaller file than held", dict(grown, bytes=rec["bytes"] - 1), flags, None),
                     ("a row too many for the bytes", dict(grown, rows=51), flags, None),
                     ("a row too few for the bytes", dict(grown, rows=49), flags, None),
                     ("bytes cut inside the last row", dict(grown, row_bytes=grown["row_bytes"] - 1), flags, None),
                     ("another buffer", grown, flags, ix.files.ptr + 64),
                     ("another file with the id of a loaded one", dict(grown, fileid=1, timestamp=1), flags, None),
                     ("more than 2^30 rows", dict(grown, rows=(1 << 30) + 1), flags, None)], "tail held, flags %d" % flags)
        assert ix.tail == tail_of(rec) and ix.entries == 50
        # the index is usable: the tail grows
        assert ix.refresh(tail=True) == 25 and ix.tail == tail_of(grown)
        files = closed_form_two(1 << 20, puts)
        fr = HSTableIndex(files, 1)
        try:
            assert snapshot(ix, q) == snapshot(fr, q)
            assert ix.get(keys) == [(0, p[1]) for b in puts for p in b]
        finally:
            fr.close()
    finally:
        ix.close()
        w.free()


# ------------------------------------------------------------- 8. an incomplete file
def test_incomplete_open_file(gpu, orc):
    """70 000 incompressible bytes in parts of 65 536 and 4 464: an entry the
    writer marks unfinished (tests/test_gpu_compact.py has why), so its file
    closes without an offset array and loads with status -1."""
    from kingdb_amd.index import HSTableIndex, NOTFOUND
    noise = np.random.default_rng(13).integers(0, 256, 70000, dtype=np.uint8).tobytes()
    batches = [[(b"before-%d" % i, b"v" * (30 + i), None) for i in range(10)],
               [(b"in-the-file-1", b"w" * 20, None)],
               [(b"incompressible", noise, [65536, 4464]), (b"behind-it", b"x" * 30, None)],
               [(b"later", b"y" * 40, None)],
               [(b"incompressible", b"z" * 500, None), (b"in-the-file-1", b"w" * 21, None)]]
    keys = [p[0] for b in batches for p in b]
    q = queries(sorted(set(keys)))
    sb = 1 << 20
    w = new_writer(sb, 1, batches, closes=3)
    ix = HSTableIndex.from_resident(w)

    def fresh(closes):
        """The files of a writer fed the same batches, closed after the batches in `closes`."""
        w2 = new_writer(sb, 1, batches, closes=3)
        try:
            for i in range(max(closes) + 1):
                feed(w2, batches[i], 1)
                if i in closes:
                    w2.close()
            return w2.files()
        finally:
            w2.free()

    def same_as(files, status):
        m = M.Model(files, orc, 1)
        assert m.file_status == status
        fr = HSTableIndex(files, 1)
        try:
            snap = snapshot(ix, q)
            assert snap == snapshot(fr, q)
            assert_model(snap, m, q)
            assert list(ix.items()) == list(fr.items())
        finally:
            fr.close()
    try:
        feed(w, batches[0], 1)
        w.close()
        feed(w, batches[1], 1)
        assert ix.refresh(tail=True) == 11 and ix.tail == {"fileid": 2, "rows": 1, "bytes": w.open_bytes()}
        feed(w, batches[2], 1)                                # file 2 turns incomplete while it is the tail
        rec = open_record(w)
        assert rec["incomplete"] == 1 and rec["fileid"] == 2
        assert ix.refresh(tail=True) == -1                    # the row it held is gone with the offset array
        assert ix.tail is None and ix.tail_stats()[:5] == (0, 0, 0, 0, 0) and ix.entries == 10
        same_as(fresh({0, 2}), {"00000001": 0, "00000002": -1})
        assert ix.get([b"in-the-file-1", b"behind-it"]) == [(NOTFOUND, b""), (NOTFOUND, b"")]
        feed(w, batches[3], 1)                                # more entries into the incomplete file
        assert ix.refresh(tail=True) == 0 and ix.tail is None
        same_as(fresh({0, 3}), {"00000001": 0, "00000002": -1})
        w.close()
        assert ix.refresh(tail=True) == 0 and ix.names == ["00000001", "00000002"]
        assert ix.file_status == {"00000001": 0, "00000002": -1} and ix.tail is None
        feed(w, batches[4], 1)                                # the value arrives whole in a later file
        assert ix.refresh(tail=True) == 2 and ix.tail["fileid"] == 3
        same_as(fresh({0, 3, 4}), {"00000001": 0, "00000002": -1, "00000003": 0})
        assert ix.get([b"incompressible", b"in-the-file-1"]) == [(0, b"z" * 500), (0, b"w" * 21)]
    finally:
        ix.close()
        w.free()


# ------------------------------------------------------------- 9. unchanged without a tail
def test_no_tail_without_asking(gpu, runs):
    from kingdb_amd.index import HSTableIndex
    r = runs(1)
    w = new_writer(r.sb, 1, r.batches)
    ix = HSTableIndex.from_resident(w)
    try:
        for step, puts in enumerate(r.batches, 1):
            feed(w, puts, 1)
            ix.refresh()
            assert ix.tail is None and ix.tail_stats()[:4] == (0, 0, 0, 0)
            s = r.steps[step - 1]
            assert ix.names == s["closed"]
            # the rows of the closed files, as the index with a tail numbers them too
            n = ix.entries
            h, loc = ix.pairs()
            assert [int(x) for x in h] == s["got"]["hash"][:n] and [int(x) for x in loc] == s["got"]["loc"][:n]
            assert n == s["got"]["entries"] - (s["tail"]["rows"] if s["tail"] else 0)
    finally:
        ix.close()
        w.free()


# ------------------------------------------------------------- 10. an add while a tail is held
CLOSED = [(b"closed-%02d" % i, b"c" * (10 + i)) for i in range(25)]
TAIL = [(b"tail-%02d" % i, b"t" * (40 + i)) for i in range(30)]
OTHER = [(b"other-%02d" % i, b"o" * (5 + 2 * i)) for i in range(20)]
ADDED = [(b"added-%02d" % i, b"a" * (70 + i)) for i in range(20)] + [(CLOSED[3][0], b"again")]


@pytest.fixture(scope="module")
def later(gpu):
    """Files 1..4 of a writer fed CLOSED, TAIL, OTHER and ADDED with a close
    after each (a file's timestamp is its id): file 1 and file 2 are, byte for
    byte, what the writers of the tests below hold closed and open."""
    batches = [CLOSED, TAIL, OTHER, ADDED]
    w = new_writer(1 << 20, 1, batches, closes=4)
    try:
        for puts in batches:
            feed(w, puts, 1)
            w.close()
        return w.files()
    finally:
        w.free()


def tail_held(extra):
    """(writer, index): CLOSED in the closed file 1, TAIL in the open file 2,
    held as the tail; `extra` bytes of the arena beyond what the writer needs."""
    from kingdb_amd import put
    from kingdb_amd.index import HSTableIndex
    w = put.DeviceHSTableWriter(1 << 20, 1, put.DeviceHSTableWriter.arena_bytes(
        1 << 20, put.entries_bound(CLOSED) + put.entries_bound(TAIL), 55) + extra)
    try:
        ix = HSTableIndex.from_resident(w)
        feed(w, CLOSED, 1)
        w.close()
        feed(w, TAIL, 1)
        assert ix.refresh(tail=True) == 55 and ix.tail["rows"] == 30 and ix.tail_stats()[5] == buckets(55)
        assert ix.get([TAIL[7][0], CLOSED[7][0]]) == [(0, TAIL[7][1]), (0, CLOSED[7][1])]
        return w, ix
    except BaseException:
        w.free()
        raise


def place_in_arena(w, ix, files):
    """Uploads `files` into the writer's arena, which the index borrows, between
    the open file's end and the rows staged backwards from the arena's end (the
    writer is not fed again): (file_off, file_size, fileid) for kdb_index_add_files."""
    from kingdb_amd import _lib
    rec = open_record(w)
    at = (rec["file_off"] + rec["bytes"] + 4096 + 63) & ~63
    off = []
    for f in files:
        off.append(at)
        at = (at + len(files[f]) + 63) & ~63
    assert at + 4096 <= rec["rows_last"] + 1 - rec["row_bytes"], "the arena has no room for the files"
    for f, o in zip(files, off):
        b = np.frombuffer(files[f], np.uint8)
        _lib.check(_lib.load().kdb_lz4_memcpy_h2d(ix.files.ptr + o, b.ctypes.data, b.nbytes, None), "h2d")
    _lib.check(_lib.load().kdb_lz4_stream_sync(None), "sync")
    return (np.array(off, np.uint64), np.array([len(files[f]) for f in files], np.uint64),
            np.array([int(f, 16) for f in files], np.uint32))


def test_add_without_rows_drops_a_tail_with_rows(gpu, orc, later):
    """One file with a broken footer CRC (-1) added while a tail of 30 rows is
    held: no row comes in, and the tail's rows leave the buckets with it."""
    from kingdb_amd.index import HSTableIndex, NOTFOUND
    b = bytearray(later["00000003"])
    b[M.footer(later["00000003"])[2] + 3] ^= 0x10            # a byte of the offset array: the footer's CRC is off
    bad = {"00000003": bytes(b)}
    assert M.Model(bad, orc, 1).file_status == {"00000003": -1}
    q = queries([p[0] for p in CLOSED + TAIL + OTHER])
    w, ix = tail_held(len(bad["00000003"]) + (64 << 10))
    try:
        off, size, fid = place_in_arena(w, ix, bad)
        assert ix._add(None, off, size, fid) == {"00000003": -1}         # _add raises unless the call returns KDB_PUT_OK
        assert ix.add_stats() == (0, buckets(25), 0)
        assert ix.tail is None and ix.entries == 25
        ix._sync_tail()                                       # the handle's own counts
        assert ix.tail is None and ix.entries == 25
        assert ix.tail_stats() == (0, 0, 0, 0, 30, buckets(25))          # [4]: the last set_tail's, as it was
        assert ix.get([p[0] for p in TAIL]) == [(NOTFOUND, b"")] * 30
        assert ix.get([p[0] for p in CLOSED]) == [(0, p[1]) for p in CLOSED]
        fr = HSTableIndex({"00000001": later["00000001"]}, 1)
        try:
            assert snapshot(ix, q) == snapshot(fr, q)
            assert list(ix.items()) == list(fr.items())
        finally:
            fr.close()
        # the tail again: every row of it is parsed
        assert ix.refresh(tail=True) == 30 and ix.tail_stats() == (1, 2, 30, w.open_bytes(), 30, buckets(55))
        fr = HSTableIndex({f: later[f] for f in ("00000001", "00000002")}, 1)
        try:
            assert snapshot(ix, q) == snapshot(fr, q)
            assert ix.get([p[0] for p in TAIL]) == [(0, p[1]) for p in TAIL]
        finally:
            fr.close()
    finally:
        ix.close()
        w.free()


def test_add_numbers_the_rows_again_with_a_tail_held(gpu, orc, later):
    """Two files added in one call while a tail of 30 rows is held: the first
    with a malformed offset array (-3, found by the parse, so the rows are
    numbered a second time beside the tail's), the second good."""
    from kingdb_amd.index import HSTableIndex
    hashes = [0, 5, 127, 128, 300, 16383, 1 << 56, (1 << 63) - 1, 1 << 63, (1 << 64) - 1, 1 << 62, 7]
    offsets = [5, 127, 128, 20000, 3000000, 0xFFFFFFF0, 0xFFFFFFFF, 0]
    rows = [(hashes[(i * 7 + i // 12) % len(hashes)], offsets[(i * 3 + i // 8) % len(offsets)]) for i in range(90)]
    g = M.with_rows(later["00000003"], rows, orc)
    assert M.parse_rows(g) == rows
    files = {"00000003": M.refooter(g, orc, num=len(rows) + 1),           # a row more than the array holds
             "00000004": later["00000004"]}
    want = {"00000001": later["00000001"], "00000004": later["00000004"]}
    assert M.Model(dict(files, **want), orc, 1).file_status == {"00000001": 0, "00000003": -3, "00000004": 0}
    q = queries([p[0] for p in CLOSED + TAIL + OTHER + ADDED])
    w, ix = tail_held(sum(len(f) for f in files.values()) + (64 << 10))
    try:
        off, size, fid = place_in_arena(w, ix, files)
        assert ix._add(None, off, size, fid) == {"00000003": -3, "00000004": 0}
        good = len(ADDED)
        # both passes count: the two files' rows, then the good file's alone
        assert ix.add_stats() == (0, buckets(25 + good), (len(rows) + 1 + good) + good)
        assert ix.tail is None and ix.entries == 25 + good
        ix._sync_tail()
        assert ix.tail is None and ix.entries == 25 + good and ix.tail_stats()[:4] == (0, 0, 0, 0)
        fr = HSTableIndex(want, 1)
        try:
            snap = snapshot(ix, q)
            assert snap == snapshot(fr, q)
            assert_model(snap, M.Model(want, orc, 1), q)
            assert list(ix.items()) == list(fr.items())
        finally:
            fr.close()
        assert ix.get([ADDED[0][0], CLOSED[3][0], CLOSED[4][0]]) == [(0, ADDED[0][1]), (0, b"again"), (0, CLOSED[4][1])]
    finally:
        ix.close()
        w.free()
