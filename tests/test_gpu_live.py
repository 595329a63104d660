"""GPU: snapshots, compaction and the hand-over over the writer's open file
(include/kdb_live.h; HSTableIndex.snapshot(tail=True), compact_copy(
closed_only=True), compact(carry_open=True), DeviceHSTableWriter.adopt_open).

The contracts under test, every comparison exact:

  * a tail snapshot answers -- entries, locate, Get, the whole scan, live,
    key bytes, longest key, whether a sort ran -- as an HSTableIndex made fresh
    over the files of a twin writer that was fed the same puts and then
    closed, and goes on answering so while the tail grows, is parsed again,
    the file closes and is added, further files come, the next file becomes
    the tail and the bucket count doubles (tests/test_live_model.py pins that
    expectation to the model of the rows below R);
  * while such a snapshot is open on a file not yet added closed, the handle
    keeps that file as its tail;
  * closed_live counts the live entries below the tail, the first of the list;
  * a file carried by adopt_open closes byte for byte as in an untouched twin;
  * compact(carry_open=True) answers as the index it was called on.

Writers use hstable_size 64 KiB and batches of 37 puts, so files close in the
middle of the put streams of tests/golden (get_keys, deletes, key_lengths).
"""
import struct

import numpy as np
import pytest

import deletes_fixture as D
import index_model as M
import keylens
import scan_model as S
from conftest import load_golden

pytestmark = pytest.mark.gpu

HS = 64 << 10
BATCH = 37
HEADER = 8192
BIG = 1 << 31                            # the largest multipart_required a lookup takes


def sync():
    from kingdb_amd import _lib
    _lib.check(_lib.load().kdb_lz4_stream_sync(None), "sync")


def feed(w, puts, ht):
    from kingdb_amd import put
    b, n = put.put_entries_device(puts, ht)
    try:
        w.append_batch(b, n)
        sync()
    finally:
        b.free()


def new_writer(ht, batches, extra=0, hs=HS):
    from kingdb_amd import put
    n = sum(len(b) for b in batches)
    return put.DeviceHSTableWriter(hs, ht, put.DeviceHSTableWriter.arena_bytes(
        hs, sum(put.entries_bound(b) for b in batches), max(n, 1)) + 16 * (HEADER + 36 + 128) + extra)


def closed_form(ht, batches, closes=(), hs=HS):
    """The files of a twin writer fed `batches`, closed after the batches whose index is in `closes`, and at the end."""
    w = new_writer(ht, batches, hs=hs)
    try:
        for i, puts in enumerate(batches):
            feed(w, puts, ht)
            if i in closes:
                w.close()
        w.close()
        return w.files()
    finally:
        w.free()


def flipped(k, at, x=0x40):
    b = bytearray(k)
    b[at] ^= x
    return bytes(b)


def queries(keys):
    """Every key and its near-misses: a byte flipped, one byte shorter, one longer, the empty key."""
    keys = sorted(set(keys))
    return keys + [flipped(k, len(k) // 2) for k in keys] + [k[:-1] for k in keys] + [k + b"\0" for k in keys] + [b""]


def view(x, q):
    """What an index or a snapshot shows: entries, locate of q, and the scan prepared again."""
    where, st = x.locate(q)
    live = x.scan_prepare()
    return {"entries": x.entries, "where": [int(v) for v in where], "status": [int(v) for v in st],
            "prepared": (live,) + tuple(x._scan[2:]), "sorted": x.scan_sort_steps() > 0,
            "scan": x.scan(multipart_required=BIG)}


def fresh_view(files, ht, q, with_get=False):
    from kingdb_amd.index import HSTableIndex
    fr = HSTableIndex(files, ht)
    try:
        v = view(fr, q)
        if with_get:
            v["get"] = fr.get(q)
        return v
    finally:
        fr.close()


def stream_items(name):
    """(items, hash_type) of a put stream of tests/golden."""
    from make_golden_put import decode_stream
    if name.startswith("deletes_"):
        s = D.load()[0][name[len("deletes_"):]]
        return s["items"], s["hash_type"]
    if name.startswith("key_lengths_"):
        s = keylens.load()[name[len("key_lengths_"):]]
        return s["puts"], s["hash_type"]
    z = load_golden("get_keys.npz")
    n = name[len("get_keys_"):]
    return decode_stream(z[f"{n}__stream"].tobytes()), int(z[f"{n}__opts"][1])


def batches_of(items, n=BATCH):
    return [items[i:i + n] for i in range(0, len(items), n)]


def closed_ids(ix):
    return {int(f, 16) for f in ix.names}


# ------------------------------------------------------------- 1. the contract, at every step
@pytest.mark.parametrize("stream", ["get_keys_xx", "deletes_mixed", "key_lengths_xx", "key_lengths_murmur"])
def test_tail_snapshot_contract_at_every_step(gpu, orc, stream):
    from kingdb_amd.index import HSTableIndex
    items, ht = stream_items(stream)
    items = items[:400]
    batches = batches_of(items)
    q = queries([it[0] for it in items])
    w = new_writer(ht, batches)
    ix = HSTableIndex.from_resident(w)
    kept = []                            # [snapshot, what it must answer], open across everything that follows
    keep_at = {1, 2, 4}
    seen = {"grew": 0, "closed": 0, "later files": 0, "doubled": 0, "reparsed": 0, "mid file": 0, "unpinned": 0}
    try:
        for step, puts in enumerate(batches, 1):
            feed(w, puts, ht)
            nb_before = ix.tail_stats()[5]
            ix.refresh(tail=True, reparse=step % 3 == 0)
            seen["reparsed"] += step % 3 == 0 and ix.tail is not None and bool(kept)
            seen["doubled"] += bool(kept) and ix.tail_stats()[5] > nb_before > 0
            snap = ix.snapshot(tail=True)
            want = fresh_view(closed_form(ht, batches[:step]), ht, q)
            assert snap.tail == ({"fileid": ix.tail["fileid"], "rows": ix.tail["rows"]} if ix.tail else None)
            assert snap.entries == ix.entries == sum(len(b) for b in batches[:step]) and snap.names == ix.names
            assert view(snap, q) == want, step
            assert view(ix, q) == want, step
            seen["mid file"] += snap.tail is not None and len(ix.names) > 0
            # the snapshots kept: the same answers after whatever this step did to the handle
            for k, kwant, kstate in kept:
                inc, fid, rows, pinned = k.tail_stats()
                assert (inc, fid, rows) == (1, k.tail["fileid"], k.tail["rows"])
                assert pinned == (0 if fid in closed_ids(ix) else 1), step        # 1 -> 0 at the add of its file
                seen["unpinned"] += kstate["pinned"] == 1 and pinned == 0
                seen["closed"] += kstate["pinned"] == 1 and pinned == 0
                seen["grew"] += pinned == 1 and ix.tail is not None and ix.tail["rows"] > kstate["tail rows"]
                seen["later files"] += pinned == 0 and len(ix.names) > kstate["names"] and kstate["pinned"] == 0
                kstate.update({"pinned": pinned, "tail rows": ix.tail["rows"] if ix.tail else 0, "names": len(ix.names)})
                assert view(k, q) == kwant, (step, rows)
            if step in keep_at and snap.tail is not None:
                kept.append((snap, want, {"pinned": 1, "tail rows": snap.tail["rows"], "names": len(ix.names)}))
            else:
                snap.close()
        assert len(kept) == 3
        assert ix.tail_stats()[5] >= 512
        for what in ("grew", "closed", "doubled", "reparsed", "mid file", "unpinned"):
            assert seen[what] >= 1, (what, seen)
        if len(items) >= 300:                                # the streams long enough for files behind a kept snapshot's own
            assert len(ix.names) + (ix.tail is not None) >= 3 and seen["later files"] >= 2, seen
    finally:
        ix.close()                       # closes the snapshots still open
        w.free()


# ------------------------------------------------------------- 2. the boundary inside the file
def test_the_boundary_inside_the_open_file(gpu, orc):
    from kingdb_amd import _lib, put
    from kingdb_amd.index import DELETED, NOTFOUND, HSTableIndex, HSTableSnapshot
    A, B, C, Dk, E, F = (b"key-" + c * 9 for c in (b"a", b"b", b"c", b"d", b"e", b"f"))
    v = {n: bytes([65 + n]) * (40 + n) for n in range(12)}
    b0 = [(A, v[0]), (B, v[1]), (C, v[2]), (Dk, v[3])]                            # file 1, closed
    b1 = [(A, v[4]), (E, v[5]), (B, put.DELETE)]                                 # file 2: ..., a delete just below R
    b2 = [(C, put.DELETE), (A, v[6]), (B, v[7]), (F, v[8])]                      # a delete just above R, A again
    b3 = [(A, v[9])]
    batches = [b0, b1, b2, b3]
    keys = [A, B, C, Dk, E, F]
    q = queries(keys)
    w = new_writer(1, batches, hs=1 << 20)
    ix = HSTableIndex.from_resident(w)
    try:
        # no file open: a tail snapshot is a plain one
        feed(w, b0, 1)
        w.close()
        with ix.snapshot(tail=True) as s0, ix.snapshot() as p0:
            assert s0.tail is None and s0.tail_stats() == (0, 0, 0, 0) and s0.entries == p0.entries == 4
            assert view(s0, q) == view(p0, q) and s0.closed_live() == p0.closed_live() == 4
            ix.drop_tail()                                   # nothing is pinned
        # a tail of 0 rows: the file as it is the moment it opens, its header block alone
        feed(w, b1[:1], 1)
        rec = w.open_file()
        assert rec.rows == 1 and rec.fileid == 2
        empty = _lib.OpenFile(open=1, fileid=2, timestamp=rec.timestamp, file_off=rec.file_off, bytes=HEADER, rows=0,
                              row_bytes=0, rows_last=rec.rows_last)
        assert ix.set_tail(empty) == 0 and ix.tail == {"fileid": 2, "rows": 0, "bytes": HEADER}
        z = HSTableSnapshot(ix, True)
        assert z.tail == {"fileid": 2, "rows": 0} and z.tail_stats() == (1, 2, 0, 1) and z.entries == 4
        zwant = fresh_view(closed_form(1, [b0]), 1, q)
        assert view(z, q) == zwant and z.closed_live() == 4
        # a tail of exactly 1 row
        one = ix.snapshot(tail=True)
        assert one.tail == {"fileid": 2, "rows": 1} and one.entries == 5
        want1 = fresh_view(closed_form(1, [b0, b1[:1]], {0}), 1, q, with_get=True)
        assert view(one, q) == {k: want1[k] for k in want1 if k != "get"}
        assert one.get(keys) == [(0, v[4]), (0, v[1]), (0, v[2]), (0, v[3]), (NOTFOUND, b""), (NOTFOUND, b"")]
        assert one.closed_live() == 3                        # B, C, D of file 1; A lives in the open file
        # R behind b1: A on both sides of it, a delete just below and one just above
        feed(w, b1[1:], 1)
        s1 = ix.snapshot(tail=True)
        assert s1.tail == {"fileid": 2, "rows": 3} and s1.entries == 7
        feed(w, b2, 1)
        s2 = ix.snapshot(tail=True)
        feed(w, b3, 1)
        ix.refresh(tail=True)
        want = {"s1": [(0, v[4]), (DELETED, b""), (0, v[2]), (0, v[3]), (0, v[5]), (NOTFOUND, b"")],
                "s2": [(0, v[6]), (0, v[7]), (DELETED, b""), (0, v[3]), (0, v[5]), (0, v[8])],
                "ix": [(0, v[9]), (0, v[7]), (DELETED, b""), (0, v[3]), (0, v[5]), (0, v[8])]}
        full = {"s1": fresh_view(closed_form(1, [b0, b1], {0}), 1, q), "s2": fresh_view(closed_form(1, [b0, b1, b2], {0}), 1, q)}

        def check():
            assert s1.get(keys) == want["s1"] and s2.get(keys) == want["s2"] and ix.get(keys) == want["ix"]
            assert view(s1, q) == full["s1"] and view(s2, q) == full["s2"]
            assert view(z, q) == zwant and one.get(keys)[0] == (0, v[4])
            assert s1.closed_live() == 2 and s2.closed_live() == 1               # C, D; then D alone
            assert [k for k, _, _ in s1.scan()] == [C, Dk, A, E] and [k for k, _, _ in s2.scan()] == [Dk, E, A, B, F]
        check()
        assert [s.tail_stats()[3] for s in (z, one, s1, s2)] == [1, 1, 1, 1]
        w.close()
        ix.refresh(tail=True)
        assert ix.names == ["00000001", "00000002"] and ix.tail is None
        assert [s.tail_stats()[3] for s in (z, one, s1, s2)] == [0, 0, 0, 0]
        check()
        ix.drop_tail()                                       # nothing is pinned any more
    finally:
        ix.close()
        w.free()


# ------------------------------------------------------------- 3. the pin
class Mirror:
    """A buffer the test owns, holding a copy of a writer's arena and what the
    writer reported of it then: HSTableIndex.from_resident() and refresh() read
    it as they read a writer."""

    def __init__(self, arena, ht):
        from kingdb_amd.lz4 import DeviceBuffer
        self.buf = DeviceBuffer(arena)
        self.arena, self.hash_type = arena, ht
        self.off = self.size = np.zeros(0, np.uint64)
        self.fid = np.zeros(0, np.uint32)
        self.open = None

    def sync_from(self, w):
        from kingdb_amd import _lib
        ptr, off, size, fid = w.resident()
        self.open = w.open_file()                            # waits for the writer's queued work
        assert w.arena == self.arena
        _lib.check(_lib.load().kdb_lz4_memcpy_d2d(self.buf.ptr, ptr, self.arena, None), "d2d")
        sync()
        self.off, self.size, self.fid = off.copy(), size.copy(), fid.copy()

    def resident(self):
        return self.buf.ptr, self.off.copy(), self.size.copy(), self.fid.copy()

    def open_file(self):
        return self.open

    def open_bytes(self):
        return int(self.open.bytes) if self.open is not None else 0

    def free(self):
        self.buf.free()


def test_the_pin(gpu, orc):
    from kingdb_amd import _lib
    from kingdb_amd.index import HSTableIndex
    puts = [[(b"first-%02d" % i, b"a" * (3 * i + 1)) for i in range(25)],
            [(b"second-%02d" % i, b"b" * (200 + i)) for i in range(25)],
            [(b"third-%02d" % i, b"c" * (5 * i + 1)) for i in range(25)],
            [(b"fourth-%02d" % i, b"d" * (7 * i + 1)) for i in range(25)]]
    keys = [p[0] for b in puts for p in b]
    q = queries(keys)
    w = new_writer(1, puts, hs=1 << 20)
    ix = HSTableIndex.from_resident(w)
    plain = snap = None
    try:
        feed(w, puts[0], 1)
        w.close()
        feed(w, puts[1], 1)
        snap = ix.snapshot(tail=True)
        plain = ix.snapshot()                                # pins nothing, sees no tail
        assert snap.tail == {"fileid": 2, "rows": 25} and plain.tail is None and plain.entries == 25
        feed(w, puts[2], 1)
        ix.refresh(tail=True)                                # growth is allowed
        ix.refresh(tail=True, reparse=True)                  # and so is a reparse
        rec = w.open_file()
        assert ix.tail["rows"] == 50

        def state():
            return view(ix, q), ix.tail, ix.tail_stats()[:4], view(snap, q), snap.tail_stats(), view(plain, q)
        before = state()
        none = _lib.OpenFile()
        fields = {n: int(getattr(rec, n)) for n, _ in rec._fields_}
        incomplete = _lib.OpenFile(**dict(fields, incomplete=1))
        other = _lib.OpenFile(**dict(fields, fileid=3, timestamp=3))
        calls = {"drop_tail": lambda: ix.drop_tail(), "set_tail to none": lambda: ix.set_tail(none),
                 "set_tail to an incomplete file": lambda: ix.set_tail(incomplete),
                 "set_tail to another file": lambda: ix.set_tail(other)}
        for what, call in calls.items():
            with pytest.raises(_lib.HipError, match="EINVAL"):
                call()
            ix._sync_tail()
            assert state() == before, what
        # the snapshot closed: each of the calls succeeds
        snap.close()
        ix.set_tail(other)                                   # file 3's id over file 2's bytes: another file all the same
        assert ix.tail["fileid"] == 3
        ix.set_tail(incomplete)
        assert ix.tail is None
        ix.set_tail(rec)
        ix.set_tail(none)
        assert ix.tail is None
        ix.set_tail(rec)
        ix.drop_tail()
        assert ix.tail is None and ix.entries == 25
        # an add that leaves the tail's file out: files 2 and 3 close, file 3 is given alone
        snap = ix.snapshot(tail=True)
        assert snap.tail_stats() == (1, 2, 50, 1)
        before = state()
        w.close()
        feed(w, puts[3], 1)
        w.close()
        ptr, off, size, fid = w.resident()
        assert [int(f) for f in fid] == [1, 2, 3]
        with pytest.raises(_lib.HipError, match="EINVAL"):
            ix._add(None, off[2:], size[2:], fid[2:])
        assert state() == before and ix.names == ["00000001"]
        assert snap.tail_stats() == (1, 2, 50, 1)
        snap.close()
        ix._add(None, off[2:], size[2:], fid[2:])            # file 2 left out for good
        assert ix.names == ["00000001", "00000003"] and ix.entries == 50 and ix.tail is None
        assert view(plain, q) == before[5]
    finally:
        ix.close()
        w.free()


def test_the_add_is_refused_when_the_pinned_rows_differ(gpu, orc):
    from kingdb_amd import _lib
    from kingdb_amd.index import HSTableIndex
    b0 = [(b"zero-%02d" % i, b"z" * (10 + i)) for i in range(20)]
    b1 = [(b"open-%02d" % i, b"o" * (30 + i)) for i in range(20)]
    b1x = list(b1)
    b1x[7] = (b"OPEN-07", b1[7][1])                          # one other put, the same lengths
    b2 = [(b"more-%02d" % i, b"m" * i) for i in range(1, 9)]
    keys = [p[0] for p in b0 + b1 + b1x + b2]
    q = queries(keys)
    real, fake = new_writer(1, [b0, b1, b2], hs=1 << 20), new_writer(1, [b0, b1, b2], hs=1 << 20)
    mirror = Mirror(real.arena, 1)
    ix = None
    try:
        for wr, second in ((real, b1), (fake, b1x)):
            feed(wr, b0, 1)
            wr.close()
            feed(wr, second, 1)
        mirror.sync_from(real)
        ix = HSTableIndex.from_resident(mirror)
        snap = ix.snapshot(tail=True)
        assert snap.tail == {"fileid": 2, "rows": 20} and snap.tail_stats()[3] == 1
        want = view(snap, q)
        assert want == fresh_view(closed_form(1, [b0, b1], {0}, hs=1 << 20), 1, q)
        # the other writer's file 2: the same id, timestamp and place, row 7 another hash
        for wr in (real, fake):
            feed(wr, b2, 1)
            wr.close()
        assert fake.open_file() is None and list(fake.resident()[1]) == list(real.resident()[1])
        assert list(fake.resident()[3]) == list(real.resident()[3]) == [1, 2]
        mirror.sync_from(fake)
        with pytest.raises(_lib.HipError, match="EINVAL"):
            ix.refresh()
        assert ix.names == ["00000001"] and ix.tail == {"fileid": 2, "rows": 20, "bytes": ix.tail["bytes"]}
        assert snap.tail_stats() == (1, 2, 20, 1) and ix.entries == 40 and snap.entries == 40
        # the file the rows came from: accepted, and the snapshot is an ordinary one
        mirror.sync_from(real)
        assert ix.refresh() == 8
        assert ix.names == ["00000001", "00000002"] and snap.tail_stats() == (1, 2, 20, 0)
        assert view(snap, q) == want
        assert view(ix, q) == fresh_view(real.files(), 1, q)
    finally:
        if ix is not None:
            ix.close()
        mirror.free()
        real.free()
        fake.free()


# ------------------------------------------------------------- 4. closed_live
def entries_of(files):
    """[(key, stored value bytes)] of every entry of `files`, file by file in name order."""
    from kingdb_amd import get as G
    out = []
    for name in sorted(files):
        f = files[name]
        out += [(e.key, f[e.value_at:e.value_at + e.stored_len]) for e in G.read_hstable(f)]
    return out


def model_closed_live(files, tail_name, orc, ht):
    rows = S.live_rows(M.Model(files, orc, ht))
    return rows, sum(1 for _, _, name, _ in rows if name != tail_name)


@pytest.mark.parametrize("shuffled", [False, True], ids=["plain path", "sorted cold path"])
def test_closed_live(gpu, orc, shuffled):
    from kingdb_amd import put
    from kingdb_amd.index import HSTableIndex
    items, ht = stream_items("deletes_mixed")
    items = items[:200]
    hot = sorted({it[0] for it in items})[:30]
    late = [(k, b"overwritten in the open file " + k) for k in hot[:15]] + [(k, put.DELETE) for k in hot[15:25]] + \
        [(b"tail-only-%d" % i, b"t" * (20 + i)) for i in range(10)]
    batches = batches_of(items) + [late]
    w = new_writer(ht, batches)
    mirror = Mirror(w.arena, ht)
    ix = out = None
    try:
        for puts in batches[:-1]:
            feed(w, puts, ht)
        if w.open_file() is not None:
            w.close()
        nclosed = len(w.resident()[3])
        assert nclosed >= 2
        feed(w, late, ht)
        rec = w.open_file()
        assert rec is not None and rec.rows == len(late)
        mirror.sync_from(w)
        files = w.files()
        if shuffled:
            # the first file's rows in another order: the scan's list needs its sort
            name = sorted(files)[0]
            rows = M.parse_rows(files[name])
            perm = np.random.default_rng(5).permutation(len(rows))
            files[name] = M.with_rows(files[name], [rows[i] for i in perm], orc)
            assert len(files[name]) == int(mirror.size[0])
            mirror.buf.upload(np.frombuffer(files[name], np.uint8), int(mirror.off[0]))
        ix = HSTableIndex.from_resident(mirror)
        snap = ix.snapshot(tail=True)
        plain = ix.snapshot()
        assert snap.tail == {"fileid": rec.fileid, "rows": len(late)}
        # the model over the closed files and the open file closed as it is
        w.close()
        tail_name = "%08x" % rec.fileid
        files[tail_name] = w.files()[tail_name]
        rows, want_closed = model_closed_live(files, tail_name, orc, ht)
        live = snap.scan_prepare()
        assert (snap.scan_sort_steps() > 0) == shuffled
        assert live == len(rows) and snap.closed_live() == want_closed and 0 < want_closed < live
        got = snap.scan(multipart_required=BIG)
        assert [k for k, _, _ in got] == [k for _, _, _, k in rows]
        assert all(name != tail_name for _, _, name, _ in rows[:want_closed])
        assert all(name == tail_name for _, _, name, _ in rows[want_closed:])
        closed_files = {f: files[f] for f in files if f != tail_name}
        prows, pclosed = model_closed_live(closed_files, tail_name, orc, ht)
        assert plain.scan_prepare() == len(prows) == pclosed == plain.closed_live()
        assert want_closed < pclosed                          # entries the open file overwrites or deletes
        # compact_copy(closed_only=True): exactly those entries, in that order, under the closed files' timestamp
        out = snap.compact_copy(HS, 50, closed_only=True)
        comp = out.files()
        model = M.Model(files, orc, ht)
        want_entries = []
        for _, off, name, key in rows[:want_closed]:
            rc, e = M.locate_entry(files[name], off, False, orc)
            at = off + e["size_header"] + e["size_key"]
            want_entries.append((key, files[name][at:at + (e["svc"] or e["size_value"])]))
        assert entries_of(comp) == want_entries
        ts = max(struct.unpack_from("<Q", closed_files[f], 16)[0] for f in closed_files)
        assert all(struct.unpack_from("<IQ", f, 12) == (2, ts) for f in comp.values())
        out.free()
        out = snap.compact_copy(HS, 50)                      # closed_only=False: the tail's entries and timestamp too
        comp = out.files()
        assert len(entries_of(comp)) == live
        assert all(struct.unpack_from("<IQ", f, 12) == (2, rec.timestamp) for f in comp.values()) and rec.timestamp > ts
        assert model.get(hot[0])[0] == 0
    finally:
        if out is not None:
            out.free()
        if ix is not None:
            ix.close()
        mirror.free()
        w.free()


# ------------------------------------------------------------- 5. adopt_open
def open_record(w):
    f = w.open_file()
    return None if f is None else {n: int(getattr(f, n)) for n, _ in f._fields_}


def writer_state(w):
    ptr, off, size, fid = w.resident()
    return ptr, list(off), list(size), list(fid), open_record(w), w.files()


def carried(rec):
    """What adopt_open keeps of an open_file() record: everything but where the file and its staging lie."""
    return {k: v for k, v in rec.items() if k not in ("file_off", "rows_last")}


@pytest.mark.parametrize("further", [0, 1, 5])
def test_adopt_open_byte_identity(gpu, orc, further):
    items, ht = stream_items("get_keys_xx")
    batches = batches_of(items[:400])
    head, rest = batches[:3], batches[3:3 + further]
    src, twin = new_writer(ht, batches), new_writer(ht, batches)
    dst = new_writer(ht, batches, extra=256 << 10)
    try:
        for wr in (src, twin, dst):
            for puts in head:
                feed(wr, puts, ht)
        rec = open_record(src)
        assert rec and rec["rows"] > 0 and rec == open_record(twin)
        dst.close()                                          # dst: some closed files of its own, none open
        own = writer_state(dst)
        src_before = writer_state(src)
        dst.adopt(100, None, [], [], [])
        dst.adopt_open(src)
        assert writer_state(src) == src_before               # src is never modified
        got = open_record(dst)
        assert carried(got) == carried(rec) and got["file_off"] % 64 == 0 and got["rows_last"] == dst.arena - 1
        assert got["file_off"] >= own[1][-1] + own[2][-1]
        assert list(dst.resident()[3]) == [100 + i for i in range(len(own[3]))]
        for puts in rest:
            feed(dst, puts, ht)
            feed(twin, puts, ht)
        dst.close()
        twin.close()
        a, b = dst.files(), twin.files()
        name = "%08x" % rec["fileid"]
        assert a[name] == b[name]
        # every file written after the move holds the same bytes; the ids go on above everything dst holds
        later_a = [a[f] for f in sorted(a) if int(f, 16) > 100 + len(own[3]) - 1]
        later_b = [b[f] for f in sorted(b) if int(f, 16) > rec["fileid"]]
        assert [f[HEADER:] for f in later_a] == [f[HEADER:] for f in later_b]
        assert [int(f, 16) for f in sorted(a) if int(f, 16) >= 100] == list(range(100, 100 + len(own[3]) + len(later_a)))
        if further == 5:
            assert later_a                                   # the carried file closed in an append, not in close()
    finally:
        for wr in (src, twin, dst):
            wr.free()


def test_adopt_open_file_that_closes_in_the_first_append(gpu, orc):
    rng = np.random.default_rng(3)
    from kingdb_amd import put
    fill = [(b"fill-%03d" % i, rng.integers(0, 256, 900, dtype=np.uint8).tobytes()) for i in range(70)]
    last = [(b"last-%d" % i, rng.integers(0, 256, 900, dtype=np.uint8).tobytes()) for i in range(12)]
    size = np.cumsum([int(x) for x in put.put_entries(fill, 1).entry_len]) + HEADER
    fill = fill[:int(np.searchsorted(size, HS - 200))]       # the most puts that leave the file open, nearly full
    assert 40 < len(fill) < 70
    src, twin, dst = (new_writer(1, [fill, last], extra=128 << 10) for _ in range(3))
    try:
        for wr in (src, twin):
            feed(wr, fill, 1)
        rec = open_record(src)
        assert rec and HS - 6 * 930 < rec["bytes"] < HS
        dst.adopt_open(src)
        feed(dst, last, 1)                                   # the file closes inside this append
        feed(twin, last, 1)
        assert "%08x" % rec["fileid"] in {"%08x" % int(f) for f in dst.resident()[3]}
        assert open_record(dst) is not None and carried(open_record(dst)) == carried(open_record(twin))
        dst.close()
        twin.close()
        assert dst.files() == twin.files()
    finally:
        for wr in (src, twin, dst):
            wr.free()


def test_adopt_open_incomplete_file(gpu, orc):
    """An entry the writer marks unfinished (tests/test_gpu_index_tail.py has
    the stream): the file is carried as bytes and state, and closes without
    an offset array, as in the twin."""
    noise = np.random.default_rng(13).integers(0, 256, 70000, dtype=np.uint8).tobytes()
    b0 = [(b"before-%d" % i, b"v" * (30 + i), None) for i in range(10)]
    b1 = [(b"incompressible", noise, [65536, 4464]), (b"behind-it", b"x" * 30, None)]
    b2 = [(b"later", b"y" * 40, None)]
    src, twin, dst = (new_writer(1, [b0, b1, b2], extra=256 << 10, hs=1 << 20) for _ in range(3))
    try:
        for wr in (src, twin):
            feed(wr, b0, 1)
            feed(wr, b1, 1)
        rec = open_record(src)
        assert rec["incomplete"] == 1 and rec["row_bytes"] == 0
        dst.adopt_open(src)
        assert carried(open_record(dst)) == carried(rec)
        feed(dst, b2, 1)
        feed(twin, b2, 1)
        dst.close()
        twin.close()
        a, b = dst.files(), twin.files()
        assert a == b and list(a) == ["00000001"]
        assert M.load_file(a["00000001"], orc)[0] == -1       # no offset array, no footer
    finally:
        for wr in (src, twin, dst):
            wr.free()


def test_adopt_open_refusals_and_no_op(gpu, orc):
    from kingdb_amd import _lib, put
    puts = [(b"key-%03d" % i, b"value %d " % i * 40) for i in range(120)]
    src = new_writer(1, [puts])
    busy = new_writer(1, [puts])
    other_size = new_writer(1, [puts], hs=128 << 10)
    other_hash = new_writer(0, [puts])
    holds_id = new_writer(1, [puts])
    small = put.DeviceHSTableWriter(HS, 1, HEADER + 64)
    compacted = put.DeviceHSTableWriter(HS, 1, src.arena, filetype=2, timestamp_lock=9)
    idle = new_writer(1, [puts])
    writers = [src, busy, other_size, other_hash, holds_id, small, compacted, idle]
    try:
        feed(src, puts[:40], 1)
        assert open_record(src)["fileid"] == 1
        feed(busy, puts[:5], 1)                              # a file open
        feed(holds_id, puts[:5], 1)
        holds_id.close()                                     # holds id 1
        s0 = writer_state(src)
        for what, dst in (("a file open", busy), ("another hstable_size", other_size), ("another hash", other_hash),
                          ("the id held", holds_id), ("no room", small), ("compacted mode", compacted),
                          ("itself", src)):
            d0 = writer_state(dst)
            with pytest.raises(_lib.HipError, match="EINVAL"):
                dst.adopt_open(src)
            assert writer_state(dst) == d0 and writer_state(src) == s0, what
        with pytest.raises(_lib.HipError, match="EINVAL"):
            idle.adopt_open(None)
        # src with no open file: nothing happens
        d0 = writer_state(holds_id)
        i0 = writer_state(idle)
        holds_id.adopt_open(idle)
        assert writer_state(holds_id) == d0 and writer_state(idle) == i0
        # and one that is accepted
        idle.adopt_open(src)
        assert carried(open_record(idle)) == carried(s0[4]) and writer_state(src) == s0
    finally:
        for wr in writers:
            wr.free()


# ------------------------------------------------------------- 6. end to end
def answers(x, q):
    return x.get(q, multipart_required=BIG), x.scan(multipart_required=BIG)


def same_but_dropped_deletes(old, new, compacted_ids, where_old):
    """N's answers against O's: equal, except that a key whose newest entry in
    O is a delete lying in a file the compaction covered reads NOTFOUND."""
    from kingdb_amd.index import DELETED, NOTFOUND
    dropped = 0
    for a, b, loc in zip(old[0], new[0], where_old):
        if a[0] == DELETED and (int(loc) >> 32) in compacted_ids:
            assert b == (NOTFOUND, b"")
            dropped += 1
        else:
            assert a == b
    assert old[1] == new[1]
    return dropped


@pytest.mark.parametrize("snapshot_file_closed", [False, True], ids=["its file still open", "its file closed since"])
def test_carry_open_end_to_end(gpu, orc, snapshot_file_closed):
    from kingdb_amd import put
    from kingdb_amd.index import HSTableIndex
    s = D.load()[0]["mixed"]
    ht = s["hash_type"]
    items = s["items"]
    keys = sorted({it[0] for it in items})
    more1 = [(k, b"second life of " + k * 3) for k in keys[:12]] + [(k, put.DELETE) for k in keys[12:18]] + \
        [(b"new-key-%d" % i, b"n" * (50 + i)) for i in range(5)]
    rng = np.random.default_rng(8)
    bulk = [(b"bulk-%03d" % i, rng.integers(0, 256, 800, dtype=np.uint8).tobytes()) for i in range(200)]
    more2 = [(k, b"third " + k) for k in keys[6:14]] + [(keys[20], put.DELETE), (b"new-key-1", put.DELETE)]
    more3 = [(keys[0], b"after the compaction"), (keys[30], put.DELETE), (b"brand-new", b"z" * 999)]
    more4 = [(keys[1], b"and after the second"), (b"brand-new", put.DELETE)]
    q = queries(keys + [b"new-key-%d" % i for i in range(5)] + [b"brand-new", b"never-put"] + [k for k, _ in bulk[::9]])
    everything = [items, more1, bulk, more2, more3, more4]
    w = new_writer(ht, everything)
    ix = HSTableIndex.from_resident(w)
    made = []
    try:
        with pytest.raises(ValueError, match="refresh"):     # closed files the index has not seen would be lost
            for puts in batches_of(items):
                feed(w, puts, ht)
            assert len(w.resident()[3]) >= 2
            ix.compact(carry_open=True)
        ix.refresh(tail=True)
        feed(w, more1, ht)
        snap = ix.snapshot(tail=True)
        assert snap.tail is not None and snap.tail_stats()[3] == 1
        held = len(ix.names)
        if snapshot_file_closed:
            for puts in batches_of(bulk, 40):                # the snapshot's file closes, and files behind it
                feed(w, puts, ht)
            ix.refresh(tail=True)
            assert len(ix.names) >= held + 2 and snap.tail_stats()[3] == 0
        feed(w, more2, ht)
        ix.refresh(tail=True)                                # O: this index at the moment of the call
        assert w.open_file() is not None and ix.tail is not None
        with pytest.raises(ValueError, match="open file"):   # the default is as it was
            ix.compact(snap)
        w_before = writer_state(w)
        w2, n1 = ix.compact(snap, hstable_size=HS, batch=50, spare_bytes=1 << 20, carry_open=True)
        made += [n1, w2]
        assert writer_state(w) == w_before                   # the old writer is untouched
        old = answers(ix, q)
        where = ix.locate(q)[0]
        compacted_ids = {int(f, 16) for f in snap.names}
        assert same_but_dropped_deletes(old, answers(n1, q), compacted_ids, where) >= 1
        # the open file went over as it was
        rec, rec1 = open_record(w), open_record(w2)
        assert carried(rec1) == carried(rec) and n1.tail == {"fileid": rec["fileid"], "rows": rec["rows"], "bytes": rec["bytes"]}
        comp = [f for f in n1.names if int(f, 16) > rec["fileid"]]
        assert comp and all(struct.unpack_from("<I", w2.files()[f], 12)[0] == 2 for f in comp)
        assert sorted(n1.names) == sorted(comp + [f for f in ix.names if f not in snap.names])
        # going on, on the new writer alone
        feed(w2, more3, ht)
        n1.refresh(tail=True)
        r = dict(zip(q, n1.get(q)))
        assert r[keys[0]] == (0, b"after the compaction") and r[b"brand-new"] == (0, b"z" * 999)
        assert r[keys[30]][0] == M.DELETED
        # a second compaction under the running writer, its snapshot taken inside
        old2 = answers(n1, q)
        where2 = n1.locate(q)[0]
        ids2 = {int(f, 16) for f in n1.names}
        w3, n3 = n1.compact(hstable_size=HS, batch=1000, spare_bytes=1 << 20, carry_open=True)
        made += [n3, w3]
        same_but_dropped_deletes(old2, answers(n3, q), ids2, where2)
        assert carried(open_record(w3)) == carried(open_record(w2))
        feed(w3, more4, ht)
        n3.refresh(tail=True)
        # at the end: the files on their own answer as N does
        final = view(n3, q)
        final_get = n3.get(q)
        h, loc = n3.pairs()
        w3.close()
        files = w3.files()
        want = fresh_view(files, ht, q, with_get=True)
        assert {k: want[k] for k in final} == final and want["get"] == final_get
        assert dict(zip(q, final_get))[keys[1]] == (0, b"and after the second")
        fr = HSTableIndex(files, ht)
        try:
            fh, floc = fr.pairs()
            assert [int(x) for x in fh] == [int(x) for x in h] and [int(x) for x in floc] == [int(x) for x in loc]
        finally:
            fr.close()
        model = M.Model(files, orc, ht)
        assert final["scan"] == S.scan(model, multipart_required=BIG)
    finally:
        for x in made[::-1]:
            (x.close if isinstance(x, HSTableIndex) else x.free)()
        ix.close()
        w.free()
