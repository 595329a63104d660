"""GPU: compaction by copy and the hand-over (include/kdb_compact.h,
csrc/compact.hip, HSTableIndex.compact_copy / compact).

Every case is checked against the bytes of tests/compact_model.py (pinned to
the reference's own Database by tests/test_compact_model.py) and through the
answers contract of DESIGN.md 4.12: the new index answers Get and scan as the
old one did, except that a key whose newest entry is a delete inside the
compacted view reads NOTFOUND.  Shapes are the smallest at which the copy can
go wrong: every residue mod 16 of source and destination, entries that end on,
start before and span the copy kernel's pieces, windows of one entry, finished
multipart values, and each refusal.
"""
import ctypes
import struct

import numpy as np
import pytest

import compact_model as C
import deletes_fixture as D
import index_model as M
import keylens
import scan_model as S

pytestmark = pytest.mark.gpu

NOTFOUND, DELETED = -3, -4
BIG = 1 << 31


def sync():
    from kingdb_amd import _lib
    _lib.check(_lib.load().kdb_lz4_stream_sync(None), "sync")


def copy_window(x, first, n, kmax, cap=None, slack=4096):
    """One scan window of `x` through kdb_compact_entries_batch on fresh
    buffers filled with 0xA5: (rc, dict of the downloaded arrays).  `cap` None
    sizes the entries buffer from a plan; the buffer has `slack` bytes behind
    the cap, which must come back untouched."""
    from kingdb_amd import _lib
    from kingdb_amd.index import _Lookup
    from kingdb_amd.lz4 import DeviceBuffer
    lib = _lib.load()
    L = _Lookup(n, n * kmax)
    sb = int(lib.kdb_compact_scratch_bytes(n))
    bufs = [L]
    try:
        scratch = DeviceBuffer(sb)
        bufs.append(scratch)
        po = DeviceBuffer(n * 32 + 64)
        bufs.append(po)
        o = po.ptr
        e_off, hashed, e_len, kind, status, total = o, o + 8 * n, o + 16 * n, o + 20 * n, o + 24 * n, o + ((28 * n + 7) & ~7)
        x.run_scan(L, None, first, n, 1 << 62)
        args = (L.keys.ptr, L.keys.nbytes, L.p("key_off"), L.p("key_len"), L.p("stored_off"), L.p("avail"), L.p("svc"),
                L.p("size"), L.p("checksum"), L.p("status"), n)
        _lib.check(lib.kdb_compact_plan_batch(None, *args, x.files.nbytes, x.hash_type, scratch.ptr, sb, e_off, e_len,
                                              total, hashed, kind, status), "plan")
        planned = int(po.download(8, total - o, dtype=np.uint64)[0])
        if cap is None:
            cap = planned
        entries = DeviceBuffer(cap + slack)
        bufs.append(entries)
        entries.memset(0xA5)
        sync()
        refused = ctypes.c_uint32(77)
        rc = lib.kdb_compact_entries_batch(None, x.files.ptr, x.files.nbytes, *args, x.hash_type, scratch.ptr, sb,
                                           entries.ptr, cap, e_off, e_len, total, hashed, kind, status,
                                           ctypes.byref(refused))
        sync()
        out = dict(
            planned=planned, refused=refused.value, cap=cap,
            entries=entries.download().tobytes(),
            entry_off=po.download(8 * n, 0, dtype=np.uint64), hashed=po.download(8 * n, 8 * n, dtype=np.uint64),
            entry_len=po.download(4 * n, 16 * n, dtype=np.uint32), kind=po.download(4 * n, 20 * n, dtype=np.uint32),
            status=po.download(4 * n, 24 * n, dtype=np.int32),
            total=int(po.download(8, total - o, dtype=np.uint64)[0]),
            stored_off=L.meta.download(8 * n, L.off["stored_off"], dtype=np.uint64),
            key_len=L.meta.download(4 * n, L.off["key_len"], dtype=np.uint32))
        return rc, out
    finally:
        for b in bufs:
            b.free()


def check_window(got, want, what=""):
    """`got` of copy_window against the model's entries `want` of the same rows."""
    n = len(want)
    assert got["refused"] == 0 and got["total"] == got["planned"] == sum(len(e[1]) for e in want), what
    at = 0
    for i, (key, entry, hashed, *_rest) in enumerate(want):
        assert int(got["entry_off"][i]) == at and int(got["entry_len"][i]) == len(entry), (what, i)
        assert got["entries"][at:at + len(entry)] == entry, (what, i, key[:20], len(entry))
        assert int(got["hashed"][i]) == hashed and got["kind"][i] == 0 and got["status"][i] == 0, (what, i)
        at += len(entry)
    assert len(got["status"]) == n
    tail = got["entries"][got["total"]:]
    assert tail == b"\xa5" * len(tail), what              # nothing written behind the stream


def all_windows(x, want, batch, what=""):
    """Every window of `batch` of the prepared scan of `x` against the model; the windows' arrays."""
    live = x.scan_prepare()
    assert live == len(want)
    kmax = x._scan[3]
    outs = []
    for first in range(0, live, batch):
        n = min(batch, live - first)
        rc, got = copy_window(x, first, n, kmax)
        assert rc == 0
        check_window(got, want[first:first + n], (what, first))
        outs.append(got)
    return outs


def contract(old, old_files, view_names, new, writer, orc, hs, batch, ht, queries):
    """DESIGN.md 4.12 for `new` = the index compact() returned over `writer`."""
    from kingdb_amd.index import HSTableIndex
    want, comp = C.directory(old_files, view_names, orc, hs, batch, ht)
    got = writer.files()
    assert sorted(got) == sorted(want)
    for f in want:
        assert got[f] == want[f], f                        # entries, type, timestamp, ids; the rest unchanged
    view = C.view_model(old_files, view_names, orc, ht)
    ts = C.timestamp_max(view)
    for f in comp:
        assert struct.unpack_from("<IQ", got[f], 12) == (2, ts) and M.footer(got[f])[:2] == (2, 0)
    assert comp == ["%08x" % (max(int(f, 16) for f in old_files) + 1 + i) for i in range(len(comp))]
    assert new.file_status == {f: 0 if f in comp else old.file_status[f] for f in got}
    order = sorted(new.names, key=lambda f: (struct.unpack_from("<Q", got[f], 16)[0], int(f, 16)))
    assert order[:len(comp)] == comp
    # answers
    a, b = old.get(queries, multipart_required=BIG), new.get(queries, multipart_required=BIG)
    whole = M.Model(old_files, orc, ht)
    for q, x, y in zip(queries, a, b):
        if x[0] == DELETED and y[0] == NOTFOUND:
            loc = whole.get(q)[2]
            assert "%08x" % (loc >> 32) in view.files, q  # the delete lay in the compacted view
        else:
            assert x == y, q
    assert new.scan(multipart_required=BIG) == old.scan(multipart_required=BIG)
    # equivalence with a fresh index over the downloaded files
    fresh = HSTableIndex(got, ht)
    try:
        assert [[int(v) for v in p] for p in fresh.pairs()] == [[int(v) for v in p] for p in new.pairs()]
        for x, y in zip(fresh.locate(queries), new.locate(queries)):
            assert list(x) == list(y)
        assert fresh.scan(multipart_required=BIG) == new.scan(multipart_required=BIG)
    finally:
        fresh.close()
    return got, comp


# ------------------------------------------------------------- 1. alignment
@pytest.fixture(scope="module")
def aligned(gpu, orc):
    """The xx stream of key_lengths.npz (keys of every length 1..80, 127-129,
    252-260, 511-516, 1000) plus values of the lengths where a 16-byte word
    begins or ends, written through this project's put path."""
    from kingdb_amd import put
    kl = keylens.load()["xx"]
    rng = np.random.default_rng(5)
    noise = rng.integers(0, 256, 8192, dtype=np.uint8).tobytes()
    text = (b"the quick brown fox jumps over the lazy dog " * 200)
    puts = [(k, v, None) for k, v, _ in kl["puts"]]      # every put in one part: every entry self-contained
    lens = (0, 1, 3, 4, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097)
    keys = kl["keys"]
    for i, n in enumerate(lens * 4):
        src = noise if i % 2 else text
        puts.append((keys[(7 * i) % len(keys)] + b"#%d" % i, src[i:i + n], None))
    files = put.write_hstables_device(puts, 32 << 20, 1, batch=97)
    return dict(files=files, puts=puts, lens=lens)


def test_alignment_every_residue(gpu, aligned, orc):
    from kingdb_amd.index import HSTableIndex
    files = aligned["files"]
    view = C.view_model(files, sorted(files), orc, 1)
    want = C.entries(view)
    assert {len(k) for k, *_ in want} >= set(range(1, 81)) | {127, 128, 129, 1000} | set(range(252, 261)) | set(range(511, 517))
    have = {e[3] for e in want}
    assert set(aligned["lens"]) <= have
    ix = HSTableIndex(files, 1)
    try:
        all_windows(ix, want, 97, "windows of 97")
        (got,) = all_windows(ix, want, len(want), "one window")
        # where the value bytes start on both sides, for values of at least one 16-byte word
        src_res, dst_res, pairs = set(), set(), set()
        for i, (key, entry, _, _, _, _, stored) in enumerate(want):
            if len(stored) >= 16:
                a = (ix.files.ptr + int(got["stored_off"][i])) % 16
                b = (int(got["entry_off"][i]) + len(entry) - len(stored)) % 16
                src_res.add(a)
                dst_res.add(b)
                pairs.add((a - b) % 16)
        assert src_res == set(range(16)) and dst_res == set(range(16))
        assert pairs == set(range(16))                     # and every shift between the two
    finally:
        ix.close()


def test_small_values_are_the_files_of_compacted_device(gpu, aligned, orc):
    """Every live entry self-contained: a plain writer fed the copied windows
    writes byte for byte what compacted_device (decode, compress again) writes,
    and the type-2 files differ from them in type and timestamp alone."""
    from kingdb_amd.index import HSTableIndex
    files = aligned["files"]
    view = C.view_model(files, sorted(files), orc, 1)
    for _, off, name, _ in S.live_rows(view):
        assert M.locate_entry(files[name], off, False, orc)[1]["flags"] == 0x8
    ix = HSTableIndex(files, 1)
    ws = []
    try:
        for hs, batch in ((64 << 10, 50), (32 << 20, 1000)):
            a, b, c = ix.compacted_device(hs, batch), ix.compact_copy(hs, batch, filetype=1, lock=False), \
                ix.compact_copy(hs, batch)
            ws += [a, b, c]
            fa, fb, fc = a.files(), b.files(), c.files()
            assert fa == fb and len(fa) >= (2 if hs == 64 << 10 else 1)
            assert fc == C.compacted_files(view, hs, batch, 1)
            assert fa == C.compacted_files(view, hs, batch, 1, filetype=1, timestamp=0)
    finally:
        for w in ws:
            w.free()
        ix.close()


# ------------------------------------------------------------- 2. piece boundaries
def test_piece_boundaries(gpu, orc):
    from oracle import hstable
    from kingdb_amd import _lib, put
    from kingdb_amd.index import HSTableIndex
    piece = int(_lib.load().kdb_compact_piece_bytes())
    rng = np.random.default_rng(9)
    noise = rng.integers(0, 256, 400000, dtype=np.uint8).tobytes()

    def entry_len(key, value):
        w = hstable.Writer(orc, 32 << 20, 1)
        w.put(key, value)
        w.close()
        return len(w.dense()[0][0])

    def sized(key, target):
        """An incompressible value whose entry is `target` bytes long."""
        n = target - 64
        for _ in range(4):
            n += target - entry_len(key, noise[:n])
        assert entry_len(key, noise[:n]) == target
        return key, noise[:n], None

    puts = [sized(b"ends-on-a-boundary", piece),              # [0, piece)
            sized(b"one-short", piece - 1),                   # [piece, 2 piece - 1)
            (b"starts-one-before", noise[7:107], None),       # starts at 2 piece - 1
            (b"s1", b"x" * 20, None),
            (b"three-pieces-and-more", noise[:300000], None),
            (b"s2", b"y" * 20, None)]
    files = put.write_hstables_device(puts, 32 << 20, 1)
    view = C.view_model(files, sorted(files), orc, 1)
    want = C.entries(view)
    assert [k for k, *_ in want] == [p[0] for p in puts]
    ix = HSTableIndex(files, 1)
    try:
        (got,) = all_windows(ix, want, len(want), "one window")
        off, ln = [int(v) for v in got["entry_off"]], [int(v) for v in got["entry_len"]]
        assert off[1] == piece and (off[1] + ln[1]) % piece == piece - 1 and off[2] % piece == piece - 1
        assert ln[4] >= 3 * piece and ln[3] < 64 and ln[5] < 64
        all_windows(ix, want, 1, "windows of one entry")
        # 20-byte values around the large one, alone in their window
        rc, got = copy_window(ix, 3, 3, ix._scan[3])
        assert rc == 0
        check_window(got, want[3:6], "small, large, small")
        w = ix.compact_copy(1 << 20, 2)
        try:
            assert w.files() == C.compacted_files(view, 1 << 20, 2, 1)
        finally:
            w.free()
    finally:
        ix.close()


# ------------------------------------------------------------- 3. multipart
def test_multipart_values_keep_their_stored_bytes(gpu, orc):
    from kingdb_amd import get as G
    from kingdb_amd import put
    from kingdb_amd.index import HSTableIndex
    rng = np.random.default_rng(13)
    text = b"All work and no play makes Jack a dull boy. " * 30000
    noise = rng.integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()

    def chunks(n):
        return [65536] * (n // 65536) + ([n % 65536] if n % 65536 else [])

    # (the 70 000 incompressible bytes are test_unfinished_multipart_value's: the reference never finishes them)
    values = {b"compressible": text[:100000], b"mixed": text[:70000] + noise[:70000] + text[:30000],
              b"one-past-a-mebibyte": text[3:3 + 1048577]}
    puts = [(b"small-before", b"v" * 30, None)] + [(k, v, chunks(len(v))) for k, v in values.items()] + \
        [(b"small-after", b"w" * 30, None)]
    hs = 4 << 20
    files = put.write_hstables_device(puts, hs, 1)
    view = C.view_model(files, sorted(files), orc, 1)
    want = C.entries(view)
    src = {k: M.locate_entry(files[name], off, True, orc)[1] for _, off, name, k in S.live_rows(view)}
    for k in values:
        assert src[k]["flags"] == 0x8 | 0x2 | 0x4 and src[k]["svc"] > 0, k     # finished multipart
    big = src[b"one-past-a-mebibyte"]
    assert big["padding"] == 136
    hl = {k: len(e) - len(k) - len(stored) for k, e, _, _, _, _, stored in want}
    assert hl[b"one-past-a-mebibyte"] == big["size_header"] - 1                # the padding varint: two bytes -> one
    ix = HSTableIndex(files, 1)
    w = old = n2 = None
    try:
        all_windows(ix, want, len(want), "multipart")
        all_windows(ix, want, 2, "multipart, windows of two")
        w = ix.compact_copy(hs, 3)
        got = w.files()
        assert got == C.compacted_files(view, hs, 3, 1)
        for f in got.values():
            assert M.footer(f)[:2] == (2, 0)                                   # no padding flag
            for e in G.read_hstable(f):
                assert e.flags == 0x8 and e.size_padding == 0
        n2 = HSTableIndex.from_resident(w)
        keys = [p[0] for p in puts]
        answers = n2.get(keys, verify=2, multipart_required=BIG)
        assert answers == [(0, p[1]) for p in puts] == ix.get(keys, verify=2, multipart_required=BIG)
        # the old compaction: the same answers out of other bytes
        old = ix.compacted_device(hs, 3)
        fo = old.files()
        o2 = HSTableIndex(fo, 1)
        try:
            assert o2.get(keys, multipart_required=BIG) == answers
        finally:
            o2.close()
        assert [e.key for f in sorted(fo) for e in G.read_hstable(fo[f])] == \
            [e.key for f in sorted(got) for e in G.read_hstable(got[f])]
        assert b"".join(fo[f] for f in sorted(fo)) != b"".join(got[f] for f in sorted(got))
    finally:
        for x in (n2, ix):
            if x is not None:
                x.close()
        for x in (w, old):
            if x is not None:
                x.free()


def test_unfinished_multipart_value(gpu, orc):
    """70 000 incompressible bytes in 64 KiB parts.  The reference's PutPart
    stores the second part with a header of its own, so its end (70 016) is
    not size_value_compressed (70 008), Order::IsLastPart never holds, the
    entry keeps its first-part header (uncompacted | padding,
    size_value_compressed 0, checksum 0) and its file gets no offset array
    (put.hip, tests/golden/make_golden_put.py `multipart`).  So this size
    cannot be a finished multipart value and does not decode to what was put,
    in the reference or here: the file loads only after recovery, which -- as
    the reference's RecoverFile -- leaves the unfinished entry out.  What
    holds: the compaction of the recovered file copies its two other entries
    as the model says and answers as the recovered file does, NOTFOUND for
    the unfinished key included."""
    from kingdb_amd import get as G
    from kingdb_amd import put
    from kingdb_amd.index import HSTableIndex
    noise = np.random.default_rng(13).integers(0, 256, 70000, dtype=np.uint8).tobytes()
    puts = [(b"small-before", b"v" * 30, None), (b"incompressible", noise, [65536, 4464]),
            (b"small-after", b"w" * 30, None)]
    files = put.write_hstables_device(puts, 4 << 20, 1)
    (name,) = files
    f = files[name]
    assert M.load_file(f, orc)[0] == -1                                        # no offset array
    ents = G.read_hstable(f)
    assert [e.key for e in ents] == [p[0] for p in puts]
    e = ents[1]
    assert (e.flags, e.size_value_compressed, e.checksum, e.size_padding) == (0xe, 0, 0, 16)
    # the model's view: the file with an offset array of the two finished entries
    rows = [(x.hashed, x.offset) for x in ents if x.key != b"incompressible"]
    arr = b"".join(M.put_varint(h) + M.put_varint(o) for h, o in rows)
    out = f + arr + struct.pack("<IIQQQ", 1, 0, len(f), len(rows), M.MAGIC)
    model_files = {name: out + struct.pack("<I", orc.crc32c(arr + out[-32:]))}
    view = C.view_model(model_files, [name], orc, 1)
    want = C.entries(view)
    assert [k for k, *_ in want] == [b"small-before", b"small-after"]
    ix = HSTableIndex(files, 1, recover="reference")
    w = n2 = None
    try:
        assert ix.file_status == {name: 0} and ix.entries == 2
        all_windows(ix, want, 2, "unfinished")
        w = ix.compact_copy(4 << 20, 2)
        assert w.files() == C.compacted_files(view, 4 << 20, 2, 1)
        n2 = HSTableIndex.from_resident(w)
        keys = [p[0] for p in puts]
        got = n2.get(keys, multipart_required=BIG)
        assert got == ix.get(keys, multipart_required=BIG)
        assert got == [(0, b"v" * 30), (NOTFOUND, b""), (0, b"w" * 30)]
    finally:
        for x in (n2, ix):
            if x is not None:
                x.close()
        if w is not None:
            w.free()


# ------------------------------------------------------------- 4. the hand-over end to end
def append(w, batch, ht):
    from kingdb_amd import put
    b, n = put.put_entries_device(batch, ht)
    try:
        w.append_batch(b, n)
        sync()
    finally:
        b.free()


def test_hand_over_end_to_end(gpu, orc):
    from kingdb_amd import put
    from kingdb_amd.index import HSTableIndex
    s = D.load()[0]["mixed"]
    hs, ht = s["hstable_size"], s["hash_type"]
    assert hs == 64 << 10                                    # `rollover`-sized files
    # the fixture's overwrites and deletes, then enough live bytes for the copy to fill several files
    noise = np.random.default_rng(21).integers(0, 256, 4096, dtype=np.uint8).tobytes()
    extra = [(b"extra-%03d" % i, noise[5 * i:5 * i + 700 + i], None) for i in range(200)]
    items = s["items"] + extra
    last = D.last_ops(s["ops"])
    live = [k for k in s["keys"] if last[k] is not None]
    dead = [k for k in s["keys"] if last[k] is None]
    assert len(live) >= 20 and dead
    more1 = [(k, b"second life of " + k * 3, None) for k in live[:12]] + [(k, put.DELETE) for k in live[12:18]] + \
        [(b"new-key-%d" % i, b"n" * (50 + i), None) for i in range(5)]
    more2 = [(k, b"third " + k, None) for k in live[6:14]] + [(dead[0], b"back again", None), (live[19], put.DELETE)]
    more3 = [(live[0], b"after the compaction", None), (live[30 % len(live)], put.DELETE), (b"brand-new", b"z" * 999, None)]
    everything = items + more1 + more2 + more3
    w = put.DeviceHSTableWriter(hs, ht, put.DeviceHSTableWriter.arena_bytes(
        hs, put.entries_bound(everything), len(everything)) + (1 << 20))
    q = list(s["keys"]) + [b"new-key-%d" % i for i in range(5)] + [b"brand-new", b"never-put"] + \
        [k for k, _, _ in extra[::9]]
    ix = snap = w2 = n1 = w3 = n3 = None
    try:
        for i in range(0, len(items), 64):
            append(w, items[i:i + 64], ht)
        w.close()
        ix = HSTableIndex.from_resident(w)
        view_names = list(ix.names)
        assert len(view_names) >= 3                          # the copy spans several files
        snap = ix.snapshot()
        for more in (more1, more2):
            append(w, more, ht)
            w.close()
        assert ix.refresh() == len(more1) + len(more2)
        assert len(ix.names) == len(view_names) + 2
        old_files = w.files()
        before = (ix.get(q, multipart_required=BIG), ix.scan(multipart_required=BIG))
        w2, n1 = ix.compact(snap, hstable_size=hs, batch=50, spare_bytes=1 << 20)
        got, comp = contract(ix, old_files, view_names, n1, w2, orc, hs, 50, ht, q)
        assert len(comp) >= 2
        # the old index, its snapshot and its writer are untouched
        assert (ix.get(q, multipart_required=BIG), ix.scan(multipart_required=BIG)) == before
        assert w.files() == old_files and snap.names == view_names
        # at least one delete of the view was dropped: its key now reads NOTFOUND
        a, b = ix.get(q), n1.get(q)
        assert any(x[0] == DELETED and y[0] == NOTFOUND for x, y in zip(a, b))
        # going on: puts into the new writer win over everything
        append(w2, more3, ht)
        w2.close()
        assert n1.refresh() == len(more3)
        newest = n1.names[-1]
        assert int(newest, 16) == max(int(f, 16) for f in got) + 1
        f_new = w2.files()[newest]
        assert struct.unpack_from("<IQ", f_new, 12) == (1, int(newest, 16))     # ordinary file, timestamp = id
        r = dict(zip(q, n1.get(q)))
        assert r[live[0]] == (0, b"after the compaction") and r[b"brand-new"] == (0, b"z" * 999)
        assert r[live[30 % len(live)]] == (DELETED, b"")
        for k, v in zip(q, b):
            if k not in (live[0], live[30 % len(live)], b"brand-new"):
                assert r[k] == v, k
        model = M.Model(w2.files(), orc, ht)
        assert n1.scan(multipart_required=BIG) == S.scan(model, multipart_required=BIG)
        # a second compaction, of everything the new index holds
        files1 = w2.files()
        w3, n3 = n1.compact(hstable_size=hs, batch=1000)
        contract(n1, files1, list(n1.names), n3, w3, orc, hs, 1000, ht, q)
        assert all(struct.unpack_from("<I", f, 12)[0] == 2 for f in w3.files().values())
    finally:
        for x in (n3, n1, snap, ix):
            if x is not None:
                x.close()
        for x in (w3, w2, w):
            if x is not None:
                x.free()


# ------------------------------------------------------------- 5. refusals
def writer_state(w):
    ptr, off, size, fid = w.resident()
    return ptr, list(off), list(size), list(fid), w.open_bytes(), w.files()


def test_hand_over_refusals(gpu, orc):
    from kingdb_amd import _lib, put
    from kingdb_amd.index import HSTableIndex
    from kingdb_amd.lz4 import DeviceBuffer
    puts = [(b"key-%03d" % i, b"value %d " % i * 40, None) for i in range(300)]
    hs = 64 << 10
    src_files = put.write_hstables_device(puts[:100], hs, 1)
    name, blob = sorted(src_files.items())[0]
    src = DeviceBuffer(len(blob) + 64)
    src.upload(np.frombuffer(blob, np.uint8))
    one = (np.zeros(1, np.uint64), np.array([len(blob)], np.uint64))
    w = put.DeviceHSTableWriter(hs, 1, put.DeviceHSTableWriter.arena_bytes(hs, put.entries_bound(puts), len(puts)) +
                                len(blob) + 64)
    tight = put.DeviceHSTableWriter(hs, 1, put.DeviceHSTableWriter.arena_bytes(hs, put.entries_bound(puts[:50]), 50))
    ix = None
    try:
        append(w, puts[:200], 1)
        assert w.open_bytes() > 0                            # a file is open
        st = writer_state(w)
        with pytest.raises(_lib.HipError, match="EINVAL"):
            w.adopt(100, src.ptr, *one, np.array([7], np.uint32))
        assert writer_state(w) == st
        ix = HSTableIndex.from_resident(w)
        with pytest.raises(ValueError, match="open file"):
            ix.compact()
        w.close()
        assert w.open_bytes() == 0
        st = writer_state(w)
        nown = len(st[3])
        two = (np.array([0, 0], np.uint64), np.array([len(blob)] * 2, np.uint64))
        for first, ids, arrs in ((100, [100], one), (100, [101], one), (100, [0], one), (100, [7, 7], two),
                                 (0, [7], one), (2 ** 32 - 2, [7], one)):
            with pytest.raises(_lib.HipError, match="EINVAL"):
                w.adopt(first, src.ptr, *arrs, np.array(ids, np.uint32))
            assert writer_state(w) == st, (first, ids)
        # bytes that do not fit
        append(tight, puts[:50], 1)
        tight.close()
        t0 = writer_state(tight)
        room = tight.arena - int(t0[1][-1] + t0[2][-1])
        k = room // len(blob) + 1                            # one file more than the room holds
        many = (np.zeros(k, np.uint64), np.array([len(blob)] * k, np.uint64))
        with pytest.raises(_lib.HipError, match="EINVAL"):
            tight.adopt(100, src.ptr, *many, np.arange(1, k + 1, dtype=np.uint32))
        assert writer_state(tight) == t0
        assert k < 100
        # and a hand-over that is accepted: the files are renumbered, the adopted one is copied
        w.adopt(100, src.ptr, *one, np.array([7], np.uint32))
        after = writer_state(w)
        assert after[3] == list(range(100, 100 + nown)) + [7] and after[4] == 0
        assert list(after[5].values())[:nown] == list(st[5].values()) and after[5]["00000007"] == blob
        assert after[1][-1] % 64 == 0 and after[1][-1] >= st[1][-1] + st[2][-1]
        append(w, puts[200:], 1)
        w.close()
        newest = w.resident()[3][-1]
        assert int(newest) == 100 + nown                       # the next id above everything held
    finally:
        if ix is not None:
            ix.close()
        for x in (w, tight):
            x.free()
        src.free()


def test_copy_refusals(gpu, orc):
    """An entries_cap one byte short refuses the window before a byte is
    copied; a row whose stored length its value region cannot hold (forged in
    an uploaded copy of a file) is refused alone."""
    from kingdb_amd import _lib, put
    from kingdb_amd.index import HSTableIndex
    rng = np.random.default_rng(3)
    text = b"It was the best of times, it was the worst of times. " * 4000
    puts = [(b"a-small", b"s" * 40, None), (b"multipart", text[:150000], [65536, 65536, 18928]),
            (b"z-small", rng.integers(0, 256, 333, dtype=np.uint8).tobytes(), None)]
    files = put.write_hstables_device(puts, 4 << 20, 1)
    (name,) = files
    view = C.view_model(files, [name], orc, 1)
    want = C.entries(view)
    ix = HSTableIndex(files, 1)
    try:
        ix.scan_prepare()
        kmax = ix._scan[3]
        total = sum(len(e[1]) for e in want)
        rc, got = copy_window(ix, 0, 3, kmax, cap=total - 1)
        assert rc == _lib.EINVAL and got["planned"] == total
        assert got["entries"] == b"\xa5" * len(got["entries"])          # nothing was copied
        rc, got = copy_window(ix, 0, 3, kmax, cap=total)
        assert rc == 0
        check_window(got, want)
    finally:
        ix.close()
    # the forged row: size_value_compressed of the multipart entry raised past size_value + padding
    f = bytearray(files[name])
    off = next(o for _, o, _, k in S.live_rows(view) if k == b"multipart")
    e = M.locate_entry(bytes(f), off, False, orc)[1]
    assert e["flags"] & 0x2 and e["svo"] == e["size_value"] + e["padding"]
    svc_at = off + e["size_header"] - 8 - len(M.put_varint(e["padding"])) - 8
    assert struct.unpack_from("<Q", f, svc_at)[0] == e["svc"]
    struct.pack_into("<Q", f, svc_at, e["svo"] + 1)
    forged = {name: bytes(f)}
    ix = HSTableIndex(forged, 1)
    try:
        assert ix.file_status == {name: 0} and ix.scan_prepare() == 3
        rc, got = copy_window(ix, 0, 3, ix._scan[3])
        assert rc == 0 and got["refused"] == 1
        assert [int(s) for s in got["status"]] == [0, -1, 0] and int(got["entry_len"][1]) == 0
        assert got["total"] == len(want[0][1]) + len(want[2][1])
        assert got["entries"][:got["total"]] == want[0][1] + want[2][1]
        tail = got["entries"][got["total"]:]
        assert tail == b"\xa5" * len(tail)
        with pytest.raises(_lib.HipError, match="stored length"):
            ix.compact_copy(4 << 20, 10)
        assert ix.scan(0, 1) == [(b"a-small", 0, b"s" * 40)]                      # the handle answers as before
    finally:
        ix.close()
