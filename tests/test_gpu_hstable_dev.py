"""GPU: HSTable files written on the device (csrc/hstable_dev.hip,
include/kdb_hstable_dev.h).

Expected bytes come from the reference's own files (hstable_streams.npz) and
from the host writer (csrc/hstable.cc), which tests/test_write_path.py pins to
the reference and the oracle.  The cut edges are fed as synthetic per-entry
arrays to both writers; kdb_index_load_files, which shares the CRC primitives
and the format constants with the device writer but verifies footers and
parses rows with code of its own, then loads what the writer left in device
memory.
"""
import os
import struct
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_golden_put import decode_stream  # noqa: E402

pytestmark = pytest.mark.gpu

HEADER = 8192


def _sets(npz, with_keys):
    z = load_golden(npz)
    out = {}
    for name in (str(n) for n in z["names"]):
        files = {str(f): z[f"{name}__file_{f}"].tobytes() for f in z[f"{name}__files"]}
        d = {"files": files, "hash_type": int(z[f"{name}__opts"][1]), "hstable_size": int(z[f"{name}__opts"][0]),
             "puts": decode_stream(z[f"{name}__stream"].tobytes())}
        if with_keys:
            d["keys"] = [k.tobytes() for k in z[f"{name}__keys"]]
        out[name] = d
    return out


@pytest.fixture(scope="module")
def streams():
    return _sets("hstable_streams.npz", False)


@pytest.fixture(scope="module")
def getkeys():
    return _sets("get_keys.npz", True)


def assert_same_files(got, want):
    assert sorted(got) == sorted(want)
    for f in want:
        assert len(got[f]) == len(want[f]), f
        assert got[f] == want[f], f


# ------------------------------------------------------------- 4, 5: the put streams
@pytest.mark.parametrize("name", ["small", "edge", "rollover", "murmur", "multipart"])
def test_reference_parity(gpu, streams, name):
    from kingdb_amd import put
    s = streams[name]
    got = put.write_hstables_device(s["puts"], s["hstable_size"], s["hash_type"])
    assert_same_files(got, s["files"])


@pytest.mark.parametrize("batch", [1, 7, 64])
def test_batches_equal_the_host_writer(gpu, streams, batch):
    from kingdb_amd import put
    s = streams["rollover"]
    want = put.write_hstables(s["puts"], s["hstable_size"], s["hash_type"], batch)
    assert len(want) == 8
    assert_same_files(put.write_hstables_device(s["puts"], s["hstable_size"], s["hash_type"], batch), want)


# ------------------------------------------------------------- 6: cut edges, fed directly
class Batch:
    """Per-entry arrays of one append, as kdb_put_entries_batch would leave them."""

    def __init__(self, lens, kinds=None, status=None, hashes=None, rng=None, offsets=None):
        n = len(lens)
        self.n = n
        self.len = np.array(lens, np.uint32)
        self.kind = np.array(kinds if kinds is not None else [0] * n, np.uint32)
        self.status = np.array(status if status is not None else [0] * n, np.int32)
        self.hashed = (np.array(hashes, np.uint64) if hashes is not None
                       else rng.integers(0, 2 ** 64, n, dtype=np.uint64))
        if offsets is None:
            off = np.zeros(n, np.uint64)
            if n > 1:
                off[1:] = np.cumsum(self.len[:-1].astype(np.uint64))
            size = int(self.len.sum())
        else:
            off = np.array(offsets, np.uint64)
            size = int((off + self.len).max()) if n else 0
        self.off = off
        self.entries = rng.integers(0, 256, max(size, 1), dtype=np.uint8)


def host_files(batches, hs, ht=1):
    from kingdb_amd import put
    w = put.HSTableWriter(hs, ht)
    for b in batches:
        w.append(put.PutBatchResult(entries=b.entries, entry_off=b.off, entry_len=b.len, hashed=b.hashed,
                                    crc=np.zeros(b.n, np.uint32), kind=b.kind, status=b.status))
    w.close()
    return w.files()


def feed(w, b):
    """One append of the device writer from uploaded copies of the arrays."""
    from kingdb_amd.lz4 import DeviceBuffer
    bufs = []
    try:
        ptrs = []
        for a in (b.entries, b.off, b.len, b.hashed, b.kind, b.status):
            d = DeviceBuffer(max(a.nbytes, 8))
            bufs.append(d)
            if a.nbytes:
                d.upload(a)
            ptrs.append(d.ptr)
        w.append_ptrs(None, *ptrs, b.n)
        from kingdb_amd import _lib
        _lib.check(_lib.load().kdb_lz4_stream_sync(None), "sync")
    finally:
        for d in bufs:
            d.free()


def device_files(batches, hs, ht=1, arena=None):
    from kingdb_amd import put
    total = sum(int(b.len.sum()) for b in batches)
    n = sum(b.n for b in batches)
    w = put.DeviceHSTableWriter(hs, ht, arena or put.DeviceHSTableWriter.arena_bytes(hs, total, n))
    try:
        for b in batches:
            feed(w, b)
        w.close()
        return w.files()
    finally:
        w.free()


def walk(state, hs, lens, kinds=None, status=None):
    """The cut rule entry by entry, to build inputs that hit its edges:
    state = [open, fsize]; returns the fsize of every file closed."""
    closed = []
    for i, ln in enumerate(lens):
        if status is not None and status[i] != 0:
            continue
        if state[0] and state[1] > hs:
            closed.append(state[1])
            state[0] = False
        if not state[0]:
            state[0], state[1] = True, HEADER
        state[1] += ln
        if kinds is not None and kinds[i] != 0 and state[1] >= hs:
            closed.append(state[1])
            state[0] = False
    if state[0] and state[1] >= hs:
        closed.append(state[1])
        state[0] = False
    return closed


def fill_to(rng, fs, target):
    """Entry lengths of 26..300 that take a file from fsize fs to exactly target."""
    lens = []
    left = target - fs
    assert left >= 26
    while left > 326:
        lens.append(int(rng.integers(26, 301)))
        left -= lens[-1]
    if left > 300:
        lens.append(100)
        left -= 100
    lens.append(left)
    return lens


def edge_batches(rng, hs, holes):
    """Three appends, 300 entries: append 1 ends with fsize == hs exactly (the
    file closes with the batch); in append 2 a file reaches exactly hs before
    an entry (which still goes in).  holes: status = -1 entries in between, a
    kind = 1 entry that ends exactly at hs and a kind = 2 entry."""
    state = [False, 0]
    # append 1: 60 entries as they come, then up to exactly hs
    l1 = [int(x) for x in rng.integers(26, 301, 60)]
    walk(state, hs, l1)
    while not state[0] or hs - state[1] < 26:          # no room to land on hs exactly: go on to the next file
        l1.append(40)
        state = [False, 0]
        walk(state, hs, l1)
    l1 += fill_to(rng, state[1], hs)
    s1 = [False, 0]
    closed1 = walk(s1, hs, l1)
    assert not s1[0] and closed1[-1] == hs
    # append 2: a new file filled to exactly hs, then entries that see fsize == hs and fsize > hs
    l2 = fill_to(rng, HEADER, hs) + [50, 60, 70]
    k2 = [0] * len(l2)
    st2 = [0] * len(l2)
    if holes:
        # a second file of the append: filled to hs - 200, then a kind = 1 entry of 200 that ends at hs
        fill = fill_to(rng, HEADER + 60 + 70, hs - 200)
        l2 += fill + [200, 33, 44]
        k2 += [0] * len(fill) + [1, 0, 0]
        st2 += [0] * (len(fill) + 3)
        for at in (3, 11, len(l2) - 2):                # failed puts: no bytes, any kind
            l2.insert(at, 0)
            k2.insert(at, 1)
            st2.insert(at, -1)
    s2 = [False, 0]
    closed2 = walk(s2, hs, l2, k2, st2)
    assert closed2[0] == hs + 50 and (not holes or closed2[1] == hs)
    # append 3: the rest, continuing the open file
    n3 = 300 - len(l1) - len(l2)
    assert n3 > 20
    l3 = [int(x) for x in rng.integers(26, 301, n3)]
    k3 = [0] * n3
    st3 = [0] * n3
    if holes:
        k3[5] = 2                                      # its file keeps no offset array
        k3[n3 - 4] = 1
        for at in (0, 1, n3 - 1):
            l3[at], st3[at] = 0, -1
    return [Batch(l1, rng=rng), Batch(l2, k2, st2, rng=rng), Batch(l3, k3, st3, rng=rng)]


def test_cut_edges_plain(gpu):
    rng = np.random.default_rng(61)
    hs = 16384
    batches = edge_batches(rng, hs, False)
    want = host_files(batches, hs)
    assert len(want) >= 4
    assert_same_files(device_files(batches, hs), want)


def test_cut_edges_holes_and_kinds(gpu):
    rng = np.random.default_rng(62)
    hs = 16384
    batches = edge_batches(rng, hs, True)
    want = host_files(batches, hs)
    # the kind = 2 entry's file has no footer, the others do
    magic = (0x4D454F57).to_bytes(8, "little")
    assert sum(f[-12:-4] != magic for f in want.values()) == 1
    assert_same_files(device_files(batches, hs), want)


def test_non_dense_stream(gpu):
    """entry_off with gaps and one backwards jump: the bytes are copied by entry_off."""
    rng = np.random.default_rng(63)
    hs = 16384
    lens = [int(x) for x in rng.integers(26, 301, 120)]
    offs, at = [], 5000
    for i, ln in enumerate(lens):
        at += int(rng.integers(0, 40)) if i % 3 else 0
        offs.append(at)
        at += ln
    offs[70] = 17                                      # backwards, to an odd address
    b = Batch(lens, rng=rng, offsets=offs)
    want = host_files([b], hs)
    assert len(want) >= 2
    assert_same_files(device_files([b], hs), want)


def test_varint_steps(gpu):
    """Hashes at every varint64 length's edge; 40 entries of 64 KiB in one
    3 MiB file: offsets of 2, 3 and 4 varint bytes."""
    rng = np.random.default_rng(64)
    hs = 3 << 20
    special = [0, 127, 128, 2 ** 56 - 1, 2 ** 56, 2 ** 63, 2 ** 64 - 1]
    hashes = [special[i % len(special)] for i in range(40)]
    b = Batch([65536] * 40, hashes=hashes, rng=rng)
    want = host_files([b], hs)
    assert len(want) == 1 and len(next(iter(want.values()))) > HEADER + 40 * 65536
    assert_same_files(device_files([b], hs), want)


def test_long_offset_array(gpu):
    """8 192 entries of 26 bytes in one file: ~100 KB of rows, so the close's
    CRC spans all its waves and goes through the combine."""
    rng = np.random.default_rng(65)
    hs = 1 << 20
    batches = [Batch([26] * 5000, rng=rng), Batch([26] * 3192, rng=rng)]
    want = host_files(batches, hs)
    assert len(want) == 1 and len(next(iter(want.values()))) > HEADER + 8192 * 26 + 80000
    assert_same_files(device_files(batches, hs), want)


def real_batch(orc, rng, n):
    """n entries of 26 to 298 bytes (the first has 26) that a recovery walk
    accepts: a header by oracle.entry_header, a key of 1 to 8 bytes and a raw
    value, kEntryFull; the rows' hashes are the headers'."""
    hashes = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    ents = []
    for i in range(n):
        key = bytes(rng.integers(0, 256, 1 + i % 8, dtype=np.uint8))
        value = bytes(rng.integers(0, 256, int(rng.integers(0, 265)) if i else 0, dtype=np.uint8))
        h = orc.entry_header(orc.crc32c(key + value), 0x8, len(key), len(value), 0, 0, int(hashes[i]))
        ents.append(h + key + value)
    assert len(ents[0]) == 26 and all(26 <= len(e) <= 300 for e in ents)
    b = Batch([len(e) for e in ents], hashes=hashes, rng=rng)
    b.entries = np.frombuffer(b"".join(ents), np.uint8).copy()
    return b


def rows_of(f):
    """(offset_indexes, bytes of the rows, num_entries) of a closed file."""
    oi, n = struct.unpack_from("<QQ", f, len(f) - 28)
    return oi, len(f) - 36 - oi, n


def test_short_offset_arrays(gpu, orc):
    """The short end of the closer's arithmetic (csrc/hstable_close.h: 64 pieces
    per file, crc::extend_block's 16 parts per piece), which the writer, the
    index load and recovery share: files of 1, 2, 5, 7, 70 and 110 rows -- one
    row; fewer than 64 bytes of rows, so some pieces are empty; just above 64,
    where a piece has two bytes; below and above 1 024, where a wave's part
    has two -- and five files of one entry each closed by one append
    (hstable_size 8193, the smallest either writer takes: above the header
    block, so the first entry already passes it).  Every
    file equals the host writer's, loads into the index where it lies, and,
    cut at its offset array, is recovered as the model recovers it."""
    import recover_model as R
    from kingdb_amd import put
    from kingdb_amd import recover as rec
    from kingdb_amd.index import HSTableIndex
    rng = np.random.default_rng(67)
    counts = (1, 2, 5, 7, 70, 110)
    sets = [(real_batch(orc, rng, n), 1 << 20, 1) for n in counts] + [(real_batch(orc, rng, 5), 8193, 5)]
    want = {}
    for s, (b, hs, nfiles) in enumerate(sets):
        host = host_files([b], hs)
        assert len(host) == nfiles
        want.update({"%d-%s" % (s, f): data for f, data in host.items()})
    assert len(want) == 11
    rb = [rows_of(want["%d-00000001" % s])[1] for s in range(6)]
    print("row bytes", rb, [rows_of(f)[1] for n, f in sorted(want.items()) if n.startswith("6-")])
    assert [rows_of(want["%d-00000001" % s])[2] for s in range(6)] == list(counts)
    assert 3 <= rb[0] <= 15 and rb[0] < rb[1] < rb[2] < 64 < rb[3] <= 128 and rb[3] < rb[4] < 1024 < rb[5]
    assert all(rows_of(f)[2] == 1 and rows_of(f)[1] <= 15 for n, f in want.items() if n.startswith("6-"))
    # a, b: the device writer's files, and the index over them where they lie
    got = {}
    for s, (b, hs, nfiles) in enumerate(sets):
        w = put.DeviceHSTableWriter(hs, 1, put.DeviceHSTableWriter.arena_bytes(hs, int(b.len.sum()), b.n))
        try:
            feed(w, b)
            w.close()
            files = w.files()
            got.update({"%d-%s" % (s, f): data for f, data in files.items()})
            ix = HSTableIndex.from_resident(w)
            try:
                assert ix.file_status == {f: 0 for f in files} and len(files) == nfiles, s
                assert ix.entries == b.n, s
            finally:
                ix.close()
        finally:
            w.free()
    assert_same_files(got, want)
    # c: the files without offset array and footer, recovered in one call
    torn = {n: f[:rows_of(f)[0]] for n, f in got.items()}
    out, rep = rec.recover_files(torn)
    assert sorted(out) == sorted(torn)
    for n, f in torn.items():
        st, model, mrep = R.recover(f, orc, "reference")
        r = rep[n]
        assert st == 0 and r.status == 0, n
        assert out[n] == model, n
        assert (r.entries_walked, r.rows_kept, r.entries_invalid, r.offset, r.footer_flags) == \
            (mrep["walked"], mrep["kept"], mrep["invalid"], mrep["offset"], mrep["flags"]), n
        assert model == want[n], n                     # the entries are whole: recovery gives the file back


# ------------------------------------------------------------- 7: refusals
def test_refused_append_leaves_no_trace(gpu):
    from kingdb_amd import _lib, put
    rng = np.random.default_rng(66)
    hs = 16384
    first = Batch([int(x) for x in rng.integers(26, 301, 90)], rng=rng)
    big = Batch([int(x) for x in rng.integers(26, 301, 400)], rng=rng)       # ~65 KB of entries
    last = Batch([int(x) for x in rng.integers(26, 301, 20)], rng=rng)
    want = host_files([first, last], hs)
    arena = 56 << 10                                   # three files of `first` and `last` fit, `big` does not
    assert int(first.len.sum()) + int(last.len.sum()) + 3 * 8400 + 2 * 15 * 110 < arena < int(big.len.sum())
    w = put.DeviceHSTableWriter(hs, 1, arena)
    try:
        feed(w, first)
        with pytest.raises(_lib.HipError, match="EINVAL"):
            feed(w, big)
        feed(w, last)
        w.close()
        assert_same_files(w.files(), want)
        # a fresh directory in the same arena: ids and timestamps from 1 again
        w.reset()
        feed(w, first)
        w.close()
        once = w.files()
        w.reset()
        for b in (first, last):
            feed(w, b)
        w.close()
        assert_same_files(w.files(), want)
        assert_same_files(once, host_files([first], hs))
    finally:
        w.free()


# ------------------------------------------------------------- 8: the index in place
@pytest.mark.parametrize("name", ["xx", "murmur"])
def test_index_over_resident_files(gpu, getkeys, name):
    from kingdb_amd import put
    from kingdb_amd.index import HSTableIndex
    s = getkeys[name]
    puts, hs, ht = s["puts"], s["hstable_size"], s["hash_type"]
    w = put.DeviceHSTableWriter(hs, ht, put.DeviceHSTableWriter.arena_bytes(hs, put.entries_bound(puts), len(puts)))
    try:
        for i in range(0, len(puts), 50):
            b, n = put.put_entries_device(puts[i:i + 50], ht)
            try:
                w.append_batch(b, n)
            finally:
                b.free()
        w.close()
        files = w.files()
        assert_same_files(files, put.write_hstables(puts, hs, ht, 50))
        keys = s["keys"] + [b"absent-1", b"absent%010d" % 2, b"absent%0300d" % 3]
        ref = HSTableIndex(files, ht)
        try:
            want_get = ref.get(keys)
            want_scan = ref.scan()
        finally:
            ref.close()
        ix = HSTableIndex.from_resident(w)
        try:
            assert ix.file_status == {f: 0 for f in files}
            assert ix.entries == len(puts)
            assert ix.get(keys) == want_get
            assert ix.scan() == want_scan
        finally:
            ix.close()
        # the index is gone, the files are the writer's still
        assert_same_files(w.files(), files)
    finally:
        w.free()


# ------------------------------------------------------------- 9: compaction on the device
@pytest.mark.parametrize("batch", [16, 65536])
@pytest.mark.parametrize("name", ["xx", "murmur"])
def test_compaction_on_the_device(gpu, getkeys, name, batch):
    from kingdb_amd.index import HSTableIndex
    s = getkeys[name]
    hs = 64 << 10
    src = HSTableIndex(s["files"], s["hash_type"])
    w = None
    try:
        live = src.scan()
        assert all(st == 0 for _, st, _ in live)
        want = src.compacted(hs, batch)
        w = src.compacted_device(hs, batch)
        assert_same_files(w.files(), want)
        ix = HSTableIndex.from_resident(w)
        try:
            assert set(ix.file_status.values()) == {0}
            assert ix.entries == len(live)
            got = ix.scan()
            assert len(got) == len(live)
            assert {(k, v) for k, _, v in got} == {(k, v) for k, _, v in live}
            assert [v for _, v in ix.get([k for k, _, _ in live])] == [v for _, _, v in live]
        finally:
            ix.close()
    finally:
        src.close()
        if w is not None:
            w.free()
