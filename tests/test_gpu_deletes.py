"""GPU: deletes through the put path and both writers (csrc/put.hip,
include/kdb_ops.h, kingdb_amd/put.py).

Expectations come from the reference: tests/golden/deletes.npz holds the files
it wrote for streams of puts and deletes and the codes its own Database::Get
returned, before and after a recovery (tests/golden/make_golden_deletes.py);
tests/test_deletes_model.py pins the Python models used here to the same
fixture.
"""
import numpy as np
import pytest

import deletes_fixture as D
import index_model as M
import scan_model as S
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture():
    return D.load()


def key_hash(orc, hash_type):
    return orc.xxh64 if hash_type == 1 else orc.murmur3_64


def delete_bytes(orc, key: bytes, hashed: int = 0) -> bytes:
    """The delete entry of `key`: the reference's with hashed = 0."""
    return orc.entry_header(0, 0x9, len(key), 0, 0, 0, hashed) + key


def raw_batch(entry: str, keys, vals, chunks, ops=None, flags=0, hash_type=1, values_null=False):
    """One call of kdb_put_ops_batch (entry "ops") or kdb_put_entries_batch
    ("entries") on explicit arrays, the scratch sized by kdb_put_scratch_bytes
    for exactly this batch: the eight outputs as host arrays."""
    from kingdb_amd import _lib
    from kingdb_amd.lz4 import DeviceBuffer
    L = _lib.load()
    n = len(keys)
    klen = np.array([len(k) for k in keys], np.uint32)
    vlen = np.array([len(v) for v in vals], np.uint64)
    koff, voff = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    koff[1:] = np.cumsum(klen[:-1].astype(np.uint64))
    voff[1:] = np.cumsum([len(v) for v in vals][:-1])
    pf = np.zeros(n + 1, np.uint32)
    pf[1:] = np.cumsum([len(c) for c in chunks])
    clen = np.array([c for ch in chunks for c in ch], np.uint32)
    kbuf, vbuf = np.frombuffer(b"".join(keys), np.uint8), np.frombuffer(b"".join(vals), np.uint8)
    nparts, raw = len(clen), len(vbuf)
    sb = int(L.kdb_put_scratch_bytes(n, nparts, raw))
    cap = raw + int(klen.sum()) + n * 128 + (raw // 65536 + n + 1) * 16 + 64
    bufs = []

    def dev(arr=None, nbytes=0):
        b = DeviceBuffer(max(arr.nbytes if arr is not None else nbytes, 8))
        bufs.append(b)
        if arr is not None and arr.nbytes:
            b.upload(arr)
        elif arr is None:
            b.memset(0)
        return b

    try:
        d_k, d_koff, d_klen, d_voff, d_vlen, d_pf = (dev(a) for a in (kbuf, koff, klen, voff, vlen, pf))
        d_v = None if values_null else dev(vbuf)
        d_cl = dev(clen) if nparts else None
        d_op = dev(np.array(ops, np.uint8)) if ops is not None else None
        d_scr, d_ent = dev(nbytes=sb), dev(nbytes=cap)
        o = {name: dev(nbytes=w * n) for name, w in (("entry_off", 8), ("entry_len", 4), ("hashed", 8), ("crc", 4),
                                                    ("kind", 4), ("status", 4))}
        d_total = dev(nbytes=8)
        L.kdb_lz4_stream_sync(None)
        tail = (d_k.ptr, d_koff.ptr, d_klen.ptr, d_v.ptr if d_v else None, d_voff.ptr, d_vlen.ptr, d_pf.ptr,
                d_cl.ptr if d_cl else None, nparts, int(clen.max()) if nparts else 0, n, hash_type, d_scr.ptr, sb, raw,
                d_ent.ptr, o["entry_off"].ptr, o["entry_len"].ptr, d_total.ptr, o["hashed"].ptr, o["crc"].ptr,
                o["kind"].ptr, o["status"].ptr)
        if entry == "ops":
            rc = L.kdb_put_ops_batch(None, d_op.ptr if d_op else None, flags, *tail)
        else:
            assert ops is None and flags == 0
            rc = L.kdb_put_entries_batch(None, *tail)
        _lib.check(rc, entry)
        _lib.check(L.kdb_lz4_stream_sync(None), "sync")
        total = int(d_total.download(8, dtype=np.uint64)[0])
        assert total <= cap
        dt = {"entry_off": np.uint64, "entry_len": np.uint32, "hashed": np.uint64, "crc": np.uint32,
              "kind": np.uint32, "status": np.int32}
        out = {k: b.download(b.nbytes if n else 0, dtype=dt[k])[:n] for k, b in o.items()}
        out["total"] = total
        out["entries"] = d_ent.download(total).tobytes() if total else b""
        return out
    finally:
        for b in bufs:
            b.free()


def entry_of(out, i: int) -> bytes:
    o = int(out["entry_off"][i])
    return out["entries"][o:o + int(out["entry_len"][i])]


# ------------------------------------------------------------- 1. the reference's files
@pytest.mark.parametrize("batch", [None, 1, 7])
@pytest.mark.parametrize("writer", ["host", "device"])
@pytest.mark.parametrize("name", ["mixed", "lengths", "cuts", "murmur"])
def test_files_equal_the_reference(gpu, fixture, orc, name, writer, batch):
    from kingdb_amd import put
    s = fixture[0][name]
    write = put.write_hstables if writer == "host" else put.write_hstables_device
    files = write(s["items"], s["hstable_size"], s["hash_type"], batch)
    assert sorted(files) == sorted(s["files"])
    for f in files:
        assert files[f] == s["files"][f], (name, writer, batch, f)
    ndel = 0
    for f in files.values():
        for _, e in D.delete_entries(f):
            ndel += 1
            assert f[e.offset:e.value_at] == delete_bytes(orc, e.key)
    assert ndel == sum(1 for it in s["items"] if put.is_delete(it)) > 0


# ------------------------------------------------------------- 2. batches of deletes alone
@pytest.mark.parametrize("n", [1, 300])
@pytest.mark.parametrize("hash_type", [1, 0])
def test_delete_only_batch(gpu, orc, n, hash_type):
    """nparts = 0, raw_bytes = 0, values = NULL, kdb_put_scratch_bytes(n, 0, 0):
    keys of 1 to 700 bytes, so both entry kernels run when n = 300."""
    from kingdb_amd import put
    rng = np.random.default_rng(n)
    keys = [rng.integers(0, 256, 1 + (i * 37) % 700, dtype=np.uint8).tobytes() for i in range(n)]
    h = key_hash(orc, hash_type)
    out = raw_batch("ops", keys, [b""] * n, [[]] * n, ops=[1] * n, hash_type=hash_type, values_null=True)
    want = [delete_bytes(orc, k) for k in keys]
    assert [entry_of(out, i) for i in range(n)] == want
    assert out["total"] == sum(map(len, want)) == len(out["entries"])
    assert list(out["entry_off"]) == list(np.cumsum([0] + [len(w) for w in want[:-1]]))
    assert [int(x) for x in out["hashed"]] == [h(k) for k in keys]
    assert not out["crc"].any() and not out["kind"].any() and not out["status"].any()
    # and through the Python layer
    r = put.put_entries([(k, put.DELETE) for k in keys], hash_type)
    assert [r.entry(i) for i in range(n)] == want and not r.status.any() and not r.crc.any()


# ------------------------------------------------------------- 3. refused items
def test_refused_deletes_leave_their_neighbours_alone(gpu, orc):
    from kingdb_amd import put
    a, c = bytes(range(200)), b"z" * 3000
    keys = [b"put-a", b"bad-value-len", b"del-b", b"bad-chunk", b"bad-op-byte", b"k" * 600, b"put-c"]
    vals = [a, b"12345", b"", b"", b"payload", b"", c]
    chunks = [[len(a)], [], [], [0], [7], [], [len(c)]]
    ops = [0, 1, 1, 1, 2, 1, 0]
    out = raw_batch("ops", keys, vals, chunks, ops=ops)
    good = put.put_entries([(keys[0], a), (keys[2], put.DELETE), (keys[5], put.DELETE), (keys[6], c)])
    assert list(out["status"]) == [0, -1, 0, -1, -1, 0, 0]
    assert [int(out["entry_len"][i]) for i in (1, 3, 4)] == [0, 0, 0]
    for j, i in enumerate((0, 2, 5, 6)):
        assert entry_of(out, i) == good.entry(j), i
        assert int(out["hashed"][i]) == int(good.hashed[j]) and int(out["crc"][i]) == int(good.crc[j])
        assert int(out["kind"][i]) == int(good.kind[j])
    assert out["total"] == int(good.entry_len.sum()) == len(good.entries)
    assert out["entries"] == good.entries.tobytes()


# ------------------------------------------------------------- 4. op = NULL
def test_null_ops_is_the_put_path(gpu):
    """All eight outputs of kdb_put_ops_batch(op = NULL, flags = 0) equal
    kdb_put_entries_batch's, on the first 200 puts of the config-5 stream."""
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_golden_put import decode_stream
    z = load_golden("hstable_streams.npz")
    puts = decode_stream(z["small__stream"].tobytes())[:200]
    keys, vals, chunks = [p[0] for p in puts], [p[1] for p in puts], [p[2] for p in puts]
    x = raw_batch("entries", keys, vals, chunks)
    y = raw_batch("ops", keys, vals, chunks)
    w = raw_batch("ops", keys, vals, chunks, ops=[0] * len(puts), flags=1)      # all puts: the flag changes nothing
    assert x["total"] > 200 * 100 and not x["status"].any()
    for other in (y, w):
        for name in ("entries", "entry_off", "entry_len", "total", "hashed", "crc", "kind", "status"):
            assert np.array_equal(x[name], other[name]), name


# ------------------------------------------------------------- 5. KDB_OPS_DELETE_HASHED
def test_delete_hashed_changes_the_hash_and_the_crc8_only(gpu, fixture, orc):
    from kingdb_amd import put
    for name in ("lengths", "murmur"):
        s = fixture[0][name]
        h = key_hash(orc, s["hash_type"])
        a = put.put_entries(s["items"], s["hash_type"])
        b = put.put_entries(s["items"], s["hash_type"], delete_hashed=True)
        for arr in ("entry_off", "entry_len", "hashed", "crc", "kind", "status"):
            assert np.array_equal(getattr(a, arr), getattr(b, arr)), arr
        ndel = 0
        for i, it in enumerate(s["items"]):
            x, y = a.entry(i), b.entry(i)
            if not put.is_delete(it):
                assert x == y
                continue
            ndel += 1
            k = it[0]
            hl = len(x) - len(k)
            assert x == delete_bytes(orc, k) and y == delete_bytes(orc, k, h(k))
            diff = {j for j in range(len(x)) if x[j] != y[j]}
            assert diff <= {0} | set(range(hl - 8, hl)), (name, i, sorted(diff))
            assert y[hl - 8:hl] == h(k).to_bytes(8, "little")
        assert ndel >= 10


# ------------------------------------------------------------- 6. read back
def test_write_refresh_get_scan_compact(gpu, fixture, orc):
    from kingdb_amd import _lib, put
    from kingdb_amd import get as G
    from kingdb_amd.index import DELETED, HSTableIndex
    s = fixture[0]["mixed"]
    items, hs, ht = s["items"], s["hstable_size"], s["hash_type"]
    last = D.last_ops(s["ops"])
    live = [k for k in s["keys"] if last[k] is not None]
    more = [(k, put.DELETE) for k in live[::2]]
    w = put.DeviceHSTableWriter(hs, ht, put.DeviceHSTableWriter.arena_bytes(
        hs, put.entries_bound(items) + put.entries_bound(more), len(items) + len(more)))
    ix = w2 = None

    def append(batch):
        b, n = put.put_entries_device(batch, ht)
        try:
            w.append_batch(b, n)
            _lib.check(_lib.load().kdb_lz4_stream_sync(None), "sync")
        finally:
            b.free()

    try:
        for i in range(0, len(items), 64):
            append(items[i:i + 64])
        w.close()
        assert w.files() == s["files"]
        ix = HSTableIndex.from_resident(w)
        D.assert_codes(ix.get(s["keys"]), s["keys"], s["code"], s["len"], s["crc"], orc, "from_resident")
        # the scan lists exactly the keys whose last op is a put
        model = M.Model(s["files"], orc, ht)
        got = ix.scan()
        assert got == S.scan(model) and sorted(k for k, _, _ in got) == sorted(live)
        assert [(st, v) for _, st, v in got] == [(0, last[k]) for k, _, _ in got]
        # a compaction holds no delete entry and no deleted key
        w2 = ix.compacted_device(hs)
        ents = [e for f in w2.files().values() for e in G.read_hstable(f)]
        assert not any(e.is_delete for e in ents) and sorted(e.key for e in ents) == sorted(live)
        # more deletes in a further file
        append(more)
        w.close()
        assert ix.refresh() == len(more)
        gone = {k for k, _ in more}
        got = ix.get(s["keys"])
        for k, g, c in zip(s["keys"], got, s["code"]):
            if k in gone or c == D.REF_DELETE_ORDER:
                assert g == (DELETED, b""), k
            else:
                assert g == (0, last[k]), k
        assert sorted(k for k, _, _ in ix.scan()) == sorted(set(live) - gone)
    finally:
        if ix is not None:
            ix.close()
        if w2 is not None:
            w2.free()
        w.free()


# ------------------------------------------------------------- 7. recovery
def test_recovery_reference_and_hashed(gpu, fixture, orc):
    from kingdb_amd import put, recover
    from kingdb_amd.index import DELETED, NOTFOUND, HSTableIndex
    sets, torn = fixture
    s = sets["mixed"]
    ht, base = s["hash_type"], torn[0]["base"]
    assert base == sorted(s["files"])[-1]
    before = sum(len(M.parse_rows(s["files"][f])) for f in s["files"] if f != base)

    def codes_after(files, recovered):
        fs = dict(files)
        fs[base] = recovered
        ix = HSTableIndex(fs, ht)
        try:
            assert set(ix.file_status.values()) == {0}
            return ix.get(s["keys"]), len(M.parse_rows(recovered))
        finally:
            ix.close()

    # the reference's bytes: its recovery, its codes, the keys that come back included
    names = ["%08x" % (i + 1) for i in range(len(torn))]
    out, rep = recover.recover_files({n: s["files"][base][:t["cut"]] for n, t in zip(names, torn)})
    for i, (n, t) in enumerate(zip(names, torn)):
        assert rep[n].status == 0 and out[n] == t["recovered"], i
        got, rows = codes_after(s["files"], out[n])
        D.assert_codes(got, s["keys"], t["code"], t["len"], t["crc"], orc, f"torn {i}")
    # the same database with the key's hash in every delete header
    hashed = put.write_hstables(s["items"], s["hstable_size"], ht, delete_hashed=True)
    assert sorted(hashed) == sorted(s["files"]) and [len(hashed[f]) for f in hashed] == [len(s["files"][f]) for f in hashed]
    out, rep = recover.recover_files({n: hashed[base][:t["cut"]] for n, t in zip(names, torn)})
    back = 0
    for i, (n, t) in enumerate(zip(names, torn)):
        assert rep[n].status == 0
        got, rows = codes_after(hashed, out[n])
        assert rows == len(M.parse_rows(t["recovered"]))
        # one row per op: the ops that survive the cut are a prefix of the stream, and every one is reachable
        last = D.last_ops(s["ops"][:before + rows])
        for k, g, c in zip(s["keys"], got, t["code"]):
            if k not in last:
                assert g == (NOTFOUND, b""), (i, k)
            elif last[k] is None:
                assert g == (DELETED, b""), (i, k)
                back += c == D.REF_OK
            else:
                assert g == (0, last[k]), (i, k)
    assert back > 0              # keys the reference's recovery brings back stay deleted here
