"""GPU: the put path's multipart policy on ragged chunkings (csrc/put.hip
put_policy_kernel, put_entry_small_kernel, put_entry_kernel; kingdb_amd/put.py).

tests/golden/hstable_ragged.npz holds streams the reference wrote
(tests/golden/make_golden_ragged.py): values cut so that a first or middle
chunk already looks last and later chunks are dropped, the disable rule on a
first, middle and last chunk, empty chunks first, in the middle and last,
calls the reference refuses, entries never finished, and multipart entries
across a file cut.  tests/put_policy_model.py names these classes and
tests/test_write_path.py::test_put_branch_table counts them.

The judge is the oracle (oracle/hstable.py), which the CPU tests of
tests/test_write_path.py pin to the reference's files on these very streams
and on the fuzz streams below.  Two things the batch API promises differ from
what the reference leaves on disk, and for a stream that has
them the oracle writer is fed the same contract (batch_contract=True) instead
of being compared with the reference's files:
  * a put with a refused call returns status -1, entry_len 0 and no bytes,
    where the reference keeps the parts it wrote before the refusal;
  * a value whose first chunks are empty makes one entry, where the reference
    also leaves an unfinished entry (header, key, zeros) per empty first call.
ragged_ok and ragged_cut have neither and are compared with the reference's
files byte for byte; ragged_odd has both.  Every comparison is exact.
"""
import numpy as np
import pytest

import put_fuzz
import put_policy_model as model
from test_write_path import RAGGED, REFUSED, oracle_writer

pytestmark = pytest.mark.gpu

_expected = {}


def expected(orc, name, puts, hs, ht):
    """The oracle under the batch API's contract, once per (stream, hash):
    (per put: entry bytes or None, hash, kind, crc), the files."""
    if (name, ht) not in _expected:
        w, files = oracle_writer(orc, puts, hs, ht, batch_contract=True)
        per = []
        refused = {p for p, _ in w.refused}
        for i, (ents, (k, v, ch)) in enumerate(zip(w.dense_by_put(), puts)):
            assert len(ents) == (0 if i in refused else 1)
            crc = orc.put_value(k, v, ch, keep_going=True)["crc"]
            per.append((ents[0] + (crc,)) if ents else None)
        _expected[name, ht] = (tuple(per), files)
    return _expected[name, ht]


def assert_batches(r_batches, per, puts):
    """put_entries results, batch by batch, against the oracle's per-put view."""
    i = 0
    for r in r_batches:
        n = len(r.entry_len)
        assert int(r.entry_len.astype(np.uint64).sum()) == len(r.entries)          # the total
        off = 0
        for j in range(n):
            want = per[i + j]
            assert int(r.entry_off[j]) == off, i + j
            if want is None:                                     # refused: status -1, no bytes
                assert (int(r.status[j]), int(r.entry_len[j])) == (-1, 0), i + j
                continue
            e, h, k, crc = want
            assert int(r.status[j]) == 0, i + j
            assert int(r.entry_len[j]) == len(e), (i + j, puts[i + j][2])
            assert int(r.kind[j]) == k, (i + j, puts[i + j][2])
            assert int(r.hashed[j]) == h, i + j
            assert int(r.crc[j]) == crc, (i + j, puts[i + j][2])
            assert r.entry(j) == e, (i + j, len(puts[i + j][1]), puts[i + j][2])
            off += len(e)
        i += n
    assert i == len(per)


# ------------------------------------------------------------- 1. the fixture through put_entries
@pytest.mark.parametrize("batch", [None, 1, 7])
@pytest.mark.parametrize("ht", [1, 0], ids=["xxhash", "murmur"])
@pytest.mark.parametrize("name", ["ragged_ok", "ragged_odd"])
def test_put_entries_match_oracle(gpu, orc, name, ht, batch):
    from kingdb_amd.put import put_entries
    puts, hs, _, _ = RAGGED[name]
    per, _ = expected(orc, name, puts, hs, ht)
    step = batch or len(puts)
    assert_batches([put_entries(puts[i:i + step], ht) for i in range(0, len(puts), step)], per, puts)
    if name == "ragged_odd":
        assert [p for p, _ in REFUSED[name]] == [i for i, w in enumerate(per) if w is None]
    else:
        assert None not in per


# ------------------------------------------------------------- 2. the files of both writers
@pytest.mark.parametrize("writer", ["host", "device"])
@pytest.mark.parametrize("name", ["ragged_ok", "ragged_cut"])
def test_files_equal_the_reference(gpu, name, writer):
    """Byte for byte the reference's files, the footer's padding flag and the
    missing offset array of a file with an unfinished entry included."""
    from kingdb_amd import put
    puts, hs, ht, files = RAGGED[name]
    write = put.write_hstables if writer == "host" else put.write_hstables_device
    got = write(puts, hs, ht)
    assert list(got) == list(files)
    for f in files:
        assert got[f] == files[f], f
    # (what the fixture must hold for that: HSTableFooter, storage/format.h:480-493)
    import struct
    from oracle import hstable
    closed = [f for f in files.values() if struct.unpack("<Q", f[-12:-4])[0] == hstable.MAGIC]
    assert any(struct.unpack("<I", f[-32:-28])[0] == 1 for f in closed)
    if name == "ragged_cut":
        assert len(files) > 1 and len(closed) < len(files)


@pytest.mark.parametrize("batch", [None, 1, 7])
@pytest.mark.parametrize("writer", ["host", "device"])
@pytest.mark.parametrize("name", ["ragged_ok", "ragged_odd", "ragged_cut"])
def test_files_equal_the_oracle_in_batches(gpu, orc, name, writer, batch):
    """The same files as the oracle writer given the same write-buffer flushes
    and the batch API's contract (module docstring): for ragged_odd that is not
    the reference's file, which also holds the parts written before a refusal
    and the unfinished entries of empty first chunks."""
    from kingdb_amd import put
    puts, hs, ht, _ = RAGGED[name]
    _, exp = oracle_writer(orc, puts, hs, ht, batch, batch_contract=True)
    write = put.write_hstables if writer == "host" else put.write_hstables_device
    got = write(puts, hs, ht, batch)
    assert list(got) == list(exp)
    for f in exp:
        assert got[f] == exp[f], (f, len(got[f]), len(exp[f]))


# ------------------------------------------------------------- 3. the per-call path
@pytest.mark.parametrize("name", ["ragged_ok", "ragged_odd", "ragged_cut"])
def test_flush_parts_on_ragged_calls(gpu, orc, name):
    """csrc/flush.hip, the per-call implementation of the same policy: every
    PutPartValidSize call of the stream, one client thread, in batches of 50."""
    import oracle
    from kingdb_amd.flush import flush_parts
    puts = RAGGED[name][0]
    calls = []
    for k, v, ch in puts:
        off = 0
        for c in ch:
            calls.append((0, k, v[off:off + c], off, len(v)))
            off += c
    st = oracle.PutState()
    want = [oracle.put_part(orc, st, k, chunk, off, size) for _, k, chunk, off, size in calls]
    states, got = {}, []
    for i in range(0, len(calls), 50):
        res, states = flush_parts(calls[i:i + 50], states)
        got += res
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert g["rc"] == w["rc"], j
        for f in ("mode", "occ", "svc", "crc") + (("chunk_final",) if w["rc"] == 0 else ()):
            assert g[f] == w[f], (j, f, calls[j][3], len(calls[j][2]), calls[j][4])
    assert sorted(j for j, w in enumerate(want) if w["rc"] != 0) == sorted(
        sum(len(ch) for _, _, ch in puts[:p]) + c for p, c in REFUSED[name])


# ------------------------------------------------------------- 4. read back what was written
def test_ragged_ok_read_back(gpu, orc):
    """HSTableIndex over the device-written files of ragged_ok: Get of every
    key returns the last value put, the scan every live entry in the
    reference's iterator order (tests/scan_model.py over the reference's
    files).  The ground truth is the input values; nothing is approximate."""
    import index_model as M
    import scan_model as S
    from kingdb_amd import put
    from kingdb_amd.index import HSTableIndex
    puts, hs, ht, files = RAGGED["ragged_ok"]
    last = {}
    for k, v, _ in puts:
        last[k] = v
    assert len(last) < len(puts)                                 # a key put twice
    got_files = put.write_hstables_device(puts, hs, ht)
    ix = HSTableIndex(got_files, ht)
    try:
        assert set(ix.file_status.values()) == {0}
        keys = sorted(last)
        assert ix.get(keys, verify=0) == [(0, last[k]) for k in keys]
        assert ix.get(keys, verify=2) == [(0, last[k]) for k in keys]
        want = S.scan(M.Model(files, orc, ht), 0)
        assert sorted(k for k, _, _ in want) == keys
        assert all(st == 0 and v == last[k] for k, st, v in want)
        assert ix.scan(verify=0) == want
    finally:
        ix.close()


# ------------------------------------------------------------- 5. the seeded ragged fuzz
@pytest.mark.parametrize("seed", put_fuzz.SEEDS)
def test_fuzz_put_entries(gpu, orc, seed):
    """About 200 ragged puts per seed (tests/put_fuzz.py): every output equals
    the oracle's under the batch API's contract.  The oracle is pinned to the
    reference on the same values by
    tests/test_write_path.py::test_ragged_fuzz_oracle_equals_reference.  The
    seeds were picked on the CPU so that each reaches every class."""
    from kingdb_amd.put import put_entries
    puts = put_fuzz.stream(orc, seed)
    tab = model.table(orc, puts)
    print({c: k for c, k in tab.items()})
    assert [c for c in model.CLASSES if tab[c] == 0] == []
    for ht in (1, 0):
        per, _ = expected(orc, "fuzz%d" % seed, puts, 32 << 20, ht)
        assert_batches([put_entries(puts, ht)], per, puts)
    per, _ = expected(orc, "fuzz%d" % seed, puts, 32 << 20, 1)
    assert_batches([put_entries(puts[i:i + 23], 1) for i in range(0, len(puts), 23)], per, puts)


# ------------------------------------------------------------- 6. the 512-byte line and crc_copy
def frame_values(orc):
    """Compressible values of several shapes with their frame lengths (the
    frame is kept: it is no longer than the value, database.cc:196-209)."""
    pool = orc.g1_pieces(40).tobytes()
    out = []
    for v in (b"a" * 300, (b"abcdefgh" * 60)[:450], pool[:50] * 7, pool[100:137] * 11 + b"xyz"):
        f = len(orc.frame(v))
        assert f <= len(v) and f < 400
        out.append((v, f))
    return out


def test_small_entry_line(gpu, orc):
    """put_entry_small_kernel takes single-chunk entries of at most 512 bytes
    of key + chunk_final, put_entry_kernel the rest: key + chunk_final of 511,
    512 and 513 bytes with chunk_final a frame, the disable header + raw
    bytes, and empty, and deletes of keys of 511, 512 and 513 bytes, all in one
    batch so that both kernels write into one entry stream."""
    from kingdb_amd.put import DELETE, put_entries
    rng = np.random.default_rng(6)
    items, modes = [], []

    def key(n, tag):
        return (tag + rng.integers(0, 256, n, dtype=np.uint8).tobytes())[:n]

    for total in (511, 512, 513):
        for v, f in frame_values(orc):                                   # a frame of f bytes
            items.append((key(total - f, b"f"), v, None))
            modes.append(0)
        for n in (5, 100, 300):                                          # 8 zero bytes + n raw bytes
            items.append((key(total - 8 - n, b"d"), rng.integers(0, 256, n, dtype=np.uint8).tobytes(), None))
            modes.append(1)
        items.append((key(total, b"e"), b"", None))                      # an empty value
        modes.append(2)
        items.append((key(total, b"x"), DELETE))
        modes.append(None)
    order = rng.permutation(len(items))
    items, modes = [items[i] for i in order], [modes[i] for i in order]
    for ht in (1, 0):
        r = put_entries(items, ht)
        assert (r.status == 0).all() and (r.kind == 0).all()
        hashf = orc.xxh64 if ht == 1 else orc.murmur3_64
        off, seen = 0, set()
        for i, (it, m) in enumerate(zip(items, modes)):
            k = it[0]
            if m is None:
                want, crc = orc.entry_header(0, 0x9, len(k), 0, 0, 0, 0) + k, 0
                seen.add(("delete", len(k)))
            else:
                pv = orc.put_value(k, it[1])
                (occ, final), = pv["parts"]
                assert occ == 0 and (final[:8] == bytes(8)) == (m == 1) and (len(final) == 0) == (m == 2)
                want = orc.entry_header(pv["crc"], 0x8, len(k), len(it[1]), pv["svc"], 0, hashf(k)) + k + final
                crc = pv["crc"]
                seen.add((m, len(k) + len(final)))
            assert int(r.entry_off[i]) == off and int(r.entry_len[i]) == len(want), i
            assert r.entry(i) == want, (i, m, len(k))
            assert int(r.crc[i]) == crc and int(r.hashed[i]) == hashf(k), i
            off += len(want)
        assert off == len(r.entries)
        assert seen == {(m, t) for m in (0, 1, 2, "delete") for t in (511, 512, 513)}


def test_crc_copy_lengths_and_alignments(gpu, orc):
    """crc_copy (the small kernel's copy with the CRC folded in, 16 dwords in
    flight): keys and raw value stretches of n bytes for n >> 2 in {0, 1, 15,
    16, 17, 31, 32, 33} and n & 3 in 0..3, keys and values packed back to back
    so that the sources start at every alignment mod 4.  CRC32C against
    orc.crc32c over key || chunk_final, the copied bytes against the input."""
    from kingdb_amd.put import put_entries
    rng = np.random.default_rng(7)
    lens = [4 * q + r for q in (0, 1, 15, 16, 17, 31, 32, 33) for r in range(4)]
    klens = [n for n in lens if n]
    puts = []
    for kl in klens:
        for vl in lens:
            # random bytes: the frame is longer than the value, so chunk_final is
            # 8 zero bytes and the vl bytes themselves (an empty value: nothing)
            puts.append((rng.integers(0, 256, kl, dtype=np.uint8).tobytes(),
                         rng.integers(0, 256, vl, dtype=np.uint8).tobytes(), None))
    order = rng.permutation(len(puts))
    puts = [puts[i] for i in order]
    koff = np.cumsum([0] + [len(k) for k, _, _ in puts[:-1]])
    voff = np.cumsum([0] + [len(v) for _, v, _ in puts[:-1]])
    assert {int(x) % 4 for x in koff} == {0, 1, 2, 3} == {int(x) % 4 for x in voff}
    assert max(len(k) + 8 + len(v) for k, v, _ in puts) <= 512           # all the small kernel's
    r = put_entries(puts, 1)
    assert (r.status == 0).all() and (r.kind == 0).all()
    seen = set()
    for i, (k, v, _) in enumerate(puts):
        final = bytes(8) + v if v else b""
        e = r.entry(i)
        hl = len(e) - len(k) - len(final)
        assert hl == len(orc.entry_header(0, 0x8, len(k), len(v), len(final), 0, 0)), i
        assert e[hl:hl + len(k)] == k, (i, len(k), len(v))
        assert e[hl + len(k):] == final, (i, len(k), len(v))
        assert int(r.crc[i]) == orc.crc32c(k + final), (i, len(k), len(v))
        assert e[:hl] == orc.entry_header(int(r.crc[i]), 0x8, len(k), len(v), len(final), 0, orc.xxh64(k)), i
        seen.add((len(k), len(v)))
    assert seen == {(a, b) for a in klens for b in lens}
