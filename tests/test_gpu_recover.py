"""GPU: files without a usable footer recovered on the device
(kdb_hstable_recover_files, kingdb_amd/recover.py, HSTableIndex(recover=...)).

  * every case of tests/golden/recover.npz, all of them separate files of ONE
    call: the recovered bytes are the reference's, removed files report why;
  * an index over damaged files with recover="reference" answers get and scan
    as an index over the reference-recovered files does;
  * `content` scope, the tile shapes and the decoy file against the model
    (tests/recover_model.py, pinned to the reference by test_recover_model.py);
    the files come from the project's own writer with the footers cut off,
    but for the 26-byte stride, which the writer cannot make;
  * a slot below kdb_hstable_recover_bound is refused, and no recovered file
    exceeds it.
"""
import struct

import numpy as np
import pytest

import recover_model as R
from conftest import load_golden
from kingdb_amd import _lib
from kingdb_amd import get as G
from kingdb_amd import put as P
from kingdb_amd import recover as rec
from kingdb_amd.index import HSTableIndex
from kingdb_amd.lz4 import DeviceBuffer

pytestmark = pytest.mark.gpu

TILE = 4096


def run(files: list, scope: str):
    """One kdb_hstable_recover_files call over `files`: [(Report, bytes | None)]."""
    size = np.array([len(f) for f in files], np.uint64)
    cap = np.array([rec.bound(len(f)) for f in files], np.uint64)
    off, total = rec.layout(size, cap)
    buf = np.zeros(total + 64, np.uint8)
    for f, o in zip(files, off):
        buf[int(o):int(o) + len(f)] = np.frombuffer(f, np.uint8)
    dev = DeviceBuffer(total + 64)
    try:
        dev.upload(buf)
        reports = rec.recover_resident(dev.ptr, off, size, cap, scope)
        data = dev.download(total)
    finally:
        dev.free()
    out = []
    for f, o, c, r in zip(files, off, cap, reports):
        assert r.size <= int(c)
        if r.status == 0:
            out.append((r, data[int(o):int(o) + r.size].tobytes()))
        else:
            # a file the reference removes is left as it was
            assert data[int(o):int(o) + len(f)].tobytes() == f
            out.append((r, None))
    return out


def check_against_model(files, got, orc, scope):
    for i, (f, (r, out)) in enumerate(zip(files, got)):
        st, want, rep = R.recover(f, orc, scope)
        assert r.status == st, i
        if st != 0:
            assert out is None
            continue
        assert out == want, i
        assert (r.entries_walked, r.rows_kept, r.entries_invalid, r.offset, r.footer_flags) == \
            (rep["walked"], rep["kept"], rep["invalid"], rep["offset"], rep["flags"]), i


@pytest.fixture(scope="module")
def fixture():
    z = load_golden("recover.npz")
    return z, R.load_cases(z)


@pytest.fixture(scope="module")
def recovered_reference(gpu, fixture):
    return run([f for _, f, _ in fixture[1]], "reference")


def test_fixture_cases_equal_the_reference(fixture, recovered_reference, orc):
    z, cases = fixture
    for (name, f, want), (r, out) in zip(cases, recovered_reference):
        if want is None:
            assert out is None and r.status == (rec.LARGE if "large_type" in name else rec.NOENTRY), name
            continue
        size, crc, oi, tail = want
        assert r.status == 0 and (r.size, r.offset) == (size, oi), name
        assert out[:oi] == f[:oi] and out[oi:] == tail and orc.crc32c(out) == crc, name
        if name.startswith("sessions/") and name.endswith("/footer_crc_flipped"):
            assert out == z["base__" + "_".join(name.split("/")[:2])].tobytes(), name
    check_against_model([f for _, f, _ in cases], recovered_reference, orc, "reference")


def test_content_scope_equals_the_model(gpu, fixture, orc):
    files = [f for n, f, _ in fixture[1] if n.startswith("multipart/")]
    got = run(files, "content")
    check_against_model(files, got, orc, "content")
    assert sum(r.rows_kept for r, _ in got) > sum(R.recover(f, orc, "reference")[2]["kept"] for f in files)


def database(z, db):
    return {str(n).split("_")[1]: z[f"base__{n}"].tobytes() for n in z["base_names"] if str(n).startswith(db + "_")}


@pytest.mark.parametrize("db,cases", [("sessions", ["00000003/cut_header24", "00000001/torn4"]),
                                      ("sessions", ["00000003/cut_8202", "00000001/footer_crc_flipped"]),
                                      ("multipart", ["00000002/torn35", "00000001/flip_entry_header"])])
def test_index_over_damaged_files_answers_as_over_the_reference_recovered(gpu, fixture, db, cases):
    z, all_cases = fixture
    base = database(z, db)
    by_name = {n: (f, want) for n, f, want in all_cases}
    damaged, recovered = dict(base), dict(base)
    for c in cases:
        f, want = by_name[f"{db}/{c}"]
        name = c.split("/")[0]
        damaged[name] = f
        if want is None:
            del recovered[name]
        else:
            recovered[name] = f[:want[2]] + want[3]
    keys = sorted({e.key for b in base.values() for e in G.read_hstable(b)}) + [b"absent-key"]
    plain = HSTableIndex(damaged)
    with_rec = HSTableIndex(damaged, recover="reference")
    ref = HSTableIndex(recovered)
    try:
        # recover=None is today's index: the damaged files stay out
        assert all(plain.file_status[c.split("/")[0]] == -1 for c in cases) and plain.recovered == {}
        assert set(ref.file_status.values()) == {0}
        for c in cases:
            name = c.split("/")[0]
            if name in recovered:
                assert with_rec.file_status[name] == 0 and with_rec.recovered[name].size == len(recovered[name])
            else:
                assert with_rec.file_status[name] == -1 and name not in with_rec.recovered
        assert with_rec.entries == ref.entries > plain.entries
        for verify in (0, 1):
            assert with_rec.get(keys, verify) == ref.get(keys, verify)
        assert with_rec.scan() == ref.scan()
        assert len(with_rec.scan()) > len(plain.scan())
    finally:
        for ix in (plain, with_rec, ref):
            ix.close()


def header_retyped(f: bytes, orc, filetype: int) -> bytes:
    b = bytearray(f)
    struct.pack_into("<I", b, 12, filetype)
    struct.pack_into("<I", b, 0, orc.crc32c(bytes(b[4:24])))
    return bytes(b)


@pytest.mark.parametrize("kind", ["large_type", "first_entry_broken"])
def test_index_after_a_new_layout_that_recovers_no_file(gpu, fixture, orc, kind):
    """The oldest file keeps its footer magic with a flipped footer CRC, so its
    slot is sized for recovery only after the first load and every later file
    moves; and recovery gives the file up (large type; no entry walked).  The
    index must answer from the new layout: as an index over the other files."""
    base = database(fixture[0], "sessions")
    name = sorted(base)[0]
    f = bytearray(base[name])
    f[-2] ^= 0x08
    if kind == "large_type":
        f = header_retyped(bytes(f), orc, 4)
    else:
        f[8192 + 6] ^= 0x02                     # the first entry's size_key: its header CRC-8 fails
    damaged = dict(base)
    damaged[name] = bytes(f)
    others = {k: v for k, v in base.items() if k != name}
    keys = sorted({e.key for b in base.values() for e in G.read_hstable(b)})
    plain, with_rec, ref = HSTableIndex(damaged), HSTableIndex(damaged, recover="reference"), HSTableIndex(others)
    try:
        assert with_rec.file_status[name] == -1 and with_rec.recovered == {}
        assert (with_rec.file_off[1:] > plain.file_off[1:]).all()          # the later files did move
        assert with_rec.entries == ref.entries == plain.entries
        for verify in (0, 1):
            assert with_rec.get(keys, verify) == ref.get(keys, verify)
        assert with_rec.scan() == ref.scan() and len(ref.scan()) > 0
    finally:
        for ix in (plain, with_rec, ref):
            ix.close()


def test_recover_files_returns_what_the_reference_leaves_on_disk(gpu, fixture, orc):
    z, cases = fixture
    by_name = {n: (f, want) for n, f, want in cases}
    good = z["base__sessions_00000002"].tobytes()
    files = {"00000001": by_name["sessions/00000001/torn4"][0],            # recovered
             "00000002": by_name["sessions/00000003/cut_8202"][0],         # removed: no entry
             "00000003": by_name["sessions/00000003/large_type_torn4"][0],  # removed: large type
             "00000004": bytes([good[0] ^ 1]) + good[1:-4],                 # bad header CRC: skipped, left as it is
             "00000005": good[:8192]}                                       # nothing behind the header block: the same
    out, rep = rec.recover_files(files)
    want = by_name["sessions/00000001/torn4"][1]
    assert out == {"00000001": files["00000001"][:want[2]] + want[3], "00000004": files["00000004"],
                   "00000005": files["00000005"]}
    assert [rep[n].status for n in sorted(files)] == [0, rec.NOENTRY, rec.LARGE, rec.BADHEADER, rec.BADHEADER]
    with pytest.raises(ValueError):
        rec.recover_files(files, "neither")


def test_undamaged_database_uploads_as_without_recover(gpu, fixture):
    base = database(fixture[0], "sessions")
    a, b = HSTableIndex(base), HSTableIndex(base, recover="content")
    try:
        assert (a.file_off == b.file_off).all() and (a.file_size == b.file_size).all()
        assert a.files.nbytes == b.files.nbytes and b.recovered == {} and a.file_status == b.file_status
        assert a.scan() == b.scan()
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ files of the project's own writer
def rnd(rng, n: int) -> bytes:
    return bytes(rng.integers(0, 256, n, dtype=np.uint8))


def entries_of(puts) -> bytes:
    """The file the project's writer leaves for `puts`, its offset array and footer cut off."""
    files = P.write_hstables(puts)
    assert len(files) == 1
    f = next(iter(files.values()))
    return f[:R.M.footer(f)[2]]


def ending_at(rng, end: int, head: list) -> bytes:
    """`head` and one more incompressible put, sized so that the entries end at byte `end`."""
    n = 1500
    for _ in range(4):
        f = entries_of(head + [(b"fit", rnd(rng, n))])
        if len(f) == end:
            return f
        n += end - len(f)
    raise AssertionError("could not size the last put")


def smallest_entries(orc, rng, head: bytes, count: int) -> bytes:
    """`count` entries of 26 to 40 bytes behind the header block `head`.  The
    writer cannot make them (a value it stores takes a frame header or its
    padding, so its smallest entry has 35 bytes): they are put together here,
    header by oracle.entry_header, an empty or raw value of up to 7 bytes, a
    key of 1 to 8 bytes, kEntryFull."""
    out = bytearray(head)
    for i in range(count):
        key, value = rnd(rng, 1 + i % 8), rnd(rng, (i // 8) % 8)
        h = orc.entry_header(orc.crc32c(key + value), 0x8, len(key), len(value), 0, 0, orc.xxh64(key))
        assert len(h) == 25
        out += h + key + value
    return bytes(out)


@pytest.fixture(scope="module")
def shapes(gpu, orc):
    rng = np.random.default_rng(77)
    small = [(b"s%03d" % i, rnd(rng, int(rng.integers(1, 300)))) for i in range(12)]
    more = [(b"m%03d" % i, rnd(rng, int(rng.integers(1, 300)))) for i in range(9)]
    on_boundary = ending_at(rng, 8192 + TILE, small)                       # ends with tile 0
    one = entries_of([(b"only", b"one value")])
    out = {
        # (an entry's bytes do not depend on where it lies: the second file's entries go behind the first's)
        "entry_ends_on_tile_boundary": on_boundary + entries_of(more)[8192:],
        "entry_over_two_tiles": entries_of(small + [(b"big", rnd(rng, 2 * TILE + 1700))] + more),
        "stop_in_first_byte_of_tile": on_boundary + bytes(50),
        "stop_in_last_byte_of_tile": ending_at(rng, 8192 + TILE - 1, small) + rnd(rng, 64),
        "entry_bytes_multiple_of_tile": ending_at(rng, 8192 + 2 * TILE, small),
        "one_entry": one,
        # the sequential hop goes from group to group (32 tiles, 128 KiB): a file of four groups, and an entry that
        # crosses a group's end by more than a tile, so that the chain enters the next group behind its first tile
        "four_groups": entries_of([(b"g%04d" % i, rnd(rng, 700 + i)) for i in range(460)]),
        "entry_over_group_end": entries_of([(b"long", rnd(rng, 120000))] + small + [(b"over", rnd(rng, 14000))] + more),
        "smallest_stride": smallest_entries(orc, rng, one[:8192], 2000),
    }
    ents, _, _ = R.walk(out["smallest_stride"], orc)
    assert len(ents) == 2000
    strides = {b[0] - a[0] for a, b in zip(ents, ents[1:])}
    assert min(strides) == 26 and max(strides) == 40, sorted(strides)
    return out


def test_tile_shapes_equal_the_model(shapes, orc):
    names = list(shapes)
    files = [shapes[n] for n in names]
    for scope in ("reference", "content"):
        got = run(files, scope)
        check_against_model(files, got, orc, scope)
        by = dict(zip(names, got))
        assert by["stop_in_first_byte_of_tile"][0].offset == 8192 + TILE
        assert by["stop_in_last_byte_of_tile"][0].offset == 8192 + TILE - 1
        assert by["entry_bytes_multiple_of_tile"][0].offset == 8192 + 2 * TILE == len(shapes["entry_bytes_multiple_of_tile"])
        assert by["one_entry"][0].rows_kept == 1 and by["smallest_stride"][0].rows_kept == 2000
        assert by["entry_ends_on_tile_boundary"][0].rows_kept == 13 + 9
        assert by["entry_over_two_tiles"][0].rows_kept == 12 + 1 + 9
        assert len(shapes["four_groups"]) > 8192 + 3 * 32 * TILE and by["four_groups"][0].rows_kept == 460
        over = [e for e in G.read_hstable(by["entry_over_group_end"][1]) if e.key == b"over"][0]
        group_end = 8192 + 32 * TILE
        assert over.offset < group_end and over.value_at + over.stored_len > group_end + TILE
        assert by["entry_over_group_end"][0].rows_kept == 1 + 12 + 1 + 9
        # the sequential part: one dependent load per tile touched, not per entry
        for f, (r, _) in zip(files, got):
            assert 0 < r.chain_loads <= (len(f) - 8192 + TILE - 1) // TILE
        tiles = sum((len(f) - 8192 + TILE - 1) // TILE for f in files)
        assert sum(r.chain_loads for r, _ in got) <= tiles < sum(r.entries_walked for r, _ in got) // 4
        assert by["four_groups"][0].chain_loads == 4


def test_decoy_entries_inside_values_are_not_listed(gpu, orc):
    rng = np.random.default_rng(78)
    # few and long inner entries: with many short ones LZ4 gains on the headers' zero bytes and the value is
    # stored as sequences, not verbatim
    inner = entries_of([(b"in%02d" % i, rnd(rng, 1200 + 10 * i)) for i in range(4)])[8192:]
    puts = []
    for i in range(5):
        puts.append((b"outer%d" % i, inner))
        puts.append((b"pad%d" % i, rnd(rng, 40 + i)))
    f = entries_of(puts)
    assert f.count(inner) == 5                       # stored verbatim: whole valid chains inside the values
    # the model, started inside a value, walks the decoys: they are valid entries
    at = f.index(inner)
    assert R.step(f, at, orc) is not None
    (r, out), = run([f], "reference")
    check_against_model([f], [(r, out)], orc, "reference")
    assert r.status == 0 and r.rows_kept == r.entries_walked == len(puts)
    rows = R.M.parse_rows(out)
    assert [o for _, o in rows] == [e.offset for e in G.read_hstable(out)]
    assert all(not (at <= o < at + len(inner)) for _, o in rows)


def test_capacity_below_the_bound_is_refused(gpu, fixture):
    f = fixture[1][0][1]
    lib = _lib.load()
    size = np.array([len(f)], np.uint64)
    off = np.zeros(1, np.uint64)
    need = int(lib.kdb_hstable_recover_scratch_bytes(size.ctypes.data, 1))
    dev, scratch = DeviceBuffer(rec.bound(len(f)) + 64), DeviceBuffer(need)
    try:
        dev.upload(np.frombuffer(f, np.uint8))
        new_size, status = np.zeros(1, np.uint64), np.zeros(1, np.int32)
        for cap, scope, sb, want in ((rec.bound(len(f)) - 64, 0, need, _lib.EINVAL), (len(f), 0, need, _lib.EINVAL),
                                     (rec.bound(len(f)), 2, need, _lib.EINVAL),
                                     (rec.bound(len(f)), 0, need - 256, _lib.EINVAL), (rec.bound(len(f)), 0, need, 0)):
            c = np.array([cap], np.uint64)
            rc = lib.kdb_hstable_recover_files(None, dev.ptr, off.ctypes.data, size.ctypes.data, c.ctypes.data, 1, scope,
                                               scratch.ptr, sb, new_size.ctypes.data, status.ctypes.data, None)
            assert rc == want, (cap, scope, sb)
        assert status[0] == 0 and len(f) < int(new_size[0]) <= rec.bound(len(f))
    finally:
        dev.free()
        scratch.free()
