"""CPU: file recovery without a GPU.

  * the Python model of RecoverFile + WriteOffsetArray (tests/recover_model.py)
    reproduces, for every case of tests/golden/recover.npz, what the
    reference's own Database::Open left on disk (see
    tests/golden/make_golden_recover.py): removed or kept, the size, every
    byte from offset_indexes on, and the CRC32C of the whole file.  After this
    it may serve as the checker for the files the GPU tests build;
  * in `content` scope every multipart entry whose bytes are undamaged is
    kept, and the flipped ones are dropped;
  * csrc/hstable_recover.h -- the step, the CRC range and the walk -- and
    csrc/hstable_close.h -- the rows and the footer, the encoders the writer's
    and recovery's kernels call -- compiled for the host into a stand-alone
    program under AddressSanitizer and UBSan, over every fixture input in both
    scopes: a clean run whose every line (the CRC32C of the whole recovered
    file among its fields) equals the model;
  * libkdb_lz4.so exports every symbol of include/kdb_recover.h.
"""
import os
import re
import struct
import subprocess

import pytest

import recover_model as R
from conftest import ROOT, load_golden
from kingdb_amd import get as G


@pytest.fixture(scope="module")
def fixture():
    z = load_golden("recover.npz")
    return z, R.load_cases(z)


def test_fixture_holds_the_cases_the_issue_lists(fixture):
    z, cases = fixture
    names = [n for n, _, _ in cases]
    assert len(z["undefined"]) * 20 <= len(names) + len(z["undefined"])
    kinds = {"torn1", "torn4", "torn35", "cut_at_offset_indexes", "cut_mid_row", "cut_header3", "cut_header24",
             "cut_in_key", "cut_in_value", "cut_on_boundary", "cut_8202", "footer_crc_flipped", "flip_entry_header",
             "flip_plain_value", "zeros50", "zeros5000", "random64", "large_type_torn4"}
    for db, extra in (("sessions", set()), ("multipart", {"flip_multipart_value", "flip_multipart_padding"})):
        per_file = {}
        for n in names:
            d, f, k = n.split("/")
            if d == db:
                per_file.setdefault(f, set()).add(k)
        assert len(per_file) >= 2
        for f, ks in per_file.items():
            assert ks | set(str(u).split("/")[2] for u in z["undefined"] if str(u).startswith(f"{db}/{f}/")) == \
                kinds | extra, (db, f)


def test_model_reproduces_the_reference(fixture, orc):
    _, cases = fixture
    removed = kept = 0
    for name, f, want in cases:
        st, out, rep = R.recover(f, orc, "reference")
        if want is None:
            assert out is None, name
            assert st == (R.LARGE if "large_type" in name else R.NOENTRY), name
            removed += 1
            continue
        size, crc, oi, tail = want
        assert st == 0, name
        assert (len(out), rep["offset"]) == (size, oi), name
        assert out[oi:] == tail, name
        assert out[:oi] == f[:oi] and orc.crc32c(out) == crc, name
        assert len(out) <= R.bound(len(f)), name
        kept += 1
    assert removed >= 8 and kept >= 60


def test_flipped_footer_crc_gives_back_the_original_file(fixture, orc):
    z, cases = fixture
    n = 0
    for name, f, want in cases:
        if name.startswith("sessions/") and name.endswith("/footer_crc_flipped"):
            base = z["base__" + "_".join(name.split("/")[:2])].tobytes()
            assert f != base and R.recover(f, orc)[1] == base, name
            n += 1
    assert n >= 2


def test_content_scope_keeps_undamaged_multipart_entries(fixture, orc):
    z, cases = fixture
    seen_drop = seen_keep = 0
    for name, f, want in cases:
        if not name.startswith("multipart/") or want is None:
            continue
        base = z["base__" + "_".join(name.split("/")[:2])].tobytes()
        ents, stop, undefined = R.walk(f, orc, "content")
        assert not undefined
        intact = {e.offset: e for e in G.read_hstable(base)}
        for off, h, kept in ents:
            e = intact[off]
            end = e.value_at + e.stored_len
            same = f[off:end] == base[off:end]
            if h["flags"] & R.UNCOMPACTED:
                assert kept == same, (name, off)
                seen_keep += kept
                seen_drop += not kept
            else:
                assert kept, (name, off)
        st, out, rep = R.recover(f, orc, "content")
        assert st == 0 and rep["invalid"] == sum(1 for _, _, k in ents if not k)
        if name.endswith("flip_multipart_value"):
            assert rep["invalid"] == 1 and rep["flags"] == 3
        elif not name.endswith("flip_entry_header"):
            assert rep["invalid"] == 0 and rep["flags"] == 1, name
    assert seen_drop == 2 and seen_keep >= 100


def model_lines(files, orc, scope):
    lines = []
    for i, f in enumerate(files):
        st, out, rep = R.recover(f, orc, scope)
        lines.append(f"file {i} {st} {len(out) if out else 0} {orc.crc32c(out) if out else 0} {rep['walked']} "
                     f"{rep['kept']} {rep['invalid']} {rep['offset']} {rep['flags']}")
    return lines


def hostile_files(z, cases, orc):
    """Inputs beyond the fixture for the host walk: the undefined rule (an
    uncompacted entry whose size_value_compressed reaches past the file, header
    CRC-8 redone), files of 0, 24, 8192 and 8193 bytes, and a bad header CRC."""
    f = next(f for n, f, _ in cases if n == "multipart/00000001/torn4")
    out = [b"", f[:24], f[:8192], f[:8193], bytes([f[0] ^ 1]) + f[1:]]
    e = next(e for e in G.read_hstable(z["base__multipart_00000001"].tobytes()) if e.flags & R.UNCOMPACTED)
    b = bytearray(f)
    at = e.offset + e.header_size - 8 - 8 - 1            # size_value_compressed (padding is one byte here)
    assert struct.unpack_from("<Q", b, at)[0] == e.size_value_compressed and e.size_padding < 128
    struct.pack_into("<Q", b, at, len(f))
    b[e.offset] = orc.crc8(bytes(b[e.offset + 1:e.offset + e.header_size]))
    out.append(bytes(b))
    return out


def test_walk_standalone_under_sanitizers(fixture, orc, tmp_path):
    exe = str(tmp_path / "recover_walk_main")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "recover_walk_main.cc"),
                        "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    z, cases = fixture
    files = [f for _, f, _ in cases] + hostile_files(z, cases, orc)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    for scope, sname in ((0, "reference"), (1, "content")):
        dump = bytearray(struct.pack("<II", scope, len(files)))
        for f in files:
            dump += struct.pack("<Q", len(f)) + f
        path = tmp_path / f"files{scope}.bin"
        path.write_bytes(bytes(dump))
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
        assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        got = r.stdout.splitlines()
        want = model_lines(files, orc, sname)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g == w
    # the crafted entry is walked and dropped, not read; the files without a usable header are told apart
    assert R.walk(files[-1], orc, "content")[2]
    assert [int(w.split()[2]) for w in want[-6:-1]] == [R.BADHEADER] * 3 + [R.NOENTRY, R.BADHEADER]


def test_library_exports_recover_symbols():
    from kingdb_amd import _lib
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "kdb_recover.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(kdb_hstable_recover_\w+)\s*\(", text)))
    assert {"kdb_hstable_recover_bound", "kdb_hstable_recover_scratch_bytes", "kdb_hstable_recover_files"} <= set(syms)
    for s in syms:
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    for name, value in (("KDB_RECOVER_NOENTRY", R.NOENTRY), ("KDB_RECOVER_LARGE", R.LARGE),
                        ("KDB_RECOVER_BADHEADER", R.BADHEADER),
                        ("KDB_RECOVER_REFERENCE", 0), ("KDB_RECOVER_CONTENT", 1)):
        assert re.search(rf"#define\s+{name}\s+\(?{value}\b", text), name
    for size in (0, 8192, 8193, 8192 + 26, 36337, 32 << 20):
        assert lib.kdb_hstable_recover_bound(size) == R.bound(size)
    import kingdb_amd
    assert kingdb_amd.recover_files is not None
