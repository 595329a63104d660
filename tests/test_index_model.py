"""CPU: Get by key without a GPU.

  * the Python model of LoadFile + GetWithIndex + GetEntry + GetRaw
    (tests/index_model.py) returns, for every key of tests/golden/get_keys.npz,
    the value the reference's own Database::Get returned (ref_db --verify, see
    tests/golden/make_golden_getkeys.py), and NotFound for keys never put: after
    this it may serve as the checker for mutated files;
  * libkdb_lz4.so exports every kdb_index_* symbol of include/kdb_put.h;
  * csrc/hstable_decode.h -- the decode, validity check and key compare the
    lookup kernel runs per candidate -- compiled for the host into a
    stand-alone program under AddressSanitizer and UBSan, over the fixture's
    files and hostile candidates: a clean run whose every line equals the model.
"""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import index_model as M
from conftest import ROOT, load_golden
from kingdb_amd import get as G


@pytest.fixture(scope="module")
def sets():
    z = load_golden("get_keys.npz")
    out = {}
    for name in (str(n) for n in z["names"]):
        files = {str(f): z[f"{name}__file_{f}"].tobytes() for f in z[f"{name}__files"]}
        keys = [k.tobytes() for k in z[f"{name}__keys"]]
        out[name] = (files, int(z[f"{name}__opts"][1]), keys, z[f"{name}__len"], z[f"{name}__crc"])
    return out


@pytest.mark.parametrize("name", ["xx", "murmur"])
def test_model_returns_what_the_reference_returned(sets, orc, name):
    files, ht, keys, lens, crcs = sets[name]
    m = M.Model(files, orc, ht)
    assert set(m.file_status.values()) == {0}
    assert len(m.rows) == sum(len(G.read_hstable(f)) for f in files.values())
    for verify in (0, 2):
        for k, n, c in zip(keys, lens, crcs):
            st, val, loc = m.get(k, verify)
            assert (st, len(val), orc.crc32c(val)) == (0, int(n), int(c)), (k, verify)
            assert loc >> 32 in [int(f, 16) for f in files]
    for i in range(64):
        assert m.get(b"absent%010d" % i)[0] == M.NOTFOUND


def test_model_header_decode_equals_entry_reader(sets, orc):
    """On files as written, the model's bounds-checked header decode reads what
    get.decode_entry reads."""
    files = sets["xx"][0]
    for f in files.values():
        for e in G.read_hstable(f):
            rc, h = M.locate_entry(f, e.offset, True, orc)
            assert rc == 0
            assert (h["flags"], h["checksum"], h["size_key"], h["size_value"], h["svc"], h["padding"], h["hash"],
                    h["size_header"]) == (e.flags, e.checksum, len(e.key), e.size_value, e.size_value_compressed,
                                          e.size_padding, e.hashed, e.header_size)


def test_library_exports_index_symbols():
    from kingdb_amd import _lib
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "kdb_put.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(kdb_index_\w+)\s*\(", text)))
    assert syms == ["kdb_index_create", "kdb_index_destroy", "kdb_index_entry_count", "kdb_index_get_batch",
                    "kdb_index_get_scratch_bytes", "kdb_index_load_files", "kdb_index_pairs"]
    for s in syms:
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    for name, value in (("KDB_GET_NOTFOUND", -3), ("KDB_GET_DELETED", -4), ("KDB_GET_MULTIPART", -5)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", text), name
    import kingdb_amd
    assert kingdb_amd.HSTableIndex is not None


def decode_cases(files: dict, orc):
    """(file list, cases): every entry of every file with its own key and with
    another key, at verify 0 and 1, then the hostile candidates."""
    flist, cases = [], []
    for f in files.values():
        fi = len(flist)
        flist.append(f)
        ents = G.read_hstable(f)
        for j, e in enumerate(ents):
            cases.append((fi, e.offset, j & 1, e.key))
            cases.append((fi, e.offset, 0, ents[j - 1].key))
            cases.append((fi, e.offset, 0, e.key[:-1]))
    hf, hkeys = M.hardened_set(files, orc)
    name = sorted(hf)[-1]
    f = hf[name]
    fi = len(flist)
    flist.append(f)
    for (_, off), verify in ((r, v) for r in M.parse_rows(f) for v in (0, 1)):
        cases.append((fi, off, verify, hkeys[0]))
    for off in (len(f), len(f) - 1, len(f) - 3, len(f) - 5, len(f) - 20, len(f) + 1, 0xFFFFFFF0, 0, 24, 8191):
        cases.append((fi, off, 0, hkeys[0]))
    # a file that ends inside an entry header, and inside a key
    e = G.read_hstable(flist[0])[-1]
    for cut in (e.offset + 3, e.offset + 7, e.offset + e.header_size - 1, e.value_at - 2, e.value_at + 1):
        flist.append(flist[0][:cut])
        cases.append((len(flist) - 1, e.offset, 0, e.key))
    return flist, cases


def model_lines(flist, cases, orc):
    lines = []
    for i, f in enumerate(flist):
        ok = len(f) >= M.HEADER + M.FOOTER
        if ok:
            _, _, oi, num, magic, _ = M.footer(f)
            ok = magic == M.MAGIC and M.HEADER <= oi <= len(f) - M.FOOTER
        rows = M.parse_rows(f) if ok else None
        x = s = 0
        for h, o in rows or []:
            x ^= h
            s += o
        lines.append(f"file {i} {int(ok)} {num if ok else 0} {int(rows is not None)} {x} {s}")
    for i, (fi, off, verify, key) in enumerate(cases):
        f = flist[fi]
        rc, h = M.locate_entry(f, off, bool(verify), orc)
        if rc == M.DECODE_ERROR:
            lines.append(f"case {i} {rc}")
            continue
        at = off + h["size_header"]
        eq = rc == 0 and h["size_key"] == len(key) and f[at:at + len(key)] == key
        lines.append(f"case {i} {rc} {h['size_header']} {h['flags']} {h['size_key']} {h['size_value']} {h['svc']} "
                     f"{h['padding']} {h['hash']} {int(eq)}")
    return lines


def test_decode_header_standalone_under_sanitizers(sets, orc, tmp_path):
    exe = str(tmp_path / "index_decode_main")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "index_decode_main.cc"),
                        "-o", exe], capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "cannot find" in b.stderr and "san" in b.stderr:
        pytest.skip("no sanitizer runtime: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-3000:]
    flist, cases = decode_cases(sets["xx"][0], orc)
    m_files, _, _, _, _ = sets["murmur"]
    for f in m_files.values():
        flist.append(f)
        for e in G.read_hstable(f):
            cases.append((len(flist) - 1, e.offset, 1, e.key))
    dump = bytearray(struct.pack("<I", len(flist)))
    for f in flist:
        dump += struct.pack("<Q", len(f)) + f
    dump += struct.pack("<I", len(cases))
    for fi, off, verify, key in cases:
        dump += struct.pack("<IQII", fi, off, verify, len(key)) + key
    path = tmp_path / "cases.bin"
    path.write_bytes(bytes(dump))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    got = r.stdout.splitlines()
    want = model_lines(flist, cases, orc)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
    # the hostile candidates are there and are rejections, not reads
    assert sum(1 for w in want if re.match(r"case \d+ -[123]\b", w)) >= 20
