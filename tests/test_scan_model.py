"""CPU: the scan without a GPU.

  * the Python model of the scan (tests/scan_model.py) returns, on the files
    the reference wrote for tests/golden/get_keys.npz, exactly the distinct
    keys with the length and CRC32C of their last values -- the set the
    reference's own Database::Get confirmed -- each key once, and as many
    entries as the reference's own iterator visited (tests/golden/scan.npz,
    `iterated` with `iterator_bad` 0: tests/golden/make_golden_scan.py);
  * its order is (file rank, offset) ascending;
  * libkdb_lz4.so exports the scan's symbols of include/kdb_scan.h.

csrc/hstable_decode.h gained no function for the scan: the kernels run the
decode, validity check and key compare that tests/test_index_model.py already
runs on the host under the sanitizers.
"""
import os
import re

import pytest

import index_model as M
import scan_model as S
from conftest import ROOT, load_golden


@pytest.fixture(scope="module")
def sets():
    z = load_golden("get_keys.npz")
    out = {}
    for name in (str(n) for n in z["names"]):
        files = {str(f): z[f"{name}__file_{f}"].tobytes() for f in z[f"{name}__files"]}
        keys = [k.tobytes() for k in z[f"{name}__keys"]]
        out[name] = (files, int(z[f"{name}__opts"][1]), keys, z[f"{name}__len"], z[f"{name}__crc"])
    return out


@pytest.fixture(scope="module")
def counts():
    z = load_golden("scan.npz")
    return {str(n): (int(z[f"{n}__iterated"][0]), int(z[f"{n}__iterator_bad"][0])) for n in z["names"]}


@pytest.mark.parametrize("name,rows", [("xx", 400), ("murmur", 60)])
def test_model_scan_is_what_the_reference_iterated(sets, counts, orc, name, rows):
    files, ht, keys, lens, crcs = sets[name]
    m = M.Model(files, orc, ht)
    assert len(m.rows) == rows
    iterated, bad = counts[name]
    assert bad == 0 and iterated == len(keys)
    want = {(k, int(n), int(c)) for k, n, c in zip(keys, lens, crcs)}
    for verify in (0, 2):
        got = S.scan(m, verify)
        assert len(got) == iterated
        assert len({k for k, _, _ in got}) == len(got)                 # no key twice
        assert all(st == 0 for _, st, _ in got)
        assert {(k, len(v), orc.crc32c(v)) for k, _, v in got} == want
        assert S.prepare(m, verify) == (len(keys), sum(map(len, keys)), max(map(len, keys)))


@pytest.mark.parametrize("name", ["xx", "murmur"])
def test_model_scan_order(sets, orc, name):
    files, ht, _, _, _ = sets[name]
    m = M.Model(files, orc, ht)
    rows = S.live_rows(m)
    order = [(rank, off) for rank, off, _, _ in rows]
    assert order == sorted(order) and len(set(order)) == len(order)
    # ranks follow the sequence order of the files, which is their (timestamp, fileid) order
    seq_files = []
    for _, fname, _ in m.rows:
        if fname not in seq_files:
            seq_files.append(fname)
    assert [fname for _, _, fname, _ in rows] == sorted((f for _, _, f, _ in rows), key=seq_files.index)
    assert len({fname for _, _, fname, _ in rows}) > (1 if name == "xx" else 0)
    # and the scan lists the entries in that order
    assert [k for k, _, _ in S.scan(m)] == [k for _, _, _, k in rows]


def test_model_drops_what_get_cannot_reach(sets, orc):
    """A row listed twice is live once (the newer row), and a row whose array
    hash is not the hash of its stored key is not live."""
    files, ht, _, _, _ = sets["xx"]
    base = S.live_rows(M.Model(files, orc, ht))
    name = sorted(files)[0]
    rows = M.parse_rows(files[name])
    from kingdb_amd import get as G
    puts = {}
    for f in files.values():
        for e in G.read_hstable(f):
            puts[e.key] = puts.get(e.key, 0) + 1
    # a live row of this file whose key was put once: no older entry comes back when it goes
    live_offs = {off for _, off, n, k in base if n == name and puts[k] == 1}
    i = next(i for i, (_, off) in enumerate(rows) if off in live_offs)
    twice = dict(files)
    twice[name] = M.with_rows(files[name], rows + [rows[i]], orc)
    assert [(n, k) for _, _, n, k in S.live_rows(M.Model(twice, orc, ht))] == [(n, k) for _, _, n, k in base]
    forged = dict(files)
    forged[name] = M.with_rows(files[name], rows[:i] + [(rows[i][0] ^ 1, rows[i][1])] + rows[i + 1:], orc)
    got = S.live_rows(M.Model(forged, orc, ht))
    assert len(got) == len(base) - 1 and (name, rows[i][1]) not in {(n, off) for _, off, n, _ in got}


def test_library_exports_scan_symbols():
    from kingdb_amd import _lib
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "kdb_scan.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(kdb_index_\w+)\s*\(", text)))
    assert syms == ["kdb_index_scan_batch", "kdb_index_scan_prepare", "kdb_index_scan_scratch_bytes",
                    "kdb_index_scan_sort_steps"]
    for s in syms:
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    assert '#include "kdb_scan.h"' in open(os.path.join(ROOT, "include", "kdb_put.h")).read()
    assert lib.kdb_index_scan_scratch_bytes(1000) >= 4000
    from kingdb_amd import HSTableIndex
    for method in ("scan_prepare", "scan", "items", "compacted"):
        assert callable(getattr(HSTableIndex, method)), method
