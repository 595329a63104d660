"""CPU: snapshots and the hand-over over the writer's open file
(include/kdb_live.h), without a GPU.

  * the header declares exactly the four functions, the library exports them,
    _lib.SIGNATURES lists them, kdb_put.h includes the header;
  * the argument checks made before any device work, on handles made without a
    GPU: a tail snapshot of an empty handle is a plain one, adopt_open of
    nothing is refused;
  * the Python interface: snapshot(tail=), compact(carry_open=),
    compact_copy(closed_only=) and adopt_open exist, with defaults that keep
    the behaviour they had;
  * csrc/live_pin.h -- may a drop, a set_tail or an add proceed while tail
    snapshots pin the open file -- compiled for the host into a stand-alone
    program (tests/cpp/live_pin_main.cc) and run for every combination;
  * the expectation tests/test_gpu_live.py rests on.  A tail snapshot reads
    the rows of sequence number < R through the files as they are; its
    contract names a handle loaded over the closed files F and X_r, the open
    file closed with exactly its first r rows.  Over the files the reference
    wrote, for every file and every cut r inside it, the model restricted to
    rows < R (tests/index_model.py, tests/scan_model.py) must select the same
    row for every key and list the same live rows as the model over F and
    X_r; at the cuts 0, 1, the middle, n - 1 and n of every file Get's values
    and the whole scan are compared as well (between the cuts named, equal
    locations in files equal up to the cut give equal values).  The files of
    the one stream with thousands of rows (deletes `cuts`) are cut at those
    five places only: the model's scan is quadratic in the rows.
"""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

import deletes_fixture as D
import index_model as M
import scan_model as S
from conftest import ROOT
from test_index_add_model import file_order, fixture_streams

FUNCTIONS = ["kdb_hstable_dev_adopt_open", "kdb_snapshot_create_tail", "kdb_snapshot_scan_closed_live",
             "kdb_snapshot_tail_stats"]


def test_header_symbols_and_signatures():
    from kingdb_amd import _lib
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "kdb_live.h")).read()
    assert "database.cc:305-306" in text and "storage_engine.h:604-1010" in text     # the reference rows it stands for
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(kdb_\w+)\s*\(", code))) == FUNCTIONS
    for s in FUNCTIONS:
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    assert '#include "kdb_live.h"' in open(os.path.join(ROOT, "include", "kdb_put.h")).read()
    assert _lib.SIGNATURES["kdb_snapshot_create_tail"] == _lib.SIGNATURES["kdb_snapshot_create"]


def test_python_interface_and_defaults():
    from kingdb_amd import index, put
    sig = inspect.signature
    assert sig(index.HSTableIndex.snapshot).parameters["tail"].default is False
    assert sig(index.HSTableIndex.compact).parameters["carry_open"].default is False
    assert sig(index.HSTableIndex.compact_copy).parameters["closed_only"].default is False
    assert index.HSTableSnapshot.compact_copy is index.HSTableIndex.compact_copy
    assert sig(index.HSTableSnapshot.__init__).parameters["tail"].default is False
    assert callable(put.DeviceHSTableWriter.adopt_open)
    assert isinstance(index.HSTableSnapshot.tail, property)
    for method in ("tail_stats", "closed_live"):
        assert callable(getattr(index.HSTableSnapshot, method)), method
    doc = index.HSTableIndex.snapshot.__doc__
    assert "tail=True" in doc and "kdb_snapshot_create_tail" in doc
    assert "are not in a snapshot" not in doc                      # the sentence the feature makes untrue
    assert "carry_open=True" in index.HSTableIndex.compact.__doc__
    assert "closed_only=True" in index.HSTableIndex.compact_copy.__doc__
    assert "tail=True" in index.__doc__ and "carry_open=True" in index.__doc__


def test_null_arguments_and_the_empty_handle():
    """KDB_PUT_EINVAL before any device work; a tail snapshot of a handle without a tail is a plain one."""
    from kingdb_amd import _lib
    lib = _lib.load()
    snap = ctypes.c_void_p()
    inc, fid, pin = ctypes.c_uint32(9), ctypes.c_uint32(9), ctypes.c_uint32(9)
    rows, n64 = ctypes.c_uint64(9), ctypes.c_uint64(9)
    n32 = ctypes.c_uint32(9)
    assert lib.kdb_snapshot_create_tail(None, ctypes.byref(snap)) == _lib.EINVAL
    assert lib.kdb_snapshot_tail_stats(None, ctypes.byref(inc), None, None, None) == _lib.EINVAL
    assert lib.kdb_snapshot_scan_closed_live(None, ctypes.byref(n64)) == _lib.EINVAL
    assert lib.kdb_hstable_dev_adopt_open(None, None, None) == _lib.EINVAL
    h = ctypes.c_void_p()
    assert lib.kdb_index_create(1, ctypes.byref(h)) == 0
    try:
        assert lib.kdb_snapshot_create_tail(h, None) == _lib.EINVAL
        plain = ctypes.c_void_p()
        assert lib.kdb_snapshot_create(h, ctypes.byref(plain)) == 0
        assert lib.kdb_snapshot_create_tail(h, ctypes.byref(snap)) == 0 and snap.value
        try:
            for s in (snap, plain):
                assert lib.kdb_snapshot_entry_count(s, ctypes.byref(n64)) == 0 and n64.value == 0
                assert lib.kdb_snapshot_file_count(s, ctypes.byref(n32)) == 0 and n32.value == 0
                assert lib.kdb_snapshot_tail_stats(s, ctypes.byref(inc), ctypes.byref(fid), ctypes.byref(rows),
                                                   ctypes.byref(pin)) == 0
                assert (inc.value, fid.value, rows.value, pin.value) == (0, 0, 0, 0)
                assert lib.kdb_snapshot_tail_stats(s, None, None, None, None) == _lib.EINVAL       # no out-pointer
                assert lib.kdb_snapshot_tail_stats(s, ctypes.byref(inc), None, None, None) == 0
                # before a prepare, and without an out-pointer
                assert lib.kdb_snapshot_scan_closed_live(s, ctypes.byref(n64)) == _lib.EINVAL
                assert lib.kdb_snapshot_scan_closed_live(s, None) == _lib.EINVAL
            # it counts as an open snapshot, and pins nothing: a drop and a set of no file pass
            assert lib.kdb_index_destroy(h) == _lib.EINVAL
            assert lib.kdb_index_drop_tail(h, None) == 0
            f = _lib.OpenFile()
            assert lib.kdb_index_set_tail(h, None, None, ctypes.byref(f), 0, None) == 0
        finally:
            assert lib.kdb_snapshot_release(snap) == 0
            assert lib.kdb_snapshot_release(plain) == 0
    finally:
        assert lib.kdb_index_destroy(h) == 0


def test_pin_rule_standalone(tmp_path):
    exe = str(tmp_path / "live_pin_main")
    src = os.path.join(ROOT, "tests", "cpp", "live_pin_main.cc")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"]
    san = ["-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    b = subprocess.run(base + san + [src, "-o", exe], capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "cannot find" in b.stderr and "san" in b.stderr:
        b = subprocess.run(base + [src, "-o", exe], capture_output=True, text=True, timeout=300)    # no sanitizer runtime
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    # pinned or not x 4 pinned row counts x (1 drop + 6 sets + 4 row counts x 6 adds); allowed: everything when
    # not pinned, and when pinned the set of the same file and the tail's own file with enough rows
    assert r.stdout == "ok %d %d\n" % (2 * 4 * 31, 4 * 31 + 4 * 1 + (4 + 3 + 3 + 3)), r.stdout[-2000:]


# ------------------------------------------------------------------ the model of a tail snapshot
def all_streams() -> dict:
    out = {}
    for name, (files, ht, keys) in fixture_streams().items():
        out[name] = (files, ht, keys)
    for name, s in D.load()[0].items():
        out["deletes_" + name] = (s["files"], s["hash_type"], s["keys"])
    return out


def truncated(f: bytes, r: int, orc) -> bytes:
    """X_r: the file closed with exactly its first r rows -- the entries up to
    where row r's begins, the first r rows, a footer of its own."""
    rows = M.parse_rows(f)
    assert [o for _, o in rows] == sorted(o for _, o in rows)       # the writer's files: entries in row order
    end = rows[r][1] if r < len(rows) else M.footer(f)[2]
    return M.with_rows(f, rows[:r], orc, f[:end])


class Limited(M.Model):
    """The model over `files` with only the rows of sequence number < R: what
    index_get_kernel<true> and index_live_kernel<true> see."""

    def __init__(self, files, orc, hash_type, R):
        super().__init__(files, orc, hash_type)
        assert R <= len(self.rows)
        self.rows = self.rows[:R]


def selection(model, keys):
    """Per key: the row Get selects and what it is (a delete or not), or None."""
    out = []
    for k in keys:
        r, e = S.select(model, k, 0)
        out.append(None if r is None else (r, model.rows[r][2], e["flags"] & 1))
    return out


def cuts_of(n: int, dense: bool):
    full = sorted({0, min(1, n), n // 2, max(n - 1, 0), n})
    if dense:
        return list(range(n + 1)), full
    return full, [n // 2]


@pytest.mark.parametrize("stream", sorted(["get_keys_xx", "get_keys_murmur", "key_lengths_xx", "key_lengths_murmur",
                                           "deletes_mixed", "deletes_lengths", "deletes_cuts", "deletes_murmur"]))
def test_rows_below_R_answer_as_the_file_cut_at_r(orc, stream):
    files, ht, keys = all_streams()[stream]
    order = file_order(files)
    keys = keys if len(keys) <= 300 else keys[::len(keys) // 300]
    q = list(keys) + [k[:-1] for k in keys[:20]] + [k + b"\0" for k in keys[:20]] + [b""]
    compared = deletes = 0
    for i, name in enumerate(order):
        closed = {f: files[f] for f in order[:i]}
        n = len(M.parse_rows(files[name]))
        base = sum(len(M.parse_rows(files[f])) for f in order[:i])
        every, full = cuts_of(n, dense=n <= 150)          # a stream of thousands of rows: its edges and its middle
        for r in every:
            x = truncated(files[name], r, orc)
            assert files[name].startswith(x[:M.footer(x)[2]])
            want = M.Model(dict(closed, **{name: x}), orc, ht)
            got = Limited(dict(closed, **{name: files[name]}), orc, ht, base + r)
            assert want.file_status[name] == 0 and len(want.rows) == base + r
            assert [(h, o) for h, _, o in got.rows] == [(h, o) for h, _, o in want.rows]
            sel = selection(got, q)
            assert sel == selection(want, q), (name, r)
            assert S.live_rows(got) == S.live_rows(want), (name, r)
            deletes += sum(1 for s in sel if s is not None and s[2])
            if r in full:
                assert [got.get(k) for k in q] == [want.get(k) for k in q], (name, r)
                assert S.scan(got) == S.scan(want) and S.prepare(got) == S.prepare(want), (name, r)
            compared += 1
    assert compared >= len(order) * 3
    if stream.startswith("deletes_"):
        assert deletes > 0
