"""CPU: the open file's tail of an index (include/kdb_index_tail.h), without a GPU.

  * the header declares exactly the new functions, the library exports them,
    _lib.SIGNATURES lists them, kdb_put.h includes the header;
  * the argument checks made before any device work, and no CPU path behind
    them;
  * csrc/index_rows.h -- the varint and row decode index_parse_kernel runs per
    thread, and the check of a staging range -- compiled for the host into a
    stand-alone program (tests/cpp/tail_rows_main.cc) under AddressSanitizer
    and UBSan: rows written by put_row into a staging stored backwards and
    read back through the reversed addressing, every varint length, row
    counts around a 256-byte tile's edge, every split of the incremental
    form, and hostile inputs refused without a read outside the range.
"""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

NAMES = ["kdb_hstable_dev_open_file", "kdb_index_drop_tail", "kdb_index_set_tail", "kdb_index_tail_stats"]


def test_header_symbols_and_defines():
    from kingdb_amd import _lib
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "kdb_index_tail.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(kdb_\w+)\s*\(", text)))
    assert syms == NAMES
    for s in syms:
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    assert '#include "kdb_index_tail.h"' in open(os.path.join(ROOT, "include", "kdb_put.h")).read()
    assert re.search(r"#define\s+KDB_INDEX_TAIL_REPARSE\s+1u\b", text)
    from kingdb_amd import index, put
    assert index.TAIL_REPARSE == 1
    for method in ("refresh", "set_tail", "drop_tail", "tail_stats"):
        assert callable(getattr(index.HSTableIndex, method)), method
    assert isinstance(index.HSTableIndex.tail, property)
    assert callable(put.DeviceHSTableWriter.open_file)
    # the record is the header's struct, field for field
    body = re.search(r"struct kdb_open_file \{(.*?)\};", text, re.S).group(1)
    fields = re.findall(r"\b(uint32_t|uint64_t)\s+(\w+);", body)
    want = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
    assert [(n, want[t]) for t, n in fields] == list(_lib.OpenFile._fields_)
    assert ctypes.sizeof(_lib.OpenFile) == 64


def test_the_docstrings_no_longer_call_the_open_file_unreadable():
    from kingdb_amd import index
    assert "tail=True" in index.HSTableIndex.refresh.__doc__
    assert "tail=True" in index.HSTableIndex.snapshot.__doc__
    assert "tail=True" in index.__doc__


def test_null_arguments():
    """KDB_PUT_EINVAL before any device work."""
    from kingdb_amd import _lib
    lib = _lib.load()
    f = _lib.OpenFile()
    held = ctypes.c_uint32(7)
    gained = ctypes.c_uint64(7)
    assert lib.kdb_hstable_dev_open_file(None, ctypes.byref(f)) == _lib.EINVAL
    assert lib.kdb_index_set_tail(None, None, 4096, ctypes.byref(f), 0, ctypes.byref(gained)) == _lib.EINVAL
    assert lib.kdb_index_drop_tail(None, None) == _lib.EINVAL
    assert lib.kdb_index_tail_stats(None, ctypes.byref(held), None, None, None, None, None) == _lib.EINVAL
    h = ctypes.c_void_p()
    assert lib.kdb_index_create(1, ctypes.byref(h)) == 0
    try:
        assert lib.kdb_index_set_tail(h, None, 4096, None, 0, ctypes.byref(gained)) == _lib.EINVAL      # no record
        assert lib.kdb_index_set_tail(h, None, 4096, ctypes.byref(f), 2, None) == _lib.EINVAL           # no such flag
        assert lib.kdb_index_tail_stats(h, None, None, None, None, None, None) == _lib.EINVAL          # no out-pointer
        # an open file and no buffer to read it from
        g = _lib.OpenFile(open=1, fileid=1, timestamp=1, file_off=0, bytes=8192 + 100, rows=1, row_bytes=2,
                          rows_last=1 << 20)
        assert lib.kdb_index_set_tail(h, None, None, ctypes.byref(g), 0, ctypes.byref(gained)) == _lib.EINVAL
        # records refused by host arithmetic alone: a row of one byte, of sixteen, a staging that begins before
        # the buffer, a file larger than a file can be; none reaches the device
        for rows, row_bytes, rows_last, nbytes in ((1, 1, 1 << 20, 9000), (1, 16, 1 << 20, 9000), (4, 8, 6, 9000),
                                                   (1, 2, 1 << 20, 1 << 62), ((1 << 30) + 1, 4 << 30, 1 << 40, 9000)):
            g = _lib.OpenFile(open=1, fileid=1, timestamp=1, file_off=0, bytes=nbytes, rows=rows,
                              row_bytes=row_bytes, rows_last=rows_last)
            assert lib.kdb_index_set_tail(h, None, 4096, ctypes.byref(g), 0, ctypes.byref(gained)) == _lib.EINVAL
            assert gained.value == 0
        # no file open, or an incomplete one: nothing to do on a handle without a tail
        assert lib.kdb_index_set_tail(h, None, None, ctypes.byref(f), 0, ctypes.byref(gained)) == 0
        assert gained.value == 0
        g = _lib.OpenFile(open=1, fileid=1, incomplete=1, timestamp=1, bytes=9000)
        assert lib.kdb_index_set_tail(h, None, None, ctypes.byref(g), 0, ctypes.byref(gained)) == 0
        assert lib.kdb_index_drop_tail(h, None) == 0
        fid, rows, nbytes, parsed, nb = (ctypes.c_uint32(9), ctypes.c_uint64(9), ctypes.c_uint64(9),
                                         ctypes.c_uint64(9), ctypes.c_uint64(9))
        assert lib.kdb_index_tail_stats(h, ctypes.byref(held), ctypes.byref(fid), ctypes.byref(rows),
                                        ctypes.byref(nbytes), ctypes.byref(parsed), ctypes.byref(nb)) == 0
        assert (held.value, fid.value, rows.value, nbytes.value, parsed.value, nb.value) == (0, 0, 0, 0, 0, 0)
        n = ctypes.c_uint64(9)
        assert lib.kdb_index_entry_count(h, ctypes.byref(n)) == 0 and n.value == 0
    finally:
        lib.kdb_index_destroy(h)


def test_no_cpu_path_without_device():
    """Without a device a tail with rows is an error, never a host parse."""
    import kingdb_amd
    from kingdb_amd import _lib
    if kingdb_amd.device_count() > 0:
        pytest.skip("a GPU is visible; this checks the no-GPU behaviour")
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.kdb_index_create(1, ctypes.byref(h)) == 0
    try:
        staging = (ctypes.c_uint8 * 64)()
        g = _lib.OpenFile(open=1, fileid=1, timestamp=1, file_off=0, bytes=8192 + 30, rows=1, row_bytes=2, rows_last=63)
        gained = ctypes.c_uint64(0)
        rc = lib.kdb_index_set_tail(h, None, ctypes.addressof(staging), ctypes.byref(g), 0, ctypes.byref(gained))
        assert rc in (_lib.EHIP, _lib.ENODEV) and gained.value == 0
        n = ctypes.c_uint64(9)
        assert lib.kdb_index_entry_count(h, ctypes.byref(n)) == 0 and n.value == 0
    finally:
        lib.kdb_index_destroy(h)


def test_row_decode_standalone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "tail_rows_main")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "tail_rows_main.cc"),
                        "-o", exe], capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "cannot find" in b.stderr and "san" in b.stderr:
        pytest.skip("no sanitizer runtime: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    m = re.fullmatch(r"ok (\d+) (\d+)\n", r.stdout)
    assert m, r.stdout[-2000:]
    rows, cases = (int(x) for x in m.groups())
    # 600 rows of the length pairs, 69 of the edge counts, 5 000, and 301 splits of 300
    assert rows >= 600 + 69 + 5000 + 301 * 300
    # 200 length pairs, 7 counts, 301 splits with 299 refused neighbours, 15 hostile and boundary cases,
    # 5 of the order rule (sorts_after_loaded)
    assert cases >= 200 + 7 + 301 + 299 + 15 + 5
