"""CPU: the device HSTable writer's host-side parts, without a GPU.

  * csrc/hstable_cut.h -- where a batch is cut into files, walked file by
    file over prefix arrays, as hsd_plan_kernel runs it -- compiled for the
    host into a stand-alone program (tests/cpp/hstable_cut_main.cc) under
    AddressSanitizer and UBSan, against a straight entry-by-entry loop of the
    rule over seeded random batches and hand-made edges: a clean run;
  * kdb_hstable_dev_arena_bytes bounds the files the reference wrote for the
    golden put streams;
  * libkdb_lz4.so exports every symbol include/kdb_hstable_dev.h declares.
"""
import os
import re
import subprocess

import pytest

from conftest import ROOT, load_golden


def test_cut_rule_standalone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "hstable_cut_main")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "hstable_cut_main.cc"),
                        "-o", exe], capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "cannot find" in b.stderr and "san" in b.stderr:
        pytest.skip("no sanitizer runtime: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    m = re.fullmatch(r"ok (\d+) (\d+) (\d+)\n", r.stdout)
    assert m, r.stdout[-2000:]
    batches, files, rows = (int(x) for x in m.groups())
    # the random part alone is 1500 rounds of 1 to 5 batches, most of which close files
    assert batches >= 3000 and files >= 10000 and rows >= 100000


def test_arena_bound_covers_the_reference_files():
    from kingdb_amd import _lib
    from kingdb_amd import get as G
    lib = _lib.load()
    z = load_golden("hstable_streams.npz")
    names = [str(n) for n in z["names"]]
    assert sorted(names) == ["edge", "multipart", "murmur", "rollover", "small"]
    for name in names:
        hs = int(z[f"{name}__opts"][0])
        files = [z[f"{name}__file_{f}"] for f in z[f"{name}__files"]]
        total = sum(len(f) for f in files)
        # every byte past a header block is an entry byte, a row byte or a footer byte, so
        # the entry bytes are at most those; the rows are counted from the offset arrays
        entry_bytes = sum(len(f) - 8192 for f in files)
        magic = (0x4D454F57).to_bytes(8, "little")
        rows = sum(len(G.read_hstable(f.tobytes())) for f in files if f[-12:-4].tobytes() == magic)
        bound = lib.kdb_hstable_dev_arena_bytes(hs, entry_bytes, max(rows, 1))
        assert bound >= total + 64 * len(files), (name, bound, total)
        assert bound % 64 == 0
    # not an allocation size: hstable_size must exceed the header block
    assert lib.kdb_hstable_dev_arena_bytes(8192, 1000, 10) == 2 ** 64 - 1
    # no entries: still room for a file's frame
    assert lib.kdb_hstable_dev_arena_bytes(1 << 20, 0, 0) >= 8192 + 36 + 64


def test_library_exports_device_writer_symbols():
    from kingdb_amd import _lib
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "kdb_hstable_dev.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(kdb_hstable_dev_\w+)\s*\(", text)))
    assert syms == ["kdb_hstable_dev_append", "kdb_hstable_dev_arena_bytes", "kdb_hstable_dev_close",
                    "kdb_hstable_dev_create", "kdb_hstable_dev_destroy", "kdb_hstable_dev_download",
                    "kdb_hstable_dev_feed", "kdb_hstable_dev_file_count", "kdb_hstable_dev_files",
                    "kdb_hstable_dev_reset"]
    for s in syms:
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    put_h = open(os.path.join(ROOT, "include", "kdb_put.h")).read()
    assert '#include "kdb_hstable_dev.h"' in put_h
    from kingdb_amd import put
    from kingdb_amd.index import HSTableIndex
    assert put.DeviceHSTableWriter and put.write_hstables_device
    assert HSTableIndex.from_resident and HSTableIndex.compacted_device


def test_create_checks_its_arguments():
    """The argument checks of kdb_hstable_writer_create2, made before any device work."""
    import ctypes
    from kingdb_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.kdb_hstable_dev_create(8192, 1, 1 << 20, ctypes.byref(h)) == _lib.EINVAL
    assert lib.kdb_hstable_dev_create(1 << 20, 2, 1 << 20, ctypes.byref(h)) == _lib.EINVAL
    assert lib.kdb_hstable_dev_create(1 << 20, 1, 100, ctypes.byref(h)) == _lib.EINVAL
    assert lib.kdb_hstable_dev_create(1 << 20, 1, 1 << 20, None) == _lib.EINVAL
    assert h.value is None


def test_no_cpu_writer_without_device():
    """Without a device create fails: there is no host fallback behind this ABI."""
    import ctypes
    import kingdb_amd
    from kingdb_amd import _lib
    if kingdb_amd.device_count() > 0:
        pytest.skip("a GPU is visible; this checks the no-GPU behaviour")
    h = ctypes.c_void_p()
    rc = _lib.load().kdb_hstable_dev_create(1 << 20, 1, 1 << 20, ctypes.byref(h))
    assert rc in (_lib.ENODEV, _lib.EHIP) and h.value is None
    from kingdb_amd import put
    with pytest.raises(_lib.HipError):
        put.DeviceHSTableWriter(1 << 20, 1, 1 << 20)
