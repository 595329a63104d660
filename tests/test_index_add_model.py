"""CPU: newly closed files added to a loaded index (include/kdb_index_add.h),
without a GPU.

  * the header declares exactly the two functions, the library exports them,
    kdb_put.h includes the header, the defines have their values;
  * the argument checks made before any device work;
  * the expectation the GPU tests of tests/test_gpu_index_add.py rest on: the
    Python model of tests/index_model.py over a PREFIX of a database's files,
    in (timestamp, fileid) order, returns for every key the value of that
    key's last entry among those files -- what an index holds after the files
    were added one by one.  This passes without the feature and is here so
    that the GPU tests compare against a checked model.
"""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

import index_model as M
import keylens
from conftest import ROOT, load_golden
from kingdb_amd import get as G


def file_order(files: dict) -> list:
    """The names in LoadDatabase's order: by (timestamp, fileid)."""
    return sorted(files, key=lambda f: (struct.unpack_from("<Q", files[f], 16)[0], int(f, 16)))


def fixture_streams() -> dict:
    """{stream: (files, hash_type, keys)} of get_keys.npz and key_lengths.npz."""
    z = load_golden("get_keys.npz")
    out = {}
    for name in (str(n) for n in z["names"]):
        files = {str(f): z[f"{name}__file_{f}"].tobytes() for f in z[f"{name}__files"]}
        out["get_keys_" + name] = (files, int(z[f"{name}__opts"][1]), [k.tobytes() for k in z[f"{name}__keys"]])
    for name, s in keylens.load().items():
        out["key_lengths_" + name] = (s["files"], s["hash_type"], s["keys"])
    return out


def test_header_symbols_and_defines():
    from kingdb_amd import _lib
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "kdb_index_add.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(kdb_\w+)\s*\(", text)))
    assert syms == ["kdb_index_add_files", "kdb_index_add_stats"]
    for s in syms:
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    assert '#include "kdb_index_add.h"' in open(os.path.join(ROOT, "include", "kdb_put.h")).read()
    assert re.search(r"#define\s+KDB_INDEX_FILE_ORDER\s+\(-4\)", text)
    assert re.search(r"#define\s+KDB_INDEX_ADD_REBUILD\s+1u\b", text)
    from kingdb_amd import index
    assert index.FILE_ORDER == -4
    for method in ("refresh", "add_files"):
        assert callable(getattr(index.HSTableIndex, method)), method


def test_null_arguments():
    """KDB_PUT_EINVAL before any device work."""
    from kingdb_amd import _lib
    lib = _lib.load()
    one64, one32, st = np.zeros(1, np.uint64), np.zeros(1, np.uint32), np.zeros(1, np.int32)
    args = (None, 4096, one64.ctypes.data, one64.ctypes.data, one32.ctypes.data, 1, 0, st.ctypes.data, None)
    assert lib.kdb_index_add_files(None, *args) == _lib.EINVAL
    assert lib.kdb_index_add_stats(None, None, None, None) == _lib.EINVAL
    h = ctypes.c_void_p()
    assert lib.kdb_index_create(1, ctypes.byref(h)) == 0
    try:
        added = ctypes.c_uint64(7)
        assert lib.kdb_index_add_files(h, None, None, None, None, None, 1, 0, None, ctypes.byref(added)) == _lib.EINVAL
        for hole in (1, 2, 3, 4, 7):                     # d_files, file_off, file_size, fileid, file_status_out
            a = list(args)
            a[hole] = None
            assert lib.kdb_index_add_files(h, *a) == _lib.EINVAL, hole
        a = list(args)
        a[6] = 2                                         # a flag that does not exist
        assert lib.kdb_index_add_files(h, *a) == _lib.EINVAL
        # no files: nothing to do, and no add to speak of yet
        assert lib.kdb_index_add_files(h, None, None, None, None, None, 0, 0, None, ctypes.byref(added)) == 0
        assert added.value == 0
        assert lib.kdb_index_add_stats(h, None, None, None) == _lib.EINVAL
        n = ctypes.c_uint64(9)
        assert lib.kdb_index_entry_count(h, ctypes.byref(n)) == 0 and n.value == 0
    finally:
        lib.kdb_index_destroy(h)


@pytest.mark.parametrize("stream", ["get_keys_xx", "get_keys_murmur", "key_lengths_xx", "key_lengths_murmur"])
def test_model_over_a_prefix_reads_the_last_entry_so_far(orc, stream):
    files, ht, keys = fixture_streams()[stream]
    order = file_order(files)
    assert order == sorted(files)                        # the writers' timestamps and ids ascend together
    last = {}                                            # key -> (file, entry) of its last entry so far
    for k in range(1, len(order) + 1):
        name = order[k - 1]
        for e in G.read_hstable(files[name]):
            last[e.key] = (name, e)
        prefix = {f: files[f] for f in order[:k]}
        m = M.Model(prefix, orc, ht)
        assert len(m.rows) == sum(len(G.read_hstable(f)) for f in prefix.values())
        for key in keys:
            st, val, loc = m.get(key)
            if key not in last:
                assert (st, val, loc) == (M.NOTFOUND, b"", 0)
                continue
            name, e = last[key]
            f = files[name]
            assert e.flags & 0x1 == 0
            want = orc.get_value(f[e.value_at:e.value_at + e.stored_len], e.size_value_compressed, e.size_value,
                                 e.checksum, orc.crc32c(key), 0)
            assert (st, val) == want and st == 0, (k, key)
            assert loc == (int(name, 16) << 32 | e.offset)
    assert set(last) == set(keys)
