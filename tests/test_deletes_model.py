"""CPU: deletes (include/kdb_ops.h, kingdb_amd/put.py) against the reference.

  * every delete entry the reference wrote (tests/golden/deletes.npz) is a
    header of flags 0x9 and zeros followed by the key, and its offset-array
    row carries the key's real hash;
  * tests/index_model.py's Model over those files answers, per key, what the
    reference's own Database::Get answered -- before a recovery and after one,
    the keys that come back included;
  * libkdb_lz4.so exports kdb_put_ops_batch, _lib.SIGNATURES has it, and the
    header's constants are Python's;
  * without a device the entry point reports KDB_PUT_ENODEV: there is no host
    fallback;
  * a delete item takes no chunks.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import deletes_fixture as D
import index_model as M
from conftest import ROOT


@pytest.fixture(scope="module")
def fixture():
    return D.load()


def test_reference_delete_entries_are_flags_and_zeros(fixture, orc):
    sets, torn = fixture
    seen = 0
    for name, s in sets.items():
        h = orc.xxh64 if s["hash_type"] == 1 else orc.murmur3_64
        ndel = 0
        for fname, f in s["files"].items():
            for row_hash, e in D.delete_entries(f):
                ndel += 1
                assert (e.flags, e.checksum, e.size_value, e.size_value_compressed, e.size_padding, e.hashed) == \
                    (0x9, 0, 0, 0, 0, 0), (name, fname, e.offset)
                assert f[e.offset:e.value_at] == orc.entry_header(0, 0x9, len(e.key), 0, 0, 0, 0) + e.key
                assert row_hash == h(e.key), (name, fname, e.offset)
        assert ndel == sum(1 for _, v, _ in s["ops"] if v is None), name
        seen += ndel
    assert seen > 3000
    # a recovered file files its deletes under the header's hash, 0
    for t in torn:
        dels = D.delete_entries(t["recovered"])
        assert dels and all(row_hash == 0 for row_hash, _ in dels)


def test_model_gives_the_reference_get_codes(fixture, orc):
    sets, torn = fixture
    for name, s in sets.items():
        m = M.Model(s["files"], orc, s["hash_type"])
        assert set(m.file_status.values()) == {0}, name
        got = [m.get(k)[:2] for k in s["keys"]]
        D.assert_codes(got, s["keys"], s["code"], s["len"], s["crc"], orc, name)
        # and the codes are the last op's: a delete answers DeleteOrder even for a key never put
        last = D.last_ops(s["ops"])
        assert [D.REF_DELETE_ORDER if last[k] is None else D.REF_OK for k in s["keys"]] == s["code"], name
    s = sets["mixed"]
    back = 0
    for i, t in enumerate(torn):
        files = dict(s["files"])
        files[t["base"]] = t["recovered"]
        m = M.Model(files, orc, s["hash_type"])
        got = [m.get(k)[:2] for k in s["keys"]]
        D.assert_codes(got, s["keys"], t["code"], t["len"], t["crc"], orc, f"torn {i}")
        # one row per op, so the ops that survive the cut are a prefix of the stream
        last = D.last_ops(s["ops"][:len(m.rows)])
        back += sum(1 for k, c in zip(s["keys"], t["code"]) if c == D.REF_OK and k in last and last[k] is None)
    assert back > 0              # keys whose last surviving op is a delete are readable again after the recovery


def test_ops_batch_is_exported_and_declared(orc):
    from kingdb_amd import _lib, put
    text = open(os.path.join(ROOT, "include", "kdb_ops.h")).read()
    assert '#include "kdb_ops.h"' in open(os.path.join(ROOT, "include", "kdb_put.h")).read()
    names = set(re.findall(r"\b(kdb_put_ops_\w+)\s*\(", text))
    assert names == {"kdb_put_ops_batch"}
    lib = _lib.load()
    for n in names:
        assert n in _lib.SIGNATURES and getattr(lib, n) is not None
    # op, flags, then kdb_put_entries_batch's arguments in its order
    res, args = _lib.SIGNATURES["kdb_put_ops_batch"]
    eres, eargs = _lib.SIGNATURES["kdb_put_entries_batch"]
    assert res == eres and args == [eargs[0], ctypes.c_void_p, ctypes.c_uint32] + eargs[1:]
    consts = {k: int(v.rstrip("u"), 0) for k, v in re.findall(r"#define\s+(KDB_OPS?_\w+)\s+(\w+)", text)
              if not k.endswith("_H_")}
    assert consts == {"KDB_OP_PUT": put.OP_PUT, "KDB_OP_DELETE": put.OP_DELETE,
                      "KDB_OPS_DELETE_HASHED": put.OPS_DELETE_HASHED}


def test_no_cpu_path_without_device():
    import kingdb_amd
    from kingdb_amd import _lib
    if kingdb_amd.device_count() > 0:
        pytest.skip("a GPU is visible; this checks the no-GPU behaviour")
    lib = _lib.load()
    total = np.zeros(1, np.uint64)
    sb = lib.kdb_put_scratch_bytes(0, 0, 0)
    rc = lib.kdb_put_ops_batch(None, None, 0, None, None, None, None, None, None, None, None, 0, 0, 0, 1, None, sb, 0,
                               None, None, None, total.ctypes.data, None, None, None, None)
    assert rc == _lib.ENODEV
    # an unknown flag is refused before any device work
    rc = lib.kdb_put_ops_batch(None, None, 2, None, None, None, None, None, None, None, None, 0, 0, 0, 1, None, sb, 0,
                               None, None, None, total.ctypes.data, None, None, None, None)
    assert rc == _lib.EINVAL


def test_a_delete_takes_no_chunks():
    from kingdb_amd import put
    with pytest.raises(ValueError):
        put._layout([(b"k", b"abc"), (b"k", put.DELETE, [0])])
    with pytest.raises(ValueError):
        put._layout([(b"k", put.DELETE, [])])
    *_, pf, clen, ops = put._layout([(b"a", b"xy"), (b"k", put.DELETE), (b"b", b"z", None), (b"c", put.DELETE, None)])
    assert list(ops) == [0, 1, 0, 1] and list(pf) == [0, 1, 1, 2, 2] and list(clen) == [2, 1]
    assert put._layout([(b"a", b"xy")])[-1] is None
    assert put.entries_bound([(b"k", put.DELETE)]) >= 25 + 1
