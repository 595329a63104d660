"""CPU: the compaction by copy without a GPU.

  * include/kdb_compact.h: its names are exported and in _lib.SIGNATURES,
    kdb_put.h includes it, the Python methods exist;
  * the argument checks of the new calls on handles made without a GPU;
  * the model (tests/compact_model.py): a self-contained source entry
    reproduces its own bytes, a finished multipart entry becomes header + key +
    its size_value_compressed stored bytes;
  * the layout rules pinned to the reference itself: the model compacts the
    first two of the four files the reference wrote for get_keys.npz `xx`, and
    the reference's own Database (oracle/_ref/ref_db --verify) opens the
    directory -- compacted files of type 2 with the view's largest timestamp
    and ids above every id, then the two other files -- and finds every key
    with its last value;
  * the same with the compacted files stamped with the largest timestamp of
    the whole directory: what the locked timestamp is for.
"""
import ctypes
import os
import re
import struct
import subprocess

import pytest

import compact_model as C
import index_model as M
import scan_model as S
from conftest import ROOT, load_golden

REF_DB = os.path.join(ROOT, "oracle", "_ref", "ref_db")
needs_ref_db = pytest.mark.skipif(not os.path.exists(REF_DB), reason="oracle/_ref/ref_db is not built")


@pytest.fixture(scope="module")
def xx():
    z = load_golden("get_keys.npz")
    files = {str(f): z[f"xx__file_{f}"].tobytes() for f in z["xx__files"]}
    hs, ht, part = (int(x) for x in z["xx__opts"])
    keys = [k.tobytes() for k in z["xx__keys"]]
    return dict(files=files, hs=hs, ht=ht, part=part, keys=keys, len=z["xx__len"], crc=z["xx__crc"],
                stream=z["xx__stream"].tobytes())


def test_library_exports_compact_symbols():
    from kingdb_amd import _lib
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "kdb_compact.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(kdb_\w+)\s*\(", text)))
    assert syms == ["kdb_compact_entries_batch", "kdb_compact_entries_batch_timed", "kdb_compact_piece_bytes", "kdb_compact_plan_batch",
                    "kdb_compact_scratch_bytes", "kdb_hstable_dev_adopt", "kdb_hstable_dev_create2",
                    "kdb_hstable_dev_open_bytes", "kdb_index_view_timestamp"]
    for s in syms:
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    assert '#include "kdb_compact.h"' in open(os.path.join(ROOT, "include", "kdb_put.h")).read()
    from kingdb_amd import put
    from kingdb_amd.index import HSTableIndex, HSTableSnapshot
    assert HSTableIndex.compact and HSTableIndex.compact_copy and HSTableSnapshot.compact_copy
    assert put.DeviceHSTableWriter.adopt and put.DeviceHSTableWriter.open_bytes
    # compacted and compacted_device stay
    assert HSTableIndex.compacted and HSTableIndex.compacted_device


def test_sizes():
    from kingdb_amd import _lib
    lib = _lib.load()
    piece = lib.kdb_compact_piece_bytes()
    assert piece >= 4096 and piece % 4096 == 0          # whole 16-byte words, a whole number of rounds
    assert lib.kdb_compact_scratch_bytes(0) >= 8
    for n in (1, 1000, 65536):
        assert lib.kdb_compact_scratch_bytes(n) >= 64 * n


def test_calls_check_their_arguments():
    """Refusals decided before any device work: they hold without a GPU."""
    from kingdb_amd import _lib
    lib = _lib.load()
    EINVAL = _lib.EINVAL
    h = ctypes.c_void_p()
    # create2: the file type is 1 or 2, the other checks are kdb_hstable_dev_create's
    for ftype in (0, 3, 4):
        assert lib.kdb_hstable_dev_create2(1 << 20, 1, 1 << 20, ftype, 7, ctypes.byref(h)) == EINVAL
    assert lib.kdb_hstable_dev_create2(8192, 1, 1 << 20, 2, 7, ctypes.byref(h)) == EINVAL
    assert lib.kdb_hstable_dev_create2(1 << 20, 2, 1 << 20, 2, 7, ctypes.byref(h)) == EINVAL
    assert lib.kdb_hstable_dev_create2(1 << 20, 1, 100, 2, 7, ctypes.byref(h)) == EINVAL
    assert lib.kdb_hstable_dev_create2(1 << 20, 1, 1 << 20, 2, 7, None) == EINVAL
    assert h.value is None
    b = ctypes.c_uint64(5)
    assert lib.kdb_hstable_dev_open_bytes(None, ctypes.byref(b)) == EINVAL
    assert lib.kdb_hstable_dev_adopt(None, None, 1, None, None, None, None, 0) == EINVAL
    # the index accessor on an empty handle (kdb_index_create needs no device)
    ix = ctypes.c_void_p()
    assert lib.kdb_index_create(1, ctypes.byref(ix)) == _lib.OK
    try:
        ts = ctypes.c_uint64(99)
        assert lib.kdb_index_view_timestamp(ix, 0, ctypes.byref(ts)) == _lib.OK and ts.value == 0
        assert lib.kdb_index_view_timestamp(ix, 1, ctypes.byref(ts)) == EINVAL
        assert lib.kdb_index_view_timestamp(ix, 0, None) == EINVAL
        assert lib.kdb_index_view_timestamp(None, 0, ctypes.byref(ts)) == EINVAL
    finally:
        lib.kdb_index_destroy(ix)
    # the copy: no total, a hash type that does not exist, a scratch too small,
    # buffers that are not 16-byte aligned (pointer values only; nothing is read)
    p = 1 << 20
    plan = [None, p, 64, p, p, p, p, p, p, p, p, 4, 1 << 20, 1, p, lib.kdb_compact_scratch_bytes(4), p, p, p, p, p, p]
    def call(changes):
        a = list(plan)
        for i, v in changes.items():
            a[i] = v
        return lib.kdb_compact_plan_batch(*a)
    assert call({18: None}) == EINVAL                   # total
    assert call({13: 2}) == EINVAL                      # hash_type
    assert call({15: lib.kdb_compact_scratch_bytes(4) - 1}) == EINVAL
    assert call({3: None}) == EINVAL                    # key_off
    ent = [None, p, 1 << 20, p, 64, p, p, p, p, p, p, p, p, 4, 1, p, lib.kdb_compact_scratch_bytes(4), p, 1 << 20,
           p, p, p, p, p, p, None]
    def ecall(changes):
        a = list(ent)
        for i, v in changes.items():
            a[i] = v
        return lib.kdb_compact_entries_batch(*a)
    assert ecall({1: p + 4}) == EINVAL                  # files
    assert ecall({17: p + 8}) == EINVAL                 # entries
    assert ecall({17: None}) == EINVAL
    assert ecall({21: None}) == EINVAL                  # total
    assert ecall({14: 2}) == EINVAL


def test_model_entries(xx, orc):
    """Over all four files: a self-contained source entry is reproduced byte
    for byte; a finished multipart one loses its padding and its two flags and
    keeps its stored bytes."""
    from kingdb_amd import get as G
    view = C.view_model(xx["files"], sorted(xx["files"]), orc, xx["ht"])
    ents = C.entries(view)
    rows = S.live_rows(view)
    assert len(ents) == len(rows) == len(xx["keys"])
    kinds = set()
    for (key, entry, hashed, size_value, svc, checksum, stored), (_, off, name, k) in zip(ents, rows):
        assert key == k
        f = xx["files"][name]
        rc, e = M.locate_entry(f, off, True, orc)
        assert rc == 0
        src = f[off:off + e["size_header"] + e["size_key"] + e["svo"]]
        if e["flags"] == 0x8:
            kinds.add("self")
            assert entry == src
        else:
            kinds.add("multipart")
            assert e["flags"] == 0x8 | 0x2 | 0x4 and e["padding"] > 0 and e["svc"] > 0
            assert len(stored) == e["svc"] <= e["svo"]      # equal where no part compressed: 8 + size
            assert entry == orc.entry_header(e["checksum"], 0x8, len(key), e["size_value"], e["svc"], 0,
                                             e["hash"]) + key + src[e["size_header"] + len(key):][:e["svc"]]
        # the copy reads as the source reads: same value, checksum still valid
        g = G.decode_entry(entry, 0)
        assert (g.key, g.size_value, g.size_value_compressed, g.size_padding, g.checksum) == (
            key, size_value, svc, 0, checksum)
        st, val = orc.get_value(entry[g.value_at:], svc, size_value, checksum, orc.crc32c(key), 2)
        assert st == 0 and val == view.get(key)[1]
    assert kinds == {"self", "multipart"}


def test_model_files_load_as_the_view(xx, orc):
    """The compacted files hold the view's live rows in scan order, are of type
    2 with the view's largest timestamp, and together with the other files
    answer every key as the four files did."""
    names = sorted(xx["files"])
    out, comp = C.directory(xx["files"], names[:2], orc, xx["hs"], 64, xx["ht"])
    assert len(comp) >= 1 and comp[0] == "%08x" % (int(names[-1], 16) + 1)
    view = C.view_model(xx["files"], names[:2], orc, xx["ht"])
    ts = C.timestamp_max(view)
    assert ts == 2
    for f in comp:
        b = out[f]
        assert struct.unpack_from("<IQ", b, 12) == (2, ts)
        assert M.footer(b)[0] == 2 and M.footer(b)[1] == 0        # no padding flag
        assert M.load_file(b, orc)[0] == 0
    assert sorted(out) == sorted(names[2:] + comp)
    # the compacted files come first by (timestamp, id)
    order = sorted(out, key=lambda f: (struct.unpack_from("<Q", out[f], 16)[0], int(f, 16)))
    assert order[:len(comp)] == comp
    old, new = M.Model(xx["files"], orc, xx["ht"]), M.Model(out, orc, xx["ht"])
    for k in xx["keys"]:
        assert new.get(k)[:2] == old.get(k)[:2]
    assert S.scan(new) == S.scan(old)
    from kingdb_amd import get as G
    got = [e.key for c in comp for e in G.read_hstable(out[c])]
    assert got == [e[0] for e in C.entries(view)]


def _verify(tmp_path, xx, orc, files):
    from oracle import hstable
    db = tmp_path / "db"
    db.mkdir()
    for f, b in files.items():
        (db / f).write_bytes(b)
    # hstable_size raised to 32 MiB, as make_golden_getkeys.py does before its own --verify run
    (db / "db_options").write_bytes(hstable.db_options_bytes(orc, 32 << 20, xx["ht"]))
    sp = tmp_path / "stream.bin"
    sp.write_bytes(xx["stream"])
    v = subprocess.run([REF_DB, "--verify", str(db), str(sp), str(xx["part"]), str(xx["hs"]), str(xx["ht"])],
                       capture_output=True, text=True, timeout=120)
    m = re.match(r"verify (\d+) found (\d+) missing (\d+) bad (\d+) iterated (\d+) iterator_bad (\d+) multipart_bad",
                 v.stdout.strip())
    assert m, (v.returncode, v.stdout, v.stderr[-2000:])
    return v.returncode, tuple(int(x) for x in m.groups())


@needs_ref_db
def test_reference_opens_the_compacted_directory(tmp_path, xx, orc):
    names = sorted(xx["files"])
    out, comp = C.directory(xx["files"], names[:2], orc, xx["hs"], 64, xx["ht"])
    rc, (found, missing, bad, iterated, it_bad, mp_bad) = _verify(tmp_path, xx, orc, out)
    z = load_golden("scan.npz")
    assert rc == 0
    assert (found, missing, bad) == (len(xx["keys"]), 0, 0)
    assert (iterated, it_bad, mp_bad) == (int(z["xx__iterated"][0]), 0, 0)


@needs_ref_db
def test_reference_without_the_locked_timestamp(tmp_path, xx, orc):
    """The compacted files stamped with the largest timestamp of the whole
    directory (4) instead of the view's (2): by (timestamp, id) they now sort
    after the two newer files, so the reference takes the compacted -- older --
    entry of every key those files overwrite.  Its Get returns stale values:
    --verify reports them as bad.  That is what LockSequenceTimestamp(the
    view's maximum) prevents."""
    names = sorted(xx["files"])
    top = max(struct.unpack_from("<Q", b, 16)[0] for b in xx["files"].values())
    assert top == 4
    out, comp = C.directory(xx["files"], names[:2], orc, xx["hs"], 64, xx["ht"], timestamp=top)
    # the keys the two newer files overwrite, whose older entry is live in the view
    view = C.view_model(xx["files"], names[:2], orc, xx["ht"])
    newer = M.Model({f: xx["files"][f] for f in names[2:]}, orc, xx["ht"])
    stale = [k for k in xx["keys"] if view.get(k)[0] == 0 and newer.get(k)[0] == 0 and view.get(k)[1] != newer.get(k)[1]]
    assert stale
    rc, (found, missing, bad, iterated, it_bad, mp_bad) = _verify(tmp_path, xx, orc, out)
    assert rc == 1 and missing == 0
    assert bad == len(stale) and found == len(xx["keys"]) - len(stale)
