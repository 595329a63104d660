#!/usr/bin/env python3
"""Adding a newly closed file to a loaded index, measured against loading
every file again (kdb_index_add_files against kdb_index_load_files).

    python tools/bench_indexadd.py [--keys 1048576] [--steps 20] [--warmup 3] [--lib OTHER/libkdb_lz4.so]

Database: `--keys` x (16 B key "%016d", 100 B G1 value) written by the device
writer (put.DeviceHSTableWriter, hstable_size 8 MiB) and left resident.  The
legs run interleaved, one after the other inside every step, in one process on
one device; each reports the median [min, max] of `--steps` steps after
`--warmup` warm-up steps:
  load         kdb_index_load_files over all files (wall clock: synchronous)
  add          an index over all files but the last (untimed), then
               kdb_index_add_files of the last one (wall clock), at a split
               where the bucket count stays: if it happens to double there,
               files are dropped from the end until it does not
  locate_loaded / locate_added
               kdb_index_get_batch of `--keys` uniformly random keys (HIP
               events) on an index made by one load, and on one made by a load
               of the first file plus one add per further file
  locate_reloaded
               the first of those two on a second handle loaded the same way
               after all the others: the same contents in other allocations,
               which shows how far the placement alone moves the number
  locate_other the first of those two on the library given by --lib (another
               build, such as the parent commit's), over the same resident
               files and the same query buffers
Prints one JSON line.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kingdb_amd as K  # noqa: E402
import oracle  # noqa: E402
from kingdb_amd import _lib, put  # noqa: E402
from kingdb_amd.index import HSTableIndex  # noqa: E402
from kingdb_amd.lz4 import Event, Stream  # noqa: E402


def write_resident(nkeys: int, hstable_size: int):
    orc = oracle.Oracle()
    pool = oracle.g1_pool(orc, 4 << 20)
    step = 1 << 17
    bound = 0
    for i in range(0, nkeys, step):
        m = min(step, nkeys - i)
        bound += 100 * m + 16 * m + m * 72 + (100 * m // 65536 + m + 1) * 16 + 64     # put.entries_bound
    w = put.DeviceHSTableWriter(hstable_size, 1, put.DeviceHSTableWriter.arena_bytes(hstable_size, bound, nkeys))
    for i in range(0, nkeys, step):
        m = min(step, nkeys - i)
        puts = [(b"%016d" % j, pool[(100 * j) % (len(pool) - 100):][:100].tobytes()) for j in range(i, i + m)]
        b, n = put.put_entries_device(puts, 1)
        try:
            w.append_batch(b, n)
            _lib.check(_lib.load().kdb_lz4_stream_sync(None), "sync")
        finally:
            b.free()
    w.close()
    return w


class Handle:
    """A kdb_index of `lib` over files of the writer's arena."""

    def __init__(self, lib, base, off, size, fid):
        self.lib, self.base = lib, base
        self.off, self.size, self.fid = (np.ascontiguousarray(off, np.uint64), np.ascontiguousarray(size, np.uint64),
                                         np.ascontiguousarray(fid, np.uint32))
        h = ctypes.c_void_p()
        _lib.check(lib.kdb_index_create(1, ctypes.byref(h)), "kdb_index_create")
        self.h = h
        self.status = np.zeros(len(self.fid) + 1, np.int32)

    def load(self, st, n: int) -> int:
        e = ctypes.c_uint64(0)
        _lib.check(self.lib.kdb_index_load_files(self.h, st, self.base, self.off.ctypes.data, self.size.ctypes.data,
                                                 self.fid.ctypes.data, n, self.status.ctypes.data, ctypes.byref(e)),
                   "kdb_index_load_files")
        assert not self.status[:n].any()
        return e.value

    def add(self, st, first: int, n: int) -> int:
        e = ctypes.c_uint64(0)
        _lib.check(self.lib.kdb_index_add_files(self.h, st, self.base, self.off[first:].ctypes.data,
                                                self.size[first:].ctypes.data, self.fid[first:].ctypes.data, n, 0,
                                                self.status.ctypes.data, ctypes.byref(e)), "kdb_index_add_files")
        assert not self.status[:n].any()
        return e.value

    def locate(self, L, st, n: int) -> None:
        _lib.check(self.lib.kdb_index_get_batch(
            self.h, st, L.keys.ptr, L.p("key_off"), L.p("key_len"), n, 0, 1 << 20, L.scratch.ptr, L.scratch_bytes,
            L.p("stored_off"), L.p("avail"), L.p("svc"), L.p("size"), L.p("checksum"), L.p("checksum_initial"),
            L.p("out_off"), L.p("location"), L.p("status"), L.p("summary")), "kdb_index_get_batch")

    def close(self) -> None:
        self.lib.kdb_index_destroy(self.h)


def other_library(path: str):
    lib = ctypes.CDLL(path)
    for name in ("kdb_index_create", "kdb_index_destroy", "kdb_index_load_files", "kdb_index_get_batch"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def buckets(rows: int) -> int:
    b = 2
    while b < 2 * rows:
        b <<= 1
    return b


def wall(fn) -> float:
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def events(stream: Stream, fn) -> float:
    stream.sync()
    a, b = Event(), Event()
    a.record(stream)
    fn()
    b.record(stream)
    return a.elapsed_ms(b)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hstable-size", type=int, default=8 << 20)
    ap.add_argument("--lib", help="another build of libkdb_lz4.so for the locate_other leg")
    a = ap.parse_args()
    if K.device_count() < 1:
        raise SystemExit("bench_indexadd: no GPU visible to libkdb_lz4.so")
    K.set_device(0)
    lib = _lib.load()
    n = a.keys
    w = write_resident(n, a.hstable_size)
    base, off, size, fid = w.resident()
    nfiles = len(fid)
    assert nfiles >= 3, nfiles
    stream = Stream()
    st = stream.ptr

    # rows of the first m files, for the split of the add legs
    probe = Handle(lib, base, off, size, fid)
    rows = [probe.load(st, m) for m in range(nfiles + 1)]
    probe.close()
    assert rows[nfiles] == n
    used = nfiles
    while used > 2 and buckets(rows[used - 1]) != buckets(rows[used]):
        used -= 1
    assert buckets(rows[used - 1]) == buckets(rows[used]), "no split of the files keeps the bucket count"

    full = Handle(lib, base, off, size, fid)               # load: all files, every step
    grown = Handle(lib, base, off, size, fid)              # add
    loaded = Handle(lib, base, off, size, fid)             # locate_loaded
    added = Handle(lib, base, off, size, fid)              # locate_added
    loaded.load(st, nfiles)
    added.load(st, 1)
    for f in range(1, nfiles):
        added.add(st, f, 1)
    other = None
    if a.lib:
        other = Handle(other_library(a.lib), base, off, size, fid)
        other.load(st, nfiles)

    reloaded = Handle(lib, base, off, size, fid)           # locate_reloaded
    reloaded.load(st, nfiles)

    rng = np.random.default_rng(301)
    q = rng.integers(0, n, n)
    view = HSTableIndex.from_resident(w, stream)           # for its query buffers
    L = view._lookup([b"%016d" % int(x) for x in q], st, 0, 1 << 20)
    where = {}
    for name, h in (("loaded", loaded), ("added", added), ("reloaded", reloaded), ("other", other)):
        if h is None:
            continue
        h.locate(L, st, n)
        stat = L.meta.download(4 * n, L.off["status"], dtype=np.int32, stream=st)
        assert not stat.any(), f"locate_{name}: a key was not found"
        where[name] = L.meta.download(8 * n, L.off["location"], dtype=np.uint64, stream=st).copy()
    assert all(np.array_equal(where["loaded"], x) for x in where.values())

    legs = {k: [] for k in ("load", "add", "locate_loaded", "locate_added", "locate_reloaded",
                            "locate_other")}
    for step in range(a.warmup + a.steps):
        t = {"load": wall(lambda: full.load(st, used))}
        grown.load(st, used - 1)
        t["add"] = wall(lambda: grown.add(st, used - 1, 1))
        t["locate_loaded"] = events(stream, lambda: loaded.locate(L, st, n))
        t["locate_added"] = events(stream, lambda: added.locate(L, st, n))
        t["locate_reloaded"] = events(stream, lambda: reloaded.locate(L, st, n))
        if other is not None:
            t["locate_other"] = events(stream, lambda: other.locate(L, st, n))
        if step >= a.warmup:
            for k, v in t.items():
                legs[k].append(v)

    res = {"bench": "indexadd", "keys": n, "files": nfiles, "files_in_add_legs": used,
           "rows_before_add": rows[used - 1], "rows_added": rows[used] - rows[used - 1], "buckets": buckets(rows[used]),
           "file_bytes": int(size.sum()), "steps": a.steps, "warmup": a.warmup}
    for k, v in legs.items():
        if v:
            res[k + "_ms"] = round(float(np.median(v)), 4)
            res[k + "_ms_range"] = [round(min(v), 4), round(max(v), 4)]
    inside = lambda x, lo_hi: lo_hi[0] <= x <= lo_hi[1]  # noqa: E731
    res["add_every_step_below_load"] = max(legs["add"]) < min(legs["load"])
    res["locate_medians_inside_each_other"] = (inside(res["locate_loaded_ms"], res["locate_added_ms_range"]) and
                                               inside(res["locate_added_ms"], res["locate_loaded_ms_range"]))
    if other is not None:
        res["locate_loaded_inside_other"] = inside(res["locate_loaded_ms"], res["locate_other_ms_range"])
    print(json.dumps(res))
    L.free()
    view.close()
    for h in (full, grown, loaded, added, reloaded, other):
        if h is not None:
            h.close()
    w.free()


if __name__ == "__main__":
    main()
