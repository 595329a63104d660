#!/usr/bin/env python3
"""Snapshots of a loaded index (include/kdb_snapshot.h), measured: what the
row limit costs the lookup and the scan's prepare, what a snapshot saves over
loading an index of the prefix again, and that the plain lookup has not moved.

    python tools/bench_snapshot.py [--keys 1048576] [--steps 20] [--warmup 3] [--lib PARENT/libkdb_lz4.so]

Database: tools/bench_indexadd.py's -- `--keys` x (16 B key "%016d", 100 B G1
value) written by the device writer (hstable_size 8 MiB: 14 files at 1 Mi keys)
and left resident.  The legs run interleaved, one after the other inside every
step, in one process on one device; each reports the median [min, max] of
`--steps` steps after `--warmup` warm-up steps:
  (a) locate / locate_control / locate_other
               kdb_index_get_batch of `--keys` uniformly random keys (HIP
               events) on a handle over all files, on a second handle loaded
               the same way after every other allocation (the same contents
               elsewhere: how far placement alone moves the number), and on the
               library given by --lib (the parent commit's build) over the same
               resident files and query buffers
  (b) locate_snapshot / locate_again / locate_snapshot_again
               the same keys through kdb_snapshot_get_batch of a snapshot of
               the first handle taken at all files (the limit admits every
               row), then the plain lookup on that handle once more, then the
               snapshot's once more: plain, limited, plain, limited on the same
               buckets, so that what a leg's place in the step does to it (a
               step's first lookup follows the host work of the step before)
               is not taken for the limit's cost or gain
  (c) prepare / prepare_snapshot_half / snapshot_create
               kdb_index_scan_prepare of the whole handle, and
               kdb_snapshot_scan_prepare of a snapshot taken when a handle held
               the first half of the files, the others added since (wall clock:
               synchronous); kdb_snapshot_create + kdb_snapshot_release (host only)
  (d) load_half
               kdb_index_load_files over the first half of the files (wall
               clock): what the reference's NewSnapshot does, against snapshot_create
Prints one JSON line.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kingdb_amd as K  # noqa: E402
from bench_indexadd import Handle, events, other_library, wall, write_resident  # noqa: E402
from kingdb_amd import _lib  # noqa: E402
from kingdb_amd.index import HSTableIndex  # noqa: E402
from kingdb_amd.lz4 import Stream  # noqa: E402


class Snapshot:
    """A kdb_snapshot of a bench_indexadd.Handle."""

    def __init__(self, lib, handle: Handle):
        self.lib = lib
        s = ctypes.c_void_p()
        _lib.check(lib.kdb_snapshot_create(handle.h, ctypes.byref(s)), "kdb_snapshot_create")
        self.s = s

    def locate(self, L, st, n: int) -> None:
        _lib.check(self.lib.kdb_snapshot_get_batch(
            self.s, st, L.keys.ptr, L.p("key_off"), L.p("key_len"), n, 0, 1 << 20, L.scratch.ptr, L.scratch_bytes,
            L.p("stored_off"), L.p("avail"), L.p("svc"), L.p("size"), L.p("checksum"), L.p("checksum_initial"),
            L.p("out_off"), L.p("location"), L.p("status"), L.p("summary")), "kdb_snapshot_get_batch")

    def prepare(self, st) -> int:
        live = ctypes.c_uint64(0)
        _lib.check(self.lib.kdb_snapshot_scan_prepare(self.s, st, 0, ctypes.byref(live), None, None),
                   "kdb_snapshot_scan_prepare")
        return live.value

    def close(self) -> None:
        _lib.check(self.lib.kdb_snapshot_release(self.s), "kdb_snapshot_release")


def prepare(lib, handle: Handle, st) -> int:
    live = ctypes.c_uint64(0)
    _lib.check(lib.kdb_index_scan_prepare(handle.h, st, 0, ctypes.byref(live), None, None), "kdb_index_scan_prepare")
    return live.value


def create_release(lib, handle: Handle) -> None:
    Snapshot(lib, handle).close()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hstable-size", type=int, default=8 << 20)
    ap.add_argument("--lib", help="another build of libkdb_lz4.so (the parent commit's) for the locate_other leg")
    a = ap.parse_args()
    if K.device_count() < 1:
        raise SystemExit("bench_snapshot: no GPU visible to libkdb_lz4.so")
    K.set_device(0)
    lib = _lib.load()
    n = a.keys
    w = write_resident(n, a.hstable_size)
    base, off, size, fid = w.resident()
    nfiles = len(fid)
    assert nfiles >= 2, nfiles
    half = nfiles // 2
    stream = Stream()
    st = stream.ptr

    full = Handle(lib, base, off, size, fid)                # (a) locate, (b) its snapshot, (c) prepare
    assert full.load(st, nfiles) == n
    whole = Snapshot(lib, full)                             # taken at all files: the limit admits every row
    grown = Handle(lib, base, off, size, fid)               # (c) a snapshot at half the files, the rest added since
    rows_half = grown.load(st, half)
    at_half = Snapshot(lib, grown)
    grown.add(st, half, nfiles - half)
    prefix = Handle(lib, base, off, size, fid)              # (d) loaded over the first half, every step
    other = None
    if a.lib:
        other = Handle(other_library(a.lib), base, off, size, fid)
        other.load(st, nfiles)
    control = Handle(lib, base, off, size, fid)             # (a) the same contents in other allocations
    control.load(st, nfiles)

    rng = np.random.default_rng(301)
    q = rng.integers(0, n, n)
    view = HSTableIndex.from_resident(w, stream)            # for its query buffers
    L = view._lookup([b"%016d" % int(x) for x in q], st, 0, 1 << 20)
    where = {}
    for name, h in (("plain", full), ("snapshot", whole), ("control", control), ("other", other)):
        if h is None:
            continue
        h.locate(L, st, n)
        stat = L.meta.download(4 * n, L.off["status"], dtype=np.int32, stream=st)
        assert not stat.any(), f"locate {name}: a key was not found"
        where[name] = L.meta.download(8 * n, L.off["location"], dtype=np.uint64, stream=st).copy()
    assert all(np.array_equal(where["plain"], x) for x in where.values())
    # the snapshot at half the files finds exactly the keys of those files, where a load of them finds them
    prefix.load(st, half)
    found = {}
    for name, h in (("at_half", at_half), ("prefix", prefix)):
        h.locate(L, st, n)
        found[name] = (L.meta.download(4 * n, L.off["status"], dtype=np.int32, stream=st).copy(),
                       L.meta.download(8 * n, L.off["location"], dtype=np.uint64, stream=st).copy())
    assert all(np.array_equal(x, y) for x, y in zip(found["at_half"], found["prefix"]))
    assert int((found["at_half"][0] == 0).sum()) == int((q < rows_half).sum())
    live_all, live_half = prepare(lib, full, st), at_half.prepare(st)
    assert (live_all, live_half) == (n, rows_half)

    legs = {k: [] for k in ("locate", "locate_snapshot", "locate_again", "locate_snapshot_again", "locate_control", "locate_other", "prepare",
                            "prepare_snapshot_half", "snapshot_create", "load_half")}
    for step in range(a.warmup + a.steps):
        t = {"locate": events(stream, lambda: full.locate(L, st, n)),
             "locate_snapshot": events(stream, lambda: whole.locate(L, st, n)),
             "locate_again": events(stream, lambda: full.locate(L, st, n)),
             "locate_snapshot_again": events(stream, lambda: whole.locate(L, st, n)),
             "locate_control": events(stream, lambda: control.locate(L, st, n))}
        if other is not None:
            t["locate_other"] = events(stream, lambda: other.locate(L, st, n))
        t["prepare"] = wall(lambda: prepare(lib, full, st))
        t["prepare_snapshot_half"] = wall(lambda: at_half.prepare(st))
        t["snapshot_create"] = wall(lambda: create_release(lib, grown))
        t["load_half"] = wall(lambda: prefix.load(st, half))
        if step >= a.warmup:
            for k, v in t.items():
                legs[k].append(v)

    res = {"bench": "snapshot", "keys": n, "files": nfiles, "files_at_half": half, "rows_at_half": rows_half,
           "file_bytes": int(size.sum()), "steps": a.steps, "warmup": a.warmup}
    for k, v in legs.items():
        if v:
            digits = 6 if k == "snapshot_create" else 4
            res[k + "_ms"] = round(float(np.median(v)), digits)
            res[k + "_ms_range"] = [round(min(v), digits), round(max(v), digits)]
    inside = lambda x, lo_hi: lo_hi[0] <= x <= lo_hi[1]  # noqa: E731
    if other is not None:
        res["locate_inside_other"] = inside(res["locate_ms"], res["locate_other_ms_range"])
        res["locate_control_inside_other"] = inside(res["locate_control_ms"], res["locate_other_ms_range"])
    plain, limited = legs["locate"] + legs["locate_again"], legs["locate_snapshot"] + legs["locate_snapshot_again"]
    res["snapshot_every_step_above_plain"] = min(limited) > max(plain)
    res["snapshot_again_every_step_above_plain_again"] = min(legs["locate_snapshot_again"]) > max(legs["locate_again"])
    res["locate_snapshot_again_over_plain_again"] = round(res["locate_snapshot_again_ms"] / res["locate_again_ms"], 4)
    res["load_half_over_snapshot_create"] = round(res["load_half_ms"] / max(res["snapshot_create_ms"], 1e-6), 1)
    print(json.dumps(res))
    L.free()
    view.close()
    for s in (whole, at_half):
        s.close()
    for h in (full, grown, prefix, control, other):
        if h is not None:
            h.close()
    w.free()


if __name__ == "__main__":
    main()
