#!/usr/bin/env python3
"""Compaction by copy measured against the compaction that decodes and
compresses again (HSTableIndex.compact_copy against compacted_device), the
hand-over, and the lookup on the index it leaves.

    python tools/bench_compact.py [--keys 1048576] [--steps 20] [--warmup 3] [--set plain|churn|multipart]

Data sets, written by the device writer and left resident:
  plain      `--keys` x (16 B key "%016d", 100 B G1 value), hstable_size 8 MiB,
             every row live (the set of tools/bench_indexadd.py)
  churn      the same, then 25 % of the keys overwritten and 10 % deleted
  multipart  `--values` (2 000) x 256 KiB G1 values sent in 64 KiB parts,
             hstable_size 32 MiB
The legs run interleaved, one after the other inside every step, in one
process on one device; each reports the median [min, max] of `--steps` steps
after `--warmup` warm-up steps, wall clock (every call ends synchronised):
  compacted_device   the yardstick: scan, decode, compress again, write
  compact_copy       scan, plan, copy, write
  hand_over          kdb_hstable_dev_adopt of half the files (by count) into a
                     writer holding the compaction of the other half
  locate_old / locate_new
                     kdb_index_get_batch of `--keys` uniformly random keys (HIP
                     events) on the old index and on the one compact() returned
and once, outside the steps, the copy kernel's own time per window (HIP events
inside kdb_compact_entries_batch_timed) with its algorithmic bytes, 2 x entry
bytes, against the 8.0 TB/s peak.  Prints one JSON line.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kingdb_amd as K  # noqa: E402
import oracle  # noqa: E402
from kingdb_amd import _lib, put  # noqa: E402
from kingdb_amd.index import HSTableIndex, _Lookup, _a8  # noqa: E402
from kingdb_amd.lz4 import DeviceBuffer, Event, Stream  # noqa: E402

PEAK_TBS = 8.0


def sync() -> None:
    _lib.check(_lib.load().kdb_lz4_stream_sync(None), "sync")


def write(batches, hstable_size: int, bound: int, n: int):
    w = put.DeviceHSTableWriter(hstable_size, 1, put.DeviceHSTableWriter.arena_bytes(hstable_size, bound, n))
    for puts in batches():
        b, m = put.put_entries_device(puts, 1)
        try:
            w.append_batch(b, m)
            sync()
        finally:
            b.free()
    w.close()
    return w


def small_set(nkeys: int, churn: bool):
    pool = oracle.g1_pool(oracle.Oracle(), 4 << 20)
    step = 1 << 17
    rng = np.random.default_rng(77)
    over = rng.choice(nkeys, nkeys // 4, replace=False) if churn else np.zeros(0, np.int64)
    gone = rng.choice(nkeys, nkeys // 10, replace=False) if churn else np.zeros(0, np.int64)

    def value(j: int, salt: int = 0) -> bytes:
        return pool[(100 * j + 37 * salt) % (len(pool) - 100):][:100].tobytes()

    def batches():
        for i in range(0, nkeys, step):
            yield [(b"%016d" % j, value(j)) for j in range(i, min(i + step, nkeys))]
        for i in range(0, len(over), step):
            yield [(b"%016d" % int(j), value(int(j), 1)) for j in over[i:i + step]]
        for i in range(0, len(gone), step):
            yield [(b"%016d" % int(j), put.DELETE) for j in gone[i:i + step]]

    n = nkeys + len(over) + len(gone)
    return write(batches, 8 << 20, n * 210 + (1 << 20), n)      # put.entries_bound and some room


def multipart_set(nvalues: int):
    pool = oracle.g1_pool(oracle.Oracle(), 8 << 20)
    size, part, step = 256 << 10, 64 << 10, 100

    def batches():
        for i in range(0, nvalues, step):
            yield [(b"%016d" % j, pool[(4099 * j) % (len(pool) - size):][:size].tobytes(), [part] * (size // part))
                   for j in range(i, min(i + step, nvalues))]

    return write(batches, 32 << 20, nvalues * (size + 256) + (1 << 20), nvalues)


def wall(fn) -> float:
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def events(stream: Stream, fn) -> float:
    stream.sync()
    a, b = Event(), Event()
    a.record(stream)
    fn()
    b.record(stream)
    return a.elapsed_ms(b)


def copy_kernel_time(ix: HSTableIndex, batch: int):
    """(ms, entry bytes) of the copy kernel over every window, once."""
    lib = _lib.load()
    live = ix.scan_prepare()
    kmax = ix._scan[3]
    n0 = min(batch, max(live, 1))
    L = _Lookup(n0, n0 * kmax)
    sb = int(lib.kdb_compact_scratch_bytes(n0))
    scratch, po = DeviceBuffer(sb), DeviceBuffer(n0 * 32 + 64)
    o = po.ptr
    e_off, hashed, e_len, kind, status, total = o, o + 8 * n0, o + 16 * n0, o + 20 * n0, o + 24 * n0, o + _a8(28 * n0)
    ms_sum, bytes_sum, entries = 0.0, 0, None
    try:
        for first in range(0, live, batch):
            n = min(batch, live - first)
            ix.run_scan(L, None, first, n, 1 << 62)
            args = (L.keys.ptr, L.keys.nbytes, L.p("key_off"), L.p("key_len"), L.p("stored_off"), L.p("avail"),
                    L.p("svc"), L.p("size"), L.p("checksum"), L.p("status"), n)
            _lib.check(lib.kdb_compact_plan_batch(None, *args, ix.files.nbytes, 1, scratch.ptr, sb, e_off, e_len, total,
                                                  hashed, kind, status), "plan")
            t = int(po.download(8, total - o, dtype=np.uint64)[0])
            if entries is None or entries.nbytes < t + 64:
                if entries is not None:
                    entries.free()
                entries = DeviceBuffer(t + t // 8 + 64)
            ms, refused = ctypes.c_float(0), ctypes.c_uint32(0)
            for _ in range(2):                                # the second run is the one reported
                _lib.check(lib.kdb_compact_entries_batch_timed(
                    None, ix.files.ptr, ix.files.nbytes, *args, 1, scratch.ptr, sb, entries.ptr, entries.nbytes - 64,
                    e_off, e_len, total, hashed, kind, status, ctypes.byref(refused), ctypes.byref(ms)), "copy")
            assert refused.value == 0
            ms_sum += ms.value
            bytes_sum += t
    finally:
        for b in (L, scratch, po, entries):
            if b is not None:
                b.free()
    return ms_sum, bytes_sum


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", choices=("plain", "churn", "multipart"), default="plain")
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--values", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=65536)
    a = ap.parse_args()
    if K.device_count() < 1:
        raise SystemExit("bench_compact: no GPU visible to libkdb_lz4.so")
    K.set_device(0)
    multipart = a.set == "multipart"
    hs = (32 << 20) if multipart else (8 << 20)
    batch = 64 if multipart else a.batch
    w = multipart_set(a.values) if multipart else small_set(a.keys, a.set == "churn")
    ix = HSTableIndex.from_resident(w)
    live = ix.scan_prepare()
    nfiles = len(ix.names)
    res = {"bench": "compact", "set": a.set, "files": nfiles, "rows": ix.entries, "live": live,
           "file_bytes": int(ix.file_size.sum()), "hstable_size": hs, "batch": batch, "steps": a.steps,
           "warmup": a.warmup}

    # the hand-over leg: a compaction of the first half of the files, adopting the other half
    half = max(nfiles // 2, 1)
    rest = list(range(half, nfiles))
    spare = int(sum((int(s) + 63) & ~63 for s in ix.file_size[rest])) + 64

    stream = Stream()
    L = None
    new_w = new_ix = None
    if not multipart:
        rng = np.random.default_rng(301)
        nq = a.keys
        L = ix._lookup([b"%016d" % int(x) for x in rng.integers(0, a.keys, nq)], stream.ptr, 0, 1 << 20)
        new_w, new_ix = ix.compact(hstable_size=hs, batch=batch)
        res["files_after"] = len(new_ix.names)
        res["file_bytes_after"] = int(new_ix.file_size.sum())
        old_status = L.meta.download(4 * nq, L.off["status"], dtype=np.int32, stream=stream.ptr).copy()
        new_ix.run_lookup(L, stream.ptr, nq)
        new_status = L.meta.download(4 * nq, L.off["status"], dtype=np.int32, stream=stream.ptr)
        # a delete the compaction dropped reads NOTFOUND (-3) instead of DELETED (-4)
        assert np.array_equal(np.where(old_status == -4, -3, old_status), new_status)

    legs = {k: [] for k in ("compacted_device", "compact_copy", "hand_over", "locate_old", "locate_new")}
    for step in range(a.warmup + a.steps):
        t = {}
        out = []
        t["compacted_device"] = wall(lambda: out.append(ix.compacted_device(hs, batch)))
        t["compact_copy"] = wall(lambda: out.append(ix.compact_copy(hs, batch)))
        if step == 0:
            res["compacted_device_file_bytes"] = sum(int(s) for s in out[0].resident()[2])
            res["compact_copy_file_bytes"] = sum(int(s) for s in out[1].resident()[2])
        for x in out:
            x.free()
        if not multipart and nfiles >= 2:
            # the compaction of the first half is made untimed; the adopt is the leg
            snap_w = put.DeviceHSTableWriter(hs, 1, spare + (1 << 20), filetype=2, timestamp_lock=half)
            t["hand_over"] = wall(lambda: snap_w.adopt(nfiles + 1, ix.files.ptr, ix.file_off[rest], ix.file_size[rest],
                                                      ix.fileid[rest]))
            snap_w.free()
            t["locate_old"] = events(stream, lambda: ix.run_lookup(L, stream.ptr, a.keys))
            t["locate_new"] = events(stream, lambda: new_ix.run_lookup(L, stream.ptr, a.keys))
        if step >= a.warmup:
            for k, v in t.items():
                legs[k].append(v)
    for k, v in legs.items():
        if v:
            res[k + "_ms"] = round(float(np.median(v)), 4)
            res[k + "_ms_range"] = [round(min(v), 4), round(max(v), 4)]
    res["hand_over_bytes"] = spare - 64 if legs["hand_over"] else 0
    res["copy_every_step_below_compacted_device"] = max(legs["compact_copy"]) < min(legs["compacted_device"])
    ms, nbytes = copy_kernel_time(ix, batch)
    res["copy_kernel_ms"] = round(ms, 4)
    res["entry_bytes"] = nbytes
    if ms > 0:
        res["copy_kernel_tbs"] = round(2 * nbytes / (ms * 1e-3) / 1e12, 4)
        res["copy_kernel_of_peak"] = round(2 * nbytes / (ms * 1e-3) / 1e12 / PEAK_TBS, 4)
    print(json.dumps(res))
    if L is not None:
        L.free()
    for x in (new_ix, ix):
        if x is not None:
            x.close()
    for x in (new_w, w):
        if x is not None:
            x.free()


if __name__ == "__main__":
    main()
