#!/usr/bin/env python3
"""Reading the writer's open file through the index (kdb_index_set_tail),
measured against the only way to the same visibility without it: closing the
file after every flush and adding it (close() + refresh()).

    python tools/bench_indextail.py [--keys 1048576] [--flush 8192] [--steps 20] [--warmup 3] [--lib OTHER/libkdb_lz4.so]

Database: `--keys` x (16 B key "%016d", 100 B G1 value) written by the device
writer (put.DeviceHSTableWriter, hstable_size 8 MiB) and left resident.  All
but the last (warmup + steps) flushes are written before the measurement; every
step then appends one flush of `--flush` puts to three writers fed the same
batches, and runs the legs one after the other, in one process on one device.
Each leg reports the median [min, max] of `--steps` steps after `--warmup`
warm-up steps:
  tail         refresh(tail=True) on an index of the first writer (wall clock:
               synchronous): the files closed by the flush are added and the
               rows the flush staged are parsed
  tail_reparse the same on a second index of that writer with
               KDB_INDEX_TAIL_REPARSE: the whole staging parsed every time
               (both also split by whether the flush closed a file: then the
               closed file is added first and the tail is a new file's, the
               same work in either leg)
  close_add    close() + refresh() on the second writer and its index: the
               file is cut at every flush
After the last step the third writer, which holds byte for byte the files and
the open file of the first, is closed and an index refresh()ed over it: the
same rows, every one in a closed file.  Then, interleaved in every step of a
second loop of the same length:
  locate_tail / locate_closed
               kdb_index_get_batch of `--keys` uniformly random keys (HIP
               events) on the first writer's index, the tail included, and on
               the closed twin's
  locate_other the closed twin's files on the library given by --lib (another
               build, such as the parent commit's), same query buffers
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


def other_library(path: str):
    lib = ctypes.CDLL(path)
    for name in ("kdb_index_create", "kdb_index_destroy", "kdb_index_load_files", "kdb_index_get_batch"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def locate(lib, h, L, st, n: int) -> None:
    _lib.check(lib.kdb_index_get_batch(
        h, st, L.keys.ptr, L.p("key_off"), L.p("key_len"), n, 0, 1 << 20, L.scratch.ptr, L.scratch_bytes,
        L.p("stored_off"), L.p("avail"), L.p("svc"), L.p("size"), L.p("checksum"), L.p("checksum_initial"),
        L.p("out_off"), L.p("location"), L.p("status"), L.p("summary")), "kdb_index_get_batch")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--flush", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hstable-size", type=int, default=8 << 20)
    ap.add_argument("--lib", help="another build of libkdb_lz4.so for the locate_other leg")
    a = ap.parse_args()
    if K.device_count() < 1:
        raise SystemExit("bench_indextail: no GPU visible to libkdb_lz4.so")
    K.set_device(0)
    lib = _lib.load()
    n, flush, rounds = a.keys, a.flush, a.warmup + a.steps
    before = n - rounds * flush
    assert before > 0, "the measured flushes are the last of the database"
    orc = oracle.Oracle()
    pool = oracle.g1_pool(orc, 4 << 20)

    def puts_of(lo: int, hi: int):
        return [(b"%016d" % j, pool[(100 * j) % (len(pool) - 100):][:100].tobytes()) for j in range(lo, hi)]

    big = 1 << 17
    bound = sum(100 * m + 16 * m + m * 72 + (100 * m // 65536 + m + 1) * 16 + 64      # put.entries_bound
                for m in [min(big, before - i) for i in range(0, before, big)] + [flush] * rounds)
    # the twin that closes at every flush writes one header block, footer and file slot per flush more
    arena = put.DeviceHSTableWriter.arena_bytes(a.hstable_size, bound, n)
    writers = [put.DeviceHSTableWriter(a.hstable_size, 1, arena + (rounds + 2) * (8192 + 36 + 64 + 64))
               for _ in range(3)]
    w_tail, w_cut, w_twin = writers

    def append(lo: int, hi: int) -> None:
        b, m = put.put_entries_device(puts_of(lo, hi), 1)
        try:
            for w in writers:
                w.append_batch(b, m)
            _lib.check(lib.kdb_lz4_stream_sync(None), "sync")
        finally:
            b.free()

    for i in range(0, before, big):
        append(i, min(i + big, before))
    ix_tail = HSTableIndex.from_resident(w_tail)
    ix_reparse = HSTableIndex.from_resident(w_tail)
    ix_cut = HSTableIndex.from_resident(w_cut)
    ix_tail.refresh(tail=True)
    ix_reparse.refresh(tail=True, reparse=True)
    w_cut.close()
    ix_cut.refresh()
    assert ix_tail.entries == ix_reparse.entries == ix_cut.entries == before

    legs = {k: [] for k in ("tail", "tail_reparse", "close_add", "locate_tail", "locate_closed", "locate_other")}
    parsed, closed_a_file = [], []
    for step in range(rounds):
        lo = before + step * flush
        append(lo, lo + flush)
        held = len(ix_tail.names)
        t = {"tail": wall(lambda: ix_tail.refresh(tail=True))}
        parsed.append(ix_tail.tail_stats()[4])
        t["tail_reparse"] = wall(lambda: ix_reparse.refresh(tail=True, reparse=True))
        t["close_add"] = wall(lambda: (w_cut.close(), ix_cut.refresh()))
        assert ix_tail.entries == ix_reparse.entries == ix_cut.entries == lo + flush
        if step >= a.warmup:
            closed_a_file.append(len(ix_tail.names) > held)
            for k, v in t.items():
                legs[k].append(v)
    tail = ix_tail.tail
    files_tail, files_cut = len(ix_tail.names), len(ix_cut.names)

    # the same rows, every one in a closed file: the twin closed now
    w_twin.close()
    ix_closed = HSTableIndex.from_resident(w_twin)
    assert ix_closed.entries == ix_tail.entries == n
    assert all(np.array_equal(x, y) for x, y in zip(ix_tail.pairs(), ix_closed.pairs()))
    other = h_other = None
    if a.lib:
        other = other_library(a.lib)
        h_other = ctypes.c_void_p()
        _lib.check(other.kdb_index_create(1, ctypes.byref(h_other)), "kdb_index_create")
        base, off, size, fid = w_twin.resident()
        status = np.zeros(len(fid) + 1, np.int32)
        e = ctypes.c_uint64(0)
        _lib.check(other.kdb_index_load_files(h_other, None, base, off.ctypes.data, size.ctypes.data, fid.ctypes.data,
                                              len(fid), status.ctypes.data, ctypes.byref(e)), "kdb_index_load_files")
        assert e.value == n and not status.any()

    stream = Stream()
    st = stream.ptr
    rng = np.random.default_rng(301)
    q = rng.integers(0, n, n)
    L = ix_tail._lookup([b"%016d" % int(x) for x in q], st, 0, 1 << 20)
    where = []
    for which, h in ((lib, ix_tail.h), (lib, ix_closed.h), (other, h_other)):
        if h is None:
            continue
        locate(which, h, L, st, n)
        stat = L.meta.download(4 * n, L.off["status"], dtype=np.int32, stream=st)
        assert not stat.any(), "a key was not found"
        where.append(L.meta.download(8 * n, L.off["location"], dtype=np.uint64, stream=st).copy())
    assert all(np.array_equal(where[0], x) for x in where)
    for step in range(rounds):
        t = {"locate_tail": events(stream, lambda: locate(lib, ix_tail.h, L, st, n)),
             "locate_closed": events(stream, lambda: locate(lib, ix_closed.h, L, st, n))}
        if h_other is not None:
            t["locate_other"] = events(stream, lambda: locate(other, h_other, L, st, n))
        if step >= a.warmup:
            for k, v in t.items():
                legs[k].append(v)

    res = {"bench": "indextail", "keys": n, "flush": flush, "rows_before": before, "steps": a.steps,
           "warmup": a.warmup, "files_closed_with_tail": files_tail, "files_closed_at_every_flush": files_cut,
           "tail_rows_at_end": tail["rows"] if tail else 0,
           "rows_parsed_per_step": [min(parsed), max(parsed)]}
    for k, v in legs.items():
        if v:
            res[k + "_ms"] = round(float(np.median(v)), 4)
            res[k + "_ms_range"] = [round(min(v), 4), round(max(v), 4)]
    res["tail_every_step_below_close_add"] = max(legs["tail"]) < min(legs["close_add"])
    res["tail_every_step_below_reparse"] = max(legs["tail"]) < min(legs["tail_reparse"])
    # a flush that closes a file of hstable_size makes refresh(tail=True) add that file first, and the tail is
    # then a new file's: both tail legs parse the same few rows.  The steps apart, by whether that happened:
    res["steps_that_closed_a_file"] = sum(closed_a_file)
    for which, pick in (("grew", False), ("closed", True)):
        for k in ("tail", "tail_reparse", "close_add"):
            v = [x for x, c in zip(legs[k], closed_a_file) if c == pick]
            if v:
                res[f"{k}_{which}_ms"] = round(float(np.median(v)), 4)
                res[f"{k}_{which}_ms_range"] = [round(min(v), 4), round(max(v), 4)]
    if any(closed_a_file) and not all(closed_a_file):
        res["tail_grew_every_step_below_close_add"] = res["tail_grew_ms_range"][1] < min(legs["close_add"])
        res["tail_grew_every_step_below_reparse_grew"] = (res["tail_grew_ms_range"][1] <
                                                          res["tail_reparse_grew_ms_range"][0])
    inside = lambda x, lo_hi: lo_hi[0] <= x <= lo_hi[1]  # noqa: E731
    res["locate_medians_inside_each_other"] = (inside(res["locate_tail_ms"], res["locate_closed_ms_range"]) and
                                               inside(res["locate_closed_ms"], res["locate_tail_ms_range"]))
    if h_other is not None:
        res["locate_tail_inside_other"] = inside(res["locate_tail_ms"], res["locate_other_ms_range"])
    print(json.dumps(res))
    L.free()
    if h_other is not None:
        other.kdb_index_destroy(h_other)
    for x in (ix_tail, ix_reparse, ix_cut, ix_closed):
        x.close()
    for w in writers:
        w.free()


if __name__ == "__main__":
    main()
