#!/usr/bin/env python3
"""Snapshots and the compaction's hand-over over the writer's open file
(include/kdb_live.h), measured against the only way to the same answers
without them: cutting the file (close() + refresh()) before every snapshot
and every compaction.

    python tools/bench_live.py [--keys 1048576] [--flush 8192] [--steps 20] [--warmup 3] [--set plain|churn]
                               [--lib PARENT/libkdb_lz4.so]

Database: `--keys` x (16 B key "%016d", 100 B G1 value) written by the device
writer (hstable_size 8 MiB) and left resident; with --set churn 25 % of the
keys are then overwritten and 10 % deleted (the sets of tools/bench_compact.py).
All but the last (warmup + steps) flushes of `--flush` puts are written before
the measurement; every step appends one flush to two writers fed the same
batches -- `live`, whose file stays open, and `cut`, closed at every flush --
and runs the legs one after the other, in one process on one device.  Each
leg reports the median [min, max] of `--steps` steps after `--warmup` warm-up
steps, wall clock (every call ends synchronised) unless said otherwise:
  (b) tail_snapshot   refresh(tail=True) + snapshot(tail=True) on live's index
      cut_snapshot    close() + refresh() + snapshot() on cut and its index
                      (both also split by whether the flush closed a file of
                      live; the file counts both end with are reported)
  (c) carry_open      compact(carry_open=True) on live's index: nothing is cut
      cut_compact     the close() + refresh() timed above + compact() on cut's
                      index: the same code the parent commit runs
      adopt_open      kdb_hstable_dev_adopt_open alone into an empty writer,
                      with the bytes it moved
  (a) locate_plain / locate_tail_snapshot / locate_plain_again /
      locate_tail_snapshot_again / locate_other
                      kdb_index_get_batch of `--keys` uniformly random keys
                      (HIP events) on live's index, the tail included, through
                      kdb_snapshot_get_batch of a tail snapshot of it, both once
                      more, and on the library given by --lib (the parent
                      commit's build: the closed files loaded, the tail set)
                      over the same resident files and query buffers
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


def sync() -> None:
    _lib.check(_lib.load().kdb_lz4_stream_sync(None), "sync")


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


def other_library(path: str):
    lib = ctypes.CDLL(path)
    for name in ("kdb_index_create", "kdb_index_destroy", "kdb_index_load_files", "kdb_index_get_batch",
                 "kdb_index_set_tail"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def get_batch(fn, h, L, st, n: int) -> None:
    _lib.check(fn(h, st, L.keys.ptr, L.p("key_off"), L.p("key_len"), n, 0, 1 << 20, L.scratch.ptr, L.scratch_bytes,
                  L.p("stored_off"), L.p("avail"), L.p("svc"), L.p("size"), L.p("checksum"), L.p("checksum_initial"),
                  L.p("out_off"), L.p("location"), L.p("status"), L.p("summary")), "get_batch")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--flush", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hstable-size", type=int, default=8 << 20)
    ap.add_argument("--set", choices=("plain", "churn"), default="plain")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--lib", help="another build of libkdb_lz4.so (the parent commit's) for the locate_other leg")
    a = ap.parse_args()
    if K.device_count() < 1:
        raise SystemExit("bench_live: no GPU visible to libkdb_lz4.so")
    K.set_device(0)
    lib = _lib.load()
    n, flush, rounds, hs = a.keys, a.flush, a.warmup + a.steps, a.hstable_size
    pool = oracle.g1_pool(oracle.Oracle(), 4 << 20)
    rng = np.random.default_rng(77)
    over = rng.choice(n, n // 4, replace=False) if a.set == "churn" else np.zeros(0, np.int64)
    gone = rng.choice(n, n // 10, replace=False) if a.set == "churn" else np.zeros(0, np.int64)

    def value(j: int, salt: int = 0) -> bytes:
        return pool[(100 * j + 37 * salt) % (len(pool) - 100):][:100].tobytes()

    # the put stream: every key, then the overwrites and the deletes; the measured flushes are its last
    def item(i: int):
        if i < n:
            return b"%016d" % i, value(i)
        if i < n + len(over):
            j = int(over[i - n])
            return b"%016d" % j, value(j, 1)
        return b"%016d" % int(gone[i - n - len(over)]), put.DELETE

    total = n + len(over) + len(gone)
    before = total - rounds * flush
    assert before > 0, "the measured flushes are the last of the database"
    arena = put.DeviceHSTableWriter.arena_bytes(hs, total * 210 + (1 << 20), total)
    # the writer that is cut at every flush writes one header block, footer and file slot per flush more
    w_live = put.DeviceHSTableWriter(hs, 1, arena)
    w_cut = put.DeviceHSTableWriter(hs, 1, arena + (rounds + 2) * (8192 + 36 + 64 + 64))

    def append(lo: int, hi: int) -> None:
        b, m = put.put_entries_device([item(i) for i in range(lo, hi)], 1)
        try:
            for w in (w_live, w_cut):
                w.append_batch(b, m)
            sync()
        finally:
            b.free()

    big = 1 << 17
    for lo in range(0, before, big):
        append(lo, min(lo + big, before))
    ix_live, ix_cut = HSTableIndex.from_resident(w_live), HSTableIndex.from_resident(w_cut)
    ix_live.refresh(tail=True)
    w_cut.close()
    ix_cut.refresh()
    stream = Stream()

    legs = {k: [] for k in ("refresh_tail", "snapshot_tail", "tail_snapshot", "close_refresh", "snapshot_plain",
                            "cut_snapshot", "carry_open", "compact_after_cut", "cut_compact", "adopt_open")}
    closed_a_file, moved = [], []
    for step in range(rounds):
        lo = before + step * flush
        append(lo, lo + flush)
        held = len(ix_live.names)
        t = {}
        snaps = []
        t["refresh_tail"] = wall(lambda: ix_live.refresh(tail=True))
        t["snapshot_tail"] = wall(lambda: snaps.append(ix_live.snapshot(tail=True)))
        t["tail_snapshot"] = t["refresh_tail"] + t["snapshot_tail"]
        t["close_refresh"] = wall(lambda: (w_cut.close(), ix_cut.refresh()))
        t["snapshot_plain"] = wall(lambda: snaps.append(ix_cut.snapshot()))
        t["cut_snapshot"] = t["close_refresh"] + t["snapshot_plain"]
        assert snaps[0].entries == snaps[1].entries == lo + flush
        for s in snaps:
            s.close()
        out = []
        t["carry_open"] = wall(lambda: out.append(ix_live.compact(hstable_size=hs, batch=a.batch, carry_open=True)))
        t["compact_after_cut"] = wall(lambda: out.append(ix_cut.compact(hstable_size=hs, batch=a.batch)))
        t["cut_compact"] = t["close_refresh"] + t["compact_after_cut"]
        if step == 0:
            (w1, n1), (w2, n2) = out
            live = n1.scan_prepare()
            assert live == n2.scan_prepare() and n1.entries >= live
            res_files = {"files_after_carry_open": len(n1.names) + (n1.tail is not None), "files_after_cut_compact": len(n2.names),
                         "live": live}
        for wx, nx in out:
            nx.close()
            wx.free()
        f = w_live.open_file()
        dst = put.DeviceHSTableWriter(hs, 1, int(f.bytes) + int(f.row_bytes) + (1 << 20))
        t["adopt_open"] = wall(lambda: dst.adopt_open(w_live))
        dst.free()
        if step >= a.warmup:
            for k, v in t.items():
                legs[k].append(v)
            closed_a_file.append(len(ix_live.names) > held)
            moved.append(int(f.bytes) + int(f.row_bytes))

    res = {"bench": "live", "set": a.set, "keys": n, "rows": total, "flush": flush, "rows_before": before,
           "steps": a.steps, "warmup": a.warmup, "hstable_size": hs, "files_live": len(ix_live.names) + 1,
           "files_cut": len(ix_cut.names), "tail_rows_at_end": ix_live.tail["rows"],
           "steps_that_closed_a_file": int(sum(closed_a_file)), "adopt_open_bytes": [min(moved), max(moved)]}
    res.update(res_files)

    def report(name: str, v, digits: int = 4) -> None:
        if v:
            res[name + "_ms"] = round(float(np.median(v)), digits)
            res[name + "_ms_range"] = [round(min(v), digits), round(max(v), digits)]
    for k, v in legs.items():
        report(k, v)
    for k in ("tail_snapshot", "cut_snapshot"):
        report(k + "_grew", [x for x, c in zip(legs[k], closed_a_file) if not c])
        report(k + "_closed", [x for x, c in zip(legs[k], closed_a_file) if c])
    res["tail_snapshot_every_step_below_cut_snapshot"] = all(x < y for x, y in zip(legs["tail_snapshot"], legs["cut_snapshot"]))
    res["carry_open_over_cut_compact"] = round(res["carry_open_ms"] / res["cut_compact_ms"], 4)

    # (a) the lookup: the kernel is the parent's; plain and through a tail snapshot, twice, and the other library
    st = stream.ptr
    q = np.random.default_rng(301).integers(0, n, n)
    L = ix_live._lookup([b"%016d" % int(x) for x in q], st, 0, 1 << 20)
    snap = ix_live.snapshot(tail=True)
    assert snap.tail is not None and snap.entries == ix_live.entries
    other = oh = None
    if a.lib:
        other = other_library(a.lib)
        oh = ctypes.c_void_p()
        _lib.check(other.kdb_index_create(1, ctypes.byref(oh)), "kdb_index_create")
        base, off, size, fid = w_live.resident()
        status, e = np.zeros(len(fid) + 1, np.int32), ctypes.c_uint64(0)
        _lib.check(other.kdb_index_load_files(oh, st, base, off.ctypes.data, size.ctypes.data, fid.ctypes.data, len(fid),
                                              status.ctypes.data, ctypes.byref(e)), "kdb_index_load_files")
        f = w_live.open_file()
        _lib.check(other.kdb_index_set_tail(oh, st, base, ctypes.byref(f), 0, None), "kdb_index_set_tail")
    where = {}
    runs = {"plain": lambda: get_batch(lib.kdb_index_get_batch, ix_live.h, L, st, n),
            "tail_snapshot": lambda: get_batch(lib.kdb_snapshot_get_batch, snap.h, L, st, n)}
    if other is not None:
        runs["other"] = lambda: get_batch(other.kdb_index_get_batch, oh, L, st, n)
    for name, run in runs.items():
        run()
        where[name] = (L.meta.download(4 * n, L.off["status"], dtype=np.int32, stream=st).copy(),
                       L.meta.download(8 * n, L.off["location"], dtype=np.uint64, stream=st).copy())
    assert all(np.array_equal(x[0], where["plain"][0]) and np.array_equal(x[1], where["plain"][1]) for x in where.values())
    order = ["plain", "tail_snapshot", "plain", "tail_snapshot"] + (["other"] if other is not None else [])
    names = ["locate_plain", "locate_tail_snapshot", "locate_plain_again", "locate_tail_snapshot_again", "locate_other"]
    look = {k: [] for k in names[:len(order)]}
    for step in range(rounds):
        t = [events(stream, runs[k]) for k in order]
        if step >= a.warmup:
            for k, v in zip(names, t):
                look[k].append(v)
    for k, v in look.items():
        report(k, v)
    res["locate_found"] = int((where["plain"][0] == 0).sum())
    print(json.dumps(res))
    L.free()
    snap.close()
    if other is not None:
        other.kdb_index_destroy(oh)
    for x in (ix_live, ix_cut):
        x.close()
    for w in (w_live, w_cut):
        w.free()


if __name__ == "__main__":
    main()
