#!/usr/bin/env python3
"""Get by key on the GPU, measured: index load, lookup alone, lookup + decode.

    python tools/bench_getkeys.py [--keys 1048576] [--steps 20] [--warmup 3] [--no-reference]

Database: `--keys` x (16 B key "%016d", 100 B G1 value) written by this
project's write path (put.put_entries + HSTableWriter, default options).
Timed with HIP events after the warm-up steps:
  load     kdb_index_load_files on the resident files (synchronous: wall clock)
  locate   kdb_index_get_batch of `--keys` uniformly random keys
  get      the same lookups + the summary download + kdb_get_values_batch
  scan     kdb_index_scan_prepare (synchronous: wall clock), then
           kdb_index_scan_batch + the same decode over all live entries in
           windows of `--window`, and `get` of the same keys in the same windows
           beside it; each step timed on its own, median and range reported
           (`--no-scan` leaves the leg out)
Reference leg, where oracle/_ref/ref_db exists: `ref_db --readrandom` (the
reference's Database::Get from 1 and 16 client threads) on the same files,
saved with kdb_hstable_writer_save.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kingdb_amd as K  # noqa: E402
import oracle  # noqa: E402
from kingdb_amd import _lib, put  # noqa: E402
from kingdb_amd.index import HSTableIndex  # noqa: E402
from kingdb_amd.lz4 import DeviceBuffer, Event, Stream  # noqa: E402

REF_DB = os.path.join(ROOT, "oracle", "_ref", "ref_db")


def write_database(nkeys: int, directory: str):
    orc = oracle.Oracle()
    pool = oracle.g1_pool(orc, 4 << 20)
    w = put.HSTableWriter()
    step = 1 << 17
    for i in range(0, nkeys, step):
        m = min(step, nkeys - i)
        vals = [pool[(100 * j) % (len(pool) - 100):][:100].tobytes() for j in range(i, i + m)]
        w.append(put.put_entries([(b"%016d" % (i + j), vals[j]) for j in range(m)]))
    w.close()
    files = w.files()
    w.save(directory)
    with open(os.path.join(directory, "db_options"), "wb") as f:
        f.write(put.db_options())
    return files, pool


def timed(stream: Stream, steps: int, warmup: int, fn) -> float:
    """Milliseconds per step of fn(), HIP events around `steps` calls."""
    for _ in range(warmup):
        fn()
    stream.sync()
    a, b = Event(), Event()
    a.record(stream)
    for _ in range(steps):
        fn()
    b.record(stream)
    return a.elapsed_ms(b) / steps


def reference_leg(directory: str, nkeys: int, threads: int):
    r = subprocess.run([REF_DB, "--readrandom", directory, str(nkeys), str(nkeys), str(threads)],
                       capture_output=True, text=True, timeout=1200)
    m = re.search(r"([\d.]+) reads_per_s found (\d+) bytes (\d+)", r.stdout)
    if r.returncode != 0 or not m:
        return {"error": (r.stdout + r.stderr)[-300:]}
    return {"keys_per_s": float(m.group(1)), "found": int(m.group(2)), "bytes": int(m.group(3))}


def per_step(stream: Stream, steps: int, warmup: int, fn) -> list:
    """Milliseconds of each of `steps` calls of fn() (HIP events around every one)."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(steps):
        stream.sync()
        a, b = Event(), Event()
        a.record(stream)
        fn()
        b.record(stream)
        out.append(a.elapsed_ms(b))
    return out


def scan_leg(ix: HSTableIndex, stream: Stream, n: int, a, pool) -> dict:
    """scan_prepare (synchronous: wall clock), then scan + decode of every
    live entry in windows; `get` of the same live keys, in the same windows and
    the same process, beside it: how a caller who already knew the keys would
    read them."""
    from kingdb_amd.index import _Lookup
    lib = _lib.load()
    st = stream.ptr
    prep = []
    for _ in range(a.warmup + 5):
        t0 = time.perf_counter()
        live = ix.scan_prepare(0, stream)
        prep.append((time.perf_counter() - t0) * 1e3)
    prep = prep[a.warmup:]
    assert live == n, (live, n)
    kmax = ix._scan[3]
    w = min(a.window, live)
    L = _Lookup(w, w * kmax)
    plan = {}

    def window(Lx, first, m, locate):
        locate(first, m)
        f, ob, fc, mi, mo = ix.decode_plan(Lx, st, m)             # the summary download (synchronises)
        if first not in plan:
            plan[first] = (DeviceBuffer(ob + 64), DeviceBuffer(int(lib.kdb_get_scratch_bytes(m, fc))))
        out, scratch = plan[first]
        ix.run_decode(Lx, st, m, 0, out, scratch, fc, mi, mo)
        return f

    def scan_step():
        found = 0
        for first in range(0, live, w):
            m = min(w, live - first)
            found += window(L, first, m, lambda f0, mm: ix.run_scan(L, st, f0, mm))
        assert found == live

    scan_ms = per_step(stream, a.steps, a.warmup, scan_step)
    # check the last window byte for byte against what was put, then reuse its keys for `get`
    first = (live - 1) // w * w
    m = live - first
    klen = L.meta.download(4 * m, L.off["key_len"], dtype=np.uint32, stream=st)
    koff = L.meta.download(8 * m, L.off["key_off"], dtype=np.uint64, stream=st)
    ooff = L.meta.download(8 * m, L.off["out_off"], dtype=np.uint64, stream=st)
    dstat = L.meta.download(4 * m, L.off["dstatus"], dtype=np.int32, stream=st)
    kdata = L.keys.download(int(koff[-1]) + int(klen[-1]), stream=st)
    data = plan[first][0].download(int(ooff[-1]) + 100, stream=st)
    assert not dstat.any()
    for i in range(0, m, max(m // 257, 1)):
        j = int(kdata[int(koff[i]):int(koff[i]) + int(klen[i])].tobytes())
        assert j == first + i, (i, j)                             # written in key order: iterator order is key order
        assert data[int(ooff[i]):int(ooff[i]) + 100].tobytes() == pool[(100 * j) % (len(pool) - 100):][:100].tobytes()

    # `get` of the same live keys, window by window (keys resident, as in the get leg)
    G = []
    for first in range(0, live, w):
        m = min(w, live - first)
        G.append((first, m, ix._lookup([b"%016d" % j for j in range(first, first + m)], st, 0, 1 << 20)))

    def get_step():
        found = 0
        for first, m, Lg in G:
            found += window(Lg, first, m, lambda f0, mm, Lg=Lg: ix.run_lookup(Lg, st, mm))
        assert found == live

    get_ms = per_step(stream, a.steps, a.warmup, get_step)
    for _, _, Lg in G:
        Lg.free()
    L.free()
    for out, scratch in plan.values():
        out.free()
        scratch.free()
    med = lambda x: float(np.median(x))  # noqa: E731
    return {
        "scan_window": w, "scan_live": live,
        "scan_prepare_ms": round(med(prep), 3), "scan_prepare_ms_range": [round(min(prep), 3), round(max(prep), 3)],
        "scan_ms": round(med(scan_ms), 4), "scan_ms_range": [round(min(scan_ms), 4), round(max(scan_ms), 4)],
        "scan_entries_per_s": round(live / med(scan_ms) * 1e3),
        "get_same_keys_ms": round(med(get_ms), 4),
        "get_same_keys_ms_range": [round(min(get_ms), 4), round(max(get_ms), 4)],
        "get_same_keys_per_s": round(live / med(get_ms) * 1e3),
    }


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--no-scan", action="store_true")
    ap.add_argument("--window", type=int, default=1 << 18, help="live entries per scan window")
    a = ap.parse_args()
    if K.device_count() < 1:
        raise SystemExit("bench_getkeys: no GPU visible to libkdb_lz4.so")
    K.set_device(0)
    lib = _lib.load()
    n = a.keys
    d = tempfile.mkdtemp(prefix="kdbgetbench")
    try:
        files, pool = write_database(n, d)
        stream = Stream()
        st = stream.ptr
        ix = HSTableIndex(files, 1, stream=stream)
        assert set(ix.file_status.values()) == {0} and ix.entries == n, (ix.file_status, ix.entries)

        # load: the synchronous call, repeated on the resident files
        status = np.zeros(len(ix.names), np.int32)
        entries = ctypes.c_uint64(0)
        loads = []
        for _ in range(a.warmup + 5):
            t0 = time.perf_counter()
            _lib.check(lib.kdb_index_load_files(ix.h, st, ix.files.ptr, ix.file_off.ctypes.data,
                                                ix.file_size.ctypes.data, ix.fileid.ctypes.data, len(ix.names),
                                                status.ctypes.data, ctypes.byref(entries)), "load")
            loads.append((time.perf_counter() - t0) * 1e3)
        load_ms = float(np.median(loads[a.warmup:]))

        rng = np.random.default_rng(301)
        q = rng.integers(0, n, n)
        keys = [b"%016d" % int(x) for x in q]
        L = ix._lookup(keys, st, 0, 1 << 20)
        locate_ms = timed(stream, a.steps, a.warmup, lambda: ix.run_lookup(L, st, n))
        stat = L.meta.download(4 * n, L.off["status"], dtype=np.int32, stream=st)
        assert not stat.any(), "locate: a key was not found"

        found, out_bytes, frame_cap, max_in, max_out = ix.decode_plan(L, st, n)
        out = DeviceBuffer(out_bytes + 64)
        scratch = DeviceBuffer(int(lib.kdb_get_scratch_bytes(n, frame_cap)))

        def get_step():
            ix.run_lookup(L, st, n)
            f, ob, fc, mi, mo = ix.decode_plan(L, st, n)      # the summary download (synchronises)
            assert ob == out_bytes and fc == frame_cap
            ix.run_decode(L, st, n, 0, out, scratch, fc, mi, mo)

        get_ms = timed(stream, a.steps, a.warmup, get_step)
        dstat = L.meta.download(4 * n, L.off["dstatus"], dtype=np.int32, stream=st)
        olen = L.meta.download(8 * n, L.off["out_len"], dtype=np.uint64, stream=st)
        ooff = L.meta.download(8 * n, L.off["out_off"], dtype=np.uint64, stream=st)
        assert not dstat.any() and int(olen.sum()) == 100 * n
        data = out.download(out_bytes, stream=st)
        for i in range(0, n, max(n // 257, 1)):              # a sample of the values, byte for byte
            j = int(q[i])
            want = pool[(100 * j) % (len(pool) - 100):][:100].tobytes()
            assert data[int(ooff[i]):int(ooff[i]) + 100].tobytes() == want, i
        returned = 100 * n
        res = {
            "bench": "getkeys", "keys": n, "files": len(files), "file_bytes": int(sum(map(len, files.values()))),
            "steps": a.steps, "warmup": a.warmup,
            "load_ms": round(load_ms, 3), "load_rows_per_s": round(n / load_ms * 1e3),
            "locate_ms": round(locate_ms, 4), "locate_keys_per_s": round(n / locate_ms * 1e3),
            "get_ms": round(get_ms, 4), "get_keys_per_s": round(n / get_ms * 1e3),
            "get_gib_per_s": round(returned / get_ms * 1e3 / 2 ** 30, 3),
            "frame_cap": frame_cap,
        }
        L.free()
        out.free()
        scratch.free()
        if hasattr(lib, "kdb_index_scan_prepare") and not a.no_scan:
            res.update(scan_leg(ix, stream, n, a, pool))
        ix.close()
        if not a.no_reference and os.path.exists(REF_DB):
            res["reference_1_thread"] = reference_leg(d, n, 1)
            res["reference_16_threads"] = reference_leg(d, n, 16)
        print(json.dumps(res))
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
