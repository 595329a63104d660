#!/usr/bin/env python3
"""HSTable framing measured: the host writer against the device writer.

    python tools/bench_putfiles.py [--puts 1048576] [--steps 20] [--warmup 3]
                                   [--compact-steps 3] [--no-compact] [--deletes PCT]

Set: `--puts` x (16 B key "%016d", 100 B G1 value), hstable_size 32 MiB.
`--deletes PCT` (default 0: the set and the output above, unchanged) replaces
that share of the puts by deletes of earlier keys (put.DELETE): item j with
j % 100 < PCT deletes key j // 2.
kdb_put_entries_batch runs once, before any timing: every leg frames the same
entries, resident in device memory.  The legs run interleaved, one after the
other in every step, in one process on one device; each is a synchronous
piece of work timed by the wall clock (median and range of `--steps` steps
after `--warmup`):
  a  host      D2H of the per-entry arrays into pinned memory,
               kdb_hstable_writer_append_device into pinned file buffers, close
  b  device    kdb_hstable_dev_append + close, the files left in device memory
  c  device_dl b + the download of the finished files into pinned memory
               (what `a` ends with: the files in host memory)
  d  device_ix b + kdb_index_load_files over the resident files
  e  host_ix   a + the upload of the files and kdb_index_load_files (what
               HSTableIndex(files) does, without its Python copies)
Then HSTableIndex.compacted against .compacted_device over the same set with
batch 65 536 (`--compact-steps` runs each, interleaved).  Prints one JSON line.
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
from kingdb_amd.lz4 import DeviceBuffer, Stream  # noqa: E402

HS = 32 << 20


def stats(ms: list) -> dict:
    return {"ms": round(float(np.median(ms)), 4), "ms_range": [round(min(ms), 4), round(max(ms), 4)]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--puts", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--compact-steps", type=int, default=3)
    ap.add_argument("--no-compact", action="store_true")
    ap.add_argument("--deletes", type=int, default=0, metavar="PCT")
    a = ap.parse_args()
    if K.device_count() < 1:
        raise SystemExit("bench_putfiles: no GPU visible to libkdb_lz4.so")
    K.set_device(0)
    lib = _lib.load()
    n = a.puts
    orc = oracle.Oracle()
    pool = oracle.g1_pool(orc, 4 << 20)
    if not 0 <= a.deletes <= 100:
        raise SystemExit("bench_putfiles: --deletes takes a percentage")
    puts = [(b"%016d" % j, pool[(100 * j) % (len(pool) - 100):][:100].tobytes()) for j in range(n)]
    ndel = 0
    if a.deletes:
        for j in range(1, n):
            if j % 100 < a.deletes:
                puts[j] = (b"%016d" % (j // 2), put.DELETE)
                ndel += 1
    stream = Stream()
    st = stream.ptr
    b, _ = put.put_entries_device(puts, 1, stream)          # once: the framing is measured alone
    stream.sync()
    o = b._optr(n)
    total = int(b.out.download(8, 32 * n, dtype=np.uint64, stream=st)[0])

    # a: the host writer, as the put pipeline drives it
    host = ctypes.c_void_p()
    _lib.check(lib.kdb_lz4_host_alloc(ctypes.byref(host), 32 * n + 8), "host_alloc")
    hp = host.value
    hw = put.HSTableWriter(HS, 1, pinned=True)

    def host_write():
        hw.reset()
        _lib.check(lib.kdb_lz4_memcpy_d2h(hp, b.out.ptr, 32 * n + 8, st), "d2h")
        stream.sync()
        hw.append_device(st, b.entries.ptr, hp, hp + 8 * n, hp + 12 * n, hp + 24 * n, hp + 28 * n, n)
        hw.close()

    def host_file_ptrs():
        c = ctypes.c_uint32(0)
        _lib.check(lib.kdb_hstable_writer_file_count(hw.h, ctypes.byref(c)), "file_count")
        out = []
        for i in range(c.value):
            fid, p, sz = ctypes.c_uint32(), ctypes.c_void_p(), ctypes.c_uint64()
            _lib.check(lib.kdb_hstable_writer_file(hw.h, i, ctypes.byref(fid), ctypes.byref(p), ctypes.byref(sz)),
                       "file")
            out.append((fid.value, p.value, sz.value))
        return out

    host_write()
    hfiles = host_file_ptrs()
    file_bytes = sum(sz for _, _, sz in hfiles)
    nfiles = len(hfiles)

    # b, c, d: the device writer
    dw = put.DeviceHSTableWriter(HS, 1, put.DeviceHSTableWriter.arena_bytes(HS, total, n))
    pin = ctypes.c_void_p()
    _lib.check(lib.kdb_lz4_host_alloc(ctypes.byref(pin), file_bytes + 64 * nfiles + 64), "host_alloc")

    def device_write():
        dw.reset()
        dw.append_ptrs(st, b.entries.ptr, o["entry_off"], o["entry_len"], o["hashed"], o["kind"], o["status"], n)
        dw.close()
        stream.sync()

    def device_download():
        _, _, size, _ = dw.resident()
        at = 0
        for i in range(len(size)):
            _lib.check(lib.kdb_hstable_dev_download(dw.h, i, pin.value + at, st), "download")
            at += (int(size[i]) + 63) & ~63

    ixh = ctypes.c_void_p()
    _lib.check(lib.kdb_index_create(1, ctypes.byref(ixh)), "index_create")
    fstatus = np.zeros(nfiles + 1, np.int32)
    rows = ctypes.c_uint64(0)

    def device_index():
        ptr, off, size, fid = dw.resident()
        _lib.check(lib.kdb_index_load_files(ixh.value, st, ptr, off.ctypes.data, size.ctypes.data, fid.ctypes.data,
                                            len(fid), fstatus.ctypes.data, ctypes.byref(rows)), "load")
        assert rows.value == n and not fstatus[:len(fid)].any()

    up = DeviceBuffer(file_bytes + 64 * nfiles + 64)

    def host_index():
        files = host_file_ptrs()
        off = np.zeros(len(files), np.uint64)
        size = np.array([sz for _, _, sz in files], np.uint64)
        fid = np.array([f for f, _, _ in files], np.uint32)
        at = 0
        for i, (_, p, sz) in enumerate(files):
            off[i] = at
            _lib.check(lib.kdb_lz4_memcpy_h2d(up.ptr + at, p, sz, st), "h2d")
            at += (sz + 63) & ~63
        _lib.check(lib.kdb_index_load_files(ixh.value, st, up.ptr, off.ctypes.data, size.ctypes.data,
                                            fid.ctypes.data, len(fid), fstatus.ctypes.data, ctypes.byref(rows)),
                   "load")
        assert rows.value == n and not fstatus[:len(fid)].any()

    # the two writers agree before anything is timed
    device_write()
    dfiles = dw.files()
    assert len(dfiles) == nfiles
    for fid, p, sz in hfiles:
        assert dfiles["%08x" % fid] == ctypes.string_at(p, sz), "device file differs from the host writer's"

    legs = {"host": [host_write], "device": [device_write], "device_dl": [device_write, device_download],
            "device_ix": [device_write, device_index], "host_ix": [host_write, host_index]}
    ms = {k: [] for k in legs}
    for step in range(a.warmup + a.steps):
        for name, fns in legs.items():
            stream.sync()
            t0 = time.perf_counter()
            for fn in fns:
                fn()
            stream.sync()
            if step >= a.warmup:
                ms[name].append((time.perf_counter() - t0) * 1e3)
        print(f"step {step}", file=sys.stderr, flush=True)
    res = {"bench": "putfiles", "puts": n, "hstable_size": HS, "files": nfiles, "file_bytes": file_bytes,
           "entry_bytes": total, "steps": a.steps, "warmup": a.warmup}
    if a.deletes:
        res.update(deletes_pct=a.deletes, deletes=ndel)
    for name in legs:
        res[name] = stats(ms[name])
    lib.kdb_index_destroy(ixh.value)
    up.free()
    dw.free()
    b.free()
    lib.kdb_lz4_host_free(pin.value)
    lib.kdb_lz4_host_free(hp)

    if not a.no_compact:
        files = {"%08x" % f: ctypes.string_at(p, sz) for f, p, sz in host_file_ptrs()}
        ix = HSTableIndex(files, 1)
        cms = {"compacted": [], "compacted_device": []}
        for step in range(1 + a.compact_steps):
            t0 = time.perf_counter()
            want = ix.compacted(HS, 65536)
            t1 = time.perf_counter()
            w = ix.compacted_device(HS, 65536)
            _lib.check(lib.kdb_lz4_stream_sync(None), "sync")
            t2 = time.perf_counter()
            if step == 0:
                got = w.files()
                assert sorted(got) == sorted(want) and all(got[f] == want[f] for f in want)
            else:
                cms["compacted"].append((t1 - t0) * 1e3)
                cms["compacted_device"].append((t2 - t1) * 1e3)
            w.free()
            del want
            print(f"compaction step {step}", file=sys.stderr, flush=True)
        ix.close()
        res["compact_batch"] = 65536
        res["compact_steps"] = a.compact_steps
        for name in cms:
            res[name] = stats(cms[name])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
