#!/usr/bin/env python3
"""File recovery on the GPU, measured (kdb_hstable_recover_files).

    python tools/bench_recover.py [--entries 250000] [--values 5500] [--runs 9]

Two files from this project's write path (put.put_entries + HSTableWriter),
their offset array and footer cut off, as a crash leaves them:
  small      `--entries` x (16 B key "%016d", 100 B G1 value), about 32 MiB,
             `reference` scope: the walk does the work
  multipart  `--values` x 6000 B G1 values sent as chunks [2500, 2500, 1000],
             about 32 MiB, `content` scope: the content CRC does the work
Per file: HIP events around kdb_hstable_recover_files (minimum and median of
`--runs`, the damaged bytes copied back into the slot before every run, outside
the timed region), the call's parts from the events of
kdb_hstable_recover_files_timed (speculate + resolve, chain, list, CRC, emit; of
the median run), the dependent loads of the chain kernel (the report), and the baseline: tests/cpp/recover_walk_main.cc, the sequential walk
over the same rules, built -O2 without sanitizers, one thread, same bytes
(minimum and median of `--runs`).  The recovered file must be the host's
(size and CRC32C).  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kingdb_amd as K  # noqa: E402
import oracle  # noqa: E402
from kingdb_amd import _lib, put  # noqa: E402
from kingdb_amd import recover as rec  # noqa: E402
from kingdb_amd.lz4 import DeviceBuffer, Event, Stream  # noqa: E402


def torn_file(puts_of, n: int, step: int) -> bytes:
    w = put.HSTableWriter(1 << 30)
    for i in range(0, n, step):
        w.append(put.put_entries(puts_of(i, min(step, n - i))))
    w.close()
    files = w.files()
    assert len(files) == 1
    f = next(iter(files.values()))
    oi = struct.unpack_from("<Q", f, len(f) - 28)[0]
    return f[:oi]


def host_walk(exe: str, tmp: str, f: bytes, scope: int, runs: int):
    path = os.path.join(tmp, "dump.bin")
    with open(path, "wb") as out:
        out.write(struct.pack("<IIQ", scope, 1, len(f)))
        out.write(f)
    r = subprocess.run([exe, path, str(runs)], capture_output=True, text=True, check=True, timeout=1200)
    line, timing = r.stdout.splitlines()[:2]
    _, _, status, size, crc, walked, kept = line.split()[:7]
    t = timing.split()
    return {"status": int(status), "size": int(size), "crc": int(crc), "walked": int(walked), "kept": int(kept),
            "min_ms": float(t[1]) / 1e3, "median_ms": float(t[2]) / 1e3}


def device_recover(orc, f: bytes, scope: str, runs: int):
    lib = _lib.load()
    stream = Stream()
    size = np.array([len(f)], np.uint64)
    cap = np.array([rec.bound(len(f))], np.uint64)
    off = np.zeros(1, np.uint64)
    need = int(lib.kdb_hstable_recover_scratch_bytes(size.ctypes.data, 1))
    pristine, work, scratch = DeviceBuffer(len(f)), DeviceBuffer(int(cap[0]) + 64), DeviceBuffer(need)
    try:
        pristine.upload(np.frombuffer(f, np.uint8))
        new_size, status = np.zeros(1, np.uint64), np.zeros(1, np.int32)
        total, parts = [], []
        report = np.zeros(1, rec._REPORT)
        for _ in range(runs + 2):                       # two warm-up runs
            _lib.check(lib.kdb_lz4_memcpy_d2d(work.ptr, pristine.ptr, len(f), stream.ptr), "d2d")
            stream.sync()
            a, b = Event(), Event()
            a.record(stream)
            ms = (ctypes.c_float * 6)()
            _lib.check(lib.kdb_hstable_recover_files_timed(stream.ptr, work.ptr, off.ctypes.data, size.ctypes.data,
                                                           cap.ctypes.data, 1, rec.scope_code(scope), scratch.ptr,
                                                           need, new_size.ctypes.data, status.ctypes.data,
                                                           report.ctypes.data, ms), "recover")
            b.record(stream)
            total.append(a.elapsed_ms(b))
            parts.append(list(ms))
        total, parts = total[2:], parts[2:]
        order = np.argsort(total)
        med = int(order[len(order) // 2])
        out = work.download(int(new_size[0]), stream=stream.ptr).tobytes()
        names = ("speculate", "chain", "list", "crc", "emit", "kernels")
        return {"status": int(status[0]), "size": int(new_size[0]), "crc": orc.crc32c(out),
                "min_ms": round(min(total), 4), "median_ms": round(total[med], 4),
                "parts_ms": {k: round(v, 4) for k, v in zip(names, parts[med])},
                "chain_loads": int(report[0]["chain_loads"]), "scratch_bytes": need}
    finally:
        for b in (pristine, work, scratch):
            b.free()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=250000)
    ap.add_argument("--values", type=int, default=5500)
    ap.add_argument("--runs", type=int, default=9)
    args = ap.parse_args()
    if K.device_count() < 1:
        raise SystemExit("bench_recover: no GPU")
    K.set_device(0)
    orc = oracle.Oracle()
    pool = oracle.g1_pool(orc, 4 << 20)

    def small(i, m):
        return [(b"%016d" % j, pool[(100 * j) % (len(pool) - 100):][:100].tobytes()) for j in range(i, i + m)]

    def multipart(i, m):
        return [(b"%016d" % j, pool[(6000 * j) % (len(pool) - 6000):][:6000].tobytes(), [2500, 2500, 1000])
                for j in range(i, i + m)]

    result = {"bench": "recover", "runs": args.runs}
    with tempfile.TemporaryDirectory(prefix="kdbrecover") as tmp:
        exe = os.path.join(tmp, "recover_walk_main")
        subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "recover_walk_main.cc"), "-o", exe],
                       check=True, timeout=600)
        for name, puts_of, n, step, scope in (("small", small, args.entries, 1 << 16, "reference"),
                                              ("multipart", multipart, args.values, 1 << 10, "content")):
            f = torn_file(puts_of, n, step)
            host = host_walk(exe, tmp, f, rec.scope_code(scope), args.runs)
            dev = device_recover(orc, f, scope, args.runs)
            if (dev["status"], dev["size"], dev["crc"]) != (host["status"], host["size"], host["crc"]):
                raise SystemExit(f"bench_recover: {name}: the device's file differs from the host walk's: {dev} {host}")
            result[name] = {"file_bytes": len(f), "entries": host["walked"], "rows": host["kept"], "scope": scope,
                            "tiles": (len(f) - 8192 + 4095) // 4096, "device": dev,
                            "host_walk_ms": {"min": round(host["min_ms"], 4), "median": round(host["median_ms"], 4)},
                            "speedup_median": round(host["median_ms"] / dev["median_ms"], 2)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
