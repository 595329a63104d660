"""HSTable files without a usable footer, recovered on the GPU
(include/kdb_recover.h, csrc/recover.hip): what Database::Open does for a file
whose offset array and footer never reached the disk (HSTableManager::
RecoverFile): the entries walked from byte 8192, the file cut where the walk
stops, a fresh offset array and footer appended.

  recover_files(files, crc_scope)   {name: bytes} -> ({name: recovered bytes},
                                    {name: Report}); a file the reference
                                    would remove (NOENTRY, LARGE) has a report
                                    only; one it would skip and leave on disk
                                    (BADHEADER) comes back unchanged
  recover_resident(...)             the same on files already in device memory
                                    (HSTableIndex(files, recover=...))

crc_scope "reference" reproduces the reference, which drops every multipart
(uncompacted) entry: it sums header bytes into the content CRC that the put
never summed.  "content" checks key || stored value, what the put computed.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _lib
from .lz4 import DeviceBuffer, Stream

NOENTRY, LARGE, BADHEADER = -6, -7, -8   # KDB_RECOVER_NOENTRY, KDB_RECOVER_LARGE, KDB_RECOVER_BADHEADER
SCOPES = {"reference": 0, "content": 1}


def lib():
    return _lib.load()


@dataclass
class Report:
    status: int                  # 0, NOENTRY, LARGE or BADHEADER
    size: int                    # bytes of the recovered file
    entries_walked: int
    rows_kept: int
    entries_invalid: int
    offset: int                  # where the walk stopped: the new offset_indexes
    footer_flags: int
    chain_loads: int = 0         # dependent loads of the sequential part


_REPORT = np.dtype([("walked", "<u8"), ("kept", "<u8"), ("invalid", "<u8"), ("offset", "<u8"), ("flags", "<u4"),
                    ("chain_loads", "<u4")])


def bound(size: int) -> int:
    return int(lib().kdb_hstable_recover_bound(size))


def scope_code(crc_scope) -> int:
    if crc_scope not in SCOPES:
        raise ValueError(f"crc_scope must be one of {sorted(SCOPES)}, not {crc_scope!r}")
    return SCOPES[crc_scope]


def recover_resident(files_ptr: int, off: np.ndarray, size: np.ndarray, cap: np.ndarray, crc_scope="reference",
                     stream: Stream | None = None) -> list[Report]:
    """kdb_hstable_recover_files on files in device memory: file i is
    [off[i], off[i] + size[i]) of the buffer at files_ptr and owns cap[i]
    bytes from off[i]."""
    n = len(off)
    off, size, cap = (np.ascontiguousarray(a, np.uint64) for a in (off, size, cap))
    if n == 0:
        return []
    need = int(lib().kdb_hstable_recover_scratch_bytes(size.ctypes.data, n))
    if need >= 1 << 63:
        raise _lib.HipError("kdb_hstable_recover_scratch_bytes: a file is too large")
    scratch = DeviceBuffer(need)
    try:
        new_size = np.zeros(n, np.uint64)
        status = np.zeros(n, np.int32)
        report = np.zeros(n, _REPORT)
        _lib.check(lib().kdb_hstable_recover_files(
            stream.ptr if stream else None, files_ptr, off.ctypes.data, size.ctypes.data, cap.ctypes.data, n,
            scope_code(crc_scope), scratch.ptr, need, new_size.ctypes.data, status.ctypes.data, report.ctypes.data),
            "kdb_hstable_recover_files")
    finally:
        scratch.free()
    return [Report(int(status[i]), int(new_size[i]), int(r["walked"]), int(r["kept"]), int(r["invalid"]),
                   int(r["offset"]), int(r["flags"]), int(r["chain_loads"])) for i, r in enumerate(report)]


def layout(sizes, caps):
    """64-byte-aligned slots of caps[i] bytes: (offsets, total)."""
    off = np.zeros(len(sizes), np.uint64)
    at = 0
    for i, c in enumerate(caps):
        off[i] = at
        at += (int(c) + 63) & ~63
    return off, at


def recover_files(files: dict[str, bytes], crc_scope="reference", stream: Stream | None = None
                  ) -> tuple[dict[str, bytes], dict[str, Report]]:
    """Every file recovered as the reference's Database::Open would leave it
    on disk: ({name: bytes}, {name: Report}).  The files it would remove have
    no bytes, and NOENTRY or LARGE as their report's status; a file without a
    usable header, which LoadDatabase skips and leaves where it is, comes
    back as it was (BADHEADER).  The caller picks the files (those that do
    not load) and saves the result."""
    scope_code(crc_scope)
    names = sorted(files)
    n = len(names)
    if n == 0:
        return {}, {}
    size = np.array([len(files[f]) for f in names], np.uint64)
    cap = np.array([bound(int(s)) for s in size], np.uint64)
    off, total = layout(size, cap)
    buf = np.zeros(total + 64, np.uint8)
    for f, o in zip(names, off):
        buf[int(o):int(o) + len(files[f])] = np.frombuffer(files[f], np.uint8)
    dev = DeviceBuffer(total + 64)
    st = stream.ptr if stream else None
    try:
        dev.upload(buf, stream=st)
        reports = recover_resident(dev.ptr, off, size, cap, crc_scope, stream)
        out, rep = {}, {}
        for f, o, r in zip(names, off, reports):
            rep[f] = r
            if r.status == 0:
                out[f] = dev.download(r.size, int(o), stream=st).tobytes()
            elif r.status == BADHEADER:
                out[f] = files[f]
        return out, rep
    finally:
        dev.free()
