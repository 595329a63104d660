"""The write path around the codec (include/kdb_put.h).

Mirrors what KingDB does with a stream of puts from one client thread --
Database::PutPart's frame policy and CRC32C (interface/database.cc:87-276),
then HSTableManager's entry and file encoding (storage/hstable_manager.h) --
with the per-value work on the GPU (csrc/put.hip) and only the per-file
framing on the host (csrc/hstable.cc).

  put_entries(puts)          one GPU batch: entry bytes, key hashes, CRCs
  HSTableWriter              the HSTable files those entries make
  write_hstables(puts, ...)  both, batch by batch: {file name: bytes}
  DeviceHSTableWriter        the same files framed on the GPU, in device memory
                             (csrc/hstable_dev.hip, include/kdb_hstable_dev.h)
  write_hstables_device(...) write_hstables with both stages on the device

A put is (key, value) or (key, value, chunks): `chunks` lists the sizes of
the PutPart calls the value arrives in (default: one call, i.e. Database::Put
of a value <= maximum_part_size; use split_parts() for Put's own splitting).
An item (key, DELETE) is Database::Delete of the key (include/kdb_ops.h): a
delete entry, header and key, in the place a put's entry would take.  It has
no value, so giving it chunks is a ValueError.  By default its bytes are the
reference's, header hash field 0; delete_hashed=True writes the key's hash
there, which keeps the delete reachable when its file has to be recovered.
Nothing here computes on the CPU except that host-side framing.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib
from .lz4 import DeviceBuffer, Stream

SELF_CONTAINED, MULTIPART, MULTIPART_UNFINISHED = 0, 1, 2
MAX_PART_SIZE = 1 << 20          # storage__maximum_part_size default (util/options.h:170-172)
OP_PUT, OP_DELETE = 0, 1         # KDB_OP_PUT, KDB_OP_DELETE
OPS_DELETE_HASHED = 1            # KDB_OPS_DELETE_HASHED


class _Delete:
    """The value of a delete item: (key, DELETE)."""

    def __repr__(self) -> str:
        return "DELETE"


DELETE = _Delete()


def is_delete(item) -> bool:
    return item[1] is DELETE


def lib():
    return _lib.load()


def padding_size(size_value: int) -> int:
    """EntryHeader::CalculatePaddingSize (storage/format.h:63-71)."""
    return (size_value // 65536 + 1) * 8


def split_parts(size: int, part_size: int = MAX_PART_SIZE) -> list[int]:
    """Database::PutPart's split of a value larger than maximum_part_size
    (interface/database.cc:96-122)."""
    if size <= part_size:
        return [size]
    return [min(part_size, size - o) for o in range(0, size, part_size)]


@dataclass
class PutBatchResult:
    entries: np.ndarray      # dense entry stream (u8)
    entry_off: np.ndarray    # u64
    entry_len: np.ndarray    # u32
    hashed: np.ndarray       # u64
    crc: np.ndarray          # u32
    kind: np.ndarray         # u32
    status: np.ndarray       # i32

    def entry(self, i: int) -> bytes:
        o = int(self.entry_off[i])
        return self.entries[o:o + int(self.entry_len[i])].tobytes()


class PutBatch:
    """Device buffers for batches of up to `n` puts / `raw` value bytes /
    `key_bytes` key bytes / `nparts` chunks, reused across calls."""

    def __init__(self, n: int, nparts: int, raw: int, key_bytes: int):
        self.n, self.nparts, self.raw, self.key_bytes = n, nparts, raw, key_bytes
        self.scratch_bytes = int(lib().kdb_put_scratch_bytes(n, nparts, raw))
        self.scratch = DeviceBuffer(self.scratch_bytes)
        self.keys = DeviceBuffer(key_bytes + 64)
        self.values = DeviceBuffer(raw + 64)
        # per value: key_off u64, key_len u32, value_off u64, value_len u64, part_first u32 (n+1)
        self.vmeta = DeviceBuffer(n * 32 + 8)
        self.chunks = DeviceBuffer(nparts * 4 + 4)
        self.ops = DeviceBuffer(n + 8)           # one KDB_OP_* byte per item (read only where a batch has deletes)
        self.entries_cap = raw + n * 64 + key_bytes + (raw // 65536 + 1) * 8 * 2 + n * 8 + 64
        self.entries = DeviceBuffer(self.entries_cap)
        # outputs: entry_off u64, entry_len u32, hashed u64, crc u32, kind u32, status i32, total u64
        self.out = DeviceBuffer(n * 32 + 64)

    def free(self) -> None:
        for b in (self.scratch, self.keys, self.values, self.vmeta, self.chunks, self.ops, self.entries, self.out):
            b.free()

    def _optr(self, n: int):
        o = self.out.ptr
        return dict(entry_off=o, entry_len=o + 8 * n, hashed=o + 12 * n, crc=o + 20 * n, kind=o + 24 * n,
                    status=o + 28 * n, total=o + 32 * n)

    def run_device(self, stream, n: int, nparts: int, max_chunk: int, raw: int, hash_type: int,
                   delete_hashed: bool = False, ops: bool = False) -> None:
        """Launches kdb_put_ops_batch on what is already resident.  ops: the
        batch has deletes and `self.ops` holds its n op bytes (otherwise every
        item is a put and the buffer is not read)."""
        if n > self.n or nparts > self.nparts or raw > self.raw:
            raise ValueError("batch larger than the buffers")
        v, c = self.vmeta.ptr, self.n     # metadata laid out for the capacity (a short batch uses a prefix)
        o = self._optr(n)
        _lib.check(lib().kdb_put_ops_batch(
            stream.ptr if stream else None, self.ops.ptr if ops else None, OPS_DELETE_HASHED if delete_hashed else 0,
            self.keys.ptr, v, v + 8 * c, self.values.ptr, v + 12 * c, v + 20 * c,
            v + 28 * c, self.chunks.ptr, nparts, max_chunk, n, hash_type, self.scratch.ptr, self.scratch_bytes, raw,
            self.entries.ptr, o["entry_off"], o["entry_len"], o["total"], o["hashed"], o["crc"], o["kind"],
            o["status"]), "kdb_put_ops_batch")


def _layout(puts):
    """The input arrays of kdb_put_ops_batch; the last is the op bytes, or
    None where no item is a delete."""
    keys = [p[0] for p in puts]
    dels = [is_delete(p) for p in puts]
    for p, d in zip(puts, dels):
        if d and len(p) > 2 and p[2] is not None:
            raise ValueError("a delete has no value: it takes no chunks")
    # a delete: value_len 0 and no chunk
    vals = [b"" if d else p[1] for p, d in zip(puts, dels)]
    chunks = [[] if d else list(p[2]) if len(p) > 2 and p[2] is not None else [len(p[1])]
              for p, d in zip(puts, dels)]
    ops = np.array(dels, np.uint8) if any(dels) else None
    for v, ch in zip(vals, chunks):
        if sum(ch) != len(v):
            raise ValueError("chunk sizes must add up to the value size")
    n = len(puts)
    klen = np.array([len(k) for k in keys], np.uint32)
    vlen = np.array([len(v) for v in vals], np.uint64)
    koff = np.zeros(n, np.uint64)
    voff = np.zeros(n, np.uint64)
    if n > 1:
        koff[1:] = np.cumsum(klen[:-1].astype(np.uint64))
        voff[1:] = np.cumsum(vlen[:-1])
    nch = np.array([len(c) for c in chunks], np.uint32)
    pf = np.zeros(n + 1, np.uint32)
    pf[1:] = np.cumsum(nch)
    clen = np.array([c for ch in chunks for c in ch], np.uint32)
    kbuf = np.frombuffer(b"".join(keys), np.uint8) if n else np.zeros(0, np.uint8)
    vbuf = np.frombuffer(b"".join(vals), np.uint8) if n else np.zeros(0, np.uint8)
    return kbuf, vbuf, koff, klen, voff, vlen, pf, clen, ops


def put_entries(puts, hash_type: int = 1, stream: Stream | None = None, delete_hashed: bool = False
                ) -> PutBatchResult:
    """One GPU batch: the HSTable entry bytes of every put and delete (see kdb_put.h, kdb_ops.h)."""
    kbuf, vbuf, koff, klen, voff, vlen, pf, clen, ops = _layout(puts)
    n = len(puts)
    nparts = len(clen)
    raw = int(vlen.sum()) if n else 0
    b = PutBatch(max(n, 1), max(nparts, 1), max(raw, 1), max(len(kbuf), 1))
    try:
        st = stream.ptr if stream else None
        if len(kbuf):
            b.keys.upload(kbuf, stream=st)
        if len(vbuf):
            b.values.upload(vbuf, stream=st)
        meta = np.concatenate([koff.view(np.uint8), klen.view(np.uint8), voff.view(np.uint8), vlen.view(np.uint8),
                               pf.view(np.uint8)])
        b.vmeta.upload(meta, stream=st)
        if nparts:
            b.chunks.upload(clen, stream=st)
        if ops is not None:
            b.ops.upload(ops, stream=st)
        b.run_device(stream, n, nparts, int(clen.max()) if nparts else 0, raw, hash_type, delete_hashed,
                     ops is not None)
        o = b._optr(n)
        # the copies back ride the caller's stream (see get_values)
        out = b.out.download(32 * n + 8, 0, stream=st)
        total = int(out[32 * n:32 * n + 8].view(np.uint64)[0])
        ents = b.entries.download(total, stream=st) if total else np.zeros(0, np.uint8)
        del o
        return PutBatchResult(
            entries=ents, entry_off=out[0:8 * n].view(np.uint64).copy(), entry_len=out[8 * n:12 * n].view(np.uint32).copy(),
            hashed=out[12 * n:20 * n].view(np.uint64).copy(), crc=out[20 * n:24 * n].view(np.uint32).copy(),
            kind=out[24 * n:28 * n].view(np.uint32).copy(), status=out[28 * n:32 * n].view(np.int32).copy())
    finally:
        b.free()


class HSTableWriter:
    """HSTable files for one database directory (csrc/hstable.cc)."""

    def __init__(self, hstable_size: int = 32 << 20, hash_type: int = 1, pinned: bool = False):
        h = ctypes.c_void_p()
        _lib.check(lib().kdb_hstable_writer_create2(hstable_size, hash_type, 1 if pinned else 0, ctypes.byref(h)),
                   "hstable_writer_create")
        self.h = h.value
        self.hstable_size, self.hash_type = hstable_size, hash_type

    def append(self, r: PutBatchResult) -> None:
        n = len(r.entry_len)
        ents = r.entries if len(r.entries) else np.zeros(1, np.uint8)
        _lib.check(lib().kdb_hstable_writer_append(
            self.h, ents.ctypes.data, r.entry_off.ctypes.data, r.entry_len.ctypes.data, r.hashed.ctypes.data,
            r.kind.ctypes.data, r.status.ctypes.data, n), "hstable_writer_append")

    def append_raw(self, entries_ptr: int, entry_off_ptr: int, entry_len_ptr: int, hashed_ptr: int, kind_ptr: int,
                   status_ptr: int, n: int) -> None:
        """append() from host pointers (pinned buffers of the bench pipeline)."""
        _lib.check(lib().kdb_hstable_writer_append(self.h, entries_ptr, entry_off_ptr, entry_len_ptr, hashed_ptr,
                                                   kind_ptr, status_ptr, n), "hstable_writer_append")

    def append_device(self, stream_ptr: int, d_entries: int, entry_off_ptr: int, entry_len_ptr: int,
                      hashed_ptr: int, kind_ptr: int, status_ptr: int, n: int) -> None:
        """append() with the entry bytes still on the device: DMA on `stream`
        straight into the files (host pointers for the per-entry arrays)."""
        _lib.check(lib().kdb_hstable_writer_append_device(self.h, stream_ptr, d_entries, entry_off_ptr, entry_len_ptr,
                                                          hashed_ptr, kind_ptr, status_ptr, n),
                   "hstable_writer_append_device")

    def close(self) -> None:
        _lib.check(lib().kdb_hstable_writer_close(self.h), "hstable_writer_close")

    def reset(self) -> None:
        """A fresh directory; the file buffers' memory is kept for reuse."""
        _lib.check(lib().kdb_hstable_writer_reset(self.h), "hstable_writer_reset")

    def files(self) -> dict[str, bytes]:
        c = ctypes.c_uint32(0)
        _lib.check(lib().kdb_hstable_writer_file_count(self.h, ctypes.byref(c)), "file_count")
        out = {}
        for i in range(c.value):
            fid, p, sz = ctypes.c_uint32(), ctypes.c_void_p(), ctypes.c_uint64()
            _lib.check(lib().kdb_hstable_writer_file(self.h, i, ctypes.byref(fid), ctypes.byref(p), ctypes.byref(sz)),
                       "file")
            out["%08x" % fid.value] = ctypes.string_at(p.value, sz.value) if sz.value else b""
        return out

    def file_bytes(self) -> int:
        c = ctypes.c_uint32(0)
        _lib.check(lib().kdb_hstable_writer_file_count(self.h, ctypes.byref(c)), "file_count")
        tot = 0
        for i in range(c.value):
            fid, p, sz = ctypes.c_uint32(), ctypes.c_void_p(), ctypes.c_uint64()
            _lib.check(lib().kdb_hstable_writer_file(self.h, i, ctypes.byref(fid), ctypes.byref(p), ctypes.byref(sz)),
                       "file")
            tot += sz.value
        return tot

    def save(self, directory: str) -> None:
        _lib.check(lib().kdb_hstable_writer_save(self.h, directory.encode()), "hstable_writer_save")

    def __del__(self):
        try:
            if self.h:
                lib().kdb_hstable_writer_destroy(self.h)
                self.h = None
        except Exception:
            pass


def db_options(hstable_size: int = 32 << 20, hash_type: int = 1) -> bytes:
    """The 48-byte db_options file (DatabaseOptionEncoder, storage/format.h:324-340)."""
    out = np.zeros(48, np.uint8)
    _lib.check(lib().kdb_hstable_db_options(hstable_size, hash_type, out.ctypes.data), "db_options")
    return out.tobytes()


def write_hstables(puts, hstable_size: int = 32 << 20, hash_type: int = 1, batch: int | None = None,
                   delete_hashed: bool = False) -> dict[str, bytes]:
    """The HSTable files KingDB writes for `puts` (one writer thread), with
    the puts handed to the GPU `batch` at a time (one write-buffer flush each)."""
    w = HSTableWriter(hstable_size, hash_type)
    step = batch or max(len(puts), 1)
    for i in range(0, len(puts), step):
        w.append(put_entries(puts[i:i + step], hash_type, delete_hashed=delete_hashed))
    w.close()
    return w.files()


def put_entries_device(puts, hash_type: int = 1, stream: Stream | None = None, delete_hashed: bool = False
                       ) -> tuple[PutBatch, int]:
    """put_entries() that leaves its outputs where they are: (the PutBatch
    holding them in device memory, n).  The caller frees the batch."""
    kbuf, vbuf, koff, klen, voff, vlen, pf, clen, ops = _layout(puts)
    n = len(puts)
    nparts = len(clen)
    raw = int(vlen.sum()) if n else 0
    b = PutBatch(max(n, 1), max(nparts, 1), max(raw, 1), max(len(kbuf), 1))
    try:
        st = stream.ptr if stream else None
        if len(kbuf):
            b.keys.upload(kbuf, stream=st)
        if len(vbuf):
            b.values.upload(vbuf, stream=st)
        # laid out for the capacity, as run_device reads it (n = 0: one empty slot)
        c = b.n
        meta = np.zeros(c * 32 + 8, np.uint8)
        for arr, at in ((koff, 0), (klen, 8 * c), (voff, 12 * c), (vlen, 20 * c), (pf, 28 * c)):
            a = arr.view(np.uint8)
            meta[at:at + len(a)] = a
        b.vmeta.upload(meta, stream=st)
        if nparts:
            b.chunks.upload(clen, stream=st)
        if ops is not None:
            b.ops.upload(ops, stream=st)
        b.run_device(stream, n, nparts, int(clen.max()) if nparts else 0, raw, hash_type, delete_hashed,
                     ops is not None)
    except Exception:
        b.free()
        raise
    return b, n


def entries_bound(puts, delete_hashed: bool = False) -> int:
    """An upper bound on the entry bytes `puts` make (PutBatch's own sizing);
    a delete's entry has the same size with either header hash."""
    raw = sum(0 if is_delete(p) else len(p[1]) for p in puts)
    return raw + sum(len(p[0]) for p in puts) + len(puts) * 72 + (raw // 65536 + len(puts) + 1) * 16 + 64


class DeviceHSTableWriter:
    """HSTable files for one database directory, built in device memory
    (include/kdb_hstable_dev.h): the files of HSTableWriter, byte for byte,
    with the cut, the offset arrays, the header blocks and the footers written
    by kernels.  `arena_bytes` is the one device buffer the files live in
    (arena_bytes() bounds what a database needs; the default holds 256 MiB of
    entries in 2 Mi puts).  An append that does not fit raises HipError and
    leaves the writer as it was."""

    def __init__(self, hstable_size: int = 32 << 20, hash_type: int = 1, arena_bytes: int | None = None,
                 filetype: int = 1, timestamp_lock: int = 0):
        """`filetype` 2 and `timestamp_lock` make the files of a compaction
        (kdb_hstable_dev_create2): kCompactedRegularType, every header with
        the locked timestamp; adopt() returns the writer to type 1."""
        if arena_bytes is None:
            arena_bytes = self.arena_bytes(hstable_size, 256 << 20, 2 << 20)
        h = ctypes.c_void_p()
        if filetype == 1 and timestamp_lock == 0:
            _lib.check(lib().kdb_hstable_dev_create(hstable_size, hash_type, arena_bytes, ctypes.byref(h)),
                       "hstable_dev_create")
        else:
            _lib.check(lib().kdb_hstable_dev_create2(hstable_size, hash_type, arena_bytes, filetype, timestamp_lock,
                                                     ctypes.byref(h)), "hstable_dev_create2")
        self.h = h.value
        self.hstable_size, self.hash_type, self.arena = hstable_size, hash_type, arena_bytes

    @staticmethod
    def arena_bytes(hstable_size: int, entry_bytes: int, n_entries: int) -> int:
        return int(lib().kdb_hstable_dev_arena_bytes(hstable_size, entry_bytes, n_entries))

    def append_ptrs(self, stream_ptr, d_entries: int, d_entry_off: int, d_entry_len: int, d_hashed: int,
                    d_kind: int, d_status: int, n: int) -> None:
        """One batch from raw device pointers (the outputs of kdb_put_entries_batch)."""
        _lib.check(lib().kdb_hstable_dev_append(self.h, stream_ptr, d_entries, d_entry_off, d_entry_len, d_hashed,
                                                d_kind, d_status, n), "hstable_dev_append")

    def append_batch(self, b: PutBatch, n: int, stream: Stream | None = None) -> None:
        """One batch from the device outputs of PutBatch.run_device(…, n, …), as they lie."""
        o = b._optr(n)
        self.append_ptrs(stream.ptr if stream else None, b.entries.ptr, o["entry_off"], o["entry_len"], o["hashed"],
                         o["kind"], o["status"], n)

    def close(self) -> None:
        _lib.check(lib().kdb_hstable_dev_close(self.h), "hstable_dev_close")

    def open_bytes(self) -> int:
        """The size so far of the file that is open, 0 where none is."""
        b = ctypes.c_uint64(0)
        _lib.check(lib().kdb_hstable_dev_open_bytes(self.h, ctypes.byref(b)), "hstable_dev_open_bytes")
        return b.value

    def open_file(self):
        """The file that is open, as HSTableIndex.refresh(tail=True) reads it
        (kdb_hstable_dev_open_file): an _lib.OpenFile record -- fileid,
        incomplete, timestamp, file_off, bytes, rows, row_bytes, rows_last --
        or None where no file is open.  Waits for the writer's queued work."""
        f = _lib.OpenFile()
        _lib.check(lib().kdb_hstable_dev_open_file(self.h, ctypes.byref(f)), "hstable_dev_open_file")
        return f if f.open else None

    def adopt(self, first_fileid: int, src_ptr: int, off, size, fileid, stream: Stream | None = None) -> None:
        """The hand-over of a compaction (kdb_hstable_dev_adopt): the writer's
        own closed files become first_fileid, first_fileid + 1, ...; the files
        src_ptr[off[f] .. +size[f]) are copied, device to device, behind them
        with their ids; files opened afterwards are ordinary ones.  Refused
        (HipError EINVAL, the writer as before): an open file, an id
        >= first_fileid or given twice, bytes that do not fit the arena."""
        off, size, fileid = (np.ascontiguousarray(off, np.uint64), np.ascontiguousarray(size, np.uint64),
                             np.ascontiguousarray(fileid, np.uint32))
        n = len(fileid)
        _lib.check(lib().kdb_hstable_dev_adopt(self.h, stream.ptr if stream else None, first_fileid,
                                               src_ptr if n else None, off.ctypes.data if n else None,
                                               size.ctypes.data if n else None, fileid.ctypes.data if n else None, n),
                   "hstable_dev_adopt")

    def adopt_open(self, src: "DeviceHSTableWriter", stream: Stream | None = None) -> None:
        """The hand-over's last step (kdb_hstable_dev_adopt_open), after
        adopt(): the file `src` has open becomes this writer's open file --
        its bytes and staged rows copied device to device, its id, timestamp,
        size, marks and row count taken over -- and closes here, after any
        further appends, byte for byte as it would have closed in `src`.
        Nothing happens where `src` has no file open.  `src` is not modified:
        stop appending to it.  Refused (HipError EINVAL, both writers as
        before): a file open here, another hstable_size or hash_type, a writer
        of compacted files, an id this writer holds, bytes that do not fit."""
        _lib.check(lib().kdb_hstable_dev_adopt_open(self.h, stream.ptr if stream else None,
                                                    src.h if src is not None else None), "hstable_dev_adopt_open")

    def reset(self) -> None:
        """A fresh directory; the arena is kept."""
        _lib.check(lib().kdb_hstable_dev_reset(self.h), "hstable_dev_reset")

    def resident(self) -> tuple[int, np.ndarray, np.ndarray, np.ndarray]:
        """The closed files where they are: (device pointer of the arena,
        file_off, file_size, fileid), the arguments of kdb_index_load_files."""
        c = ctypes.c_uint32(0)
        _lib.check(lib().kdb_hstable_dev_file_count(self.h, ctypes.byref(c)), "hstable_dev_file_count")
        n = c.value
        off, size, fid = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint32)
        base = ctypes.c_void_p()
        _lib.check(lib().kdb_hstable_dev_files(self.h, ctypes.byref(base), off.ctypes.data, size.ctypes.data,
                                               fid.ctypes.data, n), "hstable_dev_files")
        return base.value or 0, off[:n], size[:n], fid[:n]

    def files(self, stream: Stream | None = None) -> dict[str, bytes]:
        """{file name: bytes} of the closed files, downloaded."""
        _, _, size, fid = self.resident()
        out = {}
        for i in range(len(fid)):
            buf = np.empty(max(int(size[i]), 1), np.uint8)
            _lib.check(lib().kdb_hstable_dev_download(self.h, i, buf.ctypes.data, stream.ptr if stream else None),
                       "hstable_dev_download")
            out["%08x" % int(fid[i])] = buf[:int(size[i])].tobytes()
        return out

    def free(self) -> None:
        if self.h:
            lib().kdb_hstable_dev_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def write_hstables_device(puts, hstable_size: int = 32 << 20, hash_type: int = 1, batch: int | None = None,
                          delete_hashed: bool = False) -> dict[str, bytes]:
    """write_hstables() with both stages on the device: the entries never
    leave it, only the finished files come back."""
    step = batch or max(len(puts), 1)
    bound = sum(entries_bound(puts[i:i + step]) for i in range(0, len(puts), step))
    w = DeviceHSTableWriter(hstable_size, hash_type,
                            DeviceHSTableWriter.arena_bytes(hstable_size, bound, len(puts)))
    try:
        for i in range(0, len(puts), step):
            b, n = put_entries_device(puts[i:i + step], hash_type, delete_hashed=delete_hashed)
            try:
                w.append_batch(b, n)
                _lib.check(lib().kdb_lz4_stream_sync(None), "sync")     # the batch's buffers are read by queued work
            finally:
                b.free()
        w.close()
        return w.files()
    finally:
        w.free()
