"""Get by key on the GPU (include/kdb_put.h, csrc/index.hip): the index over a
set of closed HSTable files and the batched lookup in front of the decoder.

  HSTableIndex(files)     uploads the files once and loads their offset arrays
                          (HSTableManager::LoadDatabase / LoadFile); with
                          recover=, files without a usable footer are recovered
  .get(keys, verify)      [(status, value bytes)]: StorageEngine::GetWithIndex /
                          GetEntry per key, then kdb_get_values_batch over the
                          resident files (Database::GetRaw)
  .locate(keys)           the lookup alone: (locations, statuses)
  .scan(first, count)     a window of the live entries in iterator order
                          (Database::NewIterator): [(key, status, value)]
  .items(batch)           a generator over all of them, window by window
  .compacted(size)        the live entries written again as a fresh database
  .compacted_device(size) the same with no value byte leaving device memory
  .compact_copy(size)     the reference's compaction: the live entries copied
                          as they are stored, no decode, into type-2 files
                          with the view's largest timestamp (kdb_compact.h)
  .compact(snapshot)      compact_copy of a snapshot plus the hand-over:
                          (writer, index) over the compacted files and the
                          files added since (StorageEngine::Compaction)
  HSTableIndex.from_resident(writer)
                          an index over the files a put.DeviceHSTableWriter
                          holds in device memory, with no upload
  .refresh()              adds the files the writer has closed since
                          (kdb_index_add_files; StorageEngine::ProcessingLoopIndex):
                          write -> refresh -> get, with no file loaded twice
  .refresh(tail=True)     the same, and then the rows of the file the writer
                          still has open (kdb_index_set_tail): every put of an
                          appended batch can be read, with no file cut short
  .snapshot()             an HSTableSnapshot: get, locate, scan, items, compacted
                          and compacted_device as of now, while refresh() and
                          add_files() go on (kdb_snapshot_*; Database::NewSnapshot)
  .snapshot(tail=True)    the same with the entries of the writer's open file
                          in it, up to this moment (kdb_snapshot_create_tail):
                          what the reference gets by flushing before a snapshot
  .compact(carry_open=True)
                          the compaction under a running writer: the open file
                          moves into the new writer as it is (adopt_open)
  HSTableIndex(files, reserve=N) / .add_files(files)
                          the same for an uploaded index: new files go into
                          the N spare bytes behind the first ones

status: 0 OK, NOTFOUND, DELETED (the newest entry is a delete: Database::Get
returns a Status of code kDeleteOrder, or NotFound from the write buffer), MULTIPART
(MultipartRequired), or the decoder's -1 / -2 (see get.py).  Databases opened
with compression enabled only.  A file without a usable footer (status -1 in
`.file_status`: the newest file after a crash) is left out unless
HSTableIndex(files, recover="reference" | "content") is asked to recover it on
the device first (kingdb_amd/recover.py, HSTableManager::RecoverFile):
`.recovered` maps its name to the report, its status becomes 0, and a file the
reference would remove stays out with its status.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .lz4 import DeviceBuffer, Stream

NOTFOUND, DELETED, MULTIPART = -3, -4, -5
FILE_ORDER = -4                  # file status KDB_INDEX_FILE_ORDER: not newer than the loaded files
TAIL_REPARSE = 1                 # KDB_INDEX_TAIL_REPARSE
MULTIPART_REQUIRED = 1 << 20     # internal__size_multipart_required


def lib():
    return _lib.load()


def _a8(x: int) -> int:
    return (x + 7) & ~7


class _Lookup:
    """Device arrays of one batch of n lookups (inputs, outputs, the decoder's outputs)."""

    FIELDS = (("key_off", 8), ("stored_off", 8), ("avail", 8), ("svc", 8), ("size", 8), ("out_off", 8),
              ("location", 8), ("out_len", 8), ("key_len", 4), ("checksum", 4), ("checksum_initial", 4),
              ("status", 4), ("dstatus", 4))

    def __init__(self, n: int, key_bytes: int):
        self.n = n
        self.off = {}
        o = 0
        for name, w in self.FIELDS:
            self.off[name] = o
            o += _a8(n * w)
        self.off["summary"] = o
        self.meta = DeviceBuffer(o + 40)
        self.keys = DeviceBuffer(key_bytes + 64)
        self.scratch_bytes = int(lib().kdb_index_get_scratch_bytes(n))
        self.scratch = DeviceBuffer(self.scratch_bytes)

    def p(self, name: str) -> int:
        return self.meta.ptr + self.off[name]

    def free(self) -> None:
        for b in (self.meta, self.keys, self.scratch):
            b.free()


class _Borrowed:
    """A device range that belongs to someone else: free() leaves it alone."""

    def __init__(self, ptr: int, nbytes: int):
        self.ptr, self.nbytes = ptr, nbytes

    def free(self) -> None:
        pass


class _ReadPath:
    """The read path of HSTableIndex and HSTableSnapshot: the lookup, the scan
    windows, their decode and the compaction, over `self.h` through the C
    entry points `<_ABI>_get_batch`, `<_ABI>_scan_prepare`,
    `<_ABI>_scan_sort_steps` and `<_ABI>_scan_batch`.  A subclass sets _ABI
    and provides h, files, hash_type and _scan (None: no scan prepared)."""

    _ABI = "kdb_index"

    def _call(self, name: str, *args) -> None:
        name = f"{self._ABI}_{name}"
        _lib.check(getattr(lib(), name)(self.h, *args), name)

    def _lookup(self, keys, st, verify_header: int, multipart_required: int) -> _Lookup:
        n = len(keys)
        klen = np.array([len(k) for k in keys], np.uint32)
        koff = np.zeros(n, np.uint64)
        if n > 1:
            koff[1:] = np.cumsum(klen[:-1].astype(np.uint64))
        kbuf = np.frombuffer(b"".join(keys), np.uint8)
        L = _Lookup(n, len(kbuf))
        try:
            if len(kbuf):
                L.keys.upload(kbuf, stream=st)
            L.meta.upload(koff, L.off["key_off"], stream=st)
            L.meta.upload(klen, L.off["key_len"], stream=st)
            self.run_lookup(L, st, n, verify_header, multipart_required)
        except Exception:
            L.free()
            raise
        return L

    def run_lookup(self, L: _Lookup, st, n: int, verify_header: int = 0,
                   multipart_required: int = MULTIPART_REQUIRED) -> None:
        """kdb_index_get_batch / kdb_snapshot_get_batch on keys already resident in `L`."""
        self._call(
            "get_batch", st, L.keys.ptr, L.p("key_off"), L.p("key_len"), n, verify_header, multipart_required,
            L.scratch.ptr, L.scratch_bytes, L.p("stored_off"), L.p("avail"), L.p("svc"), L.p("size"),
            L.p("checksum"), L.p("checksum_initial"), L.p("out_off"), L.p("location"), L.p("status"),
            L.p("summary"))

    def decode_plan(self, L: _Lookup, st, n: int, frame_cap: int | None = None):
        """The summary download: (found, out bytes, frame_cap, max_in, max_out)."""
        s = L.meta.download(40, L.off["summary"], dtype=np.uint64, stream=st)
        found, out_bytes, max_avail, max_size, slots = (int(x) for x in s)
        if frame_cap is None:
            # frames are >= 8 bytes, so `slots` always suffices; values KingDB
            # writes hold one frame per part, far fewer (see get.get_values)
            frame_cap = min(slots, 2 * n + 8 * (slots - n) // 4096 + 64)
        return found, out_bytes, frame_cap, max_avail, max_size

    def run_decode(self, L: _Lookup, st, n: int, verify: int, out: DeviceBuffer, scratch: DeviceBuffer,
                   frame_cap: int, max_in: int, max_out: int) -> None:
        _lib.check(lib().kdb_get_values_batch(
            st, self.files.ptr, L.p("stored_off"), L.p("avail"), L.p("svc"), L.p("size"), n, out.ptr,
            L.p("out_off"), verify, L.p("checksum"), L.p("checksum_initial"), frame_cap, max_in, max_out,
            scratch.ptr, scratch.nbytes, L.p("out_len"), L.p("dstatus")), "kdb_get_values_batch")

    def locate(self, keys, verify_header: int = 0, stream: Stream | None = None,
               multipart_required: int = MULTIPART_REQUIRED) -> tuple[np.ndarray, np.ndarray]:
        n = len(keys)
        if n == 0:
            return np.zeros(0, np.uint64), np.zeros(0, np.int32)
        st = stream.ptr if stream else None
        L = self._lookup(keys, st, verify_header, multipart_required)
        try:
            loc = L.meta.download(8 * n, L.off["location"], dtype=np.uint64, stream=st)
            status = L.meta.download(4 * n, L.off["status"], dtype=np.int32, stream=st)
            return loc, status
        finally:
            L.free()

    def get(self, keys, verify: int = 0, stream: Stream | None = None,
            multipart_required: int = MULTIPART_REQUIRED, frame_cap: int | None = None
            ) -> list[tuple[int, bytes]]:
        n = len(keys)
        if n == 0:
            return []
        st = stream.ptr if stream else None
        L = self._lookup(keys, st, 1 if verify else 0, multipart_required)
        out = scratch = None
        try:
            found, out_bytes, frame_cap, max_in, max_out = self.decode_plan(L, st, n, frame_cap)
            status = L.meta.download(4 * n, L.off["status"], dtype=np.int32, stream=st)
            if found == 0:
                return [(int(s), b"") for s in status]
            out = DeviceBuffer(out_bytes + 64)
            scratch = DeviceBuffer(int(lib().kdb_get_scratch_bytes(n, frame_cap)))
            self.run_decode(L, st, n, verify, out, scratch, frame_cap, max_in, max_out)
            lo, hi = L.off["out_off"], L.off["out_len"] + 8 * n
            m = L.meta.download(hi - lo, lo, stream=st)
            ooff = m[:8 * n].view(np.uint64)
            olen = m[L.off["out_len"] - lo:][:8 * n].view(np.uint64)
            dstatus = L.meta.download(4 * n, L.off["dstatus"], dtype=np.int32, stream=st)
            data = out.download(out_bytes, stream=st)
            res = []
            for i in range(n):
                if status[i] != 0:
                    res.append((int(status[i]), b""))
                else:
                    res.append((int(dstatus[i]), data[int(ooff[i]):int(ooff[i]) + int(olen[i])].tobytes()))
            return res
        finally:
            L.free()
            for b in (out, scratch):
                if b is not None:
                    b.free()

    # ------------------------------------------------------------------ scan
    def scan_prepare(self, verify: int = 0, stream: Stream | None = None) -> int:
        """The liveness pass and the ordered live list (kdb_index_scan_prepare):
        the number of live entries.  Implicit on the first scan and repeated
        when `verify` changes (the header CRC-8 is part of liveness)."""
        live, kbytes, kmax = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
        self._scan = None
        self._call("scan_prepare", stream.ptr if stream else None, 1 if verify else 0, ctypes.byref(live),
                   ctypes.byref(kbytes), ctypes.byref(kmax))
        self._scan = (1 if verify else 0, live.value, kbytes.value, kmax.value)
        return live.value

    def _prepared(self, verify: int, stream: Stream | None) -> tuple[int, int, int]:
        s = self._scan
        if s is None or s[0] != (1 if verify else 0):
            self.scan_prepare(verify, stream)
        return self._scan[1:]

    def scan_sort_steps(self) -> int:
        """Compare-exchange passes the last scan_prepare ran (0: the files' rows ascend)."""
        steps = ctypes.c_uint32(0)
        self._call("scan_sort_steps", ctypes.byref(steps))
        return steps.value

    def run_scan(self, L: _Lookup, st, first: int, n: int, multipart_required: int = MULTIPART_REQUIRED) -> None:
        """kdb_index_scan_batch / kdb_snapshot_scan_batch into `L` (its keys buffer takes the packed keys)."""
        self._call(
            "scan_batch", st, first, n, multipart_required, L.scratch.ptr, L.scratch_bytes, L.keys.ptr, L.keys.nbytes,
            L.p("key_off"), L.p("key_len"), L.p("stored_off"), L.p("avail"), L.p("svc"), L.p("size"),
            L.p("checksum"), L.p("checksum_initial"), L.p("out_off"), L.p("location"), L.p("status"),
            L.p("summary"))

    def scan(self, first: int = 0, count: int | None = None, verify: int = 0,
             multipart_required: int = MULTIPART_REQUIRED, stream: Stream | None = None,
             frame_cap: int | None = None) -> list[tuple[bytes, int, bytes]]:
        """One window [first, first + count) of the live entries in iterator
        order (files by (timestamp, fileid), offsets ascending):
        [(key, status, value)], values decoded by kdb_get_values_batch.  status
        is 0, MULTIPART (value b"") or the decoder's -1 / -2."""
        live, _, kmax = self._prepared(verify, stream)
        n = live - first if count is None else count
        if first < 0 or n < 0 or first + n > live:
            raise _lib.HipError(f"scan window [{first}, {first + n}) outside the {live} live entries")
        if n == 0:
            return []
        st = stream.ptr if stream else None
        L = _Lookup(n, n * kmax)
        out = scratch = None
        try:
            self.run_scan(L, st, first, n, multipart_required)
            found, out_bytes, frame_cap, max_in, max_out = self.decode_plan(L, st, n, frame_cap)
            lo, hi = L.off["key_off"], L.off["key_off"] + 8 * n
            koff = L.meta.download(hi - lo, lo, dtype=np.uint64, stream=st)
            klen = L.meta.download(4 * n, L.off["key_len"], dtype=np.uint32, stream=st)
            status = L.meta.download(4 * n, L.off["status"], dtype=np.int32, stream=st)
            kbytes = int(koff[-1]) + int(klen[-1])
            kdata = L.keys.download(kbytes, stream=st) if kbytes else np.zeros(0, np.uint8)
            keys = [kdata[int(o):int(o) + int(m)].tobytes() for o, m in zip(koff, klen)]
            if found == 0:
                return [(k, int(s), b"") for k, s in zip(keys, status)]
            out = DeviceBuffer(out_bytes + 64)
            scratch = DeviceBuffer(int(lib().kdb_get_scratch_bytes(n, frame_cap)))
            self.run_decode(L, st, n, verify, out, scratch, frame_cap, max_in, max_out)
            ooff = L.meta.download(8 * n, L.off["out_off"], dtype=np.uint64, stream=st)
            olen = L.meta.download(8 * n, L.off["out_len"], dtype=np.uint64, stream=st)
            dstatus = L.meta.download(4 * n, L.off["dstatus"], dtype=np.int32, stream=st)
            data = out.download(out_bytes, stream=st)
            res = []
            for i in range(n):
                if status[i] != 0:
                    res.append((keys[i], int(status[i]), b""))
                else:
                    res.append((keys[i], int(dstatus[i]), data[int(ooff[i]):int(ooff[i]) + int(olen[i])].tobytes()))
            return res
        finally:
            L.free()
            for b in (out, scratch):
                if b is not None:
                    b.free()

    def items(self, batch: int = 65536, verify: int = 0, multipart_required: int = MULTIPART_REQUIRED,
              stream: Stream | None = None):
        """Generator over every live entry, a window of `batch` at a time, so a
        large database never has all its values in memory at once."""
        live, _, _ = self._prepared(verify, stream)
        for first in range(0, live, max(batch, 1)):
            yield from self.scan(first, min(batch, live - first), verify, multipart_required, stream)

    def compacted(self, hstable_size: int = 32 << 20, batch: int = 65536, verify: int = 0) -> dict[str, bytes]:
        """An offline compaction: the live entries (every key once, no deletes,
        no overwritten entries) written again through put.write_hstables, a
        window of the scan per write-buffer flush.  The files are an ordinary
        database holding exactly the live entries; this does not claim the
        file layout the reference's own compaction produces."""
        from . import put
        w = put.HSTableWriter(hstable_size, self.hash_type)
        window = []
        for key, status, value in self.items(batch, verify, multipart_required=1 << 62):
            if status != 0:
                raise _lib.HipError(f"compacted: value of {key!r} does not decode (status {status})")
            window.append((key, value))
            if len(window) == batch:
                w.append(put.put_entries(window, self.hash_type))
                window = []
        if window:
            w.append(put.put_entries(window, self.hash_type))
        w.close()
        return w.files()

    def compacted_device(self, hstable_size: int = 32 << 20, batch: int = 65536, verify: int = 0):
        """compacted() with no value byte leaving device memory: a closed
        put.DeviceHSTableWriter holding, batch for batch, the files
        compacted() returns (`.files()` downloads them, from_resident() opens
        them in place).  Each scan window's decode outputs are the inputs of
        kdb_put_entries_batch as they lie -- the packed keys, the decode buffer
        with out_off / out_len as value_off / value_len -- and the entries go
        to the device writer.  Per window the host sees the 40-byte summary,
        one flag and the writer's plan."""
        from . import put
        batch = max(batch, 1)
        live, kbytes, kmax = self._prepared(verify, None)
        windows = [(first, min(batch, live - first)) for first in range(0, live, batch)]
        big = 1 << 62
        # sizing pass: the window summaries alone bound the entry bytes
        bound = 0
        for first, n in windows:
            L = _Lookup(n, n * kmax)
            try:
                self.run_scan(L, None, first, n, big)
                _, out_bytes, _, _, _ = self.decode_plan(L, None, n)
            finally:
                L.free()
            bound += out_bytes + n * (72 + kmax) + (out_bytes // 65536 + n + 1) * 16 + 64
        w = put.DeviceHSTableWriter(hstable_size, self.hash_type,
                                    put.DeviceHSTableWriter.arena_bytes(hstable_size, bound, live))
        try:
            for first, n in windows:
                self._compact_window(w, first, n, kmax, verify, big)
            w.close()
        except Exception:
            w.free()
            raise
        return w

    def _compact_window(self, w, first: int, n: int, kmax: int, verify: int, big: int) -> None:
        from . import put
        L = _Lookup(n, n * kmax)
        bufs = [L]
        try:
            self.run_scan(L, None, first, n, big)
            found, out_bytes, frame_cap, max_in, max_out = self.decode_plan(L, None, n)
            if found != n:
                self._compact_fail(L, n, False)
            out = DeviceBuffer(out_bytes + 64)
            bufs.append(out)
            scratch = DeviceBuffer(int(lib().kdb_get_scratch_bytes(n, frame_cap)))
            bufs.append(scratch)
            self.run_decode(L, None, n, verify, out, scratch, frame_cap, max_in, max_out)
            # part_first u32 (n + 1), chunk_len u32 (n), flag u32
            feed = DeviceBuffer(_a8(4 * (n + 1)) + _a8(4 * n) + 8)
            bufs.append(feed)
            part_first, chunk_len = feed.ptr, feed.ptr + _a8(4 * (n + 1))
            flag = chunk_len + _a8(4 * n)
            _lib.check(lib().kdb_hstable_dev_feed(None, L.p("out_len"), L.p("status"), L.p("dstatus"), n, part_first,
                                                  chunk_len, flag), "kdb_hstable_dev_feed")
            raw = max(out_bytes, 1)
            pscratch_bytes = int(lib().kdb_put_scratch_bytes(n, n, raw))
            pscratch = DeviceBuffer(pscratch_bytes)
            bufs.append(pscratch)
            entries = DeviceBuffer(raw + n * (72 + kmax) + (raw // 65536 + n + 1) * 16 + 64)
            bufs.append(entries)
            po = DeviceBuffer(n * 32 + 64)
            bufs.append(po)
            o = po.ptr
            e_off, e_len, hashed, crc, kind, status, total = (o, o + 8 * n, o + 12 * n, o + 20 * n, o + 24 * n,
                                                              o + 28 * n, o + 32 * n)
            _lib.check(lib().kdb_put_entries_batch(
                None, L.keys.ptr, L.p("key_off"), L.p("key_len"), out.ptr, L.p("out_off"), L.p("out_len"), part_first,
                chunk_len, n, max_out, n, self.hash_type, pscratch.ptr, pscratch_bytes, raw, entries.ptr, e_off,
                e_len, total, hashed, crc, kind, status), "kdb_put_entries_batch")
            if int(feed.download(4, flag - feed.ptr, dtype=np.uint32)[0]):
                self._compact_fail(L, n, True)
            w.append_ptrs(None, entries.ptr, e_off, e_len, hashed, kind, status, n)
            _lib.check(lib().kdb_lz4_stream_sync(None), "sync")     # the window's buffers are read by queued work
        finally:
            for b in bufs:
                b.free()

    def compact_copy(self, hstable_size: int = 32 << 20, batch: int = 65536, spare_bytes: int = 0,
                     filetype: int = 2, lock: bool = True, closed_only: bool = False):
        """The compaction of the reference (StorageEngine::Compaction, steps
        6-7): every live entry of the view copied as it is stored -- a fresh
        header, the key, the stored value bytes, no decode -- into files of
        type kCompactedRegularType that all carry the largest timestamp of the
        view's files.  Returns the closed put.DeviceHSTableWriter (ids from 1
        until HSTableIndex.compact() hands it over), its arena sized for the
        copy plus `spare_bytes`.  Each scan window goes scan ->
        kdb_compact_entries_batch -> the writer; no value byte reaches the
        host, which per window sees the plan's total and the writer's plan.
        The window buffers are allocated once, for the largest window.
        filetype=1, lock=False writes the same windows as files of an ordinary
        database, timestamps counting with the ids: byte for byte the files of
        compacted_device() where every live entry is self-contained.
        closed_only=True, on a snapshot(tail=True): only the live entries that
        lie in the files closed when the snapshot was taken are copied (the
        first kdb_snapshot_scan_closed_live entries of the list), and the
        locked timestamp is those files'.  Liveness is still the snapshot's:
        an entry the open file overwrites or deletes is not copied, and what
        supersedes it stays in the open file, which HSTableIndex.compact(
        carry_open=True) carries whole.  Without a tail it changes nothing."""
        from . import put
        batch = max(batch, 1)
        live, _, kmax = self._prepared(0, None)
        if closed_only:
            live = self._closed_live(live)
        windows = [(first, min(batch, live - first)) for first in range(0, live, batch)]
        big = 1 << 62
        ts = ctypes.c_uint64(0)
        ih, nfiles = self._view()
        _lib.check(lib().kdb_index_view_timestamp(ih, nfiles, ctypes.byref(ts)), "kdb_index_view_timestamp")
        if not closed_only:
            ts.value = max(ts.value, self._tail_timestamp())  # a view's tail is a file of that view
        nmax = max([n for _, n in windows], default=1)
        L = _Lookup(nmax, nmax * kmax)
        bufs = [L]
        w = None
        try:
            scratch_bytes = int(lib().kdb_compact_scratch_bytes(nmax))
            scratch = DeviceBuffer(scratch_bytes)
            bufs.append(scratch)
            po = DeviceBuffer(nmax * 32 + 64)      # entry_off u64, hashed u64, entry_len, kind, status u32, total u64
            bufs.append(po)
            o = po.ptr
            e_off, hashed, e_len, kind, status, total = (o, o + 8 * nmax, o + 16 * nmax, o + 20 * nmax, o + 24 * nmax,
                                                         o + _a8(28 * nmax))

            def args(n):
                return (L.keys.ptr, L.keys.nbytes, L.p("key_off"), L.p("key_len"), L.p("stored_off"), L.p("avail"),
                        L.p("svc"), L.p("size"), L.p("checksum"), L.p("status"), n)

            # sizing pass: plans only, 8 bytes per window come down
            bound = most = 0
            for first, n in windows:
                self.run_scan(L, None, first, n, big)
                _lib.check(lib().kdb_compact_plan_batch(None, *args(n), self.files.nbytes, self.hash_type, scratch.ptr,
                                                        scratch_bytes, e_off, e_len, total, hashed, kind, status),
                           "kdb_compact_plan_batch")
                t = int(po.download(8, total - o, dtype=np.uint64)[0])
                bound += t
                most = max(most, t)
            w = put.DeviceHSTableWriter(hstable_size, self.hash_type,
                                        put.DeviceHSTableWriter.arena_bytes(hstable_size, bound, live) + spare_bytes,
                                        filetype=filetype, timestamp_lock=ts.value if lock else 0)
            entries = DeviceBuffer(most + 64)
            bufs.append(entries)
            refused = ctypes.c_uint32(0)
            for first, n in windows:
                self.run_scan(L, None, first, n, big)
                _lib.check(lib().kdb_compact_entries_batch(
                    None, self.files.ptr, self.files.nbytes, *args(n), self.hash_type, scratch.ptr, scratch_bytes,
                    entries.ptr, most, e_off, e_len, total, hashed, kind, status, ctypes.byref(refused)),
                    "kdb_compact_entries_batch")
                if refused.value:
                    raise _lib.HipError(f"compact_copy: {refused.value} entries of window {first} have a stored "
                                        "length their file does not hold")
                # the next window's work is queued behind this append on the same stream
                w.append_ptrs(None, entries.ptr, e_off, e_len, hashed, kind, status, n)
            w.close()
            _lib.check(lib().kdb_lz4_stream_sync(None), "sync")     # the buffers are read by queued work
        except Exception:
            if w is not None:
                w.free()                    # waits for the writer's queued work
            raise
        finally:
            for b in bufs:
                b.free()
        return w

    def _tail_timestamp(self) -> int:
        """The timestamp of the open file a view includes, 0 where it includes none."""
        return 0

    def _closed_live(self, live: int) -> int:
        """Of the `live` entries of the prepared scan, those in closed files: the list's first so many."""
        return live

    def _compact_fail(self, L: _Lookup, n: int, decoded: bool) -> None:
        """The error compacted() raises, for the window's first value that does not decode."""
        status = L.meta.download(4 * n, L.off["status"], dtype=np.int32)
        dstatus = L.meta.download(4 * n, L.off["dstatus"], dtype=np.int32) if decoded else status
        koff = L.meta.download(8 * n, L.off["key_off"], dtype=np.uint64)
        klen = L.meta.download(4 * n, L.off["key_len"], dtype=np.uint32)
        for i in range(n):
            s = int(status[i]) or int(dstatus[i])
            if s:
                key = L.keys.download(int(klen[i]), int(koff[i])).tobytes() if klen[i] else b""
                raise _lib.HipError(f"compacted: value of {key!r} does not decode (status {s})")
        raise _lib.HipError("compacted: a value of the window does not decode")


class HSTableIndex(_ReadPath):
    _snapshots = None                    # the open HSTableSnapshots, once there was one
    _tail = None                         # {"fileid", "rows", "bytes"} of the writer's open file, while held
    def __init__(self, files: dict[str, bytes], hash_type: int = 1, stream: Stream | None = None,
                 recover: str | None = None, reserve: int = 0):
        from . import recover as rec
        if reserve < 0:
            raise ValueError("reserve is a byte count")
        if recover is not None:
            rec.scope_code(recover)
        self.names = sorted(files)
        self.hash_type = hash_type
        self.recovered = {}              # name -> recover.Report of the files recovered at the load
        n = len(self.names)
        size = np.array([len(files[f]) for f in self.names], np.uint64)
        # a slot holds the file; with `recover`, one whose last bytes hold no
        # footer magic gets the room its recovery needs
        cap = size.copy()
        if recover is not None:
            for i, f in enumerate(self.names):
                b = files[f]
                if len(b) > 8192 and (len(b) < 8192 + 36 or b[-12:-4] != b"WOEM\0\0\0\0"):
                    cap[i] = rec.bound(len(b))
        self.fileid = np.array([int(f, 16) for f in self.names], np.uint32)
        self.files = None
        self.h = None
        self._scan = None                # (verify, live, key bytes, max key length) of the prepared scan
        self._owner = None               # from_resident: the writer whose arena the index borrows
        self._reserve = reserve          # spare bytes behind the uploaded files, for add_files
        st = stream.ptr if stream else None
        self._upload(files, size, cap, st)
        h = ctypes.c_void_p()
        _lib.check(lib().kdb_index_create(hash_type, ctypes.byref(h)), "kdb_index_create")
        self.h = h.value
        status = self._load(st)
        torn = [i for i in range(n) if status[i] == -1]
        if recover is not None and torn:
            # HSTableManager::LoadDatabase: a file LoadFile refuses is recovered (RecoverFile), in its slot
            relaid = any(cap[i] < rec.bound(int(size[i])) for i in torn)  # a footer with its magic and a bad CRC
            if relaid:
                for i in torn:
                    cap[i] = rec.bound(int(size[i]))
                self._upload(files, size, cap, st)
            reports = rec.recover_resident(self.files.ptr, self.file_off[torn], size[torn], cap[torn], recover, stream)
            for i, r in zip(torn, reports):
                if r.status == 0:                                        # the others the reference removes
                    self.file_size[i] = r.size
                    self.recovered[self.names[i]] = r
            # the handle holds the buffer and the offsets it was loaded over: after a new layout it is
            # loaded again even where no file came back
            if self.recovered or relaid:
                self._load(st)

    def _upload(self, files: dict[str, bytes], size: np.ndarray, cap: np.ndarray, st) -> None:
        """The files into 64-byte-aligned slots of cap[i] bytes, in one buffer."""
        n = len(self.names)
        off = np.zeros(n, np.uint64)
        if n > 1:
            off[1:] = np.cumsum((cap[:-1] + np.uint64(63)) & ~np.uint64(63))
        total = int(off[-1] + cap[-1]) if n else 0
        buf = np.zeros(total + 64, np.uint8)
        for f, o in zip(self.names, off):
            buf[int(o):int(o) + len(files[f])] = np.frombuffer(files[f], np.uint8)
        self.file_off, self.file_size = off, size.copy()
        if self.files is not None:
            self.files.free()
        self.files = DeviceBuffer(total + self._reserve + 64)
        self.files.upload(buf, stream=st)
        self._used = total               # add_files puts the next file behind this

    def _load(self, st) -> np.ndarray:
        n = len(self.names)
        status = np.zeros(max(n, 1), np.int32)
        entries = ctypes.c_uint64(0)
        self._scan = None
        _lib.check(lib().kdb_index_load_files(self.h, st, self.files.ptr, self.file_off.ctypes.data,
                                              self.file_size.ctypes.data, self.fileid.ctypes.data, n,
                                              status.ctypes.data, ctypes.byref(entries)), "kdb_index_load_files")
        self.file_status = {f: int(s) for f, s in zip(self.names, status[:n])}
        self.entries = entries.value
        return status[:n]

    @classmethod
    def from_resident(cls, writer, stream: Stream | None = None) -> "HSTableIndex":
        """An index over the closed files of a put.DeviceHSTableWriter where
        they lie in device memory: no download, no upload.  The index BORROWS
        the writer's arena: close() of such an index frees the index alone,
        and the writer must outlive it -- no reset() and no free() of the
        writer while the index is in use (the index keeps a reference to the
        writer, so it is not collected from under it)."""
        ptr, off, size, fid = writer.resident()
        self = cls.__new__(cls)
        self.names = ["%08x" % int(f) for f in fid]
        self.hash_type = writer.hash_type
        self.file_off, self.file_size, self.fileid = off.copy(), size.copy(), fid.copy()
        self.files = _Borrowed(ptr, writer.arena)
        self._owner = writer
        self._reserve = self._used = 0
        self.recovered = {}
        self.h = None
        self._scan = None
        n = len(fid)
        st = stream.ptr if stream else None
        h = ctypes.c_void_p()
        _lib.check(lib().kdb_index_create(self.hash_type, ctypes.byref(h)), "kdb_index_create")
        self.h = h.value
        status = np.zeros(max(n, 1), np.int32)
        entries = ctypes.c_uint64(0)
        _lib.check(lib().kdb_index_load_files(self.h, st, ptr, self.file_off.ctypes.data, self.file_size.ctypes.data,
                                              self.fileid.ctypes.data, n, status.ctypes.data, ctypes.byref(entries)),
                   "kdb_index_load_files")
        self.file_status = {f: int(s) for f, s in zip(self.names, status[:n])}
        self.entries = entries.value
        return self

    def _add(self, st, off: np.ndarray, size: np.ndarray, fid: np.ndarray, flags: int = 0) -> dict[str, int]:
        """kdb_index_add_files of files already resident in self.files: their
        statuses by name.  The index changes only if the call succeeds."""
        n = len(fid)
        off, size, fid = (np.ascontiguousarray(off, np.uint64), np.ascontiguousarray(size, np.uint64),
                          np.ascontiguousarray(fid, np.uint32))
        status = np.zeros(max(n, 1), np.int32)
        added = ctypes.c_uint64(0)
        rc = lib().kdb_index_add_files(self.h, st, self.files.ptr, off.ctypes.data, size.ctypes.data, fid.ctypes.data,
                                       n, flags, status.ctypes.data, ctypes.byref(added))
        names = ["%08x" % int(f) for f in fid]
        if rc != _lib.OK:
            refused = [f for f, s in zip(names, status[:n]) if s == FILE_ORDER]
            _lib.check(rc, "kdb_index_add_files" + (f" (not newer than the loaded files: {refused})" if refused else ""))
        self._scan = None
        if n:                            # the tail, where one was held, is dropped by the add
            self.entries -= self._tail["rows"] if self._tail else 0
            self._tail = None
        self.names += names
        self.file_off = np.concatenate([self.file_off, off])
        self.file_size = np.concatenate([self.file_size, size])
        self.fileid = np.concatenate([self.fileid, fid])
        res = {f: int(s) for f, s in zip(names, status[:n])}
        self.file_status.update(res)
        self.entries += added.value
        return res

    def refresh(self, stream: Stream | None = None, tail: bool = False, reparse: bool = False) -> int:
        """For an index made by from_resident(): adds the files its writer has
        closed since the index last looked (kdb_index_add_files, the part of
        StorageEngine::ProcessingLoopIndex a flush triggers) and returns the
        rows added.  Files already held are not read again.  With tail=False
        entries of the writer's still open file are not readable before it
        closes.  With tail=True the rows of that file are indexed as well,
        from where the writer stages them (kdb_index_set_tail; only the rows
        appended since the last such refresh are parsed, all of them with
        reparse=True): every entry of every appended batch is readable, and
        the index answers as one made fresh over the closed files and the
        open file closed as it is now.  Where no file is open, or the open
        file is incomplete (the last part of a multipart value has not
        arrived: it would close without an offset array), the tail is
        dropped.  The return value counts the tail's growth too.  A prepared
        scan is dropped (the next scan prepares again).  Not to run
        concurrently with lookups on this index."""
        if self._owner is None:
            raise ValueError("refresh() is for an index made by from_resident(); use add_files()")
        st = stream.ptr if stream else None
        ptr, off, size, fid = self._owner.resident()
        held = {int(f) for f in self.fileid}
        new = [i for i in range(len(fid)) if int(fid[i]) not in held]
        before = self.entries
        if new:
            self._add(st, off[new], size[new], fid[new])
        if tail:
            f = self._owner.open_file()
            self.set_tail(f if f is not None else _lib.OpenFile(), st, TAIL_REPARSE if reparse else 0)
        return self.entries - before

    def set_tail(self, f, st=None, flags: int = 0) -> int:
        """kdb_index_set_tail of an _lib.OpenFile record that lies in
        self.files: the rows the tail gained.  The index changes only if the
        call succeeds (HipError EINVAL otherwise)."""
        gained = ctypes.c_uint64(0)
        _lib.check(lib().kdb_index_set_tail(self.h, st, self.files.ptr, ctypes.byref(f), flags, ctypes.byref(gained)),
                   "kdb_index_set_tail")
        self._sync_tail()
        return gained.value

    def drop_tail(self, stream: Stream | None = None) -> None:
        """The index over the closed files alone again (kdb_index_drop_tail)."""
        _lib.check(lib().kdb_index_drop_tail(self.h, stream.ptr if stream else None), "kdb_index_drop_tail")
        self._sync_tail()

    def _sync_tail(self) -> None:
        held, fid, rows, nbytes, _, _ = self.tail_stats()
        self._tail = {"fileid": fid, "rows": rows, "bytes": nbytes} if held else None
        self._scan = None                # the C side drops the prepared scan with every change of the tail
        n = ctypes.c_uint64(0)
        _lib.check(lib().kdb_index_entry_count(self.h, ctypes.byref(n)), "kdb_index_entry_count")
        self.entries = n.value

    @property
    def tail(self):
        """None, or {"fileid", "rows", "bytes"} of the writer's open file as
        the index holds it (refresh(tail=True)).  `entries` counts its rows;
        names, file_status, file_off, file_size and fileid list the closed
        files alone."""
        return dict(self._tail) if self._tail else None

    def tail_stats(self) -> tuple[int, int, int, int, int, int]:
        """(held, fileid, rows, bytes, rows parsed by the last set_tail, buckets): kdb_index_tail_stats."""
        held, fid = ctypes.c_uint32(0), ctypes.c_uint32(0)
        rows, nbytes, parsed, nb = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        _lib.check(lib().kdb_index_tail_stats(self.h, ctypes.byref(held), ctypes.byref(fid), ctypes.byref(rows),
                                              ctypes.byref(nbytes), ctypes.byref(parsed), ctypes.byref(nb)),
                   "kdb_index_tail_stats")
        return held.value, fid.value, rows.value, nbytes.value, parsed.value, nb.value

    def _tail_timestamp(self) -> int:
        f = self._owner.open_file() if self._tail and self._owner is not None else None
        return f.timestamp if f is not None and f.fileid == self._tail["fileid"] else 0

    def _closed_live(self, live: int) -> int:
        if self._tail:
            raise ValueError("closed_only: take a snapshot(tail=True) of an index that holds a tail")
        return live

    def add_files(self, files: dict[str, bytes], stream: Stream | None = None) -> dict[str, int]:
        """Uploads `files` into the room HSTableIndex(..., reserve=) left behind
        the files the index holds, at 64-byte-aligned offsets, and adds them
        (kdb_index_add_files): their statuses by name, as `.file_status`.  The
        files must be newer, by (timestamp, fileid), than every file held.
        `recover=` is not applied: a file without a usable footer reports -1.
        ValueError, before anything is uploaded, on a name already held or
        files that do not fit the reserve; the index stays as it was."""
        if self._owner is not None:
            raise ValueError("add_files() is for an index that owns its buffer; use refresh()")
        names = sorted(files)
        dup = [f for f in names if f in self.names]
        if dup:
            raise ValueError(f"add_files: already held: {dup}")
        if not names:
            return {}
        size = np.array([len(files[f]) for f in names], np.uint64)
        start = (self._used + 63) & ~63
        off = np.zeros(len(names), np.uint64)
        off[1:] = np.cumsum((size[:-1] + np.uint64(63)) & ~np.uint64(63))
        off += np.uint64(start)
        end = int(off[-1] + size[-1])
        if end + 64 > self.files.nbytes:
            raise ValueError(f"add_files: {end - start} bytes do not fit the {self.files.nbytes - 64 - start} "
                             "bytes left of the reserve")
        buf = np.zeros(end - start + 64, np.uint8)
        for f, o in zip(names, off):
            buf[int(o) - start:int(o) - start + len(files[f])] = np.frombuffer(files[f], np.uint8)
        st = stream.ptr if stream else None
        self.files.upload(buf, start, stream=st)
        res = self._add(st, off, size, np.array([int(f, 16) for f in names], np.uint32))
        self._used = end
        return res

    def add_stats(self) -> tuple[int, int, int]:
        """(merged, buckets, rows parsed) of the last add (kdb_index_add_stats)."""
        m, b, r = ctypes.c_uint32(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        _lib.check(lib().kdb_index_add_stats(self.h, ctypes.byref(m), ctypes.byref(b), ctypes.byref(r)),
                   "kdb_index_add_stats")
        return m.value, b.value, r.value

    def pairs(self) -> tuple[np.ndarray, np.ndarray]:
        """The loaded rows in sequence order: (hashed keys, fileid << 32 | offset)."""
        h = np.zeros(max(self.entries, 1), np.uint64)
        loc = np.zeros(max(self.entries, 1), np.uint64)
        _lib.check(lib().kdb_index_pairs(self.h, h.ctypes.data, loc.ctypes.data), "kdb_index_pairs")
        return h[:self.entries], loc[:self.entries]

    def _view(self) -> tuple[int, int]:
        """(index handle, file slots of the view), for kdb_index_view_timestamp."""
        return self.h, len(self.names)

    def compact(self, snapshot: "HSTableSnapshot | None" = None, hstable_size: int = 32 << 20, batch: int = 65536,
                spare_bytes: int = 0, carry_open: bool = False):
        """The compaction of a snapshot (one is taken if none is given) and
        the hand-over, StorageEngine::Compaction as a whole: returns (writer,
        index).  The writer holds the snapshot's live entries in compacted
        files (compact_copy), numbered above every id this index holds, and
        behind them, copied as they are, every file of this index that is not
        a loaded file of the snapshot: the files added since, and files that
        loaded with a nonzero status.  `index` is
        HSTableIndex.from_resident(writer); puts appended to the writer and
        refresh()ed into it go on as on any writer, `spare_bytes` being the
        arena's room for them.  This index, its writer and its arena are left
        untouched: closing and freeing them is where the memory of the
        overwritten and deleted entries is reclaimed.  ValueError where this
        index's writer has a file open: close or cut it and refresh() first.
        carry_open=True compacts under the running writer instead
        (storage_engine.h:604-1010), with no file cut: the snapshot (taken
        here with tail=True after a refresh(tail=True) if none is given; a
        tail snapshot may be given) is compacted with closed_only=True, every
        closed file of this index that is not a loaded file of the snapshot is
        adopted, and the writer's open file moves into the new writer as its
        open file (adopt_open).  `index` has been refresh(tail=True)ed and
        answers get and scan as this index does after refresh(tail=True),
        except that a key whose newest entry is a delete in a compacted file
        reads NOTFOUND.  Stop appending to this index's writer: the new one
        goes on.  ValueError where the writer has closed files this index has
        not refreshed: they would be lost."""
        if carry_open:
            return self._compact_carry(snapshot, hstable_size, batch, spare_bytes)
        if self._owner is not None and self._owner.open_bytes():
            raise ValueError("compact: the writer has an open file; close or cut it and refresh() first")
        if snapshot is not None and snapshot.index is not self:
            raise ValueError("compact: the snapshot is of another index")
        snap = snapshot if snapshot is not None else self.snapshot()
        try:
            loaded = {f for f in snap.names if snap.file_status[f] == 0}
            rest = [i for i, f in enumerate(self.names) if f not in loaded]
            need = sum((int(self.file_size[i]) + 63) & ~63 for i in rest) + 64
            w = snap.compact_copy(hstable_size, batch, spare_bytes + need)
        finally:
            if snapshot is None:
                snap.close()
        try:
            first = max((int(f) for f in self.fileid), default=0) + 1
            w.adopt(first, self.files.ptr, self.file_off[rest], self.file_size[rest], self.fileid[rest])
            return w, HSTableIndex.from_resident(w)
        except Exception:
            w.free()
            raise

    def _compact_carry(self, snapshot, hstable_size: int, batch: int, spare_bytes: int):
        """compact(carry_open=True)."""
        if snapshot is not None and snapshot.index is not self:
            raise ValueError("compact: the snapshot is of another index")
        owner = self._owner
        if owner is not None:
            held = {int(f) for f in self.fileid}
            lost = ["%08x" % int(f) for f in owner.resident()[3] if int(f) not in held]
            if lost:
                raise ValueError(f"compact: the writer has closed files the index has not refreshed: {lost}")
        snap = snapshot if snapshot is not None else self.snapshot(tail=owner is not None)
        try:
            f = owner.open_file() if owner is not None else None
            loaded = {n for n in snap.names if snap.file_status[n] == 0}
            rest = [i for i, n in enumerate(self.names) if n not in loaded]
            need = sum((int(self.file_size[i]) + 63) & ~63 for i in rest) + 64
            if f is not None:                # the open file so far and its staged rows
                need += ((int(f.bytes) + 63) & ~63) + int(f.row_bytes) + 64
            w = snap.compact_copy(hstable_size, batch, spare_bytes + need, closed_only=True)
        finally:
            if snapshot is None:
                snap.close()
        try:
            first = max([int(x) for x in self.fileid] + ([int(f.fileid)] if f is not None else []), default=0) + 1
            w.adopt(first, self.files.ptr, self.file_off[rest], self.file_size[rest], self.fileid[rest])
            if f is not None:
                w.adopt_open(owner)
            ix = HSTableIndex.from_resident(w)
        except Exception:
            w.free()
            raise
        try:
            ix.refresh(tail=True)
        except Exception:
            ix.close()
            w.free()
            raise
        return w, ix

    def snapshot(self, tail: bool = False) -> "HSTableSnapshot":
        """A read-only view of the index as it is now (kdb_snapshot_create;
        Database::NewSnapshot): its get, locate, scan, items and compaction go
        on answering over the files held at this moment while refresh() /
        add_files() add newer ones.  It copies nothing and costs no device
        work.  With tail=False entries of the writer's still open file are not
        in it, also where refresh(tail=True) has made them readable through
        the index.  With tail=True they are (kdb_snapshot_create_tail): an
        index made by from_resident() is refresh(tail=True)ed first, and the
        snapshot answers as an index made fresh over the closed files and the
        open file closed as it is at this moment -- every put appended before
        the call, with no file cut.  Until that file has closed and been
        refresh()ed the index keeps it as its tail: drop_tail() and adds that
        leave the file out are refused (HipError EINVAL).  `.tail` is None or
        {"fileid", "rows"}; `names` lists the closed files, `entries` counts
        the tail's rows too.  close() it, or use it as a context manager;
        close() of the index closes the snapshots still open."""
        if tail and self._owner is not None:
            self.refresh(tail=True)
        return HSTableSnapshot(self, tail)

    def close(self) -> None:
        for s in list(self._snapshots or ()):
            s.close()
        if self.h:
            lib().kdb_index_destroy(self.h)
            self.h = None
        self.files.free()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HSTableSnapshot(_ReadPath):
    """HSTableIndex.snapshot(): the index as of the moment it was taken
    (include/kdb_snapshot.h).  `entries`, `names` and `file_status` are the
    index's of that moment; locate, get, scan_prepare, scan_sort_steps, scan,
    items, compacted and compacted_device are HSTableIndex's own, and answer
    as an HSTableIndex made fresh over `names` alone.  Its prepared scan is
    its own: adds to the index do not drop it.  Not to run concurrently with
    calls on the index or its other snapshots."""

    _ABI = "kdb_snapshot"

    def __init__(self, index: HSTableIndex, tail: bool = False):
        self.h = None
        self._scan = None
        self.index = index
        self.hash_type = index.hash_type
        self.names = list(index.names)
        self.file_status = dict(index.file_status)
        h = ctypes.c_void_p()
        if tail:
            _lib.check(lib().kdb_snapshot_create_tail(index.h, ctypes.byref(h)), "kdb_snapshot_create_tail")
        else:
            _lib.check(lib().kdb_snapshot_create(index.h, ctypes.byref(h)), "kdb_snapshot_create")
        self.h = h.value
        if index._snapshots is None:
            index._snapshots = []
        index._snapshots.append(self)
        n, f = ctypes.c_uint64(0), ctypes.c_uint32(0)
        _lib.check(lib().kdb_snapshot_entry_count(self.h, ctypes.byref(n)), "kdb_snapshot_entry_count")
        _lib.check(lib().kdb_snapshot_file_count(self.h, ctypes.byref(f)), "kdb_snapshot_file_count")
        self.entries = n.value
        included, fid, rows, _ = self.tail_stats()
        self._tail = {"fileid": fid, "rows": rows} if included else None
        self._tail_ts = index._tail_timestamp() if included else 0
        assert f.value == len(self.names) + included

    def tail_stats(self) -> tuple[int, int, int, int]:
        """(included, fileid, rows, pinned): kdb_snapshot_tail_stats.  pinned
        is 1 until the tail's file has closed and been added to the index."""
        inc, fid, rows, pin = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
        _lib.check(lib().kdb_snapshot_tail_stats(self.h, ctypes.byref(inc), ctypes.byref(fid), ctypes.byref(rows),
                                                 ctypes.byref(pin)), "kdb_snapshot_tail_stats")
        return inc.value, fid.value, rows.value, pin.value

    @property
    def tail(self):
        """None, or {"fileid", "rows"} of the open file as the snapshot took it (snapshot(tail=True))."""
        return dict(self._tail) if self._tail else None

    def closed_live(self) -> int:
        """After a scan_prepare: the live entries in files closed when the
        snapshot was taken, the first so many of the scan (kdb_snapshot_scan_closed_live)."""
        n = ctypes.c_uint64(0)
        _lib.check(lib().kdb_snapshot_scan_closed_live(self.h, ctypes.byref(n)), "kdb_snapshot_scan_closed_live")
        return n.value

    def _tail_timestamp(self) -> int:
        return self._tail_ts

    def _closed_live(self, live: int) -> int:
        return self.closed_live()

    @property
    def files(self):
        """The index's files buffer (the value decode reads it)."""
        return self.index.files

    def _view(self) -> tuple[int, int]:
        return self.index.h, len(self.names)

    def close(self) -> None:
        if self.h:
            lib().kdb_snapshot_release(self.h)
            self.h = None
            self.index._snapshots.remove(self)

    def __enter__(self) -> "HSTableSnapshot":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
