"""A Python model of the compaction by copy (include/kdb_compact.h), for the
compaction tests (not a test module), built on index_model / scan_model and
the oracle's encoders.

From a set of files and the names of the view's files it produces what
StorageEngine::Compaction (storage/storage_engine.h:796-1010) leaves:

  entries(view)      per live row of the view, in scan order: (key, entry
                     bytes, hash) -- a fresh header (flags kEntryFull, padding
                     0; size_value, size_value_compressed and checksum_content
                     carried over), the key, and the size_value_used() stored
                     bytes as they lie in the source file
  compacted_files()  those entries through the oracle's HSTable writer, a
                     window per write-buffer flush, as files of type
                     kCompactedRegularType that all carry one timestamp
  directory()        the compacted files, numbered above every id in use,
                     and every other file unchanged
"""
from __future__ import annotations

import struct

import index_model as M
import scan_model as S
from oracle import hstable

COMPACTED = 2                      # kCompactedRegularType (format.h:343)


def view_model(files: dict, names, orc, hash_type: int = 1) -> M.Model:
    return M.Model({f: files[f] for f in names}, orc, hash_type)


def entries(view: M.Model):
    """[(key, entry bytes, hash, size_value, svc, checksum, stored bytes)] in scan order."""
    out = []
    for _, off, name, key in S.live_rows(view):
        f = view.files[name]
        rc, e = M.locate_entry(f, off, False, view.orc)
        assert rc == 0
        used = e["svc"] or e["size_value"]              # size_value_used()
        va = off + e["size_header"] + e["size_key"]
        stored = f[va:va + used]
        assert len(stored) == used
        hashed = view.hash(key)
        hdr = view.orc.entry_header(e["checksum"], hstable.K_ENTRY_FULL, len(key), e["size_value"], e["svc"], 0,
                                    hashed)
        out.append((key, hdr + key + stored, hashed, e["size_value"], e["svc"], e["checksum"], stored))
    return out


def timestamp_max(view: M.Model) -> int:
    """The largest header timestamp among the view's loaded files."""
    return max((struct.unpack_from("<Q", f, 16)[0] for name, f in view.files.items()
                if view.file_status[name] == 0), default=0)


class _Writer(hstable.Writer):
    """The oracle's writer with the compaction's file identity: every file of
    `filetype`, every header with `timestamp` (LockSequenceTimestamp)."""

    def __init__(self, orc, hstable_size, hash_type, filetype, timestamp):
        super().__init__(orc, hstable_size, hash_type)
        self.filetype, self.lock = filetype, timestamp

    def _open(self) -> None:
        super()._open()
        ts = self.lock or self.timestamp
        self.files[self.cur] = bytearray(hstable.hstable_header_block(self.orc, ts, self.size_block, self.hash_type,
                                                                      self.filetype))

    def _write_offarray(self, fid: int) -> None:
        f = self.files[fid]
        rows = b"".join(hstable.varint(h) + hstable.varint(o) for h, o in self.offarray[fid])
        footer = struct.pack("<IIQQQ", self.filetype, 1 if self.padding_flag[fid] else 0, len(f),
                             len(self.offarray[fid]), hstable.MAGIC)
        body = rows + footer
        f += body + struct.pack("<I", self.orc.crc32c(body))


def compacted_files(view: M.Model, hstable_size: int, batch: int, first_fileid: int = 1,
                    filetype: int = COMPACTED, timestamp: int | None = None, hash_type: int = 1) -> dict[str, bytes]:
    """{name: bytes} of the compacted files, ids from first_fileid; timestamp
    None locks the view's largest, 0 leaves the writer's own (ids)."""
    ts = timestamp_max(view) if timestamp is None else timestamp
    w = _Writer(view.orc, hstable_size, hash_type, filetype, ts)
    ents = entries(view)
    step = max(batch, 1)
    for i in range(0, len(ents), step):
        for key, _, _, size_value, svc, checksum, stored in ents[i:i + step]:
            w._order(key, stored, 0, size_value, svc, checksum)
        w._flush(0, 0)                                  # the end of a window's append
    files = w.close()
    return {"%08x" % (first_fileid + i): files[f] for i, f in enumerate(sorted(files))}


def directory(files: dict, names, orc, hstable_size: int, batch: int, hash_type: int = 1,
              timestamp: int | None = None) -> tuple[dict[str, bytes], list[str]]:
    """(the directory after Compaction() of the view `names`, the compacted
    files' names): the compacted files ++ every file that is not a loaded
    file of the view."""
    view = view_model(files, names, orc, hash_type)
    first = max(int(f, 16) for f in files) + 1
    comp = compacted_files(view, hstable_size, batch, first, timestamp=timestamp, hash_type=hash_type)
    rest = {f: b for f, b in files.items() if f not in view.files or view.file_status[f] != 0}
    out = dict(comp)
    out.update(rest)
    return out, sorted(comp)
