// kingdb_amd/csrc/live_pin.h -- the pin a tail snapshot puts on a kdb_index
// (include/kdb_live.h): while a snapshot that includes rows of the writer's
// open file is open and that file has not been added closed, the handle must
// keep those rows where they are, numbered as they are.  Whether a drop, a
// set_tail or an add may proceed is decided here, in one function without a
// HIP dependency, so a stand-alone host program runs the same text
// (tests/cpp/live_pin_main.cc).  What the function cannot decide -- that the
// arriving file's first rows equal the rows held -- is index_rows_equal_kernel's
// (csrc/index.hip), run after it.
#ifndef KDB_LIVE_PIN_H_
#define KDB_LIVE_PIN_H_

#include <stdint.h>

namespace kdb_live_pin {

// The open file the handle holds as its tail, and the most rows of it that an
// open tail snapshot stands on.
struct Pin {
  bool pinned;           // some tail snapshot is open on a file not yet added closed
  uint32_t fileid;
  uint64_t timestamp, file_off;
  uint64_t rows;         // the largest row count among those snapshots
};

enum Op { kDrop = 0, kSet = 1, kAdd = 2 };

// What is asked of the handle.
//   kDrop  nothing else is read
//   kSet   open, incomplete, fileid: the record given to kdb_index_set_tail
//   kAdd   has_file: some new file loaded with status 0; then fileid, timestamp,
//          file_off and num_entries of the oldest such file by (timestamp, fileid)
struct Request {
  Op op;
  bool open, incomplete, has_file;
  uint32_t fileid;
  uint64_t timestamp, file_off, num_entries;
};

// True where the request may proceed.  Not pinned: always.  Pinned: the tail
// may only grow or be parsed again (a set of the same, complete, open file),
// and an add must bring the tail's own file first, where it lay, with at least
// the pinned rows.
inline bool allows(const Pin& p, const Request& r) {
  if (!p.pinned) return true;
  switch (r.op) {
    case kDrop:
      return false;
    case kSet:
      return r.open && !r.incomplete && r.fileid == p.fileid;
    case kAdd:
      return r.has_file && r.fileid == p.fileid && r.timestamp == p.timestamp && r.file_off == p.file_off &&
             r.num_entries >= p.rows;
  }
  return false;
}

}  // namespace kdb_live_pin

#endif  // KDB_LIVE_PIN_H_
