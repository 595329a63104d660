// kingdb_amd/csrc/index_rows.h -- the varint rows of an offset array
// (OffsetArrayRow, format.h:523-528: varint64 hashed key, varint32 offset),
// decoded a terminator at a time: what one thread of index_parse_kernel
// (csrc/index.hip) does with its byte.  Host and device code, no HIP
// dependency, so a stand-alone host program runs the same text under the
// sanitizers (tests/cpp/tail_rows_main.cc).
//
// The rows are read through a byte view: forwards for the offset array of a
// closed file, backwards for the rows the device writer stages at the end of
// its arena while a file is open (csrc/hstable_dev.hip: staged byte b lies at
// arena[arena_bytes - 1 - b]).  The host's checks of an open file's record sit
// here too: tail_range_ok and the order rule, sorts_after_loaded.
#ifndef KDB_INDEX_ROWS_H_
#define KDB_INDEX_ROWS_H_

#include <stdint.h>

#include "hstable_decode.h"

namespace kdb_index_rows {

// Byte p of a row region whose byte 0 lies at *at0 and whose bytes follow
// downwards.  (A region that reads forwards is a plain const uint8_t*.)
struct Reversed {
  const uint8_t* at0;
  KDB_HD uint8_t operator[](uint64_t p) const { return *(at0 - p); }
};

KDB_HD bool is_terminator(uint8_t byte) { return (byte & 0x80u) == 0; }

// The varint whose last byte is byte `pos` of reg (a terminator): walks back
// to its first byte, never below byte 0 of the region, and assembles the
// value.  False where it is longer than GetVarint64 / GetVarint32 accept
// (coding.cc:147, 175: 10 bytes for a hash, 5 for an offset).
template <class B>
KDB_HD bool varint_ending_at(const B& reg, uint64_t pos, bool is_offset, uint64_t* value) {
  uint64_t start = pos;
  uint32_t len = 1;
  while (start > 0 && len <= 10u && (reg[start - 1u] & 0x80u)) {
    start--;
    len++;
  }
  if (len > (is_offset ? 5u : 10u)) return false;
  uint64_t v = 0;
  for (uint32_t i = 0; i < len; i++) v |= (uint64_t)(reg[start + i] & 127u) << (7u * i);
  *value = v;
  return true;
}

// What kdb_index_set_tail checks of a staging range before any byte is read:
// bytes [held_bytes, row_bytes) are to hold rows [held_rows, rows), two
// varints of at least a byte each per row, and staged byte row_bytes - 1 is
// not below the buffer's start (rows_last is an offset into it).
KDB_HD bool tail_range_ok(uint64_t held_rows, uint64_t held_bytes, uint64_t rows, uint64_t row_bytes,
                          uint64_t rows_last) {
  if (rows < held_rows || row_bytes < held_bytes) return false;
  const uint64_t nr = rows - held_rows, nb = row_bytes - held_bytes;
  if (nr > (1ull << 30) || nb < 2u * nr || nb > 15u * nr) return false;
  return row_bytes == 0 || rows_last >= row_bytes - 1u;
}

// The order rule of kdb_index_add_files and, ahead of time, of
// kdb_index_set_tail: a fresh load of all the files numbers a new file's rows
// after the loaded ones only if the file sorts after every loaded file by
// (timestamp, fileid).  A file that did not load (status != 0) has no rows.
KDB_HD bool sorts_after_loaded(const uint64_t* timestamps, const uint32_t* fileids, const int32_t* status,
                               uint32_t nfiles, uint64_t timestamp, uint32_t fileid) {
  for (uint32_t o = 0; o < nfiles; o++)
    if (status[o] == 0 && (timestamp < timestamps[o] || (timestamp == timestamps[o] && fileid <= fileids[o])))
      return false;
  return true;
}

}  // namespace kdb_index_rows

#endif  // KDB_INDEX_ROWS_H_
