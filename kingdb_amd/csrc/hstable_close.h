// kingdb_amd/csrc/hstable_close.h -- how an HSTable file is closed: the rows
// of its offset array, the footer and the footer's CRC32C, for the device
// writer (hstable_dev.hip), for file recovery (recover.hip) and for the host
// (tests/cpp/recover_walk_main.cc).
//
//   row_len / put_row   OffsetArrayRow::EncodeTo (format.h:523-528):
//                       varint64(hashed key) varint32(offset of the entry)
//   encode_footer       HSTableFooter::EncodeTo (format.h:480-493) without its
//                       last field: the 32 bytes the CRC is extended over
// are plain inline functions, no HIP runtime, the same text for hipcc and g++.
// Under hipcc there is also the closer itself (WriteOffsetArray,
// hstable_manager.h:381-428: crc32c over the rows, extended over the footer's
// first 32 bytes, stored as its last 4):
//   rows_piece_crc      a file's rows are kCrcPieces equal pieces, a workgroup
//                       each: the CRC32C of one piece (crc::extend_block)
//   close_file          one thread: the pieces' CRCs joined, extended over the
//                       encoded footer, and the 36 bytes stored behind the rows
// Neither checks a bound: where the rows lie, that they and the footer fit
// there, and the footer's fields are the calling kernel's.
#pragma once
#include <stdint.h>

#include "hstable_cut.h"
#include "hstable_decode.h"
#if defined(__HIPCC__)
#include "crc_device.h"
#endif

namespace kdb_hstable_close {

namespace hs = kdb_hstable;
namespace cut = kdb_hstable_cut;

KDB_HD uint32_t row_len(uint64_t hash, uint32_t offset) { return cut::varint_len(hash) + cut::varint_len(offset); }

// The row's bytes through put(k, byte), k = 0 .. row_len - 1; no byte at or
// past rl (the length the caller reserved) is put.
template <class Put>
KDB_HD void put_row(uint64_t hash, uint32_t offset, uint32_t rl, Put put) {
  const uint32_t hl = cut::put_varint(hash, [&](uint32_t k, uint8_t byte) {
    if (k < rl) put(k, byte);
  });
  cut::put_varint(offset, [&](uint32_t k, uint8_t byte) {
    if (hl + k < rl) put(hl + k, byte);
  });
}

constexpr uint32_t kFooterCrcBytes = 32;      // the footer without its crc32
static_assert(kFooterCrcBytes + 4u == hs::kFooterSize, "the CRC is the footer's last field");

// filetype, flags, offset of the rows, their number, magic: little-endian.
KDB_HD void encode_footer(uint32_t filetype, uint32_t flags, uint64_t offset_indexes, uint64_t num_entries,
                          uint8_t out[kFooterCrcBytes]) {
  const uint32_t w32[2] = {filetype, flags};
  const uint64_t w64[3] = {offset_indexes, num_entries, hs::kMagic};
  for (uint32_t i = 0; i < 8u; i++) out[i] = (uint8_t)(w32[i >> 2] >> (8u * (i & 3u)));
  for (uint32_t i = 0; i < 24u; i++) out[8u + i] = (uint8_t)(w64[i >> 3] >> (8u * (i & 7u)));
}

#if defined(__HIPCC__)
namespace crc = kdb_lz4::crc;

constexpr uint32_t kCrcPieces = 64;           // workgroups per closing file's rows

// A file's rows as kCrcPieces equal pieces: piece p is bytes [*a, *b).
__device__ __forceinline__ void crc_piece(uint64_t nbytes, uint32_t p, uint64_t* a, uint64_t* b) {
  const uint64_t piece = (nbytes + kCrcPieces - 1u) / kCrcPieces;
  *a = min((uint64_t)p * piece, nbytes);
  *b = min(*a + piece, nbytes);
}

// crc32c of piece `piece` of rows[0 .. nbytes), by a workgroup of kWaves
// waves: crc::extend_block's contract (reached uniformly, the result on
// thread 0, s_t staged, s_crc kWaves words).
template <uint32_t kWaves>
__device__ __forceinline__ uint32_t rows_piece_crc(const uint8_t* rows, uint64_t nbytes, uint32_t piece,
                                                   const uint32_t* s_t, uint32_t* s_crc) {
  uint64_t lo, hi;
  crc_piece(nbytes, piece, &lo, &hi);
  return crc::extend_block<kWaves>(rows + lo, hi - lo, s_t, s_crc);
}

// One thread: piece_crc[0 .. kCrcPieces) of rows[0 .. nbytes) joined, extended
// over the footer's first 32 bytes, and the footer stored at rows + nbytes.
__device__ __forceinline__ void close_file(uint8_t* rows, uint64_t nbytes, const uint32_t* __restrict__ piece_crc,
                                           uint32_t filetype, uint32_t flags, uint64_t offset_indexes,
                                           uint64_t num_entries, const uint32_t* s_t) {
  uint32_t c = piece_crc[0];                  // crc(A || B) = crc(B) ^ shift(crc(A), |B|)
  for (uint32_t p = 1; p < kCrcPieces; p++) {
    uint64_t lo, hi;
    crc_piece(nbytes, p, &lo, &hi);
    c = piece_crc[p] ^ crc::shift_n(c, hi - lo);
  }
  uint8_t ft[hs::kFooterSize];
  encode_footer(filetype, flags, offset_indexes, num_entries, ft);
  c ^= 0xFFFFFFFFu;                           // crc32c::Extend
  for (uint32_t i = 0; i < kFooterCrcBytes; i++) c = crc::step(c, ft[i], s_t);
  c ^= 0xFFFFFFFFu;
  for (uint32_t i = 0; i < 4u; i++) ft[kFooterCrcBytes + i] = (uint8_t)(c >> (8u * i));
  uint8_t* dst = rows + nbytes;
  for (uint32_t i = 0; i < hs::kFooterSize; i++) dst[i] = ft[i];
}
#endif

}  // namespace kdb_hstable_close
