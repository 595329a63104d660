// kingdb_amd/csrc/entry_encode.h -- EntryHeader::EncodeTo on the device
// (storage/format.h:224-255, compression enabled) and the CRC-8 of the header
// (crc32c::crc8, algorithm/crc32c.cc:439-475), for the write path (put.hip) and
// for the compaction by copy (compact.hip): one encoder, two callers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kdb_lz4 {
namespace {

// ----------------------------------------------------------------- CRC-8 of the header
// crc32c::crc8 (crc32c.cc:439-475): reflected, polynomial 0xB2, pre/post xor 0xff.
struct Crc8Table {
  uint8_t t[256];
};
constexpr Crc8Table make_crc8() {
  Crc8Table c{};
  for (unsigned i = 0; i < 256; i++) {
    unsigned v = i;
    for (int k = 0; k < 8; k++) v = (v & 1u) ? (v >> 1) ^ 0xB2u : v >> 1;
    c.t[i] = (uint8_t)v;
  }
  return c;
}
__constant__ Crc8Table kCrc8 = make_crc8();

__host__ __device__ __forceinline__ uint32_t varint_len(uint64_t v) {
  uint32_t n = 1;
  while (v >= 128) { v >>= 7; n++; }
  return n;
}
__device__ __forceinline__ uint8_t* put_varint(uint8_t* p, uint64_t v) {
  while (v >= 128) { *p++ = (uint8_t)(v | 128); v >>= 7; }
  *p++ = (uint8_t)v;
  return p;
}

// EntryHeader::EncodeTo's size (compression on: fixed64 size_value_compressed).
__host__ __device__ __forceinline__ uint32_t header_len(uint32_t flags, uint64_t klen, uint64_t size_value,
                                                        uint64_t pad) {
  return 1u + 4u + varint_len(flags) + varint_len(klen) + varint_len(size_value) + 8u + varint_len(pad) + 8u;
}

// The header's hl = header_len(flags, klen, size_value, pad) bytes into
// hdr[0 .. hl): checksum_content, flags, size_key, size_value,
// size_value_compressed, size_padding, hash, and in hdr[0] the CRC-8 of the
// rest.  c8 is the 256-entry table (kCrc8.t, or a copy of it in LDS).
__device__ __forceinline__ void encode_entry_header(uint8_t* hdr, uint32_t hl, uint32_t checksum_content,
                                                    uint32_t flags, uint64_t klen, uint64_t size_value,
                                                    uint64_t svc, uint64_t pad, uint64_t hash, const uint8_t* c8t) {
  uint8_t* q = hdr + 1;
  for (int i = 0; i < 4; i++) *q++ = (uint8_t)(checksum_content >> (8 * i));
  q = put_varint(q, flags);
  q = put_varint(q, klen);
  q = put_varint(q, size_value);
  for (int i = 0; i < 8; i++) *q++ = (uint8_t)(svc >> (8 * i));
  q = put_varint(q, pad);
  for (int i = 0; i < 8; i++) *q++ = (uint8_t)(hash >> (8 * i));
  uint32_t c8 = 0xffu;                        // crc8(0, header + 1, hl - 1)
  for (uint32_t i = 1; i < hl; i++) c8 = c8t[(c8 ^ hdr[i]) & 0xffu];
  hdr[0] = (uint8_t)(c8 ^ 0xffu);
}

}  // namespace
}  // namespace kdb_lz4
