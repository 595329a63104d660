// kingdb_amd/csrc/hstable_decode.h -- decoding what an HSTable file holds, for
// the lookup (index.hip) and for the host (tests/cpp/index_decode_main.cc):
// plain inline functions, no HIP runtime, the same text for hipcc and g++.
//
//   get_varint32 / get_varint64   algorithm/coding.cc:143-200: running past
//                                 the limit, or an over-long encoding, is -1
//   decode_entry_header           EntryHeader::DecodeFrom, compression enabled
//                                 (storage/format.h:164-211), CRC-8 check :213-218
//   entry_valid                   GetEntry's checks (storage_engine.h:491-495,
//                                 format.h:105-108, 140-146)
//   locate_entry                  both, for the entry at `offset` of a file
//   decode_footer, decode_file_header, decode_row
//                                 format.h:397-414, 467-478, 501-521
//
// Every read is checked against the bytes available before it happens.  The
// reference reads the first five header bytes and size_value_compressed
// without a check and never checks that the offset lies in the file
// (storage_engine.h:465-469); here both are decode errors.  Sums of sizes are
// compared without wrapping, so a size_key of 2^63 is invalid, not a small
// number.  With these, locate_entry() == 0 implies that the header, the key
// and size_value_offset() bytes after it lie inside [0, file_size).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KDB_HD __host__ __device__ inline
#else
#define KDB_HD inline
#endif

namespace kdb_hstable {

constexpr uint32_t kTypeDelete = 0x1, kIsUncompacted = 0x2, kHasPadding = 0x4, kEntryFull = 0x8;   // format.h:34-42
constexpr uint64_t kHeaderBlock = 8192;       // internal__hstable_header_size
constexpr uint64_t kFooterSize = 36;          // HSTableFooter::GetFixedSize
constexpr uint64_t kMagic = 0x4D454F57;       // HSTableManager::get_magic_number
constexpr uint64_t kMaxFileSize = 0xFFFFFF00ull;   // entry offsets are 32-bit (OffsetArrayRow)
constexpr uint32_t kMaxEntryHeader = 1 + 4 + 5 + 10 + 10 + 8 + 10 + 8;

constexpr int kDecodeOk = 0, kDecodeError = -1, kDecodeChecksum = -2, kDecodeInvalid = -3;

KDB_HD uint32_t get_fixed32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
KDB_HD uint64_t get_fixed64(const uint8_t* p) {
  return (uint64_t)get_fixed32(p) | ((uint64_t)get_fixed32(p + 4) << 32);
}

// Bytes read, or -1.  At most 5 bytes (shift <= 28); the fifth byte's high
// bits fall off the 32-bit result as in the reference.
KDB_HD int get_varint32(const uint8_t* p, uint64_t size, uint32_t* value) {
  uint32_t result = 0;
  uint64_t i = 0;
  for (uint32_t shift = 0; shift <= 28 && i < size; shift += 7) {
    const uint32_t byte = p[i++];
    if (byte & 128u) {
      result |= (byte & 127u) << shift;
    } else {
      result |= byte << shift;
      *value = result;
      return (int)i;
    }
  }
  return -1;
}
// At most 10 bytes (shift <= 63).
KDB_HD int get_varint64(const uint8_t* p, uint64_t size, uint64_t* value) {
  uint64_t result = 0;
  uint64_t i = 0;
  for (uint32_t shift = 0; shift <= 63 && i < size; shift += 7) {
    const uint64_t byte = p[i++];
    if (byte & 128u) {
      result |= (byte & 127u) << shift;
    } else {
      result |= byte << shift;
      *value = result;
      return (int)i;
    }
  }
  return -1;
}

// crc32c::crc8 (algorithm/crc32c.cc:439-475): reflected, polynomial 0xB2,
// register pre/post-inverted.
KDB_HD uint8_t crc8(const uint8_t* p, uint32_t n) {
  uint32_t c = 0xffu;
  for (uint32_t i = 0; i < n; i++) {
    c ^= p[i];
    for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0xB2u : c >> 1;
  }
  return (uint8_t)(c ^ 0xffu);
}

struct EntryHeader {
  uint8_t checksum_header;
  uint32_t checksum_content;
  uint32_t flags;
  uint64_t size_key;
  uint64_t size_value;
  uint64_t size_value_compressed;
  uint64_t size_padding;
  uint64_t hash;
  uint32_t size_header;        // size_header_serialized
};

KDB_HD bool is_compressed(const EntryHeader& h) { return h.size_value_compressed > 0; }
KDB_HD bool is_uncompacted(const EntryHeader& h) { return (h.flags & kIsUncompacted) != 0; }
// size_value_offset() (format.h:140-146): false where size_value + size_padding wraps
KDB_HD bool size_value_offset(const EntryHeader& h, uint64_t* out) {
  if (!is_compressed(h) || is_uncompacted(h)) {
    *out = h.size_value + h.size_padding;
    return *out >= h.size_value;
  }
  *out = h.size_value_compressed;
  return true;
}

// EntryHeader::DecodeFrom over buf[0 .. size): kDecodeOk, kDecodeError, or
// kDecodeChecksum (verify, header CRC-8 mismatch).
KDB_HD int decode_entry_header(const uint8_t* buf, uint64_t size, bool verify, EntryHeader* out) {
  if (size < 5) return kDecodeError;
  uint64_t at = 0;
  out->checksum_header = buf[0];
  out->checksum_content = get_fixed32(buf + 1);
  at = 5;
  int length = get_varint32(buf + at, size - at, &out->flags);
  if (length < 0) return kDecodeError;
  at += (uint64_t)length;
  length = get_varint64(buf + at, size - at, &out->size_key);
  if (length < 0) return kDecodeError;
  at += (uint64_t)length;
  length = get_varint64(buf + at, size - at, &out->size_value);
  if (length < 0) return kDecodeError;
  at += (uint64_t)length;
  if (size - at < 8) return kDecodeError;
  out->size_value_compressed = get_fixed64(buf + at);
  at += 8;
  length = get_varint64(buf + at, size - at, &out->size_padding);
  if (length < 0) return kDecodeError;
  at += (uint64_t)length;
  if (size - at < 8) return kDecodeError;
  out->hash = get_fixed64(buf + at);
  at += 8;
  out->size_header = (uint32_t)at;
  if (verify && crc8(buf + 1, out->size_header - 1u) != out->checksum_header) return kDecodeChecksum;
  return kDecodeOk;
}

// AreSizesValid && IsEntryFull for the entry at `offset` (offset + size_header
// <= file_size holds after a successful decode).
KDB_HD bool entry_valid(const EntryHeader& h, uint64_t offset, uint64_t file_size) {
  if (h.size_key == 0 || (h.flags & kEntryFull) == 0) return false;
  if (offset > file_size || h.size_header > file_size - offset) return false;
  uint64_t left = file_size - offset - h.size_header;
  if (h.size_key > left) return false;
  left -= h.size_key;
  uint64_t svo;
  if (!size_value_offset(h, &svo)) return false;
  return svo <= left;
}

// GetEntry's header work for the candidate at `offset` of file[0 .. file_size).
KDB_HD int locate_entry(const uint8_t* file, uint64_t file_size, uint64_t offset, bool verify, EntryHeader* out) {
  if (offset >= file_size) return kDecodeError;
  const int r = decode_entry_header(file + offset, file_size - offset, verify, out);
  if (r != kDecodeOk) return r;
  return entry_valid(*out, offset, file_size) ? kDecodeOk : kDecodeInvalid;
}

// key == the stored key of a located entry (serial; the lookup kernel compares
// with the lanes of a wave instead).
KDB_HD bool key_equal(const uint8_t* file, uint64_t offset, const EntryHeader& h, const uint8_t* key,
                      uint64_t key_len) {
  if (h.size_key != key_len) return false;
  const uint8_t* s = file + offset + h.size_header;
  for (uint64_t i = 0; i < key_len; i++)
    if (s[i] != key[i]) return false;
  return true;
}

struct Footer {
  uint32_t filetype, flags;
  uint64_t offset_indexes, num_entries, magic_number;
  uint32_t crc32;
};
// The footer of file[0 .. file_size): false unless the file is larger than
// the header block plus a footer, the magic matches and the offset array lies
// in [kHeaderBlock, file_size - kFooterSize].  (The CRC is the caller's.)
KDB_HD bool decode_footer(const uint8_t* file, uint64_t file_size, Footer* f) {
  if (file_size < kHeaderBlock + kFooterSize) return false;
  const uint8_t* p = file + file_size - kFooterSize;
  f->filetype = get_fixed32(p);
  f->flags = get_fixed32(p + 4);
  f->offset_indexes = get_fixed64(p + 8);
  f->num_entries = get_fixed64(p + 16);
  f->magic_number = get_fixed64(p + 24);
  f->crc32 = get_fixed32(p + 32);
  return f->magic_number == kMagic && f->offset_indexes >= kHeaderBlock &&
         f->offset_indexes <= file_size - kFooterSize;
}

// HSTableHeader's fixed fields; its CRC32C over bytes [4, 24) is the caller's.
struct FileHeader {
  uint32_t crc32, version_major, version_minor, filetype;
  uint64_t timestamp;
};
KDB_HD bool decode_file_header(const uint8_t* file, uint64_t file_size, FileHeader* h) {
  if (file_size < 24) return false;
  h->crc32 = get_fixed32(file);
  h->version_major = get_fixed32(file + 4);
  h->version_minor = get_fixed32(file + 8);
  h->filetype = get_fixed32(file + 12);
  h->timestamp = get_fixed64(file + 16);
  return h->version_major == 1u && h->version_minor == 0u;   // kVersionDataFormat{Major,Minor}
}

// OffsetArrayRow::DecodeFrom: bytes read, or -1.
KDB_HD int decode_row(const uint8_t* p, uint64_t size, uint64_t* hashed_key, uint32_t* offset_entry) {
  const int a = get_varint64(p, size, hashed_key);
  if (a < 0) return -1;
  const int b = get_varint32(p + a, size - (uint64_t)a, offset_entry);
  if (b < 0) return -1;
  return a + b;
}

}  // namespace kdb_hstable
