// kingdb_amd/csrc/index.hip -- Get by key on the GPU: the index over a set of
// closed HSTable files and the batched lookup that feeds kdb_get_values_batch.
//
// Reference semantics:
//   * HSTableManager::LoadDatabase / LoadFile (storage/hstable_manager.h:906-1099):
//     files in (timestamp, fileid) order, each file's offset array inserted row
//     by row into a multimap<hashed key, fileid << 32 | offset>;
//   * StorageEngine::GetWithIndex / GetEntry (storage/storage_engine.h:424-521):
//     the candidates of the key's hash, newest first; EntryHeader::DecodeFrom,
//     the validity checks, the key compare;
//   * Database::GetRaw (interface/database.cc:9-75): a delete entry is
//     NotFound, MultipartRequired for large compressed values.
//
// Load (synchronous, like Database::Open):
//   index_file_kernel    workgroup per file: HSTableHeader, footer, magic,
//                        bounds, CRC32C of the offset array and the footer's
//                        first 32 bytes (crc::extend_block, crc_device.h)
//   host                 files ordered by (timestamp, fileid); the exclusive
//                        sum of num_entries numbers every row (its insertion
//                        order into the reference's multimap)
//   index_count_kernel   terminator bytes (top bit clear) per 256-byte tile
//   scan                 launch_exclusive_scan over the tiles
//   index_parse_kernel   thread per byte: a terminator's rank is its varint's
//                        number; varints 2r and 2r+1 are row r; the owner walks
//                        back to the varint's first byte (across wave and
//                        workgroup boundaries: plain global reads inside the
//                        row region) and assembles the value
//   index_hist_kernel / scan / index_fill_kernel
//                        CSR buckets over hash & (B - 1), B a power of two >= 2 x rows
// Add (include/kdb_index_add.h; StorageEngine::ProcessingLoopIndex,
// storage/storage_engine.h:298-372; synchronous; the load is an add to an
// empty handle): the kernels above over the new files alone, their rows
// appended to the row arrays, then hist / scan / fill over all resident rows
// Tail (include/kdb_index_tail.h; the rest of ProcessingLoopIndex: the file
// still being written): the rows the device writer stages backwards at its
// arena's end while a file is open, parsed by index_count_kernel<true> /
// index_parse_kernel<true> (csrc/index_rows.h) behind the closed files' rows,
// only the bytes staged since the last call; the open file takes the next file
// slot and rank, and hist / scan / fill run over all resident rows
// Staged build and swap: load, add and tail are one transaction (Staged).  Its
// steps build the per-file tables, the rows and the buckets beside the
// handle's, every array owned by a DevBuf (hip_host.h); one commit() swaps in
// what was staged once nothing can fail any more, and leaving before it frees
// what was staged and leaves the handle as it was
// Lookup (stream-ordered):
//   index_get_kernel     wave per key: hash, bucket scan, candidates in
//                        descending sequence number, header decode + checks
//                        (hstable_decode.h), key compare and crc32c(key) on the lanes
//   scan                 64-byte-aligned output slots
//   index_summary_kernel what the host needs to size the decode
// Snapshot (include/kdb_snapshot.h; Database::NewSnapshot, interface/database.cc:301-327,
// interface/snapshot.h): a row limit R, the handle's row count when it was
// taken.  Rows keep their sequence numbers through every add, so the lookup
// and the liveness pass restricted to rows of sequence number < R, over the
// handle's current buckets, answer as a handle loaded over the files held
// then: index_get_kernel<true>, index_live_kernel<true>, and the scan's other
// kernels over the snapshot's own list
// Tail snapshot (include/kdb_live.h): R also counts the rows of the open file
// held as the tail.  The same kernels; the handle keeps those rows in place
// while such a snapshot is open (csrc/live_pin.h), and when the file arrives
// closed index_rows_equal_kernel checks that its first rows are the rows held
// Scan (include/kdb_scan.h; Database::NewIterator, interface/iterator.h:112-214):
//   index_live_kernel    wave per row: the row is live iff the lookup of its
//                        own stored key would select it (prepare, synchronous)
//   scan / index_live_scatter_kernel
//                        the live rows compacted in sequence order into a list
//                        of file rank << 32 | offset: iterator order when every
//                        file's rows ascend
//   index_bitonic_kernel the cold path when they do not: a global-memory
//                        bitonic network over the list padded with ~0
//   scan                 the live keys' lengths -> their places in the packed keys
//   index_scan_emit_kernel
//                        wave per live row of a window: the lookup's outputs
//                        for that entry, and its key (stream-ordered)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <new>
#include <vector>

#include "../../include/kdb_lz4.h"
#include "../../include/kdb_put.h"
#include "crc_device.h"
#include "hash_device.h"
#include "hip_host.h"
#include "hstable_decode.h"
#include "index_rows.h"
#include "live_pin.h"
#include "lz4_device.h"

namespace hs = kdb_hstable;
namespace ir = kdb_index_rows;
namespace lp = kdb_live_pin;

namespace kdb_lz4 {
namespace {

constexpr int kFileBlock = 1024;           // index_file_kernel: 16 waves share one file's CRC
constexpr uint32_t kParseTile = 256;       // bytes of an offset array per workgroup, one per thread
constexpr int kGetBlock = 256;
constexpr uint32_t kKeyStage = 256;        // query keys up to this many bytes are hashed from LDS
constexpr uint32_t kHeaderStage = 64;      // >= hs::kMaxEntryHeader, one byte per lane
static_assert(kHeaderStage >= hs::kMaxEntryHeader && kHeaderStage <= 64, "one load per lane covers a header");
constexpr uint64_t kMaxRows = 1ull << 30;

struct FileRec {
  uint64_t num_entries, offset_indexes, timestamp;
  uint32_t flags;
  int32_t status;
  uint32_t filetype, pad;        // the header's (kdb_index_view_timestamp refuses the large type)
};

struct ParseFile {
  uint64_t reg_off;      // the row region [offset_indexes, size - 36), in the files buffer
  uint64_t reg_len;
  uint64_t nvar;         // 2 * num_entries: the varints that count
  uint64_t row_base;     // sequence number of the file's row 0
  uint32_t first_tile, ntiles;
  uint32_t slot;         // the file's position in the caller's arrays
  uint32_t pad;
};

struct Slot {
  uint64_t hash;
  uint32_t file;         // file slot
  uint32_t offset;       // entry offset in the file
  uint32_t seq;          // insertion order into the reference's multimap
  uint32_t pad;
};

__global__ __launch_bounds__(kFileBlock) void index_file_kernel(const uint8_t* __restrict__ files,
                                                                const uint64_t* __restrict__ file_off,
                                                                const uint64_t* __restrict__ file_size,
                                                                FileRec* __restrict__ rec) {
  constexpr uint32_t kWaves = kFileBlock / 64;
  __shared__ uint32_t s_t[256];
  __shared__ uint32_t s_crc[kWaves];
  __shared__ FileRec s_rec;
  __shared__ uint32_t s_want;
  crc::stage_table(s_t);
  __syncthreads();
  const uint32_t f = blockIdx.x;
  const uint8_t* p = files + file_off[f];
  const uint64_t size = file_size[f];
  if (threadIdx.x == 0) {
    FileRec r{0, 0, 0, 0, 0, 0, 0};
    hs::FileHeader fh;
    hs::Footer ft;
    uint32_t want = 0;
    if (size <= hs::kHeaderBlock || !hs::decode_file_header(p, size, &fh)) {
      r.status = -2;
    } else {
      uint32_t c = 0xFFFFFFFFu;                      // crc32c::Value(buffer + 4, 20), format.h:407
      for (uint32_t i = 4; i < 24; i++) c = crc::step(c, p[i], s_t);
      if ((c ^ 0xFFFFFFFFu) != fh.crc32) {
        r.status = -2;
      } else if (!hs::decode_footer(p, size, &ft)) {
        r.status = -1;
      } else {
        r.num_entries = ft.num_entries;
        r.offset_indexes = ft.offset_indexes;
        r.timestamp = fh.timestamp;
        r.filetype = fh.filetype;
        r.flags = ft.flags;
        want = ft.crc32;
      }
    }
    s_rec = r;
    s_want = want;
  }
  __syncthreads();
  if (s_rec.status != 0) {
    if (threadIdx.x == 0) rec[f] = s_rec;
    return;
  }
  // CRC32C over [offset_indexes, size - 4) (LoadFile:1068); s_rec.status is the same for every thread
  const uint64_t oi = s_rec.offset_indexes;
  const uint32_t c = crc::extend_block<kWaves>(p + oi, size - 4u - oi, s_t, s_crc);   // oi <= size - 36
  if (threadIdx.x == 0) {
    FileRec r = s_rec;
    const uint64_t rows_bytes = size - hs::kFooterSize - oi;
    if (c != s_want) r.status = -1;
    else if (r.num_entries > rows_bytes / 2u) r.status = -3;   // a row is at least two bytes
    rec[f] = r;
  }
}

// Terminators of the tile and, per thread, whether its byte is one.
// kReversed (the tail, include/kdb_index_tail.h): the region is a range of the
// device writer's staging, its byte p at files[reg_off - p]; reads stay inside
// [reg_off - reg_len + 1, reg_off].  The `false` forms of the three functions
// are the ones the load and the add have always run.
template <bool kReversed>
__device__ __forceinline__ bool tile_byte(const uint8_t* __restrict__ files, const ParseFile& F, uint32_t t,
                                          uint64_t* pos_out) {
  const uint64_t pos = (uint64_t)(t - F.first_tile) * kParseTile + threadIdx.x;
  *pos_out = pos;
  return pos < F.reg_len && (files[kReversed ? F.reg_off - pos : F.reg_off + pos] & 0x80u) == 0;
}

template <bool kReversed>
__global__ __launch_bounds__(kParseTile) void index_count_kernel(const uint8_t* __restrict__ files,
                                                                 const ParseFile* __restrict__ pf,
                                                                 const uint32_t* __restrict__ tile_file,
                                                                 uint32_t* __restrict__ tile_count) {
  __shared__ uint32_t s_w[kParseTile / 64];
  const uint32_t t = blockIdx.x;
  const ParseFile F = pf[tile_file[t]];
  uint64_t pos;
  const bool term = tile_byte<kReversed>(files, F, t, &pos);
  const uint64_t m = ballot(term);
  if (lane_id() == 0) s_w[threadIdx.x / 64u] = (uint32_t)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (uint32_t k = 0; k < kParseTile / 64; k++) s += s_w[k];
    tile_count[t] = s;
  }
}

template <bool kReversed>
__global__ __launch_bounds__(kParseTile) void index_parse_kernel(
    const uint8_t* __restrict__ files, const ParseFile* __restrict__ pf, const uint32_t* __restrict__ tile_file,
    const uint64_t* __restrict__ tile_prefix, uint64_t* __restrict__ row_hash, uint32_t* __restrict__ row_off,
    uint32_t* __restrict__ row_file, uint32_t* __restrict__ malformed) {
  __shared__ uint32_t s_w[kParseTile / 64];
  const uint32_t t = blockIdx.x;
  const ParseFile F = pf[tile_file[t]];
  uint64_t pos;
  const bool term = tile_byte<kReversed>(files, F, t, &pos);
  const uint64_t m = ballot(term);
  const uint32_t w = threadIdx.x / 64u;
  if (lane_id() == 0) s_w[w] = (uint32_t)__popcll(m);
  __syncthreads();
  uint64_t k = tile_prefix[t] - tile_prefix[F.first_tile];   // varints of the file before this tile
  uint32_t tile_total = 0;
  for (uint32_t i = 0; i < kParseTile / 64; i++) {
    if (i < w) k += s_w[i];
    tile_total += s_w[i];
  }
  if (kReversed) {
    // a staging range holds exactly its rows: 2 * rows varints, the last byte ending one
    if (threadIdx.x == 0 && t == F.first_tile + F.ntiles - 1u &&
        tile_prefix[t] - tile_prefix[F.first_tile] + tile_total != F.nvar)
      malformed[F.slot] = 1u;
    if (pos == F.reg_len - 1u && !term) malformed[F.slot] = 1u;
  } else {
    if (threadIdx.x == 0 && t == F.first_tile + F.ntiles - 1u &&
        tile_prefix[t] - tile_prefix[F.first_tile] + tile_total < F.nvar)
      malformed[F.slot] = 1u;                                // fewer varints than 2 * num_entries
  }
  if (!term) return;
  k += (uint64_t)__popcll(m & mask_lt(lane_id()));
  if (k >= F.nvar) return;                                    // only the first 2 * num_entries count
  const bool is_offset = (k & 1u) != 0;
  uint64_t v;
  bool ok;
  if (kReversed) ok = ir::varint_ending_at(ir::Reversed{files + F.reg_off}, pos, is_offset, &v);
  else ok = ir::varint_ending_at(files + F.reg_off, pos, is_offset, &v);
  if (!ok) {                                                  // coding.cc:147, 175
    malformed[F.slot] = 1u;
    return;
  }
  const uint64_t r = F.row_base + (k >> 1);
  if (is_offset) {
    row_off[r] = (uint32_t)v;
  } else {
    row_hash[r] = v;
    row_file[r] = F.slot;
  }
}

__global__ void index_hist_kernel(const uint64_t* __restrict__ row_hash, uint32_t n, uint64_t mask,
                                  uint32_t* __restrict__ count) {
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x)
    atomicAdd(&count[row_hash[r] & mask], 1u);
}

// count[b] still holds the bucket's size: each row takes the next free slot from the back.
__global__ void index_fill_kernel(const uint64_t* __restrict__ row_hash, const uint32_t* __restrict__ row_off,
                                  const uint32_t* __restrict__ row_file, uint32_t n, uint64_t mask,
                                  const uint64_t* __restrict__ start, uint32_t* __restrict__ count,
                                  Slot* __restrict__ slots) {
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
    const uint64_t h = row_hash[r];
    const uint64_t b = h & mask;
    const uint32_t at = atomicSub(&count[b], 1u) - 1u;
    slots[start[b] + at] = Slot{h, row_file[r], row_off[r], r, 0u};
  }
}

// The pin's check (include/kdb_live.h): rows [0, n) of the two row arrays --
// the rows the handle holds of the open file, and the same file's rows parsed
// again from its closed form -- must be equal, hash and offset.  One flag.
__global__ void index_rows_equal_kernel(const uint64_t* __restrict__ held_hash,
                                        const uint32_t* __restrict__ held_off,
                                        const uint64_t* __restrict__ new_hash, const uint32_t* __restrict__ new_off,
                                        uint32_t n, uint32_t* __restrict__ mismatch) {
  bool diff = false;
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x)
    diff |= held_hash[r] != new_hash[r] || held_off[r] != new_off[r];
  if (ballot(diff) != 0 && lane_id() == 0) atomicOr(mismatch, 1u);
}

struct IndexView {
  const uint8_t* files;
  const uint64_t* file_off;
  const uint64_t* file_size;
  const uint32_t* fileid;
  const uint64_t* start;     // nbuckets + 1
  const Slot* slots;
  uint64_t mask;             // nbuckets - 1
  uint32_t nrows;
  uint32_t hash_type;
};

typedef uint32_t __attribute__((aligned(1))) u32u;

// LDS bytes written by some lanes of the wave are read by others after this.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint64_t wave_max64(uint64_t x) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const uint64_t o = __shfl_xor((unsigned long long)x, s);
    x = o > x ? o : x;
  }
  return x;
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t x) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) x += __shfl_xor((unsigned long long)x, s);
  return x;
}

// Wave per key.  Everything but the bucket scan, the key compare and the
// key's CRC is the same on every lane (same addresses: broadcast loads).
// kLimited (a snapshot's lookup): ix.nrows is the snapshot's row limit R, not
// the handle's row count, and only slots with seq < R are candidates.  The
// limit rides in a field the kernel reads already, and the `false` form is the
// kernel kdb_index_get_batch has always launched, instruction for instruction
// (same resource figures).
template <bool kLimited>
__global__ __launch_bounds__(kGetBlock) void index_get_kernel(
    IndexView ix, const uint8_t* __restrict__ keys, const uint64_t* __restrict__ key_off,
    const uint32_t* __restrict__ key_len, uint32_t n, int verify_header, uint64_t multipart_required,
    uint64_t* __restrict__ stored_off, uint64_t* __restrict__ avail, uint64_t* __restrict__ svc,
    uint64_t* __restrict__ size, uint32_t* __restrict__ checksum, uint32_t* __restrict__ checksum_initial,
    uint32_t* __restrict__ slot_len, uint64_t* __restrict__ location, int32_t* __restrict__ status) {
  __shared__ uint32_t s_t[256];
  // Per wave: the query key (when it fits) and the candidate's first bytes,
  // fetched by the lanes in one load each.  The hash and the header decode
  // walk bytes one after the other; from global memory every step of those
  // chains is a load of its own (3.65 -> 3.53 ms per 1 Mi lookups of 16-byte
  // keys).
  __shared__ uint8_t s_key[kGetBlock / 64][kKeyStage];
  __shared__ uint8_t s_hdr[kGetBlock / 64][kHeaderStage];
  crc::stage_table(s_t);
  __syncthreads();
  const uint32_t lane = lane_id();
  const uint32_t wib = threadIdx.x / 64u;
  const uint32_t nw = gridDim.x * (kGetBlock / 64);
  for (uint32_t v = blockIdx.x * (kGetBlock / 64) + wib; v < n; v += nw) {
    const uint32_t klen = uni(key_len[v]);
    const uint8_t* key = keys + key_off[v];
    if (klen <= kKeyStage) {
      for (uint32_t i = lane; i < klen; i += 64u) s_key[wib][i] = key[i];
      wave_lds_sync();
      key = s_key[wib];
    }
    const uint64_t h = ix.hash_type == 1 ? xxh64(key, klen) : murmur3_64(key, klen);
    int32_t st = KDB_GET_NOTFOUND;
    uint64_t o_stored = 0, o_avail = 0, o_svc = 0, o_size = 0, o_loc = 0;
    uint32_t o_ck = 0, o_ci = 0;
    if (ix.nrows) {
      const uint64_t b = h & ix.mask;
      const uint64_t s0 = ix.start[b], s1 = ix.start[b + 1u];
      // candidates taken so far have (seq + 1) << 32 | slot >= bound; slot < 2^32,
      // so (R + 1) << 32 admits exactly the slots with seq < R
      uint64_t bound = kLimited ? ((uint64_t)ix.nrows + 1u) << 32 : ~0ull;
      for (;;) {
        uint64_t best = 0;
        for (uint64_t i = s0 + lane; i < s1; i += 64u) {
          const Slot s = ix.slots[i];
          const uint64_t pk = ((uint64_t)s.seq + 1u) << 32 | (uint32_t)(i - s0);
          if (s.hash == h && pk < bound && pk > best) best = pk;
        }
        best = wave_max64(best);
        if (best == 0) break;
        bound = best;
        const Slot c = ix.slots[s0 + (uint32_t)best];
        const uint64_t fo = ix.file_off[c.file], fs = ix.file_size[c.file];
        const uint8_t* file = ix.files + fo;
        hs::EntryHeader hd;
        // locate_entry() on a copy of the candidate's first bytes: a header is
        // at most kMaxEntryHeader <= kHeaderStage bytes, so decoding
        // min(room, kHeaderStage) bytes is decoding all `room` of them.
        // A candidate that does not decode or validate is skipped (GetWithIndex:446).
        const uint64_t room = c.offset < fs ? min(fs - c.offset, (uint64_t)kHeaderStage) : 0u;
        wave_lds_sync();
        if (lane < room) s_hdr[wib][lane] = file[(uint64_t)c.offset + lane];
        wave_lds_sync();
        if (room == 0 || hs::decode_entry_header(s_hdr[wib], room, verify_header != 0, &hd) != hs::kDecodeOk ||
            !hs::entry_valid(hd, c.offset, fs))
          continue;
        if (hd.size_key != klen) continue;
        // locate_entry: [offset + size_header, + size_key) lies inside the file
        const uint8_t* stored_key = file + c.offset + hd.size_header;
        bool diff = false;
        for (uint32_t o = 4u * lane; o < klen; o += 256u) {
          if (o + 4u <= klen) {
            diff |= *reinterpret_cast<const u32u*>(stored_key + o) != *reinterpret_cast<const u32u*>(key + o);
          } else {
            for (uint32_t j = o; j < klen; j++) diff |= stored_key[j] != key[j];
          }
        }
        if (ballot(diff) != 0) continue;
        o_loc = (uint64_t)ix.fileid[c.file] << 32 | c.offset;
        if (hd.flags & hs::kTypeDelete) {                       // database.cc:16, storage_engine.h:511
          st = KDB_GET_DELETED;
        } else if (hs::is_compressed(hd) && hd.size_value > multipart_required) {   // database.cc:60-63
          st = KDB_GET_MULTIPART;
        } else {
          st = 0;
          uint64_t svo = 0;
          hs::size_value_offset(hd, &svo);
          o_stored = fo + c.offset + hd.size_header + klen;
          o_avail = svo;
          o_svc = hd.size_value_compressed;
          o_size = hd.size_value;
          o_ck = hd.checksum_content;
          const crc::BytesMsg msg{key};                               // == the stored key
          o_ci = crc::extend_wave(0u, klen, msg, s_t);          // storage_engine.h:497-500
        }
        break;
      }
    }
    if (lane == 0) {
      stored_off[v] = o_stored;
      avail[v] = o_avail;
      svc[v] = o_svc;
      size[v] = o_size;
      checksum[v] = o_ck;
      checksum_initial[v] = o_ci;
      slot_len[v] = (uint32_t)((o_size + 63u) & ~63ull);
      location[v] = o_loc;
      status[v] = st;
    }
  }
}

// summary: [0] rows found, [1] output bytes (the scan's total), [2] max avail,
// [3] max size, [4] sum of avail / 8 + 1.  One atomic per wave and field.
__global__ __launch_bounds__(256) void index_summary_kernel(const uint64_t* __restrict__ avail,
                                                            const uint64_t* __restrict__ size,
                                                            const int32_t* __restrict__ status, uint32_t n,
                                                            unsigned long long* __restrict__ summary) {
  uint64_t found = 0, max_avail = 0, max_size = 0, frames = 0;
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
    found += status[v] == 0;
    const uint64_t a = avail[v], s = size[v];
    max_avail = a > max_avail ? a : max_avail;
    max_size = s > max_size ? s : max_size;
    frames += a / 8u + 1u;
  }
  found = wave_sum64(found);
  frames = wave_sum64(frames);
  max_avail = wave_max64(max_avail);
  max_size = wave_max64(max_size);
  if (lane_id() == 0) {
    atomicAdd(&summary[0], (unsigned long long)found);
    atomicMax(&summary[2], (unsigned long long)max_avail);
    atomicMax(&summary[3], (unsigned long long)max_size);
    atomicAdd(&summary[4], (unsigned long long)frames);
  }
}

// ------------------------------------------------------------------ scan
// One candidate's first bytes staged in the wave's LDS row and decoded there:
// locate_entry() on a copy.  A header is at most kMaxEntryHeader <=
// kHeaderStage bytes, so decoding min(room, kHeaderStage) bytes is decoding
// all `room` of them.  False where the entry does not decode or validate.
__device__ __forceinline__ bool stage_entry_header(const uint8_t* file, uint64_t fs, uint32_t offset,
                                                   int verify_header, uint8_t* s_hdr, uint32_t lane,
                                                   hs::EntryHeader* hd) {
  const uint64_t room = offset < fs ? min(fs - offset, (uint64_t)kHeaderStage) : 0u;
  wave_lds_sync();
  if (lane < room) s_hdr[lane] = file[(uint64_t)offset + lane];
  wave_lds_sync();
  return room != 0 && hs::decode_entry_header(s_hdr, room, verify_header != 0, hd) == hs::kDecodeOk &&
         hs::entry_valid(*hd, offset, fs);
}

// The candidate walk of index_get_kernel, for the scan's liveness pass: among the slots of h's bucket whose hash equals h and whose
// packed rank (seq + 1) << 32 | position lies above `floor`, newest first, the
// first whose header decodes, is valid (GetWithIndex:446 skips the others) and
// whose stored key equals key[0 .. klen).  floor 0 takes every row;
// (r + 1) << 32 | 0xFFFFFFFF only the rows newer than row r.  `top` is the
// walk's first bound: ~0 takes every row above the floor, (R + 1) << 32 only
// the rows of sequence number < R (a snapshot: rows >= R do not exist for it).
// A second copy of the walk, on purpose: with index_get_kernel calling this
// function instead of its own loop, `locate` measured 3.55-3.57 ms against the
// 3.52-3.53 ms of the unchanged kernel, interleaved on one device (126 VGPRs
// against 125, another spill pattern), which is outside that kernel's own
// run-to-run spread.  So the lookup keeps its text.
__device__ __forceinline__ bool find_candidate(const IndexView& ix, uint64_t h, const uint8_t* key, uint32_t klen,
                                               uint64_t floor, uint64_t top, int verify_header, uint8_t* s_hdr,
                                               uint32_t lane, Slot* c_out, hs::EntryHeader* hd_out,
                                               uint64_t* fo_out) {
  if (ix.nrows == 0) return false;
  const uint64_t b = h & ix.mask;
  const uint64_t s0 = ix.start[b], s1 = ix.start[b + 1u];
  uint64_t bound = top;                 // candidates taken so far have (seq + 1) << 32 | slot >= bound
  for (;;) {
    uint64_t best = floor;
    for (uint64_t i = s0 + lane; i < s1; i += 64u) {
      const Slot s = ix.slots[i];
      const uint64_t pk = ((uint64_t)s.seq + 1u) << 32 | (uint32_t)(i - s0);
      if (s.hash == h && pk < bound && pk > best) best = pk;
    }
    best = wave_max64(best);
    if (best == floor) return false;
    bound = best;
    const Slot c = ix.slots[s0 + (uint32_t)best];
    const uint64_t fo = ix.file_off[c.file], fs = ix.file_size[c.file];
    const uint8_t* file = ix.files + fo;
    hs::EntryHeader hd;
    if (!stage_entry_header(file, fs, c.offset, verify_header, s_hdr, lane, &hd)) continue;
    if (hd.size_key != klen) continue;
    // locate_entry: [offset + size_header, + size_key) lies inside the file
    const uint8_t* stored_key = file + c.offset + hd.size_header;
    bool diff = false;
    for (uint32_t o = 4u * lane; o < klen; o += 256u) {
      if (o + 4u <= klen) {
        diff |= *reinterpret_cast<const u32u*>(stored_key + o) != *reinterpret_cast<const u32u*>(key + o);
      } else {
        for (uint32_t j = o; j < klen; j++) diff |= stored_key[j] != key[j];
      }
    }
    if (ballot(diff) != 0) continue;
    *c_out = c;
    *hd_out = hd;
    *fo_out = fo;
    return true;
  }
}

// What the scan needs beside the lookup's view: the rows in sequence order
// and the files' ranks in that order.
struct RowView {
  const uint64_t* hash;
  const uint32_t* off;
  const uint32_t* file;      // file slot
  const uint32_t* file_rank; // file slot -> rank in (timestamp, fileid) order
};

// stats: [0] some row's offset is not above its predecessor's in the same
// file, [1] key bytes of the live rows, [2] their longest key.
//
// Wave per row r: the row is live iff the lookup of its own stored key would
// select it.  Its entry decodes, is valid and is no delete; the hash of the
// stored key is the row's hash (else Get cannot reach the row); and no newer
// equal-hash row holds a valid entry with the same key.  klen[r] = the key's
// length for a live row, 0 for a dead one (a valid entry's key is not empty).
// kLimited (a snapshot's prepare): ix.nrows is the snapshot's row limit R; the
// pass runs over rows r < R and the walk over newer equal-hash rows examines
// the rows in (r, R) only, so a row whose key is overwritten or deleted only
// by a row >= R is live.  The `false` form passes the constant ~0 and is the
// kernel the handle's own prepare has always run.
template <bool kLimited>
__global__ __launch_bounds__(kGetBlock) void index_live_kernel(IndexView ix, RowView rows, int verify_header,
                                                               uint32_t* __restrict__ flag,
                                                               uint32_t* __restrict__ klen_out,
                                                               unsigned long long* __restrict__ stats) {
  __shared__ uint8_t s_key[kGetBlock / 64][kKeyStage];
  __shared__ uint8_t s_hdr[kGetBlock / 64][kHeaderStage];
  const uint32_t lane = lane_id();
  const uint32_t wib = threadIdx.x / 64u;
  const uint32_t nw = gridDim.x * (kGetBlock / 64);
  uint64_t bytes = 0;
  uint32_t longest = 0;
  bool unordered = false;
  for (uint32_t r = blockIdx.x * (kGetBlock / 64) + wib; r < ix.nrows; r += nw) {
    const uint32_t f = uni(rows.file[r]), off = uni(rows.off[r]);
    const uint64_t h = rows.hash[r];
    if (r > 0 && rows.file[r - 1u] == f && rows.off[r - 1u] >= off) unordered = true;
    const uint64_t fo = ix.file_off[f], fs = ix.file_size[f];
    const uint8_t* file = ix.files + fo;
    uint32_t live_len = 0;
    hs::EntryHeader hd;
    if (stage_entry_header(file, fs, off, verify_header, s_hdr[wib], lane, &hd) &&
        (hd.flags & hs::kTypeDelete) == 0) {
      // entry_valid: the key lies inside the file, so its length fits 32 bits
      const uint32_t klen = (uint32_t)hd.size_key;
      const uint8_t* key = file + off + hd.size_header;
      if (klen <= kKeyStage) {
        for (uint32_t i = lane; i < klen; i += 64u) s_key[wib][i] = key[i];
        wave_lds_sync();
        key = s_key[wib];
      }
      const uint64_t hk = ix.hash_type == 1 ? xxh64(key, klen) : murmur3_64(key, klen);
      Slot c;
      hs::EntryHeader ch;
      uint64_t cfo;
      // no newer equal-hash row (the common case): live without a second header read
      if (hk == h && !find_candidate(ix, h, key, klen, ((uint64_t)r + 1u) << 32 | 0xFFFFFFFFull,
                                     kLimited ? ((uint64_t)ix.nrows + 1u) << 32 : ~0ull, verify_header,
                                     s_hdr[wib], lane, &c, &ch, &cfo))
        live_len = klen;
    }
    if (lane == 0) {
      flag[r] = live_len != 0;
      klen_out[r] = live_len;
    }
    bytes += live_len;
    longest = live_len > longest ? live_len : longest;
  }
  if (lane == 0) {                      // one atomic per wave and field
    if (unordered) atomicOr(&stats[0], 1ull);
    if (bytes) atomicAdd(&stats[1], (unsigned long long)bytes);
    if (longest) atomicMax(&stats[2], (unsigned long long)longest);
  }
}

// Live row r goes to position pos[r] of the live list: rank << 32 | offset,
// so that the list's order is the iterator's and a sort needs no second key.
__global__ void index_live_scatter_kernel(RowView rows, uint32_t n, const uint32_t* __restrict__ flag,
                                          const uint32_t* __restrict__ klen, const uint64_t* __restrict__ pos,
                                          uint64_t* __restrict__ list, uint32_t* __restrict__ list_klen) {
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
    if (!flag[r]) continue;
    const uint64_t at = pos[r];
    list[at] = (uint64_t)rows.file_rank[rows.file[r]] << 32 | rows.off[r];
    list_klen[at] = klen[r];
  }
}

// One compare-exchange step (k, j) of the bitonic network over n = 2^m keys
// (the list padded with ~0), the key lengths carried along.
__global__ void index_bitonic_kernel(uint64_t* __restrict__ key, uint32_t* __restrict__ val, uint32_t n, uint32_t k,
                                     uint32_t j) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t p = i ^ j;
    if (p <= i) continue;               // the lower index of a pair does the work; p < n as j < n = 2^m
    const uint64_t a = key[i], b = key[p];
    const bool up = (i & k) == 0;
    if (up ? a > b : a < b) {
      key[i] = b;
      key[p] = a;
      const uint32_t va = val[i], vb = val[p];
      val[i] = vb;
      val[p] = va;
    }
  }
}

// Wave per live row of the window [first, first + n): the header decoded
// again, the outputs of index_get_kernel for that entry, its key's length and
// place in the packed keys, and the key bytes.
__global__ __launch_bounds__(kGetBlock) void index_scan_emit_kernel(
    IndexView ix, const uint64_t* __restrict__ list, const uint32_t* __restrict__ rank_file,
    const uint64_t* __restrict__ key_prefix, uint64_t first, uint32_t n, uint64_t multipart_required,
    uint8_t* __restrict__ keys_out, uint64_t* __restrict__ key_off, uint32_t* __restrict__ key_len,
    uint64_t* __restrict__ stored_off, uint64_t* __restrict__ avail, uint64_t* __restrict__ svc,
    uint64_t* __restrict__ size, uint32_t* __restrict__ checksum, uint32_t* __restrict__ checksum_initial,
    uint32_t* __restrict__ slot_len, uint64_t* __restrict__ location, int32_t* __restrict__ status) {
  __shared__ uint32_t s_t[256];
  __shared__ uint8_t s_hdr[kGetBlock / 64][kHeaderStage];
  crc::stage_table(s_t);
  __syncthreads();
  const uint32_t lane = lane_id();
  const uint32_t wib = threadIdx.x / 64u;
  const uint32_t nw = gridDim.x * (kGetBlock / 64);
  const uint64_t base = key_prefix[first];
  for (uint32_t v = blockIdx.x * (kGetBlock / 64) + wib; v < n; v += nw) {
    const uint64_t e = list[first + v];
    const uint32_t f = uni(rank_file[(uint32_t)(e >> 32)]), off = uni((uint32_t)e);
    const uint64_t ko = key_prefix[first + v] - base;
    const uint32_t klen = uni((uint32_t)(key_prefix[first + v + 1u] - key_prefix[first + v]));
    const uint64_t fo = ix.file_off[f], fs = ix.file_size[f];
    const uint8_t* file = ix.files + fo;
    int32_t st = KDB_GET_NOTFOUND;
    uint64_t o_stored = 0, o_avail = 0, o_svc = 0, o_size = 0, o_loc = 0;
    uint32_t o_ck = 0, o_ci = 0, o_klen = 0;
    hs::EntryHeader hd;
    // the entry prepare() found live; the files have not changed since, so it
    // decodes to the same header (checked all the same: its key must be the
    // klen bytes the prepared prefix reserved)
    if (stage_entry_header(file, fs, off, 0, s_hdr[wib], lane, &hd) && hd.size_key == klen) {
      const uint8_t* key = file + off + hd.size_header;
      uint8_t* dst = keys_out + ko;
      for (uint32_t o = 4u * lane; o < klen; o += 256u) {
        if (o + 4u <= klen) {
          *reinterpret_cast<u32u*>(dst + o) = *reinterpret_cast<const u32u*>(key + o);
        } else {
          for (uint32_t j = o; j < klen; j++) dst[j] = key[j];
        }
      }
      o_klen = klen;
      o_loc = (uint64_t)ix.fileid[f] << 32 | off;
      if (hs::is_compressed(hd) && hd.size_value > multipart_required) {   // the lookup's rule
        st = KDB_GET_MULTIPART;
      } else {
        st = 0;
        uint64_t svo = 0;
        hs::size_value_offset(hd, &svo);
        o_stored = fo + off + hd.size_header + klen;
        o_avail = svo;
        o_svc = hd.size_value_compressed;
        o_size = hd.size_value;
        o_ck = hd.checksum_content;
        const crc::BytesMsg msg{key};
        o_ci = crc::extend_wave(0u, klen, msg, s_t);          // storage_engine.h:497-500
      }
    }
    if (lane == 0) {
      key_off[v] = ko;
      key_len[v] = o_klen;
      stored_off[v] = o_stored;
      avail[v] = o_avail;
      svc[v] = o_svc;
      size[v] = o_size;
      checksum[v] = o_ck;
      checksum_initial[v] = o_ci;
      slot_len[v] = (uint32_t)((o_size + 63u) & ~63ull);
      location[v] = o_loc;
      status[v] = st;
    }
  }
}

}  // namespace
}  // namespace kdb_lz4

using namespace kdb_lz4;

// A prepared scan (kdb_index_scan_prepare, kdb_snapshot_scan_prepare): the
// live list, rank << 32 | offset in iterator order, and the exclusive sum of
// the live keys' lengths (live + 1 entries, on the device for the emit and on
// the host for the window checks).  The handle has one and every snapshot its
// own; dropping one is assigning a fresh ScanState.
struct ScanState {
  bool ready = false;
  uint64_t live = 0;
  uint64_t closed_live = 0;              // of them, rows below the tail of a tail snapshot (kdb_live.h)
  uint32_t sort_steps = 0;
  std::vector<uint64_t> key_prefix;
  DevBuf<uint64_t> d_key_prefix, d_live;
};

// The closed files per slot, on the host: what kdb_index_add_files extends.
// Mirrors of the device tables, the loaded files' timestamps (the order rule)
// and the headers' file types.
struct HostFiles {
  std::vector<uint64_t> file_off, file_size, timestamp;
  std::vector<uint32_t> fileid, filetype;
  std::vector<int32_t> status;
  std::vector<uint32_t> rank, rank_file;
};

// What a load, an add or a tail replaces, as one value.  The host vectors
// stand before the device buffers, here and in every function that stages
// arrays: members and locals go in reverse order, so the buffers are freed
// first, and hipFree waits for the copies that read the vectors.
// The buffers are declared last freed first, so that they go as they always
// went -- file tables, buckets, rows -- and so do the temporaries of Staged and
// of index_add: freed the other way round, a load and an add were measured
// 0.2 to 0.3 ms slower (profiles/refactor/index_host_timing.txt).
struct IndexArrays {
  HostFiles host;
  uint64_t nbuckets = 0, row_cap = 0;
  DevBuf<uint32_t> d_row_file, d_row_off;
  DevBuf<uint64_t> d_row_hash;           // the rows; they grow geometrically, row_cap has room
  DevBuf<Slot> d_slots;
  DevBuf<uint64_t> d_start;              // the buckets
  DevBuf<uint32_t> d_rank_file;          // rank in (timestamp, fileid) order -> file slot
  DevBuf<uint32_t> d_file_rank;          // and back
  DevBuf<uint32_t> d_fileid;
  DevBuf<uint64_t> d_file_size, d_file_off;
};

struct kdb_snapshot;

struct kdb_index {
  uint32_t hash_type = 1;
  const uint8_t* d_files = nullptr;      // the caller's
  uint32_t nfiles = 0;
  uint64_t nrows = 0;
  IndexArrays a;
  uint32_t nloaded = 0;                  // files of status 0: the ranks in use
  // kdb_index_add_stats
  bool add_done = false;
  uint64_t add_rows_parsed = 0;
  ScanState scan;                        // kdb_index_scan_prepare: dropped by every add
  // open kdb_snapshots: while there are any, the rows keep their sequence
  // numbers (no load) and the handle stays (no destroy)
  uint32_t snapshots = 0;
  // the tail (include/kdb_index_tail.h): the rows of the writer's open file,
  // rows [nrows, nrows + tail.rows) of the row arrays and of the buckets, the
  // file in slot nfiles and rank nloaded of the device arrays.  nrows, nfiles,
  // nloaded and a.host count the closed files alone: they are what an add
  // extends and a snapshot takes.
  struct Tail {
    bool held = false;
    uint32_t fileid = 0;
    uint64_t timestamp = 0, file_off = 0, bytes = 0;
    uint64_t rows = 0, row_bytes = 0;
  } tail;
  uint64_t tail_rows_parsed = 0;         // kdb_index_tail_stats
  uint64_t visible_rows() const { return nrows + tail.rows; }
  // the open tail snapshots whose file has not been added closed
  // (include/kdb_live.h): while there are any, the tail stays the file it is
  std::vector<kdb_snapshot*> pins;
  lp::Pin pin() const;
};

// The handle as of kdb_snapshot_create: its first `nrows` rows, `nfiles` file
// slots and `nloaded` ranks.  Everything else is read from the handle as it is
// when a call comes: the rows, slots and ranks below these counts do not move.
struct kdb_snapshot {
  kdb_index* ix = nullptr;
  uint64_t nrows = 0;
  uint32_t nfiles = 0, nloaded = 0;
  // kdb_snapshot_create_tail: nrows, nfiles and nloaded count the tail held
  // then; closed_rows are the rows below it (= nrows without a tail)
  uint64_t closed_rows = 0;
  bool tail_included = false, pinned = false;
  uint32_t tail_fileid = 0;
  uint64_t tail_rows = 0;
  ScanState scan;
};

lp::Pin kdb_index::pin() const {
  lp::Pin p{!pins.empty(), tail.fileid, tail.timestamp, tail.file_off, 0u};
  for (const kdb_snapshot* s : pins) p.rows = std::max(p.rows, s->tail_rows);
  return p;
}

namespace {

void index_release(kdb_index* ix) {
  ix->scan = ScanState{};
  ix->a = IndexArrays{};
  ix->d_files = nullptr;
  ix->nfiles = ix->nloaded = 0;
  ix->nrows = 0;
  ix->add_done = false;
  ix->add_rows_parsed = 0;
  ix->tail = kdb_index::Tail{};
  ix->tail_rows_parsed = 0;
}

template <class T>
hipError_t upload(hipStream_t st, DevBuf<T>* d, const T* h, size_t n) {
  KDB_TRY(d->alloc(std::max<size_t>(n, 1)));
  if (n) KDB_TRY(hipMemcpyAsync(d->get(), h, n * sizeof(T), hipMemcpyHostToDevice, st));
  return hipSuccess;
}

enum class Refused { kNo, kTooMany, kOrder, kPinned };

// The order rule of an add and, ahead of time, of a tail: see index_rows.h.
bool sorts_after_loaded(const kdb_index* ix, uint64_t timestamp, uint32_t fileid) {
  const HostFiles& h = ix->a.host;
  return ir::sorts_after_loaded(h.timestamp.data(), h.fileid.data(), h.status.data(), ix->nfiles, timestamp, fileid);
}

// One load, add or tail: everything is built here, beside the handle, by the
// steps below, and commit() swaps it in at the very end.  A buffer no step
// filled stays null and means "keep the handle's".  Leaving without commit()
// frees what was staged and leaves the handle as it was; after commit() this
// holds what the handle held before, and frees that.
struct Staged {
  const kdb_index* ix;
  const bool closed_files;               // an add: a.host goes to the handle.  A tail's file is in the device tables only
  IndexArrays a;                         // host: the handle's, copied; the steps extend them
  bool rebuilt = false;                  // build_buckets ran: a.d_start, a.d_slots and a.nbuckets count, null or not
  // temporaries of the steps
  DevBuf<uint32_t> d_count, d_malformed;
  DevBuf<uint64_t> d_tile_prefix;
  DevBuf<uint32_t> d_tile_count, d_tile_file;
  DevBuf<ParseFile> d_pf;

  // (a tail uploads from five of the eight vectors; all are copied, a few words a file)
  Staged(const kdb_index* from, bool closed) : ix(from), closed_files(closed) { a.host = from->a.host; }

  // the row arrays the parse writes and the buckets are built over
  uint64_t* row_hash() const { return a.d_row_hash.get() ? a.d_row_hash.get() : ix->a.d_row_hash.get(); }
  uint32_t* row_off() const { return a.d_row_hash.get() ? a.d_row_off.get() : ix->a.d_row_off.get(); }
  uint32_t* row_file() const { return a.d_row_hash.get() ? a.d_row_file.get() : ix->a.d_row_file.get(); }
  uint64_t row_cap() const { return a.d_row_hash.get() ? a.row_cap : ix->a.row_cap; }

  void append_file(uint64_t off, uint64_t size, uint32_t id) {
    a.host.file_off.push_back(off);
    a.host.file_size.push_back(size);
    a.host.fileid.push_back(id);
  }

  hipError_t upload_file_tables(hipStream_t st, uint32_t nf) {
    KDB_TRY(upload(st, &a.d_file_off, a.host.file_off.data(), nf));
    KDB_TRY(upload(st, &a.d_file_size, a.host.file_size.data(), nf));
    return upload(st, &a.d_fileid, a.host.fileid.data(), nf);
  }

  // An add knows its ranks only after its parse.  The tail knows them at once
  // and uploads them with the file tables: after the parse's synchronise the
  // same two copies cost a refresh 0.1 ms (profiles/refactor/index_host_timing.txt)
  hipError_t upload_ranks(hipStream_t st, uint32_t nf) {
    KDB_TRY(upload(st, &a.d_file_rank, a.host.rank.data(), nf));
    return upload(st, &a.d_rank_file, a.host.rank_file.data(), nf);
  }

  // Room for nrows rows beside the handle's row arrays, their first `keep`
  // rows copied: the arrays grow geometrically past the handle's capacity (a
  // load sizes them exactly) and the handle keeps its own until the swap.
  hipError_t grow_rows(hipStream_t st, uint64_t nrows, uint64_t keep) {
    const uint64_t held = ix->a.row_cap;
    const uint64_t cap = nrows > held ? std::max(nrows, std::min(2u * held, kMaxRows)) : held;
    KDB_TRY(a.d_row_hash.alloc(cap));
    KDB_TRY(a.d_row_off.alloc(cap));
    KDB_TRY(a.d_row_file.alloc(cap));
    if (keep) {
      KDB_TRY(hipMemcpyAsync(a.d_row_hash.get(), ix->a.d_row_hash.get(), keep * 8u, hipMemcpyDeviceToDevice, st));
      KDB_TRY(hipMemcpyAsync(a.d_row_off.get(), ix->a.d_row_off.get(), keep * 4u, hipMemcpyDeviceToDevice, st));
      KDB_TRY(hipMemcpyAsync(a.d_row_file.get(), ix->a.d_row_file.get(), keep * 4u, hipMemcpyDeviceToDevice, st));
    }
    a.row_cap = cap;
    return hipSuccess;
  }

  // count -> scan -> parse over the ntiles tiles of the npf row regions in
  // `files`, into row_hash() / row_off() / row_file() at each region's
  // row_base; `reversed` for the staging of an open file.  tile_file names
  // every tile's region (nullptr: there is one).  Synchronises; of the nf file
  // slots, bad[i] != 0 where the region of slot bad_from + i is malformed.
  hipError_t parse(hipStream_t st, const uint8_t* files, const ParseFile* pf, size_t npf, const uint32_t* tile_file,
                   uint32_t ntiles, bool reversed, uint32_t nf, uint32_t bad_from, uint32_t bad_n, uint32_t* bad) {
    KDB_TRY(upload(st, &d_pf, pf, npf));
    if (tile_file) {
      KDB_TRY(upload(st, &d_tile_file, tile_file, ntiles));
    } else {
      KDB_TRY(d_tile_file.alloc(ntiles));
      KDB_TRY(hipMemsetAsync(d_tile_file.get(), 0, (size_t)ntiles * 4u, st));
    }
    KDB_TRY(d_tile_count.alloc(ntiles));
    KDB_TRY(d_tile_prefix.alloc((size_t)ntiles + 1u));
    KDB_TRY(d_malformed.alloc(nf));
    KDB_TRY(hipMemsetAsync(d_malformed.get(), 0, (size_t)nf * 4u, st));
    const auto count = reversed ? index_count_kernel<true> : index_count_kernel<false>;
    const auto rows = reversed ? index_parse_kernel<true> : index_parse_kernel<false>;
    hipLaunchKernelGGL(count, dim3(ntiles), dim3(kParseTile), 0, st, files, d_pf.get(), d_tile_file.get(),
                       d_tile_count.get());
    KDB_TRY(hipGetLastError());
    KDB_TRY(launch_exclusive_scan(st, d_tile_count.get(), ntiles, d_tile_prefix.get(), d_tile_prefix.get() + ntiles));
    // beyond every row the handle's lookups and scans read now
    hipLaunchKernelGGL(rows, dim3(ntiles), dim3(kParseTile), 0, st, files, d_pf.get(), d_tile_file.get(),
                       d_tile_prefix.get(), row_hash(), row_off(), row_file(), d_malformed.get());
    KDB_TRY(hipGetLastError());
    KDB_TRY(hipMemcpyAsync(bad, d_malformed.get() + bad_from, (size_t)bad_n * 4u, hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
  }

  // The buckets over rows [0, nrows) of row_hash() / row_off() / row_file():
  // built from all resident rows, as a load builds them, whether B doubles or
  // stays -- moving the old slots and placing only the new rows was measured
  // and not kept.  No rows: no buckets, nbuckets = 0
  // (the lookup asks the row count first).
  hipError_t build_buckets(hipStream_t st, uint64_t nrows) {
    rebuilt = true;
    a.nbuckets = 0;
    if (nrows == 0) return hipSuccess;
    uint64_t B = 2;
    while (B < 2u * nrows) B <<= 1;
    const uint32_t n = (uint32_t)nrows;
    KDB_TRY(a.d_start.alloc(B + 1u));
    KDB_TRY(a.d_slots.alloc(nrows));
    KDB_TRY(d_count.alloc(B));
    KDB_TRY(hipMemsetAsync(d_count.get(), 0, B * 4u, st));
    const uint32_t g = grid_for(n, 256, 2048);
    hipLaunchKernelGGL(index_hist_kernel, dim3(g), dim3(256), 0, st, row_hash(), n, B - 1u, d_count.get());
    KDB_TRY(hipGetLastError());
    KDB_TRY(launch_exclusive_scan(st, d_count.get(), (uint32_t)B, a.d_start.get(), a.d_start.get() + B));
    hipLaunchKernelGGL(index_fill_kernel, dim3(g), dim3(256), 0, st, row_hash(), row_off(), row_file(), n, B - 1u,
                       a.d_start.get(), d_count.get(), a.d_slots.get());
    KDB_TRY(hipGetLastError());
    a.nbuckets = B;
    return hipSuccess;
  }

  // Nothing can fail any more: the handle takes what was staged, this what it
  // held.  The caller has synchronised.  The handle's prepared scan goes; a
  // snapshot's list stands on rows that did not move.
  void commit(kdb_index* to) {
    IndexArrays& h = to->a;
    h.d_file_off.swap(a.d_file_off);
    h.d_file_size.swap(a.d_file_size);
    h.d_fileid.swap(a.d_fileid);
    h.d_file_rank.swap(a.d_file_rank);
    h.d_rank_file.swap(a.d_rank_file);
    if (rebuilt) {
      h.d_start.swap(a.d_start);
      h.d_slots.swap(a.d_slots);
      h.nbuckets = a.nbuckets;
    }
    if (a.d_row_hash.get()) {
      h.d_row_hash.swap(a.d_row_hash);
      h.d_row_off.swap(a.d_row_off);
      h.d_row_file.swap(a.d_row_file);
      h.row_cap = a.row_cap;
    }
    if (closed_files) std::swap(h.host, a.host);
    to->scan = ScanState{};
  }
};

// The one way rows get into a handle.  The handle holds nfiles files (none:
// the add is the load); the host arrays describe the nadd new ones, all in
// ix->d_files.  The handle changes only at the end, in the commit.
hipError_t index_add(kdb_index* ix, hipStream_t st, const uint64_t* file_off, const uint64_t* file_size,
                     const uint32_t* fileid, uint32_t nadd, int32_t* file_status, uint64_t* rows_added,
                     Refused* refused) {
  const uint8_t* d_files = ix->d_files;
  const uint32_t nf0 = ix->nfiles, nf = nf0 + nadd;
  const uint64_t nrows0 = ix->nrows;
  std::vector<FileRec> rec(nadd);
  std::vector<int32_t> status(nadd);
  std::vector<uint32_t> order, tile_file, bad(nf);
  std::vector<ParseFile> pf;
  DevBuf<uint32_t> d_mismatch;           // the pin's check
  Staged s(ix, true);
  DevBuf<FileRec> d_rec;
  for (uint32_t f = 0; f < nadd; f++) s.append_file(file_off[f], file_size[f], fileid[f]);
  KDB_TRY(s.upload_file_tables(st, nf));
  if (nadd) {
    KDB_TRY(d_rec.alloc(nadd));
    hipLaunchKernelGGL(index_file_kernel, dim3(nadd), dim3(kFileBlock), 0, st, d_files, s.a.d_file_off.get() + nf0,
                       s.a.d_file_size.get() + nf0, d_rec.get());
    KDB_TRY(hipGetLastError());
    KDB_TRY(hipMemcpyAsync(rec.data(), d_rec.get(), nadd * sizeof(FileRec), hipMemcpyDeviceToHost, st));
  }
  KDB_TRY(hipStreamSynchronize(st));
  for (uint32_t f = 0; f < nadd; f++) status[f] = rec[f].status;

  // LoadDatabase's order (:1007-1014): by (timestamp, fileid), the new files
  // among themselves; their rows are numbered after the rows the handle holds
  uint64_t rows_new = 0, rows_parsed = 0;
  for (;;) {
    order.clear();
    for (uint32_t f = 0; f < nadd; f++)
      if (status[f] == 0) order.push_back(f);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
      if (rec[a].timestamp != rec[b].timestamp) return rec[a].timestamp < rec[b].timestamp;
      return fileid[a] < fileid[b];
    });
    pf.clear();
    tile_file.clear();
    rows_new = 0;
    for (uint32_t f : order) {
      ParseFile p{};
      p.reg_off = file_off[f] + rec[f].offset_indexes;
      p.reg_len = file_size[f] - hs::kFooterSize - rec[f].offset_indexes;
      p.nvar = 2u * rec[f].num_entries;
      p.row_base = nrows0 + rows_new;
      p.first_tile = (uint32_t)tile_file.size();
      p.ntiles = (uint32_t)((p.reg_len + kParseTile - 1u) / kParseTile);
      p.slot = nf0 + f;
      rows_new += rec[f].num_entries;
      if (nrows0 + rows_new > kMaxRows || tile_file.size() + p.ntiles > 0x7FFFFFFFull) {
        *refused = Refused::kTooMany;
        return hipSuccess;
      }
      tile_file.insert(tile_file.end(), p.ntiles, (uint32_t)pf.size());
      pf.push_back(p);
    }
    const uint32_t ntiles = (uint32_t)tile_file.size();
    if (rows_new == 0 || ntiles == 0) break;
    // the handle keeps its own arrays until the swap.  Later passes number
    // fewer rows.  Rows of a tail lie where the new rows go and stay readable
    // until the swap: the new rows go beside them then
    if (nrows0 + rows_new > s.row_cap() || (ix->tail.rows && !s.a.d_row_hash.get()))
      KDB_TRY(s.grow_rows(st, nrows0 + rows_new, nrows0));
    // rows [nrows0, nrows0 + rows_new)
    KDB_TRY(s.parse(st, d_files, pf.data(), pf.size(), tile_file.data(), ntiles, false, nf, 0, nf, bad.data()));
    rows_parsed += rows_new;
    bool again = false;
    for (uint32_t f = 0; f < nadd; f++)
      if (bad[nf0 + f] && status[f] == 0) {
        status[f] = -3;       // no row of a malformed array is kept: number the rows again without it
        again = true;
      }
    if (!again) break;
  }
  for (uint32_t f : order)
    if (!sorts_after_loaded(ix, rec[f].timestamp, fileid[f])) {
      status[f] = KDB_INDEX_FILE_ORDER;
      *refused = Refused::kOrder;
    }
  for (uint32_t f = 0; f < nadd; f++) file_status[f] = status[f];
  if (*refused != Refused::kNo) return hipSuccess;

  // the pin (include/kdb_live.h): the tail's own file arrives first, where it
  // lay, and its first rows are the rows the open tail snapshots stand on
  const lp::Pin pin = ix->pin();
  if (pin.pinned) {
    lp::Request rq{lp::kAdd, false, false, !order.empty(), 0u, 0u, 0u, 0u};
    if (rq.has_file) {
      const uint32_t f = order[0];
      rq.fileid = fileid[f];
      rq.timestamp = rec[f].timestamp;
      rq.file_off = file_off[f];
      rq.num_entries = rec[f].num_entries;
    }
    // rows held and rows parsed lie in arrays of their own (a tail with rows forces grow_rows above)
    if (!lp::allows(pin, rq) || (pin.rows && !s.a.d_row_hash.get())) {
      *refused = Refused::kPinned;
      return hipSuccess;
    }
    if (pin.rows) {
      uint32_t mismatch = 0;
      const uint32_t n = (uint32_t)pin.rows;
      KDB_TRY(d_mismatch.alloc(1));
      KDB_TRY(hipMemsetAsync(d_mismatch.get(), 0, 4u, st));
      hipLaunchKernelGGL(index_rows_equal_kernel, dim3(grid_for(n, 256, 2048)), dim3(256), 0, st,
                         ix->a.d_row_hash.get() + nrows0, ix->a.d_row_off.get() + nrows0, s.row_hash() + nrows0,
                         s.row_off() + nrows0, n, d_mismatch.get());
      KDB_TRY(hipGetLastError());
      KDB_TRY(hipMemcpyAsync(&mismatch, d_mismatch.get(), 4u, hipMemcpyDeviceToHost, st));
      KDB_TRY(hipStreamSynchronize(st));
      if (mismatch) {
        *refused = Refused::kPinned;
        return hipSuccess;
      }
    }
  }

  // the scan orders by the file's rank; a file that did not load has no rows and no rank
  HostFiles& h = s.a.host;
  h.rank.resize(nf, 0xFFFFFFFFu);
  h.rank_file.resize(nf, 0u);
  for (uint32_t i = 0; i < order.size(); i++) {
    h.rank[nf0 + order[i]] = ix->nloaded + i;
    h.rank_file[ix->nloaded + i] = nf0 + order[i];
  }
  KDB_TRY(s.upload_ranks(st, nf));
  for (uint32_t f = 0; f < nadd; f++) {
    h.timestamp.push_back(rec[f].timestamp);
    h.filetype.push_back(rec[f].filetype);
    h.status.push_back(status[f]);
  }
  const uint64_t nrows = nrows0 + rows_new;
  // rows of a tail leave the buckets with it, also where no row comes in
  if (rows_new || ix->tail.rows) KDB_TRY(s.build_buckets(st, nrows));
  KDB_TRY(hipStreamSynchronize(st));

  s.commit(ix);
  ix->nloaded += (uint32_t)order.size();
  ix->nfiles = nf;
  ix->nrows = nrows;
  ix->add_done = true;
  ix->add_rows_parsed = rows_parsed;
  ix->tail = kdb_index::Tail{};          // the file that was open arrives closed, or has: its rows are numbered as they were
  for (kdb_snapshot* sn : ix->pins) sn->pinned = false;    // checked above: from here on ordinary prefix snapshots
  ix->pins.clear();
  *rows_added = rows_new;
  return hipSuccess;
}

// kdb_index_set_tail (f) and kdb_index_drop_tail (f == nullptr): the handle's
// per-file arrays with the open file in the next slot and rank, its staged
// rows parsed behind the closed files' rows, the buckets over all of them;
// built beside the handle and committed at the end, like an add.
hipError_t index_tail(kdb_index* ix, hipStream_t st, const kdb_open_file* f, bool reparse, uint64_t* gained,
                      bool* refused) {
  const kdb_index::Tail held = ix->tail;
  if (!f && !held.held) return hipSuccess;
  const bool grows = f && held.held && held.fileid == f->fileid;
  const bool incremental = grows && !reparse;
  const uint32_t nf0 = ix->nfiles, nf = nf0 + (f ? 1u : 0u);
  const uint64_t nrows0 = ix->nrows, trows = f ? f->rows : 0u, nrows = nrows0 + trows;
  const uint64_t hr = incremental ? held.rows : 0u, hb = incremental ? held.row_bytes : 0u;
  if (f) {
    *refused = true;
    if (nf0 == 0xFFFFFFFFu || f->bytes > hs::kMaxFileSize || f->rows > kMaxRows || nrows > kMaxRows) return hipSuccess;
    // an open file only grows, where it lies
    if (grows && (f->rows < held.rows || f->row_bytes < held.row_bytes || f->bytes < held.bytes ||
                  f->file_off != held.file_off || f->timestamp != held.timestamp))
      return hipSuccess;
    if (!ir::tail_range_ok(hr, hb, f->rows, f->row_bytes, f->rows_last)) return hipSuccess;
    // it closes after every loaded file: index_add's order rule, ahead of time
    if (!sorts_after_loaded(ix, f->timestamp, f->fileid)) return hipSuccess;
    *refused = false;
    if (incremental && f->rows == held.rows && f->row_bytes == held.row_bytes && f->bytes == held.bytes) {
      ix->tail_rows_parsed = 0;            // nothing was appended: nothing changes
      *gained = 0;
      return hipSuccess;
    }
  }
  ParseFile p{};
  uint32_t bad = 0;
  Staged s(ix, false);
  if (f) {
    s.append_file(f->file_off, f->bytes, f->fileid);
    s.a.host.rank.push_back(ix->nloaded);
    s.a.host.rank_file.resize(nf, 0u);
    s.a.host.rank_file[ix->nloaded] = nf0;
  }
  KDB_TRY(s.upload_file_tables(st, nf));
  KDB_TRY(s.upload_ranks(st, nf));

  const uint64_t parsed = trows - hr;
  if (parsed) {
    // rows [nrows0 + hr, nrows): in place only where they lie beyond every
    // row the handle's lookups and scans read now
    if (!incremental || nrows > ix->a.row_cap) KDB_TRY(s.grow_rows(st, nrows, nrows0 + hr));
    p.reg_len = f->row_bytes - hb;         // >= 2 * parsed
    p.reg_off = f->rows_last - hb;         // staged byte hb; the range ends at rows_last - (row_bytes - 1) >= 0
    p.nvar = 2u * parsed;
    p.row_base = nrows0 + hr;
    p.first_tile = 0;
    p.ntiles = (uint32_t)((p.reg_len + kParseTile - 1u) / kParseTile);   // reg_len <= 15 * 2^30
    p.slot = nf0;
    KDB_TRY(s.parse(st, ix->d_files, &p, 1, nullptr, p.ntiles, true, nf, nf0, 1, &bad));
    if (bad) {                        // not two varints per row, or one too long
      *refused = true;
      return hipSuccess;
    }
  }
  KDB_TRY(s.build_buckets(st, nrows));
  KDB_TRY(hipStreamSynchronize(st));

  s.commit(ix);
  ix->tail = f ? kdb_index::Tail{true, f->fileid, f->timestamp, f->file_off, f->bytes, f->rows, f->row_bytes}
               : kdb_index::Tail{};
  ix->tail_rows_parsed = parsed;
  *gained = grows ? trows - held.rows : trows;
  return hipSuccess;
}

}  // namespace

// ------------------------------------------------------------------ C ABI
extern "C" int kdb_index_create(uint32_t hash_type, kdb_index** ix) {
  if (!ix || hash_type > 1) return KDB_PUT_EINVAL;
  kdb_index* p = new (std::nothrow) kdb_index;
  if (!p) return KDB_PUT_EINVAL;
  p->hash_type = hash_type;
  *ix = p;
  return KDB_PUT_OK;
}

extern "C" int kdb_index_destroy(kdb_index* ix) {
  if (!ix || ix->snapshots) return KDB_PUT_EINVAL;
  delete ix;
  return KDB_PUT_OK;
}

extern "C" int kdb_index_load_files(kdb_index* ix, void* stream, const uint8_t* d_files, const uint64_t* file_off,
                                    const uint64_t* file_size, const uint32_t* fileid, uint32_t nfiles,
                                    int32_t* file_status_out, uint64_t* entries_out) {
  if (!ix || ix->snapshots || (nfiles && (!d_files || !file_off || !file_size || !fileid || !file_status_out)))
    return KDB_PUT_EINVAL;
  for (uint32_t f = 0; f < nfiles; f++)
    if (file_size[f] > hs::kMaxFileSize) return KDB_PUT_EINVAL;
  index_release(ix);
  ix->d_files = d_files;
  Refused refused = Refused::kNo;
  uint64_t added = 0;
  const hipError_t e = index_add(ix, (hipStream_t)stream, file_off, file_size, fileid, nfiles, file_status_out,
                                 &added, &refused);
  if (e != hipSuccess || refused != Refused::kNo) {
    index_release(ix);
    return e != hipSuccess ? hip_code(e) : KDB_PUT_EINVAL;
  }
  ix->add_done = false;                  // kdb_index_add_stats speaks of adds
  if (entries_out) *entries_out = ix->nrows;
  return KDB_PUT_OK;
}

extern "C" int kdb_index_add_files(kdb_index* ix, void* stream, const uint8_t* d_files, const uint64_t* file_off,
                                   const uint64_t* file_size, const uint32_t* fileid, uint32_t nadd, uint32_t flags,
                                   int32_t* file_status_out, uint64_t* entries_added_out) {
  if (!ix || (flags & ~KDB_INDEX_ADD_REBUILD) ||
      (nadd && (!d_files || !file_off || !file_size || !fileid || !file_status_out)))
    return KDB_PUT_EINVAL;
  if (entries_added_out) *entries_added_out = 0;
  if (nadd == 0) return KDB_PUT_OK;
  if (nadd > 0xFFFFFFFFu - ix->nfiles || ((ix->nfiles || ix->tail.held) && d_files != ix->d_files))
    return KDB_PUT_EINVAL;
  for (uint32_t f = 0; f < nadd; f++)
    if (file_size[f] > hs::kMaxFileSize) return KDB_PUT_EINVAL;
  const uint8_t* held = ix->d_files;
  ix->d_files = d_files;                 // a handle without files adopts the buffer
  Refused refused = Refused::kNo;
  uint64_t added = 0;
  const hipError_t e = index_add(ix, (hipStream_t)stream, file_off, file_size, fileid, nadd, file_status_out,
                                 &added, &refused);
  if (e != hipSuccess || refused != Refused::kNo) {
    ix->d_files = held;
    return e != hipSuccess ? hip_code(e) : KDB_PUT_EINVAL;
  }
  if (entries_added_out) *entries_added_out = added;
  return KDB_PUT_OK;
}

extern "C" int kdb_index_add_stats(const kdb_index* ix, uint32_t* merged, uint64_t* nbuckets, uint64_t* rows_parsed) {
  if (!ix || !ix->add_done) return KDB_PUT_EINVAL;
  if (merged) *merged = 0u;                // the buckets are always rebuilt
  if (nbuckets) *nbuckets = ix->a.nbuckets;
  if (rows_parsed) *rows_parsed = ix->add_rows_parsed;
  return KDB_PUT_OK;
}

extern "C" int kdb_index_set_tail(kdb_index* ix, void* stream, const uint8_t* d_files, const kdb_open_file* f,
                                  uint32_t flags, uint64_t* rows_added_out) {
  if (rows_added_out) *rows_added_out = 0;
  if (!ix || !f || (flags & ~KDB_INDEX_TAIL_REPARSE)) return KDB_PUT_EINVAL;
  const bool none = !f->open || f->incomplete;
  if (!lp::allows(ix->pin(), lp::Request{lp::kSet, f->open != 0, f->incomplete != 0, false, f->fileid, 0u, 0u, 0u}))
    return KDB_PUT_EINVAL;
  if (!none && (!d_files || ((ix->nfiles || ix->tail.held) && d_files != ix->d_files))) return KDB_PUT_EINVAL;
  const uint8_t* held = ix->d_files;
  if (!none) ix->d_files = d_files;      // a handle without files adopts the buffer
  bool refused = false;
  uint64_t gained = 0;
  const hipError_t e = index_tail(ix, (hipStream_t)stream, none ? nullptr : f, (flags & KDB_INDEX_TAIL_REPARSE) != 0,
                                  &gained, &refused);
  if (e != hipSuccess || refused) {
    ix->d_files = held;
    return e != hipSuccess ? hip_code(e) : KDB_PUT_EINVAL;
  }
  if (none) ix->tail_rows_parsed = 0;
  if (rows_added_out) *rows_added_out = gained;
  return KDB_PUT_OK;
}

extern "C" int kdb_index_drop_tail(kdb_index* ix, void* stream) {
  if (!ix || !lp::allows(ix->pin(), lp::Request{lp::kDrop, false, false, false, 0u, 0u, 0u, 0u})) return KDB_PUT_EINVAL;
  bool refused = false;
  uint64_t gained = 0;
  return hip_code(index_tail(ix, (hipStream_t)stream, nullptr, false, &gained, &refused));
}

extern "C" int kdb_index_tail_stats(const kdb_index* ix, uint32_t* held, uint32_t* fileid, uint64_t* rows,
                                    uint64_t* bytes, uint64_t* rows_parsed_last, uint64_t* nbuckets) {
  if (!ix || !held) return KDB_PUT_EINVAL;
  *held = ix->tail.held ? 1u : 0u;
  if (fileid) *fileid = ix->tail.fileid;
  if (rows) *rows = ix->tail.rows;
  if (bytes) *bytes = ix->tail.bytes;
  if (rows_parsed_last) *rows_parsed_last = ix->tail_rows_parsed;
  if (nbuckets) *nbuckets = ix->a.nbuckets;
  return KDB_PUT_OK;
}

// kdb_compact.h: the timestamp the compacted files lock (storage_engine.h:806-810, 927-934)
extern "C" int kdb_index_view_timestamp(const kdb_index* ix, uint32_t nfiles, uint64_t* timestamp_max) {
  if (!ix || !timestamp_max || nfiles > ix->nfiles) return KDB_PUT_EINVAL;
  const HostFiles& h = ix->a.host;
  uint64_t ts = 0;
  for (uint32_t f = 0; f < nfiles; f++) {
    if (h.status[f] != 0) continue;
    if (h.filetype[f] & 4u) return KDB_PUT_EINVAL;       // kCompactedLargeType
    ts = std::max(ts, h.timestamp[f]);
  }
  *timestamp_max = ts;
  return KDB_PUT_OK;
}

extern "C" int kdb_index_entry_count(const kdb_index* ix, uint64_t* count) {
  if (!ix || !count) return KDB_PUT_EINVAL;
  *count = ix->visible_rows();
  return KDB_PUT_OK;
}

extern "C" int kdb_index_pairs(const kdb_index* ix, uint64_t* hash_out, uint64_t* location_out) {
  if (!ix || (ix->visible_rows() && (!hash_out || !location_out))) return KDB_PUT_EINVAL;
  if (ix->visible_rows() == 0) return KDB_PUT_OK;
  const size_t n = (size_t)ix->visible_rows();
  std::vector<uint32_t> off(n), file(n);
  hipError_t e = hipMemcpy(hash_out, ix->a.d_row_hash.get(), n * 8u, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(off.data(), ix->a.d_row_off.get(), n * 4u, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(file.data(), ix->a.d_row_file.get(), n * 4u, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hip_code(e);
  for (size_t r = 0; r < n; r++) {
    if (file[r] >= ix->nfiles + (ix->tail.held ? 1u : 0u)) return KDB_PUT_EHIP;
    const uint32_t id = file[r] < ix->nfiles ? ix->a.host.fileid[file[r]] : ix->tail.fileid;   // the tail's slot is the next one
    location_out[r] = (uint64_t)id << 32 | off[r];
  }
  return KDB_PUT_OK;
}

extern "C" uint64_t kdb_index_get_scratch_bytes(uint32_t n) { return (uint64_t)n * 4u + 256u; }

namespace {

// The handle's arrays as they are now; nrows is the handle's row count, or a
// snapshot's row limit (index_get_kernel<true>, index_live_kernel<true>).
IndexView view_of(const kdb_index* ix, uint64_t nrows) {
  const IndexArrays& a = ix->a;
  return IndexView{ix->d_files,     a.d_file_off.get(), a.d_file_size.get(),         a.d_fileid.get(), a.d_start.get(),
                   a.d_slots.get(), a.nbuckets ? a.nbuckets - 1u : 0u, (uint32_t)nrows, ix->hash_type};
}

// Workgroups of kGetBlock threads for n items, a wave each.
uint32_t wave_grid(uint32_t n) { return grid_for(n, kGetBlock / 64, 16384); }

// What a lookup batch and a scan batch do before their kernel:
// internal__size_multipart_required where the caller names none, the summary cleared.
hipError_t batch_begin(hipStream_t st, uint64_t* multipart_required, uint64_t* summary) {
  if (*multipart_required == 0) *multipart_required = 1048576u;
  return hipMemsetAsync(summary, 0, 5 * 8, st);
}

// And after it (`launched`: what the launch left): the 64-byte-aligned output
// slots and what the host needs to size the decode, over n >= 1 items.
int batch_end(hipStream_t st, hipError_t launched, const uint32_t* slot_len, uint32_t n, uint64_t* out_off,
              const uint64_t* avail, const uint64_t* size, const int32_t* status, uint64_t* summary) {
  hipError_t e = launched;
  if (e == hipSuccess) e = launch_exclusive_scan(st, slot_len, n, out_off, summary + 1);
  if (e != hipSuccess) return hip_code(e);
  hipLaunchKernelGGL(index_summary_kernel, dim3(grid_for(n, 256, 1024)), dim3(256), 0, st, avail, size, status, n,
                     reinterpret_cast<unsigned long long*>(summary));
  return hip_code(hipGetLastError());
}

// kdb_index_get_batch (snap = nullptr) and kdb_snapshot_get_batch: the same
// checks, scan and summary around index_get_kernel<false> and <true>.
int lookup_batch(const kdb_index* ix, const kdb_snapshot* snap, void* stream, const uint8_t* keys,
                 const uint64_t* key_off, const uint32_t* key_len, uint32_t n, int verify_header,
                 uint64_t multipart_required, uint8_t* scratch, uint64_t scratch_bytes, uint64_t* stored_off,
                 uint64_t* avail, uint64_t* svc, uint64_t* size, uint32_t* checksum, uint32_t* checksum_initial,
                 uint64_t* out_off, uint64_t* location, int32_t* status, uint64_t* summary) {
  if (!ix || !summary || verify_header < 0 || verify_header > 1 || multipart_required > (1ull << 31) ||
      scratch_bytes < kdb_index_get_scratch_bytes(n) ||
      (n && (!keys || !key_off || !key_len || !scratch || !stored_off || !avail || !svc || !size || !checksum ||
             !checksum_initial || !out_off || !location || !status)))
    return KDB_PUT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = batch_begin(st, &multipart_required, summary);
  if (e != hipSuccess) return hip_code(e);
  if (n == 0) return KDB_PUT_OK;
  uint32_t* slot_len = reinterpret_cast<uint32_t*>(scratch);
  // a snapshot: the handle's arrays as they are now, the row count its own limit
  const auto get = snap ? index_get_kernel<true> : index_get_kernel<false>;
  hipLaunchKernelGGL(get, dim3(wave_grid(n)), dim3(kGetBlock), 0, st, view_of(ix, snap ? snap->nrows : ix->visible_rows()),
                     keys, key_off, key_len, n, verify_header, multipart_required, stored_off, avail, svc, size,
                     checksum, checksum_initial, slot_len, location, status);
  return batch_end(st, hipGetLastError(), slot_len, n, out_off, avail, size, status, summary);
}

}  // namespace

extern "C" int kdb_index_get_batch(const kdb_index* ix, void* stream, const uint8_t* keys, const uint64_t* key_off,
                                   const uint32_t* key_len, uint32_t n, int verify_header,
                                   uint64_t multipart_required, uint8_t* scratch, uint64_t scratch_bytes,
                                   uint64_t* stored_off, uint64_t* avail, uint64_t* svc, uint64_t* size,
                                   uint32_t* checksum, uint32_t* checksum_initial, uint64_t* out_off,
                                   uint64_t* location, int32_t* status, uint64_t* summary) {
  return lookup_batch(ix, nullptr, stream, keys, key_off, key_len, n, verify_header, multipart_required, scratch,
                      scratch_bytes, stored_off, avail, svc, size, checksum, checksum_initial, out_off, location,
                      status, summary);
}

// ------------------------------------------------------------------ scan
namespace {

// Temporaries of one prepare, freed on every way out.
struct ScanTemps {
  DevBuf<uint32_t> d_list_klen;
  DevBuf<unsigned long long> d_stats;
  DevBuf<uint64_t> d_pos;                // nrows + 1: the last is the live count
  DevBuf<uint32_t> d_klen, d_flag;
};

// The liveness pass and the ordered list over the handle's first nrows rows,
// into `sc`: all the handle's rows for its own scan (limited = false), a
// snapshot's for the snapshot's.  The rank tables are the handle's current
// ones: the ranks of loaded files do not move.
// closed_rows <= nrows: the rows below a tail snapshot's tail; the live rows
// among them are the exclusive sum of the flags read at that row.
hipError_t scan_prepare(const kdb_index* ix, ScanState* sc, uint64_t nrows, uint64_t closed_rows, bool limited,
                        hipStream_t st, int verify_header, uint64_t* stats_out) {
  unsigned long long stats[3] = {0, 0, 0};
  uint64_t live = 0, closed_live = 0;
  ScanTemps t;
  const uint32_t n = (uint32_t)nrows;
  const bool below_tail = closed_rows < nrows;
  if (n) {
    KDB_TRY(t.d_flag.alloc(n));
    KDB_TRY(t.d_klen.alloc(n));
    KDB_TRY(t.d_pos.alloc((size_t)n + 1u));
    KDB_TRY(t.d_stats.alloc(3));
    KDB_TRY(hipMemsetAsync(t.d_stats.get(), 0, sizeof stats, st));
    const RowView rows{ix->a.d_row_hash.get(), ix->a.d_row_off.get(), ix->a.d_row_file.get(), ix->a.d_file_rank.get()};
    const auto alive = limited ? index_live_kernel<true> : index_live_kernel<false>;
    hipLaunchKernelGGL(alive, dim3(wave_grid(n)), dim3(kGetBlock), 0, st, view_of(ix, nrows), rows, verify_header,
                       t.d_flag.get(), t.d_klen.get(), t.d_stats.get());
    KDB_TRY(hipGetLastError());
    KDB_TRY(launch_exclusive_scan(st, t.d_flag.get(), n, t.d_pos.get(), t.d_pos.get() + n));
    KDB_TRY(hipMemcpyAsync(&live, t.d_pos.get() + n, 8, hipMemcpyDeviceToHost, st));
    if (below_tail)
      KDB_TRY(hipMemcpyAsync(&closed_live, t.d_pos.get() + closed_rows, 8, hipMemcpyDeviceToHost, st));
    KDB_TRY(hipMemcpyAsync(stats, t.d_stats.get(), sizeof stats, hipMemcpyDeviceToHost, st));
    KDB_TRY(hipStreamSynchronize(st));
    // iterator order is (file rank, offset): the compaction gives it unless
    // some file's rows do not ascend; then the list is sorted, padded to a
    // power of two with ~0
    uint64_t cap = live;
    if (stats[0] && live > 1) {
      cap = 2;
      while (cap < live) cap <<= 1;
    }
    KDB_TRY(sc->d_live.alloc(std::max<uint64_t>(cap, 1)));
    KDB_TRY(t.d_list_klen.alloc(std::max<uint64_t>(cap, 1)));
    if (cap > live) {
      KDB_TRY(hipMemsetAsync(sc->d_live.get(), 0xFF, cap * 8u, st));
      KDB_TRY(hipMemsetAsync(t.d_list_klen.get(), 0, cap * 4u, st));
    }
    hipLaunchKernelGGL(index_live_scatter_kernel, dim3(grid_for(n, 256, 2048)), dim3(256), 0, st, rows, n,
                       t.d_flag.get(), t.d_klen.get(), t.d_pos.get(), sc->d_live.get(), t.d_list_klen.get());
    KDB_TRY(hipGetLastError());
    if (cap > live || (stats[0] && live > 1)) {
      const uint32_t m = (uint32_t)cap;
      const uint32_t bg = grid_for(m, 256, 2048);
      for (uint32_t k = 2; k != 0 && k <= m; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
          hipLaunchKernelGGL(index_bitonic_kernel, dim3(bg), dim3(256), 0, st, sc->d_live.get(), t.d_list_klen.get(),
                             m, k, j);
          sc->sort_steps++;
        }
      KDB_TRY(hipGetLastError());
    }
  }
  sc->live = live;
  sc->closed_live = below_tail ? closed_live : live;
  sc->key_prefix.assign((size_t)live + 1u, 0);
  KDB_TRY(sc->d_key_prefix.alloc((size_t)live + 1u));
  if (live) {
    KDB_TRY(launch_exclusive_scan(st, t.d_list_klen.get(), (uint32_t)live, sc->d_key_prefix.get(),
                                  sc->d_key_prefix.get() + live));
    KDB_TRY(hipMemcpyAsync(sc->key_prefix.data(), sc->d_key_prefix.get(), ((size_t)live + 1u) * 8u,
                           hipMemcpyDeviceToHost, st));
  } else {
    KDB_TRY(hipMemsetAsync(sc->d_key_prefix.get(), 0, 8, st));
  }
  KDB_TRY(hipStreamSynchronize(st));
  stats_out[0] = live;
  stats_out[1] = stats[1];
  stats_out[2] = stats[2];
  return hipSuccess;
}

// kdb_index_scan_prepare and kdb_snapshot_scan_prepare.
int scan_prepare_checked(const kdb_index* ix, ScanState* sc, uint64_t nrows, uint64_t closed_rows, bool limited,
                         void* stream, int verify_header, uint64_t* live, uint64_t* key_bytes, uint32_t* max_key_len) {
  *sc = ScanState{};
  uint64_t stats[3] = {0, 0, 0};
  const hipError_t e = scan_prepare(ix, sc, nrows, closed_rows, limited, (hipStream_t)stream, verify_header, stats);
  if (e != hipSuccess) {
    *sc = ScanState{};
    return hip_code(e);
  }
  // the list's own sum of key lengths and the liveness pass's must agree
  if (sc->key_prefix.back() != stats[1]) {
    *sc = ScanState{};
    return KDB_PUT_EHIP;
  }
  sc->ready = true;
  if (live) *live = stats[0];
  if (key_bytes) *key_bytes = stats[1];
  if (max_key_len) *max_key_len = (uint32_t)stats[2];
  return KDB_PUT_OK;
}

// kdb_index_scan_batch and kdb_snapshot_scan_batch: a window of the list `sc`
// holds, read through the handle's current arrays.
int scan_batch(const kdb_index* ix, const ScanState* sc, uint64_t nrows, void* stream, uint64_t first, uint32_t n,
               uint64_t multipart_required, void* scratch, uint64_t scratch_bytes, uint8_t* keys_out,
               uint64_t keys_cap, uint64_t* key_off, uint32_t* key_len, uint64_t* stored_off, uint64_t* avail,
               uint64_t* svc, uint64_t* size, uint32_t* checksum, uint32_t* checksum_initial, uint64_t* out_off,
               uint64_t* location, int32_t* status, uint64_t* summary) {
  if (!ix || !sc->ready || !summary || first > sc->live || n > sc->live - first ||
      scratch_bytes < kdb_index_scan_scratch_bytes(n) ||
      (n && (!scratch || !keys_out || !key_off || !key_len || !stored_off || !avail || !svc || !size || !checksum ||
             !checksum_initial || !out_off || !location || !status)))
    return KDB_PUT_EINVAL;
  if (sc->key_prefix[first + n] - sc->key_prefix[first] > keys_cap) return KDB_PUT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = batch_begin(st, &multipart_required, summary);
  if (e != hipSuccess) return hip_code(e);
  if (n == 0) return KDB_PUT_OK;
  uint32_t* slot_len = reinterpret_cast<uint32_t*>(scratch);
  hipLaunchKernelGGL(index_scan_emit_kernel, dim3(wave_grid(n)), dim3(kGetBlock), 0, st, view_of(ix, nrows),
                     sc->d_live.get(), ix->a.d_rank_file.get(), sc->d_key_prefix.get(), first, n, multipart_required,
                     keys_out, key_off, key_len, stored_off, avail, svc, size, checksum, checksum_initial, slot_len,
                     location, status);
  return batch_end(st, hipGetLastError(), slot_len, n, out_off, avail, size, status, summary);
}

}  // namespace

extern "C" int kdb_index_scan_prepare(kdb_index* ix, void* stream, int verify_header, uint64_t* live,
                                      uint64_t* key_bytes, uint32_t* max_key_len) {
  if (!ix || verify_header < 0 || verify_header > 1) return KDB_PUT_EINVAL;
  return scan_prepare_checked(ix, &ix->scan, ix->visible_rows(), ix->visible_rows(), false, stream, verify_header,
                              live, key_bytes, max_key_len);
}

extern "C" int kdb_index_scan_sort_steps(const kdb_index* ix, uint32_t* steps) {
  if (!ix || !steps || !ix->scan.ready) return KDB_PUT_EINVAL;
  *steps = ix->scan.sort_steps;
  return KDB_PUT_OK;
}

extern "C" uint64_t kdb_index_scan_scratch_bytes(uint32_t n) { return (uint64_t)n * 4u + 256u; }

extern "C" int kdb_index_scan_batch(const kdb_index* ix, void* stream, uint64_t first, uint32_t n,
                                    uint64_t multipart_required, void* scratch, uint64_t scratch_bytes,
                                    uint8_t* keys_out, uint64_t keys_cap, uint64_t* key_off, uint32_t* key_len,
                                    uint64_t* stored_off, uint64_t* avail, uint64_t* svc, uint64_t* size,
                                    uint32_t* checksum, uint32_t* checksum_initial, uint64_t* out_off,
                                    uint64_t* location, int32_t* status, uint64_t* summary) {
  if (!ix) return KDB_PUT_EINVAL;
  return scan_batch(ix, &ix->scan, ix->visible_rows(), stream, first, n, multipart_required, scratch, scratch_bytes, keys_out,
                    keys_cap, key_off, key_len, stored_off, avail, svc, size, checksum, checksum_initial, out_off,
                    location, status, summary);
}

// ------------------------------------------------------------------ snapshot
// Database::NewSnapshot (interface/database.cc:301-327): host bookkeeping alone.
extern "C" int kdb_snapshot_create(kdb_index* ix, kdb_snapshot** snap) {
  if (!ix || !snap || ix->snapshots == 0xFFFFFFFFu) return KDB_PUT_EINVAL;
  kdb_snapshot* p = new (std::nothrow) kdb_snapshot;
  if (!p) return KDB_PUT_EINVAL;
  p->ix = ix;
  p->nrows = p->closed_rows = ix->nrows;
  p->nfiles = ix->nfiles;
  p->nloaded = ix->nloaded;
  ix->snapshots++;
  *snap = p;
  return KDB_PUT_OK;
}

// include/kdb_live.h: the same with the tail held; host bookkeeping alone
extern "C" int kdb_snapshot_create_tail(kdb_index* ix, kdb_snapshot** snap) {
  const int rc = kdb_snapshot_create(ix, snap);
  if (rc != KDB_PUT_OK || !ix->tail.held) return rc;
  kdb_snapshot* p = *snap;
  p->nrows = ix->visible_rows();
  p->nfiles = ix->nfiles + 1u;
  p->nloaded = ix->nloaded + 1u;
  p->tail_included = p->pinned = true;
  p->tail_fileid = ix->tail.fileid;
  p->tail_rows = ix->tail.rows;
  ix->pins.push_back(p);
  return KDB_PUT_OK;
}

extern "C" int kdb_snapshot_tail_stats(const kdb_snapshot* snap, uint32_t* included, uint32_t* fileid, uint64_t* rows,
                                       uint32_t* pinned) {
  if (!snap || !included) return KDB_PUT_EINVAL;
  *included = snap->tail_included ? 1u : 0u;
  if (fileid) *fileid = snap->tail_fileid;
  if (rows) *rows = snap->tail_rows;
  if (pinned) *pinned = snap->pinned ? 1u : 0u;
  return KDB_PUT_OK;
}

extern "C" int kdb_snapshot_scan_closed_live(const kdb_snapshot* snap, uint64_t* n) {
  if (!snap || !n || !snap->scan.ready) return KDB_PUT_EINVAL;
  *n = snap->scan.closed_live;
  return KDB_PUT_OK;
}

// Snapshot::Close (interface/snapshot.h:67-76)
extern "C" int kdb_snapshot_release(kdb_snapshot* snap) {
  if (!snap) return KDB_PUT_EINVAL;
  std::vector<kdb_snapshot*>& pins = snap->ix->pins;
  pins.erase(std::remove(pins.begin(), pins.end(), snap), pins.end());
  snap->ix->snapshots--;
  delete snap;
  return KDB_PUT_OK;
}

extern "C" int kdb_snapshot_entry_count(const kdb_snapshot* snap, uint64_t* count) {
  if (!snap || !count) return KDB_PUT_EINVAL;
  *count = snap->nrows;
  return KDB_PUT_OK;
}

extern "C" int kdb_snapshot_file_count(const kdb_snapshot* snap, uint32_t* count) {
  if (!snap || !count) return KDB_PUT_EINVAL;
  *count = snap->nfiles;
  return KDB_PUT_OK;
}

// Snapshot::Get (interface/snapshot.h:78-92)
extern "C" int kdb_snapshot_get_batch(const kdb_snapshot* snap, void* stream, const uint8_t* keys,
                                      const uint64_t* key_off, const uint32_t* key_len, uint32_t n,
                                      int verify_header, uint64_t multipart_required, uint8_t* scratch,
                                      uint64_t scratch_bytes, uint64_t* stored_off, uint64_t* avail, uint64_t* svc,
                                      uint64_t* size, uint32_t* checksum, uint32_t* checksum_initial,
                                      uint64_t* out_off, uint64_t* location, int32_t* status, uint64_t* summary) {
  if (!snap) return KDB_PUT_EINVAL;
  return lookup_batch(snap->ix, snap, stream, keys, key_off, key_len, n, verify_header, multipart_required, scratch,
                      scratch_bytes, stored_off, avail, svc, size, checksum, checksum_initial, out_off, location,
                      status, summary);
}

// Snapshot::NewIterator (interface/snapshot.h:110-121)
extern "C" int kdb_snapshot_scan_prepare(kdb_snapshot* snap, void* stream, int verify_header, uint64_t* live,
                                         uint64_t* key_bytes, uint32_t* max_key_len) {
  if (!snap || verify_header < 0 || verify_header > 1) return KDB_PUT_EINVAL;
  return scan_prepare_checked(snap->ix, &snap->scan, snap->nrows, snap->closed_rows, true, stream, verify_header,
                              live, key_bytes, max_key_len);
}

extern "C" int kdb_snapshot_scan_sort_steps(const kdb_snapshot* snap, uint32_t* steps) {
  if (!snap || !steps || !snap->scan.ready) return KDB_PUT_EINVAL;
  *steps = snap->scan.sort_steps;
  return KDB_PUT_OK;
}

extern "C" int kdb_snapshot_scan_batch(const kdb_snapshot* snap, void* stream, uint64_t first, uint32_t n,
                                       uint64_t multipart_required, void* scratch, uint64_t scratch_bytes,
                                       uint8_t* keys_out, uint64_t keys_cap, uint64_t* key_off, uint32_t* key_len,
                                       uint64_t* stored_off, uint64_t* avail, uint64_t* svc, uint64_t* size,
                                       uint32_t* checksum, uint32_t* checksum_initial, uint64_t* out_off,
                                       uint64_t* location, int32_t* status, uint64_t* summary) {
  if (!snap) return KDB_PUT_EINVAL;
  return scan_batch(snap->ix, &snap->scan, snap->nrows, stream, first, n, multipart_required, scratch, scratch_bytes,
                    keys_out, keys_cap, key_off, key_len, stored_off, avail, svc, size, checksum, checksum_initial,
                    out_off, location, status, summary);
}
