// kingdb_amd/csrc/recover.hip -- HSTable files without a usable footer,
// recovered on the GPU (include/kdb_recover.h): HSTableManager::RecoverFile
// (storage/hstable_manager.h:1101-1185) and WriteOffsetArray (:381-428), in
// place in the files' slots, byte for byte the file the reference leaves.
//
// The walk is a chain: an entry's length gives the next entry's offset, one
// dependent load per entry as the reference runs it.  Here every byte position
// of a file is tried as if an entry began there (hstable_recover.h,
// recover_step_at: the header CRC-8 rejects nearly every false position), the
// chains are resolved inside 4 KiB tiles in LDS, and only the hop from tile to
// tile is left.  That is folded once more: 32 tiles make a group, the hops
// across a group run side by side for every position of its first tile, and
// what stays sequential is one dependent load per group touched.
//
//   recover_next_kernel   workgroup per tile of file positions [8192 + 4096 t,
//                         + 4096): the tile and a 64-byte halo staged in LDS,
//                         next[p] for every position (thread per position),
//                         then every position follows next[] until the chain
//                         leaves the tile or stops: exit[p], to global scratch
//   recover_hop_kernel    workgroup per group of 32 tiles: for every position
//                         of the group's first tile, the hops over exit[] to
//                         the group's end, side by side: exit2[p]
//   recover_chain_kernel  wave per file: the HSTableHeader check (large type
//                         and bad header end here), then from 8192 the hop
//                         over exit2[] from group to group: the only
//                         sequential part; where it stops is the truncation
//                         offset
//   recover_fill_kernel   thread per group: the hops inside the group again:
//                         entry[t] = where the true chain enters tile t
//   recover_list_kernel   wave per tile with an entry[t]: the true chain
//                         inside the tile walked again from LDS, counted; after
//                         launch_exclusive_scan over the counts, walked once
//                         more to write the entries in file order (offset,
//                         hash, flags, CRC range, checksum_content)
//   recover_crc_kernel    wave per entry with kIsUncompacted: CRC32C of its
//                         range against checksum_content; ranges above 32 KiB
//                         go to recover_crc_big_kernel, a workgroup of 16
//                         waves (crc::extend_block, crc_device.h)
//   recover_rowlen_kernel thread per entry: the length of its row if kept
//   scan x 2              where each row starts; how many are kept
//   recover_rows_kernel   thread per kept entry: varint64(hash) varint32(offset)
//                         at the truncation offset of the file's slot
//   recover_rowcrc_kernel 64 workgroups per file: CRC32C of a piece of its rows
//   recover_close_kernel  wave per file: the pieces' CRCs joined and extended
//                         over the footer's first 32 bytes, the footer, the report
// The row encoder and the closer (the last two kernels' work) are
// hstable_close.h's, shared with the device writer; which rows a file keeps,
// where they lie in its slot (rows_of) and the footer's fields are decided here.
// Every store into a slot is checked against the slot's capacity in the
// kernel that makes it.  All temporaries live in the caller's scratch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/kdb_put.h"
#include "../../include/kdb_recover.h"
#include "crc_device.h"
#include "hip_host.h"
#include "hstable_close.h"
#include "hstable_recover.h"
#include "lz4_device.h"

namespace hs = kdb_hstable;
namespace hsc = kdb_hstable_close;

namespace kdb_lz4 {
namespace {

constexpr uint32_t kTile = 4096;             // file positions per workgroup
constexpr uint32_t kHalo = 64;               // >= hs::kMaxEntryHeader: a header that starts in the tile is staged whole
static_assert(kHalo >= hs::kMaxEntryHeader && kHalo % 4 == 0, "the halo covers a header");
constexpr int kNextBlock = 256;
constexpr uint32_t kGroup = 32;              // tiles per hop of the sequential chain
constexpr uint32_t kMaxSteps = kTile / (uint32_t)hs::kMinEntry + 2u;   // entries of one chain inside a tile
constexpr int kBigBlock = 1024;              // recover_crc_big_kernel / recover_rowcrc_kernel: 16 waves
constexpr uint64_t kBigCrc = 32768;          // CRC ranges above this take a workgroup
constexpr uint32_t kEntCheck = 1, kEntPadding = 2;
constexpr uint32_t kHdrLarge = 1, kHdrBad = 2;  // large type (RecoverFile gives up); no usable header (LoadDatabase skips)

struct FileIn {
  uint64_t off, size, cap;
  uint64_t exit_base;        // exit[exit_base + p - 8192] belongs to position p
  uint32_t tile_first, ntiles;
  uint32_t group_first, pad;   // groups of kGroup tiles
};

struct FileState {
  uint32_t hdr_bad, filetype;  // hdr_bad: 0, kHdrLarge or kHdrBad
  uint32_t trunc;            // where the walk stops
  uint32_t footer_flags;     // kFooterHasPadding from recover_rowlen_kernel, kFooterHasInvalid at the close
  uint32_t chain_steps;
  int32_t status;
  uint64_t new_size, walked, kept;
};

struct Entries {
  uint32_t *off, *file, *flags, *begin, *len, *want, *keep, *rowlen;
  uint64_t* hash;
};

// The file that owns tile t: the last one whose first tile is <= t (a file
// without tiles shares its first tile with the file after it).
__device__ __forceinline__ uint32_t file_of_tile(const FileIn* __restrict__ files, uint32_t nfiles, uint32_t t) {
  uint32_t l = 0, r = nfiles;
  while (l < r) {
    const uint32_t m = l + (r - l) / 2u;
    if (files[m].tile_first > t) r = m;
    else l = m + 1u;
  }
  return l - 1u;                              // files[0].tile_first == 0 <= t
}

__device__ __forceinline__ uint32_t file_of_group(const FileIn* __restrict__ files, uint32_t nfiles, uint32_t g) {
  uint32_t l = 0, r = nfiles;
  while (l < r) {
    const uint32_t m = l + (r - l) / 2u;
    if (files[m].group_first > g) r = m;
    else l = m + 1u;
  }
  return l - 1u;
}

// Bytes [t0, t0 + kTile + kHalo) of the file, as far as the file goes, into
// LDS: aligned dwords (file offsets and t0 are multiples of 4; the last dword
// may reach up to 3 bytes past the file, inside its slot).
__device__ __forceinline__ void stage_tile(const uint8_t* __restrict__ file, uint64_t size, uint64_t t0, uint32_t* s_w) {
  const uint64_t have = min(size - t0, (uint64_t)(kTile + kHalo));
  const uint32_t nd = (uint32_t)((have + 3u) / 4u);
  const uint32_t* src = reinterpret_cast<const uint32_t*>(file + t0);
  for (uint32_t i = threadIdx.x; i < nd; i += blockDim.x) s_w[i] = src[i];
}

__global__ __launch_bounds__(kNextBlock) void recover_next_kernel(const uint8_t* __restrict__ d_files,
                                                                  const FileIn* __restrict__ files, uint32_t nfiles,
                                                                  uint32_t* __restrict__ exit_pos) {
  __shared__ uint32_t s_w[(kTile + kHalo) / 4];
  __shared__ uint32_t s_next[kTile];
  const uint32_t t = blockIdx.x;
  const FileIn F = files[file_of_tile(files, nfiles, t)];
  const uint64_t t0 = hs::kHeaderBlock + (uint64_t)(t - F.tile_first) * kTile, tile_end = t0 + kTile;
  stage_tile(d_files + F.off, F.size, t0, s_w);
  __syncthreads();
  const uint8_t* s_b = reinterpret_cast<const uint8_t*>(s_w);
  // speculate: as if an entry began at every position
  for (uint32_t i = threadIdx.x; i < kTile; i += kNextBlock) {
    const uint64_t pos = t0 + i;
    uint64_t nxt = pos;                       // next == position: the walk stops here
    if (pos < F.size) {
      hs::EntryHeader h;
      uint64_t len = 0;
      if (hs::recover_step_at(s_b + i, F.size - pos, &h, &len) == hs::kDecodeOk) nxt = pos + len;
    }
    s_next[i] = (uint32_t)nxt;                // <= size < 2^32
  }
  __syncthreads();
  // resolve: follow the chain to where it leaves the tile or stops (next > position: every loop ends)
  for (uint32_t i = threadIdx.x; i < kTile; i += kNextBlock) {
    const uint64_t pos = t0 + i;
    if (pos >= F.size) break;
    uint64_t q = pos;
    for (uint32_t s = 0; s < kMaxSteps; s++) {
      const uint64_t n = s_next[q - t0];
      if (n <= q || n >= tile_end) {
        q = n <= q ? q : n;
        break;
      }
      q = n;
    }
    exit_pos[F.exit_base + (pos - hs::kHeaderBlock)] = (uint32_t)q;
  }
}

__device__ __forceinline__ uint32_t crc32c_bits(const uint8_t* p, uint32_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (uint32_t i = 0; i < n; i++) {
    c ^= p[i];
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0x82F63B78u & (0u - (c & 1u)));
  }
  return c ^ 0xFFFFFFFFu;
}

// A group is kGroup consecutive tiles of a file.  For every position p of a
// group's first tile: exit2 = where the chain from p, hopping over exit[] tile
// by tile, first reaches the group's end or beyond -- or, a position inside
// the group, where it stops.  At most kGroup dependent loads per thread,
// 4096 threads' worth of them side by side per group.
__global__ __launch_bounds__(kNextBlock) void recover_hop_kernel(const FileIn* __restrict__ files, uint32_t nfiles,
                                                                 const uint32_t* __restrict__ exit_pos,
                                                                 uint32_t* __restrict__ exit2) {
  const uint32_t gi = blockIdx.x;
  const FileIn F = files[file_of_group(files, nfiles, gi)];
  const uint64_t g0 = hs::kHeaderBlock + (uint64_t)(gi - F.group_first) * kGroup * kTile;
  const uint64_t group_end = g0 + (uint64_t)kGroup * kTile;
  for (uint32_t i = threadIdx.x; i < kTile; i += kNextBlock) {
    const uint64_t pos = g0 + i;
    if (pos >= F.size) break;
    uint64_t q = pos;
    for (uint32_t s = 0; s < kGroup; s++) {     // every hop lands in a later tile
      if (q >= F.size || q >= group_end) break;
      const uint64_t tile_end = hs::kHeaderBlock + ((q - hs::kHeaderBlock) / kTile + 1u) * kTile;
      const uint64_t e = exit_pos[F.exit_base + (q - hs::kHeaderBlock)];
      const bool stopped = e < tile_end;        // a position inside the tile: the chain stopped there
      q = e < q ? q : e;
      if (stopped) break;
    }
    exit2[(uint64_t)gi * kTile + i] = (uint32_t)q;
  }
}

// Wave per file (one lane works): the HSTableHeader check, then the only
// sequential part, the hop from group to group over exit2[].  A chain that
// enters a group behind its first tile (an entry longer than a tile carried
// it there) goes on tile by tile over exit[] until it meets a first tile.
__global__ __launch_bounds__(64) void recover_chain_kernel(const uint8_t* __restrict__ d_files,
                                                           const FileIn* __restrict__ files,
                                                           const uint32_t* __restrict__ exit_pos,
                                                           const uint32_t* __restrict__ exit2,
                                                           uint32_t* __restrict__ tile_entry,
                                                           uint32_t* __restrict__ group_entry,
                                                           FileState* __restrict__ state) {
  if (threadIdx.x != 0) return;
  const uint32_t f = blockIdx.x;
  const FileIn F = files[f];
  const uint8_t* p = d_files + F.off;
  FileState S{};
  S.trunc = (uint32_t)hs::kHeaderBlock;
  hs::FileHeader fh;
  const bool bad = F.size <= hs::kHeaderBlock || !hs::decode_file_header(p, F.size, &fh) ||
                   crc32c_bits(p + 4, 20) != fh.crc32;
  if (bad || (fh.filetype & hs::kCompactedLargeType)) {
    S.hdr_bad = bad ? kHdrBad : kHdrLarge;
    state[f] = S;
    return;
  }
  S.filetype = hs::recover_filetype(fh.filetype);
  uint64_t q = hs::kHeaderBlock;
  uint32_t steps = 0;
  while (q < F.size && steps < F.ntiles) {    // every hop lands in a later tile
    const uint64_t lt = (q - hs::kHeaderBlock) / kTile;
    uint64_t e, end;
    if (lt % kGroup == 0) {
      const uint64_t g = lt / kGroup;
      group_entry[F.group_first + g] = (uint32_t)q;
      e = exit2[(F.group_first + g) * kTile + (q - (hs::kHeaderBlock + lt * kTile))];
      end = hs::kHeaderBlock + (g + 1u) * kGroup * kTile;
    } else {
      tile_entry[F.tile_first + lt] = (uint32_t)q;
      e = exit_pos[F.exit_base + (q - hs::kHeaderBlock)];
      end = hs::kHeaderBlock + (lt + 1u) * kTile;
    }
    steps++;
    const bool stopped = e < end;             // a position before the end: the chain stopped there
    q = e < q ? q : e;
    if (stopped) break;
  }
  S.trunc = (uint32_t)min(q, F.size);
  S.chain_steps = steps;
  state[f] = S;
}

// Thread per group the chain entered at its first tile: the hops inside the
// group once more, entry[t] recorded for every tile touched.
__global__ __launch_bounds__(256) void recover_fill_kernel(const FileIn* __restrict__ files, uint32_t nfiles,
                                                           uint32_t ngroups, const uint32_t* __restrict__ exit_pos,
                                                           const uint32_t* __restrict__ group_entry,
                                                           uint32_t* __restrict__ tile_entry) {
  const uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x;
  if (gi >= ngroups) return;
  uint64_t q = group_entry[gi];
  if (q == 0) return;
  const FileIn F = files[file_of_group(files, nfiles, gi)];
  const uint64_t group_end = hs::kHeaderBlock + (uint64_t)(gi - F.group_first + 1u) * kGroup * kTile;
  for (uint32_t s = 0; s < kGroup; s++) {
    if (q >= F.size || q >= group_end) break;
    const uint64_t lt = (q - hs::kHeaderBlock) / kTile;
    tile_entry[F.tile_first + lt] = (uint32_t)q;
    const uint64_t e = exit_pos[F.exit_base + (q - hs::kHeaderBlock)];
    if (e < hs::kHeaderBlock + (lt + 1u) * kTile) break;      // stopped inside the tile
    q = e;
  }
}

// The true chain inside tile t, from where the hop entered it to the tile's
// end or the truncation offset.  kWrite false: counted; true: listed at the
// tile's place in the entry arrays.
template <bool kWrite>
__global__ __launch_bounds__(64) void recover_list_kernel(const uint8_t* __restrict__ d_files,
                                                          const FileIn* __restrict__ files, uint32_t nfiles,
                                                          const FileState* __restrict__ state,
                                                          const uint32_t* __restrict__ tile_entry,
                                                          uint32_t* __restrict__ tile_count,
                                                          const uint64_t* __restrict__ tile_prefix, uint32_t crc_scope,
                                                          Entries E) {
  __shared__ uint32_t s_w[(kTile + kHalo) / 4];
  const uint32_t t = blockIdx.x;
  const uint32_t start = tile_entry[t];
  if (start == 0u) {                          // the chain never enters this tile
    if (!kWrite && threadIdx.x == 0) tile_count[t] = 0u;
    return;
  }
  const uint32_t f = file_of_tile(files, nfiles, t);
  const FileIn F = files[f];
  const uint64_t t0 = hs::kHeaderBlock + (uint64_t)(t - F.tile_first) * kTile, tile_end = t0 + kTile;
  stage_tile(d_files + F.off, F.size, t0, s_w);
  __syncthreads();
  if (threadIdx.x != 0) return;
  const uint8_t* s_b = reinterpret_cast<const uint8_t*>(s_w);
  const uint64_t trunc = state[f].trunc;
  const uint64_t base = kWrite ? tile_prefix[t] : 0u, room = kWrite ? tile_prefix[t + 1u] - base : kMaxSteps;
  uint64_t q = start;
  uint32_t count = 0;
  while (q >= t0 && q < tile_end && q < trunc && count < room) {
    hs::EntryHeader h;
    uint64_t len = 0;
    if (hs::recover_step_at(s_b + (q - t0), F.size - q, &h, &len) != hs::kDecodeOk) break;
    if (kWrite) {
      const uint64_t e = base + count;
      uint32_t flags = (h.flags & hs::kHasPadding) ? kEntPadding : 0u;
      uint32_t keep = 1u;
      uint64_t begin = 0, n = 0;
      if (hs::is_uncompacted(h)) {
        bool key_only;
        if (hs::recover_crc_range(h, q, F.size, crc_scope, &begin, &n, &key_only)) flags |= kEntCheck;
        keep = 0u;                            // until the CRC kernel says otherwise; a range past the file: invalid
      }
      E.off[e] = (uint32_t)q;
      E.file[e] = f;
      E.flags[e] = flags;
      E.begin[e] = (uint32_t)begin;
      E.len[e] = (uint32_t)n;
      E.want[e] = h.checksum_content;
      E.keep[e] = keep;
      E.hash[e] = h.hash;
    }
    count++;
    q += len;
  }
  if (!kWrite) tile_count[t] = count;
}

__global__ __launch_bounds__(256) void recover_crc_kernel(const uint8_t* __restrict__ d_files,
                                                          const FileIn* __restrict__ files, Entries E, uint32_t n) {
  __shared__ uint32_t s_t[256];
  crc::stage_table(s_t);
  __syncthreads();
  const uint32_t nw = gridDim.x * 4u;
  for (uint32_t e = blockIdx.x * 4u + threadIdx.x / 64u; e < n; e += nw) {
    if (!(E.flags[e] & kEntCheck)) continue;
    const uint64_t len = E.len[e];
    if (len > kBigCrc) continue;
    const FileIn& F = files[E.file[e]];
    const uint64_t begin = E.begin[e];
    if (begin > F.size || len > F.size - begin) continue;
    const crc::BytesMsg msg{d_files + F.off + begin};
    const uint32_t c = crc::extend_wave(0u, len, msg, s_t);
    if (lane_id() == 0) E.keep[e] = c == E.want[e] ? 1u : 0u;
  }
}

__global__ __launch_bounds__(kBigBlock) void recover_crc_big_kernel(const uint8_t* __restrict__ d_files,
                                                                    const FileIn* __restrict__ files, Entries E,
                                                                    uint32_t n) {
  __shared__ uint32_t s_t[256];
  __shared__ uint32_t s_crc[kBigBlock / 64];
  crc::stage_table(s_t);
  __syncthreads();
  for (uint32_t e = blockIdx.x; e < n; e += gridDim.x) {      // the same for every thread of the workgroup
    if (!(E.flags[e] & kEntCheck)) continue;
    const uint64_t len = E.len[e];
    if (len <= kBigCrc) continue;
    const FileIn& F = files[E.file[e]];
    const uint64_t begin = E.begin[e];
    if (begin > F.size || len > F.size - begin) continue;
    const uint32_t c = crc::extend_block<kBigBlock / 64>(d_files + F.off + begin, len, s_t, s_crc);
    if (threadIdx.x == 0) E.keep[e] = c == E.want[e] ? 1u : 0u;
  }
}

__global__ __launch_bounds__(256) void recover_rowlen_kernel(Entries E, uint32_t n, FileState* __restrict__ state) {
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
    E.rowlen[e] = E.keep[e] ? hsc::row_len(E.hash[e], E.off[e]) : 0u;
    if (E.flags[e] & kEntPadding) atomicOr(&state[E.file[e]].footer_flags, hs::kFooterHasPadding);
  }
}

__global__ __launch_bounds__(256) void recover_rows_kernel(uint8_t* __restrict__ d_files,
                                                           const FileIn* __restrict__ files,
                                                           const FileState* __restrict__ state, Entries E, uint32_t n,
                                                           const uint64_t* __restrict__ tile_prefix,
                                                           const uint64_t* __restrict__ R) {
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
    const uint32_t rl = E.rowlen[e];
    if (rl == 0) continue;
    const uint32_t f = E.file[e];
    const FileIn& F = files[f];
    const uint64_t first = tile_prefix[F.tile_first];           // the file's first entry
    const uint64_t pos = (uint64_t)state[f].trunc + (R[e] - R[first]);
    if (pos > F.cap || rl > F.cap - pos) continue;
    uint8_t* dst = d_files + F.off + pos;
    hsc::put_row(E.hash[e], E.off[e], rl, [&](uint32_t k, uint8_t byte) { dst[k] = byte; });
  }
}

// Where a recovered file's rows lie and how many they are; false for a file
// the reference removes (no tiles, or no entry) or whose slot is too small
// (the bound rules that out).
struct Rows {
  uint64_t at, nbytes, kept, walked;
};
__device__ __forceinline__ bool rows_of(const FileIn& F, const FileState& S, const uint64_t* __restrict__ tile_prefix,
                                        const uint64_t* __restrict__ R, const uint64_t* __restrict__ K, Rows* out) {
  if (S.hdr_bad || S.trunc <= hs::kHeaderBlock) return false;
  // trunc > 8192: the file has tiles and at least one entry
  const uint64_t first = tile_prefix[F.tile_first], last = tile_prefix[F.tile_first + F.ntiles];
  *out = Rows{S.trunc, R[last] - R[first], K[last] - K[first], last - first};
  return out->at <= F.cap && out->nbytes <= F.cap - out->at && hs::kFooterSize <= F.cap - out->at - out->nbytes;
}

// crc32c of piece blockIdx.x % kCrcPieces of the rows of file blockIdx.x / kCrcPieces.
__global__ __launch_bounds__(kBigBlock) void recover_rowcrc_kernel(const uint8_t* __restrict__ d_files,
                                                                   const FileIn* __restrict__ files,
                                                                   const FileState* __restrict__ state,
                                                                   const uint64_t* __restrict__ tile_prefix,
                                                                   const uint64_t* __restrict__ R,
                                                                   const uint64_t* __restrict__ K,
                                                                   uint32_t* __restrict__ piece_crc) {
  __shared__ uint32_t s_t[256];
  __shared__ uint32_t s_crc[kBigBlock / 64];
  const uint32_t f = blockIdx.x / hsc::kCrcPieces, p = blockIdx.x % hsc::kCrcPieces;
  const FileIn F = files[f];
  Rows rows;
  if (!rows_of(F, state[f], tile_prefix, R, K, &rows)) return;
  crc::stage_table(s_t);
  __syncthreads();
  const uint32_t c = hsc::rows_piece_crc<kBigBlock / 64>(d_files + F.off + rows.at, rows.nbytes, p, s_t, s_crc);
  if (threadIdx.x == 0) piece_crc[(uint64_t)f * hsc::kCrcPieces + p] = c;
}

// Wave per file: the pieces' CRCs joined, extended over the footer's first 32
// bytes, the footer, and what the host is told.
__global__ __launch_bounds__(64) void recover_close_kernel(uint8_t* __restrict__ d_files,
                                                           const FileIn* __restrict__ files,
                                                           FileState* __restrict__ state,
                                                           const uint64_t* __restrict__ tile_prefix,
                                                           const uint64_t* __restrict__ R,
                                                           const uint64_t* __restrict__ K,
                                                           const uint32_t* __restrict__ piece_crc) {
  __shared__ uint32_t s_t[256];
  const uint32_t f = blockIdx.x;
  const FileIn F = files[f];
  const FileState S = state[f];
  Rows rows;
  if (!rows_of(F, S, tile_prefix, R, K, &rows)) {
    if (threadIdx.x == 0) {
      state[f].status = S.hdr_bad == kHdrBad     ? KDB_RECOVER_BADHEADER
                        : S.hdr_bad == kHdrLarge ? KDB_RECOVER_LARGE
                        : S.trunc <= hs::kHeaderBlock ? KDB_RECOVER_NOENTRY      // the reference removes the file
                                                      : KDB_PUT_EHIP;
      state[f].new_size = 0;
    }
    return;
  }
  crc::stage_table(s_t);
  __syncthreads();
  if (threadIdx.x != 0) return;
  const uint32_t flags = (S.footer_flags & hs::kFooterHasPadding) | (rows.kept < rows.walked ? hs::kFooterHasInvalid : 0u);
  hsc::close_file(d_files + F.off + rows.at, rows.nbytes, piece_crc + (uint64_t)f * hsc::kCrcPieces, S.filetype, flags,
                  rows.at, rows.kept, s_t);
  FileState O = S;
  O.status = 0;
  O.new_size = rows.at + rows.nbytes + hs::kFooterSize;
  O.walked = rows.walked;
  O.kept = rows.kept;
  O.footer_flags = flags;
  state[f] = O;
}

// The scratch's arrays for files of these sizes.
struct Scratch {
  FileIn* files;
  FileState* state;
  uint32_t *exit_pos, *tile_entry, *tile_count, *piece_crc, *exit2, *group_entry;
  uint64_t *tile_prefix, *R, *K;
  Entries E;
  uint64_t positions, ntiles, ngroups, cap;  // exit[] entries, tiles, groups, most entries
  uint64_t bytes;
};

bool carve(uint8_t* base, const uint64_t* file_size, uint32_t nfiles, Scratch* out) {
  Scratch k{};
  if (nfiles > (1u << 20)) return false;     // kCrcPieces workgroups per file in one grid
  for (uint32_t f = 0; f < nfiles; f++) {
    if (file_size[f] >= hs::kMaxFileSize) return false;
    if (file_size[f] <= hs::kHeaderBlock) continue;
    const uint64_t body = file_size[f] - hs::kHeaderBlock;
    k.positions += body;
    k.ntiles += (body + kTile - 1u) / kTile;
    k.ngroups += (body + (uint64_t)kGroup * kTile - 1u) / ((uint64_t)kGroup * kTile);
    k.cap += body / hs::kMinEntry;
  }
  if (k.ntiles > 0x7FFFFFFFull || k.cap > 0x7FFFFFFFull) return false;
  uint64_t at = 0;
  auto take = [&](uint64_t bytes) {
    uint8_t* p = base ? base + at : nullptr;
    at += align256(std::max<uint64_t>(bytes, 1));
    return p;
  };
  k.files = reinterpret_cast<FileIn*>(take((uint64_t)nfiles * sizeof(FileIn)));
  k.state = reinterpret_cast<FileState*>(take((uint64_t)nfiles * sizeof(FileState)));
  k.exit_pos = reinterpret_cast<uint32_t*>(take(k.positions * 4u));
  k.exit2 = reinterpret_cast<uint32_t*>(take(k.ngroups * kTile * 4u));
  k.group_entry = reinterpret_cast<uint32_t*>(take(k.ngroups * 4u));
  k.tile_entry = reinterpret_cast<uint32_t*>(take(k.ntiles * 4u));
  k.tile_count = reinterpret_cast<uint32_t*>(take(k.ntiles * 4u));
  k.tile_prefix = reinterpret_cast<uint64_t*>(take((k.ntiles + 1u) * 8u));
  k.piece_crc = reinterpret_cast<uint32_t*>(take((uint64_t)nfiles * hsc::kCrcPieces * 4u));
  uint32_t** u32s[] = {&k.E.off, &k.E.file, &k.E.flags, &k.E.begin, &k.E.len, &k.E.want, &k.E.keep, &k.E.rowlen};
  for (uint32_t** p : u32s) *p = reinterpret_cast<uint32_t*>(take(k.cap * 4u));
  k.E.hash = reinterpret_cast<uint64_t*>(take(k.cap * 8u));
  k.R = reinterpret_cast<uint64_t*>(take((k.cap + 1u) * 8u));
  k.K = reinterpret_cast<uint64_t*>(take((k.cap + 1u) * 8u));
  k.bytes = at;
  *out = k;
  return true;
}

// The timing events of a call that asks for its parts' times (ms != nullptr).
struct Events {
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  ~Events() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

hipError_t recover(hipStream_t st, uint8_t* d_files, const uint64_t* file_off, const uint64_t* file_size,
                   const uint64_t* file_cap, uint32_t nfiles, uint32_t crc_scope, const Scratch& k,
                   std::vector<FileState>* states, float* ms) {
  Events evs;
  if (ms)
    for (hipEvent_t& e : evs.ev) KDB_TRY(hipEventCreate(&e));
  auto mark = [&](int i) { return ms ? hipEventRecord(evs.ev[i], st) : hipSuccess; };
  std::vector<FileIn> in(nfiles);
  uint64_t exit_base = 0;
  uint32_t tile = 0, group = 0;
  for (uint32_t f = 0; f < nfiles; f++) {
    const uint64_t body = file_size[f] > hs::kHeaderBlock ? file_size[f] - hs::kHeaderBlock : 0u;
    in[f] = FileIn{file_off[f], file_size[f], file_cap[f], exit_base, tile, (uint32_t)((body + kTile - 1u) / kTile),
                   group, 0u};
    exit_base += body;
    tile += in[f].ntiles;
    group += (in[f].ntiles + kGroup - 1u) / kGroup;
  }
  const uint32_t ntiles = tile, ngroups = group;
  KDB_TRY(hipMemcpyAsync(k.files, in.data(), nfiles * sizeof(FileIn), hipMemcpyHostToDevice, st));
  KDB_TRY(hipMemsetAsync(k.state, 0, nfiles * sizeof(FileState), st));
  if (ntiles) {
    KDB_TRY(hipMemsetAsync(k.tile_entry, 0, (size_t)ntiles * 4u, st));
    KDB_TRY(hipMemsetAsync(k.group_entry, 0, (size_t)ngroups * 4u, st));
  }
  KDB_TRY(mark(0));
  if (ntiles) {
    hipLaunchKernelGGL(recover_next_kernel, dim3(ntiles), dim3(kNextBlock), 0, st, d_files, k.files, nfiles,
                       k.exit_pos);
    KDB_TRY(hipGetLastError());
  }
  KDB_TRY(mark(1));
  if (ntiles) {
    hipLaunchKernelGGL(recover_hop_kernel, dim3(ngroups), dim3(kNextBlock), 0, st, k.files, nfiles, k.exit_pos, k.exit2);
    KDB_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(recover_chain_kernel, dim3(nfiles), dim3(64), 0, st, d_files, k.files, k.exit_pos, k.exit2,
                     k.tile_entry, k.group_entry, k.state);
  KDB_TRY(hipGetLastError());
  if (ntiles) {
    hipLaunchKernelGGL(recover_fill_kernel, dim3(grid_for(ngroups, 256, 1u << 30)), dim3(256), 0, st, k.files, nfiles,
                       ngroups, k.exit_pos, k.group_entry, k.tile_entry);
    KDB_TRY(hipGetLastError());
  }
  KDB_TRY(mark(2));
  uint64_t n64 = 0;
  if (ntiles) {
    hipLaunchKernelGGL(recover_list_kernel<false>, dim3(ntiles), dim3(64), 0, st, d_files, k.files, nfiles, k.state,
                       k.tile_entry, k.tile_count, k.tile_prefix, crc_scope, k.E);
    KDB_TRY(hipGetLastError());
    KDB_TRY(launch_exclusive_scan(st, k.tile_count, ntiles, k.tile_prefix, k.tile_prefix + ntiles));
    KDB_TRY(hipMemcpyAsync(&n64, k.tile_prefix + ntiles, 8, hipMemcpyDeviceToHost, st));
  }
  KDB_TRY(hipStreamSynchronize(st));           // the entry count sizes the launches below; `in` has gone up
  if (n64 > k.cap) return hipErrorUnknown;     // an entry is at least kMinEntry bytes
  const uint32_t n = (uint32_t)n64;
  if (n) {
    hipLaunchKernelGGL(recover_list_kernel<true>, dim3(ntiles), dim3(64), 0, st, d_files, k.files, nfiles, k.state,
                       k.tile_entry, k.tile_count, k.tile_prefix, crc_scope, k.E);
    KDB_TRY(hipGetLastError());
  }
  KDB_TRY(mark(3));
  if (n) {
    hipLaunchKernelGGL(recover_crc_kernel, dim3(grid_for(n, 4, 16384)), dim3(256), 0, st, d_files, k.files, k.E, n);
    KDB_TRY(hipGetLastError());
    hipLaunchKernelGGL(recover_crc_big_kernel, dim3(grid_for(n, 1, 1024)), dim3(kBigBlock), 0, st, d_files, k.files,
                       k.E, n);
    KDB_TRY(hipGetLastError());
  }
  KDB_TRY(mark(4));
  if (n) {
    const uint32_t g = grid_for(n, 256, 4096);
    hipLaunchKernelGGL(recover_rowlen_kernel, dim3(g), dim3(256), 0, st, k.E, n, k.state);
    KDB_TRY(hipGetLastError());
    KDB_TRY(launch_exclusive_scan(st, k.E.rowlen, n, k.R, k.R + n));
    KDB_TRY(launch_exclusive_scan(st, k.E.keep, n, k.K, k.K + n));
    hipLaunchKernelGGL(recover_rows_kernel, dim3(g), dim3(256), 0, st, d_files, k.files, k.state, k.E, n,
                       k.tile_prefix, k.R);
    KDB_TRY(hipGetLastError());
  }
  if (n) {
    hipLaunchKernelGGL(recover_rowcrc_kernel, dim3(nfiles * hsc::kCrcPieces), dim3(kBigBlock), 0, st, d_files, k.files,
                       k.state, k.tile_prefix, k.R, k.K, k.piece_crc);
    KDB_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(recover_close_kernel, dim3(nfiles), dim3(64), 0, st, d_files, k.files, k.state, k.tile_prefix, k.R,
                     k.K, k.piece_crc);
  KDB_TRY(hipGetLastError());
  KDB_TRY(mark(5));
  states->resize(nfiles);
  KDB_TRY(hipMemcpyAsync(states->data(), k.state, nfiles * sizeof(FileState), hipMemcpyDeviceToHost, st));
  KDB_TRY(hipStreamSynchronize(st));
  if (ms) {
    for (int i = 0; i < 5; i++) KDB_TRY(hipEventElapsedTime(&ms[i], evs.ev[i], evs.ev[i + 1]));
    KDB_TRY(hipEventElapsedTime(&ms[5], evs.ev[0], evs.ev[5]));
  }
  return hipSuccess;
}

}  // namespace
}  // namespace kdb_lz4

using namespace kdb_lz4;

// ------------------------------------------------------------------ C ABI
extern "C" uint64_t kdb_hstable_recover_bound(uint64_t file_size) { return hs::recover_bound(file_size); }

extern "C" uint64_t kdb_hstable_recover_scratch_bytes(const uint64_t* file_size, uint32_t nfiles) {
  Scratch k;
  if ((nfiles && !file_size) || !carve(nullptr, file_size, nfiles, &k)) return ~0ull;
  return k.bytes;
}

extern "C" int kdb_hstable_recover_files_timed(void* stream, uint8_t* d_files, const uint64_t* file_off,
                                               const uint64_t* file_size, const uint64_t* file_cap, uint32_t nfiles,
                                               uint32_t crc_scope, void* d_scratch, uint64_t scratch_bytes,
                                               uint64_t* new_size, int32_t* status,
                                               struct kdb_recover_report* report, float* ms) {
  if (ms) memset(ms, 0, 6 * sizeof(float));
  if (nfiles == 0) return KDB_PUT_OK;
  if (!d_files || !file_off || !file_size || !file_cap || !d_scratch || !new_size || !status ||
      crc_scope > KDB_RECOVER_CONTENT || (reinterpret_cast<uintptr_t>(d_files) & 3u) ||
      (reinterpret_cast<uintptr_t>(d_scratch) & 255u))
    return KDB_PUT_EINVAL;
  for (uint32_t f = 0; f < nfiles; f++)
    if (file_size[f] >= hs::kMaxFileSize || (file_off[f] & 3u) || file_cap[f] < hs::recover_bound(file_size[f]))
      return KDB_PUT_EINVAL;
  Scratch k;
  if (!carve(static_cast<uint8_t*>(d_scratch), file_size, nfiles, &k) || scratch_bytes < k.bytes) return KDB_PUT_EINVAL;
  std::vector<FileState> states;
  const hipError_t e = recover((hipStream_t)stream, d_files, file_off, file_size, file_cap, nfiles, crc_scope, k,
                               &states, ms);
  if (e != hipSuccess) return hip_code(e);
  for (uint32_t f = 0; f < nfiles; f++) {
    const FileState& s = states[f];
    if (s.status > 0 || s.status == KDB_PUT_EHIP) return KDB_PUT_EHIP;
    status[f] = s.status;
    new_size[f] = s.new_size;
    if (report) {
      const bool ok = s.status == 0;
      report[f] = kdb_recover_report{ok ? s.walked : 0u, ok ? s.kept : 0u, ok ? s.walked - s.kept : 0u,
                                     s.hdr_bad ? 0u : s.trunc, ok ? s.footer_flags : 0u, s.chain_steps};
    }
  }
  return KDB_PUT_OK;
}

extern "C" int kdb_hstable_recover_files(void* stream, uint8_t* d_files, const uint64_t* file_off,
                                         const uint64_t* file_size, const uint64_t* file_cap, uint32_t nfiles,
                                         uint32_t crc_scope, void* d_scratch, uint64_t scratch_bytes,
                                         uint64_t* new_size, int32_t* status, struct kdb_recover_report* report) {
  return kdb_hstable_recover_files_timed(stream, d_files, file_off, file_size, file_cap, nfiles, crc_scope, d_scratch,
                                         scratch_bytes, new_size, status, report, nullptr);
}
