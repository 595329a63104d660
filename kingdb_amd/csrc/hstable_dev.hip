// kingdb_amd/csrc/hstable_dev.hip -- HSTable files written on the GPU
// (include/kdb_hstable_dev.h): what hstable.cc does on the host -- where a
// file is cut, the varint rows of its offset array, the 8 KiB header block,
// the footer and its CRC32C -- over the outputs of kdb_put_entries_batch where
// they lie, into one device buffer, byte for byte the host writer's files.
//
// One append (stream-ordered, one synchronisation):
//   hsd_prepare_kernel   thread per entry: effective length and the three
//                        flags (valid, kind != 0, kind == 2)
//   scan x 4             launch_exclusive_scan (pack.hip): P, CV, CM, C2
//   hsd_plan_kernel      one lane: the chain over files (hstable_cut.h), one
//                        FileRec per file touched; refusals are flags in the
//                        plan's head, nothing is written
//   hsd_rowlen_kernel    thread per entry: its record (binary search over the
//                        records' first entries) and the length of its row,
//                        varint64(hash) + varint32(offset in the file)
//   scan                 R: where each row starts among the batch's rows
//   hsd_rowsum_kernel    thread per record: the bytes of its rows
//   download             the head and the records: all an append brings down.
//                        The host checks the arena's capacity, places the
//                        files and uploads one Place per record
//   hsd_unstage_kernel   a carried file that closes: its staged rows (stored
//                        backwards from the arena's end) go behind its entries
//   hsd_rows_kernel      thread per entry: the row's bytes, behind the entries
//                        of a closing file or into the staging of the open one
//   hsd_copy_kernel      wave per entry: its bytes, dword stores on the
//                        destination side (the alignbyte copy of pack.hip)
//   hsd_header_kernel    workgroup per opened file: the header block
//   hsd_crc_kernel       64 workgroups per closing file: CRC32C of a piece of
//                        its rows (hstable_close.h, rows_piece_crc)
//   hsd_close_kernel     wave per closing file: the pieces' CRCs joined,
//                        extended over the footer's first 32 bytes, and the
//                        footer (hstable_close.h, close_file)
// Every store into the arena is checked against the arena's size in the kernel
// that makes it, whatever the plan or the caller's arrays say.  The row
// encoder and the closer are hstable_close.h's, shared with recover.hip; where
// the rows lie and what the footer says is decided here.
// kdb_index_load_files shares the CRC primitives (crc_device.h) and the format
// constants (hstable_decode.h) with this file.  It still verifies every footer
// CRC and parses every row with kernels and decode functions of its own:
// decode_footer and encode_footer stay separate texts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/kdb_put.h"
#include "crc_device.h"
#include "hip_host.h"
#include "hstable_close.h"
#include "hstable_cut.h"
#include "lz4_device.h"

namespace hs = kdb_hstable;
namespace cut = kdb_hstable_cut;
namespace hsc = kdb_hstable_close;

namespace kdb_lz4 {
namespace {

constexpr uint32_t kHeadRecs = 64;            // records that come down with the head in one copy
constexpr int kCloseBlock = 1024;             // hsd_crc_kernel: 16 waves share one piece's CRC
constexpr uint32_t kRefusedOffset = 1, kRefusedRecords = 2;

struct PlanHead {
  uint32_t nrec, refused, pad0, pad1;
};

// Where the host put a record's file.
constexpr uint32_t kRowsNone = 0, kRowsFinal = 1, kRowsStaged = 2;
struct Place {
  uint64_t base;          // the file's offset in the arena
  uint64_t rows_at;       // kRowsFinal: arena offset of this batch's first row; kRowsStaged: its place in the staging
  uint64_t staged;        // closing carried file: staged bytes that go in front of this batch's rows
  uint64_t rows_total;    // closing file: bytes of all its rows
  uint64_t nrows_total;   // and their number
  uint32_t rows_mode, pad;
  uint8_t hdr[72];        // opened file: HSTableHeader + DatabaseOptionEncoder
};

__device__ __forceinline__ bool in_arena(uint64_t off, uint64_t len, uint64_t arena_bytes) {
  return off <= arena_bytes && len <= arena_bytes - off;
}

__global__ __launch_bounds__(256) void hsd_prepare_kernel(const uint32_t* __restrict__ len,
                                                          const uint32_t* __restrict__ kind,
                                                          const int32_t* __restrict__ status, uint32_t n,
                                                          uint32_t* __restrict__ eff, uint32_t* __restrict__ valid,
                                                          uint32_t* __restrict__ marked,
                                                          uint32_t* __restrict__ unfinished) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const bool ok = status[i] == 0;
    const uint32_t k = kind[i];
    eff[i] = ok ? len[i] : 0u;
    valid[i] = ok ? 1u : 0u;
    marked[i] = ok && k != 0u ? 1u : 0u;
    unfinished[i] = ok && k == 2u ? 1u : 0u;
  }
}

__global__ __launch_bounds__(64) void hsd_plan_kernel(cut::Prefix A, uint64_t sb, cut::State st,
                                                      PlanHead* __restrict__ head, cut::FileRec* __restrict__ recs,
                                                      uint32_t cap) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  uint32_t nrec = 0, refused = 0;
  const bool ok = cut::plan_batch(A, sb, &st, [&](const cut::FileRec& r) {
    if (nrec >= cap) {
      refused |= kRefusedRecords;
      return false;
    }
    recs[nrec++] = r;
    return true;
  });
  if (!ok && !refused) refused |= kRefusedOffset;
  *head = PlanHead{nrec, refused, 0u, 0u};
}

// The record that holds entry i: the last one whose first entry is <= i (a
// record without entries shares its `first` with the one after it).
__device__ __forceinline__ uint32_t record_of(const cut::FileRec* __restrict__ recs, uint32_t nrec, uint32_t i) {
  uint32_t l = 0, r = nrec;
  while (l < r) {
    const uint32_t m = l + (r - l) / 2u;
    if (recs[m].first > i) r = m;
    else l = m + 1u;
  }
  if (l == 0) return ~0u;
  const cut::FileRec& f = recs[l - 1u];
  return i - f.first < f.count ? l - 1u : ~0u;
}

__global__ __launch_bounds__(256) void hsd_rowlen_kernel(const PlanHead* __restrict__ head,
                                                         const cut::FileRec* __restrict__ recs,
                                                         const int32_t* __restrict__ status,
                                                         const uint64_t* __restrict__ hashed,
                                                         const uint64_t* __restrict__ P, uint32_t n, uint32_t cap,
                                                         uint32_t* __restrict__ rowlen, uint32_t* __restrict__ erec) {
  const uint32_t nrec = head->refused ? 0u : min(head->nrec, cap);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    uint32_t r = ~0u, rl = 0;
    if (status[i] == 0) r = record_of(recs, nrec, i);
    if (r != ~0u) {
      const cut::FileRec& f = recs[r];
      if (!(f.flags & cut::kIncomplete)) {
        const uint64_t off = f.fs + (P[i] - P[f.first]);
        rl = hsc::row_len(hashed[i], (uint32_t)off);
      }
    }
    rowlen[i] = rl;
    erec[i] = r;
  }
}

__global__ __launch_bounds__(64) void hsd_rowsum_kernel(const PlanHead* __restrict__ head,
                                                        cut::FileRec* __restrict__ recs,
                                                        const uint64_t* __restrict__ R, uint32_t n, uint32_t cap) {
  const uint32_t nrec = head->refused ? 0u : min(head->nrec, cap);
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < nrec; r += gridDim.x * blockDim.x) {
    const uint32_t a = recs[r].first, b = a + recs[r].count;
    recs[r].row_bytes = a <= n && b <= n && a <= b ? R[b] - R[a] : 0u;
  }
}

// Byte b of the staging lies at arena[arena_bytes - 1 - b].
__global__ __launch_bounds__(256) void hsd_unstage_kernel(uint8_t* __restrict__ arena, uint64_t arena_bytes,
                                                          uint64_t dst, uint64_t bytes) {
  if (!in_arena(dst, bytes, arena_bytes) || bytes > arena_bytes - (dst + bytes)) return;   // the two ranges are apart
  for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < bytes; b += (uint64_t)gridDim.x * blockDim.x)
    arena[dst + b] = arena[arena_bytes - 1u - b];
}

__global__ __launch_bounds__(256) void hsd_rows_kernel(uint8_t* __restrict__ arena, uint64_t arena_bytes,
                                                       const cut::FileRec* __restrict__ recs,
                                                       const Place* __restrict__ places, uint32_t nrec,
                                                       const uint64_t* __restrict__ hashed,
                                                       const uint64_t* __restrict__ P, const uint64_t* __restrict__ R,
                                                       const uint32_t* __restrict__ rowlen,
                                                       const uint32_t* __restrict__ erec, uint32_t n) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t r = erec[i], rl = rowlen[i];
    if (r >= nrec || rl == 0) continue;
    const cut::FileRec& f = recs[r];
    const Place& pl = places[r];
    if (pl.rows_mode == kRowsNone) continue;
    const uint64_t pos = pl.rows_at + (R[i] - R[f.first]);
    if (!in_arena(pos, rl, arena_bytes)) continue;
    // forwards behind the entries, or backwards from the arena's end
    const bool staged = pl.rows_mode == kRowsStaged;
    const uint64_t off = f.fs + (P[i] - P[f.first]);
    hsc::put_row(hashed[i], (uint32_t)off, rl, [&](uint32_t k, uint8_t byte) {
      const uint64_t at = pos + k;
      arena[staged ? arena_bytes - 1u - at : at] = byte;
    });
  }
}

__device__ __forceinline__ uint32_t ld32(const uint8_t* p) { return *reinterpret_cast<const uint32_t*>(p); }

__global__ __launch_bounds__(256) void hsd_copy_kernel(uint8_t* __restrict__ arena, uint64_t arena_bytes,
                                                       const cut::FileRec* __restrict__ recs,
                                                       const Place* __restrict__ places, uint32_t nrec,
                                                       const uint8_t* __restrict__ src,
                                                       const uint64_t* __restrict__ src_off,
                                                       const uint32_t* __restrict__ len,
                                                       const uint64_t* __restrict__ P,
                                                       const uint32_t* __restrict__ erec, uint32_t n) {
  const uint32_t lane = lane_id();
  const uint32_t nw = gridDim.x * (blockDim.x / 64u);
  for (uint32_t v = blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; v < n; v += nw) {
    const uint32_t r = erec[v];
    if (r >= nrec) continue;
    const uint32_t L = len[v];
    if (L == 0) continue;
    const cut::FileRec& f = recs[r];
    const uint64_t so = src_off[v], d0 = places[r].base + f.fs + (P[v] - P[f.first]);
    if (!in_arena(d0, L, arena_bytes)) continue;
    const uint64_t da = d0 & ~3ull;
    const uint64_t nd = (((d0 + L + 3u) & ~3ull) - da) >> 2;
    for (uint64_t k = lane; k < nd; k += 64u) {
      const uint64_t dpos = da + 4u * k;
      const int64_t rel = (int64_t)dpos - (int64_t)d0;
      if (rel >= 0 && rel + 4 <= (int64_t)L) {
        // a whole destination dword from the two aligned source dwords around it
        const uint64_t s = so + (uint64_t)rel;
        const uint64_t sa = s & ~3ull;
        const uint32_t sh = (uint32_t)(s & 3u);
        const uint32_t w0 = ld32(src + sa);
        const uint32_t w1 = sh ? ld32(src + sa + 4u) : 0u;
        *reinterpret_cast<uint32_t*>(arena + dpos) = __builtin_amdgcn_alignbyte(w1, w0, sh);
      } else {
        for (int b = 0; b < 4; b++) {
          const int64_t q = rel + b;
          if (q >= 0 && q < (int64_t)L) arena[dpos + (uint64_t)b] = src[so + (uint64_t)q];
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void hsd_header_kernel(uint8_t* __restrict__ arena, uint64_t arena_bytes,
                                                         const cut::FileRec* __restrict__ recs,
                                                         const Place* __restrict__ places) {
  const uint32_t r = blockIdx.x;
  if (!(recs[r].flags & cut::kOpened)) return;
  const Place& pl = places[r];
  if ((pl.base & 15u) != 0 || !in_arena(pl.base, cut::kHeaderBlock, arena_bytes)) return;
  uint4* dst = reinterpret_cast<uint4*>(arena + pl.base);
  for (uint32_t q = threadIdx.x; q < cut::kHeaderBlock / 16u; q += blockDim.x) {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (q * 16u < sizeof pl.hdr)
      for (uint32_t b = 0; b < 16u; b++)
        if (q * 16u + b < sizeof pl.hdr) w[b >> 2] |= (uint32_t)pl.hdr[q * 16u + b] << (8u * (b & 3u));
    dst[q] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// crc32c of piece blockIdx.x % kCrcPieces of the rows of record blockIdx.x / kCrcPieces.
__global__ __launch_bounds__(kCloseBlock) void hsd_crc_kernel(const uint8_t* __restrict__ arena, uint64_t arena_bytes,
                                                              const cut::FileRec* __restrict__ recs,
                                                              const Place* __restrict__ places,
                                                              uint32_t* __restrict__ piece_crc) {
  constexpr uint32_t kWaves = kCloseBlock / 64;
  __shared__ uint32_t s_t[256];
  __shared__ uint32_t s_crc[kWaves];
  const uint32_t r = blockIdx.x / hsc::kCrcPieces, p = blockIdx.x % hsc::kCrcPieces;
  const cut::FileRec f = recs[r];
  if ((f.flags & (cut::kCloses | cut::kIncomplete)) != cut::kCloses) return;
  const Place& pl = places[r];
  const uint64_t rows = pl.base + f.fs_end;
  if (!in_arena(rows, pl.rows_total, arena_bytes)) return;
  crc::stage_table(s_t);
  __syncthreads();
  const uint32_t c = hsc::rows_piece_crc<kWaves>(arena + rows, pl.rows_total, p, s_t, s_crc);
  if (threadIdx.x == 0) piece_crc[(uint64_t)r * hsc::kCrcPieces + p] = c;
}

// One wave per closing file: the pieces' CRCs joined, extended over the
// footer's first 32 bytes, and the footer.
__global__ __launch_bounds__(64) void hsd_close_kernel(uint8_t* __restrict__ arena, uint64_t arena_bytes,
                                                       const cut::FileRec* __restrict__ recs,
                                                       const Place* __restrict__ places,
                                                       const uint32_t* __restrict__ piece_crc, uint32_t filetype) {
  __shared__ uint32_t s_t[256];
  const uint32_t r = blockIdx.x;
  const cut::FileRec f = recs[r];
  if ((f.flags & (cut::kCloses | cut::kIncomplete)) != cut::kCloses) return;
  const Place& pl = places[r];
  const uint64_t rows = pl.base + f.fs_end, nbytes = pl.rows_total;
  if (!in_arena(rows, nbytes, arena_bytes) || !in_arena(rows + nbytes, hs::kFooterSize, arena_bytes)) return;
  crc::stage_table(s_t);
  __syncthreads();
  if (threadIdx.x != 0) return;
  // the rows begin where the entries end
  hsc::close_file(arena + rows, nbytes, piece_crc + (uint64_t)r * hsc::kCrcPieces, filetype,
                  (f.flags & cut::kPadding) ? 1u : 0u, f.fs_end, pl.nrows_total, s_t);
}

// Compaction on the device (HSTableIndex.compacted_device): a scan window's
// decode outputs become puts of one chunk each.  part_first = 0 .. n,
// chunk_len = out_len; *flag is raised where a value did not decode (status or
// dstatus nonzero) or is too long for a chunk.
__global__ __launch_bounds__(256) void hsd_feed_kernel(const uint64_t* __restrict__ out_len,
                                                       const int32_t* __restrict__ status,
                                                       const int32_t* __restrict__ dstatus, uint32_t n,
                                                       uint32_t* __restrict__ part_first,
                                                       uint32_t* __restrict__ chunk_len, uint32_t* __restrict__ flag) {
  bool bad = false;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += gridDim.x * blockDim.x) {
    part_first[i] = i;
    if (i == n) break;
    const uint64_t len = out_len[i];
    chunk_len[i] = (uint32_t)len;
    bad |= status[i] != 0 || dstatus[i] != 0 || len > kMaxInput;
  }
  if (ballot(bad) != 0 && lane_id() == 0) atomicOr(flag, 1u);
}

uint32_t host_crc32c(const uint8_t* p, size_t n) {      // 20 bytes per file opened
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; i++) {
    c ^= p[i];
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0x82F63B78u & (0u - (c & 1u)));
  }
  return c ^ 0xFFFFFFFFu;
}
void put32(uint8_t* p, uint32_t v) { for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i)); }
void put64(uint8_t* p, uint64_t v) { for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (8 * i)); }

}  // namespace
}  // namespace kdb_lz4

using namespace kdb_lz4;

struct kdb_hstable_dev {
  uint64_t sb = 0;
  uint32_t hash_type = 1;
  uint64_t arena_bytes = 0;
  uint8_t* arena = nullptr;
  uint8_t opts[48] = {0};                 // DatabaseOptionEncoder bytes, the same in every file
  // the per-entry work area, grown to the largest batch seen
  uint8_t* work = nullptr;
  uint64_t work_bytes = 0;
  uint32_t work_n = 0;
  uint8_t* pinned = nullptr;              // where the plan's head and first records land
  Place* pinned_places = nullptr;         // and from where up to kHeadRecs places go up
  hipStream_t last = nullptr;             // the stream of the last append
  // the database so far
  cut::State st{0, 0, 0, 0, 0};
  uint64_t open_base = 0;                 // the open file's offset in the arena
  uint64_t open_rows = 0;                 // its rows so far
  uint64_t staged = 0;                    // and their bytes, staged at the arena's end
  uint64_t next_off = 0;                  // the end of the last closed file
  uint32_t fileid = 0;                    // the largest id given out
  // the open file's id and header timestamp: fileid and the timestamp of its
  // day, unless the file was carried in from another writer
  // (kdb_hstable_dev_adopt_open, kdb_live.h) and keeps its own
  uint32_t open_id = 0;
  uint64_t open_ts = 0;
  // kdb_hstable_dev_create2 (kdb_compact.h): the type of the files written and,
  // where nonzero, the timestamp every header carries instead of the file's id
  // (LockSequenceTimestamp).  kdb_hstable_dev_adopt returns both to 1 and 0.
  uint32_t filetype = 1;                  // kUncompactedRegularType
  uint64_t ts_lock = 0;
  std::vector<uint64_t> file_off, file_size;
  std::vector<uint32_t> file_id;
};

namespace {

// The work area's arrays for a batch of up to n entries and cap records.
struct Work {
  uint32_t *eff, *valid, *marked, *unfinished, *rowlen, *erec;
  uint64_t *P, *CV, *CM, *C2, *R;
  PlanHead* head;
  cut::FileRec* recs;
  Place* places;
  uint32_t* piece_crc;                    // kCrcPieces per record
  uint64_t bytes;
};

uint32_t record_cap(const kdb_hstable_dev* w, uint32_t n) {
  // a file opened needs its header block in the arena
  return (uint32_t)std::min<uint64_t>(n, w->arena_bytes / cut::kHeaderBlock) + 2u;
}

Work carve(uint8_t* base, uint32_t n, uint32_t cap) {
  Work k{};
  uint64_t at = 0;
  auto take = [&](uint64_t bytes) {
    uint8_t* p = base ? base + at : nullptr;
    at += align256(bytes);
    return p;
  };
  uint32_t** u32s[] = {&k.eff, &k.valid, &k.marked, &k.unfinished, &k.rowlen, &k.erec};
  for (uint32_t** p : u32s) *p = reinterpret_cast<uint32_t*>(take((uint64_t)n * 4u));
  uint64_t** u64s[] = {&k.P, &k.CV, &k.CM, &k.C2, &k.R};
  for (uint64_t** p : u64s) *p = reinterpret_cast<uint64_t*>(take(((uint64_t)n + 1u) * 8u));
  // head and records lie together: one copy brings both down
  k.head = reinterpret_cast<PlanHead*>(take(sizeof(PlanHead) + (uint64_t)cap * sizeof(cut::FileRec)));
  k.recs = reinterpret_cast<cut::FileRec*>(base ? reinterpret_cast<uint8_t*>(k.head) + sizeof(PlanHead) : nullptr);
  k.places = reinterpret_cast<Place*>(take((uint64_t)cap * sizeof(Place)));
  k.piece_crc = reinterpret_cast<uint32_t*>(take((uint64_t)cap * hsc::kCrcPieces * 4u));
  k.bytes = at;
  return k;
}

hipError_t ensure_work(kdb_hstable_dev* w, uint32_t n) {
  if (w->work && n <= w->work_n) return hipSuccess;
  const uint64_t bytes = carve(nullptr, n, record_cap(w, n)).bytes;
  if (w->work) {
    KDB_TRY(hipStreamSynchronize(w->last));
    KDB_TRY(hipFree(w->work));
    w->work = nullptr;
    w->work_n = 0;
  }
  KDB_TRY(hipMalloc(reinterpret_cast<void**>(&w->work), bytes));
  w->work_bytes = bytes;
  w->work_n = n;
  return hipSuccess;
}

void file_header(const kdb_hstable_dev* w, uint64_t timestamp, uint8_t* b) {
  memset(b, 0, 72);
  put32(b + 4, 1);                        // data format 1.0 (format.h:28-29)
  put32(b + 8, 0);
  put32(b + 12, w->filetype);
  put64(b + 16, timestamp);
  put32(b, host_crc32c(b + 4, 20));
  memcpy(b + 24, w->opts, 48);
}

// What the database becomes with the records applied; nothing of *w changes
// before commit().
struct Placement {
  std::vector<Place> places;
  cut::State st;
  uint64_t open_base, open_rows, staged, next_off;
  uint32_t fileid, open_id;
  uint64_t open_ts;
  std::vector<uint64_t> file_off, file_size;
  std::vector<uint32_t> file_id;
  uint64_t unstage_dst = 0, unstage_bytes = 0;
};

bool place_records(const kdb_hstable_dev* w, const cut::FileRec* recs, uint32_t nrec, Placement* out) {
  Placement& p = *out;
  p.st = w->st;
  p.open_base = w->open_base;
  p.open_rows = w->open_rows;
  p.staged = w->staged;
  p.next_off = w->next_off;
  p.fileid = w->fileid;
  p.open_id = w->open_id;
  p.open_ts = w->open_ts;
  uint64_t max_extent = 0, max_staged = w->staged;
  const uint64_t lim = w->arena_bytes;
  for (uint32_t r = 0; r < nrec; r++) {
    const cut::FileRec& f = recs[r];
    Place pl{};
    if (f.flags & cut::kOpened) {
      if (p.st.open || f.fs != cut::kHeaderBlock) return false;
      p.open_base = align64(p.next_off);
      p.open_rows = 0;
      p.staged = 0;
      p.fileid++;
      p.open_id = p.fileid;
      p.open_ts = w->ts_lock ? w->ts_lock : p.fileid;                 // timestamps count with the ids, unless locked
      file_header(w, p.open_ts, pl.hdr);
    } else if (r != 0 || !p.st.open || f.fs != p.st.fsize) {
      return false;                         // only the first record continues a file
    }
    if (f.fs_end < f.fs || f.fs_end > (1ull << 40) || f.row_bytes > 15ull * f.nvalid || p.open_base > lim)
      return false;
    const bool incomplete = (f.flags & cut::kIncomplete) != 0;
    const uint64_t rb = incomplete ? 0 : f.row_bytes;
    if (incomplete) p.staged = 0;
    pl.base = p.open_base;
    uint64_t extent;
    if (f.flags & cut::kCloses) {
      uint64_t size = f.fs_end;
      if (!incomplete) {
        pl.rows_mode = kRowsFinal;
        pl.staged = p.staged;
        pl.rows_at = p.open_base + f.fs_end + p.staged;
        pl.rows_total = p.staged + rb;
        pl.nrows_total = p.open_rows + f.nvalid;
        size += pl.rows_total + hs::kFooterSize;
        if (p.staged) {
          p.unstage_dst = p.open_base + f.fs_end;
          p.unstage_bytes = p.staged;
        }
      }
      extent = p.open_base + size;
      p.file_off.push_back(p.open_base);
      p.file_size.push_back(size);
      p.file_id.push_back(p.open_id);
      p.next_off = extent;
      p.st = cut::State{0, 0, 0, 0, 0};
      p.staged = 0;
      p.open_rows = 0;
    } else {
      pl.rows_mode = incomplete ? kRowsNone : kRowsStaged;
      pl.rows_at = p.staged;
      extent = p.open_base + f.fs_end;
      p.staged += rb;
      p.open_rows += f.nvalid;
      p.st.open = 1;
      p.st.fsize = f.fs_end;
      p.st.padding = (f.flags & cut::kPadding) != 0;
      p.st.incomplete = incomplete;
    }
    max_extent = std::max(max_extent, extent);
    max_staged = std::max(max_staged, p.staged);
    p.places.push_back(pl);
  }
  // the files from the arena's start and the staging from its end never meet
  return max_extent <= lim && max_staged <= lim - max_extent;
}

void commit(kdb_hstable_dev* w, const Placement& p) {
  w->st = p.st;
  w->open_base = p.open_base;
  w->open_rows = p.open_rows;
  w->staged = p.staged;
  w->next_off = p.next_off;
  w->fileid = p.fileid;
  w->open_id = p.open_id;
  w->open_ts = p.open_ts;
  w->file_off.insert(w->file_off.end(), p.file_off.begin(), p.file_off.end());
  w->file_size.insert(w->file_size.end(), p.file_size.begin(), p.file_size.end());
  w->file_id.insert(w->file_id.end(), p.file_id.begin(), p.file_id.end());
}

// The kernels that write the arena, for records already placed (uploaded to k.recs / k.places).
hipError_t write_files(kdb_hstable_dev* w, hipStream_t st, const Work& k, const Placement& p, uint32_t nrec,
                       const uint8_t* d_entries, const uint64_t* d_entry_off, const uint32_t* d_entry_len,
                       const uint64_t* d_hashed, uint32_t n) {
  if (p.unstage_bytes) {
    hipLaunchKernelGGL(hsd_unstage_kernel, dim3(grid_for(p.unstage_bytes, 256, 4096)), dim3(256), 0, st, w->arena,
                       w->arena_bytes, p.unstage_dst, p.unstage_bytes);
    KDB_TRY(hipGetLastError());
  }
  if (n) {
    hipLaunchKernelGGL(hsd_rows_kernel, dim3(grid_for(n, 256, 4096)), dim3(256), 0, st, w->arena, w->arena_bytes,
                       k.recs, k.places, nrec, d_hashed, k.P, k.R, k.rowlen, k.erec, n);
    KDB_TRY(hipGetLastError());
    hipLaunchKernelGGL(hsd_copy_kernel, dim3(grid_for(n, 4, 16384)), dim3(256), 0, st, w->arena, w->arena_bytes,
                       k.recs, k.places, nrec, d_entries, d_entry_off, d_entry_len, k.P, k.erec, n);
    KDB_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(hsd_header_kernel, dim3(nrec), dim3(256), 0, st, w->arena, w->arena_bytes, k.recs, k.places);
  KDB_TRY(hipGetLastError());
  if (!p.file_id.empty()) {                  // some file closes
    hipLaunchKernelGGL(hsd_crc_kernel, dim3(hsc::kCrcPieces * nrec), dim3(kCloseBlock), 0, st, w->arena, w->arena_bytes,
                       k.recs, k.places, k.piece_crc);
    KDB_TRY(hipGetLastError());
    hipLaunchKernelGGL(hsd_close_kernel, dim3(nrec), dim3(64), 0, st, w->arena, w->arena_bytes, k.recs, k.places,
                       k.piece_crc, w->filetype);
  }
  return hipGetLastError();
}

// The places go up from the pinned buffer without a wait: it is next written
// after the next append's own synchronisation of the stream (close_open
// synchronises before it writes).  More than kHeadRecs of them (rare) go from
// pageable memory and are waited for.
hipError_t upload_places(kdb_hstable_dev* w, hipStream_t st, const Work& k, const Placement& p) {
  const size_t bytes = p.places.size() * sizeof(Place);
  if (p.places.size() <= kHeadRecs) {
    memcpy(w->pinned_places, p.places.data(), bytes);
    return hipMemcpyAsync(k.places, w->pinned_places, bytes, hipMemcpyHostToDevice, st);
  }
  KDB_TRY(hipMemcpyAsync(k.places, p.places.data(), bytes, hipMemcpyHostToDevice, st));
  return hipStreamSynchronize(st);
}

hipError_t append(kdb_hstable_dev* w, hipStream_t st, const uint8_t* d_entries, const uint64_t* d_entry_off,
                  const uint32_t* d_entry_len, const uint64_t* d_hashed, const uint32_t* d_kind,
                  const int32_t* d_status, uint32_t n, bool* refused) {
  KDB_TRY(ensure_work(w, n));
  if (w->last != st) KDB_TRY(hipStreamSynchronize(w->last));     // the arena and the work area are one stream's at a time
  w->last = st;
  const uint32_t cap = record_cap(w, n);
  const Work k = carve(w->work, w->work_n, record_cap(w, w->work_n));
  const uint32_t g = grid_for(n, 256, 4096);
  hipLaunchKernelGGL(hsd_prepare_kernel, dim3(g), dim3(256), 0, st, d_entry_len, d_kind, d_status, n, k.eff, k.valid,
                     k.marked, k.unfinished);
  KDB_TRY(hipGetLastError());
  KDB_TRY(launch_exclusive_scan(st, k.eff, n, k.P, k.P + n));
  KDB_TRY(launch_exclusive_scan(st, k.valid, n, k.CV, k.CV + n));
  KDB_TRY(launch_exclusive_scan(st, k.marked, n, k.CM, k.CM + n));
  KDB_TRY(launch_exclusive_scan(st, k.unfinished, n, k.C2, k.C2 + n));
  hipLaunchKernelGGL(hsd_plan_kernel, dim3(1), dim3(64), 0, st, cut::Prefix{k.P, k.CV, k.CM, k.C2, n}, w->sb, w->st,
                     k.head, k.recs, cap);
  KDB_TRY(hipGetLastError());
  hipLaunchKernelGGL(hsd_rowlen_kernel, dim3(g), dim3(256), 0, st, k.head, k.recs, d_status, d_hashed, k.P, n, cap,
                     k.rowlen, k.erec);
  KDB_TRY(hipGetLastError());
  KDB_TRY(launch_exclusive_scan(st, k.rowlen, n, k.R, k.R + n));
  hipLaunchKernelGGL(hsd_rowsum_kernel, dim3(grid_for(cap, 64, 64)), dim3(64), 0, st, k.head, k.recs, k.R, n, cap);
  KDB_TRY(hipGetLastError());
  // the plan: the head and the first records in one copy, the rest (rare) in a second
  const uint32_t first = std::min(cap, kHeadRecs);
  KDB_TRY(hipMemcpyAsync(w->pinned, k.head, sizeof(PlanHead) + first * sizeof(cut::FileRec), hipMemcpyDeviceToHost,
                         st));
  KDB_TRY(hipStreamSynchronize(st));
  PlanHead head;
  memcpy(&head, w->pinned, sizeof head);
  if (head.refused || head.nrec > cap) {
    *refused = true;
    return hipSuccess;
  }
  std::vector<cut::FileRec> recs(head.nrec);
  memcpy(recs.data(), w->pinned + sizeof(PlanHead), std::min(head.nrec, first) * sizeof(cut::FileRec));
  if (head.nrec > first)
    KDB_TRY(hipMemcpy(recs.data() + first, k.recs + first, (head.nrec - first) * sizeof(cut::FileRec),
                      hipMemcpyDeviceToHost));
  if (head.nrec == 0) return hipSuccess;                         // nothing but failed puts
  Placement p;
  if (!place_records(w, recs.data(), head.nrec, &p)) {
    *refused = true;
    return hipSuccess;
  }
  KDB_TRY(upload_places(w, st, k, p));
  commit(w, p);
  return write_files(w, st, k, p, head.nrec, d_entries, d_entry_off, d_entry_len, d_hashed, n);
}

// Database::Close: the open file closes as it is, one record made here.
hipError_t close_open(kdb_hstable_dev* w, bool* refused) {
  if (!w->st.open) return hipSuccess;
  KDB_TRY(ensure_work(w, 1));
  hipStream_t st = w->last;
  const Work k = carve(w->work, w->work_n, record_cap(w, w->work_n));
  uint32_t flags = cut::kCloses;
  if (w->st.padding) flags |= cut::kPadding;
  if (w->st.incomplete) flags |= cut::kIncomplete;
  const cut::FileRec rec{0, 0, w->st.fsize, w->st.fsize, 0, flags, 0};
  Placement p;
  if (!place_records(w, &rec, 1, &p)) {
    *refused = true;
    return hipSuccess;
  }
  KDB_TRY(hipStreamSynchronize(st));       // the pinned buffers are free
  memcpy(w->pinned, &rec, sizeof rec);
  KDB_TRY(hipMemcpyAsync(k.recs, w->pinned, sizeof rec, hipMemcpyHostToDevice, st));
  KDB_TRY(upload_places(w, st, k, p));
  commit(w, p);
  return write_files(w, st, k, p, 1, nullptr, nullptr, nullptr, nullptr, 0);
}

}  // namespace

// ------------------------------------------------------------------ C ABI
extern "C" uint64_t kdb_hstable_dev_arena_bytes(uint64_t hstable_size, uint64_t entry_bytes, uint64_t n_entries) {
  if (hstable_size <= cut::kHeaderBlock) return ~0ull;
  if (n_entries > (1ull << 56) || entry_bytes > (1ull << 60)) return ~0ull;
  const uint64_t files = entry_bytes / (hstable_size - cut::kHeaderBlock) + 2u;
  if (files > (1ull << 48)) return ~0ull;
  return align64(entry_bytes + 30u * n_entries + files * (cut::kHeaderBlock + hs::kFooterSize + 64u));
}

extern "C" int kdb_hstable_dev_create(uint64_t hstable_size, uint32_t hash_type, uint64_t arena_bytes,
                                      kdb_hstable_dev** w) {
  return kdb_hstable_dev_create2(hstable_size, hash_type, arena_bytes, 1u, 0u, w);
}

extern "C" int kdb_hstable_dev_create2(uint64_t hstable_size, uint32_t hash_type, uint64_t arena_bytes,
                                       uint32_t filetype, uint64_t timestamp_lock, kdb_hstable_dev** w) {
  if (!w || hash_type > 1 || (filetype != 1u && filetype != 2u) || hstable_size <= cut::kHeaderBlock || arena_bytes < cut::kHeaderBlock + 64u ||
      arena_bytes > (1ull << 46))
    return KDB_PUT_EINVAL;
  int count = 0;
  const hipError_t e0 = hipGetDeviceCount(&count);
  if (e0 != hipSuccess) return hip_code(e0);
  if (count < 1) return KDB_PUT_ENODEV;
  kdb_hstable_dev* p = new (std::nothrow) kdb_hstable_dev;
  if (!p) return KDB_PUT_EINVAL;
  p->sb = hstable_size;
  p->hash_type = hash_type;
  p->arena_bytes = arena_bytes;
  p->filetype = filetype;
  p->ts_lock = timestamp_lock;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&p->arena), arena_bytes);
  if (e == hipSuccess)
    e = hipHostMalloc(reinterpret_cast<void**>(&p->pinned), sizeof(PlanHead) + kHeadRecs * sizeof(cut::FileRec),
                      hipHostMallocDefault);
  if (e == hipSuccess)
    e = hipHostMalloc(reinterpret_cast<void**>(&p->pinned_places), kHeadRecs * sizeof(Place), hipHostMallocDefault);
  if (e != hipSuccess || kdb_hstable_db_options(hstable_size, hash_type, p->opts) != KDB_PUT_OK) {
    kdb_hstable_dev_destroy(p);
    return e != hipSuccess ? hip_code(e) : KDB_PUT_EINVAL;
  }
  *w = p;
  return KDB_PUT_OK;
}

extern "C" int kdb_hstable_dev_destroy(kdb_hstable_dev* w) {
  if (!w) return KDB_PUT_OK;
  if (w->arena || w->work) (void)hipStreamSynchronize(w->last);
  if (w->arena) (void)hipFree(w->arena);
  if (w->work) (void)hipFree(w->work);
  if (w->pinned) (void)hipHostFree(w->pinned);
  if (w->pinned_places) (void)hipHostFree(w->pinned_places);
  delete w;
  return KDB_PUT_OK;
}

extern "C" int kdb_hstable_dev_append(kdb_hstable_dev* w, void* stream, const uint8_t* d_entries,
                                      const uint64_t* d_entry_off, const uint32_t* d_entry_len,
                                      const uint64_t* d_hashed, const uint32_t* d_kind, const int32_t* d_status,
                                      uint32_t n) {
  if (!w || (n && (!d_entries || !d_entry_off || !d_entry_len || !d_hashed || !d_kind || !d_status)))
    return KDB_PUT_EINVAL;
  if (n == 0) return KDB_PUT_OK;           // no entry: nothing opens, and an open file is below hstable_size
  bool refused = false;
  const hipError_t e = append(w, (hipStream_t)stream, d_entries, d_entry_off, d_entry_len, d_hashed, d_kind, d_status,
                              n, &refused);
  if (e != hipSuccess) return hip_code(e);
  return refused ? KDB_PUT_EINVAL : KDB_PUT_OK;
}

extern "C" int kdb_hstable_dev_close(kdb_hstable_dev* w) {
  if (!w) return KDB_PUT_EINVAL;
  bool refused = false;
  const hipError_t e = close_open(w, &refused);
  if (e != hipSuccess) return hip_code(e);
  return refused ? KDB_PUT_EINVAL : KDB_PUT_OK;
}

extern "C" int kdb_hstable_dev_file_count(const kdb_hstable_dev* w, uint32_t* count) {
  if (!w || !count) return KDB_PUT_EINVAL;
  *count = (uint32_t)w->file_id.size();
  return KDB_PUT_OK;
}

extern "C" int kdb_hstable_dev_files(const kdb_hstable_dev* w, const uint8_t** d_base, uint64_t* file_off,
                                     uint64_t* file_size, uint32_t* fileid, uint32_t cap) {
  if (!w) return KDB_PUT_EINVAL;
  const hipError_t e = hipStreamSynchronize(w->last);
  if (e != hipSuccess) return hip_code(e);
  if (d_base) *d_base = w->arena;
  const uint32_t m = std::min<uint32_t>(cap, (uint32_t)w->file_id.size());
  for (uint32_t f = 0; f < m; f++) {
    if (file_off) file_off[f] = w->file_off[f];
    if (file_size) file_size[f] = w->file_size[f];
    if (fileid) fileid[f] = w->file_id[f];
  }
  return KDB_PUT_OK;
}

// kdb_index_tail.h: the open file as kdb_index_set_tail reads it
extern "C" int kdb_hstable_dev_open_file(const kdb_hstable_dev* w, kdb_open_file* out) {
  if (!w || !out) return KDB_PUT_EINVAL;
  const hipError_t e = hipStreamSynchronize(w->last);
  if (e != hipSuccess) return hip_code(e);
  *out = kdb_open_file{};
  if (!w->st.open) return KDB_PUT_OK;
  out->open = 1u;
  out->fileid = w->open_id;
  out->incomplete = w->st.incomplete ? 1u : 0u;
  out->timestamp = w->open_ts;
  out->file_off = w->open_base;
  out->bytes = w->st.fsize;
  out->rows = w->open_rows;
  out->row_bytes = w->staged;
  out->rows_last = w->arena_bytes - 1u;
  return KDB_PUT_OK;
}

extern "C" int kdb_hstable_dev_download(const kdb_hstable_dev* w, uint32_t i, uint8_t* host_dst, void* stream) {
  if (!w || i >= w->file_id.size() || !host_dst) return KDB_PUT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = st != w->last ? hipStreamSynchronize(w->last) : hipSuccess;
  if (e == hipSuccess)
    e = hipMemcpyAsync(host_dst, w->arena + w->file_off[i], w->file_size[i], hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return hip_code(e);
}

extern "C" int kdb_hstable_dev_reset(kdb_hstable_dev* w) {
  if (!w) return KDB_PUT_EINVAL;
  const hipError_t e = hipStreamSynchronize(w->last);
  if (e != hipSuccess) return hip_code(e);
  w->st = cut::State{0, 0, 0, 0, 0};
  w->open_base = w->open_rows = w->staged = w->next_off = 0;
  w->fileid = 0;
  w->open_id = 0;
  w->open_ts = 0;
  w->file_off.clear();
  w->file_size.clear();
  w->file_id.clear();
  return KDB_PUT_OK;
}

extern "C" int kdb_hstable_dev_open_bytes(const kdb_hstable_dev* w, uint64_t* bytes) {
  if (!w || !bytes) return KDB_PUT_EINVAL;
  *bytes = w->st.open ? w->st.fsize : 0u;
  return KDB_PUT_OK;
}

// Compaction() steps 8, 9 and 14 (storage_engine.h:940-1010): the compacted
// files take ids above every id in use, and the files the compaction did not
// cover stay in the database beside them -- here, in this writer's arena.
extern "C" int kdb_hstable_dev_adopt(kdb_hstable_dev* w, void* stream, uint32_t first_fileid, const uint8_t* d_src,
                                     const uint64_t* src_off, const uint64_t* src_size, const uint32_t* src_id,
                                     uint32_t nsrc) {
  if (!w || first_fileid == 0 || (nsrc && (!d_src || !src_off || !src_size || !src_id))) return KDB_PUT_EINVAL;
  if (w->st.open) return KDB_PUT_EINVAL;
  const uint64_t own = w->file_id.size();
  if ((uint64_t)first_fileid + own + 1u > 0xFFFFFFFFull) return KDB_PUT_EINVAL;
  std::vector<uint32_t> ids(src_id, src_id + nsrc);
  std::sort(ids.begin(), ids.end());
  for (uint32_t f = 0; f < nsrc; f++)
    if (ids[f] == 0 || ids[f] >= first_fileid || (f && ids[f] == ids[f - 1u])) return KDB_PUT_EINVAL;
  // where the adopted files go: nothing is staged while no file is open, so
  // the room ends with the arena
  std::vector<uint64_t> at(nsrc);
  uint64_t pos = w->next_off;
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(w->arena), a1 = a0 + w->arena_bytes;
  for (uint32_t f = 0; f < nsrc; f++) {
    if (src_size[f] > hs::kMaxFileSize || src_off[f] > (1ull << 46)) return KDB_PUT_EINVAL;
    pos = align64(pos);
    if (pos > w->arena_bytes || src_size[f] > w->arena_bytes - pos) return KDB_PUT_EINVAL;
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_src) + src_off[f], s1 = s0 + src_size[f];
    if (s0 < a1 && a0 < s1) return KDB_PUT_EINVAL;
    at[f] = pos;
    pos += src_size[f];
  }
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = st != w->last ? hipStreamSynchronize(w->last) : hipSuccess;
  for (uint32_t f = 0; f < nsrc && e == hipSuccess; f++)
    if (src_size[f])
      e = hipMemcpyAsync(w->arena + at[f], d_src + src_off[f], src_size[f], hipMemcpyDeviceToDevice, st);
  if (e != hipSuccess) return hip_code(e);   // bytes behind next_off are nobody's: the writer is as before
  w->last = st;
  for (uint64_t i = 0; i < own; i++) w->file_id[i] = first_fileid + (uint32_t)i;
  for (uint32_t f = 0; f < nsrc; f++) {
    w->file_off.push_back(at[f]);
    w->file_size.push_back(src_size[f]);
    w->file_id.push_back(src_id[f]);
  }
  w->next_off = pos;
  w->fileid = first_fileid + (uint32_t)own - 1u;      // above the adopted ids too: they are below first_fileid
  w->filetype = 1u;
  w->ts_lock = 0u;
  return KDB_PUT_OK;
}

// kdb_live.h: the hand-over's last step, the open file itself
extern "C" int kdb_hstable_dev_adopt_open(kdb_hstable_dev* dst, void* stream, const kdb_hstable_dev* src) {
  if (!dst || !src || dst == src) return KDB_PUT_EINVAL;
  if (!src->st.open) return KDB_PUT_OK;
  if (dst->st.open || dst->sb != src->sb || dst->hash_type != src->hash_type) return KDB_PUT_EINVAL;
  if (dst->filetype != 1u || dst->ts_lock || src->filetype != 1u || src->ts_lock) return KDB_PUT_EINVAL;
  const uint32_t id = src->open_id;
  if (id == 0) return KDB_PUT_EINVAL;
  for (uint32_t held : dst->file_id)
    if (held == id) return KDB_PUT_EINVAL;
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(dst->arena), a1 = a0 + dst->arena_bytes;
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(src->arena), s1 = s0 + src->arena_bytes;
  if (s0 < a1 && a0 < s1) return KDB_PUT_EINVAL;
  // what place_records() asks of an open file: the files from the arena's
  // start and the staging from its end never meet
  const uint64_t fsize = src->st.fsize, staged = src->st.incomplete ? 0u : src->staged;
  const uint64_t base = align64(dst->next_off);
  if (src->open_base > src->arena_bytes || fsize > src->arena_bytes - src->open_base || staged > src->arena_bytes)
    return KDB_PUT_EINVAL;
  if (base > dst->arena_bytes || fsize > dst->arena_bytes - base || staged > dst->arena_bytes - base - fsize)
    return KDB_PUT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = st != src->last ? hipStreamSynchronize(src->last) : hipSuccess;
  if (e == hipSuccess && st != dst->last && dst->last != src->last) e = hipStreamSynchronize(dst->last);
  if (e == hipSuccess && fsize)
    e = hipMemcpyAsync(dst->arena + base, src->arena + src->open_base, fsize, hipMemcpyDeviceToDevice, st);
  // staged byte b lies at arena[arena_bytes - 1 - b] in both: the block as it is
  if (e == hipSuccess && staged)
    e = hipMemcpyAsync(dst->arena + (dst->arena_bytes - staged), src->arena + (src->arena_bytes - staged), staged,
                       hipMemcpyDeviceToDevice, st);
  if (e != hipSuccess) return hip_code(e);   // bytes behind next_off are nobody's: the writer is as before
  dst->last = st;
  dst->st = src->st;
  dst->open_base = base;
  dst->open_rows = src->open_rows;
  dst->staged = staged;
  dst->open_id = id;
  dst->open_ts = src->open_ts;
  dst->fileid = std::max(dst->fileid, id);   // files opened later: one above every id held
  return KDB_PUT_OK;
}

extern "C" int kdb_hstable_dev_feed(void* stream, const uint64_t* d_out_len, const int32_t* d_status,
                                    const int32_t* d_dstatus, uint32_t n, uint32_t* d_part_first,
                                    uint32_t* d_chunk_len, uint32_t* d_flag) {
  if (!d_part_first || !d_flag || (n && (!d_out_len || !d_status || !d_dstatus || !d_chunk_len))) return KDB_PUT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(d_flag, 0, 4, st);
  if (e != hipSuccess) return hip_code(e);
  hipLaunchKernelGGL(hsd_feed_kernel, dim3(grid_for((uint64_t)n + 1u, 256, 4096)), dim3(256), 0, st, d_out_len,
                     d_status, d_dstatus, n, d_part_first, d_chunk_len, d_flag);
  return hip_code(hipGetLastError());
}
