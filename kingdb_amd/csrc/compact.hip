// kingdb_amd/csrc/compact.hip -- compaction by copy (include/kdb_compact.h):
// the live entries of a scan window moved from the files where they lie into
// the dense entry stream kdb_hstable_dev_append takes, without decoding a
// value.  What StorageEngine::Compaction does in its step 6
// (storage/storage_engine.h:796-920): one self-contained Order per kept entry
// out of the stored bytes -- size_value_used() bytes, size_value,
// size_value_compressed and checksum_content carried over -- which
// WriteFirstPartOrSmallOrder (storage/hstable_manager.h:637-673) writes with a
// fresh header: flags kEntryFull, no padding.
//
//   compact_plan_kernel   thread per entry: the refusals, the key hash, the
//                         header (entry_encode.h, the encoder of put.hip) into
//                         a 64-byte record, entry_len
//   scan                  launch_exclusive_scan (pack.hip): entry_off, total
//   compact_copy_kernel   workgroup per kPiece bytes of the dense output
//                         stream, thread per aligned 16-byte word of it.  The
//                         word's entry is found by a binary search in
//                         entry_off, narrowed to the entries the piece touches.
//                         A word that lies inside one value is two aligned
//                         16-byte loads of the source, realigned by alignbyte,
//                         and one 16-byte store; a word that touches a header,
//                         a key or two entries is put together byte by byte.
// The work is divided by output bytes, so a window of 30-byte entries around
// one of several MiB is as balanced as one of equal entries.
//
// Why an aligned load that reaches past the value's ends is safe.  A value
// the scan emitted lies inside a file that loaded with status 0: in front of
// it are its own header and key (at least 26 bytes), behind it the file's
// offset array and the 36-byte footer.  The two aligned 16-byte words around
// any 16 value bytes reach at most 15 bytes beyond them on either side, so
// they stay inside the value's own file whatever buffer holds it: the device
// writer's arena, where files start on 64-byte boundaries and the arena is
// one allocation, or an uploaded buffer, where the slots are 64-byte aligned
// and 64 spare bytes follow the last.  The kernel does not rely on that: a
// word whose loads would end past files_bytes takes the byte path.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/kdb_put.h"
#include "entry_encode.h"
#include "hash_device.h"
#include "hip_host.h"
#include "lz4_device.h"

namespace kdb_lz4 {
namespace {

constexpr uint32_t kEntryFull = 0x8;          // format.h:34-42; a put has no type bit
constexpr uint32_t kPiece = 16384;            // output bytes per workgroup
constexpr uint32_t kCopyBlock = 256;
constexpr uint32_t kHdrBytes = 56;            // >= 1 + 4 + 1 + 5 + 10 + 8 + 1 + 8
static_assert(kPiece % (16u * kCopyBlock) == 0, "a piece is whole rounds of the block's 16-byte words");

struct HdrRec {
  uint8_t hdr[kHdrBytes];
  uint32_t hl, klen;
};
static_assert(sizeof(HdrRec) == 64, "one record per entry, 64 bytes");

__global__ __launch_bounds__(256) void compact_plan_kernel(
    const uint8_t* __restrict__ keys, uint64_t keys_bytes, const uint64_t* __restrict__ key_off,
    const uint32_t* __restrict__ key_len, const uint64_t* __restrict__ stored_off, const uint64_t* __restrict__ avail,
    const uint64_t* __restrict__ svc, const uint64_t* __restrict__ size, const uint32_t* __restrict__ checksum,
    const int32_t* __restrict__ status_in, uint32_t n, uint64_t files_bytes, uint32_t hash_type,
    HdrRec* __restrict__ rec, uint32_t* __restrict__ entry_len, uint64_t* __restrict__ hashed,
    uint32_t* __restrict__ kind, int32_t* __restrict__ status, uint32_t* __restrict__ refused) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
    const uint32_t klen = key_len[v];
    const uint64_t ko = key_off[v], so = stored_off[v], c = svc[v], V = size[v];
    const uint64_t used = c ? c : V;                                  // size_value_used(), format.h
    const uint32_t hl = header_len(kEntryFull, klen, V, 0);
    const bool ok = status_in[v] == 0 && klen != 0 && ko <= keys_bytes && klen <= keys_bytes - ko &&
                    used <= avail[v] && so <= files_bytes && used <= files_bytes - so &&
                    used <= 0xFFFFFFFFull && (uint64_t)hl + klen + used <= 0xFFFFFFFFull;
    uint64_t h = 0;
    if (ok) {
      const uint8_t* key = keys + ko;
      h = hash_type == 1 ? xxh64(key, klen) : murmur3_64(key, klen);
      encode_entry_header(rec[v].hdr, hl, checksum[v], kEntryFull, klen, V, c, 0, h, kCrc8.t);
      rec[v].hl = hl;
      rec[v].klen = klen;
    } else {
      rec[v].hl = 0;
      rec[v].klen = 0;
      atomicAdd(refused, 1u);
    }
    entry_len[v] = ok ? hl + klen + (uint32_t)used : 0u;
    hashed[v] = h;
    kind[v] = KDB_PUT_SELF_CONTAINED;
    status[v] = ok ? 0 : -1;
  }
}

// The last entry of [a, b) that starts at or before o (off[a] <= o).  Entries
// of length 0 share their offset with the entry behind them, so the entry
// found is the one that holds byte o.
__device__ __forceinline__ uint32_t find_entry(const uint64_t* __restrict__ off, uint32_t a, uint32_t b, uint64_t o) {
  uint32_t l = a, r = b;
  while (r - l > 1u) {
    const uint32_t m = l + (r - l) / 2u;
    if (off[m] <= o) l = m;
    else r = m;
  }
  return l;
}

__global__ __launch_bounds__(kCopyBlock) void compact_copy_kernel(
    const uint8_t* __restrict__ files, uint64_t files_bytes, const uint8_t* __restrict__ keys,
    const uint64_t* __restrict__ key_off, const uint64_t* __restrict__ stored_off, const HdrRec* __restrict__ rec,
    const uint64_t* __restrict__ entry_off, const uint32_t* __restrict__ entry_len, uint32_t n,
    const uint64_t* __restrict__ total_ptr, uint8_t* __restrict__ entries, uint64_t entries_cap) {
  const uint64_t total = *total_ptr;
  if (total > entries_cap) return;            // the host refused it already
  const uint64_t npieces = (total + kPiece - 1u) / kPiece;
  for (uint64_t piece = blockIdx.x; piece < npieces; piece += gridDim.x) {
    const uint64_t lo = piece * kPiece, hi = min(lo + kPiece, total);
    // the entries the piece touches (the same for every thread)
    const uint32_t e_lo = find_entry(entry_off, 0u, n, lo);
    const uint32_t e_hi = find_entry(entry_off, e_lo, n, hi - 1u);
    for (uint64_t o = lo + 16u * threadIdx.x; o < hi; o += 16u * kCopyBlock) {
      uint32_t e = find_entry(entry_off, e_lo, e_hi + 1u, o);
      uint64_t eo = entry_off[e];
      uint32_t el = entry_len[e], hl = rec[e].hl, klen = rec[e].klen;
      const uint64_t rel = o - eo;
      const uint64_t vstart = (uint64_t)hl + klen;
      uint4* dst = reinterpret_cast<uint4*>(entries + o);
      if (rel >= vstart && rel + 16u <= el) {
        // 16 bytes of one value: the two aligned source words around them
        const uint64_t s = stored_off[e] + (rel - vstart);
        const uint64_t sa = s & ~15ull;
        const uint32_t sh = (uint32_t)(s & 15u);
        if (sa + (sh ? 32u : 16u) <= files_bytes) {
          const uint4 A = *reinterpret_cast<const uint4*>(files + sa);
          if (sh == 0) {
            *dst = A;
            continue;
          }
          const uint4 B = *reinterpret_cast<const uint4*>(files + sa + 16u);
          const uint32_t w[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
          const uint32_t d = sh >> 2, b = sh & 3u;
          uint32_t r[5];
#pragma unroll
          for (uint32_t i = 0; i < 5u; i++) r[i] = d == 0 ? w[i] : d == 1 ? w[i + 1] : d == 2 ? w[i + 2] : w[i + 3];
          *dst = make_uint4(__builtin_amdgcn_alignbyte(r[1], r[0], b), __builtin_amdgcn_alignbyte(r[2], r[1], b),
                            __builtin_amdgcn_alignbyte(r[3], r[2], b), __builtin_amdgcn_alignbyte(r[4], r[3], b));
          continue;
        }
      }
      // a header, a key, the end of a value, or more than one entry: byte by byte
      const uint8_t* kp = keys + key_off[e];
      const uint8_t* vp = files + stored_off[e];
      uint32_t out[4] = {0u, 0u, 0u, 0u};
      uint32_t nb = 0;
      for (; nb < 16u && o + nb < hi; nb++) {
        const uint64_t q = o + nb;
        while (q >= eo + el && e + 1u < n) {  // the next entry that has bytes
          e++;
          eo = entry_off[e];
          el = entry_len[e];
          hl = rec[e].hl;
          klen = rec[e].klen;
          kp = keys + key_off[e];
          vp = files + stored_off[e];
        }
        if (q >= eo + el) break;
        const uint64_t x = q - eo;
        const uint32_t byte = x < hl ? rec[e].hdr[x] : x < (uint64_t)hl + klen ? kp[x - hl] : vp[x - hl - klen];
        out[nb >> 2] |= byte << (8u * (nb & 3u));
      }
      if (nb == 16u) {
        *dst = make_uint4(out[0], out[1], out[2], out[3]);
      } else {
        for (uint32_t j = 0; j < nb; j++) entries[o + j] = (uint8_t)(out[j >> 2] >> (8u * (j & 3u)));
      }
    }
  }
}

struct Scratch {
  uint32_t* refused;
  HdrRec* rec;
};
Scratch carve(uint8_t* scratch) { return Scratch{reinterpret_cast<uint32_t*>(scratch), reinterpret_cast<HdrRec*>(scratch + 256)}; }
uint64_t scratch_bytes_for(uint32_t n) { return 256u + (uint64_t)n * sizeof(HdrRec); }

hipError_t launch_plan(hipStream_t st, const uint8_t* keys, uint64_t keys_bytes, const uint64_t* key_off,
                       const uint32_t* key_len, const uint64_t* stored_off, const uint64_t* avail,
                       const uint64_t* svc, const uint64_t* size, const uint32_t* checksum, const int32_t* status_in,
                       uint32_t n, uint64_t files_bytes, uint32_t hash_type, uint8_t* scratch, uint64_t* entry_off,
                       uint32_t* entry_len, uint64_t* total, uint64_t* hashed, uint32_t* kind, int32_t* status) {
  const Scratch k = carve(scratch);
  KDB_TRY(hipMemsetAsync(k.refused, 0, 4, st));
  hipLaunchKernelGGL(compact_plan_kernel, dim3(grid_for(n, 256, 4096)), dim3(256), 0, st, keys, keys_bytes, key_off,
                     key_len, stored_off, avail, svc, size, checksum, status_in, n, files_bytes, hash_type, k.rec,
                     entry_len, hashed, kind, status, k.refused);
  KDB_TRY(hipGetLastError());
  return launch_exclusive_scan(st, entry_len, n, entry_off, total);
}

bool plan_args_ok(const uint8_t* keys, const uint64_t* key_off, const uint32_t* key_len, const uint64_t* stored_off,
                  const uint64_t* avail, const uint64_t* svc, const uint64_t* size, const uint32_t* checksum,
                  const int32_t* status_in, uint32_t n, uint32_t hash_type, uint8_t* scratch, uint64_t scratch_bytes,
                  uint64_t* entry_off, uint32_t* entry_len, uint64_t* total, uint64_t* hashed, uint32_t* kind,
                  int32_t* status) {
  if (!total || hash_type > 1) return false;
  if (n == 0) return true;
  return keys && key_off && key_len && stored_off && avail && svc && size && checksum && status_in && scratch &&
         (reinterpret_cast<uintptr_t>(scratch) & 7u) == 0 && scratch_bytes >= scratch_bytes_for(n) && entry_off &&
         entry_len && hashed && kind && status;
}

}  // namespace
}  // namespace kdb_lz4

using namespace kdb_lz4;

extern "C" uint64_t kdb_compact_scratch_bytes(uint32_t n) { return scratch_bytes_for(n); }

extern "C" uint32_t kdb_compact_piece_bytes(void) { return kPiece; }

extern "C" int kdb_compact_plan_batch(void* stream, const uint8_t* keys, uint64_t keys_bytes, const uint64_t* key_off,
                                      const uint32_t* key_len, const uint64_t* stored_off, const uint64_t* avail,
                                      const uint64_t* svc, const uint64_t* size, const uint32_t* checksum,
                                      const int32_t* status_in, uint32_t n, uint64_t files_bytes, uint32_t hash_type,
                                      uint8_t* scratch, uint64_t scratch_bytes, uint64_t* entry_off,
                                      uint32_t* entry_len, uint64_t* total, uint64_t* hashed, uint32_t* kind,
                                      int32_t* status) {
  if (!plan_args_ok(keys, key_off, key_len, stored_off, avail, svc, size, checksum, status_in, n, hash_type, scratch,
                    scratch_bytes, entry_off, entry_len, total, hashed, kind, status))
    return KDB_PUT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) return hip_code(hipMemsetAsync(total, 0, 8, st));
  return hip_code(launch_plan(st, keys, keys_bytes, key_off, key_len, stored_off, avail, svc, size, checksum,
                              status_in, n, files_bytes, hash_type, scratch, entry_off, entry_len, total, hashed, kind,
                              status));
}

extern "C" int kdb_compact_entries_batch_timed(void* stream, const uint8_t* files, uint64_t files_bytes,
                                               const uint8_t* keys, uint64_t keys_bytes, const uint64_t* key_off,
                                               const uint32_t* key_len, const uint64_t* stored_off,
                                               const uint64_t* avail, const uint64_t* svc, const uint64_t* size,
                                               const uint32_t* checksum, const int32_t* status_in, uint32_t n,
                                               uint32_t hash_type, uint8_t* scratch, uint64_t scratch_bytes,
                                               uint8_t* entries, uint64_t entries_cap, uint64_t* entry_off,
                                               uint32_t* entry_len, uint64_t* total, uint64_t* hashed, uint32_t* kind,
                                               int32_t* status, uint32_t* refused, float* copy_ms) {
  if (copy_ms) *copy_ms = 0.f;
  if (!plan_args_ok(keys, key_off, key_len, stored_off, avail, svc, size, checksum, status_in, n, hash_type, scratch,
                    scratch_bytes, entry_off, entry_len, total, hashed, kind, status))
    return KDB_PUT_EINVAL;
  if (n && (!files || !entries || (reinterpret_cast<uintptr_t>(files) & 15u) || (reinterpret_cast<uintptr_t>(entries) & 15u)))
    return KDB_PUT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (refused) *refused = 0;
  if (n == 0) return hip_code(hipMemsetAsync(total, 0, 8, st));
  hipError_t e = launch_plan(st, keys, keys_bytes, key_off, key_len, stored_off, avail, svc, size, checksum, status_in,
                             n, files_bytes, hash_type, scratch, entry_off, entry_len, total, hashed, kind, status);
  if (e != hipSuccess) return hip_code(e);
  // the plan's total and its refusals: all the host sees of the window
  uint64_t h_total = 0;
  uint32_t h_refused = 0;
  e = hipMemcpyAsync(&h_total, total, 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(&h_refused, carve(scratch).refused, 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return hip_code(e);
  if (refused) *refused = h_refused;
  if (h_total > entries_cap) return KDB_PUT_EINVAL;
  if (h_total == 0) return KDB_PUT_OK;
  hipEvent_t ev[2] = {nullptr, nullptr};
  if (copy_ms) {                              // the copy kernel alone, for tools/bench_compact.py
    e = hipEventCreate(&ev[0]);
    if (e == hipSuccess) e = hipEventCreate(&ev[1]);
    if (e == hipSuccess) e = hipEventRecord(ev[0], st);
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(compact_copy_kernel, dim3(grid_for(h_total, kPiece, 1u << 20)), dim3(kCopyBlock), 0, st, files,
                       files_bytes, keys, key_off, stored_off, carve(scratch).rec, entry_off, entry_len, n, total,
                       entries, entries_cap);
    e = hipGetLastError();
  }
  if (copy_ms) {
    if (e == hipSuccess) e = hipEventRecord(ev[1], st);
    if (e == hipSuccess) e = hipEventSynchronize(ev[1]);
    if (e == hipSuccess) e = hipEventElapsedTime(copy_ms, ev[0], ev[1]);
    for (hipEvent_t x : ev)
      if (x) (void)hipEventDestroy(x);
  }
  return hip_code(e);
}

extern "C" int kdb_compact_entries_batch(void* stream, const uint8_t* files, uint64_t files_bytes,
                                         const uint8_t* keys, uint64_t keys_bytes, const uint64_t* key_off,
                                         const uint32_t* key_len, const uint64_t* stored_off, const uint64_t* avail,
                                         const uint64_t* svc, const uint64_t* size, const uint32_t* checksum,
                                         const int32_t* status_in, uint32_t n, uint32_t hash_type, uint8_t* scratch,
                                         uint64_t scratch_bytes, uint8_t* entries, uint64_t entries_cap,
                                         uint64_t* entry_off, uint32_t* entry_len, uint64_t* total, uint64_t* hashed,
                                         uint32_t* kind, int32_t* status, uint32_t* refused) {
  return kdb_compact_entries_batch_timed(stream, files, files_bytes, keys, keys_bytes, key_off, key_len, stored_off,
                                         avail, svc, size, checksum, status_in, n, hash_type, scratch, scratch_bytes,
                                         entries, entries_cap, entry_off, entry_len, total, hashed, kind, status,
                                         refused, nullptr);
}
