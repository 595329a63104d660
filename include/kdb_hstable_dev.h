/* include/kdb_hstable_dev.h -- HSTable files built in device memory: the
 * writer of kdb_hstable_writer_* (csrc/hstable.cc) with the framing on the GPU
 * (csrc/hstable_dev.hip).  Part of include/kdb_put.h, which includes it.
 *
 * append() takes the outputs of kdb_put_entries_batch where they lie, in
 * device memory, and cuts them into files by the rule of
 * HSTableManager::WriteOrdersAndFlushFile (csrc/hstable_cut.h): the entry
 * bytes, the 8 KiB header block, the varint rows of the offset array and the
 * footer with its CRC32C are all written by kernels into one device buffer,
 * the arena.  The closed files are byte for byte those of the host writer;
 * kdb_index_load_files can load them where they are.
 *
 * The arena is allocated once and never grows.  Files lie one after the other
 * from its start, each at a 64-byte-aligned offset; the rows of the file that
 * is still open are staged at the arena's end, growing downwards, until the
 * file closes.  What a database needs is bounded by
 *     entry_bytes                         every entry byte, once
 *   + 15 * n_entries                      the rows in the files: a varint64 hash
 *                                         (<= 10 bytes) and a varint32 offset (<= 5)
 *   + 15 * n_entries                      the open file's rows while staged (they
 *                                         are copied, so both copies exist at a close)
 *   + files * (8192 + 36 + 64)            header block, footer, alignment
 * with files = entry_bytes / (hstable_size - 8192) + 2: every file but the
 * last is closed with at least hstable_size bytes, 8192 of them its header
 * block (one more for the remainder, one for rounding).
 * kdb_hstable_dev_arena_bytes returns that sum, rounded up to 64.
 *
 * One writer belongs to one thread and one device; every function returns
 * KDB_PUT_OK or a negative code of kdb_put.h.  There is no CPU path: without
 * a device, create fails with KDB_PUT_ENODEV or KDB_PUT_EHIP.
 */
#ifndef KDB_HSTABLE_DEV_H_
#define KDB_HSTABLE_DEV_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kdb_hstable_dev kdb_hstable_dev;

/* Upper bound on the arena for a database of n_entries entries totalling
 * entry_bytes bytes (host arithmetic; ~0 where the sum does not fit 64 bits
 * or hstable_size <= 8192). */
uint64_t kdb_hstable_dev_arena_bytes(uint64_t hstable_size, uint64_t entry_bytes, uint64_t n_entries);

/* One device allocation of arena_bytes (>= 8192 + 64).  Argument checks as
 * kdb_hstable_writer_create2: hash_type <= 1, hstable_size > 8192. */
int kdb_hstable_dev_create(uint64_t hstable_size, uint32_t hash_type, uint64_t arena_bytes, kdb_hstable_dev** w);
int kdb_hstable_dev_destroy(kdb_hstable_dev* w);

/* One batch (a write-buffer flush): the seven arrays are device pointers, the
 * outputs of kdb_put_entries_batch (entry v is d_entries[d_entry_off[v] ..
 * +d_entry_len[v]); the stream need not be dense or ascending).  Work is
 * queued on `stream`; the call synchronises it once, to download the plan:
 * one record of 40 bytes per file the batch touches.  The inputs may be reused
 * once later work on `stream` is ordered after the call.  A per-entry work
 * area of the handle grows to the largest n seen.
 * KDB_PUT_EINVAL, the writer (files, open file, arena) exactly as before:
 * the batch does not fit the arena, or an entry would start past offset
 * 2^32 - 1 of its file. */
int kdb_hstable_dev_append(kdb_hstable_dev* w, void* stream, const uint8_t* d_entries, const uint64_t* d_entry_off,
                           const uint32_t* d_entry_len, const uint64_t* d_hashed, const uint32_t* d_kind,
                           const int32_t* d_status, uint32_t n);
/* Database::Close: closes the open file (queued on the stream of the last append). */
int kdb_hstable_dev_close(kdb_hstable_dev* w);

int kdb_hstable_dev_file_count(const kdb_hstable_dev* w, uint32_t* count);
/* The closed files, as kdb_index_load_files takes them: *d_base = the arena,
 * file f = d_base[file_off[f] .. +file_size[f]) with id fileid[f] (host
 * arrays of `cap` entries, filled for min(cap, count) files; any may be NULL).
 * Waits for the writer's queued work.  The arena stays the writer's: it is
 * valid until reset or destroy. */
int kdb_hstable_dev_files(const kdb_hstable_dev* w, const uint8_t** d_base, uint64_t* file_off, uint64_t* file_size,
                          uint32_t* fileid, uint32_t cap);
/* Copies closed file i (file_size bytes) to host_dst on `stream` and waits for it. */
int kdb_hstable_dev_download(const kdb_hstable_dev* w, uint32_t i, uint8_t* host_dst, void* stream);
/* A fresh database directory (ids and timestamps from 1 again); the arena is kept. */
int kdb_hstable_dev_reset(kdb_hstable_dev* w);

/* Compaction without a host copy: turns the decode outputs of a scan window
 * (kdb_index_scan_batch + kdb_get_values_batch, device arrays of n) into the
 * chunk arrays of kdb_put_entries_batch, one chunk per value: part_first[0..n]
 * = 0..n, chunk_len[v] = out_len[v].  *d_flag (u32) is set to 1 where some
 * status or dstatus is nonzero or a value is longer than a chunk may be, else
 * to 0.  Stream-ordered. */
int kdb_hstable_dev_feed(void* stream, const uint64_t* d_out_len, const int32_t* d_status, const int32_t* d_dstatus,
                         uint32_t n, uint32_t* d_part_first, uint32_t* d_chunk_len, uint32_t* d_flag);

#ifdef __cplusplus
}
#endif

#endif /* KDB_HSTABLE_DEV_H_ */
