/* include/kdb_compact.h -- compaction by copy: the live entries of a view moved
 * from their files into compacted files without decoding a value, the
 * compacted files' identity, and the hand-over that lets the database go on
 * over the compacted files and the files added since.  Part of
 * include/kdb_put.h, which includes it.  Replaces
 *   StorageEngine::Compaction, steps 6-9 and 14     storage/storage_engine.h:796-1010
 *   HSTableManager::LockSequenceTimestamp           storage/hstable_manager.h
 *   HSTableManager::WriteFirstPartOrSmallOrder      storage/hstable_manager.h:637-673
 * (steps 1-4, which entries are kept, are the scan of kdb_scan.h /
 * kdb_snapshot.h).  Codes are kdb_put.h's.
 */
#ifndef KDB_COMPACT_H_
#define KDB_COMPACT_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct kdb_index;
struct kdb_hstable_dev;

/* ------------------------------------------------------------------ the copy
 * A scan window as kdb_index_scan_batch / kdb_snapshot_scan_batch leave it in
 * device memory (the packed keys, key_off, key_len, stored_off, avail, svc,
 * size, checksum, status) becomes the output arrays of kdb_put_entries_batch,
 * which kdb_hstable_dev_append takes as they are.  Entry v is what
 * WriteFirstPartOrSmallOrder writes for a self-contained put:
 *   flags kEntryFull (no delete, uncompacted and padding clear), size_key,
 *   size_value = size[v], size_value_compressed = svc[v], size_padding 0, the
 *   key's hash, checksum_content = checksum[v] (carried over, never computed
 *   again: storage_engine.h:848), the header CRC-8; then the key; then
 *   used = svc[v] ? svc[v] : size[v] bytes from files[stored_off[v] ..).
 * kind[v] = KDB_PUT_SELF_CONTAINED, hashed[v] = the key hash.  A row is
 * REFUSED -- status[v] = -1, entry_len[v] = 0, nothing copied -- where
 * status_in[v] != 0, used > avail[v], stored_off[v] + used > files_bytes, the
 * key is empty or lies outside keys[0, keys_bytes), or the entry would not fit
 * 32 bits.  No byte of a value is read outside [stored_off, stored_off + avail)
 * except by the aligned 16-byte loads around its ends, which stay inside
 * files[0, files_bytes) and inside the value's own file. */

/* Device scratch bytes for a window of n (one 64-byte header record each). */
uint64_t kdb_compact_scratch_bytes(uint32_t n);
/* Bytes of the dense output stream one workgroup of the copy kernel writes. */
uint32_t kdb_compact_piece_bytes(void);

/* The plan alone, stream-ordered, no synchronisation: entry_len, entry_off
 * (exclusive sum), *total = the sum (device u64), hashed, kind, status, and the
 * encoded headers in the scratch.  A caller sizes its buffers from the totals. */
int kdb_compact_plan_batch(void* stream, const uint8_t* keys, uint64_t keys_bytes, const uint64_t* key_off,
                           const uint32_t* key_len, const uint64_t* stored_off, const uint64_t* avail,
                           const uint64_t* svc, const uint64_t* size, const uint32_t* checksum,
                           const int32_t* status_in, uint32_t n, uint64_t files_bytes, uint32_t hash_type,
                           uint8_t* scratch, uint64_t scratch_bytes, uint64_t* entry_off, uint32_t* entry_len,
                           uint64_t* total, uint64_t* hashed, uint32_t* kind, int32_t* status);

/* The plan, then the copy into entries[0, entries_cap) (16-byte aligned, as
 * `files` must be).  Synchronises `stream` once, between the two, to read the
 * plan's total: a total above entries_cap returns KDB_PUT_EINVAL before any
 * byte is copied.  *refused (host, may be NULL) = rows refused. */
int kdb_compact_entries_batch(void* stream, const uint8_t* files, uint64_t files_bytes, const uint8_t* keys,
                              uint64_t keys_bytes, const uint64_t* key_off, const uint32_t* key_len,
                              const uint64_t* stored_off, const uint64_t* avail, const uint64_t* svc,
                              const uint64_t* size, const uint32_t* checksum, const int32_t* status_in, uint32_t n,
                              uint32_t hash_type, uint8_t* scratch, uint64_t scratch_bytes, uint8_t* entries,
                              uint64_t entries_cap, uint64_t* entry_off, uint32_t* entry_len, uint64_t* total,
                              uint64_t* hashed, uint32_t* kind, int32_t* status, uint32_t* refused);

/* The same, for measurement: with copy_ms != NULL the copy kernel is bracketed
 * by events and waited for, *copy_ms = its time alone (0 where none ran). */
int kdb_compact_entries_batch_timed(void* stream, const uint8_t* files, uint64_t files_bytes, const uint8_t* keys,
                                    uint64_t keys_bytes, const uint64_t* key_off, const uint32_t* key_len,
                                    const uint64_t* stored_off, const uint64_t* avail, const uint64_t* svc,
                                    const uint64_t* size, const uint32_t* checksum, const int32_t* status_in,
                                    uint32_t n, uint32_t hash_type, uint8_t* scratch, uint64_t scratch_bytes,
                                    uint8_t* entries, uint64_t entries_cap, uint64_t* entry_off, uint32_t* entry_len,
                                    uint64_t* total, uint64_t* hashed, uint32_t* kind, int32_t* status,
                                    uint32_t* refused, float* copy_ms);

/* ------------------------------------------------- the compacted files' identity
 * The timestamp to lock: the largest header timestamp among the status-0 files
 * of the handle's first nfiles file slots (a snapshot's files; the handle's own
 * count for the whole index), 0 where there is none.  KDB_PUT_EINVAL where
 * nfiles exceeds the files held, or one of those files is of the large type
 * (kCompactedLargeType): this project writes none and compacts none. */
int kdb_index_view_timestamp(const struct kdb_index* ix, uint32_t nfiles, uint64_t* timestamp_max);

/* kdb_hstable_dev_create with the files' type (1 kUncompactedRegularType, 2
 * kCompactedRegularType; header block and footer) and a locked timestamp:
 * where timestamp_lock != 0 every file's header carries it instead of the
 * file's id (HSTableManager::LockSequenceTimestamp).  (1, 0) is
 * kdb_hstable_dev_create. */
int kdb_hstable_dev_create2(uint64_t hstable_size, uint32_t hash_type, uint64_t arena_bytes, uint32_t filetype,
                            uint64_t timestamp_lock, struct kdb_hstable_dev** w);

/* *bytes = the size so far of the file that is open, 0 where none is. */
int kdb_hstable_dev_open_bytes(const struct kdb_hstable_dev* w, uint64_t* bytes);

/* The hand-over (Compaction() steps 8, 9 and 14), with no file open:
 *   1. the writer's closed files are renumbered first_fileid, first_fileid + 1,
 *      ... (ids are names only, no file holds its own);
 *   2. nsrc files, file f = d_src[src_off[f] .. +src_size[f]) with id
 *      src_id[f] (host arrays), are copied device to device on `stream` behind
 *      the writer's files, at 64-byte-aligned offsets, keeping their ids;
 *   3. the writer returns to normal operation: files opened from now on are of
 *      type 1 with id = timestamp = the next id above everything it holds.
 * KDB_PUT_EINVAL, the writer exactly as before: a file is open, the new ids
 * would pass 2^32 - 1, an adopted id is 0, >= first_fileid or given twice, an
 * adopted file is larger than a file may be, the source overlaps the arena, or
 * the adopted bytes do not fit between the closed files and the row staging
 * at the arena's end. */
int kdb_hstable_dev_adopt(struct kdb_hstable_dev* w, void* stream, uint32_t first_fileid, const uint8_t* d_src,
                          const uint64_t* src_off, const uint64_t* src_size, const uint32_t* src_id, uint32_t nsrc);

#ifdef __cplusplus
}
#endif

#endif /* KDB_COMPACT_H_ */
