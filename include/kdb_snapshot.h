/* include/kdb_snapshot.h -- a read-only view of a kdb_index as of a point:
 * Database::NewSnapshot (interface/database.cc:301-327) and the Snapshot it
 * returns (interface/snapshot.h), which every Database::NewIterator is made
 * over (database.cc:361-368) and which the reference's compaction relies on
 * (storage/storage_engine.h:1078, 1120-1192).  Part of include/kdb_put.h, which
 * includes it; the declarations live here because the exported-symbol tests of
 * the lookup, the scan and the add pin the exact lists of kdb_index_* names the
 * other headers declare.
 *
 * Let F be the files the handle held at kdb_snapshot_create and R their rows.
 * The rows a handle holds keep their sequence numbers, file slots and ranks
 * through every kdb_index_add_files (DESIGN.md 4.8 "Adding files"), so "the
 * lookup restricted to rows of sequence number < R", run over the handle's
 * current buckets, is what a handle that kdb_index_load_files loaded over F
 * alone, in the same buffer, answers: every output of kdb_snapshot_get_batch
 * equals that handle's kdb_index_get_batch element for element, and after
 * kdb_snapshot_scan_prepare every output of kdb_snapshot_scan_batch, live,
 * key_bytes, max_key_len and whether a sort ran equal its scan's -- after any
 * number of successful or refused adds, whether the bucket count stayed or
 * doubled.  The snapshot copies no row, no bucket and no file.  DESIGN.md 4.11
 * records where this differs from the reference.
 *
 * Calls on a handle and its snapshots are serialised by the caller, and the
 * files buffer outlives the snapshots as it outlives the lookups.
 */
#ifndef KDB_SNAPSHOT_H_
#define KDB_SNAPSHOT_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct kdb_index;
struct kdb_snapshot;

/* Database::NewSnapshot (database.cc:301-327) without the second
 * StorageEngine (:313-318) and without its LoadDatabase up to fileid_end
 * (storage/hstable_manager.h:983): records the handle's row count, file slot
 * count and loaded-file count.  Launches nothing and allocates nothing on the
 * device.  The open file is not flushed (database.cc:305-306,
 * FlushCurrentFileForSnapshot, storage_engine.h:1181-1183): the snapshot is taken
 * over the files the handle holds, and closing the writer's file first is the
 * caller's step.  A handle without rows gives a valid empty snapshot.  Several
 * snapshots of one handle may be open at once; while one is,
 * kdb_index_load_files and kdb_index_destroy of the handle return
 * KDB_PUT_EINVAL and change nothing (a load replaces the sequence numbers the
 * snapshot stands on). */
int kdb_snapshot_create(struct kdb_index* ix, struct kdb_snapshot** snap);
/* Snapshot::Close (snapshot.h:67-76): frees the snapshot's prepared scan and
 * lowers the handle's count of open snapshots.  No file is pinned while a
 * snapshot is open and none is removed at its release
 * (StorageEngine::ReleaseSnapshot, storage_engine.h:1132-1156). */
int kdb_snapshot_release(struct kdb_snapshot* snap);

/* Rows, and file slots (every file given to the handle, whatever its status),
 * as of kdb_snapshot_create. */
int kdb_snapshot_entry_count(const struct kdb_snapshot* snap, uint64_t* count);
int kdb_snapshot_file_count(const struct kdb_snapshot* snap, uint32_t* count);

/* Snapshot::Get (snapshot.h:78-92): kdb_index_get_batch as of the snapshot.
 * The arguments after the snapshot, the outputs, the summary and the statuses
 * are kdb_index_get_batch's; kdb_index_get_scratch_bytes sizes the scratch.  A
 * key whose newest entry below the limit is a put that a later file deletes or
 * overwrites is found with its old value; an empty snapshot answers
 * KDB_GET_NOTFOUND for every key. */
int kdb_snapshot_get_batch(const struct kdb_snapshot* snap, void* stream, const uint8_t* keys,
                           const uint64_t* key_off, const uint32_t* key_len, uint32_t n, int verify_header,
                           uint64_t multipart_required, uint8_t* scratch, uint64_t scratch_bytes,
                           uint64_t* stored_off, uint64_t* avail, uint64_t* svc, uint64_t* size, uint32_t* checksum,
                           uint32_t* checksum_initial, uint64_t* out_off, uint64_t* location, int32_t* status,
                           uint64_t* summary);

/* Snapshot::NewIterator (snapshot.h:110-121): kdb_index_scan_prepare,
 * kdb_index_scan_sort_steps and kdb_index_scan_batch (include/kdb_scan.h) as of
 * the snapshot, with their argument lists and their KDB_PUT_EINVAL cases.  The
 * live list, the key prefix and its host copy belong to the snapshot: a
 * prepare here touches neither the handle's prepared scan nor another
 * snapshot's, and an add to the handle, which drops the handle's prepared
 * scan, drops no snapshot's. */
int kdb_snapshot_scan_prepare(struct kdb_snapshot* snap, void* stream, int verify_header, uint64_t* live,
                              uint64_t* key_bytes, uint32_t* max_key_len);
int kdb_snapshot_scan_sort_steps(const struct kdb_snapshot* snap, uint32_t* steps);
int kdb_snapshot_scan_batch(const struct kdb_snapshot* snap, void* stream, uint64_t first, uint32_t n,
                            uint64_t multipart_required, void* scratch, uint64_t scratch_bytes, uint8_t* keys_out,
                            uint64_t keys_cap, uint64_t* key_off, uint32_t* key_len, uint64_t* stored_off,
                            uint64_t* avail, uint64_t* svc, uint64_t* size, uint32_t* checksum,
                            uint32_t* checksum_initial, uint64_t* out_off, uint64_t* location, int32_t* status,
                            uint64_t* summary);

#ifdef __cplusplus
}
#endif

#endif /* KDB_SNAPSHOT_H_ */
