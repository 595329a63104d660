/* include/kdb_index_add.h -- newly closed HSTable files added to a loaded
 * kdb_index: what StorageEngine::ProcessingLoopIndex does with the map_index_out
 * of HSTableManager::WriteOrdersAndFlushFile after every write-buffer flush
 * (storage/storage_engine.h:298-372), a closed file at a time.  Part of
 * include/kdb_put.h, which includes it; the declarations live here because the
 * exported-symbol tests of the lookup and the scan pin the exact lists of
 * kdb_index_* names kdb_put.h and kdb_scan.h themselves declare.
 *
 * After a successful add the handle answers kdb_index_entry_count,
 * kdb_index_pairs, kdb_index_get_batch and, after a new
 * kdb_index_scan_prepare, the scan exactly as a handle that
 * kdb_index_load_files loaded over the union of the files.  DESIGN.md 4.8
 * ("Adding files") records where this differs from the reference.
 */
#ifndef KDB_INDEX_ADD_H_
#define KDB_INDEX_ADD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct kdb_index;

#define KDB_INDEX_FILE_ORDER   (-4)  /* file_status: sorts at or before a loaded file */
#define KDB_INDEX_ADD_REBUILD  1u    /* flags: rebuild the buckets from the resident rows even where a merge would do;
                                        accepted and without effect, the rebuild being the only path */

/* Adds nadd files resident in d_files, the buffer the handle was loaded over
 * (a handle that holds no files adopts d_files: the add is then a load).  The
 * arrays are host arrays as for kdb_index_load_files, of the new files alone.
 * Synchronous, like the load, and not to run concurrently with lookups on the
 * handle.  The new files are verified as the load verifies them
 * (file_status_out 0 / -1 / -2 / -3; a file with a nonzero status takes a file
 * slot and contributes no rows), ordered by (timestamp, fileid) among
 * themselves, and their rows take the sequence numbers after the loaded rows.
 * Every new file of status 0 must sort strictly after every loaded file of
 * status 0; otherwise those files report KDB_INDEX_FILE_ORDER, the call
 * returns KDB_PUT_EINVAL and nothing is added (a file added twice is refused
 * by this rule).  After any error -- KDB_PUT_EINVAL (also: another d_files
 * than the handle's, which writes no status; more than 2^30 rows in all) or a
 * HIP error -- the handle answers every lookup as before the call.  A
 * successful add drops a prepared scan: kdb_index_scan_batch returns
 * KDB_PUT_EINVAL until kdb_index_scan_prepare runs again.  nadd = 0 changes
 * nothing.  *entries_added_out = rows added (may be NULL). */
int kdb_index_add_files(struct kdb_index* ix, void* stream, const uint8_t* d_files, const uint64_t* file_off,
                        const uint64_t* file_size, const uint32_t* fileid, uint32_t nadd, uint32_t flags,
                        int32_t* file_status_out, uint64_t* entries_added_out);

/* Debug counters of the last successful add with nadd > 0 (KDB_PUT_EINVAL
 * before one, and after a load): *merged = 0, the buckets having been rebuilt
 * from all resident rows (1 is kept for a path that moves the old buckets'
 * slots and places only the new rows; none is built); *nbuckets = the bucket
 * count after it; *rows_parsed = rows the parse wrote, every pass counted.  For
 * tests and tuning; any may be NULL. */
int kdb_index_add_stats(const struct kdb_index* ix, uint32_t* merged, uint64_t* nbuckets, uint64_t* rows_parsed);

#ifdef __cplusplus
}
#endif

#endif /* KDB_INDEX_ADD_H_ */
