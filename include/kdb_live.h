/* include/kdb_live.h -- snapshots and the compaction's hand-over over the
 * device writer's open file: what lets a writer, its index, its snapshots and
 * its compactions go on with no file cut short.  Part of include/kdb_put.h,
 * which includes it; the declarations live here because the exported-symbol
 * tests pin the exact name lists of the other headers.
 *
 * The reference flushes before it takes a snapshot (Database::NewSnapshot,
 * interface/database.cc:305-306) and compacts under a running writer
 * (storage/storage_engine.h:604-1010).  Here nothing is flushed: a snapshot is
 * taken at row granularity inside the open file, and the open file is carried
 * into the compaction's writer as it is.
 */
#ifndef KDB_LIVE_H_
#define KDB_LIVE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct kdb_index;
struct kdb_snapshot;
struct kdb_hstable_dev;

/* kdb_snapshot_create (include/kdb_snapshot.h) over the closed files and the
 * tail the handle holds (include/kdb_index_tail.h): the row limit is the closed
 * files' rows plus the tail's, the file slots and the loaded ranks one more
 * than the closed files'.  With no tail held it is exactly kdb_snapshot_create.
 * Launches nothing and allocates nothing on the device.
 *
 * Let F be the closed files held and X the file the writer would have produced
 * had it closed at this moment, with exactly the tail's rows.  The snapshot
 * answers as a handle kdb_index_load_files loaded over F and X: every output
 * of kdb_snapshot_get_batch, kdb_snapshot_scan_prepare and
 * kdb_snapshot_scan_batch, element for element -- after the tail has grown or
 * been parsed again, after the file has closed and been added, after further
 * files, a new tail on the next file and any doubling of the buckets.  It
 * rests on the open file being numbered closed as it was numbered open, which
 * the handle checks (below) instead of trusting the caller.
 *
 * The pin.  While a snapshot made here with a tail is open and the tail's file
 * has not been added closed, the handle returns KDB_PUT_EINVAL and changes
 * nothing for
 *   kdb_index_drop_tail;
 *   kdb_index_set_tail with no open file, an incomplete file or another fileid
 *   (growth and KDB_INDEX_TAIL_REPARSE of the same file are allowed);
 *   kdb_index_add_files, unless the oldest new file of status 0 by (timestamp,
 *   fileid) is the tail's file -- same id, timestamp and offset in the buffer
 *   -- with at least the pinned rows, the first of which, (hash, offset) by
 *   (hash, offset), equal the rows held (compared on the device before the
 *   handle changes).  The file statuses are reported as by any refused add.
 * After such an add the pin is gone and the snapshot is an ordinary prefix
 * snapshot.  Snapshots of kdb_snapshot_create pin nothing. */
int kdb_snapshot_create_tail(struct kdb_index* ix, struct kdb_snapshot** snap);

/* *included = 1 where the snapshot took a tail, with its *fileid and *rows;
 * *pinned = 1 until that file has been added closed.  All 0 for a snapshot
 * without a tail.  Any out-pointer but included may be NULL. */
int kdb_snapshot_tail_stats(const struct kdb_snapshot* snap, uint32_t* included, uint32_t* fileid, uint64_t* rows,
                            uint32_t* pinned);

/* After kdb_snapshot_scan_prepare: *n = the live entries that lie in files
 * closed when the snapshot was made.  The tail's rank is the largest the
 * snapshot has and the live list is ordered by rank << 32 | offset, so these
 * are entries [0, n) of the list, the windows kdb_snapshot_scan_batch takes.
 * Counted on the device during the prepare: the exclusive sum of the liveness
 * flags in sequence order, read at the first row of the tail.  Where the
 * sorted cold path ran the same holds, because the sort's key is that rank
 * and offset and the count is of rows, taken before the sort.  n = live for a
 * snapshot without a tail.  KDB_PUT_EINVAL before a prepare. */
int kdb_snapshot_scan_closed_live(const struct kdb_snapshot* snap, uint64_t* n);

/* The hand-over with an open file, after kdb_hstable_dev_adopt
 * (include/kdb_compact.h): src's open file becomes dst's open file.  Copied
 * device to device on `stream`: the file's bytes so far, to dst's next
 * 64-byte-aligned offset, and its staged rows, to the end of dst's arena in
 * the same backward layout.  dst takes over the file's id, header timestamp,
 * size, padding and incomplete marks, row count and staged bytes; an
 * incomplete file has no staging and is carried as bytes and state.  For any
 * appends fed afterwards to dst and to an untouched twin of src the file
 * closes byte for byte equal in both; files dst opens later take id =
 * timestamp = one above every id it holds.  src is never modified: the caller
 * stops appending to it.
 * src has no open file: KDB_PUT_OK, nothing done.  KDB_PUT_EINVAL, both
 * writers as before: dst has a file open, hstable_size or hash_type differ,
 * either writer writes compacted files (type 2 or a locked timestamp), the id
 * is 0 or held by dst, the arenas overlap, or the file and its staging do not
 * fit between dst's closed files and its arena's end. */
int kdb_hstable_dev_adopt_open(struct kdb_hstable_dev* dst, void* stream, const struct kdb_hstable_dev* src);

#ifdef __cplusplus
}
#endif

#endif /* KDB_LIVE_H_ */
