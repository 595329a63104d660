/* include/kdb_index_tail.h -- read your writes: the rows of the device
 * writer's one open file, the "tail" of a kdb_index.  What the rest of
 * StorageEngine::ProcessingLoopIndex does after every flush
 * (storage/storage_engine.h:298-372): the (hash, location) pairs of the file
 * still being written go into the live index.  kdb_index_add_files took that
 * row a closed file at a time; this takes the open file, after every append.
 * Part of include/kdb_put.h, which includes it; the declarations live here
 * because the exported-symbol tests pin the exact name lists of the other
 * headers.
 *
 * The open file has no footer and no offset array yet: its rows (varint64
 * hash, varint32 offset) are staged at the end of the writer's arena, stored
 * backwards, and are indexed from there.  After a successful
 * kdb_index_set_tail the handle answers kdb_index_entry_count,
 * kdb_index_pairs, kdb_index_get_batch and, after a new
 * kdb_index_scan_prepare, the scan exactly as a handle that
 * kdb_index_load_files loaded over the closed files and the file the writer
 * would produce if it closed now.  DESIGN.md 4.8 ("The open file's tail")
 * records where this differs from the reference.
 */
#ifndef KDB_INDEX_TAIL_H_
#define KDB_INDEX_TAIL_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct kdb_index;
struct kdb_hstable_dev;

#define KDB_INDEX_TAIL_REPARSE  1u   /* flags: parse the whole staging again, not only what was appended
                                        since the last call; the same handle results (tests, A/B runs) */

/* The writer's open file, as kdb_hstable_dev_open_file reports it. */
struct kdb_open_file {
  uint32_t open;         /* 1: a file is open; 0: none, every other field is 0 */
  uint32_t fileid;
  uint32_t incomplete;   /* the writer has discarded the staging: the file would close without an offset array */
  uint32_t pad;
  uint64_t timestamp;    /* the header's */
  uint64_t file_off;     /* the file's offset in the arena */
  uint64_t bytes;        /* its size so far, the 8 KiB header block included */
  uint64_t rows;         /* entries registered so far */
  uint64_t row_bytes;    /* bytes of their staged rows */
  uint64_t rows_last;    /* arena offset of staged byte 0; staged byte b lies at rows_last - b */
};

/* Waits for the writer's queued work, as kdb_hstable_dev_files does. */
int kdb_hstable_dev_open_file(const struct kdb_hstable_dev* w, struct kdb_open_file* out);

/* Sets, grows or replaces the tail: the rows of *f, which lies in d_files (the
 * buffer the handle was loaded over; a handle that holds no files adopts it).
 * Synchronous, and not to run concurrently with lookups on the handle.  The
 * tail's rows take the sequence numbers after the closed files' rows, and the
 * file the next file slot and rank: what kdb_index_add_files gives the same
 * file when it arrives closed.  A tail of the same fileid as the one held
 * grows: only the staging bytes and rows beyond those held are parsed.  A tail
 * of another fileid replaces the one held (that file has closed; the caller
 * adds it through kdb_index_add_files).  f->open == 0 or f->incomplete != 0:
 * any tail held is dropped, no rows are added (the closed form of an
 * incomplete file loads with status -1 and no rows).
 * KDB_PUT_EINVAL, and after it or a HIP error the handle answers as before the
 * call, tail included: another d_files than the handle's; a file that does not
 * sort strictly after every loaded file of status 0 by (timestamp, fileid);
 * the fileid held with fewer rows or row_bytes than held; staging bytes that
 * do not hold exactly two varints per row, a hash of more than 10 bytes or an
 * offset of more than 5; a range outside d_files as far as the record tells
 * (rows_last < row_bytes - 1); more than 2^30 rows in all.  A successful call
 * drops a prepared scan.  Snapshots of kdb_snapshot_create do not see the tail
 * and may be open; one of kdb_snapshot_create_tail (include/kdb_live.h) holds
 * the tail to the file it took until that file has been added closed.
 * *rows_added_out = the rows the tail gained: all of a new tail's, those
 * beyond the rows held of a tail that grew (may be NULL). */
int kdb_index_set_tail(struct kdb_index* ix, void* stream, const uint8_t* d_files, const struct kdb_open_file* f,
                       uint32_t flags, uint64_t* rows_added_out);

/* Drops the tail, if one is held: the handle is again the closed files'. */
int kdb_index_drop_tail(struct kdb_index* ix, void* stream);

/* *held = 1 where a tail is held, with its *fileid, *rows and *bytes (the
 * file's size); *rows_parsed_last = rows the last successful
 * kdb_index_set_tail parsed; *nbuckets = the handle's bucket count.  A
 * successful kdb_index_add_files with nadd > 0 and kdb_index_load_files drop
 * the tail.  Any out-pointer but held may be NULL. */
int kdb_index_tail_stats(const struct kdb_index* ix, uint32_t* held, uint32_t* fileid, uint64_t* rows,
                         uint64_t* bytes, uint64_t* rows_parsed_last, uint64_t* nbuckets);

#ifdef __cplusplus
}
#endif

#endif /* KDB_INDEX_TAIL_H_ */
