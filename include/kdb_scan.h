/* include/kdb_scan.h -- the scan over a loaded kdb_index: every live entry of
 * the database, in iterator order (Database::NewIterator, RegularIterator::Next,
 * interface/iterator.h:112-214).  Part of include/kdb_put.h, which includes it;
 * the declarations live here because the exported-symbol test of the lookup
 * pins the exact list of kdb_index_* names kdb_put.h itself declares.
 *
 * Row r (sequence number r of kdb_index_pairs) is LIVE iff the lookup of
 * kdb_index_get_batch, run on the key stored in r's entry, selects row r with
 * status 0 or KDB_GET_MULTIPART: the entry decodes, is valid and is no delete,
 * the hash of its stored key is the row's hash, and no newer equal-hash row
 * holds a valid entry with the same key.  The scan returns the live rows
 * ordered by (file rank in (timestamp, fileid) order, offset ascending), each
 * once.  DESIGN.md 4.9 records where this differs from the reference.
 */
#ifndef KDB_SCAN_H_
#define KDB_SCAN_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct kdb_index;

/* The liveness pass over all rows and the ordered live list, kept in the
 * handle.  Synchronous, like the load; replaces an earlier list;
 * kdb_index_load_files drops it.  verify_header as in kdb_index_get_batch (the
 * CRC-8 of every header examined).  *live = live rows, *key_bytes = the sum of
 * their key lengths, *max_key_len = the longest (any may be NULL).  An index
 * with zero rows prepares to live = 0. */
int kdb_index_scan_prepare(struct kdb_index* ix, void* stream, int verify_header, uint64_t* live,
                           uint64_t* key_bytes, uint32_t* max_key_len);
/* Compare-exchange passes the last prepare ran to order its list: 0 when every
 * file's rows ascend by offset (the compaction is then already in iterator
 * order), the passes of a bitonic network otherwise.  For tests and tuning. */
int kdb_index_scan_sort_steps(const struct kdb_index* ix, uint32_t* steps);

/* Device scratch bytes kdb_index_scan_batch needs for a window of n. */
uint64_t kdb_index_scan_scratch_bytes(uint32_t n);
/* Live rows [first, first + n) of the prepared list, device pointers,
 * stream-ordered.  Row v of the window: its key is keys_out[key_off[v] ..
 * +key_len[v]) (packed, key_off[0] = 0); the remaining arrays are the outputs
 * of kdb_index_get_batch for that entry, same order and meaning, so
 * kdb_get_values_batch runs on them as is.  status is 0 or KDB_GET_MULTIPART
 * (is_compressed && size_value > multipart_required, 0 = the 1 MiB default).
 * KDB_PUT_EINVAL, writing nothing: before prepare, first + n > live, or the
 * window's key bytes exceed keys_cap (n * max_key_len always suffices). */
int kdb_index_scan_batch(const struct kdb_index* ix, void* stream, uint64_t first, uint32_t n,
                         uint64_t multipart_required, void* scratch, uint64_t scratch_bytes, uint8_t* keys_out,
                         uint64_t keys_cap, uint64_t* key_off, uint32_t* key_len, uint64_t* stored_off,
                         uint64_t* avail, uint64_t* svc, uint64_t* size, uint32_t* checksum,
                         uint32_t* checksum_initial, uint64_t* out_off, uint64_t* location, int32_t* status,
                         uint64_t* summary);

#ifdef __cplusplus
}
#endif

#endif /* KDB_SCAN_H_ */
