/* include/kdb_ops.h -- puts and deletes through one batch: the write path of
 * kdb_put_entries_batch with an operation per item, so that Database::Delete
 * (interface/database.cc:279-286 -> WriteBuffer::Delete, cache/write_buffer.cc:
 * 149-152 -> HSTableManager::WriteFirstPartOrSmallOrder,
 * storage/hstable_manager.h:694-710) has its counterpart.  Part of
 * include/kdb_put.h, which includes it; the declarations live here for the
 * reason kdb_scan.h gives.
 *
 * A delete is a self-contained entry, EntryHeader || key:
 *   flags kTypeDelete | kEntryFull (0x9), checksum_content 0, size_value 0,
 *   size_value_compressed 0, size_padding 0, hash 0
 * and one offset-array row (hash(key), offset) with the key's real hash.  The
 * reference never assigns the header's size_padding and hash (EntryHeader()
 * sets flags alone, storage/format.h:46); its build writes 0 for both, and so
 * does this one.  As RecoverFile takes a recovered row's hash from the header
 * (hstable_manager.h:1149), a delete whose file loses its offset array is
 * filed under hash 0 and the deleted key comes back; KDB_OPS_DELETE_HASHED
 * writes hash(key) into the header instead (the corrected form; the entry
 * differs from the reference's in those 8 bytes and the header's CRC-8).
 */
#ifndef KDB_OPS_H_
#define KDB_OPS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KDB_OP_PUT 0
#define KDB_OP_DELETE 1
#define KDB_OPS_DELETE_HASHED 1u   /* header.hash = hash(key), so that recovery keeps the delete reachable */

/* kdb_put_entries_batch with op[v] (device bytes, one per item; NULL: every
 * item a put) and flags (0 or KDB_OPS_DELETE_HASHED); the remaining arguments
 * are kdb_put_entries_batch's, in its order and with its meaning.  A delete has
 * value_len 0 and no chunks (part_first[v] == part_first[v + 1]); its outputs
 * are the entry, hashed[v] = hash(key), crc[v] = 0, kind[v] =
 * KDB_PUT_SELF_CONTAINED, status[v] = 0.  A delete with a value length or a
 * chunk, and an op byte above KDB_OP_DELETE, is refused as a put that fails
 * is: status[v] = -1, entry_len[v] = 0, the other items unaffected.  A batch
 * of deletes alone takes nparts = 0, raw_bytes = 0 and values = NULL.
 * kdb_put_entries_batch(...) is kdb_put_ops_batch(stream, NULL, 0, ...). */
int kdb_put_ops_batch(void* stream, const uint8_t* op, uint32_t flags, const uint8_t* keys,
                      const uint64_t* key_off, const uint32_t* key_len, const uint8_t* values,
                      const uint64_t* value_off, const uint64_t* value_len, const uint32_t* part_first,
                      const uint32_t* chunk_len, uint32_t nparts, uint32_t max_chunk, uint32_t n, uint32_t hash_type,
                      uint8_t* scratch, uint64_t scratch_bytes, uint64_t raw_bytes, uint8_t* entries,
                      uint64_t* entry_off, uint32_t* entry_len, uint64_t* total, uint64_t* hashed, uint32_t* crc,
                      uint32_t* kind, int32_t* status);

#ifdef __cplusplus
}
#endif

#endif /* KDB_OPS_H_ */
