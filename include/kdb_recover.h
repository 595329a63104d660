/* include/kdb_recover.h -- HSTable files that have no usable footer, recovered
 * on the device (csrc/recover.hip): what HSTableManager::RecoverFile
 * (storage/hstable_manager.h:1101-1185) does at Database::Open for a file
 * LoadFile refused -- walk the entries from byte 8192, cut the file where the
 * walk stops, append a fresh offset array and footer -- byte for byte the
 * file the reference leaves on disk.  The rules per entry are
 * csrc/hstable_recover.h; DESIGN.md 4.10 has the kernels.
 *
 * Error codes are include/kdb_put.h's (KDB_PUT_*).
 */
#ifndef KDB_RECOVER_H_
#define KDB_RECOVER_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Per-file status. */
#define KDB_RECOVER_NOENTRY (-6)  /* no entry could be walked: the reference removes the file */
#define KDB_RECOVER_LARGE   (-7)  /* HSTableHeader of large type: RecoverFile gives up and the file is removed */
#define KDB_RECOVER_BADHEADER (-8) /* no byte behind the header block, or a header that does not decode:
                                     LoadDatabase skips such a file before LoadFile and leaves it on disk as
                                     it is (hstable_manager.h:1000-1005); so does this call */

/* Which bytes an uncompacted entry's checksum_content is compared with. */
#define KDB_RECOVER_REFERENCE 0   /* RecoverFile's range, header bytes [5, size_header) first: never matches,
                                     so every multipart entry is dropped, as the reference drops it */
#define KDB_RECOVER_CONTENT   1   /* key || value[0, size_value_used): what the put computed and Get verifies */

struct kdb_recover_report {
  uint64_t entries_walked;        /* entries the walk accepted, valid or not */
  uint64_t rows_kept;             /* rows of the new offset array */
  uint64_t entries_invalid;       /* walked - kept */
  uint64_t offset;                /* where the walk stopped: the new offset_indexes */
  uint32_t footer_flags;          /* 0x1 padding in values, 0x2 invalid entries */
  uint32_t chain_loads;           /* dependent global loads of the sequential part for this file: groups of 32
                                     tiles touched, plus single tiles where an entry longer than a tile carried
                                     the chain behind a group's first tile; never more than the tiles touched */
};

/* Bytes a file's slot must hold for the recovered file: file_size, a 15-byte
 * row per 26 bytes behind the header block, the footer; a multiple of 64. */
uint64_t kdb_hstable_recover_bound(uint64_t file_size);
/* Device scratch bytes kdb_hstable_recover_files needs for these files: four
 * bytes per byte behind the header block, plus the entry lists. */
uint64_t kdb_hstable_recover_scratch_bytes(const uint64_t* file_size, uint32_t nfiles);

/* Recovers every file it is given, in place.  Synchronous; host arrays, like
 * kdb_index_load_files.  File f is d_files[file_off[f] .. + file_size[f]) and
 * owns file_cap[f] bytes from file_off[f] (file_off a multiple of 4).
 * status[f] == 0: new_size[f] bytes at the slot are the recovered file; else
 * KDB_RECOVER_NOENTRY / KDB_RECOVER_LARGE / KDB_RECOVER_BADHEADER, the slot
 * unchanged, new_size[f] = 0.
 * report may be NULL.  KDB_PUT_EINVAL before any launch: file_cap[f] below
 * kdb_hstable_recover_bound(file_size[f]), a file of 0xFFFFFF00 bytes or more,
 * crc_scope neither of the two, scratch_bytes too small.  No allocation on the
 * stream beyond the scan's. */
int kdb_hstable_recover_files(void* stream, uint8_t* d_files, const uint64_t* file_off, const uint64_t* file_size,
                              const uint64_t* file_cap, uint32_t nfiles, uint32_t crc_scope, void* d_scratch,
                              uint64_t scratch_bytes, uint64_t* new_size, int32_t* status,
                              struct kdb_recover_report* report);

/* The same call; with ms != NULL it also records HIP events on the stream
 * between its parts and writes their milliseconds: speculate + resolve, hop +
 * chain + fill, list, content CRC, emit, all.  For tools/bench_recover.py;
 * kdb_hstable_recover_files creates no event. */
int kdb_hstable_recover_files_timed(void* stream, uint8_t* d_files, const uint64_t* file_off,
                                    const uint64_t* file_size, const uint64_t* file_cap, uint32_t nfiles,
                                    uint32_t crc_scope, void* d_scratch, uint64_t scratch_bytes, uint64_t* new_size,
                                    int32_t* status, struct kdb_recover_report* report, float* ms);

#ifdef __cplusplus
}
#endif

#endif /* KDB_RECOVER_H_ */
