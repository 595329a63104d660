// tests/cpp/index_decode_main.cc -- csrc/hstable_decode.h on the host, as a
// stand-alone program for AddressSanitizer / UBSan (tests/test_index_model.py
// compiles and runs it): the decode, validity check and key compare the lookup
// kernel runs per candidate, and the offset-array rows, over files and
// candidate offsets read from a dump.  Every file and key sits in a heap block
// of exactly its size, so a read outside it is a sanitizer report.
//
//   index_decode_main <dump>
// dump:   u32 nfiles, nfiles x (u64 size, bytes),
//         u32 ncases, ncases x (u32 file, u64 offset, u32 verify, u32 key_len, key bytes)
// prints: "file <i> <footer ok> <num_entries> <rows ok> <xor of hashes> <sum of offsets>"
//         "case <i> <rc> <size_header> <flags> <size_key> <size_value> <svc> <padding> <hash> <key equal>"
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../kingdb_amd/csrc/hstable_decode.h"

namespace hs = kdb_hstable;

struct Block {
  uint8_t* p = nullptr;
  uint64_t n = 0;
};

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static bool read_block(FILE* f, uint64_t n, Block* b) {
  b->n = n;
  b->p = static_cast<uint8_t*>(malloc(n ? n : 1));
  return b->p && rd(f, b->p, n);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t nfiles = 0, ncases = 0;
  if (!rd(f, &nfiles, 4)) return 2;
  std::vector<Block> files(nfiles);
  for (uint32_t i = 0; i < nfiles; i++) {
    uint64_t n;
    if (!rd(f, &n, 8) || !read_block(f, n, &files[i])) return 2;
  }
  for (uint32_t i = 0; i < nfiles; i++) {
    const Block& b = files[i];
    hs::Footer ft{};
    const bool ok = hs::decode_footer(b.p, b.n, &ft);
    bool rows_ok = ok;
    uint64_t x = 0, s = 0;
    if (ok) {
      uint64_t at = ft.offset_indexes;
      const uint64_t end = b.n - hs::kFooterSize;
      for (uint64_t r = 0; r < ft.num_entries; r++) {
        uint64_t h;
        uint32_t o;
        const int len = at <= end ? hs::decode_row(b.p + at, end - at, &h, &o) : -1;
        if (len < 0) {
          rows_ok = false;
          break;
        }
        x ^= h;
        s += o;
        at += (uint64_t)len;
      }
    }
    printf("file %u %d %" PRIu64 " %d %" PRIu64 " %" PRIu64 "\n", i, ok ? 1 : 0, ok ? ft.num_entries : 0,
           rows_ok ? 1 : 0, rows_ok ? x : 0, rows_ok ? s : 0);
  }
  if (!rd(f, &ncases, 4)) return 2;
  for (uint32_t i = 0; i < ncases; i++) {
    uint32_t file, verify, klen;
    uint64_t offset;
    Block key;
    if (!rd(f, &file, 4) || !rd(f, &offset, 8) || !rd(f, &verify, 4) || !rd(f, &klen, 4) ||
        !read_block(f, klen, &key) || file >= nfiles)
      return 2;
    const Block& b = files[file];
    hs::EntryHeader h{};
    const int rc = hs::locate_entry(b.p, b.n, offset, verify != 0, &h);
    const bool eq = rc == hs::kDecodeOk && hs::key_equal(b.p, offset, h, key.p, key.n);
    if (rc == hs::kDecodeError)
      printf("case %u %d\n", i, rc);
    else
      printf("case %u %d %u %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %d\n", i, rc,
             h.size_header, h.flags, h.size_key, h.size_value, h.size_value_compressed, h.size_padding, h.hash,
             eq ? 1 : 0);
    free(key.p);
  }
  for (Block& b : files) free(b.p);
  fclose(f);
  return 0;
}
