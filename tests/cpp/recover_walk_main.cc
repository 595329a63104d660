// tests/cpp/recover_walk_main.cc -- csrc/hstable_recover.h on the host, as a
// stand-alone program: the sequential recovery walk, entry after entry, and
// the file it leaves (truncated, fresh offset array, footer: the encoders of
// csrc/hstable_close.h that the kernels use, on the host).  Built under
// AddressSanitizer / UBSan by tests/test_recover_model.py, and -O2 without
// them as the one-thread baseline of tools/bench_recover.py.  Every file sits
// in a heap block of exactly its size, so a read outside it is a sanitizer
// report.
//
//   recover_walk_main <dump> [repeats]
// dump:   u32 scope, u32 nfiles, nfiles x (u64 size, bytes)
// prints: "file <i> <status> <new size> <crc32c of the new file> <walked> <kept> <invalid> <offset> <flags>"
//         status 0 recovered, -6 nothing to save, -7 large type, -8 no usable header
//         with repeats: "time_us <min> <median>" of recovering all files again, repeats times
#include <algorithm>
#include <chrono>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../kingdb_amd/csrc/hstable_close.h"
#include "../../kingdb_amd/csrc/hstable_recover.h"

namespace hs = kdb_hstable;
namespace hsc = kdb_hstable_close;

static uint32_t g_table[8][256];

static void crc_init() {
  for (uint32_t i = 0; i < 256; i++) {
    uint32_t v = i;
    for (int k = 0; k < 8; k++) v = (v >> 1) ^ (0x82F63B78u & (0u - (v & 1u)));
    g_table[0][i] = v;
  }
  for (int k = 1; k < 8; k++)
    for (uint32_t i = 0; i < 256; i++) g_table[k][i] = (g_table[k - 1][i] >> 8) ^ g_table[0][g_table[k - 1][i] & 0xffu];
}

// crc32c::Extend, slice-by-8 as the reference's software path (crc32c.cc:296-340)
static uint32_t crc32c(uint32_t init, const uint8_t* p, uint64_t n) {
  uint32_t c = init ^ 0xFFFFFFFFu;
  while (n >= 8) {
    uint32_t lo, hi;
    memcpy(&lo, p, 4);
    memcpy(&hi, p + 4, 4);
    lo ^= c;
    c = g_table[7][lo & 0xffu] ^ g_table[6][(lo >> 8) & 0xffu] ^ g_table[5][(lo >> 16) & 0xffu] ^ g_table[4][lo >> 24] ^
        g_table[3][hi & 0xffu] ^ g_table[2][(hi >> 8) & 0xffu] ^ g_table[1][(hi >> 16) & 0xffu] ^ g_table[0][hi >> 24];
    p += 8;
    n -= 8;
  }
  while (n--) c = g_table[0][(c ^ *p++) & 0xffu] ^ (c >> 8);
  return c ^ 0xFFFFFFFFu;
}

struct Result {
  int status = 0;
  uint64_t walked = 0, kept = 0, offset = 0;
  uint32_t flags = 0;
  std::vector<uint8_t> tail;     // the offset array and the footer
};

static Result recover(const uint8_t* p, uint64_t n, uint32_t scope) {
  Result r;
  hs::FileHeader fh;
  if (n <= hs::kHeaderBlock || !hs::decode_file_header(p, n, &fh) || crc32c(0, p + 4, 20) != fh.crc32) {
    r.status = -8;
    return r;
  }
  if (fh.filetype & hs::kCompactedLargeType) {
    r.status = -7;
    return r;
  }
  bool padding = false;
  r.offset = hs::recover_walk(
      p, n, scope, [](const uint8_t* q, uint64_t len) { return crc32c(0, q, len); },
      [&](uint64_t offset, const hs::EntryHeader& h, bool kept) {
        r.walked++;
        if (h.flags & hs::kHasPadding) padding = true;
        if (!kept) return;
        r.kept++;
        const size_t at = r.tail.size();
        const uint32_t rl = hsc::row_len(h.hash, (uint32_t)offset);
        r.tail.resize(at + rl);
        hsc::put_row(h.hash, (uint32_t)offset, rl, [&](uint32_t k, uint8_t byte) { r.tail[at + k] = byte; });
      });
  r.flags = (padding ? hs::kFooterHasPadding : 0u) | (r.kept < r.walked ? hs::kFooterHasInvalid : 0u);
  if (r.offset <= hs::kHeaderBlock) {
    r.status = -6;
    r.tail.clear();
    return r;
  }
  // the footer: its first 32 bytes, then the CRC of the rows extended over them
  const size_t rows = r.tail.size();
  r.tail.resize(rows + hs::kFooterSize);
  uint8_t* ft = r.tail.data() + rows;
  hsc::encode_footer(hs::recover_filetype(fh.filetype), r.flags, r.offset, r.kept, ft);
  const uint32_t c = crc32c(0, r.tail.data(), rows + hsc::kFooterCrcBytes);
  for (uint32_t i = 0; i < 4; i++) ft[hsc::kFooterCrcBytes + i] = (uint8_t)(c >> (8 * i));
  return r;
}

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  crc_init();
  uint32_t scope = 0, nfiles = 0;
  if (!rd(f, &scope, 4) || !rd(f, &nfiles, 4) || scope > 1) return 2;
  std::vector<uint8_t*> files(nfiles);
  std::vector<uint64_t> sizes(nfiles);
  for (uint32_t i = 0; i < nfiles; i++) {
    if (!rd(f, &sizes[i], 8)) return 2;
    files[i] = static_cast<uint8_t*>(malloc(sizes[i] ? sizes[i] : 1));
    if (!files[i] || !rd(f, files[i], sizes[i])) return 2;
  }
  fclose(f);
  for (uint32_t i = 0; i < nfiles; i++) {
    const Result r = recover(files[i], sizes[i], scope);
    uint64_t size = 0;
    uint32_t crc = 0;
    if (r.status == 0) {
      size = r.offset + r.tail.size();
      crc = crc32c(crc32c(0, files[i], r.offset), r.tail.data(), r.tail.size());
      if (size > hs::recover_bound(sizes[i])) return 3;
    }
    printf("file %u %d %" PRIu64 " %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u\n", i, r.status, size, crc,
           r.walked, r.kept, r.walked - r.kept, r.offset, r.flags);
  }
  const int repeats = argc > 2 ? atoi(argv[2]) : 0;
  if (repeats > 0) {
    std::vector<double> us;
    uint64_t sink = 0;
    for (int k = 0; k < repeats; k++) {
      const auto t0 = std::chrono::steady_clock::now();
      for (uint32_t i = 0; i < nfiles; i++) sink += recover(files[i], sizes[i], scope).tail.size();
      us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(us.begin(), us.end());
    printf("time_us %.1f %.1f %" PRIu64 "\n", us[0], us[us.size() / 2], sink);
  }
  for (uint8_t* p : files) free(p);
  return 0;
}
