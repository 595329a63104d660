// tests/cpp/tail_rows_main.cc -- csrc/index_rows.h on the host, under
// AddressSanitizer and UBSan (tests/test_index_tail_model.py builds and runs
// it): rows encoded with put_row (csrc/hstable_close.h) into a staging that is
// stored backwards, as the device writer stages the rows of its open file, and
// decoded back through the reversed addressing the way index_parse_kernel<true>
// does it, a byte at a time: a terminator's rank among the terminators is its
// varint's number, the owner walks back to the varint's first byte.  Every
// range is parsed out of a heap block of exactly its size, so a read outside
// it on either side is a sanitizer error.  Prints "ok <rows> <cases>" and
// exits 0, or the first difference and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../kingdb_amd/csrc/hstable_close.h"
#include "../../kingdb_amd/csrc/index_rows.h"

namespace hsc = kdb_hstable_close;
namespace ir = kdb_index_rows;

namespace {

struct Row {
  uint64_t hash;
  uint32_t off;
  bool operator==(const Row& o) const { return hash == o.hash && off == o.off; }
};

uint64_t g_rows = 0, g_cases = 0;
uint64_t g_seed = 0x9E3779B97F4A7C15ull;

uint64_t rnd() {                          // splitmix64
  uint64_t z = (g_seed += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

[[noreturn]] void fail(const char* what, uint64_t a = 0, uint64_t b = 0) {
  std::printf("FAIL %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
  std::exit(1);
}

// The staging's logical bytes: row after row.
std::vector<uint8_t> stage(const std::vector<Row>& rows, std::vector<uint64_t>* ends = nullptr) {
  std::vector<uint8_t> out;
  for (const Row& r : rows) {
    const uint32_t rl = hsc::row_len(r.hash, r.off);
    const size_t at = out.size();
    out.resize(at + rl);
    hsc::put_row(r.hash, r.off, rl, [&](uint32_t k, uint8_t byte) { out[at + k] = byte; });
    if (ends) ends->push_back(out.size());
  }
  return out;
}

// kdb_index_set_tail's check of the record and the parse of logical bytes
// [lo, hi) into rows [held_rows, rows): false where it refuses.  The bytes
// are read from a block of hi - lo bytes that holds them backwards.
bool parse(const std::vector<uint8_t>& logical, uint64_t lo, uint64_t hi, uint64_t held_rows, uint64_t rows,
           std::vector<Row>* out) {
  if (hi > logical.size()) fail("test range", hi, logical.size());
  if (!ir::tail_range_ok(held_rows, lo, rows, hi, hi ? hi - 1u : 0u)) return false;
  const uint64_t len = hi - lo, nvar = 2u * (rows - held_rows);
  if (nvar == 0) return true;             // tail_range_ok: no bytes either
  uint8_t* block = static_cast<uint8_t*>(std::malloc(len));
  if (!block) fail("malloc");
  for (uint64_t p = 0; p < len; p++) block[len - 1u - p] = logical[lo + p];
  const ir::Reversed reg{block + len - 1u};
  bool malformed = false;
  uint64_t k = 0;
  out->resize(rows);
  for (uint64_t pos = 0; pos < len; pos++) {
    if (!ir::is_terminator(reg[pos])) continue;
    if (k < nvar) {
      const bool is_offset = (k & 1u) != 0;
      uint64_t v = 0;
      if (!ir::varint_ending_at(reg, pos, is_offset, &v)) {
        malformed = true;
      } else if (is_offset) {
        (*out)[held_rows + (k >> 1)].off = (uint32_t)v;
      } else {
        (*out)[held_rows + (k >> 1)].hash = v;
      }
    }
    k++;
  }
  if (k != nvar || !ir::is_terminator(reg[len - 1u])) malformed = true;
  std::free(block);
  return !malformed;
}

void round_trip(const std::vector<Row>& rows, const char* what) {
  const std::vector<uint8_t> bytes = stage(rows);
  std::vector<Row> got;
  if (!parse(bytes, 0, bytes.size(), 0, rows.size(), &got)) fail(what, rows.size(), bytes.size());
  got.resize(rows.size());
  if (!(got == rows)) fail(what, rows.size(), 1);
  g_rows += rows.size();
  g_cases++;
}

void refused(const std::vector<uint8_t>& bytes, uint64_t lo, uint64_t hi, uint64_t held_rows, uint64_t rows,
             const char* what) {
  std::vector<Row> got;
  if (parse(bytes, lo, hi, held_rows, rows, &got)) fail(what, hi, rows);
  g_cases++;
}

Row random_row() {
  // every varint length: a hash of 1..64 significant bits, an offset of 1..32
  const uint64_t h = rnd() >> (rnd() % 64u);
  const uint32_t o = (uint32_t)(rnd() >> 32) >> (rnd() % 32u);
  return Row{h, o};
}

}  // namespace

int main() {
  // hashes of every varint length 1..10 with offsets of every length 1..5, the smallest and the largest of each
  for (uint32_t hl = 1; hl <= 10; hl++)
    for (uint32_t ol = 1; ol <= 5; ol++) {
      const uint64_t hmin = hl == 1 ? 0 : 1ull << (7u * (hl - 1u));
      const uint64_t hmax = hl == 10 ? ~0ull : (1ull << (7u * hl)) - 1u;
      const uint32_t omin = ol == 1 ? 0 : 1u << (7u * (ol - 1u));
      const uint32_t omax = ol == 5 ? ~0u : (1u << (7u * ol)) - 1u;
      for (uint64_t h : {hmin, hmax})
        for (uint32_t o : {omin, omax}) {
          if (hsc::row_len(h, o) != hl + ol) fail("row_len", hl, ol);
          round_trip({Row{h, o}, Row{h, o}, Row{hmax, omin}}, "lengths");
        }
    }
  // 0, 1 and 2 rows; 21, 22 and 23 rows of 12 bytes (252, 264, 276: both sides of a 256-byte tile's edge); many tiles
  for (uint32_t n : {0u, 1u, 2u, 21u, 22u, 23u}) {
    std::vector<Row> rows;
    for (uint32_t i = 0; i < n; i++)
      rows.push_back(Row{(rnd() | 1ull << 56) & ~(1ull << 63), (uint32_t)(1u << 14 | (rnd() & 0x1FFFFFu))});
    if (stage(rows).size() != 12u * n) fail("twelve-byte rows", n);
    round_trip(rows, "edge counts");
  }
  {
    std::vector<Row> rows;
    for (uint32_t i = 0; i < 5000; i++) rows.push_back(random_row());
    if (stage(rows).size() < 40u * 256u) fail("many tiles");
    round_trip(rows, "many tiles");
  }
  // the incremental form: every split of a stream of 300 rows
  {
    std::vector<Row> rows;
    for (uint32_t i = 0; i < 300; i++) rows.push_back(random_row());
    std::vector<uint64_t> ends;
    const std::vector<uint8_t> bytes = stage(rows, &ends);
    for (uint32_t held = 0; held <= 300; held++) {
      const uint64_t hb = held ? ends[held - 1u] : 0u;
      std::vector<Row> got;
      if (!parse(bytes, 0, hb, 0, held, &got)) fail("split, first part", held);
      if (!parse(bytes, hb, bytes.size(), held, 300, &got)) fail("split, second part", held);
      got.resize(300);
      if (!(got == rows)) fail("split", held);
      // one byte less held: the last terminator of the rows held is one too many
      if (held && held < 300) refused(bytes, hb - 1u, bytes.size(), held, 300, "split inside a row");
      g_rows += 300;
      g_cases++;
    }
    // fewer rows or bytes than held
    refused(bytes, ends[9], ends[4], 10, 5, "shrinks");
    refused(bytes, ends[9], ends[19], 10, 9, "fewer rows");
  }
  // hostile inputs
  {
    const std::vector<Row> rows{Row{0x1234567890ull, 300}, Row{7, 5}, Row{~0ull, 70000}};
    std::vector<uint64_t> ends;
    const std::vector<uint8_t> bytes = stage(rows, &ends);
    const uint64_t all = bytes.size();
    refused(bytes, 0, all - 1u, 0, 3, "row_bytes cut inside a varint");
    refused(bytes, 0, all - 3u, 0, 3, "one terminator too few");
    std::vector<uint8_t> more(bytes);
    more.push_back(0x05);
    refused(more, 0, more.size(), 0, 3, "one terminator too many");
    refused(bytes, 0, all, 0, 2, "a row too many");
    refused(bytes, 0, all, 0, 4, "a row too few");
    // the same counts with the varints where they do not belong: two rows of (2 + 2) bytes claimed, (1 + 3) present
    std::vector<uint8_t> hash11(10, 0x80);
    hash11.push_back(0x01);
    hash11.push_back(0x02);
    refused(hash11, 0, hash11.size(), 0, 1, "an 11-byte hash");
    std::vector<uint8_t> off6{0x01, 0x80, 0x80, 0x80, 0x80, 0x80, 0x01};
    refused(off6, 0, off6.size(), 0, 1, "a 6-byte offset");
    // a 10-byte hash and a 5-byte offset are the longest that pass
    std::vector<Row> got;
    std::vector<uint8_t> longest(9, 0xFF);
    longest.push_back(0x01);
    longest.insert(longest.end(), {0xFF, 0xFF, 0xFF, 0xFF, 0x0F});
    if (!parse(longest, 0, longest.size(), 0, 1, &got) || !(got[0] == Row{~0ull, ~0u})) fail("longest");
    g_cases++;
    // nothing but continuation bytes, and a range that begins with them: the walk back stops at the range's start
    const std::vector<uint8_t> cont(30, 0x80);
    refused(cont, 0, cont.size(), 0, 2, "no terminator");
    std::vector<uint8_t> lead(12, 0x80);
    lead.insert(lead.end(), {0x01, 0x02});
    refused(lead, 0, lead.size(), 0, 1, "twelve continuation bytes");
    // a range that begins inside those bytes is a row of its own (4 + 1 bytes): nothing in front of it is read
    if (!parse(lead, 9, lead.size(), 0, 1, &got) || !(got[0] == Row{1ull << 21, 2})) fail("lead");
    g_cases++;
    std::vector<uint8_t> lead2{0x80, 0x80, 0x01, 0x02};
    if (!parse(lead2, 0, 4, 0, 1, &got) || !(got[0] == Row{1ull << 14, 2})) fail("lead2");
    g_cases++;
    // records the host refuses before a byte is read
    if (ir::tail_range_ok(0, 0, 1, 1, 0)) fail("a row of one byte");
    if (ir::tail_range_ok(0, 0, 1, 16, 15)) fail("a row of sixteen bytes");
    if (ir::tail_range_ok(0, 0, 4, 8, 6)) fail("a staging that begins before the buffer");
    if (ir::tail_range_ok(0, 0, (1ull << 30) + 1u, 4ull << 30, 1ull << 40)) fail("too many rows");
    if (!ir::tail_range_ok(0, 0, 0, 0, 0) || !ir::tail_range_ok(3, 30, 3, 30, 100)) fail("nothing to parse");
    g_cases += 5;
  }
  // the order rule: three loaded files of timestamp 5, 7, 7 and ids 4, 2, 9, and one that did not load
  {
    const uint64_t ts[4] = {5, 7, 9, 7};
    const uint32_t id[4] = {4, 2, 100, 9};
    const int32_t st[4] = {0, 0, -1, 0};
    auto after = [&](uint32_t n, uint64_t t, uint32_t f) { return ir::sorts_after_loaded(ts, id, st, n, t, f); };
    // the newest timestamp again: a smaller, an equal and a larger id
    if (after(4, 7, 8) || after(4, 7, 9) || !after(4, 7, 10)) fail("equal timestamp");
    if (after(4, 6, 1000) || after(4, 5, 5) || !after(4, 8, 0)) fail("older and newer timestamps");
    // the file of timestamp 9 did not load: it is not in the way, with any id
    if (!after(4, 8, 100) || !after(4, 9, 1)) fail("an unloaded file counts");
    // only the files held: the first two, one, none
    if (!after(2, 7, 3) || after(2, 7, 2) || !after(1, 5, 5) || after(1, 5, 4)) fail("files beyond the count");
    if (!after(0, 0, 0) || !ir::sorts_after_loaded(nullptr, nullptr, nullptr, 0, 0, 0)) fail("an empty handle");
    g_cases += 5;
  }
  std::printf("ok %llu %llu\n", (unsigned long long)g_rows, (unsigned long long)g_cases);
  return 0;
}
