// tests/cpp/hstable_cut_main.cc -- csrc/hstable_cut.h on the host, under
// AddressSanitizer and UBSan (tests/test_hstable_cut_model.py builds and runs
// it): the file-by-file chain over the prefix arrays against a straight
// entry-by-entry loop of the rule, over seeded random batches and hand-made
// edge cases.  Prints "ok <batches> <files> <rows>" and exits 0, or the first
// difference and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../kingdb_amd/csrc/hstable_cut.h"

namespace cut = kdb_hstable_cut;

namespace {

struct Batch {
  std::vector<uint32_t> len, kind;
  std::vector<int32_t> status;
};

struct Row {
  uint32_t file;      // ordinal of the file (1 = the first one opened)
  uint64_t off;
  bool operator==(const Row& o) const { return file == o.file && off == o.off; }
};

struct Closed {
  uint32_t file;
  uint64_t fsize, nrows;
  bool padding, incomplete;
  bool operator==(const Closed& o) const {
    return file == o.file && fsize == o.fsize && nrows == o.nrows && padding == o.padding && incomplete == o.incomplete;
  }
};

// What one writer holds between batches, for either walk.
struct Writer {
  cut::State st{0, 0, 0, 0, 0};
  uint32_t fileid = 0;
  uint64_t nrows = 0;
  std::vector<Closed> closed;
  void open() {
    fileid++;
    st = cut::State{cut::kHeaderBlock, 1, 0, 0, 0};
    nrows = 0;
  }
  void close() {
    closed.push_back(Closed{fileid, st.fsize, nrows, st.padding != 0, st.incomplete != 0});
    st = cut::State{0, 0, 0, 0, 0};
    nrows = 0;
  }
};

// The rule, entry by entry.  rows[i].file == 0: no row.
bool walk_loop(Writer& w, uint64_t sb, const Batch& b, std::vector<Row>& rows) {
  const size_t n = b.len.size();
  rows.assign(n, Row{0, 0});
  for (size_t i = 0; i < n; i++) {
    if (b.status[i] != 0) continue;
    if (w.st.open && w.st.fsize > sb) w.close();
    if (!w.st.open) w.open();
    if (w.st.fsize > cut::kMaxOffset) return false;
    rows[i] = Row{w.fileid, w.st.fsize};
    w.nrows++;
    w.st.fsize += b.len[i];
    if (b.kind[i] != 0) {
      w.st.padding = 1;
      if (b.kind[i] == 2) w.st.incomplete = 1;
      if (w.st.fsize >= sb) w.close();
    }
  }
  if (w.st.open && w.st.fsize >= sb) w.close();
  return true;
}

// The same through plan_batch over the prefix arrays.
bool walk_chain(Writer& w, uint64_t sb, const Batch& b, std::vector<Row>& rows) {
  const uint32_t n = (uint32_t)b.len.size();
  std::vector<uint64_t> P(n + 1u, 0), CV(n + 1u, 0), CM(n + 1u, 0), C2(n + 1u, 0);
  for (uint32_t i = 0; i < n; i++) {
    const bool ok = b.status[i] == 0;
    P[i + 1] = P[i] + (ok ? b.len[i] : 0u);
    CV[i + 1] = CV[i] + (ok ? 1u : 0u);
    CM[i + 1] = CM[i] + (ok && b.kind[i] != 0 ? 1u : 0u);
    C2[i + 1] = C2[i] + (ok && b.kind[i] == 2 ? 1u : 0u);
  }
  const cut::Prefix A{P.data(), CV.data(), CM.data(), C2.data(), n};
  std::vector<cut::FileRec> recs;
  cut::State st = w.st;
  const cut::State before = st;
  const bool ok = cut::plan_batch(A, sb, &st, [&](const cut::FileRec& r) {
    recs.push_back(r);
    return true;
  });
  rows.assign(n, Row{0, 0});
  if (!ok) {
    if (st.fsize != before.fsize || st.open != before.open) {
      printf("state changed by a refused batch\n");
      exit(1);
    }
    return false;
  }
  for (const cut::FileRec& r : recs) {
    if (r.flags & cut::kOpened) w.open();
    uint32_t valid = 0;
    for (uint32_t i = r.first; i < r.first + r.count; i++) {
      if (b.status[i] != 0) continue;
      rows[i] = Row{w.fileid, r.fs + (P[i] - P[r.first])};
      valid++;
    }
    if (valid != r.nvalid || w.st.fsize != r.fs) {
      printf("record of file %u: nvalid %u (walked %u), fs %llu (carried %llu)\n", w.fileid, r.nvalid, valid,
             (unsigned long long)r.fs, (unsigned long long)w.st.fsize);
      exit(1);
    }
    w.nrows += valid;
    w.st.fsize = r.fs_end;
    w.st.padding = (r.flags & cut::kPadding) != 0;
    w.st.incomplete = (r.flags & cut::kIncomplete) != 0;
    if (r.flags & cut::kCloses) w.close();
  }
  if (w.st.open != st.open || w.st.fsize != st.fsize || w.st.padding != st.padding ||
      w.st.incomplete != st.incomplete) {
    printf("carried state differs from the records'\n");
    exit(1);
  }
  return true;
}

uint64_t g_batches = 0, g_files = 0, g_rows = 0;

// Runs the batches through both walks on one carried state each; expect_error:
// the last batch must be refused by both.
void run_case(const char* what, uint64_t sb, const std::vector<Batch>& batches, bool expect_error = false) {
  Writer a, c;
  for (size_t k = 0; k < batches.size(); k++) {
    std::vector<Row> ra, rc;
    const bool oka = walk_loop(a, sb, batches[k], ra);
    const bool okc = walk_chain(c, sb, batches[k], rc);
    const bool last = k + 1 == batches.size();
    if (oka != okc || (!oka) != (expect_error && last)) {
      printf("%s: batch %zu: loop %s, chain %s, error expected %d\n", what, k, oka ? "ok" : "refused",
             okc ? "ok" : "refused", (int)(expect_error && last));
      exit(1);
    }
    if (!oka) return;
    for (size_t i = 0; i < ra.size(); i++)
      if (!(ra[i] == rc[i])) {
        printf("%s: batch %zu entry %zu: loop (%u, %llu) chain (%u, %llu)\n", what, k, i, ra[i].file,
               (unsigned long long)ra[i].off, rc[i].file, (unsigned long long)rc[i].off);
        exit(1);
      }
    if (a.st.open != c.st.open || a.st.fsize != c.st.fsize || a.st.padding != c.st.padding ||
        a.st.incomplete != c.st.incomplete || a.fileid != c.fileid || a.nrows != c.nrows) {
      printf("%s: batch %zu: carried state differs (fsize %llu / %llu, open %u / %u)\n", what, k,
             (unsigned long long)a.st.fsize, (unsigned long long)c.st.fsize, a.st.open, c.st.open);
      exit(1);
    }
    if (a.closed.size() != c.closed.size()) {
      printf("%s: batch %zu: %zu files closed by the loop, %zu by the chain\n", what, k, a.closed.size(),
             c.closed.size());
      exit(1);
    }
    for (size_t f = 0; f < a.closed.size(); f++)
      if (!(a.closed[f] == c.closed[f])) {
        printf("%s: batch %zu: closed file %zu differs\n", what, k, f);
        exit(1);
      }
    g_batches++;
    for (const Row& r : ra) g_rows += r.file != 0;
  }
  g_files += a.closed.size();
}

struct Rng {
  uint64_t s;
  uint64_t next() {                       // splitmix64
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  uint64_t range(uint64_t lo, uint64_t hi) { return lo + next() % (hi - lo + 1); }
};

Batch make(std::initializer_list<uint32_t> len) {
  Batch b;
  for (uint32_t l : len) {
    b.len.push_back(l);
    b.kind.push_back(0);
    b.status.push_back(0);
  }
  return b;
}

}  // namespace

int main() {
  // seeded random batches
  Rng rng{20260801};
  for (int round = 0; round < 1500; round++) {
    const uint64_t sb = round % 3 == 0 ? rng.range(8193, 9000) : rng.range(8193, 1u << 20);
    const int nb = (int)rng.range(1, 5);
    std::vector<Batch> batches;
    for (int k = 0; k < nb; k++) {
      Batch b;
      const uint32_t n = (uint32_t)rng.range(0, round % 5 == 0 ? 400 : 60);
      const uint64_t small = rng.range(0, 3);   // 0: any length; else mostly small ones
      for (uint32_t i = 0; i < n; i++) {
        const uint64_t r = rng.range(0, 99);
        if (r < 8) {                            // a failed put
          b.len.push_back(0);
          b.kind.push_back((uint32_t)rng.range(0, 2));
          b.status.push_back(-1);
          continue;
        }
        b.len.push_back((uint32_t)(small && rng.range(0, 9) ? rng.range(26, 400) : rng.range(26, 70000)));
        b.kind.push_back(r < 14 ? 1u : r < 17 ? 2u : 0u);
        b.status.push_back(0);
      }
      batches.push_back(b);
    }
    run_case("random", sb, batches);
  }

  const uint64_t sb = 16384;
  // fsize == sb exactly at the end of a batch: closed there, the next batch opens a file
  run_case("end of batch at sb", sb, {make({4096, 4096}), make({100, 200})});
  // fsize == sb before an entry (inside a batch): the entry still goes in, the file closes after the batch
  run_case("sb before an entry", sb, {make({8192, 50, 60})});
  run_case("sb before an entry, next batch", sb, {make({8000}), make({192, 50}), make({60})});
  // one past: closed before the next entry
  run_case("past sb", sb, {make({8193, 50, 60})});
  {
    // a kind = 1 entry ending exactly at sb, and one ending short of it
    Batch b = make({4096, 4096, 70, 80});
    b.kind[1] = 1;
    run_case("kind 1 at sb", sb, {b});
    Batch c = make({4096, 4095, 70, 80});
    c.kind[1] = 1;
    run_case("kind 1 short of sb", sb, {c, make({1, 1, 1})});
    Batch d = make({100, 9000, 70});
    d.kind[1] = 2;
    run_case("kind 2 past sb", sb, {d, make({30})});
    Batch e = make({100, 200, 70});
    e.kind[0] = 2;
    run_case("kind 2 stays open", sb, {e, make({30}), make({8192})});
  }
  run_case("n = 0", sb, {make({})});
  run_case("n = 0 with a carried file", sb, {make({100}), make({}), make({8092}), make({})});
  {
    Batch f = make({0, 0, 0, 0});
    f.status = {-1, -1, -1, -1};
    f.kind = {0, 1, 2, 0};
    run_case("only failed puts", sb, {f});
    run_case("only failed puts, carried file", sb, {make({300}), f, make({9000}), f});
    Batch g = make({0, 0, 500, 0, 8000, 0, 40});
    g.status = {-1, -1, 0, -1, 0, -1, 0};
    run_case("leading and trailing failed puts", sb, {g, g});
  }
  {
    // an entry that takes fsize past 2^32: the entry after it is refused
    const uint64_t big = 1ull << 33;
    run_case("offset past 2^32", big, {make({0xFFFFFFFFu, 100})}, true);
    run_case("offset past 2^32, carried", big, {make({0xFFFFFF00u}), make({0xFFFFu, 50})}, true);
    run_case("offset past 2^32 in one batch", big, {make({0xFFFFFFF0u, 0xFFFFu, 7})}, true);
    // exactly 2^32 - 1 is still an offset
    run_case("offset 2^32 - 1", big, {make({0xFFFFFFFFu - 8192u, 100, 5})}, true);
    run_case("offset 2^32 - 1, last entry", big, {make({0xFFFFFFFFu - 8192u, 100})});
    // hstable_size near 2^64: nothing wraps
    run_case("huge hstable_size", ~0ull, {make({70000, 1, 2}), make({3})});
  }
  printf("ok %llu %llu %llu\n", (unsigned long long)g_batches, (unsigned long long)g_files,
         (unsigned long long)g_rows);
  return 0;
}
