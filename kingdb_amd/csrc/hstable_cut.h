// kingdb_amd/csrc/hstable_cut.h -- where a batch of entries is cut into HSTable
// files, for the device writer (hstable_dev.hip) and for the host
// (tests/cpp/hstable_cut_main.cc): plain inline functions, no HIP runtime, the
// same text for hipcc and g++.
//
// The rule is append_loop's (hstable.cc), itself WriteOrdersAndFlushFile /
// FlushCurrentFile.  sb = hstable_size, fsize = the open file's length so far;
// for the entries in order:
//   * status != 0: skipped, no row and no bytes;
//   * before an entry, a file open with fsize > sb is closed;
//   * no file open: one is opened, fsize = 8192;
//   * fsize > 0xFFFFFFFF before an entry is an error;
//   * the entry's row is (hashed, fsize); fsize += entry_len;
//   * kind != 0 sets the file's padding flag, kind == 2 marks it incomplete
//     (no offset array), and after such an entry fsize >= sb closes the file;
//   * after the batch's last entry, a file open with fsize >= sb is closed.
//
// Walked entry by entry that is a chain of n dependent loads.  Here it is
// walked file by file over four exclusive prefix arrays of n + 1 entries each,
// which parallel kernels prepare:
//   P   effective lengths (status == 0 ? entry_len : 0)
//   CV  valid entries      (status == 0)
//   CM  marked entries     (status == 0 && kind != 0)
//   C2  unfinished entries (status == 0 && kind == 2)
// (CM stands in for a compacted list of the marked indices: "the first marked
// index >= k" is one binary search in it.)  The file that holds valid entry v
// at offset fs ends
//   * after the first marked k in [v, j) with fs + P[k+1] - P[v] >= sb, or else
//   * before j, the first index with fs + P[j] - P[v] > sb, or else
//   * at n, closed there iff its fsize reached sb exactly,
// each a binary search, so the chain has as many steps as files touched.  A
// leading run of skipped entries, a batch of only skipped entries, n = 0 and a
// file carried in from the previous batch all take the same steps.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KDB_CUT_HD __host__ __device__ inline
#else
#define KDB_CUT_HD inline
#endif

namespace kdb_hstable_cut {

constexpr uint64_t kHeaderBlock = 8192;          // internal__hstable_header_size
constexpr uint64_t kMaxOffset = 0xFFFFFFFFull;   // entry offsets are 32-bit (OffsetArrayRow)

constexpr uint32_t kOpened = 1;       // the file is opened by this batch
constexpr uint32_t kCloses = 2;       // and/or closed by it
constexpr uint32_t kPadding = 4;      // HSTableFooter flags: some entry had kind != 0
constexpr uint32_t kIncomplete = 8;   // some entry had kind == 2: no offset array
constexpr uint32_t kOverflow = 16;    // an entry of it would start past kMaxOffset: the batch is refused

// The open file between batches.
struct State {
  uint64_t fsize;
  uint32_t open, padding, incomplete, pad;
};

struct Prefix {
  const uint64_t* P;
  const uint64_t* CV;
  const uint64_t* CM;
  const uint64_t* C2;
  uint32_t n;
};

// One file touched by the batch: its entries are the valid ones of
// [first, first + count); entry i of them lies at fs + P[i] - P[first].
struct FileRec {
  uint32_t first, count;
  uint64_t fs;          // fsize before entry `first`
  uint64_t fs_end;      // and after the last
  uint32_t nvalid;      // rows this batch adds
  uint32_t flags;
  uint64_t row_bytes;   // their encoded length (filled in after the cut; 0 for an incomplete file)
};

// The first index in [lo, hi] with a[index] > x, hi + 1 if none (a ascends).
KDB_CUT_HD uint32_t first_above(const uint64_t* a, uint32_t lo, uint32_t hi, uint64_t x) {
  uint32_t l = lo, r = hi + 1u;
  while (l < r) {
    const uint32_t m = l + (r - l) / 2u;
    if (a[m] > x) r = m;
    else l = m + 1u;
  }
  return l;
}

KDB_CUT_HD uint64_t sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }

// The first i >= from with entry i counted by the prefix c (c[i+1] > c[i]), n if none.
KDB_CUT_HD uint32_t first_counted(const uint64_t* c, uint32_t n, uint32_t from) {
  if (from >= n) return n;
  return first_above(c, from + 1u, n, c[from]) - 1u;      // n + 1 - 1 if none
}

// The file that is open with `st` before valid entry v (v == n: no valid
// entry is left).  Returns its record; *end = the index its walk stops at.
KDB_CUT_HD FileRec file_end(const Prefix& A, uint64_t sb, uint32_t v, const State& st, uint32_t* end_out) {
  const uint32_t n = A.n;
  const uint64_t fs = st.fsize, pv = A.P[v];
  FileRec r{v, 0, fs, fs, 0, 0, 0};
  // j: the first index with fsize before it > sb (n + 1: not even after the last entry)
  const uint32_t j = fs > sb ? v : first_above(A.P, v, n, sat_add(pv, sb - fs));
  const uint32_t stop = j < n ? j : n;
  uint32_t end = stop;
  bool closes = j <= n;
  if (v < stop) {
    // k0: the first entry after which fsize >= sb; k: the first marked one from there
    const uint32_t k0 = fs >= sb ? v : first_above(A.P, v + 1u, n, sat_add(pv, sb - fs) - 1u) - 1u;
    const uint32_t k = first_counted(A.CM, n, k0);
    if (k < stop) {
      end = k + 1u;
      closes = true;
    }
  }
  const uint64_t fe = fs + (A.P[end] - pv);
  if (!closes && fe >= sb) closes = true;                 // the end of the batch
  r.count = end - v;
  r.fs_end = fe;
  r.nvalid = (uint32_t)(A.CV[end] - A.CV[v]);
  uint32_t flags = closes ? kCloses : 0u;
  if (st.padding || A.CM[end] > A.CM[v]) flags |= kPadding;
  if (st.incomplete || A.C2[end] > A.C2[v]) flags |= kIncomplete;
  if (r.nvalid) {
    // offsets ascend: the last valid entry's is the largest
    const uint32_t lv = first_above(A.CV, v + 1u, end, A.CV[end] - 1u) - 1u;
    if (fs + (A.P[lv] - pv) > kMaxOffset) flags |= kOverflow;
  }
  r.flags = flags;
  *end_out = end;
  return r;
}

// The chain over one batch.  emit(rec) is called for every file touched, in
// order (at most one of them without kCloses, the last).  Returns false, with
// *st unchanged, where a record carries kOverflow (it is emitted last) or emit
// returns false (no room for the record).
template <class Emit>
KDB_CUT_HD bool plan_batch(const Prefix& A, uint64_t sb, State* st, Emit emit) {
  State s = *st;
  uint32_t i = 0;
  for (;;) {
    const uint32_t v = first_counted(A.CV, A.n, i);
    if (v == A.n && !s.open) break;
    bool opened = false;
    if (!s.open) {
      s = State{kHeaderBlock, 1u, 0u, 0u, 0u};
      opened = true;
    }
    uint32_t end = v;
    FileRec r = file_end(A, sb, v, s, &end);
    if (opened) r.flags |= kOpened;
    const bool closes = (r.flags & kCloses) != 0;
    if (v == A.n && !closes) break;                       // the carried file, untouched
    if (!emit(r) || (r.flags & kOverflow)) return false;
    if (closes) {
      s = State{0, 0u, 0u, 0u, 0u};
    } else {
      s.fsize = r.fs_end;
      s.padding = (r.flags & kPadding) != 0;
      s.incomplete = (r.flags & kIncomplete) != 0;
    }
    i = end;
    if (!closes || v == A.n) break;
  }
  *st = s;
  return true;
}

// Length of v as a varint: 1..10 bytes.
KDB_CUT_HD uint32_t varint_len(uint64_t v) {
  return (70u - (uint32_t)__builtin_clzll(v | 1u)) / 7u;
}

// Writes v as a varint through put(k, byte), k = 0 .. len - 1; returns len.
template <class Put>
KDB_CUT_HD uint32_t put_varint(uint64_t v, Put put) {
  uint32_t k = 0;
  while (v >= 128u) {
    put(k++, (uint8_t)(v | 128u));
    v >>= 7;
  }
  put(k++, (uint8_t)v);
  return k;
}

}  // namespace kdb_hstable_cut
