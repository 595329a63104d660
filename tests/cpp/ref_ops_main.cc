// tests/cpp/ref_ops_main.cc -- TEST INFRASTRUCTURE ONLY: the driver behind
// tests/golden/make_golden_deletes.py.  Compiled by that script into
// oracle/_ref/ref_ops (git-ignored) against the objects `make -C oracle ref`
// leaves in oracle/_ref/obj/, which are compiled from the reference in place;
// no reference source is copied here.
//
// Drives the reference's own Database with a stream of puts AND deletes
// (oracle/ref_db.cc knows puts only), and reads a database back through
// Database::Get with the status CODE of every key, which is what tells a
// delete entry (kDeleteOrder) from a key that was never written (kNotFound).
//
//   ref_ops <dbdir> <ops.bin> [maximum_part_size [hstable_size [hash]]]
//       opens the database, issues the ops in order from one thread, closes it
//       (hash: 0 MurmurHash3-64, 1 xxHash-64)
//   ref_ops --get <dbdir> <ops.bin> <out.bin>
//       opens the database (its options come from its db_options file; a
//       file without a usable footer is recovered by the open), and for every
//       distinct key of ops.bin, in order of first appearance, appends to
//       out.bin:  u32 key_len, key, i32 code, u64 value_len, value
//       code: 0 OK, 1 NotFound, 2 DeleteOrder, 3 InvalidArgument, 4 IOError,
//       5 Done, 6 MultipartRequired (util/status.h's enum, read through the
//       Is*() predicates); the value is present for code 0 only
//
// ops.bin: ref_db's records,
//   u32 key_len, key, u64 size_value, u32 nchunks, nchunks x (u32 chunk_len, chunk)
// each chunk handed to Database::PutPart(key, chunk, offset, size_value) in
// order; a record with size_value = 2^64 - 1 and nchunks = 0 is
// Database::Delete(key).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "interface/database.h"
#include "util/byte_array.h"
#include "util/status.h"

static const uint64_t kDeleteMark = ~(uint64_t)0;

struct Op {
  std::string key;
  uint64_t size_value;
  std::vector<std::string> chunks;
};

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static bool read_ops(const char* path, std::vector<Op>* ops) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  for (;;) {
    uint32_t klen, nchunks;
    if (fread(&klen, 4, 1, f) != 1) break;
    Op op;
    op.key.assign(klen, '\0');
    if (!rd(f, &op.key[0], klen) || !rd(f, &op.size_value, 8) || !rd(f, &nchunks, 4)) return false;
    if (op.size_value == kDeleteMark && nchunks != 0) return false;
    for (uint32_t c = 0; c < nchunks; c++) {
      uint32_t clen;
      if (!rd(f, &clen, 4)) return false;
      std::string buf(clen, '\0');
      if (!rd(f, &buf[0], clen)) return false;
      op.chunks.push_back(buf);
    }
    ops->push_back(op);
  }
  fclose(f);
  return true;
}

static int code_of(const kdb::Status& s) {
  if (s.IsOK()) return 0;
  if (s.IsNotFound()) return 1;
  if (s.IsDeleteOrder()) return 2;
  if (s.IsInvalidArgument()) return 3;
  if (s.IsIOError()) return 4;
  if (s.IsDone()) return 5;
  if (s.IsMultipartRequired()) return 6;
  return -1;
}

static int get_all(int argc, char** argv) {
  std::vector<Op> ops;
  if (!read_ops(argv[3], &ops)) return 2;
  kdb::DatabaseOptions options;
  kdb::Database db(options, argv[2]);
  kdb::Status s = db.Open();
  if (!s.IsOK()) {
    fprintf(stderr, "open: %s\n", s.ToString().c_str());
    return 1;
  }
  FILE* out = fopen(argv[4], "wb");
  if (!out) return 1;
  std::set<std::string> seen;
  kdb::ReadOptions ro;
  unsigned long long n = 0;
  for (auto& op : ops) {
    if (!seen.insert(op.key).second) continue;
    std::string value;
    kdb::Status g = db.Get(ro, op.key, &value);
    const int32_t code = code_of(g);
    if (code != 0) value.clear();
    const uint32_t klen = (uint32_t)op.key.size();
    const uint64_t vlen = value.size();
    fwrite(&klen, 4, 1, out);
    fwrite(op.key.data(), 1, klen, out);
    fwrite(&code, 4, 1, out);
    fwrite(&vlen, 8, 1, out);
    fwrite(value.data(), 1, vlen, out);
    n++;
  }
  fclose(out);
  db.Close();
  printf("%llu keys read\n", n);
  return 0;
}

int main(int argc, char** argv) {
  kdb::Logger::set_current_level("emerg");
  if (argc >= 5 && !strcmp(argv[1], "--get")) return get_all(argc, argv);
  if (argc < 3) {
    fprintf(stderr, "usage: ref_ops <dbdir> <ops.bin> [maximum_part_size [hstable_size [hash]]]\n"
                    "       ref_ops --get <dbdir> <ops.bin> <out.bin>\n");
    return 2;
  }
  kdb::DatabaseOptions options;
  options.compression = kdb::kLZ4Compression;
  if (argc > 3) options.storage__maximum_part_size = strtoull(argv[3], nullptr, 0);
  if (argc > 4) options.storage__hstable_size = strtoull(argv[4], nullptr, 0);
  if (argc > 5) options.hash = strtoul(argv[5], nullptr, 0) ? kdb::kxxHash_64 : kdb::kMurmurHash3_64;
  kdb::Database db(options, argv[1]);
  kdb::Status s = db.Open();
  if (!s.IsOK()) {
    fprintf(stderr, "open: %s\n", s.ToString().c_str());
    return 1;
  }
  // (the ops are read after the open, as oracle/ref_db.cc does: HSTableManager
  // never clears the 8 KiB header block of its write buffer past the 72 bytes
  // it encodes, so a heap this program had already used would show in the files)
  std::vector<Op> ops;
  if (!read_ops(argv[2], &ops)) return 2;
  kdb::WriteOptions wo;
  unsigned long long puts = 0, deletes = 0;
  for (size_t i = 0; i < ops.size(); i++) {
    const Op& op = ops[i];
    kdb::ByteArray k = kdb::NewDeepCopyByteArray(op.key.data(), op.key.size());
    if (op.size_value == kDeleteMark) {
      s = db.Delete(wo, k);
      if (!s.IsOK()) {
        fprintf(stderr, "op %zu delete: %s\n", i, s.ToString().c_str());
        return 1;
      }
      deletes++;
      continue;
    }
    uint64_t off = 0;
    for (auto& c : op.chunks) {
      kdb::ByteArray kk = kdb::NewDeepCopyByteArray(op.key.data(), op.key.size());
      kdb::ByteArray v = kdb::NewDeepCopyByteArray(c.data(), c.size());
      s = db.PutPart(wo, kk, v, off, op.size_value);
      if (!s.IsOK()) {
        fprintf(stderr, "op %zu put: %s\n", i, s.ToString().c_str());
        return 1;
      }
      off += c.size();
    }
    puts++;
  }
  db.Close();
  printf("%llu puts %llu deletes\n", puts, deletes);
  return 0;
}
