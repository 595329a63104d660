// kingdb_amd/csrc/hip_host.h -- host-side plumbing of the entry points that
// report KDB_PUT_* codes (index.hip, hstable_dev.hip, recover.hip).  Internal:
// the KDB_LZ4_* mappings of the codec's entry points are their own.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/kdb_put.h"

// Inside a function that returns hipError_t: leaves with the first failure.
#define KDB_TRY(expr)                     \
  do {                                    \
    const hipError_t e_ = (expr);         \
    if (e_ != hipSuccess) return e_;      \
  } while (0)

namespace kdb_lz4 {

inline int hip_code(hipError_t e) {
  if (e == hipSuccess) return KDB_PUT_OK;
  return (e == hipErrorNoDevice || e == hipErrorInvalidDevice) ? KDB_PUT_ENODEV : KDB_PUT_EHIP;
}

inline uint64_t align64(uint64_t x) { return (x + 63u) & ~63ull; }
inline uint64_t align256(uint64_t x) { return (x + 255u) & ~255ull; }

// Workgroups for n items, per_block each, at most `most` and at least one.
inline uint32_t grid_for(uint64_t n, uint32_t per_block, uint32_t most) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + per_block - 1u) / per_block, most));
}

// The owner of one hipMalloc'd array of T: move-only, freed when it goes.
template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept { swap(o); }
  DevBuf& operator=(DevBuf&& o) noexcept {   // the array held goes with o
    swap(o);
    return *this;
  }
  ~DevBuf() {
    if (p_) (void)hipFree(p_);
  }
  // n elements; what it held is freed first
  hipError_t alloc(size_t n) {
    DevBuf().swap(*this);
    return hipMalloc(reinterpret_cast<void**>(&p_), n * sizeof(T));
  }
  T* get() const { return p_; }
  void swap(DevBuf& o) { std::swap(p_, o.p_); }

 private:
  T* p_ = nullptr;
};

}  // namespace kdb_lz4
