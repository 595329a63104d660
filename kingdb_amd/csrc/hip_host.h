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

}  // namespace kdb_lz4
