// kingdb_amd/csrc/hash_device.h -- the key hashes on the device (algorithm/hash.cc:9-23):
// XXH64 and MurmurHash3_x64_128, for the write path (put.hip: the offset array's
// hashed keys) and the read path (index.hip: the lookup's bucket).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kdb_lz4 {
namespace {

// ----------------------------------------------------------------- hashes
__device__ __forceinline__ uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
__device__ __forceinline__ uint64_t ld64(const uint8_t* p) {
  uint64_t v = 0;
  for (int i = 7; i >= 0; i--) v = (v << 8) | p[i];
  return v;
}
__device__ __forceinline__ uint32_t ld32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// XXH64(p, len, 0) (algorithm/xxhash.cc:427).
constexpr uint64_t XP1 = 11400714785074694791ULL, XP2 = 14029467366897019727ULL, XP3 = 1609587929392839161ULL,
                   XP4 = 9650029242287828579ULL, XP5 = 2870177450012600261ULL;
__device__ __forceinline__ uint64_t xround(uint64_t acc, uint64_t in) {
  acc += in * XP2;
  acc = rotl64(acc, 31);
  return acc * XP1;
}
__device__ uint64_t xxh64(const uint8_t* p, uint32_t len) {
  const uint8_t* end = p + len;
  uint64_t h;
  if (len >= 32) {
    uint64_t v1 = XP1 + XP2, v2 = XP2, v3 = 0, v4 = 0 - XP1;
    const uint8_t* lim = end - 32;
    do {
      v1 = xround(v1, ld64(p));
      v2 = xround(v2, ld64(p + 8));
      v3 = xround(v3, ld64(p + 16));
      v4 = xround(v4, ld64(p + 24));
      p += 32;
    } while (p <= lim);
    h = rotl64(v1, 1) + rotl64(v2, 7) + rotl64(v3, 12) + rotl64(v4, 18);
    h = (h ^ xround(0, v1)) * XP1 + XP4;
    h = (h ^ xround(0, v2)) * XP1 + XP4;
    h = (h ^ xround(0, v3)) * XP1 + XP4;
    h = (h ^ xround(0, v4)) * XP1 + XP4;
  } else {
    h = XP5;
  }
  h += (uint64_t)len;
  while (p + 8 <= end) {
    h ^= xround(0, ld64(p));
    h = rotl64(h, 27) * XP1 + XP4;
    p += 8;
  }
  if (p + 4 <= end) {
    h ^= (uint64_t)ld32(p) * XP1;
    h = rotl64(h, 23) * XP2 + XP3;
    p += 4;
  }
  while (p < end) {
    h ^= (uint64_t)(*p) * XP5;
    h = rotl64(h, 11) * XP1;
    p++;
  }
  h ^= h >> 33;
  h *= XP2;
  h ^= h >> 29;
  h *= XP3;
  h ^= h >> 32;
  return h;
}

// MurmurHash3_x64_128(p, len, 0), first 8 bytes (murmurhash3.cc:255-330).
__device__ __forceinline__ uint64_t fmix64(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdULL;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ULL;
  k ^= k >> 33;
  return k;
}
__device__ uint64_t murmur3_64(const uint8_t* d, uint32_t len) {
  const uint64_t c1 = 0x87c37b91114253d5ULL, c2 = 0x4cf5ad432745937fULL;
  uint64_t h1 = 0, h2 = 0;
  const uint32_t nb = len / 16u;
  for (uint32_t i = 0; i < nb; i++) {
    uint64_t k1 = ld64(d + 16u * i), k2 = ld64(d + 16u * i + 8u);
    k1 *= c1; k1 = rotl64(k1, 31); k1 *= c2; h1 ^= k1;
    h1 = rotl64(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52dce729;
    k2 *= c2; k2 = rotl64(k2, 33); k2 *= c1; h2 ^= k2;
    h2 = rotl64(h2, 31); h2 += h1; h2 = h2 * 5 + 0x38495ab5;
  }
  const uint8_t* t = d + 16u * nb;
  const uint32_t r = len & 15u;
  uint64_t k1 = 0, k2 = 0;
  for (uint32_t i = r; i > 8u; i--) k2 ^= (uint64_t)t[i - 1u] << (8u * (i - 9u));
  if (r > 8u) { k2 *= c2; k2 = rotl64(k2, 33); k2 *= c1; h2 ^= k2; }
  for (uint32_t i = r < 8u ? r : 8u; i > 0u; i--) k1 ^= (uint64_t)t[i - 1u] << (8u * (i - 1u));
  if (r > 0u) { k1 *= c1; k1 = rotl64(k1, 31); k1 *= c2; h1 ^= k1; }
  h1 ^= (uint64_t)len;
  h2 ^= (uint64_t)len;
  h1 += h2;
  h2 += h1;
  h1 = fmix64(h1);
  h2 = fmix64(h2);
  return h1 + h2;
}

}  // namespace
}  // namespace kdb_lz4
