// The home slot of an element in the lookup's open-addressing table (lookup.cuh): ONE function of the
// element's eight 32-bit words and capacity_log, for the device kernels and for the host (ark_hip_test_lookup_slot calls it so
// that tests can construct colliding tables).  Every word passes through a multiply-rotate-multiply step that is a bijection of
// the running state, then the 32-bit finaliser of MurmurHash3 spreads the state over all bits; the TOP capacity_log bits are the slot.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ARK_LOOKUP_HD __host__ __device__ __forceinline__
#else
#define ARK_LOOKUP_HD inline
#endif

namespace arkhip {

constexpr unsigned LOOKUP_MAX_TABLE_LOG = 28;                        // table_len <= 2^28
constexpr unsigned LOOKUP_MAX_CAPACITY_LOG = LOOKUP_MAX_TABLE_LOG + 1;

// the smallest c >= 1 with 2^c >= 2 table_len: the load factor is at most 1/2 and an empty slot always exists
static inline unsigned lookup_capacity_log(size_t table_len) {
  unsigned c = 1;
  while (((size_t)1 << c) < 2 * table_len) c++;
  return c;
}

ARK_LOOKUP_HD uint32_t lookup_home_slot(const uint32_t* w, unsigned capacity_log) {
  uint32_t h = 0x9E3779B9u;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint32_t k = w[i] * 0xCC9E2D51u;
    k = (k << 15) | (k >> 17);
    h ^= k * 0x1B873593u;
    h = (h << 13) | (h >> 19);
    h = h * 5u + 0xE6546B64u;
  }
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h >> (32 - capacity_log);   // 1 <= capacity_log <= 29
}

}  // namespace arkhip
