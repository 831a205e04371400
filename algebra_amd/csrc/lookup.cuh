// Lookup by value on device-resident vectors of Fr, in section 12's conventions (canonical Montgomery
// residues; two elements are equal exactly when their eight 32-bit words are): the indices idx[i] = min{j : table[j] = values[i]}
// and the multiplicities m[j] = #{i : idx[i] = j} of a lookup, from the values themselves.
//   lookup_clear_kernel   every slot of the open-addressing table that the call will read <- EMPTY; the miss counter <- 0;
//   lookup_build_kernel   one lane per table entry j: linear probing from the home slot (lookup_hash.hpp) with atomicCAS; a slot
//                         that already holds an entry of the same value takes atomicMin(slot, j);
//   lookup_probe_kernel   one lane per witness cell: walks from the home slot to the entry of its value or to an empty slot,
//                         writes the index, counts the misses (one atomic per wave) and, fused, the multiplicities into the
//                         first word of the output's cells (cleared by fr_count_clear_kernel before, converted in place by
//                         fr_count_mont_kernel after: fraction_sum.cuh).
// No LDS, no barrier.  No lane waits on another lane anywhere: every probe loop is a for loop of at most `capacity` steps, and
// the capacity 2^capacity_log >= 2 table_len exceeds the number of entries, so an empty slot ends every walk long before.
//
// Determinism.  A slot changes from EMPTY to an entry once (the CAS) and afterwards only to a lower entry of the SAME value (the
// atomicMin is issued only after table[old] == key was read), so the value class of an occupied slot never changes.  A lane
// walking from its home slot therefore meets the same classes whatever the timing, stops at the slot of its own class if one
// exists before the first slot it could claim, and no class can come to own two slots: the later lane of a class would have
// had to pass the first one's slot, which it could only see as EMPTY (and then claim) or as its own class (and then stop).
// Each distinct value ends in exactly one slot holding the minimum of the indices that carried it.  WHICH slot a value owns
// depends on the order of the claims; what the probe returns does not.
#pragma once
#include "fraction_sum.cuh"
#include "lookup_hash.hpp"

namespace arkhip {

constexpr u32 LOOKUP_EMPTY = 0xFFFFFFFFu;   // also the index of a witness cell that is not in the table

// rounds of combining equal cells within a wave in front of the counts' atomicAdd.  Builds of 0, 1, 2 and 4 were timed in one
// process (tools/bench_lookup.py): at 2^24 cells the witness-like mix takes 1.5385 / 1.5369 / 1.5363 /
// 1.5335 ms, 1 within 4's spreads, so the lower ships; all cells equal takes 190.2 ms at 0 and 3.02 ms from 1 on.
// -DARK_LOOKUP_ROUNDS=0|1|2|4 on field_unit.hip builds the variants.
#ifdef ARK_LOOKUP_ROUNDS
constexpr int LOOKUP_COMBINE_ROUNDS = ARK_LOOKUP_ROUNDS;
#else
constexpr int LOOKUP_COMBINE_ROUNDS = 1;
#endif
static_assert(LOOKUP_COMBINE_ROUNDS >= 0 && LOOKUP_COMBINE_ROUNDS <= 8, "a fixed, small number of rounds");

// one call's pointers: the scratch cells lie in Context::poly_work behind the result slot
struct FrLookup {
  const void* table;
  size_t table_len;
  const void* values;
  size_t n;
  u32* indices;                  // n entries, or nullptr
  void* mult;                    // table_len elements, or nullptr
  unsigned long long* missing;   // one device cell
  u32* slots;                    // 2^capacity_log of them
  unsigned capacity_log;
};
// bytes of poly_work a call asks for: [result slot | miss counter (one element) | slots], whole elements
static inline size_t lookup_scratch_bytes(unsigned capacity_log) {
  return 64 + ((((size_t)4 << capacity_log) + 31) & ~(size_t)31);
}

template <class F>
__global__ void __launch_bounds__(256) lookup_clear_kernel(u32* slots, size_t capacity, unsigned long long* missing) {
  const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s == 0) *missing = 0;
  if (s < capacity) slots[s] = LOOKUP_EMPTY;
}

template <class F>
__global__ void __launch_bounds__(256) lookup_build_kernel(const char* __restrict__ table, size_t table_len, u32* slots,
                                                           unsigned capacity_log) {
  static_assert(F::N == 8, "the scalar fields served are 256-bit");
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= table_len) return;
  const F key = F::load(table + j * F::BYTES);
  const u32 mask = ((u32)1 << capacity_log) - 1;
  u32 s = lookup_home_slot(key.l, capacity_log);
  for (u32 step = 0; step <= mask; step++, s = (s + 1) & mask) {
    const u32 old = atomicCAS(slots + s, LOOKUP_EMPTY, (u32)j);
    if (old == LOOKUP_EMPTY) break;
    if (F::eq(F::load(table + (size_t)old * F::BYTES), key)) {   // old < table_len: only build lanes write slots after the clear
      atomicMin(slots + s, (u32)j);
      break;
    }
  }
}

template <class F>
__global__ void __launch_bounds__(256) lookup_probe_kernel(const char* __restrict__ table, const u32* __restrict__ slots,
                                                           unsigned capacity_log, const char* __restrict__ values, size_t n,
                                                           u32* indices, char* mult, unsigned long long* missing) {
  static_assert(F::N == 8, "the scalar fields served are 256-bit");
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned lane = threadIdx.x & 63;
  const bool live = i < n;
  u32 k = LOOKUP_EMPTY;
  if (live) {
    const F key = F::load(values + i * F::BYTES);
    const u32 mask = ((u32)1 << capacity_log) - 1;
    u32 s = lookup_home_slot(key.l, capacity_log);
    for (u32 step = 0; step <= mask; step++, s = (s + 1) & mask) {
      const u32 j = slots[s];
      if (j == LOOKUP_EMPTY) break;
      if (F::eq(F::load(table + (size_t)j * F::BYTES), key)) {
        k = j;
        break;
      }
    }
    if (indices) indices[i] = k;
  }
  // the misses of the wave in one atomic
  const unsigned long long miss = __ballot(live && k == LOOKUP_EMPTY);
  if (miss && lane == (unsigned)(__ffsll(miss) - 1)) atomicAdd(missing, (unsigned long long)__popcll(miss));
  if (!mult) return;
  // the counts.  Lanes past n and lanes that missed never take part.  A round: the first still-active lane's cell is
  // broadcast, the lanes with the same cell are found with a ballot, that first lane adds their number in one atomic and
  // they all retire.  Inside `if (active)` the active lanes are exactly the executing ones, so readfirstlane reads the first
  // of them and the ballot sees only them; the first active lane always matches itself.
  bool active = live && k != LOOKUP_EMPTY;
#pragma unroll
  for (int r = 0; r < LOOKUP_COMBINE_ROUNDS; r++) {
    if (active) {
      const u32 lead = (u32)__builtin_amdgcn_readfirstlane((int)k);
      const unsigned long long same = __ballot(k == lead);
      if (lane == (unsigned)(__ffsll(same) - 1)) atomicAdd((unsigned int*)(mult + (size_t)lead * F::BYTES), (unsigned int)__popcll(same));
      if (k == lead) active = false;
    }
  }
  if (active) atomicAdd((unsigned int*)(mult + (size_t)k * F::BYTES), 1u);
}

// the launches of one call on one stream.  n = 0 still builds the table: the build phase alone, for a caller that times it.
template <class F>
int fr_lookup_launch(const FrLookup& lk, hipStream_t s) {
  const size_t capacity = (size_t)1 << lk.capacity_log;
  const size_t cells = (lk.table_len + 255) / 256, items = (lk.n + 255) / 256, clears = (capacity + 255) / 256;
  if (lk.table_len == 0 || lk.capacity_log < 1 || lk.capacity_log > LOOKUP_MAX_CAPACITY_LOG || capacity < 2 * lk.table_len ||
      items > 0x7fffffffu)
    return -1000;
  hipLaunchKernelGGL((lookup_clear_kernel<F>), dim3((unsigned)clears), dim3(256), 0, s, lk.slots, capacity, lk.missing);
  hipLaunchKernelGGL((lookup_build_kernel<F>), dim3((unsigned)cells), dim3(256), 0, s, (const char*)lk.table, lk.table_len, lk.slots,
                     lk.capacity_log);
  if (lk.mult) hipLaunchKernelGGL((fr_count_clear_kernel<F>), dim3((unsigned)cells), dim3(256), 0, s, (char*)lk.mult, lk.table_len);
  if (lk.n)
    hipLaunchKernelGGL((lookup_probe_kernel<F>), dim3((unsigned)items), dim3(256), 0, s, (const char*)lk.table, (const u32*)lk.slots,
                       lk.capacity_log, (const char*)lk.values, lk.n, lk.indices, (char*)lk.mult, lk.missing);
  if (lk.mult && lk.n) hipLaunchKernelGGL((fr_count_mont_kernel<F>), dim3((unsigned)cells), dim3(256), 0, s, (char*)lk.mult, lk.table_len);
  return hipGetLastError() == hipSuccess ? 0 : -1000;
}

}  // namespace arkhip
