// Open-addressing table of 64-bit keys on the device (the contingency table of csrc/eval.hip, the face-pair table of
// csrc/morph.hip): linear probing from a mixed hash, insertion by compare-and-swap, an overflow bit instead of a silent loss.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bsmi {

constexpr uint64_t kEmpty = ~0ull;

static __device__ __forceinline__ uint64_t mix64(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

// slot of `key` in an open-addressing table of cap (power of two) slots, inserted if absent; -1 (and an overflow bit) when
// the table is full.  `key` must not be kEmpty.
static __device__ int64_t table_slot(uint64_t* keys, uint64_t cap, uint64_t key, uint32_t* inserts, uint32_t* flags, uint32_t bit) {
  uint64_t h = mix64(key) & (cap - 1);
  for (uint64_t probe = 0; probe < cap; ++probe) {
    uint64_t k = __atomic_load_n(&keys[h], __ATOMIC_RELAXED);
    if (k == key) return (int64_t)h;
    if (k == kEmpty) {
      const unsigned long long old = atomicCAS((unsigned long long*)&keys[h], (unsigned long long)kEmpty, (unsigned long long)key);
      if (old == kEmpty) {
        // a table past 7/8 full probes long: report it as an overflow before it fills up
        if (atomicAdd(inserts, 1u) + 1 > (uint32_t)(cap - cap / 8)) atomicOr(flags, bit);
        return (int64_t)h;
      }
      if (old == key) return (int64_t)h;
    }
    h = (h + 1) & (cap - 1);
  }
  atomicOr(flags, bit);
  return -1;
}

}  // namespace bsmi
