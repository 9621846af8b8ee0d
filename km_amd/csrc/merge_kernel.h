// merge_kernel.h — records of existing tables into the counting table: the kernel behind km_counter_add_records /
// km_counter_add_jf (DESIGN.md §10 "Merging tables").  A record brings a key AND a count, so the count is combined
// by a mode (sum, saturating at 2^32 - 1, or max) instead of the + 1 per window of k_count_insert.  Every
// combination is one atomic read-modify-write whose result does not depend on the order of arrival.
#pragma once
#include "count_kernel.h"

namespace kmd {

// count_add's probe with the slot handed back instead of added to: the index of the slot of `key`, found or claimed
// (*claimed = 1 if claimed here), NO_SLOT behind the same CM_ERROR guard.  (A probe of its own, not one shared
// with count_add: folding the two changes the machine code of k_count_insert, which this path leaves as it is.)
constexpr uint64_t NO_SLOT = ~0ull;
__device__ inline uint64_t count_find(CountSlot* tab, uint64_t smask, uint64_t key, unsigned long long* meta,
                                      uint32_t* claimed) {
  uint64_t idx = mix64(key) & smask;
  for (uint64_t step = 0; step <= smask; ++step) {
    unsigned long long* kp = reinterpret_cast<unsigned long long*>(&tab[idx].key);
    unsigned long long cur = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t mine = 0;
    if (cur == EMPTY) {
      cur = atomicCAS(kp, (unsigned long long)EMPTY, (unsigned long long)key);
      if (cur == EMPTY) { cur = key; mine = 1; }
    }
    if (cur == key) {
      *claimed = mine;
      return idx;
    }
    idx = (idx + 1) & smask;
  }
  atomicAdd(&meta[CM_ERROR], 1ull);
  *claimed = 0;
  return NO_SLOT;
}

// count = min(count + add, 2^32 - 1) as a compare-and-swap loop: a saturating add commutes and associates, so the
// final value is the clipped total whatever order the adds arrive in (an atomicAdd with a repair afterwards would
// let a reader, or a second wrap, see the wrapped value).  A slot that has reached the top takes no more swaps.
__device__ inline void count_add_saturating(uint32_t* cell, uint32_t add) {
  uint32_t old = __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (old != 0xFFFFFFFFu) {
    const uint32_t sum = old + add;
    const uint32_t seen = atomicCAS(cell, old, sum < old ? 0xFFFFFFFFu : sum);
    if (seen == old) break;
    old = seen;
  }
}

// raw[0 .. n * (kb + cb)): n `binary/sorted` records as they sit in a file, [kb little-endian key bytes][cb count
// bytes], kb <= 8, 1 <= cb <= 4.  One record per lane and trip, decoded and inserted in one pass.  A record with
// count 0 is skipped and claims no slot.  The key ~0 (EMPTY; T^32 of a non-canonical k = 32 table) lives in
// CM_ALLT as in k_count_insert, a 64-bit cell that km_counter_finish clamps.  mode: KM_MERGE_SUM / KM_MERGE_MAX.
__global__ __launch_bounds__(256) void k_count_add_records(const uint8_t* raw, uint64_t n, uint32_t kb, uint32_t cb,
                                                           int mode, CountSlot* tab, uint64_t smask,
                                                           unsigned long long* meta) {
  uint32_t claimed = 0, taken = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    // (k_unpack_records' decode, written out again: one function for both reorders the instructions of both kernels)
    uint64_t key = 0;
    uint32_t cnt = 0;
    if (kb == 8 && cb == 4) {                 // 12-byte records: three aligned dwords
      const uint32_t* w = reinterpret_cast<const uint32_t*>(raw) + 3 * i;
      key = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
      cnt = w[2];
    } else {
      const uint8_t* r = raw + i * (kb + cb);
      for (uint32_t b = 0; b < kb; ++b) key |= (uint64_t)r[b] << (8 * b);
      for (uint32_t b = 0; b < cb; ++b) cnt |= (uint32_t)r[kb + b] << (8 * b);
    }
    if (cnt == 0) continue;
    ++taken;
    if (key == EMPTY) {
      if (mode == KM_MERGE_MAX) atomicMax(&meta[CM_ALLT], (unsigned long long)cnt);
      else atomicAdd(&meta[CM_ALLT], (unsigned long long)cnt);
      continue;
    }
    uint32_t mine;
    const uint64_t idx = count_find(tab, smask, key, meta, &mine);
    if (idx == NO_SLOT) continue;
    claimed += mine;
    if (mode == KM_MERGE_MAX) atomicMax(&tab[idx].count, cnt);
    else count_add_saturating(&tab[idx].count, cnt);
  }
  wave_add(&meta[CM_DISTINCT], claimed);
  wave_add(&meta[CM_RECORDS], taken);
}

}  // namespace kmd
