// mark_kernel.h — records of existing tables into a counter whose count cells are membership masks: the kernel behind
// km_counter_mark_records / km_counter_mark_jf (DESIGN.md §10 "Compare").  Input g (0-based, g < 32) sets bit g of the
// count cell of every key one of its records brings with lower <= count <= upper.  An OR is idempotent, commutes and
// associates: a key with several records, records fed twice, the order of arrival and the piece size change nothing.
// k_count_rehash carries a count cell into the grown table by adding it to a fresh slot's 0, so a mask survives growth.
#pragma once
#include "merge_kernel.h"

namespace kmd {

// raw[0 .. n * (kb + cb)): records as k_count_add_records takes them (its decode, written out again, as
// merge_kernel.h explains).  A record with count 0, or outside the cut, is absent: it claims no slot.  The key ~0
// (EMPTY) has no slot: CM_ALLT is its mask, a 64-bit cell.
__global__ __launch_bounds__(256) void k_mark_records(const uint8_t* raw, uint64_t n, uint32_t kb, uint32_t cb,
                                                      uint32_t lower, uint32_t upper, uint32_t g, CountSlot* tab,
                                                      uint64_t smask, unsigned long long* meta) {
  uint32_t claimed = 0, taken = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
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
    if (cnt == 0 || cnt < lower || cnt > upper) continue;
    ++taken;
    if (key == EMPTY) {
      atomicOr(&meta[CM_ALLT], 1ull << g);
      continue;
    }
    uint32_t mine;
    const uint64_t idx = count_find(tab, smask, key, meta, &mine);
    if (idx == NO_SLOT) continue;
    claimed += mine;
    atomicOr(&tab[idx].count, 1u << g);
  }
  wave_add(&meta[CM_DISTINCT], claimed);
  wave_add(&meta[CM_RECORDS], taken);
}

}  // namespace kmd
