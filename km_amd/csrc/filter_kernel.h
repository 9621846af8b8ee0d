// filter_kernel.h — counting only a given set of k-mers: the kernels behind km_counter_set_filter and what
// add_bases / add_text / add_fastq launch on a counter that has a filter (DESIGN.md §10 "Filtered counting").
// The filter's keys are claimed ONCE, with count 0, in the counting table of count_kernel.h (k_filter_seed); from then
// on the table only takes lookups, so it never grows and a probe ends at the key or at the first empty slot.  The
// counting pass has two tiers over the same table and the same slot indices:
//   LDS tier  (slots <= FILTER_LDS_SLOTS): a block copies the table's key column into LDS once and then makes trip
//             after trip over the text (a bounded grid: the copy is amortised over the trips); a window's key is
//             probed in LDS with the table's own hash and mask, and only a hit touches HBM: one integer atomic on
//             tab[idx].count;
//   HBM tier  (larger sets): the same loop, the probe is count_lookup on the table itself.
// Either tier leaves the same table bytes: the slot a key sits in is settled by the seed, and the adds commute.
#pragma once
#include "setops_kernel.h"

namespace kmd {

constexpr uint32_t FILTER_LDS_SLOTS = 8192;          // key column of the LDS tier: 64 KiB of static LDS per block
constexpr uint32_t FILTER_THREADS = 256;

// keys[0 .. n): k-mers in the counter's encoding, repeats allowed.  Every key, canonicalised when the counter is,
// claims its slot through count_find's compare-and-swap; the count stays 0 and a repeated key claims once.  The key
// ~0 (T^32 of a non-canonical k = 32 counter) has no slot: CM_ALLT_HAVE says that it is in the filter.
__global__ __launch_bounds__(256) void k_filter_seed(const uint64_t* keys, uint64_t n, int k, int canonical,
                                                     CountSlot* tab, uint64_t smask, unsigned long long* meta) {
  uint32_t claimed = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t key = keys[i];
    if (canonical) {
      const uint64_t rc = revcomp(key, k);
      if (rc < key) key = rc;
    }
    if (key == EMPTY) {
      atomicMax(&meta[CM_ALLT_HAVE], 1ull);
      continue;
    }
    uint32_t mine;
    if (count_find(tab, smask, key, meta, &mine) != NO_SLOT) claimed += mine;
  }
  wave_add(&meta[CM_DISTINCT], claimed);
}

// count_lookup's probe over the key column in LDS: the same hash, mask and order, so the same slot index.
__device__ inline uint64_t filter_lookup_lds(const uint64_t* lkeys, uint64_t smask, uint64_t key,
                                             unsigned long long* meta) {
  uint64_t idx = mix64(key) & smask;
  for (uint64_t step = 0; step <= smask; ++step) {
    const uint64_t cur = lkeys[idx];
    if (cur == key) return idx;
    if (cur == EMPTY) return NO_SLOT;
    idx = (idx + 1) & smask;
  }
  atomicAdd(&meta[CM_ERROR], 1ull);
  return NO_SLOT;
}

// text, n, own_from, k, canonical as for k_count_insert, and the same walk of a lane (count_kernel.h: count_lane).
// A bounded grid: lane g of trip t owns the starts [32 (g + t * lanes of the grid), + 32).  A window adds 1 to its
// key's count only if the key is in the table; the key ~0 goes to CM_ALLT only if the filter holds it (CM_ALLT_HAVE).
// CM_BASES / CM_KMERS tally all bases and all windows as k_count_insert does, CM_HITS the windows that were counted.
template <bool LDS>
__global__ __launch_bounds__(256) void k_count_filtered(const uint8_t* text, uint64_t n, uint32_t own_from, int k,
                                                        int canonical, CountSlot* tab, uint64_t smask,
                                                        unsigned long long* meta) {
  __shared__ uint64_t lkeys[LDS ? FILTER_LDS_SLOTS : 1];
  if (LDS) {                                           // (smask < FILTER_LDS_SLOTS: the host chose this tier)
    const uint4* src = reinterpret_cast<const uint4*>(tab);
    for (uint32_t i = threadIdx.x; i <= (uint32_t)smask; i += FILTER_THREADS) {
      const uint4 v = src[i];
      lkeys[i] = ((uint64_t)v.y << 32) | v.x;
    }
    __syncthreads();
  }
  const bool allt_have = meta[CM_ALLT_HAVE] != 0;     // (written by the seed, long before this launch)
  const uint64_t* keys = lkeys;
  uint32_t bases = 0, kmers = 0, allt = 0, hits = 0;
  for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g * COUNT_RUN < n;
       g += (uint64_t)gridDim.x * blockDim.x) {
    // hits | allt << 16 of this trip (each <= 32; unpacked per trip: a block may make thousands of them)
    const uint32_t tally = count_lane(text, n, g * COUNT_RUN, own_from, k, canonical, bases, kmers, [=](uint64_t key) {
      if (key == EMPTY) return allt_have ? (1u << 16) | 1u : 0u;
      const uint64_t idx = LDS ? filter_lookup_lds(keys, smask, key, meta) : count_lookup(tab, smask, key, meta);
      if (idx == NO_SLOT) return 0u;
      atomicAdd(&tab[idx].count, 1u);
      return 1u;
    });
    hits += tally & 0xFFFFu;
    allt += tally >> 16;
  }
  wave_add(&meta[CM_BASES], bases);
  wave_add(&meta[CM_KMERS], kmers);
  wave_add(&meta[CM_ALLT], allt);
  wave_add(&meta[CM_HITS], hits);
}

}  // namespace kmd
