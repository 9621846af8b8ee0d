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

// text, n, own_from, k, canonical as for k_count_insert, and its walk over a lane's 64 bytes: 32 own window starts,
// k - 1 bytes of the neighbour, a break at any byte that is no base or lies at or behind n.  Lane g of trip t owns the
// starts [32 (g + t * lanes of the grid), + 32).  A window adds 1 to its key's count only if the key is in the table;
// the key ~0 goes to CM_ALLT only if the filter holds it (CM_ALLT_HAVE).  CM_BASES / CM_KMERS tally all bases and all
// windows as k_count_insert does, CM_HITS the windows that were counted.
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
  const uint64_t kmask = k >= 32 ? ~0ull : ((1ull << (2 * k)) - 1);
  const uint32_t rshift = 2u * (uint32_t)(k - 1);
  const uint32_t jend = (uint32_t)k + COUNT_RUN - 1;   // bytes a lane looks at (<= 63)
  uint32_t bases = 0, kmers = 0, allt = 0, hits = 0;
  for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g * COUNT_RUN < n;
       g += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t s = g * COUNT_RUN;
    const uint4* p = reinterpret_cast<const uint4*>(text + s);
    const uint4 q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3];
    const uint32_t w[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w,
                            q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
    uint64_t fwd = 0, rev = 0;
    uint32_t run = 0;
#pragma unroll
    for (uint32_t d = 0; d < 16; ++d) {
      if (4 * d < jend) {
        const uint32_t word = w[d];
#pragma unroll 1
        for (uint32_t b = 0; b < 4; ++b) {
          const uint32_t j = 4 * d + b;
          const uint32_t ch = (word >> (8 * b)) & 0xFFu;
          const uint32_t up = ch & 0xDFu;
          const bool base = (up == 'A' || up == 'C' || up == 'G' || up == 'T') && s + j < n && j < jend;
          uint32_t c = (ch >> 1) & 3u;                         // A 0, C 1, T 2, G 3
          c ^= c >> 1;                                         // A 0, C 1, G 2, T 3
          fwd = ((fwd << 2) | c) & kmask;
          rev = (rev >> 2) | ((uint64_t)(3u - c) << rshift);
          run = base ? run + 1 : 0;
          bases += (base && j < COUNT_RUN && s + j >= own_from) ? 1u : 0u;
          if (run >= (uint32_t)k) {                            // (j < jend: the window starts at j - k + 1 < 32)
            const uint64_t key = (canonical && rev < fwd) ? rev : fwd;
            ++kmers;
            if (key == EMPTY) {
              if (allt_have) { ++allt; ++hits; }
            } else {
              const uint64_t idx = LDS ? filter_lookup_lds(lkeys, smask, key, meta) : count_lookup(tab, smask, key, meta);
              if (idx != NO_SLOT) {
                atomicAdd(&tab[idx].count, 1u);
                ++hits;
              }
            }
          }
        }
      }
    }
  }
  wave_add(&meta[CM_BASES], bases);
  wave_add(&meta[CM_KMERS], kmers);
  wave_add(&meta[CM_ALLT], allt);
  wave_add(&meta[CM_HITS], hits);
}

}  // namespace kmd
