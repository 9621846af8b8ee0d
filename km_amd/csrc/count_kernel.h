// count_kernel.h — counting k-mers from reads: a counting hash table in HBM and the three kernels that fill it,
// grow it and empty it into the record arrays kmjf_upload_from_device takes.  How a lane walks the
// text is count_rule.h's; count_lane here loads its 64 bytes, for this kernel and for those of filter_kernel.h and
// sketch_kernel.h.
//
// Table: open addressing with linear probing over 16-byte slots {u64 key, u32 count, u32 unused}; the key and
// its count share one 16-byte piece of a line, so the add that follows a key's lookup hits the line that lookup
// brought in.  Empty key = ~0 (device_common.h: EMPTY).  That value is also the k-mer T^32 of a non-canonical
// k = 32 table (in canonical mode T^32 is stored as A^32 = 0): it is counted in a cell of its own (CM_ALLT).
// Counts are integers added with atomics: the final set of (key, count) does not depend on arrival order.
// The slot's fourth word is 0 everywhere except under the set operations of setops_kernel.h.
#pragma once
#include "count_rule.h"
#include "device_common.h"

namespace kmd {

struct __attribute__((aligned(16))) CountSlot {
  uint64_t key;
  uint32_t count;
  uint32_t unused;
};
static_assert(sizeof(CountSlot) == 16, "one dwordx4 per slot");

constexpr uint32_t COUNT_RUN = kmcount::RUN;      // window start positions a lane owns
constexpr uint32_t COUNT_PAD = kmcount::PAD;      // readable bytes behind a staged chunk (the last lane loads 64 from its start)
// cells of the counter's device meta block (u64 each)
// (CM_FORMAT: fastq_kernel.h's smallest (stream offset << 8 | kind), ~0 while the text is well-formed)
// (CM_RECORDS: merge_kernel.h's tally of the records taken; CM_BASES / CM_KMERS tally text only)
// (CM_ALLT_HAVE / CM_ALLT_MATCH: setops_kernel.h's "claimed" and spare word of the key ~0, which has no slot;
//  filter_kernel.h: CM_ALLT_HAVE = the key ~0 is in the filter)
// (CM_HITS: filter_kernel.h's tally of the windows whose key was in the filter)
// (CM_NOTED / CM_ADMITTED: sketch_kernel.h's tallies of the windows noted in pass 1 and counted in pass 2;
//  CM_BITS_1 / CM_BITS_2: the set bits of the sketch's two planes, k_sketch_fill)
enum { CM_DISTINCT = 0, CM_BASES = 1, CM_KMERS = 2, CM_ALLT = 3, CM_ERROR = 4, CM_OUT = 5, CM_FORMAT = 6, CM_RECORDS = 7,
       CM_ALLT_HAVE = 8, CM_ALLT_MATCH = 9, CM_HITS = 10, CM_NOTED = 11, CM_ADMITTED = 12, CM_BITS_1 = 13, CM_BITS_2 = 14,
       CM_WORDS = 15 };

__global__ void k_count_init(CountSlot* slots, uint64_t n_slots) {
  uint4* p = reinterpret_cast<uint4*>(slots);
  const uint4 empty = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u);
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots;
       i += (uint64_t)gridDim.x * blockDim.x)
    p[i] = empty;
}

// Find or claim the slot of `key` and add `add` to its count; returns 1 if the slot was claimed here.
// The slot is read first; the compare-and-swap is issued only for a slot that looks empty, the add only once
// the slot is known to hold the key.  A key, once written, never changes, so a slot read as another key is
// another key for good.  The host keeps occupied <= slots / 2 (km_counter: the limit is checked against the
// worst case of a chunk before the chunk is inserted), so an empty slot always ends the probe; the bound on
// the loop only makes a broken invariant an error (CM_ERROR) instead of a hang.
__device__ inline uint32_t count_add(CountSlot* tab, uint64_t smask, uint64_t key, uint32_t add,
                                     unsigned long long* meta) {
  uint64_t idx = mix64(key) & smask;
  for (uint64_t step = 0; step <= smask; ++step) {
    unsigned long long* kp = reinterpret_cast<unsigned long long*>(&tab[idx].key);
    unsigned long long cur = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t claimed = 0;
    if (cur == EMPTY) {
      cur = atomicCAS(kp, (unsigned long long)EMPTY, (unsigned long long)key);
      if (cur == EMPTY) { cur = key; claimed = 1; }
    }
    if (cur == key) {
      atomicAdd(&tab[idx].count, add);
      return claimed;
    }
    idx = (idx + 1) & smask;
  }
  atomicAdd(&meta[CM_ERROR], 1ull);
  return 0;
}

// One add per wave of the lanes' sum (nothing when the sum is 0).
__device__ inline void wave_add(unsigned long long* cell, uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if (lane_id() == 0 && v) atomicAdd(cell, (unsigned long long)v);
}

// The walk of one lane (count_rule.h: kmcount::lane_walk) over the 64 bytes from text + s, loaded as four aligned
// dwordx4; s = 32 * the lane's index, s < n.  The four counting kernels (k_count_insert here, k_count_filtered,
// k_sketch_note, k_count_solid) are each a distribution of lanes and a functor given to this.
template <class Window>
__device__ inline uint32_t count_lane(const uint8_t* text, uint64_t n, uint64_t s, uint32_t own_from, int k, int canonical,
                                      uint32_t& bases, uint32_t& kmers, Window window) {
  const uint4* p = reinterpret_cast<const uint4*>(text + s);
  const uint4 q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3];
  const uint32_t w[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w,
                          q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
  return kmcount::lane_walk(w, n, s, own_from, k, canonical, bases, kmers, window);
}

// text[0 .. n): bases and breaks, PAD readable bytes behind them; own_from: bytes [0, own_from) were counted as bases
// by the piece before (count_rule.h).  One lane per thread; every window's key is inserted with count 1, the key ~0
// tallied in CM_ALLT instead.
__global__ __launch_bounds__(256) void k_count_insert(const uint8_t* text, uint64_t n, uint32_t own_from, int k,
                                                      int canonical, CountSlot* tab, uint64_t smask,
                                                      unsigned long long* meta) {
  const uint64_t s = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * COUNT_RUN;
  uint32_t bases = 0, kmers = 0, tally = 0;              // tally: claimed | allt << 8 (each <= 32)
  if (s < n)
    tally = count_lane(text, n, s, own_from, k, canonical, bases, kmers, [=](uint64_t key) {
      if (key == EMPTY) return 1u << 8;
      return count_add(tab, smask, key, 1u, meta);
    });
  wave_add(&meta[CM_DISTINCT], tally & 0xFFu);
  wave_add(&meta[CM_BASES], bases);
  wave_add(&meta[CM_KMERS], kmers);
  wave_add(&meta[CM_ALLT], tally >> 8);
}

// Every occupied slot of the old table into the new one (twice the capacity or more), its count added.
__global__ void k_count_rehash(const CountSlot* old_tab, uint64_t old_slots, CountSlot* tab, uint64_t smask,
                               unsigned long long* meta) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < old_slots;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint4 v = *reinterpret_cast<const uint4*>(old_tab + i);
    const uint64_t key = ((uint64_t)v.y << 32) | v.x;
    if (key != EMPTY) (void)count_add(tab, smask, key, v.z, meta);
  }
}

// The occupied slots with count >= lower_count, dense, in keys[] / counts[]: a ballot per wave, one atomic
// append per wave.  n_slots is a multiple of 64 and so is the stride: a wave's lanes stay together.
__global__ void k_count_compact(const CountSlot* tab, uint64_t n_slots, uint32_t lower_count, uint64_t* keys,
                                uint32_t* counts, unsigned long long* meta) {
  const uint32_t lane = (uint32_t)lane_id();
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint4 v = *reinterpret_cast<const uint4*>(tab + i);
    const uint64_t key = ((uint64_t)v.y << 32) | v.x;
    const bool keep = key != EMPTY && v.z >= lower_count;
    const unsigned long long m = __ballot(keep);
    if (m == 0) continue;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(&meta[CM_OUT], (unsigned long long)__popcll(m));
    base = lane_u64(base, 0);
    if (keep) {
      const uint64_t at = base + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
      keys[at] = key;
      counts[at] = v.z;
    }
  }
}

}  // namespace kmd
