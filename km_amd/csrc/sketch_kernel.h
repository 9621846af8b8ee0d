// sketch_kernel.h — solid k-mers in two passes: the kernels add_bases / add_text / add_fastq launch on a counter that has
// a sketch (km_counter_set_sketch), and the one behind km_counter_sketch_stats (DESIGN.md §10 "Solid k-mers, two
// passes"; the rule and why no key seen twice is lost: sketch_rule.h).
//   pass 1  k_sketch_note   every window's key is noted in the sketch; the counting table is not touched
//   pass 2  k_count_solid   k_count_insert, but a window is counted only if the sketch admits its key
//           k_sketch_fill   the set bits of either plane (statistics)
// The two passes walk a lane's 64 bytes as k_count_insert does (count_kernel.h: count_lane), each with a functor of its
// own.  Only vector loads, vector stores and vector atomics touch the sketch.
#pragma once
#include "count_kernel.h"
#include "sketch_rule.h"

namespace kmd {

constexpr uint32_t SKETCH_THREADS = 256;

// One add per wave of the lanes' 64-bit sum (nothing when the sum is 0).
__device__ inline void wave_add64(unsigned long long* cell, unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if (lane_id() == 0 && v) atomicAdd(cell, v);
}

// Pass 1.  text, n, own_from, k, canonical as for k_count_insert; a bounded grid, lane g of trip t owns the starts
// [32 (g + t * lanes of the grid), + 32) as in k_count_filtered.  Every window's key but ~0 (T^32 of a non-canonical
// k = 32 counter, which has no slot in the table and no entry here) is noted in sketch[0 .. 2^(64 - shift)).
// CM_BASES / CM_KMERS are left to pass 2; CM_NOTED tallies the windows noted.
__global__ __launch_bounds__(256) void k_sketch_note(const uint8_t* text, uint64_t n, uint32_t own_from, int k,
                                                     int canonical, uint64_t* sketch, uint32_t shift,
                                                     unsigned long long* meta) {
  uint32_t bases = 0, kmers = 0, noted = 0;
  for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g * COUNT_RUN < n;
       g += (uint64_t)gridDim.x * blockDim.x)
    noted += count_lane(text, n, g * COUNT_RUN, own_from, k, canonical, bases, kmers, [=](uint64_t key) {
      if (key == EMPTY) return 0u;
      kmsketch::note(
          sketch, kmsketch::slot_of(key, shift), [](uint64_t* p) { return *p; },
          [](uint64_t* p, uint64_t bits) {
            return (uint64_t)atomicOr(reinterpret_cast<unsigned long long*>(p), (unsigned long long)bits);
          });
      return 1u;
    });
  wave_add(&meta[CM_NOTED], noted);
}

// Pass 2.  k_count_insert with one more condition: a window adds 1 to its key only if the sketch, which no one writes
// any more, admits the key.  CM_BASES / CM_KMERS tally all bases and all windows, CM_ADMITTED the windows counted.  The
// key ~0 is always tallied in CM_ALLT, and the cut at finish decides about it as for a plain counter.
__global__ __launch_bounds__(256) void k_count_solid(const uint8_t* text, uint64_t n, uint32_t own_from, int k,
                                                     int canonical, CountSlot* tab, uint64_t smask,
                                                     const uint64_t* sketch, uint32_t shift, unsigned long long* meta) {
  const uint64_t s = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * COUNT_RUN;
  uint32_t bases = 0, kmers = 0, tally = 0;              // tally: claimed | allt << 8 | admitted << 16 (each <= 32)
  if (s < n)
    tally = count_lane(text, n, s, own_from, k, canonical, bases, kmers, [=](uint64_t key) {
      if (key == EMPTY) return 1u << 8;
      if (!kmsketch::admits(sketch, kmsketch::slot_of(key, shift))) return 0u;
      return (1u << 16) | count_add(tab, smask, key, 1u, meta);
    });
  wave_add(&meta[CM_DISTINCT], tally & 0xFFu);
  wave_add(&meta[CM_BASES], bases);
  wave_add(&meta[CM_KMERS], kmers);
  wave_add(&meta[CM_ALLT], (tally >> 8) & 0xFFu);
  wave_add(&meta[CM_ADMITTED], tally >> 16);
}

// The set bits of plane 1 and of plane 2 over sketch[0 .. words) into meta[CM_BITS_1] / meta[CM_BITS_2]: a popcount
// per word, a wave reduction, one atomic per wave and plane.
__global__ __launch_bounds__(256) void k_sketch_fill(const uint64_t* sketch, uint64_t words, unsigned long long* meta) {
  unsigned long long b1 = 0, b2 = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t v = sketch[i];
    b1 += (unsigned long long)__popc((uint32_t)v);
    b2 += (unsigned long long)__popc((uint32_t)(v >> 32));
  }
  wave_add64(&meta[CM_BITS_1], b1);
  wave_add64(&meta[CM_BITS_2], b2);
}

}  // namespace kmd
