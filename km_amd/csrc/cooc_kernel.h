// cooc_kernel.h — how the inputs of a mark counter relate: one streaming pass over its table that counts, for every
// pair of inputs, the keys both hold, and per key how many inputs hold it.  The kernel behind km_counter_cooccurrence
// (DESIGN.md §10 "Compare"; the arithmetic: cooc_rule.h).
//
// A trip of a wave is 64 slots, one aligned dwordx4 per lane.  The n ballots b_i of "bit i of my mask" turn the 64
// masks into n words of 64 slots each; pair (i, j) gains popcount(b_i & b_j).  The ballots are wave-uniform but the
// pairs are per lane (pair lane + 64 t, at most 9 of the 528), and a lane cannot index the wave's scalars, so the
// ballots pass through an LDS row of n words that belongs to this wave alone.
//
// Why there is no block barrier in the loop, and what stands in its place.  Slot counts are powers of two >= 64 and a
// block has four waves: at a 64-slot table waves 1 .. 3 of block 0 make no trip at all, and in any table the waves of
// a block may make different numbers of trips (and skip different all-empty ones), so __syncthreads() inside the loop
// would hang.  None is needed: row w is written and read by wave w only.  Within one wave the order "lane i stores
// b_i, then every lane loads the words of its pairs" (and "every lane has loaded, then lane i stores the next trip's
// b_i") is made an order of the memory model by wave_lds_sync(): a release fence at wavefront scope, the wave barrier
// (__builtin_amdgcn_wave_barrier, which keeps the compiler from moving LDS accesses of any lane across it), and an
// acquire fence at wavefront scope.  The lanes of a wave issue their LDS instructions in program order and the LDS
// serves one wave's instructions in that order, so the fences cost no wait beyond the load's own.
// The two __syncthreads() of the kernel stand outside the loop, where every thread of the block arrives.
//
// Accumulators: a pair gains at most 64 per trip.  They are 64-bit registers (18 VGPRs), so no number of trips
// overflows them.  A block first sums its four waves' accumulators in LDS (64-bit LDS adds), then adds every non-zero
// pair to the result in HBM with one 64-bit atomic each.  The result exists COOC_SETS times and a block adds to set
// blockIdx % COOC_SETS, so the blocks, which all end at about the same time, do not queue on 33 lines; the host sums
// the sets.  in_exactly and private go per lane through a small LDS histogram of the block (32-bit bins: a block
// visits fewer than 2^32 slots, mark_host.h refuses a table where it would not) and are flushed the same way.
#pragma once
#include "cooc_rule.h"
#include "count_kernel.h"

namespace kmd {

constexpr uint32_t COOC_THREADS = 256, COOC_WAVES = COOC_THREADS / 64;
constexpr uint32_t COOC_GRID = 2048;          // 256 CUs x 8 resident blocks; the rest is grid-stride
constexpr uint32_t COOC_SETS = 16;            // copies of the result (kmcooc::CELLS cells each)

// Orders one wave's own LDS accesses: those before it, of every lane, happen before those after it, of every lane.
__device__ inline void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// tab[0 .. n_slots): the table of a mark counter with n inputs, 1 <= n <= 32, n_slots a multiple of 64 (so is the
// stride: a wave's lanes stay together).  cell_sets[COOC_SETS][kmcooc::CELLS] gain what the table holds.  The table
// is only read.
__global__ __launch_bounds__(COOC_THREADS) void k_cooc_table(const CountSlot* tab, uint64_t n_slots, uint32_t n,
                                                             unsigned long long* cell_sets) {
  __shared__ unsigned long long rows[COOC_WAVES][kmcooc::MAX_INPUTS];
  __shared__ unsigned long long block_pairs[kmcooc::MAX_PAIRS];
  __shared__ uint32_t hist[kmcooc::HIST_BINS];
  for (uint32_t i = threadIdx.x; i < kmcooc::MAX_PAIRS; i += COOC_THREADS) block_pairs[i] = 0;
  for (uint32_t i = threadIdx.x; i < kmcooc::HIST_BINS; i += COOC_THREADS) hist[i] = 0;
  __syncthreads();

  const uint32_t lane = (uint32_t)lane_id();
  unsigned long long* row = rows[threadIdx.x >> 6];
  const uint32_t np = kmcooc::n_pairs(n), trips = kmcooc::lane_trips(n);
  // the lane's pairs; a lane without a pair t reads word 0 twice and its sum is never flushed
  uint32_t pi[kmcooc::PAIRS_PER_LANE], pj[kmcooc::PAIRS_PER_LANE];
  unsigned long long acc[kmcooc::PAIRS_PER_LANE];
#pragma unroll
  for (uint32_t t = 0; t < kmcooc::PAIRS_PER_LANE; ++t) {
    const uint32_t p = kmcooc::lane_pair(lane, t);
    const bool have = p < np;
    pi[t] = have ? kmcooc::pair_row(p) : 0u;
    pj[t] = have ? kmcooc::pair_col(p, pi[t]) : 0u;
    acc[t] = 0;
  }

  const uint64_t stride = (uint64_t)gridDim.x * COOC_THREADS;
  for (uint64_t at = (uint64_t)blockIdx.x * COOC_THREADS + (threadIdx.x - lane); at < n_slots; at += stride) {
    const uint64_t i0 = at + lane;
    uint4 v = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u);
    if (i0 < n_slots) v = *reinterpret_cast<const uint4*>(tab + i0);
    const uint32_t mask = (v.x & v.y) != 0xFFFFFFFFu ? kmcooc::input_bits(v.z, n) : 0u;
    if (__ballot(mask != 0u) == 0ull) continue;            // (wave-uniform) 64 empty slots
    for (uint32_t i = 0; i < n; ++i) {
      const unsigned long long b = __ballot((mask >> i) & 1u);
      if (lane == i) row[i] = b;
    }
    wave_lds_sync();                                       // the row is written before any lane reads it
#pragma unroll
    for (uint32_t t = 0; t < kmcooc::PAIRS_PER_LANE; ++t)
      if (t < trips) acc[t] += (unsigned long long)__popcll(row[pi[t]] & row[pj[t]]);
    wave_lds_sync();                                       // ... and read before the next trip writes it
    if (mask) {
      atomicAdd(&hist[kmcooc::exact_bin(mask)], 1u);
      if ((mask & (mask - 1u)) == 0u) atomicAdd(&hist[kmcooc::private_bin(mask)], 1u);
    }
  }

#pragma unroll
  for (uint32_t t = 0; t < kmcooc::PAIRS_PER_LANE; ++t) {
    const uint32_t p = kmcooc::lane_pair(lane, t);
    if (p < np && acc[t]) atomicAdd(&block_pairs[p], acc[t]);
  }
  __syncthreads();
  unsigned long long* cells = cell_sets + (uint64_t)(blockIdx.x % COOC_SETS) * kmcooc::CELLS;
  for (uint32_t p = threadIdx.x; p < np; p += COOC_THREADS) {
    const unsigned long long v = block_pairs[p];
    if (v) atomicAdd(&cells[p], v);
  }
  for (uint32_t i = threadIdx.x; i < kmcooc::HIST_BINS; i += COOC_THREADS) {
    const uint32_t v = hist[i];
    if (v) atomicAdd(&cells[kmcooc::CELL_EXACT + i], (unsigned long long)v);
  }
}

}  // namespace kmd
