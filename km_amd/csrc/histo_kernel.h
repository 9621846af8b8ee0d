// histo_kernel.h — the histogram of counts and the four statistics in one streaming pass: the kernels behind
// km_counter_histo / km_jf_histo (DESIGN.md §10 "Histogram and statistics"; the bin rule: histo_layout.h).
//
// One body (histo_add / histo_begin / histo_end), three ways of fetching counts: the counting table before finish
// (k_histo_table), the dense counts after it (k_histo_counts), raw file records (k_histo_records).  A count c takes
// part iff lo <= c <= hi (lo >= 1: a count of 0 is no key); bins and statistics see exactly those.
//
// Bins: 32-bit counters in LDS per block for the first min(n_bins, HISTO_W) bins, flushed at block end with one global
// 64-bit atomic per NON-ZERO LDS bin; counts that fall at or beyond HISTO_W (the thin tail of real data) go straight
// to the global bins.  A block's LDS bin cannot overflow: it counts at most the elements the block fetches, a launch
// covers at most HISTO_CHUNK items, and a grid smaller than HISTO_GRID only where every thread has at most
// HISTO_ITEMS_PER_THREAD of them, so a block takes at most HISTO_CHUNK / HISTO_GRID + 2 * 256 = 2^27 + 512 items of at
// most four counts each: fewer than 2^30 elements.  The host (histo_host.h: histo_launch) cuts anything longer into
// several launches.
//
// Hot bins: on real reads most keys have count 1 or 2, so a plain version sends most lanes of every wave to one LDS
// address.  Before LDS is touched the wave aggregates: for `rounds` rounds the bin of the first lane still active is
// broadcast, the lanes holding the same bin are balloted, the first lane adds their number, and they retire; whoever
// is left afterwards adds 1 on its own.  Every element is added exactly once whatever `rounds` is (0 included).
#pragma once
#include "count_kernel.h"

namespace kmd {

constexpr uint32_t HISTO_W = 4096;             // bins held in LDS: 16 KiB, eight blocks of 256 on a CU (all 32 waves)
constexpr uint32_t HISTO_THREADS = 256;
constexpr uint32_t HISTO_GRID = 2048;          // 256 CUs x 8 resident blocks; the rest is grid-stride
constexpr uint64_t HISTO_CHUNK = 1ull << 38;   // items per launch (see above)
constexpr uint32_t HISTO_ITEMS_PER_THREAD = 4; // below HISTO_GRID blocks: fewer, fuller blocks (fewer flushes)
constexpr uint32_t HISTO_ROUNDS = 0;           // aggregation rounds (the runs that chose it)
enum { HS_UNIQUE = 0, HS_DISTINCT = 1, HS_TOTAL = 2, HS_MAX = 3, HS_WORDS = 4 };   // the order of km_histo_stats_t
// The four statistics cells exist HISTO_CELL_SETS times, each set on a 128-byte line of its own, and a block adds to
// set blockIdx % HISTO_CELL_SETS; the host sums the sets.  With one set every wave of the grid queues on one line
// (DESIGN.md §10 has the figures).
constexpr uint32_t HISTO_CELL_SETS = 64, HISTO_CELL_STRIDE = 16;

struct HistoRule {
  uint64_t base, ceil;       // histo_layout.h
  uint32_t inc;              // min(increment, 2^32 - 1): c - base < 2^32 - 1 divides to 0 by either
  uint32_t n_bins;           // <= 2^24
  uint32_t lo, hi;           // the cut, lo >= 1
  uint32_t rounds;
};

struct HistoLane {           // what a lane has seen (a block sees fewer than 2^30 elements: n and n1 fit)
  uint32_t n, n1, max;
  uint64_t sum;              // several counts near 2^32 can meet in one lane
};

__device__ inline uint32_t histo_bin(uint32_t c, const HistoRule& r) {
  if ((uint64_t)c < r.base) return 0;
  if ((uint64_t)c > r.ceil) return r.n_bins - 1;
  const uint32_t d = c - (uint32_t)r.base;
  return r.inc == 1 ? d : d / r.inc;           // (wave-uniform choice)
}

__device__ inline void histo_bump(uint32_t b, uint32_t by, uint32_t* lds, unsigned long long* bins) {
  if (b < HISTO_W) atomicAdd(&lds[b], by);
  else atomicAdd(&bins[b], (unsigned long long)by);
}

// One element per lane (valid: the lane has one).  Called by all lanes of a wave together.
__device__ inline void histo_add(bool valid, uint32_t c, const HistoRule& r, uint32_t* lds, unsigned long long* bins,
                                 HistoLane& a) {
  valid = valid && c >= r.lo && c <= r.hi;
  if (valid) {
    ++a.n;
    a.n1 += c == 1 ? 1u : 0u;
    a.sum += c;
    a.max = c > a.max ? c : a.max;
  }
  const uint32_t b = histo_bin(c, r);
  const uint32_t lane = (uint32_t)lane_id();
  unsigned long long active = __ballot(valid);
  for (uint32_t round = 0; round < r.rounds && active; ++round) {
    const uint32_t first = (uint32_t)__ffsll((long long)active) - 1;
    const uint32_t fb = lane_u32(b, first);
    const unsigned long long same = __ballot(valid && b == fb);
    if (lane == first) histo_bump(fb, (uint32_t)__popcll(same), lds, bins);
    valid = valid && b != fb;
    active &= ~same;
  }
  if (valid) histo_bump(b, 1u, lds, bins);
}

__device__ inline void histo_begin(uint32_t* lds, HistoLane& a) {
  for (uint32_t i = threadIdx.x; i < HISTO_W; i += HISTO_THREADS) lds[i] = 0;
  a.n = a.n1 = a.max = 0;
  a.sum = 0;
  __syncthreads();
}

// The block's LDS bins into the global ones, the lanes' statistics once per wave into the block's set of four cells.
__device__ inline void histo_end(const uint32_t* lds, const HistoRule& r, const HistoLane& a, unsigned long long* bins,
                                 unsigned long long* cell_sets) {
  unsigned long long* cells = cell_sets + (blockIdx.x % HISTO_CELL_SETS) * HISTO_CELL_STRIDE;
  uint32_t n = a.n, n1 = a.n1, mx = a.max;
  unsigned long long sum = a.sum;
  for (int o = 32; o > 0; o >>= 1) {
    n += __shfl_xor(n, o);
    n1 += __shfl_xor(n1, o);
    const uint32_t om = __shfl_xor(mx, o);
    mx = om > mx ? om : mx;
    sum += __shfl_xor(sum, o);
  }
  if (lane_id() == 0 && n) {
    if (n1) atomicAdd(&cells[HS_UNIQUE], (unsigned long long)n1);
    atomicAdd(&cells[HS_DISTINCT], (unsigned long long)n);
    atomicAdd(&cells[HS_TOTAL], sum);
    atomicMax(&cells[HS_MAX], (unsigned long long)mx);
  }
  __syncthreads();
  const uint32_t w = r.n_bins < HISTO_W ? r.n_bins : HISTO_W;
  for (uint32_t i = threadIdx.x; i < w; i += HISTO_THREADS) {
    const uint32_t v = lds[i];
    if (v) atomicAdd(&bins[i], (unsigned long long)v);
  }
}

// The counting table: every lane loads whole slots as one aligned dwordx4, two per trip (both requested before either
// is looked at); a slot whose key is EMPTY is skipped.  A pure stream read of 16 * n_slots bytes.
__global__ __launch_bounds__(HISTO_THREADS) void k_histo_table(const CountSlot* tab, uint64_t n_slots, HistoRule r,
                                                               unsigned long long* bins, unsigned long long* cells) {
  __shared__ uint32_t lds[HISTO_W];
  HistoLane a;
  histo_begin(lds, a);
  const uint64_t stride = (uint64_t)gridDim.x * HISTO_THREADS;
  const uint32_t lane = (uint32_t)lane_id();
  // (the trip count is the wave's, not the lane's: the ballots of histo_add need the whole wave)
  for (uint64_t at = (uint64_t)blockIdx.x * HISTO_THREADS + (threadIdx.x - lane); at < n_slots; at += 2 * stride) {
    const uint64_t i0 = at + lane, i1 = i0 + stride;
    uint4 v0 = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u), v1 = v0;
    if (i0 < n_slots) v0 = *reinterpret_cast<const uint4*>(tab + i0);
    if (i1 < n_slots) v1 = *reinterpret_cast<const uint4*>(tab + i1);
    histo_add((v0.x & v0.y) != 0xFFFFFFFFu, v0.z, r, lds, bins, a);
    histo_add((v1.x & v1.y) != 0xFFFFFFFFu, v1.z, r, lds, bins, a);
  }
  histo_end(lds, r, a, bins, cells);
}

// Dense counts: one aligned dwordx4 = four counts per lane and trip; the n % 4 counts of the tail go one per lane
// through the first wave of block 0.
__global__ __launch_bounds__(HISTO_THREADS) void k_histo_counts(const uint32_t* counts, uint64_t n, HistoRule r,
                                                                unsigned long long* bins, unsigned long long* cells) {
  __shared__ uint32_t lds[HISTO_W];
  HistoLane a;
  histo_begin(lds, a);
  const uint64_t stride = (uint64_t)gridDim.x * HISTO_THREADS, quads = n / 4;
  const uint32_t lane = (uint32_t)lane_id();
  for (uint64_t at = (uint64_t)blockIdx.x * HISTO_THREADS + (threadIdx.x - lane); at < quads; at += stride) {
    const uint64_t i = at + lane;
    const bool have = i < quads;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (have) v = reinterpret_cast<const uint4*>(counts)[i];
    histo_add(have, v.x, r, lds, bins, a);
    histo_add(have, v.y, r, lds, bins, a);
    histo_add(have, v.z, r, lds, bins, a);
    histo_add(have, v.w, r, lds, bins, a);
  }
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    const uint64_t i = quads * 4 + lane;
    const bool have = i < n;
    histo_add(have, have ? counts[i] : 0u, r, lds, bins, a);
  }
  histo_end(lds, r, a, bins, cells);
}

// raw[0 .. n * (kb + cb)): n `binary/sorted` records as they sit in a file, [kb key bytes][cb count bytes], kb <= 8,
// 1 <= cb <= 4, raw 16-byte aligned.  Keys are not decoded.  12-byte records: a lane takes four records as three
// aligned dwordx4 and uses dwords 2, 5, 8 and 11, the n % 4 records of the tail go one per lane through the first
// wave of block 0; other widths are read by bytes, one record per lane and trip, as k_count_add_records does.
__global__ __launch_bounds__(HISTO_THREADS) void k_histo_records(const uint8_t* raw, uint64_t n, uint32_t kb, uint32_t cb,
                                                                 HistoRule r, unsigned long long* bins,
                                                                 unsigned long long* cells) {
  __shared__ uint32_t lds[HISTO_W];
  HistoLane a;
  histo_begin(lds, a);
  const uint64_t stride = (uint64_t)gridDim.x * HISTO_THREADS;
  const uint32_t lane = (uint32_t)lane_id();
  const uint64_t first = (uint64_t)blockIdx.x * HISTO_THREADS + (threadIdx.x - lane);
  if (kb == 8 && cb == 4) {
    const uint64_t quads = n / 4;
    for (uint64_t at = first; at < quads; at += stride) {
      const uint64_t i = at + lane;
      const bool have = i < quads;
      uint4 q0 = make_uint4(0u, 0u, 0u, 0u), q1 = q0, q2 = q0;
      if (have) {
        const uint4* p = reinterpret_cast<const uint4*>(raw) + 3 * i;
        q0 = p[0]; q1 = p[1]; q2 = p[2];
      }
      histo_add(have, q0.z, r, lds, bins, a);
      histo_add(have, q1.y, r, lds, bins, a);
      histo_add(have, q2.x, r, lds, bins, a);
      histo_add(have, q2.w, r, lds, bins, a);
    }
    if (blockIdx.x == 0 && threadIdx.x < 64) {
      const uint64_t i = quads * 4 + lane;
      const bool have = i < n;
      histo_add(have, have ? reinterpret_cast<const uint32_t*>(raw)[3 * i + 2] : 0u, r, lds, bins, a);
    }
  } else {
    for (uint64_t at = first; at < n; at += stride) {
      const uint64_t i = at + lane;
      const bool have = i < n;
      uint32_t cnt = 0;
      if (have) {
        const uint8_t* p = raw + i * (kb + cb) + kb;
        for (uint32_t b = 0; b < cb; ++b) cnt |= (uint32_t)p[b] << (8 * b);
      }
      histo_add(have, cnt, r, lds, bins, a);
    }
  }
  histo_end(lds, r, a, bins, cells);
}

}  // namespace kmd
