// cooc_rule.h — the arithmetic of `compare`: which pair of inputs a pair index names, and what one trip of a wave over
// 64 slots of a mark counter's table adds to the result (plain C++17, no HIP headers; __host__ __device__ under hipcc,
// so cooc_kernel.h, mark_host.h and tests/host/cooc_rule.cpp run the same code).  DESIGN.md §10 "Compare".
//
// The rule (include/kmgpu.h states it for the callers):
//   A slot's count cell is a membership mask: bit i set = the key is in the set of input i, 0 <= i < n <= 32.  An
//   empty slot counts as mask 0, and bits at or above n are never set.
//   shared[i][j] = the slots whose mask has bits i and j (i == j: bit i), kept for j <= i as pair p = i (i + 1) / 2 + j.
//   in_exactly[m] = the slots whose mask has exactly m bits, 1 <= m <= n; private[i] = the slots whose mask is 1 << i.
//   A trip sees 64 masks as n ballots b_i (bit s of b_i = bit i of mask s): pair (i, j) gains popcount(b_i & b_j).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KM_COOC_HD __host__ __device__
#else
#define KM_COOC_HD
#endif

namespace kmcooc {

constexpr uint32_t MAX_INPUTS = 32;
constexpr uint32_t WAVE = 64;                                        // slots per trip, lanes that share the pairs
constexpr uint32_t MAX_PAIRS = MAX_INPUTS * (MAX_INPUTS + 1) / 2;    // 528
constexpr uint32_t PAIRS_PER_LANE = (MAX_PAIRS + WAVE - 1) / WAVE;   // 9
// what the table pass leaves on the device, 64-bit cells: the pairs, in_exactly[0 .. 32], private[0 .. 31]
constexpr uint32_t CELL_EXACT = MAX_PAIRS, CELL_PRIVATE = CELL_EXACT + MAX_INPUTS + 1, CELLS = CELL_PRIVATE + MAX_INPUTS;
// the block's small histogram of popcount(mask): in_exactly[0 .. 32] (bin 0 unused), then private[0 .. 31]
constexpr uint32_t HIST_PRIVATE = MAX_INPUTS + 1, HIST_BINS = HIST_PRIVATE + MAX_INPUTS;

KM_COOC_HD inline uint32_t n_pairs(uint32_t n) { return n * (n + 1) / 2; }
KM_COOC_HD inline uint32_t pair_index(uint32_t i, uint32_t j) { return i * (i + 1) / 2 + j; }     // j <= i
// the i of pair p: the largest i with i (i + 1) / 2 <= p (p < 2^31; a walk of at most 32 steps where it is used)
KM_COOC_HD inline uint32_t pair_row(uint32_t p) {
  uint32_t i = 0;
  while ((i + 1) * (i + 2) / 2 <= p) ++i;
  return i;
}
KM_COOC_HD inline uint32_t pair_col(uint32_t p, uint32_t i) { return p - i * (i + 1) / 2; }
// pair t of lane `lane`: lane + 64 t, so the pairs of a trip are spread over the lanes, at most PAIRS_PER_LANE each
KM_COOC_HD inline uint32_t lane_pair(uint32_t lane, uint32_t t) { return lane + WAVE * t; }
KM_COOC_HD inline uint32_t lane_trips(uint32_t n) { return (n_pairs(n) + WAVE - 1) / WAVE; }

KM_COOC_HD inline uint32_t popc64(uint64_t v) { return (uint32_t)__builtin_popcountll((unsigned long long)v); }
KM_COOC_HD inline uint32_t popc32(uint32_t v) { return (uint32_t)__builtin_popcount(v); }
KM_COOC_HD inline uint32_t input_bits(uint32_t mask, uint32_t n) { return n >= 32u ? mask : mask & ((1u << n) - 1u); }

// ballot i of 64 masks (what __ballot(mask >> i & 1) gives the wave)
KM_COOC_HD inline uint64_t ballot_of(const uint32_t* masks, uint32_t i) {
  uint64_t b = 0;
  for (uint32_t s = 0; s < WAVE; ++s) b |= (uint64_t)((masks[s] >> i) & 1u) << s;
  return b;
}
// what pair p gains from the trip whose ballots are row[0 .. n)
KM_COOC_HD inline uint32_t pair_gain(const uint64_t* row, uint32_t i, uint32_t j) { return popc64(row[i] & row[j]); }
// the bin of the block's histogram a lane with this mask adds 1 to for in_exactly (mask != 0), and for private
// (popcount 1 only)
KM_COOC_HD inline uint32_t exact_bin(uint32_t mask) { return popc32(mask); }
KM_COOC_HD inline uint32_t private_bin(uint32_t mask) { return HIST_PRIVATE + (uint32_t)__builtin_ctz(mask); }

// One trip, as the kernel makes it: 64 masks in; pairs[n_pairs(n)], exact[n + 1] and priv[n] gain what the trip adds.
// The pairs go the kernel's way (ballots into a row, lane by lane over lane_pair), the other two slot by slot.
inline void trip_model(const uint32_t* masks, uint32_t n, uint64_t* pairs, uint64_t* exact, uint64_t* priv) {
  uint64_t row[MAX_INPUTS];
  uint32_t m[WAVE];
  for (uint32_t s = 0; s < WAVE; ++s) m[s] = input_bits(masks[s], n);
  for (uint32_t i = 0; i < n; ++i) row[i] = ballot_of(m, i);
  const uint32_t np = n_pairs(n);
  for (uint32_t lane = 0; lane < WAVE; ++lane)
    for (uint32_t t = 0; t < lane_trips(n); ++t) {
      const uint32_t p = lane_pair(lane, t);
      if (p >= np) break;
      const uint32_t i = pair_row(p);
      pairs[p] += pair_gain(row, i, pair_col(p, i));
    }
  for (uint32_t s = 0; s < WAVE; ++s) {
    if (!m[s]) continue;
    ++exact[exact_bin(m[s])];
    if (popc32(m[s]) == 1) ++priv[private_bin(m[s]) - HIST_PRIVATE];
  }
}

// ---- the result the callers see, from the device's cells and the mask of the key that has no slot (T^32 of a
// non-canonical k = 32 table; 0: it is in no input): the full symmetric matrix, union, in_exactly, private
struct Result {
  uint64_t shared[MAX_INPUTS * MAX_INPUTS];
  uint64_t in_exactly[MAX_INPUTS + 1];
  uint64_t priv[MAX_INPUTS];
  uint64_t n_union;
};
inline void fold(const uint64_t* cells, uint32_t n, uint32_t extra_mask, Result* r) {
  *r = Result{};
  extra_mask = input_bits(extra_mask, n);
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t j = 0; j <= i; ++j) {
      const uint64_t v = cells[pair_index(i, j)] + ((extra_mask >> i) & (extra_mask >> j) & 1u);
      r->shared[i * MAX_INPUTS + j] = r->shared[j * MAX_INPUTS + i] = v;
    }
  for (uint32_t m = 1; m <= n; ++m) r->in_exactly[m] = cells[CELL_EXACT + m];
  for (uint32_t i = 0; i < n; ++i) r->priv[i] = cells[CELL_PRIVATE + i];
  if (extra_mask) {
    ++r->in_exactly[popc32(extra_mask)];
    if (popc32(extra_mask) == 1) ++r->priv[__builtin_ctz(extra_mask)];
  }
  for (uint32_t m = 1; m <= n; ++m) r->n_union += r->in_exactly[m];
}

}  // namespace kmcooc
