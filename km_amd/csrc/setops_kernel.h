// setops_kernel.h — set operations over the inputs of one counter: the kernels behind km_counter_set_records /
// km_counter_set_jf and km_counter_finish_range (DESIGN.md §10 "Set operations").
//   intersect: the keys present (count > 0) in every input, with the minimum over all their records;
//   subtract:  the records of input 1 whose key occurs (count > 0) in no later input, repeats summed with saturation.
// Input 1 claims slots as k_count_add_records does.  Every later input only LOOKS UP: a key that is not in the table
// after input 1 is in neither result, so the table never grows again and a probe ends at an empty slot or the key.
// What a later input leaves behind sits in the slot's fourth word (CountSlot::unused), which is 0 all through input 1
// (k_count_rehash drops it: growth during input 1 loses nothing):
//   intersect: the number of later inputs matched IN A ROW.  Input g (1-based, g >= 2) moves the word from g - 2 to
//              g - 1 and from nothing else; a key that missed input 2 stays at 0 through input 3 and is dead for good.
//              During input g the word is g - 2 or g - 1 (alive) or below (dead), whatever the records of g, of this
//              key or another, have done so far: the outcome depends neither on arrival order nor on the piece size.
//   subtract:  1 = dead.
// Intersect keeps ~count in the count cell and combines with atomicMax: a freshly claimed slot holds 0, the identity
// of that max (it reads as 2^32 - 1, the identity of min), so a record that finds the slot before its claimer has
// written a count loses nothing.  Subtract keeps the plain count (count_add_saturating).
#pragma once
#include "merge_kernel.h"

namespace kmd {

// count_find's probe without the claim: the slot of `key`, NO_SLOT at the first empty slot.  (The host keeps the
// table at most half full, so an empty slot always ends the probe; the bound only turns a broken invariant into
// CM_ERROR instead of a hang.)
__device__ inline uint64_t count_lookup(CountSlot* tab, uint64_t smask, uint64_t key, unsigned long long* meta) {
  uint64_t idx = mix64(key) & smask;
  for (uint64_t step = 0; step <= smask; ++step) {
    unsigned long long* kp = reinterpret_cast<unsigned long long*>(&tab[idx].key);
    const unsigned long long cur = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == key) return idx;
    if (cur == EMPTY) return NO_SLOT;
    idx = (idx + 1) & smask;
  }
  atomicAdd(&meta[CM_ERROR], 1ull);
  return NO_SLOT;
}

// raw[0 .. n * (kb + cb)): records as k_count_add_records takes them (its decode, written out again), of input g
// (1-based) of the set operation op.  A record with count 0 is absent: it claims, matches and removes nothing.
// The key ~0 (EMPTY) has no slot: CM_ALLT is its count cell, CM_ALLT_HAVE its "claimed", CM_ALLT_MATCH its spare word.
__global__ __launch_bounds__(256) void k_set_records(const uint8_t* raw, uint64_t n, uint32_t kb, uint32_t cb, int op,
                                                     uint32_t g, CountSlot* tab, uint64_t smask,
                                                     unsigned long long* meta) {
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
    if (cnt == 0) continue;
    ++taken;
    if (key == EMPTY) {
      if (g == 1) {
        atomicMax(&meta[CM_ALLT_HAVE], 1ull);
        if (op == KM_SET_INTERSECT) atomicMax(&meta[CM_ALLT], (unsigned long long)(uint32_t)~cnt);
        else atomicAdd(&meta[CM_ALLT], (unsigned long long)cnt);         // (64-bit: the host clamps it)
      } else if (__hip_atomic_load(&meta[CM_ALLT_HAVE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
        // not in input 1: as a key without a slot
      } else if (op == KM_SET_INTERSECT) {
        atomicMax(&meta[CM_ALLT], (unsigned long long)(uint32_t)~cnt);
        atomicCAS(&meta[CM_ALLT_MATCH], (unsigned long long)(g - 2), (unsigned long long)(g - 1));
      } else {
        atomicMax(&meta[CM_ALLT_MATCH], 1ull);
      }
      continue;
    }
    if (g == 1) {
      uint32_t mine;
      const uint64_t idx = count_find(tab, smask, key, meta, &mine);
      if (idx == NO_SLOT) continue;
      claimed += mine;
      if (op == KM_SET_INTERSECT) atomicMax(&tab[idx].count, ~cnt);
      else count_add_saturating(&tab[idx].count, cnt);
      continue;
    }
    const uint64_t idx = count_lookup(tab, smask, key, meta);
    if (idx == NO_SLOT) continue;
    uint32_t* spare = &tab[idx].unused;
    const uint32_t seen = __hip_atomic_load(spare, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (op == KM_SET_INTERSECT) {
      if (seen + 2 < g) continue;             // missed an earlier input: dead, and nothing of input g changes that
      atomicMax(&tab[idx].count, ~cnt);
      if (seen + 2 == g) atomicCAS(spare, g - 2, g - 1);
    } else if (seen == 0) {
      __hip_atomic_store(spare, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  wave_add(&meta[CM_DISTINCT], claimed);
  wave_add(&meta[CM_RECORDS], taken);
}

// k_count_compact with the cut on both sides and the spare word: a slot is kept iff its spare word equals `want`
// (intersect of N inputs: N - 1; subtract, and a table no set operation touched: 0) and lower <= count <= upper,
// the count read as ~cell when `complemented`.  One ballot and one append per wave.
__global__ void k_set_compact(const CountSlot* tab, uint64_t n_slots, uint32_t want, int complemented, uint32_t lower,
                              uint32_t upper, uint64_t* keys, uint32_t* counts, unsigned long long* meta) {
  const uint32_t lane = (uint32_t)lane_id();
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint4 v = *reinterpret_cast<const uint4*>(tab + i);
    const uint64_t key = ((uint64_t)v.y << 32) | v.x;
    const uint32_t cnt = complemented ? ~v.z : v.z;
    const bool keep = key != EMPTY && v.w == want && cnt >= lower && cnt <= upper;
    const unsigned long long m = __ballot(keep);
    if (m == 0) continue;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(&meta[CM_OUT], (unsigned long long)__popcll(m));
    base = lane_u64(base, 0);
    if (keep) {
      const uint64_t at = base + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
      keys[at] = key;
      counts[at] = cnt;
    }
  }
}

}  // namespace kmd
