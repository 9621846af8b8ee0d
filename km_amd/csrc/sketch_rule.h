// sketch_rule.h — the two-plane Bloom sketch of `count --solid`: where a key lives in it, how a key is noted in the
// first pass over the reads and when the second pass admits it (plain C++17, no HIP headers; __host__ __device__ under
// hipcc, so sketch_kernel.h, sketch_host.h and tests/host/sketch_rule.cpp run the same code).
// DESIGN.md §10 "Solid k-mers, two passes".
//
// The rule (include/kmgpu.h states it for the callers):
//   The sketch is W 64-bit words, W a power of two, 64 <= W <= 2^40.  The low 32 bits of a word are plane 1 ("seen"),
//   the high 32 bits plane 2 ("seen again").
//   A key's slot:  h = mix64(key ^ 0x9E3779B97F4A7C15), word = h >> (64 - log2 W),
//                  mask = 1 << (h & 31) | 1 << (h >> 5 & 31) | 1 << (h >> 10 & 31): one to three bits of a plane.
//   Note a key:    load the word (a plain load); if plane 2 already holds the mask, nothing to do; otherwise
//                  old = fetch_or(word, mask), and if plane 1 of `old` held the mask, fetch_or(word, mask << 32) too.
//   Admit a key:   plane 2 of its word holds its mask (plain loads, in a pass of its own after all notes).
//
// No false negatives: a key noted twice is admitted, whatever the order in which the lanes of the device arrive.
//   Bits are only ever set within a pass.  What the plain load returns may be stale, but a stale word holds a subset of
//   the bits the word has now, so the load can fail to skip a key whose mask plane 2 holds already (the two atomics then
//   set bits that are set) and can never skip one whose mask plane 2 does not hold.  A key that is skipped finds its
//   mask in plane 2, which is all the second pass asks.  Of the occurrences of one key that are not skipped, every one
//   issues the first fetch_or, and all fetch_ors on one word are totally ordered: the one that comes second in that order
//   gets an `old` whose plane 1 holds the mask the first one set, and sets the mask in plane 2.  So once a key has been
//   noted twice, skipped or not, plane 2 holds its mask.
// False positives: plane 2 may hold a key's mask although the key was noted once, when other keys of the same word set
//   its bits; such a key is admitted and counted exactly, with count 1, and the cut at finish drops it.  Which of them
//   are admitted can depend on arrival order (plane 1 is read by the fetch_or that may set plane 2); that they number
//   few is a matter of the sizing below and costs table slots only, never a count.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define KM_SKETCH_HD __host__ __device__
#else
#define KM_SKETCH_HD
#endif

namespace kmsketch {

constexpr uint64_t MIN_WORDS = 64;
constexpr uint64_t MAX_WORDS = 1ull << 40;
constexpr uint64_t SALT = 0x9E3779B97F4A7C15ull;

// (the finalizer the counting table hashes with, device_common.h; restated: this header stands alone)
KM_SKETCH_HD inline uint64_t mix64(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return x;
}

KM_SKETCH_HD inline bool words_valid(uint64_t words) {
  return words >= MIN_WORDS && words <= MAX_WORDS && (words & (words - 1)) == 0;
}

// log2 of a valid word count (6 .. 40)
KM_SKETCH_HD inline uint32_t log2_words(uint64_t words) {
  uint32_t l = 0;
  while ((1ull << l) < words) ++l;
  return l;
}

// smallest power of two >= max(64, ceil(expected_distinct / 2)), capped at MAX_WORDS
KM_SKETCH_HD inline uint64_t sketch_words_for(uint64_t expected_distinct) {
  const uint64_t need = expected_distinct / 2 + (expected_distinct & 1);
  uint64_t w = MIN_WORDS;
  while (w < need && w < MAX_WORDS) w <<= 1;
  return w;
}

struct Slot {
  uint64_t word;
  uint32_t mask;
};

// shift = 64 - log2 W (24 .. 58)
KM_SKETCH_HD inline Slot slot_of(uint64_t key, uint32_t shift) {
  const uint64_t h = mix64(key ^ SALT);
  Slot s;
  s.word = h >> shift;
  s.mask = (1u << (h & 31u)) | (1u << ((h >> 5) & 31u)) | (1u << ((h >> 10) & 31u));
  return s;
}

KM_SKETCH_HD inline bool plane1_holds(uint64_t word, uint32_t mask) { return ((uint32_t)word & mask) == mask; }
KM_SKETCH_HD inline bool plane2_holds(uint64_t word, uint32_t mask) { return ((uint32_t)(word >> 32) & mask) == mask; }

// Note one key.  load(p) is the plain load, fetch_or(p, bits) returns the word as it was: on the device a vector load
// and a vector atomic, in tests/host/sketch_rule.cpp the sequential ones.
template <class Load, class FetchOr>
KM_SKETCH_HD inline void note(uint64_t* sketch, Slot s, Load load, FetchOr fetch_or) {
  uint64_t* p = sketch + s.word;
  if (plane2_holds(load(p), s.mask)) return;
  const uint64_t old = fetch_or(p, (uint64_t)s.mask);
  if (plane1_holds(old, s.mask)) (void)fetch_or(p, (uint64_t)s.mask << 32);
}

KM_SKETCH_HD inline bool admits(const uint64_t* sketch, Slot s) { return plane2_holds(sketch[s.word], s.mask); }

}  // namespace kmsketch
