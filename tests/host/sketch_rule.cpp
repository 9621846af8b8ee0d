// sketch_rule.cpp — km_amd/csrc/sketch_rule.h on the CPU (built with AddressSanitizer + UBSan by
// tests/test_count_solid_cpu.py): note and admit played sequentially on a host array of exactly W words, so a word
// index past the sketch is an error the sanitizer names.
//   every key noted twice is admitted, in whatever order the notes of different keys interleave;
//   a key never noted is admitted iff plane 2 of its word covers its mask, and one whose mask is not covered is not;
//   a key noted once in a sketch of its own is not admitted;
//   masks whose three bit positions coincide (one or two bits) are handled like any other;
//   the sizing rule and the range of valid sizes.
// Prints "SKETCH RULE OK" and exits 0, or names what failed and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../km_amd/csrc/sketch_rule.h"

namespace {
int failures = 0;
#define CHECK(cond, ...)                                      \
  do {                                                        \
    if (!(cond)) {                                            \
      std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                               \
      std::printf("\n");                                      \
      if (++failures > 20) std::exit(1);                      \
    }                                                         \
  } while (0)

uint64_t rng_state = 0x243F6A8885A308D3ull;
uint64_t next_u64() {                                  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

int popcount32(uint32_t v) {
  int n = 0;
  for (; v; v &= v - 1) ++n;
  return n;
}

struct Sketch {
  std::vector<uint64_t> w;
  uint32_t shift;
  uint64_t atomics = 0;
  explicit Sketch(uint64_t words) : w(words, 0), shift(64u - kmsketch::log2_words(words)) {}
  kmsketch::Slot slot(uint64_t key) const {
    const kmsketch::Slot s = kmsketch::slot_of(key, shift);
    CHECK(s.word < w.size(), "word %llu of %llu", (unsigned long long)s.word, (unsigned long long)w.size());
    CHECK(popcount32(s.mask) >= 1 && popcount32(s.mask) <= 3, "mask %08x", s.mask);
    return s;
  }
  void note(uint64_t key) {
    kmsketch::note(
        w.data(), slot(key), [](uint64_t* p) { return *p; },
        [this](uint64_t* p, uint64_t bits) {
          const uint64_t old = *p;
          *p |= bits;
          ++atomics;
          return old;
        });
  }
  bool admits(uint64_t key) const { return kmsketch::admits(w.data(), slot(key)); }
  bool covered(uint64_t key) const {                    // by plane 2, from the definition
    const kmsketch::Slot s = kmsketch::slot_of(key, shift);
    return ((w[s.word] >> 32) & s.mask) == s.mask;
  }
};

void twice_is_admitted(uint64_t words, size_t n_keys, int order) {
  Sketch sk(words);
  std::vector<uint64_t> keys(n_keys);
  for (auto& k : keys) k = next_u64();
  keys[0] = 0;
  keys[1] = (1ull << 62) - 1;
  keys[2] = ~0ull - 1;
  if (order == 0) {                                    // a a b b ...
    for (uint64_t k : keys) { sk.note(k); sk.note(k); }
  } else if (order == 1) {                             // a b c ... a b c ...
    for (uint64_t k : keys) sk.note(k);
    for (uint64_t k : keys) sk.note(k);
  } else {                                             // a b c ... then backwards, and a third time for some
    for (uint64_t k : keys) sk.note(k);
    for (size_t i = keys.size(); i-- > 0;) sk.note(keys[i]);
    for (size_t i = 0; i < keys.size(); i += 3) sk.note(keys[i]);
  }
  for (uint64_t k : keys) CHECK(sk.admits(k), "W=%llu order %d key %016llx", (unsigned long long)words, order, (unsigned long long)k);
  // keys never noted: admitted iff covered, and with a sparse sketch most are not
  size_t strangers = 0, admitted = 0;
  for (size_t i = 0; i < 4 * n_keys; ++i) {
    const uint64_t k = next_u64();
    ++strangers;
    CHECK(sk.admits(k) == sk.covered(k), "W=%llu stranger %016llx", (unsigned long long)words, (unsigned long long)k);
    admitted += sk.admits(k) ? 1 : 0;
  }
  if (words >= 16 * n_keys) CHECK(admitted * 10 < strangers, "%zu of %zu strangers admitted", admitted, strangers);
}

void once_is_not_admitted() {
  for (int i = 0; i < 1000; ++i) {
    Sketch sk(64);
    const uint64_t k = next_u64();
    sk.note(k);
    CHECK(!sk.admits(k), "key %016llx admitted after one note", (unsigned long long)k);
    CHECK(sk.atomics == 1, "%llu atomics for a first note", (unsigned long long)sk.atomics);
    const kmsketch::Slot s = sk.slot(k);
    CHECK(sk.w[s.word] == (uint64_t)s.mask, "word %016llx mask %08x", (unsigned long long)sk.w[s.word], s.mask);
    sk.note(k);
    CHECK(sk.admits(k), "key %016llx", (unsigned long long)k);
    CHECK(sk.atomics == 3, "%llu atomics for two notes", (unsigned long long)sk.atomics);
    CHECK(sk.w[s.word] == (((uint64_t)s.mask << 32) | s.mask), "word %016llx", (unsigned long long)sk.w[s.word]);
    sk.note(k);                                        // the third occurrence is skipped on the plain load
    CHECK(sk.atomics == 3, "%llu atomics after a skipped note", (unsigned long long)sk.atomics);
  }
}

// A stranger whose mask is covered bit by bit by two other keys noted twice is admitted; one bit short, it is not.
void covered_and_uncovered() {
  Sketch sk(64);
  const kmsketch::Slot a = sk.slot(12345);
  sk.w[a.word] = (uint64_t)(a.mask & (a.mask - 1)) << 32;      // plane 2 lacks the mask's lowest bit
  if (popcount32(a.mask) > 1) CHECK(!sk.admits(12345), "admitted one bit short");
  sk.w[a.word] |= (uint64_t)a.mask << 32;
  CHECK(sk.admits(12345), "not admitted when covered");
  sk.w[a.word] = a.mask;                                        // plane 1 alone admits nothing
  CHECK(!sk.admits(12345), "admitted from plane 1");
}

void coinciding_bits() {
  int seen[4] = {0, 0, 0, 0};
  for (uint64_t k = 0; (seen[1] < 3 || seen[2] < 50) && k < (1ull << 22); ++k) {
    Sketch sk(64);
    const kmsketch::Slot s = sk.slot(k);
    const int bits = popcount32(s.mask);
    if (bits == 3 && seen[3] > 100) continue;
    ++seen[bits];
    const uint64_t h = kmsketch::mix64(k ^ kmsketch::SALT);
    const uint32_t want = (1u << (h & 31)) | (1u << ((h >> 5) & 31)) | (1u << ((h >> 10) & 31));
    CHECK(s.mask == want && s.word == h >> 58, "key %llu", (unsigned long long)k);
    sk.note(k);
    CHECK(!sk.admits(k), "key %llu (%d bits) admitted after one note", (unsigned long long)k, bits);
    sk.note(k);
    CHECK(sk.admits(k), "key %llu (%d bits) not admitted after two notes", (unsigned long long)k, bits);
  }
  CHECK(seen[1] >= 3 && seen[2] >= 50 && seen[3] >= 100, "masks of 1 / 2 / 3 bits: %d %d %d", seen[1], seen[2], seen[3]);
}

void sizing() {
  using kmsketch::sketch_words_for;
  using kmsketch::words_valid;
  CHECK(sketch_words_for(0) == 64 && sketch_words_for(1) == 64 && sketch_words_for(128) == 64, "small");
  CHECK(sketch_words_for(129) == 128 && sketch_words_for(256) == 128 && sketch_words_for(257) == 256, "edges");
  CHECK(sketch_words_for(22000) == 16384, "22000 -> %llu", (unsigned long long)sketch_words_for(22000));
  CHECK(sketch_words_for(1ull << 41) == 1ull << 40 && sketch_words_for(~0ull) == 1ull << 40, "cap");
  CHECK(!words_valid(0) && !words_valid(32) && words_valid(64) && !words_valid(96) && words_valid(1ull << 40) &&
            !words_valid(1ull << 41) && !words_valid((1ull << 40) - 1),
        "words_valid");
  CHECK(kmsketch::log2_words(64) == 6 && kmsketch::log2_words(1ull << 40) == 40, "log2_words");
  // the widest sketch: the word index stays below 2^40 (the array is not allocated)
  for (int i = 0; i < 10000; ++i) CHECK(kmsketch::slot_of(next_u64(), 24).word < (1ull << 40), "word past 2^40");
}
}  // namespace

int main() {
  for (int order = 0; order < 3; ++order) {
    twice_is_admitted(64, 10000, order);               // saturated: every word takes ~156 keys
    twice_is_admitted(1 << 10, 3000, order);
    twice_is_admitted(1 << 16, 3000, order);           // sparse
  }
  once_is_not_admitted();
  covered_and_uncovered();
  coinciding_bits();
  sizing();
  if (failures) return 1;
  std::printf("SKETCH RULE OK\n");
  return 0;
}
