// count_rule.cpp — km_amd/csrc/count_rule.h on the CPU (built with AddressSanitizer + UBSan by
// tests/test_count_rule_cpu.py): every lane of a padded piece played through kmcount::lane_walk and compared with a
// naive enumeration that asks, for every start, whether the k bytes are all ACGTacgt and lie before n, and takes the
// key from those k bytes alone.  Compared: the keys in the order the lanes hand them over (so also as a multiset), the
// windows of every lane, `bases`, `kmers`, and the sum of what the functor returned.
//   every k from 2 to 32, canonical or not; own_from 0, 1, k - 1, 31;
//   text lengths 0, 1, k - 1, k, k + 1, 31, 32, 33, 32 + k - 1, 63, 64, 65, 2 049, upper, lower and mixed case;
//   a non-base at each of the places of n_positions (tests/test_text_kernels_every_k.py), and other non-base bytes;
//   the piece lies in a heap block of exactly n + PAD bytes, so a load behind the padding is an error the sanitizer
//   names, and the padding holds base characters, so a walk that looks at or behind n finds windows that are not there;
//   k = 32: T x 40 (the key ~0), and keys at or above 2^63 on the forward strand only and on the reverse strand only.
// Prints "COUNT RULE OK" with the number of cases and exits 0, or names what failed and exits 1.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../km_amd/csrc/count_rule.h"

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

uint64_t rng_state = 0x13198A2E03707344ull;
uint64_t next_u64() {                                  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

enum Case { UPPER, LOWER, MIXED };
std::string random_bases(size_t n, Case how) {
  static const char both[] = "ACGTacgt";
  std::string s(n, 'A');
  for (char& ch : s) {
    const uint64_t r = next_u64();
    ch = both[(r & 3) + (how == LOWER || (how == MIXED && (r & 4)) ? 4 : 0)];
  }
  return s;
}

// ---- the naive side: nothing of count_rule.h or scan_rule.h
int digit(unsigned char ch) {                          // -1: no base
  switch (ch) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
  }
  return -1;
}

struct Naive {
  std::vector<uint64_t> keys;                          // by window start
  std::vector<uint32_t> per_lane;                      // windows that start in [32 g, 32 g + 32)
  uint64_t bases = 0;
};
Naive naive(const std::string& text, int k, int canonical, uint32_t own_from) {
  Naive out;
  const size_t n = text.size();
  out.per_lane.assign((n + 31) / 32, 0);
  for (size_t i = own_from; i < n; ++i) out.bases += digit((unsigned char)text[i]) >= 0 ? 1 : 0;
  for (size_t i = 0; i + (size_t)k <= n; ++i) {
    uint64_t fwd = 0, rev = 0;
    bool valid = true;
    for (int j = 0; j < k; ++j) {
      const int d = digit((unsigned char)text[i + j]);
      const int e = digit((unsigned char)text[i + k - 1 - j]);
      if (d < 0) { valid = false; break; }
      fwd = fwd * 4 + (uint64_t)d;                     // (k = 32: the 64 bits are full, nothing is lost)
      rev = rev * 4 + (uint64_t)(3 - (e < 0 ? 0 : e));
    }
    if (!valid) continue;
    out.keys.push_back(canonical && rev < fwd ? rev : fwd);
    ++out.per_lane[i / 32];
  }
  return out;
}

// what the functor returns for a key: three tallies of a byte each, as the kernels pack them
uint32_t tally_of(uint64_t key) { return 1u | (key == ~0ull ? 1u << 8 : 0u) | ((key & 1) ? 1u << 16 : 0u); }

// ---- one piece through the header's walk, lane by lane
uint64_t n_cases = 0;
void check_piece(const std::string& text, int k, int canonical, uint32_t own_from, const char* what) {
  const size_t n = text.size();
  std::vector<uint8_t> block(n + kmcount::PAD);        // exactly: the sanitizer guards its end
  std::memcpy(block.data(), text.data(), n);
  for (size_t i = n; i < block.size(); ++i) block[i] = (uint8_t)"TGCAtgca"[next_u64() & 7];
  const Naive want = naive(text, k, canonical, own_from);
  std::vector<uint64_t> got;
  uint64_t bases = 0, kmers = 0, sum = 0, want_sum = 0;
  for (uint64_t key : want.keys) want_sum += tally_of(key);
  for (uint64_t g = 0; g * kmcount::RUN < n; ++g) {
    const uint64_t s = g * kmcount::RUN;
    uint32_t w[16];
    for (uint32_t d = 0; d < 16; ++d) {                // (s + 64 <= n + 31 + 64 < n + PAD)
      const uint8_t* p = block.data() + s + 4 * d;
      w[d] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    }
    uint32_t lane_bases = 0, lane_kmers = 0;
    std::vector<uint64_t>* sink = &got;
    const uint32_t lane_sum = kmcount::lane_walk(w, (uint64_t)n, s, own_from, k, canonical, lane_bases, lane_kmers,
                                                 [=](uint64_t key) { sink->push_back(key); return tally_of(key); });
    CHECK(lane_kmers == want.per_lane[g], "%s k=%d canonical=%d n=%zu own_from=%u lane %llu: %u windows, %u expected", what, k,
          canonical, n, own_from, (unsigned long long)g, lane_kmers, want.per_lane[g]);
    bases += lane_bases;
    kmers += lane_kmers;
    sum += lane_sum;
  }
  CHECK(got == want.keys, "%s k=%d canonical=%d n=%zu own_from=%u: %zu keys, %zu expected, or other keys", what, k, canonical, n,
        own_from, got.size(), want.keys.size());
  std::vector<uint64_t> a = got, b = want.keys;        // (the multiset, should the order ever be let go)
  std::sort(a.begin(), a.end());
  std::sort(b.begin(), b.end());
  CHECK(a == b, "%s k=%d canonical=%d n=%zu own_from=%u: the multisets of keys differ", what, k, canonical, n, own_from);
  CHECK(bases == want.bases, "%s k=%d canonical=%d n=%zu own_from=%u: bases %llu, %llu expected", what, k, canonical, n, own_from,
        (unsigned long long)bases, (unsigned long long)want.bases);
  CHECK(kmers == want.keys.size(), "%s k=%d canonical=%d n=%zu own_from=%u: kmers %llu, %zu expected", what, k, canonical, n,
        own_from, (unsigned long long)kmers, want.keys.size());
  CHECK(sum == want_sum, "%s k=%d canonical=%d n=%zu own_from=%u: functor sum %llu, %llu expected", what, k, canonical, n, own_from,
        (unsigned long long)sum, (unsigned long long)want_sum);
  ++n_cases;
}

void check_text(const std::string& text, int k, const char* what) {
  const uint32_t froms[4] = {0u, 1u, (uint32_t)k - 1u, 31u};
  for (int canonical = 0; canonical < 2; ++canonical)
    for (uint32_t own_from : froms) check_piece(text, k, canonical, own_from, what);
}

std::string revcomp_text(const std::string& s) {
  std::string out(s.rbegin(), s.rend());
  for (char& ch : out) ch = "TGCA"[digit((unsigned char)ch)];
  return out;
}
}  // namespace

int main() {
  static_assert(kmcount::RUN == 32 && kmcount::PAD >= 2 * kmcount::RUN, "a lane loads 64 bytes from a start below n");
  for (int k = 2; k <= 32; ++k) {
    const size_t lengths[] = {0, 1, (size_t)k - 1, (size_t)k, (size_t)k + 1, 31, 32, 33, 32 + (size_t)k - 1, 63, 64, 65, 2049};
    for (size_t n : lengths) {
      check_text(random_bases(n, UPPER), k, "upper");
      check_text(random_bases(n, LOWER), k, "lower");
      check_text(random_bases(n, MIXED), k, "mixed");
    }
    // n_positions(k, length) of tests/test_text_kernels_every_k.py
    const size_t length = 64 + (size_t)k;
    std::vector<std::vector<size_t>> places = {{0}, {(size_t)k - 1}, {(size_t)k}, {31}, {32}, {length - 1}, {}};
    for (size_t p = 0; p < length; p += (size_t)k) places.back().push_back(p);
    for (const auto& at : places) {
      std::string s = random_bases(length, MIXED);
      for (size_t p : at) s[p] = 'N';
      check_text(s, k, "non-base");
    }
    std::string odd = random_bases(3 * length, MIXED);   // bytes that are no letters, one of them 'A' | 0x80
    const char others[] = {'-', '\0', '\xff', '*', '\n', '\xc1', 'U', '@', '`'};
    for (size_t i = 0; i < sizeof others; ++i) odd[(i + 1) * odd.size() / (sizeof others + 2)] = others[i];
    check_text(odd, k, "other bytes");
    check_text(std::string(2 * length, 'T'), k, "T run");
    check_text(std::string(2 * length, 'a'), k, "a run");
  }
  // k = 32: the key ~0, and keys whose top bit is set on one strand only
  check_text(std::string(40, 'T'), 32, "T x 40");
  CHECK(naive(std::string(40, 'T'), 32, 0, 0).keys == std::vector<uint64_t>(9, ~0ull), "T x 40 is nine windows of key ~0");
  const std::string fwd_top = "T" + std::string(30, 'C') + "T", rev_top = "A" + std::string(30, 'C') + "A";
  const uint64_t top = 1ull << 63;
  CHECK(naive(fwd_top, 32, 0, 0).keys.at(0) >= top && naive(fwd_top, 32, 1, 0).keys.at(0) < top, "forward strand at or above 2^63");
  CHECK(naive(rev_top, 32, 0, 0).keys.at(0) < top && naive(revcomp_text(rev_top), 32, 0, 0).keys.at(0) >= top &&
            naive(rev_top, 32, 1, 0).keys.at(0) < top,
        "reverse strand at or above 2^63");
  for (const std::string& mer : {fwd_top, rev_top}) {
    check_text(mer, 32, "top bit");
    check_text(random_bases(37, MIXED) + mer + random_bases(41, LOWER), 32, "top bit inside");
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("COUNT RULE OK %llu cases\n", (unsigned long long)n_cases);
  return 0;
}
