// CPU-only driver for km_amd/csrc/histo_layout.h (the bin rule of km_counter_histo / km_jf_histo, its argument checks
// and the two text writers), built with -fsanitize=address,undefined by tests/test_histo_cpu.py:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o histo_layout \
//       tests/host/histo_layout.cpp && ./histo_layout
// For a grid of small (low, high, inc) it compares base / ceil / n_bins and bin(c), c = 0 .. ceil + 3 inc, against a
// brute-force restatement: the bins are walked label by label and a count goes to the last one whose label it
// reaches.  The bin arrays are heap buffers of EXACTLY n_bins, the text buffers of exactly the length asked for, so
// an index or a byte too far is a heap overflow the sanitizer reports.  Prints "LAYOUT OK".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../km_amd/csrc/histo_layout.h"

#define REQUIRE(cond)                                                                  \
  do {                                                                                 \
    if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

static int check_rule(uint64_t low, uint64_t high, uint64_t inc) {
  kmhisto::Layout l;
  char why[160];
  REQUIRE(kmhisto::make(low, high, inc, &l, why, sizeof why) == 0);
  // the definition, written out again
  uint64_t base = 1;
  if (low > 1) base = inc >= low ? 1 : low - inc;
  const uint64_t ceil = high + inc;
  uint64_t n_bins = 0;
  while ((n_bins + 1) * inc <= ceil + inc - base) ++n_bins;             // floor((ceil + inc - base) / inc)
  REQUIRE(l.base == base && l.ceil == ceil && l.n_bins == n_bins && n_bins >= 1);
  REQUIRE(base >= 1 && base <= (low > 1 ? low : 1));
  std::vector<uint64_t> hits(n_bins, 0);                                // exactly n_bins
  uint64_t last = 0;
  for (uint64_t c = 0; c <= ceil + 3 * inc; ++c) {
    uint64_t want;
    if (c < base) want = 0;
    else if (c > ceil) want = n_bins - 1;
    else {
      want = 0;
      while (base + (want + 1) * inc <= c) ++want;                      // the last bin whose label c reaches
    }
    const uint64_t got = kmhisto::bin(l, c);
    REQUIRE(got == want && got < n_bins);
    REQUIRE(got >= last);                                               // monotone in c
    last = got;
    ++hits[got];
  }
  REQUIRE(last == n_bins - 1);
  for (uint64_t i = 0; i < n_bins; ++i) REQUIRE(hits[i] >= 1);          // no bin is unreachable
  REQUIRE(kmhisto::bin(l, ~0ull) == n_bins - 1);
  return 0;
}

static int check_refusals() {
  kmhisto::Layout l;
  char why[160];
  REQUIRE(kmhisto::make(1, 10, 0, &l, why, sizeof why) && strstr(why, "increment 0"));
  REQUIRE(kmhisto::make(11, 10, 1, &l, why, sizeof why) && strstr(why, "11") && strstr(why, "10"));
  REQUIRE(kmhisto::make(1, ~0ull - 1, 1, &l, why, sizeof why) && strstr(why, "18446744073709551614"));
  REQUIRE(kmhisto::make(1, 1ull << 63, 1ull << 62, &l, why, sizeof why) && strstr(why, "4611686018427387904"));
  REQUIRE(kmhisto::make(1, ~0ull - 2, 1, &l, why, sizeof why) && strstr(why, "bins"));    // fits 64 bits, too many bins
  REQUIRE(kmhisto::make(1, (1ull << 24) - 1, 1, &l, why, sizeof why) == 0 && l.n_bins == 1ull << 24);
  REQUIRE(kmhisto::make(1, 1ull << 24, 1, &l, why, sizeof why) && strstr(why, "16777217"));
  REQUIRE(kmhisto::make(1, ~0ull - 4, 2, &l, why, sizeof why) && strstr(why, "bins"));
  REQUIRE(kmhisto::make(~0ull / 2, ~0ull / 2, ~0ull / 4, &l, why, sizeof why) == 0 && l.n_bins >= 1 &&
          kmhisto::bin(l, ~0ull) == l.n_bins - 1 && kmhisto::bin(l, 0) == 0);
  // the cases the header quotes
  REQUIRE(kmhisto::make(1, 10000, 1, &l, why, sizeof why) == 0 && l.base == 1 && l.n_bins == 10001);
  REQUIRE(kmhisto::bin(l, 10001) == 10000 && kmhisto::bin(l, 10002) == 10000 && kmhisto::bin(l, 10000) == 9999);
  REQUIRE(kmhisto::make(5, 20, 5, &l, why, sizeof why) == 0 && l.base == 1 && l.n_bins == 5);
  REQUIRE(kmhisto::make(100, 200, 10, &l, why, sizeof why) == 0 && l.base == 90 && l.n_bins == 13);
  REQUIRE(kmhisto::make(1, 1, 1, &l, why, sizeof why) == 0 && l.base == 1 && l.n_bins == 2);
  return 0;
}

static int check_text() {
  const uint64_t bins[5] = {3, 0, 18446744073709551615ull, 0, 10};
  uint64_t len = 0;
  REQUIRE(kmhisto::write_histo(90, 10, bins, 5, false, nullptr, 0, &len));
  const std::string want = "90 3\n110 18446744073709551615\n130 10\n";
  REQUIRE(len == want.size());
  std::vector<char> out(len);                                           // exactly the length asked for
  REQUIRE(kmhisto::write_histo(90, 10, bins, 5, false, out.data(), out.size(), &len));
  REQUIRE(std::string(out.data(), out.size()) == want);
  std::vector<char> small(len - 1, 'x');
  REQUIRE(!kmhisto::write_histo(90, 10, bins, 5, false, small.data(), small.size(), &len) && len == want.size());
  for (char ch : small) REQUIRE(ch == 'x');                             // refused: nothing written
  const std::string full = "90 3\n100 0\n110 18446744073709551615\n120 0\n130 10\n";
  REQUIRE(kmhisto::write_histo(90, 10, bins, 5, true, nullptr, 0, &len) && len == full.size());
  out.assign(len, 0);
  REQUIRE(kmhisto::write_histo(90, 10, bins, 5, true, out.data(), out.size(), &len));
  REQUIRE(std::string(out.data(), out.size()) == full);
  const uint64_t zeros[3] = {0, 0, 0};
  REQUIRE(kmhisto::write_histo(1, 1, zeros, 3, false, nullptr, 0, &len) && len == 0);
  REQUIRE(kmhisto::write_histo(1, 1, zeros, 3, false, out.data(), 0, &len) && len == 0);
  REQUIRE(kmhisto::write_histo(1, 1, nullptr, 0, true, nullptr, 0, &len) && len == 0);
  // labels up to the largest the checks allow
  kmhisto::Layout l;
  char why[160];
  REQUIRE(kmhisto::make(~0ull - 2, ~0ull - 2, 1, &l, why, sizeof why) == 0 && l.n_bins == 3);
  const uint64_t ones[3] = {1, 1, 1};
  const std::string top = "18446744073709551612 1\n18446744073709551613 1\n18446744073709551614 1\n";
  REQUIRE(kmhisto::write_histo(l.base, l.inc, ones, 3, false, nullptr, 0, &len) && len == top.size());
  out.assign(len, 0);
  REQUIRE(kmhisto::write_histo(l.base, l.inc, ones, 3, false, out.data(), out.size(), &len));
  REQUIRE(std::string(out.data(), out.size()) == top);

  const std::string stats = "Unique:    7\nDistinct:  4294967296\nTotal:     18446744073709551615\nMax_count: 0\n";
  REQUIRE(kmhisto::write_stats(7, 1ull << 32, ~0ull, 0, nullptr, 0, &len) && len == stats.size());
  out.assign(len, 0);
  REQUIRE(kmhisto::write_stats(7, 1ull << 32, ~0ull, 0, out.data(), out.size(), &len));
  REQUIRE(std::string(out.data(), out.size()) == stats);
  small.assign(len - 1, 'x');
  REQUIRE(!kmhisto::write_stats(7, 1ull << 32, ~0ull, 0, small.data(), small.size(), &len));
  for (char ch : small) REQUIRE(ch == 'x');
  return 0;
}

int main() {
  const uint64_t lows[] = {1, 2, 3, 5, 7, 12, 30};
  const uint64_t spans[] = {0, 1, 2, 5, 11, 40};
  const uint64_t incs[] = {1, 2, 3, 5, 7, 12, 13, 50};
  for (uint64_t low : lows)
    for (uint64_t span : spans)
      for (uint64_t inc : incs)
        if (check_rule(low, low + span, inc)) {
          fprintf(stderr, "at low=%llu high=%llu inc=%llu\n", (unsigned long long)low, (unsigned long long)(low + span),
                  (unsigned long long)inc);
          return 1;
        }
  if (check_refusals()) return 1;
  if (check_text()) return 1;
  printf("LAYOUT OK\n");
  return 0;
}
