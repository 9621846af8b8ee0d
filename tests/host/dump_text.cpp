// CPU-only driver for km_amd/csrc/dump_text.h (the text of one record of `dump` / `query`: line length, digits, the
// writer of one line), built with -fsanitize=address,undefined by tests/test_dump_cpu.py:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o dump_text tests/host/dump_text.cpp
// For every k in 2..32, every digit count 1..10 and the three formats it writes records with the header's host writer
// and compares them with snprintf over a mer spelled out base by base.  Every record goes into a heap buffer of
// EXACTLY its length between guard bytes, so a byte too far is a heap overflow the sanitizer reports, and a byte too
// few leaves a guard pattern in the line.  The worst case k + 13 is checked for every k.  Prints "DUMP TEXT OK".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../km_amd/csrc/dump_text.h"

#define REQUIRE(cond)                                                                  \
  do {                                                                                 \
    if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

static std::string model(uint64_t key, uint32_t count, int k, int fmt) {
  std::string mer;
  for (int j = 0; j < k; ++j) mer += "ACGT"[(key >> (2 * (k - 1 - j))) & 3];
  char buf[128];
  if (fmt == KM_DUMP_FASTA) snprintf(buf, sizeof buf, ">%u\n%s\n", count, mer.c_str());
  else snprintf(buf, sizeof buf, "%s%c%u\n", mer.c_str(), fmt == KM_DUMP_TAB ? '\t' : ' ', count);
  return buf;
}

static int check_record(uint64_t key, uint32_t count, int k, int fmt) {
  const std::string want = model(key, count, k, fmt);
  char digits[16];
  const uint32_t nd = (uint32_t)snprintf(digits, sizeof digits, "%u", count);
  REQUIRE(kmdump::digits(count) == nd);
  const uint32_t len = kmdump::line_len(k, nd, fmt);
  REQUIRE(len == want.size());
  REQUIRE(len <= kmdump::worst_line(k));
  // exactly len bytes on the heap, then the same inside guards that must survive
  std::vector<char> exact(len);
  REQUIRE(kmdump::put_record(exact.data(), key, count, k, fmt) == len);
  REQUIRE(memcmp(exact.data(), want.data(), len) == 0);
  std::vector<char> guarded(len + 16, (char)0x5A);
  REQUIRE(kmdump::put_record(guarded.data() + 8, key, count, k, fmt) == len);
  REQUIRE(memcmp(guarded.data() + 8, want.data(), len) == 0);
  for (int g = 0; g < 8; ++g) REQUIRE(guarded[g] == (char)0x5A && guarded[8 + len + g] == (char)0x5A);
  return 0;
}

int main() {
  // the first and the last count of every digit length
  std::vector<uint32_t> counts = {0};
  uint32_t p = 1;
  for (int d = 1; d <= 10; ++d) {
    counts.push_back(p);
    counts.push_back(d < 10 ? p * 10 - 1 : 0xFFFFFFFFu);
    if (d < 10) p *= 10;
  }
  counts.push_back(4000000000u);
  bool seen[11] = {false};
  for (uint32_t c : counts) seen[kmdump::digits(c)] = true;
  for (int d = 1; d <= 10; ++d) REQUIRE(seen[d]);
  REQUIRE(kmdump::MAX_DIGITS == 10);

  uint64_t x = 0x9E3779B97F4A7C15ull;
  for (int k = 2; k <= 32; ++k) {
    const uint64_t mask = k == 32 ? ~0ull : (1ull << (2 * k)) - 1;
    REQUIRE(kmdump::worst_line(k) == (uint32_t)k + 13);
    REQUIRE(kmdump::line_len(k, 10, KM_DUMP_FASTA) == kmdump::worst_line(k));     // the bound is reached
    REQUIRE(kmdump::line_len(k, 10, KM_DUMP_COLUMN) == (uint32_t)k + 12);
    for (int fmt = 0; fmt < 3; ++fmt)
      for (uint32_t c : counts) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        const uint64_t keys[4] = {0, mask, x & mask, x | ~mask};                  // bits above 2k are not looked at
        for (uint64_t key : keys) {
          if (check_record(key, c, k, fmt)) return 1;
          REQUIRE(model(key, c, k, fmt) == model(key & mask, c, k, fmt));
        }
      }
  }
  // the literal cases of the rule
  REQUIRE(model(0x7, 9, 2, KM_DUMP_COLUMN) == "CT 9\n");
  {
    char buf[64];
    REQUIRE(kmdump::put_record(buf, 0x7, 10, 2, KM_DUMP_FASTA) == 7 && memcmp(buf, ">10\nCT\n", 7) == 0);
    REQUIRE(kmdump::put_record(buf, ~0ull, 0, 32, KM_DUMP_TAB) == 35 &&
            memcmp(buf, "TTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTT\t0\n", 35) == 0);
  }
  // the filter
  REQUIRE(kmdump::kept(0, 0, 0xFFFFFFFFu) && !kmdump::kept(0, 1, 0xFFFFFFFFu) && kmdump::kept(5, 5, 5));
  REQUIRE(!kmdump::kept(5, 6, 4) && !kmdump::kept(4, 6, 4) && !kmdump::kept(6, 6, 4));
  REQUIRE(kmdump::format_known(0) && kmdump::format_known(2) && !kmdump::format_known(3) && !kmdump::format_known(-1));
  printf("DUMP TEXT OK\n");
  return 0;
}
