// dump_text.h — the text of one record as `dump` and `query` print it: the three formats, the line length, the filter
// and the writer of one line (plain C++17, no HIP headers; __host__ __device__ under hipcc, so dump_kernel.h and
// tests/host/dump_text.cpp run the same code).  DESIGN.md §10 "Dump and query".
//
// The rule is that of `jellyfish dump [-c [-t]] [-L lower] [-U upper]` and of `jellyfish query` AS THIS PROJECT READS
// THEM, not checked against a run of Jellyfish:
//   KM_DUMP_FASTA   ">COUNT\nMER\n"      (the default of `jellyfish dump`)
//   KM_DUMP_COLUMN  "MER COUNT\n"        (-c; also every line of `query`)
//   KM_DUMP_TAB     "MER\tCOUNT\n"       (-c -t)
// MER: k letters, ACGT for 0..3, the first base from the most significant used bit pair (bits 2k-1, 2k-2); bits above
// 2k are never looked at.  COUNT: decimal, no padding, "0" for zero.  A record is printed iff lower <= count <= upper;
// lower > upper prints nothing.  Nothing is sorted: lines come in the order of the records.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef KM_DUMP_FASTA
#define KM_DUMP_FASTA 0
#define KM_DUMP_COLUMN 1
#define KM_DUMP_TAB 2
#endif

#if defined(__HIPCC__)
#define KM_DUMP_HD __host__ __device__
#else
#define KM_DUMP_HD
#endif

namespace kmdump {

constexpr uint32_t MAX_DIGITS = 10;                    // of a 32-bit count
// the longest line of any format: FASTA with ten digits, '>' + 10 + '\n' + k + '\n'
KM_DUMP_HD inline uint32_t worst_line(int k) { return (uint32_t)k + 13u; }

KM_DUMP_HD inline bool format_known(int fmt) { return fmt == KM_DUMP_FASTA || fmt == KM_DUMP_COLUMN || fmt == KM_DUMP_TAB; }

KM_DUMP_HD inline bool kept(uint32_t count, uint32_t lower, uint32_t upper) { return count >= lower && count <= upper; }

// decimal digits of c: 1..10
KM_DUMP_HD inline uint32_t digits(uint32_t c) {
  return 1u + (c >= 10u) + (c >= 100u) + (c >= 1000u) + (c >= 10000u) + (c >= 100000u) + (c >= 1000000u) +
         (c >= 10000000u) + (c >= 100000000u) + (c >= 1000000000u);
}

// bytes of the line of a record with a count of n_digits digits
KM_DUMP_HD inline uint32_t line_len(int k, uint32_t n_digits, int fmt) {
  return (uint32_t)k + n_digits + (fmt == KM_DUMP_FASTA ? 3u : 2u);
}

// two bits -> letter ("ACGT" packed into one word: no table in memory on either side)
KM_DUMP_HD inline char letter(uint32_t two_bits) { return (char)((0x54474341u >> (8u * (two_bits & 3u))) & 0xFFu); }

KM_DUMP_HD inline void put_mer(char* p, uint64_t key, int k) {
  for (int j = 0; j < k; ++j) p[j] = letter((uint32_t)(key >> (2 * (k - 1 - j))));
}

// the n_digits = digits(c) digits of c at p
KM_DUMP_HD inline void put_count(char* p, uint32_t c, uint32_t n_digits) {
  for (uint32_t d = n_digits; d-- > 0;) {
    p[d] = (char)('0' + c % 10u);
    c /= 10u;
  }
}

// The line of (key, count) at p, which has room for line_len(k, digits(count), fmt) bytes: exactly those are written.
// Returns that length.  (The filter is the caller's.)
KM_DUMP_HD inline uint32_t put_record(char* p, uint64_t key, uint32_t count, int k, int fmt) {
  const uint32_t nd = digits(count);
  if (fmt == KM_DUMP_FASTA) {
    p[0] = '>';
    put_count(p + 1, count, nd);
    p[1 + nd] = '\n';
    put_mer(p + 2 + nd, key, k);
    p[2 + nd + k] = '\n';
  } else {
    put_mer(p, key, k);
    p[k] = fmt == KM_DUMP_TAB ? '\t' : ' ';
    put_count(p + k + 1, count, nd);
    p[k + 1 + nd] = '\n';
  }
  return line_len(k, nd, fmt);
}

}  // namespace kmdump
