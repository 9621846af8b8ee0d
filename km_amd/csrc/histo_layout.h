// histo_layout.h — the bin rule of the count histogram, its argument checks and the two text writers (host only, no
// HIP; histo_host.h and tests/host/histo_layout.cpp).  DESIGN.md §10 "Histogram and statistics".
//
// The rule is that of `jellyfish histo -l low -h high -i increment` AS THIS PROJECT READS IT, not checked against a
// run of Jellyfish.  With 64-bit unsigned low <= high and inc >= 1:
//   base   = low > 1 ? (inc >= low ? 1 : low - inc) : 1
//   ceil   = high + inc
//   n_bins = (ceil + inc - base) / inc                      (integer division)
//   bin(c) = c < base ? 0 : c > ceil ? n_bins - 1 : (c - base) / inc
// and bin i is labelled base + i * inc.  For c <= ceil, (c - base) / inc <= (ceil - base) / inc = n_bins - 1, so
// every bin is inside the array; the largest label is base + (n_bins - 1) * inc <= ceil + inc = high + 2 inc, which
// the checks keep inside 64 bits.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

namespace kmhisto {

constexpr uint64_t MAX_BINS = 1ull << 24;

struct Layout {
  uint64_t low, high, inc;
  uint64_t base, ceil, n_bins;
};

// 0, or why (low, high, inc) is refused, as text in msg[cap] naming the value
inline int make(uint64_t low, uint64_t high, uint64_t inc, Layout* out, char* msg, size_t cap) {
  if (inc == 0) { snprintf(msg, cap, "increment 0"); return 1; }
  if (low > high) { snprintf(msg, cap, "low %llu above high %llu", (unsigned long long)low, (unsigned long long)high); return 1; }
  if (inc > (~0ull - high) / 2) {
    snprintf(msg, cap, "high %llu + 2 * increment %llu does not fit 64 bits", (unsigned long long)high, (unsigned long long)inc);
    return 1;
  }
  Layout l;
  l.low = low; l.high = high; l.inc = inc;
  l.base = low > 1 ? (inc >= low ? 1 : low - inc) : 1;
  l.ceil = high + inc;
  l.n_bins = (l.ceil + inc - l.base) / inc;
  if (l.n_bins > MAX_BINS) {
    snprintf(msg, cap, "%llu bins, at most %llu", (unsigned long long)l.n_bins, (unsigned long long)MAX_BINS);
    return 1;
  }
  *out = l;
  return 0;
}

inline uint64_t bin(const Layout& l, uint64_t c) {
  return c < l.base ? 0 : c > l.ceil ? l.n_bins - 1 : (c - l.base) / l.inc;
}

// decimal digits of v at p (no terminator) -> how many
inline size_t put_u64(char* p, uint64_t v) {
  char tmp[20];
  size_t n = 0;
  do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
  for (size_t i = 0; i < n; ++i) p[i] = tmp[n - 1 - i];
  return n;
}
inline size_t len_u64(uint64_t v) {
  size_t n = 1;
  while (v >= 10) { v /= 10; ++n; }
  return n;
}

// "<label> <n>\n" per bin with n > 0 (every bin with full).  *len = the bytes of the whole text; they are written to
// out[cap] only when they fit (returns false otherwise, out untouched).  out == nullptr asks for *len alone.
inline bool write_histo(uint64_t base, uint64_t inc, const uint64_t* bins, uint64_t n_bins, bool full, char* out,
                        uint64_t cap, uint64_t* len) {
  uint64_t need = 0;
  for (uint64_t i = 0; i < n_bins; ++i)
    if (full || bins[i]) need += len_u64(base + i * inc) + 1 + len_u64(bins[i]) + 1;
  *len = need;
  if (!out) return true;
  if (cap < need) return false;
  char* p = out;
  for (uint64_t i = 0; i < n_bins; ++i) {
    if (!full && !bins[i]) continue;
    p += put_u64(p, base + i * inc);
    *p++ = ' ';
    p += put_u64(p, bins[i]);
    *p++ = '\n';
  }
  return true;
}

// the block of `jellyfish stats`, labels padded to one column
inline bool write_stats(uint64_t unique, uint64_t distinct, uint64_t total, uint64_t max_count, char* out, uint64_t cap,
                        uint64_t* len) {
  static const char* const label[4] = {"Unique:    ", "Distinct:  ", "Total:     ", "Max_count: "};
  const uint64_t v[4] = {unique, distinct, total, max_count};
  uint64_t need = 0;
  for (int i = 0; i < 4; ++i) need += strlen(label[i]) + len_u64(v[i]) + 1;
  *len = need;
  if (!out) return true;
  if (cap < need) return false;
  char* p = out;
  for (int i = 0; i < 4; ++i) {
    const size_t n = strlen(label[i]);
    memcpy(p, label[i], n);
    p += n;
    p += put_u64(p, v[i]);
    *p++ = '\n';
  }
  return true;
}

}  // namespace kmhisto
