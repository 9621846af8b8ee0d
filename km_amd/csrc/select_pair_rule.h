// select_pair_rule.h — which pairs of two pieces of 4-line FASTQ text are kept: the score of a pair, its keep, the two
// lengths a kept pair adds to the outputs, how much of a piece R pairs consume, and the comparison of two mates' names
// (plain C++17, no HIP headers; __host__ __device__ under hipcc, so select_pair_kernel.h, select_pair_host.h and
// tests/host/select_pair_rule.cpp run the same code).  DESIGN.md §10 "Select, pairs".
//
// The rule (include/kmgpu.h states it for the callers):
//   Record r of mate 1 and record r of mate 2 are pair r.  h1, h2: their hits as select_rule.h defines them.
//   score = max(h1, h2) (any), min(h1, h2) (both) or h1 + h2 saturating at 2^32 - 1 (sum);
//   keep = (score >= min_hits) != invert; a pair is kept or dropped whole.
//   The name of a record: the bytes of its header line behind '@' up to the first space, tab, '\r' or '\n'; a name of
//   at least two bytes that ends in "/1" or "/2" loses those two.  Mates agree iff their names are byte-equal.
#pragma once
#include "select_rule.h"

namespace kmpair {

enum : uint32_t { RULE_ANY = 0, RULE_BOTH = 1, RULE_SUM = 2, RULE_COUNT = 3 };

KM_SCAN_HD inline uint32_t score(uint32_t h1, uint32_t h2, uint32_t rule) {
  if (rule == RULE_BOTH) return h1 < h2 ? h1 : h2;
  if (rule == RULE_SUM) {
    const uint32_t s = h1 + h2;
    return s < h1 ? 0xFFFFFFFFu : s;
  }
  return h1 > h2 ? h1 : h2;
}
KM_SCAN_HD inline bool keep(uint32_t h1, uint32_t h2, uint32_t rule, uint32_t min_hits, bool invert) {
  return kmsel::keep(score(h1, h2, rule), min_hits, invert);
}

// the bytes pair r adds to the two outputs: both records' lengths if it is kept, else 0 and 0
struct Lens {
  uint32_t len1, len2;
  bool kept;
};
KM_SCAN_HD inline Lens pair_lens(const uint32_t* line_start1, uint32_t n1, const uint32_t* line_start2, uint32_t n2,
                                 uint32_t r, uint32_t h1, uint32_t h2, uint32_t rule, uint32_t min_hits, bool invert) {
  if (!keep(h1, h2, rule, min_hits, invert)) return Lens{0u, 0u, false};
  return Lens{kmsel::record_end(line_start1, r, n1) - kmsel::record_begin(line_start1, r),
              kmsel::record_end(line_start2, r, n2) - kmsel::record_begin(line_start2, r), true};
}

// pairs of two pieces of records1 and records2 records
KM_SCAN_HD inline uint32_t pair_count(uint32_t records1, uint32_t records2) { return records1 < records2 ? records1 : records2; }
// where record n_pairs of a piece of n bytes begins: the bytes its first n_pairs records take
KM_SCAN_HD inline uint32_t consumed(const uint32_t* line_start, uint32_t n_pairs, uint32_t n) {
  return n_pairs ? kmsel::record_end(line_start, n_pairs - 1u, n) : 0u;
}

// ---- names
KM_SCAN_HD inline bool name_ends(uint32_t ch) { return ch == ' ' || ch == '\t' || ch == '\r' || ch == '\n'; }
// byte(i): byte i < n of the piece.  The name of the record whose header begins at `header`: [begin, begin + len)
struct Name {
  uint32_t begin, len;
};
template <typename Byte>
KM_SCAN_HD inline Name name_of(Byte& byte, uint32_t header, uint32_t n) {
  const uint32_t begin = header + 1u < n ? header + 1u : n;
  uint32_t end = begin;
  while (end < n && !name_ends(byte(end))) ++end;
  uint32_t len = end - begin;
  if (len >= 2u && byte(end - 2u) == '/' && (byte(end - 1u) == '1' || byte(end - 1u) == '2')) len -= 2u;
  return Name{begin, len};
}
template <typename Byte1, typename Byte2>
KM_SCAN_HD inline bool names_agree(Byte1& byte1, uint32_t header1, uint32_t n1, Byte2& byte2, uint32_t header2, uint32_t n2) {
  const Name a = name_of(byte1, header1, n1), b = name_of(byte2, header2, n2);
  if (a.len != b.len) return false;
  for (uint32_t i = 0; i < a.len; ++i)
    if (byte1(a.begin + i) != byte2(b.begin + i)) return false;
  return true;
}

}  // namespace kmpair
