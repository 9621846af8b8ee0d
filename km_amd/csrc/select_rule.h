// select_rule.h — which records of a piece of 4-line FASTQ text are kept, and where their bytes go: record bounds from
// the line table, the hit walk of one lane, the sizes, and the assembly of one 16-byte word of the dense output (plain
// C++17, no HIP headers; __host__ __device__ under hipcc, so select_kernel.h, select_host.h and
// tests/host/select_rule.cpp run the same code).  DESIGN.md §10 "Select".
//
// The rule (include/kmgpu.h states it for the callers):
//   A piece is text[0 .. n) of whole records with the line table of fastq_kernel.h: line l is
//   [line_start[l], line_start[l + 1]), its newline included; line_start[L] of a piece whose last byte is no newline
//   is n + 1.  Record r is lines 4r .. 4r + 3, its bytes are [line_start[4r], min(line_start[4r + 4], n)).
//   hits(r): the windows of k consecutive bytes of the record's sequence line that are all ACGTacgt (after quality
//   masking) and whose k-mer has a count > 0 in the table.  The masked text (k_fq_mask) holds a break at every byte
//   that is no base of a sequence line, so with the line table as the offsets of kmscan::lane_walk only sequence lines
//   have valid windows, and a window never spans two lines: every line ends in its newline, a break.
//   keep(r) = (hits(r) >= min_hits) != invert.
//   The output is the kept records' bytes end to end, in input order, from the UNMASKED text.
#pragma once
#include "scan_rule.h"

namespace kmsel {

constexpr uint32_t THREADS = 256;
constexpr uint32_t WORD = 16;            // bytes of the dense output one lane assembles and stores
constexpr uint32_t MIN_RECORD = 6;       // "@\n\n+\n\n": a piece that passed the validation holds at most n / 6 records
constexpr uint32_t SRC_PAD = 32;         // readable bytes behind the source text (two aligned 16-byte loads from a byte < n)
constexpr uint32_t OUT_PAD = 16;         // writable bytes behind the output's `stage` bytes (the last word is stored whole)

// ---- records
KM_SCAN_HD inline uint32_t line_count(uint32_t newlines, bool last_is_newline) { return newlines + (last_is_newline ? 0u : 1u); }
KM_SCAN_HD inline uint32_t max_records(uint64_t n) { return (uint32_t)(n / MIN_RECORD) + 1u; }
// records the sizes and the gather look at: all of a well-formed piece; a malformed one (more lines than n / 6
// records could have) is cut at the bound, and is never written
KM_SCAN_HD inline uint32_t record_count(uint32_t n_lines, uint64_t n) {
  const uint32_t r = n_lines >> 2, m = max_records(n);
  return r < m ? r : m;
}
KM_SCAN_HD inline uint32_t record_begin(const uint32_t* line_start, uint32_t r) { return line_start[4u * r]; }
KM_SCAN_HD inline uint32_t record_end(const uint32_t* line_start, uint32_t r, uint32_t n) {
  const uint32_t e = line_start[4u * r + 4u];
  return e < n ? e : n;                  // (n + 1 behind a last line without newline)
}
KM_SCAN_HD inline bool keep(uint32_t hits, uint32_t min_hits, bool invert) { return (hits >= min_hits) != invert; }
KM_SCAN_HD inline uint32_t record_len(const uint32_t* line_start, uint32_t r, uint32_t n, uint32_t hits, uint32_t min_hits,
                                      bool invert) {
  return keep(hits, min_hits, invert) ? record_end(line_start, r, n) - record_begin(line_start, r) : 0u;
}
// scan chunks (of `chunk` entries) of the lengths of a piece of n bytes: its records and the entry behind them, which
// the scan turns into the total
KM_SCAN_HD inline uint64_t len_chunks(uint64_t n, uint32_t chunk) { return ((uint64_t)max_records(n) + 1 + chunk - 1) / chunk; }
// entries of the hit array a piece of n bytes can touch: line l < n + 1 adds to hits[l >> 2]
KM_SCAN_HD inline uint64_t hit_cells(uint64_t n) { return n / 4 + 2; }

// ---- hits: the walk of one lane over the masked text
// Env: count(fwd, rev) -> the table's count of a valid window; add(r, c) -> hits[r] += c (an atomic on the device).
template <typename Env>
struct HitSink {
  Env& env;
  uint32_t c;
  KM_SCAN_HD void leave(uint64_t line) {
    if (c) env.add((uint32_t)(line >> 2), c);
    c = 0;
  }
  KM_SCAN_HD void nonbase() {}
  KM_SCAN_HD void window(uint32_t, uint64_t fwd, uint64_t rev, bool valid) {
    if (valid && env.count(fwd, rev) > 0) ++c;
  }
};

// w: the 64 bytes of the masked piece from s (a multiple of kmscan::RUN, s < n).  The lane owns the window starts
// [s, s + 32) that lie in the piece; line_start[0 .. n_lines] with n_lines >= 1.
template <typename Env>
KM_SCAN_HD inline void lane_hits(const uint32_t (&w)[16], uint32_t s, uint32_t n, const uint32_t* line_start,
                                 uint32_t n_lines, int k, Env& env) {
  const uint32_t own = n - s < kmscan::RUN ? n - s : kmscan::RUN;
  const uint64_t line = kmscan::seq_of(line_start, 0, (uint64_t)n_lines - 1, s);
  HitSink<Env> sink{env, 0u};
  sink.leave(kmscan::lane_walk(w, s, own, n, line_start, line, k, sink));
}

// ---- gather: one aligned 16-byte word of the dense output
struct U128 {
  uint64_t lo, hi;                       // bytes 0..7, 8..15, little-endian
};
KM_SCAN_HD inline U128 bytes_or(U128 a, U128 b) { return U128{a.lo | b.lo, a.hi | b.hi}; }
// byte j of the result is byte j + s of x, zeros behind it (s 0..15)
KM_SCAN_HD inline U128 bytes_down(U128 x, uint32_t s) {
  const uint32_t b = 8u * s;
  if (b == 0) return x;
  if (b < 64) return U128{(x.lo >> b) | (x.hi << (64u - b)), x.hi >> b};
  return U128{x.hi >> (b - 64u), 0ull};
}
// byte j + s of the result is byte j of x, zeros in front of it (s 0..16)
KM_SCAN_HD inline U128 bytes_up(U128 x, uint32_t s) {
  const uint32_t b = 8u * s;
  if (b == 0) return x;
  if (b < 64) return U128{x.lo << b, (x.hi << b) | (x.lo >> (64u - b))};
  if (b < 128) return U128{0ull, x.lo << (b - 64u)};
  return U128{0ull, 0ull};
}
// the first c bytes of x, zeros behind them (c 1..16)
KM_SCAN_HD inline U128 bytes_first(U128 x, uint32_t c) {
  if (c >= 16) return x;
  if (c > 8) return U128{x.lo, x.hi & (~0ull >> (8u * (16u - c)))};
  return U128{c == 8 ? x.lo : x.lo & ((1ull << (8u * c)) - 1ull), 0ull};
}

// The c source bytes from sp (any alignment), in bytes 0 .. c of the result; what lies behind them is not defined.
// load(a): the 16 bytes at the aligned offset a.  The second word is loaded only when the bytes reach into it.
template <typename Load>
KM_SCAN_HD inline U128 source_bytes(Load& load, uint32_t sp, uint32_t c) {
  const uint32_t a = sp & ~15u, s = sp & 15u;
  U128 x = bytes_down(load(a), s);
  if (s + c > 16u) x = bytes_or(x, bytes_up(load(a + 16u), 16u - s));
  return x;
}

// Word w of the output, bytes [16 w, 16 w + 16) of the kept records end to end (16 w < total); bytes at and behind
// `total` are zero.  rec_off[0 .. n_rec]: the exclusive scan of the record lengths, rec_off[n_rec] = total.  The record
// of the word's first byte comes from one binary search (the last r with rec_off[r] <= 16 w: dropped records have
// length 0 and are passed over), the records behind it by stepping, with another search where the step meets a dropped one.
// gather_word_of is the same over entries that are not the records themselves: entry e of rec_off holds the bytes of
// record rec_of(e), which is asked only for entries of a length > 0 (select_label_rule.h: the labels' planes end to end).
struct SameRecord {
  KM_SCAN_HD uint32_t operator()(uint32_t e) const { return e; }
};
template <typename Load, typename RecOf>
KM_SCAN_HD inline U128 gather_word_of(Load& load, const uint32_t* line_start, const uint32_t* rec_off, uint32_t n_rec,
                                      uint32_t total, uint32_t w, const RecOf& rec_of) {
  uint32_t o = w * WORD;
  const uint32_t end = total - o < WORD ? total : o + WORD;
  uint32_t r = (uint32_t)kmscan::seq_of(rec_off, 0, (uint64_t)n_rec - 1, o);
  uint32_t r_begin = rec_off[r], r_end = rec_off[r + 1];
  U128 out{0ull, 0ull};
  uint32_t filled = 0;
  for (;;) {
    const uint32_t c = (r_end < end ? r_end : end) - o;
    const uint32_t sp = record_begin(line_start, rec_of(r)) + (o - r_begin);
    out = bytes_or(out, bytes_up(bytes_first(source_bytes(load, sp, c), c), filled));
    filled += c;
    o += c;
    if (o >= end) break;
    ++r;                                   // the next record, and if that one was dropped, the next kept one by another
    r_begin = r_end;                       // search: where one read in a thousand is kept, stepping over the dropped
    r_end = rec_off[r + 1];                // ones costs a thousand dependent loads (rec_off[r] = o < total: it ends)
    if (r_end <= o) {
      r = (uint32_t)kmscan::seq_of(rec_off, (uint64_t)r, (uint64_t)n_rec - 1, o);
      r_begin = rec_off[r];
      r_end = rec_off[r + 1];
    }
  }
  return out;
}
template <typename Load>
KM_SCAN_HD inline U128 gather_word(Load& load, const uint32_t* line_start, const uint32_t* rec_off, uint32_t n_rec,
                                   uint32_t total, uint32_t w) {
  return gather_word_of(load, line_start, rec_off, n_rec, total, w, SameRecord{});
}

}  // namespace kmsel
