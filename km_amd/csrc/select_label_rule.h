// select_label_rule.h — which records of a piece of 4-line FASTQ text go to which of up to 32 outputs: the walk of one
// lane with a label mask per window, the sizes per label, and the virtual stream the gather reads words of (plain
// C++17, no HIP headers; __host__ __device__ under hipcc, so select_label_kernel.h, select_label_host.h and
// tests/host/select_label_rule.cpp run the same code).  DESIGN.md §10 "Select, labels".
//
// The rule (include/kmgpu.h states it for the callers):
//   The piece, its line table, its masked text and the ownership of a window are those of select_rule.h.
//   The table's "count" of a k-mer is a 32-bit mask: bit l set = the k-mer belongs to label l, 0 <= l < n_labels <= 32;
//   bits at or above n_labels are ignored.
//   hits_l(r): the valid windows of record r's sequence line whose mask has bit l.  keep_l(r) = hits_l(r) >= min_hits.
//   Output l is the records with keep_l, end to end in input order, from the UNMASKED text.
//   The virtual stream of a piece is output 0, then output 1, ... : entry v = l * len_stride + r of the length array is
//   record r in label l (0 where it is dropped, and in the padding behind the records), and the exclusive scan of the
//   whole array gives every kept record's place in the stream and, at l * len_stride, where label l starts.
#pragma once
#include "select_rule.h"

namespace kmlab {

constexpr uint32_t MAX_LABELS = 32;
constexpr uint32_t PLANES = 6;             // a lane owns at most kmscan::RUN = 32 windows: its counts fit 6 bits

KM_SCAN_HD inline uint32_t label_bits(uint32_t mask, uint32_t n_labels) {
  return n_labels >= 32u ? mask : mask & ((1u << n_labels) - 1u);
}

// ---- hits: the walk of one lane over the masked text
// Env: mask(fwd, rev) -> the table's mask of a valid window; add(l, r, c) -> hits_l[r] += c (an atomic on the device).
// The lane counts per label in bit slices: bit l of plane[p] is bit p of the label's count within the current line, so
// a window costs a ripple-carry add over the planes whatever its mask is and however masks alternate, and nothing of
// the record has to be known before the lane leaves the line.  Then one add per label that has a count.
template <typename Env>
struct LabelSink {
  Env& env;
  uint32_t n_labels;
  uint32_t plane[PLANES];
  KM_SCAN_HD void leave(uint64_t line) {
    uint32_t any = 0;
    KM_SCAN_UNROLL
    for (uint32_t p = 0; p < PLANES; ++p) any |= plane[p];
    while (any) {
      const uint32_t l = (uint32_t)__builtin_ctz(any);
      any &= any - 1u;
      uint32_t c = 0;
      KM_SCAN_UNROLL
      for (uint32_t p = 0; p < PLANES; ++p) c |= ((plane[p] >> l) & 1u) << p;
      env.add(l, (uint32_t)(line >> 2), c);
    }
    KM_SCAN_UNROLL
    for (uint32_t p = 0; p < PLANES; ++p) plane[p] = 0u;
  }
  KM_SCAN_HD void nonbase() {}
  KM_SCAN_HD void window(uint32_t, uint64_t fwd, uint64_t rev, bool valid) {
    if (!valid) return;
    uint32_t carry = label_bits(env.mask(fwd, rev), n_labels);
    if (!carry) return;
    KM_SCAN_UNROLL
    for (uint32_t p = 0; p < PLANES; ++p) {
      const uint32_t t = plane[p] & carry;
      plane[p] ^= carry;
      carry = t;
    }
  }
};

// w, s, n, line_start, n_lines: as kmsel::lane_hits takes them
template <typename Env>
KM_SCAN_HD inline void lane_label_hits(const uint32_t (&w)[16], uint32_t s, uint32_t n, const uint32_t* line_start,
                                       uint32_t n_lines, int k, uint32_t n_labels, Env& env) {
  const uint32_t own = n - s < kmscan::RUN ? n - s : kmscan::RUN;
  const uint64_t line = kmscan::seq_of(line_start, 0, (uint64_t)n_lines - 1, s);
  LabelSink<Env> sink{env, n_labels, {0u, 0u, 0u, 0u, 0u, 0u}};
  sink.leave(kmscan::lane_walk(w, s, own, n, line_start, line, k, sink));
}

// ---- sizes
KM_SCAN_HD inline bool keeps(uint32_t hits, uint32_t min_hits) { return hits >= min_hits; }
// bit l = keep_l(r); hits: the planes, hits[l * hit_stride + r]
KM_SCAN_HD inline uint32_t keep_mask(const uint32_t* hits, uint64_t hit_stride, uint32_t r, uint32_t n_labels,
                                     uint32_t min_hits) {
  uint32_t m = 0;
  for (uint32_t l = 0; l < n_labels; ++l) m |= (keeps(hits[l * hit_stride + r], min_hits) ? 1u : 0u) << l;
  return m;
}
KM_SCAN_HD inline uint32_t record_bytes(const uint32_t* line_start, uint32_t r, uint32_t n) {
  return kmsel::record_end(line_start, r, n) - kmsel::record_begin(line_start, r);
}
// entries per label of the length array of a piece of n bytes: whole scan chunks, at least one entry behind the records
KM_SCAN_HD inline uint32_t len_stride(uint64_t n, uint32_t chunk) { return (uint32_t)(kmsel::len_chunks(n, chunk) * chunk); }

// ---- the virtual stream
// off[0 .. n_labels * stride): the exclusive scan of the length array.  Its last entry is padding of length 0, so it
// holds the total, and the entries in front of it are what gather_word_of searches.
KM_SCAN_HD inline uint32_t stream_entries(uint32_t n_labels, uint32_t stride) { return n_labels * stride - 1u; }
KM_SCAN_HD inline uint32_t label_begin(const uint32_t* off, uint32_t n_labels, uint32_t stride, uint32_t l) {
  return l < n_labels ? off[(uint64_t)l * stride] : off[stream_entries(n_labels, stride)];
}
struct RecordOfEntry {
  uint32_t stride;
  KM_SCAN_HD uint32_t operator()(uint32_t e) const { return e % stride; }
};
// bytes per gather pass when the output buffer holds buffer_bytes: whole words
KM_SCAN_HD inline uint64_t pass_bytes(uint64_t buffer_bytes) { return buffer_bytes & ~(uint64_t)(kmsel::WORD - 1u); }
KM_SCAN_HD inline uint64_t pass_count(uint64_t total, uint64_t cap) { return total <= cap ? 1u : (total + cap - 1) / cap; }

// Word w0 + w of the virtual stream (16 (w0 + w) < total), as kmsel::gather_word assembles a word of one output.
template <typename Load>
KM_SCAN_HD inline kmsel::U128 stream_word(Load& load, const uint32_t* line_start, const uint32_t* off, uint32_t n_labels,
                                          uint32_t stride, uint32_t total, uint32_t word) {
  return kmsel::gather_word_of(load, line_start, off, stream_entries(n_labels, stride), total, word, RecordOfEntry{stride});
}

}  // namespace kmlab
