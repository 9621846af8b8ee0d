// scan_rule.h — the windows of a batch of sequences: which bytes are bases, which window belongs to which sequence,
// how a batch is cut into pieces, and the walk of one lane over its 32 window starts (plain C++17, no HIP headers;
// __host__ __device__ under hipcc, so scan_kernel.h, scan_host.h and tests/host/scan_rule.cpp run the same code).
// DESIGN.md §10 "Scan".
//
// The rule (include/kmgpu.h states it for the callers):
//   text[off[0] .. off[n_seqs]) is the sequences end to end with nothing between them; sequence q is
//   text[off[q] .. off[q + 1]), off ascends, equal neighbours are an empty sequence.
//   ACGTacgt are bases, every other byte is a non-base.
//   A window is k consecutive bytes of ONE sequence: the window that starts at byte p belongs to sequence q iff
//   off[q] <= p and p + k <= off[q + 1].  A start whose k bytes reach past its sequence is no window at all.
//   A window is valid iff its k bytes are bases; a window with a non-base is skipped (and counted as skipped).
//
// Nothing marks a boundary in the text itself: a lane knows its sequence from `off` alone (one binary search for its
// first byte, then stepping forward), so no byte value is reserved and a non-base next to a boundary is counted like
// any other.
//
// Pieces: every byte position of the text is a window START of exactly one piece (starts [first, first + n_starts)),
// and a piece stages the k - 1 bytes behind its last start as well, so that every window is complete in the piece that
// owns its start.  Nothing is counted twice because nothing is owned twice.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define KM_SCAN_HD __host__ __device__
#else
#define KM_SCAN_HD
#endif
#if defined(__clang__)
#define KM_SCAN_UNROLL _Pragma("unroll")
#define KM_SCAN_NO_UNROLL _Pragma("unroll 1")
#else
#define KM_SCAN_UNROLL
#define KM_SCAN_NO_UNROLL
#endif

namespace kmscan {

constexpr uint32_t RUN = 32;                 // window starts a lane owns
constexpr uint32_t WAVE_STARTS = 64 * RUN;   // ... a wave
constexpr uint32_t THREADS = 256;
constexpr uint32_t BLOCK_STARTS = THREADS * RUN;
constexpr uint32_t PAD = 128;                // readable bytes behind a staged piece (the last lane loads 64 from its start)
constexpr uint64_t MAX_SEQS = 1ull << 26;    // sequences of one call (KM_SCAN_MAX_SEQS)

KM_SCAN_HD inline bool is_base(uint32_t ch) {
  const uint32_t up = ch & 0xDFu;
  return up == 'A' || up == 'C' || up == 'G' || up == 'T';
}
// A 0, C 1, G 2, T 3 (either case; anything for a non-base)
KM_SCAN_HD inline uint32_t code(uint32_t ch) {
  const uint32_t c = (ch >> 1) & 3u;         // A 0, C 1, T 2, G 3
  return c ^ (c >> 1);
}
KM_SCAN_HD inline uint64_t n_windows(uint64_t len, int k) { return len >= (uint64_t)k ? len - (uint64_t)k + 1 : 0; }
KM_SCAN_HD inline bool window_in_seq(uint64_t start, int k, uint64_t seq_begin, uint64_t seq_end) {
  return start >= seq_begin && start + (uint64_t)k <= seq_end;
}

// The sequence of byte `pos`: the last q of [lo, hi] with off[q] <= pos (the caller knows off[lo] <= pos).  Empty
// sequences in front of pos are passed over: they own no byte.  (Off: uint64_t offsets of a call's text, or the 32-bit
// line starts of a FASTQ piece, select_rule.h)
template <typename Off>
KM_SCAN_HD inline uint64_t seq_of(const Off* off, uint64_t lo, uint64_t hi, uint64_t pos) {
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo + 1) / 2;
    if (off[mid] <= pos) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// ---- pieces
struct Piece {
  uint64_t first;      // text position of the piece's first start (and first staged byte)
  uint64_t n_starts;   // starts it owns
  uint64_t n_bytes;    // bytes it stages: the starts and up to k - 1 behind them
};
// starts per piece when a staged piece may hold stage_bytes bytes (stage_bytes >= k)
KM_SCAN_HD inline uint64_t starts_per_piece(uint64_t stage_bytes, int k) { return stage_bytes - (uint64_t)(k - 1); }
KM_SCAN_HD inline uint64_t n_pieces(uint64_t begin, uint64_t end, uint64_t per) { return (end - begin + per - 1) / per; }
KM_SCAN_HD inline Piece piece(uint64_t begin, uint64_t end, uint64_t per, int k, uint64_t i) {
  Piece p;
  p.first = begin + i * per;
  p.n_starts = end - p.first < per ? end - p.first : per;
  p.n_bytes = end - p.first < p.n_starts + (uint64_t)(k - 1) ? end - p.first : p.n_starts + (uint64_t)(k - 1);
  return p;
}

// ---- statistics of one sequence, as a lane keeps them
struct Acc {
  uint64_t total;
  uint32_t n_kmers, n_zero, n_skipped, n_nonbase, min, max;
};
KM_SCAN_HD inline void acc_clear(Acc& a) {
  a.total = 0;
  a.n_kmers = a.n_zero = a.n_skipped = a.n_nonbase = 0;
  a.min = 0xFFFFFFFFu;
  a.max = 0;
}
KM_SCAN_HD inline bool acc_empty(const Acc& a) { return (a.n_kmers | a.n_skipped | a.n_nonbase) == 0; }
KM_SCAN_HD inline void acc_count(Acc& a, uint32_t c) {
  a.total += c;
  ++a.n_kmers;
  a.n_zero += c == 0 ? 1u : 0u;
  a.min = c < a.min ? c : a.min;
  a.max = c > a.max ? c : a.max;
}

// ---- the walk of one lane
// w: the 64 bytes from the lane's first start as sixteen little-endian words (its own 32 and k - 1 <= 31 of its
// neighbour's).  g0: the text position of the first of them.  own: the starts of [g0, g0 + RUN) that the piece owns,
// 1..RUN.  end_all = off[n_seqs]: no byte at or behind it is looked at.  q: the sequence of g0 (seq_of).
// The sink is told, in text order,
//   sink.leave(q)                          the lane is done with sequence q and goes on to a later one
//   sink.nonbase()                         an owned byte of the current sequence is a non-base
//   sink.window(j, fwd, rev, valid)        the window that starts at g0 + j (j < own) lies in the current sequence;
//                                          fwd / rev: its key and the reverse complement's when valid
// Returns the sequence the lane ended in.
template <typename Sink, typename Off>
KM_SCAN_HD inline uint64_t lane_walk(const uint32_t (&w)[16], uint64_t g0, uint32_t own, uint64_t end_all,
                                     const Off* off, uint64_t q, int k, Sink& sink) {
  const uint64_t kmask = k >= 32 ? ~0ull : ((1ull << (2 * k)) - 1);
  const uint32_t rshift = 2u * (uint32_t)(k - 1);
  const uint32_t jend = (uint32_t)k + own - 1;               // bytes this lane looks at (<= 63)
  uint64_t fwd = 0, rev = 0;
  uint64_t seq_end = off[q + 1];
  uint32_t run = 0, in_seq = 0;                              // bases since the last non-base; bytes of this sequence seen
  KM_SCAN_UNROLL
  for (uint32_t d = 0; d < 16; ++d) {
    if (4 * d < jend) {
      const uint32_t word = w[d];
      KM_SCAN_NO_UNROLL
      for (uint32_t b = 0; b < 4; ++b) {
        const uint32_t j = 4 * d + b;
        const uint64_t p = g0 + j;
        if (j < jend && p < end_all) {
          if (p >= seq_end) {                                // (p < end_all = off[n_seqs]: the search ends)
            sink.leave(q);
            do {
              ++q;
              seq_end = off[q + 1];
            } while (p >= seq_end);
            run = 0;
            in_seq = 0;
          }
          const uint32_t ch = (word >> (8 * b)) & 0xFFu;
          const bool base = is_base(ch);
          const uint32_t c = code(ch);
          fwd = ((fwd << 2) | c) & kmask;
          rev = (rev >> 2) | ((uint64_t)(3u - c) << rshift);
          run = base ? run + 1 : 0;
          ++in_seq;
          if (!base && j < own) sink.nonbase();
          // (in_seq >= k: the k bytes up to j are this sequence's; j < jend: the window starts at j + 1 - k < own)
          if (in_seq >= (uint32_t)k) sink.window(j + 1 - (uint32_t)k, fwd, rev, run >= (uint32_t)k);
        }
      }
    }
  }
  return q;
}

// the key `query` prints for a valid window
KM_SCAN_HD inline uint64_t printed_key(uint64_t fwd, uint64_t rev, int canonical) {
  return (canonical && rev < fwd) ? rev : fwd;
}

}  // namespace kmscan
