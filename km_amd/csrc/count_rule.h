// count_rule.h — the windows of a staged piece of reads as the counting kernels see them: which bytes are bases, which
// windows and which bases a lane owns, and the walk of one lane over its 64 bytes (plain C++17, no HIP headers;
// __host__ __device__ under hipcc, so count_kernel.h, filter_kernel.h, sketch_kernel.h and tests/host/count_rule.cpp
// run the same code).  DESIGN.md §10 "count_rule.h".
//
// The rule:
//   text[0 .. n) is one piece of the counter's byte stream.  ACGTacgt are bases (scan_rule.h: is_base, code); every
//   other byte is a break, and so is the end of the piece: NOTHING at or behind n is looked at, whatever the bytes that
//   can be read there hold (PAD of them are readable: the last lane loads 64 from its start).
//   A window is k consecutive bases that end before n; its key is those k bases, 2 bits each, the first base most
//   significant, or the smaller of that and its reverse complement's when the counter is canonical.
//   Lane g owns the window STARTS [RUN g, RUN g + RUN): it is given the 64 bytes from s = RUN g (its own 32 and
//   k - 1 <= 31 of its neighbour's) and hands over every window that starts in its own range, so every window of the
//   piece is handed over by exactly one lane.
//   A lane tallies in `bases` the bases among its own 32 bytes at or behind own_from: pieces of one call overlap by
//   k - 1 bytes, and bytes [0, own_from) were counted as bases by the piece before.  The windows that reach into them
//   are this piece's: own_from cuts the bases only.
//   `kmers` tallies the windows handed over.
//
// The functor is called with every window's key, and the walk returns the sum of what it returned: at most RUN calls,
// so a functor may pack several tallies into one value, a byte each.  It is taken BY VALUE and captures by value: a
// tally it captured by reference would live in scratch on the device (12 bytes per lane in k_count_solid, and 0.05 ms
// of 1.94), while a returned value stays in a register.
#pragma once
#include "scan_rule.h"

namespace kmcount {

constexpr uint32_t RUN = 32;                 // window starts a lane owns
constexpr uint32_t PAD = 128;                // readable bytes behind a staged piece

// w: the 64 bytes from the lane's first byte s (s < n) as sixteen little-endian words, as kmscan::lane_walk takes them.
template <class Window>
KM_SCAN_HD inline uint32_t lane_walk(const uint32_t (&w)[16], uint64_t n, uint64_t s, uint32_t own_from, int k,
                                     int canonical, uint32_t& bases, uint32_t& kmers, Window window) {
  const uint64_t kmask = k >= 32 ? ~0ull : ((1ull << (2 * k)) - 1);
  const uint32_t rshift = 2u * (uint32_t)(k - 1);
  const uint32_t jend = (uint32_t)k + RUN - 1;                 // bytes this lane looks at (<= 63)
  uint64_t fwd = 0, rev = 0;
  uint32_t run = 0, sum = 0;                                   // run: bases since the last break
  KM_SCAN_UNROLL
  for (uint32_t d = 0; d < 16; ++d) {
    if (4 * d < jend) {
      const uint32_t word = w[d];
      KM_SCAN_NO_UNROLL
      for (uint32_t b = 0; b < 4; ++b) {
        const uint32_t j = 4 * d + b;
        const uint32_t ch = (word >> (8 * b)) & 0xFFu;
        const bool base = kmscan::is_base(ch) && s + j < n && j < jend;
        const uint32_t c = kmscan::code(ch);
        fwd = ((fwd << 2) | c) & kmask;
        rev = (rev >> 2) | ((uint64_t)(3u - c) << rshift);
        run = base ? run + 1 : 0;
        bases += (base && j < RUN && s + j >= own_from) ? 1u : 0u;
        if (run >= (uint32_t)k) {                              // (j < jend: the window starts at j - k + 1 < RUN)
          ++kmers;
          sum += window((canonical && rev < fwd) ? rev : fwd);
        }
      }
    }
  }
  return sum;
}

}  // namespace kmcount
