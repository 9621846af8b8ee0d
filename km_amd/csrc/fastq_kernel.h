// fastq_kernel.h — raw 4-line FASTQ text on the device: a table of line starts, then one pass that pairs every
// base with its quality byte, masks, strips and validates (DESIGN.md §10 "Quality masking, FASTQ on the device").
// Host side: count_host.h (km_counter_add_fastq); the tile counts are scanned by table_kernels.h's k_scan_*.
//
// A piece is text[0 .. n) that begins at the first byte of a record and ends at the end of one.  Line l runs from
// line_start[l] to the newline before line_start[l + 1]; with NL newlines in the piece there are L = NL lines, or
// NL + 1 when the last byte is no newline.  line_start[NL + 1] = n + 1 stands for a newline behind the piece, so
// that the end of every line l < L is line_start[l + 1] - 1.  Line l is a header (l mod 4 = 0), a sequence (1), a
// '+' line (2) or a quality line (3).  Offsets inside a piece are 32-bit.
#pragma once
#include "device_common.h"

namespace kmd {

constexpr int FQ_THREADS = 256;
constexpr uint32_t FQ_LANE_BYTES = 16;                       // one dwordx4 per lane
constexpr uint32_t FQ_TILE = FQ_THREADS * FQ_LANE_BYTES;     // bytes a block owns
constexpr uint8_t FQ_BREAK = '\n';
// what the validation finds; the meta cell holds the smallest ((stream offset << 8) | kind), ~0 = nothing found
enum { FQ_OK = 0, FQ_NO_AT = 1, FQ_NO_PLUS = 2, FQ_QUAL_LEN = 3, FQ_TRUNCATED = 4 };
constexpr unsigned long long FQ_NO_ERROR = ~0ull;

// bit j = byte j of the lane's 16 bytes is a newline, for the first `valid` bytes (those inside the piece)
__device__ inline uint32_t fq_newlines(uint4 q, uint64_t valid) {
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
  uint32_t m = 0;
#pragma unroll
  for (uint32_t d = 0; d < 4; ++d) {
    const uint32_t x = w[d] ^ 0x0A0A0A0Au;                                       // a zero byte where a newline was
    const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);   // 0x80 in exactly those bytes
    m |= (((z >> 7) * 0x01020408u) >> 24 & 0xFu) << (4 * d);                     // bits 0, 8, 16, 24 -> 24..27
  }
  return valid >= FQ_LANE_BYTES ? m : m & ((1u << valid) - 1u);
}

// Exclusive prefix of v (0..16 per lane) over the block's lanes in byte order, and the block's total.  Inside a
// wave the prefix is taken by ballots: one per bit of v, the lanes below counted with a popcount and weighted by
// the bit; the four waves meet in LDS.
__device__ inline uint32_t fq_block_prefix(uint32_t v, uint32_t* total) {
  __shared__ uint32_t wave_sum[FQ_THREADS / 64];
  const uint32_t lane = (uint32_t)lane_id(), wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  uint32_t before = 0, all = 0;
#pragma unroll
  for (uint32_t j = 0; j < 5; ++j) {
    const unsigned long long b = __ballot((v >> j) & 1u);
    before += (uint32_t)__popcll(b & below) << j;
    all += (uint32_t)__popcll(b) << j;
  }
  if (lane == 0) wave_sum[wave] = all;
  __syncthreads();
  uint32_t sum = 0;
  for (uint32_t q = 0; q < FQ_THREADS / 64; ++q) {
    const uint32_t ws = wave_sum[q];
    if (q < wave) before += ws;
    sum += ws;
  }
  __syncthreads();
  *total = sum;
  return before;
}

// One block per tile of FQ_TILE bytes: tile_count[tile] = its newlines.
__global__ __launch_bounds__(FQ_THREADS) void k_fq_count_lines(const uint8_t* text, uint64_t n, uint32_t* tile_count) {
  const uint64_t off = (uint64_t)blockIdx.x * FQ_TILE + threadIdx.x * FQ_LANE_BYTES;
  uint32_t m = 0;
  if (off < n) m = fq_newlines(*reinterpret_cast<const uint4*>(text + off), n - off);
  uint32_t total;
  (void)fq_block_prefix((uint32_t)__popc(m), &total);
  if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

// tile_off[] is the exclusive scan of the tile counts (tile_off[n_tiles] = NL).  The newline number r (from 0)
// at offset o gives line_start[r + 1] = o + 1.
__global__ __launch_bounds__(FQ_THREADS) void k_fq_line_starts(const uint8_t* text, uint64_t n, const uint32_t* tile_off,
                                                               uint32_t n_tiles, uint32_t* line_start) {
  const uint64_t off = (uint64_t)blockIdx.x * FQ_TILE + threadIdx.x * FQ_LANE_BYTES;
  uint32_t m = 0;
  if (off < n) m = fq_newlines(*reinterpret_cast<const uint4*>(text + off), n - off);
  uint32_t total;
  uint32_t r = tile_off[blockIdx.x] + fq_block_prefix((uint32_t)__popc(m), &total);
  while (m) {
    const uint32_t j = (uint32_t)__ffs(m) - 1u;
    m &= m - 1u;
    line_start[++r] = (uint32_t)off + j + 1u;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    line_start[0] = 0;
    line_start[tile_off[n_tiles] + 1] = (uint32_t)n + 1u;
  }
}

__device__ inline void fq_report(unsigned long long* cell, uint64_t stream_offset, uint32_t kind) {
  atomicMin(cell, (unsigned long long)((stream_offset << 8) | kind));
}

// length of line l < L without its newline and without a '\r' in front of that
__device__ inline uint32_t fq_line_len(const uint8_t* text, const uint32_t* line_start, uint32_t l) {
  const uint32_t s = line_start[l];
  uint32_t e = line_start[l + 1] - 1u;
  if (e > s && text[e - 1] == '\r') --e;
  return e - s;
}

// Where the quality bytes of sequence line l begin: the start of line l + 2, or n (no byte there passes) when l
// is no sequence line or the piece ends before that line.
__device__ inline uint32_t fq_partner(const uint32_t* line_start, uint32_t l, uint32_t n_lines, uint32_t n) {
  return ((l & 3u) == 1u && l + 2u < n_lines) ? line_start[l + 2] : n;
}

// out[i] = text[i] where i lies in a sequence line, is neither '\r' nor '\n' and its quality byte — the byte at
// the same column two lines below — is >= min_qual (min_qual = 0: the quality is not read); FQ_BREAK everywhere
// else, up to the end of the lane's 16 bytes.  Same offsets in and out: no compaction, no atomics but the error's.
// The lane that owns a line's first byte checks that line: '@' at a header, '+' at a '+' line, at a quality
// line its length against the sequence's; lane 0 checks that the lines are a multiple of four.  base: the
// piece's offset in the stream, added to what is reported.
__global__ __launch_bounds__(FQ_THREADS) void k_fq_mask(const uint8_t* text, uint64_t n, const uint32_t* tile_off,
                                                        uint32_t n_tiles, const uint32_t* line_start,
                                                        uint32_t min_qual, uint64_t base, uint8_t* out,
                                                        unsigned long long* error_cell) {
  const uint64_t off64 = (uint64_t)blockIdx.x * FQ_TILE + threadIdx.x * FQ_LANE_BYTES;
  uint4 q = make_uint4(0u, 0u, 0u, 0u);
  uint32_t m = 0;
  if (off64 < n) {
    q = *reinterpret_cast<const uint4*>(text + off64);
    m = fq_newlines(q, n - off64);
  }
  uint32_t total;
  uint32_t l = tile_off[blockIdx.x] + fq_block_prefix((uint32_t)__popc(m), &total);   // the line of byte `off`
  if (off64 >= n) return;
  const uint32_t off = (uint32_t)off64, n32 = (uint32_t)n;
  const uint32_t n_lines = tile_off[n_tiles] + (text[n - 1] != '\n' ? 1u : 0u);
  if (off == 0 && (n_lines & 3u)) fq_report(error_cell, base + line_start[n_lines & ~3u], FQ_TRUNCATED);
  uint32_t ls = line_start[l];
  uint32_t qs = fq_partner(line_start, l, n_lines, n32);
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
  uint32_t o[4];
#pragma unroll
  for (uint32_t d = 0; d < 4; ++d) {
    uint32_t res = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b) {
      const uint32_t p = off + 4 * d + b;
      const uint32_t ch = (w[d] >> (8 * b)) & 0xFFu;
      uint32_t keep = FQ_BREAK;
      if (p < n32) {
        const uint32_t phase = l & 3u;
        if (p == ls) {                                         // the first byte of line l
          if (phase == 0 && ch != '@') fq_report(error_cell, base + p, FQ_NO_AT);
          if (phase == 2 && ch != '+') fq_report(error_cell, base + p, FQ_NO_PLUS);
          if (phase == 3 && fq_line_len(text, line_start, l) != fq_line_len(text, line_start, l - 2))
            fq_report(error_cell, base + p, FQ_QUAL_LEN);
        }
        if (phase == 1 && ch != '\n' && ch != '\r') {
          const uint64_t qp = (uint64_t)qs + (p - ls);
          if (min_qual == 0 || (qp < n && text[qp] >= min_qual)) keep = ch;
        }
        if (ch == '\n') {
          ++l;
          ls = p + 1u;
          qs = fq_partner(line_start, l, n_lines, n32);
        }
      }
      res |= keep << (8 * b);
    }
    o[d] = res;
  }
  *reinterpret_cast<uint4*>(out + off64) = make_uint4(o[0], o[1], o[2], o[3]);
}

}  // namespace kmd
