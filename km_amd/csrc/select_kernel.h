// select_kernel.h — the FASTQ records that hit a k-mer table, gathered densely on the device: the kernels behind
// km_select_add_fastq and kmjf_fastq_hits (DESIGN.md §10 "Select"; the rule and the arithmetic of a lane: select_rule.h).
//
// In front of them run the line table and k_fq_mask of fastq_kernel.h, unchanged: text is the raw piece, masked the
// same bytes with a break wherever there is no base of a sequence line, line_start the piece's line table, tile_off
// its scanned newline counts (tile_off[n_tiles] = the newlines of the piece).
//   k_sel_clear    hits[0 .. n_lines / 4] = 0, the piece's cells = {0, 0, records}
//   k_sel_hits     k_scan_stats' work distribution (a lane owns 32 window starts of the masked text, four aligned
//                  dwordx4) with the line table as the offsets: the lane counts the windows of its line that the table
//                  holds and adds them to hits[line >> 2] with one 32-bit atomicAdd when it leaves the line, if there
//                  are any.  Integer adds: no order dependence.
//   k_sel_sizes    len[r] = the bytes of record r if it is kept, else 0, zeros up to the end of the last scan chunk;
//                  the piece's byte total and kept count by one atomicAdd per wave that has any.
//   k_scan_*       (table_kernels.h) len -> its exclusive scan in place, chunk by chunk
//   k_sel_gather   output-centric: a lane owns one aligned 16-byte word of the dense output, finds the record of its
//                  first byte by one binary search over the scanned lengths (and another where a record ends inside
//                  the word and dropped ones follow), assembles the word from the unmasked
//                  text — two aligned dwordx4 loads and a byte shift per stretch of one record — and stores one
//                  dwordx4.  No atomics; no byte at or behind the total rounded up to 16 is written.
#pragma once
#include "device_common.h"
#include "fastq_kernel.h"
#include "select_rule.h"

namespace kmd {

enum { SEL_BYTES = 0, SEL_KEPT = 1, SEL_RECORDS = 2, SEL_CELLS = 4 };   // the uint32 cells of a piece

__device__ inline uint32_t sel_n_lines(const uint8_t* text, uint64_t n, const uint32_t* tile_off, uint32_t n_tiles) {
  return kmsel::line_count(tile_off[n_tiles], text[n - 1] == '\n');
}

__global__ __launch_bounds__(kmsel::THREADS) void k_sel_clear(const uint8_t* text, uint64_t n, const uint32_t* tile_off,
                                                              uint32_t n_tiles, uint32_t* hits, uint32_t* cells) {
  const uint32_t n_lines = sel_n_lines(text, n, tile_off, n_tiles);
  const uint32_t m = (n_lines >> 2) + 1u;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) hits[i] = 0u;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    cells[SEL_BYTES] = 0u;
    cells[SEL_KEPT] = 0u;
    cells[SEL_RECORDS] = kmsel::record_count(n_lines, n);
    cells[3] = 0u;
  }
}

struct SelHitEnv {
  const TableView& t;
  uint32_t* hits;
  __device__ uint32_t count(uint64_t fwd, uint64_t) const {
    uint32_t f = 0;
    return query_one(t, fwd, &f);
  }
  __device__ void add(uint32_t r, uint32_t c) const { atomicAdd(hits + r, c); }
};

__global__ __launch_bounds__(kmscan::THREADS) void k_sel_hits(TableView t, const uint8_t* text, const uint8_t* masked,
                                                              uint32_t n, const uint32_t* tile_off, uint32_t n_tiles,
                                                              const uint32_t* line_start, uint32_t* hits) {
  const uint64_t s64 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * kmscan::RUN;
  if (s64 >= n) return;
  const uint32_t s = (uint32_t)s64;
  const uint4* v = reinterpret_cast<const uint4*>(masked + s);
  const uint4 q0 = v[0], q1 = v[1], q2 = v[2], q3 = v[3];
  const uint32_t w[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w,
                          q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
  SelHitEnv env{t, hits};
  kmsel::lane_hits(w, s, n, line_start, sel_n_lines(text, n, tile_off, n_tiles), t.k, env);
}

// one record per lane, r < n_pad = the grid's threads (whole scan chunks)
__global__ __launch_bounds__(kmsel::THREADS) void k_sel_sizes(const uint32_t* line_start, uint32_t n, const uint32_t* hits,
                                                              uint32_t min_hits, uint32_t invert, uint32_t* len,
                                                              uint32_t* cells) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t l = 0;
  if (r < cells[SEL_RECORDS]) l = kmsel::record_len(line_start, r, n, hits[r], min_hits, invert != 0u);
  len[r] = l;
  uint32_t sum = l;
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  const uint32_t kept = (uint32_t)__popcll(__ballot(l != 0u));
  if (lane_id() == 0 && kept) {
    atomicAdd(cells + SEL_BYTES, sum);
    atomicAdd(cells + SEL_KEPT, kept);
  }
}

struct SelLoad {
  const uint8_t* text;
  __device__ kmsel::U128 operator()(uint32_t a) const {
    const uint4 v = *reinterpret_cast<const uint4*>(text + a);
    return kmsel::U128{((uint64_t)v.y << 32) | v.x, ((uint64_t)v.w << 32) | v.z};
  }
};

// out: 16-byte aligned, room for the total rounded up to 16
__global__ __launch_bounds__(kmsel::THREADS) void k_sel_gather(const uint8_t* text, const uint32_t* line_start,
                                                               const uint32_t* rec_off, const uint32_t* cells,
                                                               uint8_t* out) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t total = cells[SEL_BYTES];
  if (w * kmsel::WORD >= total) return;
  SelLoad load{text};
  const kmsel::U128 x = kmsel::gather_word(load, line_start, rec_off, cells[SEL_RECORDS], total, (uint32_t)w);
  reinterpret_cast<uint4*>(out)[w] =
      make_uint4((uint32_t)x.lo, (uint32_t)(x.lo >> 32), (uint32_t)x.hi, (uint32_t)(x.hi >> 32));
}

}  // namespace kmd
