// select_label_kernel.h — the FASTQ records of a piece sorted into up to 32 outputs by the labels of their k-mers, on
// the device: the kernels behind km_select_labels_add_fastq and kmjf_fastq_label_hits (DESIGN.md §10 "Select, labels";
// the rule and the arithmetic of a lane: select_label_rule.h).
//
// In front of them run the line table and k_fq_mask of fastq_kernel.h, unchanged, as in front of select_kernel.h.
//   k_lab_clear    the n_labels hit planes hits[l * hit_stride + 0 .. n_lines / 4] = 0, the piece's cells
//   k_lab_hits     k_sel_hits' work distribution; the table's count of a window is its label mask, and the lane counts
//                  per label in bit slices until it leaves the line, then adds each label's count to
//                  hits[l * hit_stride + line >> 2] with one 32-bit atomicAdd.  Integer adds: no order dependence.
//   k_lab_sizes    one lane per record, looping over the labels (a plane's reads and writes are coalesced across the
//                  lanes): len[l * len_stride + r] = the bytes of record r if keep_l(r), else 0, zeros up to the end
//                  of the plane; per label the bytes and the kept count by one atomicAdd per wave that has any; the
//                  records kept by at least one label and by at least two.
//   k_scan_*       (table_kernels.h) the n_labels planes of len as ONE array -> its exclusive scan in place
//   k_lab_offsets  label_off[0 .. n_labels] and the total from the scanned array, into the cells that come back
//   k_lab_gather   output-centric as k_sel_gather: a lane owns the aligned 16-byte word w0 + w of the virtual stream
//                  (label 0's bytes, then label 1's, ...) and stores it at out[w].  No atomics; no byte at or behind
//                  the total rounded up to 16 is written, and none at or behind 16 * (the grid's lanes).
#pragma once
#include "select_kernel.h"
#include "select_label_rule.h"

namespace kmd {

// the uint32 cells of a labelled piece
enum {
  LAB_RECORDS = 0, LAB_ANY = 1, LAB_MULTI = 2, LAB_TOTAL = 3,
  LAB_BYTES = 4,                           // [32]
  LAB_KEPT = LAB_BYTES + 32,               // [32]
  LAB_OFF = LAB_KEPT + 32,                 // [33] label_off
  LAB_CELLS = 104
};

__global__ __launch_bounds__(kmsel::THREADS) void k_lab_clear(const uint8_t* text, uint64_t n, const uint32_t* tile_off,
                                                              uint32_t n_tiles, uint32_t n_labels, uint64_t hit_stride,
                                                              uint32_t* hits, uint32_t* cells) {
  const uint32_t n_lines = sel_n_lines(text, n, tile_off, n_tiles);
  const uint32_t m = (n_lines >> 2) + 1u;
  for (uint32_t l = 0; l < n_labels; ++l)
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) hits[l * hit_stride + i] = 0u;
  if (blockIdx.x == 0 && threadIdx.x < LAB_CELLS)
    cells[threadIdx.x] = threadIdx.x == LAB_RECORDS ? kmsel::record_count(n_lines, n) : 0u;
}

struct LabHitEnv {
  const TableView& t;
  uint32_t* hits;
  uint64_t hit_stride;
  __device__ uint32_t mask(uint64_t fwd, uint64_t) const {
    uint32_t f = 0;
    return query_one(t, fwd, &f);
  }
  __device__ void add(uint32_t l, uint32_t r, uint32_t c) const { atomicAdd(hits + l * hit_stride + r, c); }
};

__global__ __launch_bounds__(kmscan::THREADS) void k_lab_hits(TableView t, const uint8_t* text, const uint8_t* masked,
                                                              uint32_t n, const uint32_t* tile_off, uint32_t n_tiles,
                                                              const uint32_t* line_start, uint32_t n_labels,
                                                              uint64_t hit_stride, uint32_t* hits) {
  const uint64_t s64 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * kmscan::RUN;
  if (s64 >= n) return;
  const uint32_t s = (uint32_t)s64;
  const uint4* v = reinterpret_cast<const uint4*>(masked + s);
  const uint4 q0 = v[0], q1 = v[1], q2 = v[2], q3 = v[3];
  const uint32_t w[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w,
                          q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
  LabHitEnv env{t, hits, hit_stride};
  kmlab::lane_label_hits(w, s, n, line_start, sel_n_lines(text, n, tile_off, n_tiles), t.k, n_labels, env);
}

// one record per lane, r < len_stride = the grid's threads (whole scan chunks)
__global__ __launch_bounds__(kmsel::THREADS) void k_lab_sizes(const uint32_t* line_start, uint32_t n, const uint32_t* hits,
                                                              uint64_t hit_stride, uint32_t n_labels, uint32_t min_hits,
                                                              uint32_t* len, uint32_t len_stride, uint32_t* cells) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  const bool real = r < cells[LAB_RECORDS];
  const uint32_t bytes = real ? kmlab::record_bytes(line_start, r, n) : 0u;
  uint32_t keep = 0;
  for (uint32_t l = 0; l < n_labels; ++l) {
    const bool kept = real && kmlab::keeps(hits[l * hit_stride + r], min_hits);
    len[(uint64_t)l * len_stride + r] = kept ? bytes : 0u;
    keep |= (kept ? 1u : 0u) << l;
    const unsigned long long who = __ballot(kept);
    if (who) {                               // (wave-uniform)
      uint32_t sum = kept ? bytes : 0u;
      for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
      if (lane_id() == 0) {
        atomicAdd(cells + LAB_BYTES + l, sum);
        atomicAdd(cells + LAB_KEPT + l, (uint32_t)__popcll(who));
      }
    }
  }
  const uint32_t any = (uint32_t)__popcll(__ballot(keep != 0u));
  const uint32_t multi = (uint32_t)__popcll(__ballot((keep & (keep - 1u)) != 0u));
  if (lane_id() == 0 && any) {
    atomicAdd(cells + LAB_ANY, any);
    if (multi) atomicAdd(cells + LAB_MULTI, multi);
  }
}

// off: the scanned planes
__global__ void k_lab_offsets(const uint32_t* off, uint32_t n_labels, uint32_t len_stride, uint32_t* cells) {
  const uint32_t l = threadIdx.x;
  if (blockIdx.x != 0 || l > n_labels) return;
  const uint32_t at = kmlab::label_begin(off, n_labels, len_stride, l);
  cells[LAB_OFF + l] = at;
  if (l == n_labels) cells[LAB_TOTAL] = at;
}

// out: 16-byte aligned, room for 16 bytes per lane of the grid; w0: the first word of this pass
__global__ __launch_bounds__(kmsel::THREADS) void k_lab_gather(const uint8_t* text, const uint32_t* line_start,
                                                               const uint32_t* off, uint32_t n_labels, uint32_t len_stride,
                                                               uint32_t w0, uint32_t pass_words, uint8_t* out) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t total = off[kmlab::stream_entries(n_labels, len_stride)];
  if (w >= pass_words || (w0 + w) * kmsel::WORD >= total) return;
  SelLoad load{text};
  const kmsel::U128 x = kmlab::stream_word(load, line_start, off, n_labels, len_stride, total, (uint32_t)(w0 + w));
  reinterpret_cast<uint4*>(out)[w] =
      make_uint4((uint32_t)x.lo, (uint32_t)(x.lo >> 32), (uint32_t)x.hi, (uint32_t)(x.hi >> 32));
}

}  // namespace kmd
