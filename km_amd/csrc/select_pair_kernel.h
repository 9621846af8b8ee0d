// select_pair_kernel.h — the mates of a paired-end run kept together: the kernels behind km_select_pair_add_fastq
// (DESIGN.md §10 "Select, pairs"; the rule: select_pair_rule.h).
//
// Each mate's piece goes through the front half of fastq_kernel.h and k_sel_clear / k_sel_hits of select_kernel.h,
// unchanged, into its own line table, hit array and cells.  Then, with R = min(records of piece 1, records of piece 2)
// read from those cells on the device:
//   k_pair_clear   the pair's cells = 0, the name cell = nothing found
//   k_pair_sizes   one lane per pair: len1[r], len2[r] = the bytes of the two records of pair r if it is kept, else 0,
//                  zeros up to the end of each array's last scan chunk; per mate the byte total, and the kept count,
//                  by one atomicAdd per wave that has any; R and, per mate, the offset at which record R begins
//   k_pair_names   one lane per pair: the two names compared byte by byte; the smallest pair that disagrees by atomicMin
//   k_scan_*       (table_kernels.h) each length array -> its exclusive scan in place
//   k_pair_gather  k_sel_gather's word assembly (kmsel::gather_word) for both mates in one launch: blockIdx.y picks
//                  the mate, and R bounds the search, not the piece's own record count
#pragma once
#include "select_kernel.h"
#include "select_pair_rule.h"

namespace kmd {

// the uint32 cells of a pair of pieces
enum { PAIR_BYTES1 = 0, PAIR_BYTES2 = 1, PAIR_KEPT = 2, PAIR_R = 3, PAIR_USED1 = 4, PAIR_USED2 = 5, PAIR_CELLS = 8 };
constexpr unsigned long long PAIR_NAMES_AGREE = ~0ull;

// one mate's piece as the pair kernels see it
struct PairSide {
  const uint8_t* text;                    // the raw piece, n bytes
  const uint32_t* line_start;
  const uint32_t* hits;
  const uint32_t* cells;                  // the piece's SEL_* cells
  uint32_t* len;                          // n_pad entries: whole scan chunks
  uint32_t n, n_pad;
};

__global__ void k_pair_clear(unsigned long long* name_cell, uint32_t* pc) {
  if (blockIdx.x == 0 && threadIdx.x < PAIR_CELLS) pc[threadIdx.x] = 0u;
  if (blockIdx.x == 0 && threadIdx.x == 0) *name_cell = PAIR_NAMES_AGREE;
}

// r < the grid's threads >= max(a.n_pad, b.n_pad)
__global__ __launch_bounds__(kmsel::THREADS) void k_pair_sizes(PairSide a, PairSide b, uint32_t min_hits, uint32_t invert,
                                                               uint32_t rule, uint32_t* pc) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t n_pairs = kmpair::pair_count(a.cells[SEL_RECORDS], b.cells[SEL_RECORDS]);
  kmpair::Lens l{0u, 0u, false};
  if (r < n_pairs)
    l = kmpair::pair_lens(a.line_start, a.n, b.line_start, b.n, r, a.hits[r], b.hits[r], rule, min_hits, invert != 0u);
  if (r < a.n_pad) a.len[r] = l.len1;
  if (r < b.n_pad) b.len[r] = l.len2;
  uint32_t sum1 = l.len1, sum2 = l.len2;
  for (int o = 32; o > 0; o >>= 1) {
    sum1 += __shfl_xor(sum1, o);
    sum2 += __shfl_xor(sum2, o);
  }
  const uint32_t kept = (uint32_t)__popcll(__ballot(l.kept));
  if (lane_id() == 0 && kept) {
    atomicAdd(pc + PAIR_BYTES1, sum1);
    atomicAdd(pc + PAIR_BYTES2, sum2);
    atomicAdd(pc + PAIR_KEPT, kept);
  }
  if (r == 0) {
    pc[PAIR_R] = n_pairs;
    pc[PAIR_USED1] = kmpair::consumed(a.line_start, n_pairs, a.n);
    pc[PAIR_USED2] = kmpair::consumed(b.line_start, n_pairs, b.n);
  }
}

struct PairByte {
  const uint8_t* text;
  __device__ uint32_t operator()(uint32_t i) const { return text[i]; }
};

__global__ __launch_bounds__(kmsel::THREADS) void k_pair_names(PairSide a, PairSide b, unsigned long long* name_cell) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= kmpair::pair_count(a.cells[SEL_RECORDS], b.cells[SEL_RECORDS])) return;
  PairByte b1{a.text}, b2{b.text};
  if (!kmpair::names_agree(b1, kmsel::record_begin(a.line_start, r), a.n, b2, kmsel::record_begin(b.line_start, r), b.n))
    atomicMin(name_cell, (unsigned long long)r);
}

// one mate's way out: out is 16-byte aligned, with room for the total rounded up to 16
struct PairOut {
  const uint8_t* text;
  const uint32_t* line_start;
  const uint32_t* rec_off;                // the scanned lengths, rec_off[R] = the mate's total
  uint8_t* out;
};

__global__ __launch_bounds__(kmsel::THREADS) void k_pair_gather(PairOut a, PairOut b, const uint32_t* pc) {
  const bool second = blockIdx.y != 0u;
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t total = pc[second ? PAIR_BYTES2 : PAIR_BYTES1];
  if (w * kmsel::WORD >= total) return;
  SelLoad load{second ? b.text : a.text};
  const kmsel::U128 x = kmsel::gather_word(load, second ? b.line_start : a.line_start, second ? b.rec_off : a.rec_off,
                                           pc[PAIR_R], total, (uint32_t)w);
  reinterpret_cast<uint4*>(second ? b.out : a.out)[w] =
      make_uint4((uint32_t)x.lo, (uint32_t)(x.lo >> 32), (uint32_t)x.hi, (uint32_t)(x.hi >> 32));
}

}  // namespace kmd
