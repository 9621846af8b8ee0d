// scan_kernel.h — the k-mers of sequences, cut and looked up on the device: the kernels behind kmjf_cov_seqs and
// kmjf_scan_text (DESIGN.md §10 "Scan"; the window rule and the walk of one lane: scan_rule.h).
//
// The work distribution is k_count_insert's (count_kernel.h): lane g of a piece owns the window starts
// [32 g, 32 g + 32), loads the 64 bytes from 32 g as four aligned dwordx4 (its own 32 and k - 1 <= 31 of its
// neighbour's) and rolls the forward and the reverse-complement key over them.  Where that kernel ends in a hash
// insert, this one ends in a table lookup (query_one), and it knows which sequence each byte belongs to: one binary
// search of the piece's slice of the offsets per lane, then stepping forward (kmscan::lane_walk).
//   k_scan_init    the cells of a call: zeros, min = 0xFFFFFFFF
//   k_scan_stats   per sequence the km_cov_t sums.  A lane accumulates in registers while it stays in one sequence and
//                  flushes when it leaves it; at the end a wave whose lanes all stand in one sequence combines them
//                  by shuffles and issues one atomic per field, otherwise every lane flushes its own.  All fields are
//                  integers (64-bit adds, 32-bit min / max): the result does not depend on arrival order.
//   k_scan_text    per window start of the piece the printed key, its count, and one bit "has a line" (a word per
//                  lane); DumpScan hands them to the sizes / scan / write pass of dump_kernel.h.
#pragma once
#include "device_common.h"
#include "dump_kernel.h"
#include "scan_rule.h"

namespace kmd {

static_assert(sizeof(km_cov_t) == 48, "km_cov_t: five u64 and two u32");

__global__ void k_scan_init(km_cov_t* cells, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    km_cov_t c;
    c.total = c.n_kmers = c.n_zero = c.n_skipped = c.n_nonbase = 0;
    c.min = 0xFFFFFFFFu;
    c.max = 0;
    cells[i] = c;
  }
}

// What one launch scans: text[0 .. ) is the staged piece, whose first byte is byte `first` of the call's text; the
// piece owns n_starts starts.  off[0 .. n_seqs]: the offsets of the whole call; the piece's first byte lies in
// sequence q_lo and its last start in q_hi.
struct ScanPiece {
  const uint8_t* text;
  uint64_t first, n_starts, end_all;
  const uint64_t* off;
  uint64_t q_lo, q_hi;
};

__device__ inline void scan_flush(km_cov_t* cell, const kmscan::Acc& a) {
  if (a.total) atomicAdd(reinterpret_cast<unsigned long long*>(&cell->total), (unsigned long long)a.total);
  if (a.n_kmers) {
    atomicAdd(reinterpret_cast<unsigned long long*>(&cell->n_kmers), (unsigned long long)a.n_kmers);
    atomicMin(&cell->min, a.min);
    atomicMax(&cell->max, a.max);
  }
  if (a.n_zero) atomicAdd(reinterpret_cast<unsigned long long*>(&cell->n_zero), (unsigned long long)a.n_zero);
  if (a.n_skipped) atomicAdd(reinterpret_cast<unsigned long long*>(&cell->n_skipped), (unsigned long long)a.n_skipped);
  if (a.n_nonbase) atomicAdd(reinterpret_cast<unsigned long long*>(&cell->n_nonbase), (unsigned long long)a.n_nonbase);
}

struct ScanStatsSink {
  const TableView& t;
  km_cov_t* cells;
  kmscan::Acc a;
  __device__ void leave(uint64_t q) {
    if (!kmscan::acc_empty(a)) scan_flush(cells + q, a);
    kmscan::acc_clear(a);
  }
  __device__ void nonbase() { ++a.n_nonbase; }
  __device__ void window(uint32_t, uint64_t fwd, uint64_t, bool valid) {
    if (valid) {
      uint32_t f = 0;
      kmscan::acc_count(a, query_one(t, fwd, &f));
    } else {
      ++a.n_skipped;
    }
  }
};

struct ScanTextSink {
  const TableView& t;
  uint64_t* keys;          // of the lane's first start
  uint32_t* counts;
  uint32_t lines;          // bit j: the window that starts at j has a line
  __device__ void leave(uint64_t) {}
  __device__ void nonbase() {}
  __device__ void window(uint32_t j, uint64_t fwd, uint64_t rev, bool valid) {
    if (valid) {
      uint32_t f = 0;
      keys[j] = kmscan::printed_key(fwd, rev, t.canonical);
      counts[j] = query_one(t, fwd, &f);
      lines |= 1u << j;
    }
  }
};

// the lane's 64 bytes and its sequence -> kmscan::lane_walk; returns the sequence the lane ended in
template <typename Sink>
__device__ inline uint64_t scan_lane(const ScanPiece& p, uint64_t s, int k, Sink& sink) {
  const uint4* v = reinterpret_cast<const uint4*>(p.text + s);
  const uint4 q0 = v[0], q1 = v[1], q2 = v[2], q3 = v[3];
  const uint32_t w[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w,
                          q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
  const uint64_t g0 = p.first + s;
  const uint32_t own = (uint32_t)min((uint64_t)kmscan::RUN, p.n_starts - s);
  return kmscan::lane_walk(w, g0, own, p.end_all, p.off, kmscan::seq_of(p.off, p.q_lo, p.q_hi, g0), k, sink);
}

__global__ __launch_bounds__(kmscan::THREADS) void k_scan_stats(TableView t, ScanPiece p, km_cov_t* cells) {
  const uint64_t s = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * kmscan::RUN;
  const bool active = s < p.n_starts;
  ScanStatsSink sink{t, cells, {}};
  kmscan::acc_clear(sink.a);
  uint64_t q = ~0ull;
  if (active) q = scan_lane(p, s, t.k, sink);
  // (lane 0 of a wave has the smallest s: when it is idle the whole wave is, and there is nothing to flush)
  const uint64_t q_first = lane_u64(q, 0);
  if (__all(!active || q == q_first)) {
    kmscan::Acc a = sink.a;
    for (int o = 32; o > 0; o >>= 1) {
      a.total += __shfl_xor((unsigned long long)a.total, o);
      a.n_kmers += __shfl_xor(a.n_kmers, o);
      a.n_zero += __shfl_xor(a.n_zero, o);
      a.n_skipped += __shfl_xor(a.n_skipped, o);
      a.n_nonbase += __shfl_xor(a.n_nonbase, o);
      a.min = min(a.min, (uint32_t)__shfl_xor(a.min, o));
      a.max = max(a.max, (uint32_t)__shfl_xor(a.max, o));
    }
    if (lane_id() == 0 && active && !kmscan::acc_empty(a)) scan_flush(cells + q_first, a);
  } else if (active && !kmscan::acc_empty(sink.a)) {
    scan_flush(cells + q, sink.a);
  }
}

// keys, counts: n_starts entries; line_bits: one word per lane, ceil(n_starts / 32)
__global__ __launch_bounds__(kmscan::THREADS) void k_scan_text(TableView t, ScanPiece p, uint64_t* keys, uint32_t* counts,
                                                               uint32_t* line_bits) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t s = g * kmscan::RUN;
  if (s >= p.n_starts) return;
  ScanTextSink sink{t, keys + s, counts + s, 0u};
  (void)scan_lane(p, s, t.k, sink);
  line_bits[g] = sink.lines;
}

// The window starts of a scanned piece as records of the dump pass: a start without a valid window has no line.
struct DumpScan {
  const uint64_t* keys;
  const uint32_t* counts;
  const uint32_t* line_bits;
  __device__ bool line(uint32_t i) const { return (line_bits[i >> 5] >> (i & 31u)) & 1u; }
  __device__ uint32_t count(uint32_t i) const { return counts[i]; }
  __device__ uint64_t key(uint32_t i) const { return keys[i]; }
};

}  // namespace kmd
