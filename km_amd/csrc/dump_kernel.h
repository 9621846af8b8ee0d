// dump_kernel.h — (key, count) records -> the text of `dump` / `query`: the kernels behind km_dump_text, km_jf_dump,
// km_counter_dump and kmjf_query_text (DESIGN.md §10 "Dump and query"; the text rule: dump_text.h).
//
// One piece of n records becomes one dense run of text bytes.  Lines have variable length (a count has 1 to 10
// digits, a filtered record has none), so it is sizes / scan / write, as the FASTQ line table is:
//   k_dump_sizes   one block per tile of DUMP_TILE records, one record per lane: the line length (0 when filtered
//                  out), summed by shuffles per wave and through four LDS words per block -> tile_bytes[tile],
//                  tile_kept[tile].  No atomics.
//   k_scan_*       (table_kernels.h) the exclusive scan of tile_bytes in place; the host keeps tiles + 1 <= SCAN_CHUNK,
//                  so it is one chunk and the entry behind the last tile is the piece's byte total
//   k_dump_write   the block computes the lengths again, scans them in LDS, every lane composes its line into the
//                  block's LDS image, and the image goes to text + tile_off[tile] cooperatively.
// A tile's offset has no alignment.  The image is laid out in LDS at the same residue mod 16 as its place in the text,
// so beyond the head bytes up to the next 16-byte boundary both sides are 16-byte aligned: the body is LDS b128 reads
// and global dwordx4 stores, head and tail are byte stores.  Neighbouring tiles share boundary words, so no lane
// writes a byte outside [tile_off[tile], tile_off[tile] + the tile's bytes).
//
// Where the records come from is a small decode functor: DumpRaw reads them as they sit in a file, DumpArrays from
// (keys, counts) arrays on the device (a finished counter; the answer of k_query), DumpScan (scan_kernel.h) from the
// window starts of scanned sequences.  A source says per record whether it has a line at all: line(i).
#pragma once
#include "dump_text.h"
#include "table_kernels.h"

namespace kmd {

constexpr uint32_t DUMP_THREADS = SCAN_THREADS;   // (block_exclusive_scan is written for that many)
constexpr uint32_t DUMP_TILE = DUMP_THREADS;      // records per block, one per lane: an image of at most 11.3 KiB, so
                                                  // the eight blocks that fill a CU's 32 wave slots need 90 of 160 KiB
constexpr uint32_t DUMP_IMAGE_BYTES = DUMP_TILE * (32u + 13u) + 16u;   // worst lines of k = 32, + the residue shift
// records of one piece: tiles + 1 entries fit one scan chunk (and the text stays far inside 32 bits)
constexpr uint64_t DUMP_MAX_RECORDS = (uint64_t)(SCAN_CHUNK - 1) * DUMP_TILE;

struct DumpRule {
  int32_t k, fmt;
  uint32_t lower, upper;
};

// raw[0 .. n * (kb + cb)): `binary/sorted` records as they sit in a file, [kb key bytes][cb count bytes], kb 1..8,
// cb 1..4, little-endian, raw 16-byte aligned.  12-byte records are three aligned dwords; other widths go by bytes.
struct DumpRaw {
  const uint8_t* raw;
  uint32_t kb, cb;
  __device__ bool line(uint32_t) const { return true; }
  __device__ uint32_t count(uint32_t i) const {
    if (kb == 8 && cb == 4) return reinterpret_cast<const uint32_t*>(raw)[3ull * i + 2];
    const uint8_t* p = raw + (uint64_t)i * (kb + cb) + kb;
    uint32_t c = 0;
    for (uint32_t b = 0; b < cb; ++b) c |= (uint32_t)p[b] << (8 * b);
    return c;
  }
  __device__ uint64_t key(uint32_t i) const {
    if (kb == 8 && cb == 4) {
      const uint32_t* p = reinterpret_cast<const uint32_t*>(raw) + 3ull * i;
      return ((uint64_t)p[1] << 32) | p[0];
    }
    const uint8_t* p = raw + (uint64_t)i * (kb + cb);
    uint64_t v = 0;
    for (uint32_t b = 0; b < kb; ++b) v |= (uint64_t)p[b] << (8 * b);
    return v;
  }
};

struct DumpArrays {
  const uint64_t* keys;
  const uint32_t* counts;
  __device__ bool line(uint32_t) const { return true; }
  __device__ uint32_t count(uint32_t i) const { return counts[i]; }
  __device__ uint64_t key(uint32_t i) const { return keys[i]; }
};

// the line length of record i of the piece (0: none, no line, or filtered out) and its count
template <typename Src>
__device__ inline uint32_t dump_lane_len(const Src& src, uint32_t i, uint32_t n, const DumpRule& r, uint32_t* count) {
  if (i >= n || !src.line(i)) return 0;
  const uint32_t c = src.count(i);
  *count = c;
  return kmdump::kept(c, r.lower, r.upper) ? kmdump::line_len(r.k, kmdump::digits(c), r.fmt) : 0u;
}

template <typename Src>
__global__ __launch_bounds__(DUMP_THREADS) void k_dump_sizes(Src src, uint32_t n, DumpRule r, uint32_t* tile_bytes,
                                                             uint32_t* tile_kept) {
  __shared__ uint32_t wave_bytes[DUMP_THREADS / 64], wave_kept[DUMP_THREADS / 64];
  uint32_t c = 0;
  const uint32_t len = dump_lane_len(src, blockIdx.x * DUMP_TILE + threadIdx.x, n, r, &c);
  uint32_t sum = len;
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  const uint32_t kept = (uint32_t)__popcll(__ballot(len != 0));
  if (lane_id() == 0) {
    wave_bytes[threadIdx.x >> 6] = sum;
    wave_kept[threadIdx.x >> 6] = kept;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t b = 0, m = 0;
    for (uint32_t w = 0; w < DUMP_THREADS / 64; ++w) {
      b += wave_bytes[w];
      m += wave_kept[w];
    }
    tile_bytes[blockIdx.x] = b;
    tile_kept[blockIdx.x] = m;
  }
}

// tile_off: the exclusive scan of tile_bytes.  text: 16-byte aligned, room for tile_off[tiles] bytes.
template <typename Src>
__global__ __launch_bounds__(DUMP_THREADS) void k_dump_write(Src src, uint32_t n, DumpRule r, const uint32_t* tile_off,
                                                             uint8_t* text) {
  __shared__ __attribute__((aligned(16))) uint8_t image[DUMP_IMAGE_BYTES];
  const uint32_t i = blockIdx.x * DUMP_TILE + threadIdx.x;
  uint32_t c = 0;
  const uint32_t len = dump_lane_len(src, i, n, r, &c);
  uint32_t total;
  const uint32_t at = block_exclusive_scan(len, &total);
  const uint32_t base = tile_off[blockIdx.x];
  const uint32_t shift = base & 15u;                   // image[shift + j] is text[base + j]
  if (len) (void)kmdump::put_record(reinterpret_cast<char*>(image) + shift + at, src.key(i), c, r.k, r.fmt);
  __syncthreads();
  const uint32_t head = min(total, (16u - shift) & 15u);   // bytes in front of the first 16-byte boundary
  const uint32_t n_vec = (total - head) / 16u;
  const uint32_t tail_at = head + n_vec * 16u;
  uint8_t* dst = text + base;
  const uint8_t* img = image + shift;
  if (threadIdx.x < head) dst[threadIdx.x] = img[threadIdx.x];
  uint4* dst_vec = reinterpret_cast<uint4*>(dst + head);
  const uint4* img_vec = reinterpret_cast<const uint4*>(img + head);
  for (uint32_t v = threadIdx.x; v < n_vec; v += DUMP_THREADS) dst_vec[v] = img_vec[v];
  if (threadIdx.x < total - tail_at) dst[tail_at + threadIdx.x] = img[tail_at + threadIdx.x];
}

}  // namespace kmd
