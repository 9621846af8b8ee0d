// jf_order_kernel.h — records in Jellyfish's own file order: pos = M · key over GF(2), sorted by (pos, key).
// DESIGN.md §10 "File, Jellyfish order".  Host side: jf_order_host.h.
#pragma once
#include "device_common.h"

namespace kmd {

constexpr int JF_THREADS = 256;
constexpr uint32_t JF_LDS_SORT = 2048;     // entries one block sorts in LDS (20 B each: 40 KB, 4 blocks per CU)

// Bucket of a position: its top `bits` bits (of the r it has).  bits == 0: one bucket.
__device__ inline uint32_t jf_bucket(uint64_t pos, int shift, int bits) { return bits ? (uint32_t)(pos >> shift) : 0u; }

// pos[i] = XOR over the set bits b of keys[i] of columns[c - 1 - b], masked to r bits; hist[bucket(pos)] += 1.
// The matrix is laid out per block as 8 tables of 256 words indexed by one key byte each (16 KB of LDS): a key
// costs 8 ds_read_b64 and 7 XORs.  The table index is data, so the lanes of a half-wave spread over the 64 banks
// at random (two dwords per read): some 2- and 3-way conflicts per read, no systematic one.
__global__ __launch_bounds__(JF_THREADS) void k_jf_position(const uint64_t* columns, int c, uint64_t mask,
                                                            const uint64_t* keys, uint64_t n, uint64_t* pos,
                                                            uint32_t* hist, int shift, int bits) {
  __shared__ uint64_t tab[8][256];
  for (uint32_t e = threadIdx.x; e < 8 * 256; e += JF_THREADS) {
    const uint32_t byte = e >> 8, v = e & 255;
    uint64_t x = 0;
    for (uint32_t j = 0; j < 8; ++j) {
      const int b = (int)(8 * byte + j);
      if (((v >> j) & 1) && b < c) x ^= columns[c - 1 - b];
    }
    tab[byte][v] = x & mask;
  }
  __syncthreads();
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t key = keys[i];
    uint64_t p = 0;
#pragma unroll
    for (int byte = 0; byte < 8; ++byte) p ^= tab[byte][(key >> (8 * byte)) & 255];
    pos[i] = p;
    atomicAdd(&hist[jf_bucket(p, shift, bits)], 1u);
  }
}

// off[] is the exclusive scan of the histogram; cursor[] starts at zero.  Which record of a bucket lands where
// inside it depends on the order of the atomics; the sort that follows does not care.
__global__ void k_jf_scatter(const uint64_t* pos, const uint64_t* keys, const uint32_t* counts, uint64_t n,
                             const uint32_t* off, uint32_t* cursor, int shift, int bits, uint64_t* pos2,
                             uint64_t* keys2, uint32_t* counts2) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t p = pos[i];
    const uint32_t b = jf_bucket(p, shift, bits);
    const uint32_t at = off[b] + atomicAdd(&cursor[b], 1u);
    pos2[at] = p;
    keys2[at] = keys[i];
    counts2[at] = counts[i];
  }
}

// stats[0] = largest bucket, stats[1] = buckets above JF_LDS_SORT
__global__ void k_jf_bucket_stats(const uint32_t* off, uint32_t n_buckets, unsigned long long* stats) {
  for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < n_buckets; b += gridDim.x * blockDim.x) {
    const uint32_t m = off[b + 1] - off[b];
    atomicMax(&stats[0], (unsigned long long)m);
    if (m > JF_LDS_SORT) atomicAdd(&stats[1], 1ull);
  }
}

// Bitonic sort of m entries by (pos, key), ascending, by the whole block, for any m: the network is the one for
// the next power of two with every exchange ascending (the first step of a merge pairs i with its mirror image
// in the block, the others i with i + j), and a pair whose upper index is >= m is skipped — what the exchange
// with an entry larger than all others would do.  Called with LDS arrays and with global ones (inlined: the
// address space follows the caller's pointers).
__device__ __forceinline__ void jf_bitonic(uint64_t* pos, uint64_t* key, uint32_t* cnt, uint32_t m) {
  uint32_t P = 1;
  while (P < m) P <<= 1;
  for (uint32_t k = 2; k <= P; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t t = threadIdx.x; t < (P >> 1); t += JF_THREADS) {
        const uint32_t base = 2 * j * (t / j), r = t % j;
        const uint32_t i = base + r;
        const uint32_t l = (j == (k >> 1)) ? base + 2 * j - 1 - r : i + j;
        if (l < m) {
          const uint64_t pi = pos[i], pl = pos[l], ki = key[i], kl = key[l];
          if (pl < pi || (pl == pi && kl < ki)) {
            pos[i] = pl; pos[l] = pi;
            key[i] = kl; key[l] = ki;
            const uint32_t ci = cnt[i];
            cnt[i] = cnt[l]; cnt[l] = ci;
          }
        }
      }
      __syncthreads();
    }
  }
}

// The finished file record of entry `at`: kb little-endian key bytes, 4 count bytes (the inverse of
// k_unpack_records).
__device__ inline void jf_put_record(unsigned char* records, uint64_t at, uint32_t kb, uint64_t key, uint32_t cnt) {
  if (kb == 8) {                                   // 12-byte records: three aligned dwords
    uint32_t* w = reinterpret_cast<uint32_t*>(records) + 3 * at;
    w[0] = (uint32_t)key;
    w[1] = (uint32_t)(key >> 32);
    w[2] = cnt;
  } else {
    unsigned char* r = records + at * (kb + 4);
    for (uint32_t b = 0; b < kb; ++b) r[b] = (unsigned char)(key >> (8 * b));
    for (uint32_t b = 0; b < 4; ++b) r[kb + b] = (unsigned char)(cnt >> (8 * b));
  }
}

// One block per bucket (grid-stride over the buckets): sort its entries and write their records, and their
// positions if asked, at the bucket's offset.  A bucket of at most JF_LDS_SORT entries is sorted in LDS; a
// larger one (positions that share their top bits: a degenerate matrix, not real keys) by the same network in
// place in pos2 / keys2 / counts2, one block working in global memory — slow and exact.
__global__ __launch_bounds__(JF_THREADS) void k_jf_sort_buckets(const uint32_t* off, uint32_t n_buckets,
                                                                uint64_t* pos2, uint64_t* keys2, uint32_t* counts2,
                                                                uint32_t kb, unsigned char* records,
                                                                uint64_t* pos_out) {
  __shared__ uint64_t s_pos[JF_LDS_SORT];
  __shared__ uint64_t s_key[JF_LDS_SORT];
  __shared__ uint32_t s_cnt[JF_LDS_SORT];
  for (uint32_t b = blockIdx.x; b < n_buckets; b += gridDim.x) {
    const uint32_t lo = off[b], m = off[b + 1] - lo;
    if (m == 0) continue;
    if (m <= JF_LDS_SORT) {
      for (uint32_t t = threadIdx.x; t < m; t += JF_THREADS) {
        s_pos[t] = pos2[lo + t];
        s_key[t] = keys2[lo + t];
        s_cnt[t] = counts2[lo + t];
      }
      __syncthreads();
      jf_bitonic(s_pos, s_key, s_cnt, m);
      for (uint32_t t = threadIdx.x; t < m; t += JF_THREADS) {
        jf_put_record(records, (uint64_t)lo + t, kb, s_key[t], s_cnt[t]);
        if (pos_out) pos_out[lo + t] = s_pos[t];
      }
      __syncthreads();                             // the next bucket overwrites the arrays
    } else {
      // (the entries come from the kernel before; between the steps of the network the block's barrier, which
      // carries a workgroup-scope fence, makes one wave's global stores visible to the others: all waves of a
      // block share one CU's vector cache — the code object is not built for tgsplit mode)
      jf_bitonic(pos2 + lo, keys2 + lo, counts2 + lo, m);
      for (uint32_t t = threadIdx.x; t < m; t += JF_THREADS) {
        jf_put_record(records, (uint64_t)lo + t, kb, keys2[lo + t], counts2[lo + t]);
        if (pos_out) pos_out[lo + t] = pos2[lo + t];
      }
    }
  }
}

}  // namespace kmd
