// kmin_kernel.h — `km linear_kmin` (km/tools/linear_kmin.py:7-46) as one reduction over all diagonals.
//
// For a target s of length n the reference looks for the smallest k >= start at which the k-mers of s
// are unique (km/utils/common.py:48-63) and their (k-1)-overlap graph is linear.  Both tests are
// monotone in k, so the answer follows from two numbers:
//   R    = the longest repeated substring of s (overlaps allowed) = the longest maximal run of
//          s[a] == s[a+d] over every diagonal d >= 1;
//   flag = some run of length R is not one of the three exempt (k-1)-mer pairs at k = R+1.
// A maximal run that starts at x on diagonal d with length len (it ends at p = x + len) is exempt iff
//   (d == 1 && x == 0) || (d == 1 && p + d == n) || (x == 0 && p + d == n),
// i.e. on the diagonal's own length L = n - d: the run that covers the whole diagonal, and on d == 1
// the diagonal's first and last run.  The host turns (R, flag) into k (km_linear_kmin in kmgpu.hip).
//
// Work unit = (target, 64 consecutive diagonals d0 .. d0+63), one wave.  Lane l walks diagonal
// d = d0 + l four bytes per step: every lane reads the same aligned word s[a..a+3] and its own
// s[a+d..a+d+3], funnelled out of two aligned words with v_alignbyte (the lane keeps the upper word for
// the next step, so each step loads one new dword per lane; the 64 lanes read 68 consecutive bytes).
// Four steps per loop iteration, their loads issued together.
// Equality is decided per byte, exactly: high bit of byte i of ((x & 0x7f..) + 0x7f..) | x is set iff
// byte i of x = u ^ v is non-zero.  Runs are then read off with ctz / clz / popcount:
//   z   = equal bytes below the first unequal one: they close the run carried in (cur + z);
//   top = equal bytes above the last unequal one: they open the run carried out;
//   the bytes between can hold runs of at most 2, looked at only while the lane's best is below 3.
// Bytes past the diagonal's end count as unequal, so the run that reaches the end closes at p == L.
// Each lane keeps key = max over its runs of (len << 1 | not_exempt); the wave takes the max and one
// lane merges it into the target's 64-bit key with atomicMax: a longer run wins, and at equal length
// flag = 1 wins, which is the OR over the runs of length R.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kmd {

constexpr uint32_t KMIN_LANES = 64;            // diagonals per work unit (one wave)
constexpr uint32_t KMIN_WAVES_PER_BLOCK = 4;
constexpr uint32_t KMIN_PAD = 128;             // readable bytes past the end of the staged text

// key of a run that ends at p (exclusive) with length len on a diagonal of length L
__device__ inline uint32_t kmin_run_key(uint32_t len, uint32_t p, uint32_t L, bool d1) {
  const bool x0 = (p == len), pe = (p == L);
  const bool exempt = (x0 && (d1 || pe)) || (d1 && pe);
  return (len << 1) | (exempt ? 0u : 1u);
}

// text:     the targets, each at a 16-byte aligned offset stage_off[t], KMIN_PAD readable bytes after the last
// len:      n of each target
// unit_off: [n_targets + 1] exclusive prefix of the units per target (ceil((n - 1) / 64) for n >= 2, else 0)
// keys:     [n_targets] zeroed by the caller; (R << 1) | flag on return
__global__ __launch_bounds__(KMIN_LANES * KMIN_WAVES_PER_BLOCK)
void k_linear_kmin(const uint8_t* __restrict__ text, const uint64_t* __restrict__ stage_off,
                   const uint32_t* __restrict__ len, const uint32_t* __restrict__ unit_off,
                   uint32_t n_targets, uint32_t n_units, unsigned long long* __restrict__ keys) {
  const uint32_t unit = blockIdx.x * KMIN_WAVES_PER_BLOCK + (threadIdx.x >> 6);
  if (unit >= n_units) return;                 // wave-uniform
  const uint32_t lane = threadIdx.x & 63;
  // the target of this unit: the last t with unit_off[t] <= unit (targets without units share its offset)
  uint32_t lo = 0, hi = n_targets;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (unit_off[mid] <= unit) lo = mid; else hi = mid;
  }
  const uint32_t t = lo;
  const uint32_t n = len[t];
  const uint8_t* s = text + stage_off[t];
  const uint32_t d0 = 1 + (unit - unit_off[t]) * KMIN_LANES;
  const uint32_t d = d0 + lane;
  const uint32_t L = n > d ? n - d : 0;        // this lane's diagonal length (0: past the last diagonal)
  const uint32_t steps_end = n - d0;           // the longest diagonal of the unit (lane 0)
  const bool d1 = (d == 1);
  const uint32_t sh = d & 3;

  uint32_t cur = 0, key = 0;
  // one step: the 4 bytes at a of the target (u) against the 4 bytes at a + d (v)
  auto step = [&](uint32_t u, uint32_t v, uint32_t a) {
    const uint32_t x = u ^ v;
    uint32_t ne = (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
    const int rem = (int)(L - a);              // bytes of this step still on the diagonal
    if (rem < 4) ne |= 0x80808080u << (8 * (rem > 0 ? rem : 0));
    if (ne == 0) {
      cur += 4;
      return;
    }
    const uint32_t z = (uint32_t)__builtin_ctz(ne) >> 3;
    const uint32_t top = (uint32_t)__builtin_clz(ne) >> 3;
    const uint32_t run = cur + z;
    if (run) key = max(key, kmin_run_key(run, a + z, L, d1));
    const uint32_t mid = 4 - z - top - (uint32_t)__builtin_popcount(ne);   // equal bytes strictly inside
    if (mid && key < 5) {
      uint32_t c = 0;
      for (uint32_t i = z + 1; i <= 3 - top; ++i) {
        if ((ne >> (8 * i + 7)) & 1) {
          if (c) key = max(key, kmin_run_key(c, a + i, L, d1));
          c = 0;
        } else {
          ++c;
        }
      }
    }
    cur = top;
  };
  // 16 bytes per iteration, every load issued before the first step uses one.  Steps past a lane's end see
  // only unequal bytes and change nothing (the one at a == L closes the run that reaches the end).
  const uint32_t* lane_w = reinterpret_cast<const uint32_t*>(s + (d & ~3u));
  uint32_t w0 = lane_w[0];
  for (uint32_t a = 0; a < steps_end; a += 16) {
    const uint4 u = *reinterpret_cast<const uint4*>(s + a);
    const uint32_t* p = lane_w + (a >> 2);
    const uint32_t w1 = p[1], w2 = p[2], w3 = p[3], w4 = p[4];
    step(u.x, __builtin_amdgcn_alignbyte(w1, w0, sh), a);
    step(u.y, __builtin_amdgcn_alignbyte(w2, w1, sh), a + 4);
    step(u.z, __builtin_amdgcn_alignbyte(w3, w2, sh), a + 8);
    step(u.w, __builtin_amdgcn_alignbyte(w4, w3, sh), a + 12);
    w0 = w4;
  }
  if (cur) key = max(key, kmin_run_key(cur, L, L, d1));   // lane 0 when its diagonal ends on a step boundary

  for (int o = 32; o > 0; o >>= 1) key = max(key, (uint32_t)__shfl_xor((int)key, o));
  if (lane == 0 && key) atomicMax(keys + t, (unsigned long long)key);
}

}  // namespace kmd
