// kmin_rule.h — the closed form of `km linear_kmin`: from a target's length n, the reference's
// --start, the longest repeated substring R and the kernel's flag to the k the reference prints (plain C++17, no HIP
// headers, so kmin_host.h and tests/host/kmin_rule.cpp run the same code).
//
//   n == 0            -> flag = 0; 0 if start <= 0, else start - 1
//   R == 0            -> flag = (n >= 3): at k = 1 every (k-1)-mer is ""
//   start - 1 >= n    -> start - 1 (the reference's loop never runs)
//   lo = max(start, R + 1); lo > R + 1 -> lo; else flag ? min(R + 2, n) : R + 1
#pragma once
#include <stdint.h>

#include <algorithm>

namespace kmlin {

// *flag comes in as the kernel's "some run of length R is not exempt" and leaves as the flag the call reports
inline int32_t kmin_closed_form(uint64_t n, int32_t start, uint64_t R, uint8_t* flag) {
  if (n == 0) { *flag = 0; return start <= 0 ? 0 : start - 1; }
  if (R == 0) *flag = n >= 3;                          // k = 1: every (k-1)-mer is ""
  if ((int64_t)start - 1 >= (int64_t)n) return start - 1;   // the reference's loop never runs
  const int64_t lo = std::max<int64_t>(start, (int64_t)R + 1);
  if (lo > (int64_t)R + 1) return (int32_t)lo;
  return (int32_t)(*flag ? std::min<uint64_t>(R + 2, n) : R + 1);
}

}  // namespace kmlin
