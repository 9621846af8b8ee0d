// The largest number of reference k-mers the LDS tier of the walk and graph kernels accepts, asked of the batch's own
// geometry code (km_amd/csrc/tier_geometry.h: fast_tier_fits, what km_batch bisects over) for the k and max_break
// given.  Prints "<largest n_ref that fits> <n_ref the bisection settles on for a longer target>".  No GPU is touched.
#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include "../../km_amd/csrc/tier_geometry.h"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const int k = atoi(argv[1]);
  const uint32_t bcap = std::min<uint32_t>((uint32_t)atoi(argv[2]), FAST_BCAP_MAX - 1) + 1;
  uint32_t largest = 0;
  for (uint32_t n = 1; n < 0xFFFF; ++n) if (fast_tier_fits(k, n, bcap)) largest = n;
  uint32_t lo = 1, hi = 0xFFFF;                // (as fast_geometry does between 1 and the longest target)
  while (lo + 1 < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (fast_tier_fits(k, mid, bcap)) lo = mid; else hi = mid;
  }
  printf("%u %u\n", largest, lo);
  return 0;
}
