// rle_less of the delivery (km_amd/csrc/deliver_kernel.h: the order k_out_pack ranks a target's paths by), on the
// host.  stdin holds pairs of run lists as unsigned numbers separated by white space:
//   na  start len (na times)  nb  start len (nb times)
// For every pair one line "x y" is printed: x = rle_less(a, b), y = rle_less(b, a).  Every list sits in a heap block
// of exactly its size, so a read past a list's end is an error under AddressSanitizer.  No GPU is touched.
#include <cstdio>
#include <cstdint>
#include <memory>
#include "../../km_amd/csrc/deliver_kernel.h"

struct Runs {
  uint32_t n = 0;
  std::unique_ptr<uint32_t[]> start, len;
  bool read() {
    if (scanf("%u", &n) != 1) return false;
    start.reset(new uint32_t[n]);
    len.reset(new uint32_t[n]);
    for (uint32_t i = 0; i < n; ++i)
      if (scanf("%u %u", &start[i], &len[i]) != 2) return false;
    return true;
  }
};

int main() {
  for (;;) {
    Runs a, b;
    if (!a.read()) break;
    if (!b.read()) return 2;                         // (half a pair)
    printf("%d %d\n", (int)kmd::rle_less(a.start.get(), a.len.get(), a.n, b.start.get(), b.len.get(), b.n),
           (int)kmd::rle_less(b.start.get(), b.len.get(), b.n, a.start.get(), a.len.get(), a.n));
  }
  return 0;
}
