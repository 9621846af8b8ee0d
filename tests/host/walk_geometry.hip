// The sizes km_batch launches the LDS tier of k_dfs and k_graph with, asked of the batch's own geometry code
// (km_amd/csrc/tier_geometry.h: fast_tier_geometry, what batch_host.h's fast_geometry calls) for k, the batch's longest
// target in bases, max_stack and max_break.  Prints "hs_cap pcap words_cap fcap bcap ncap hcap".  With a fifth
// argument N it prints one such line for every target length from k to N bases instead.  No GPU is touched.
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include "../../km_amd/csrc/tier_geometry.h"

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const int k = atoi(argv[1]);
  const uint32_t len = (uint32_t)atoi(argv[2]), max_stack = (uint32_t)atoi(argv[3]), max_break = (uint32_t)atoi(argv[4]);
  const uint32_t last = argc > 5 ? (uint32_t)atoi(argv[5]) : len;
  for (uint32_t L = len; L <= last; ++L) {
    const uint32_t max_nref = L >= (uint32_t)k ? L - (uint32_t)k + 1 : 1;      // (as fast_geometry reads max_len)
    const FastGeometry g = fast_tier_geometry(k, max_nref, max_stack, max_break);
    printf("%u %u %u %u %u %u %u\n", g.hs_cap, g.pcap, g.words_cap, g.fcap, g.bcap, g.ncap, g.hcap);
  }
  return 0;
}
