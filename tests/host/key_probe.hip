// "bucket tag flip cls" of make_key (km_amd/csrc/device_common.h) for (k-1)-mers, on the host: the table view is
// filled the way table_shape (km_amd/csrc/db_host.h) fills it before a build.  No GPU is touched.
//   key_probe K CANONICAL LOG2_BUCKETS [P ...]      P: a (k-1)-mer as a decimal or 0x number; none given: one per line
//                                                   of stdin
#include <cinttypes>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include "../../km_amd/csrc/device_common.h"

static uint64_t mask_bits(int nbases) { return nbases >= 32 ? ~0ull : ((1ull << (2 * nbases)) - 1); }

static kmd::TableView shape(int k, int canonical, uint32_t n_buckets) {
  kmd::TableView t;
  memset(&t, 0, sizeof t);
  t.kmask = mask_bits(k);
  t.pmask = mask_bits(k - 1);
  t.n_buckets = n_buckets;
  t.bshift = 31;
  while (t.bshift > 1 && (1ull << (32 - t.bshift)) < n_buckets) --t.bshift;
  t.unit = 2;
  t.max_probe = 2;
  t.k = k;
  t.canonical = canonical;
  t.m = kmd::minimizer_len(k);
  t.w = k - t.m;
  t.mmask = (uint32_t)mask_bits(t.m);
  t.inv32 = (uint32_t)((1ull << 32) / ((uint64_t)2 * t.w * 256));
  t.cshift = 1;
  while ((1u << t.cshift) < 2u * (uint32_t)t.w) ++t.cshift;
  return t;
}

static void show(const kmd::TableView& t, uint64_t P) {
  const kmd::Key key = kmd::make_key(t, P & t.pmask);
  printf("%u %" PRIu64 " %u %u\n", key.bucket, key.tag, key.flip, key.cls);
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const int k = atoi(argv[1]), canonical = atoi(argv[2]), log2b = atoi(argv[3]);
  if (k < 2 || k > 32 || log2b < 1 || log2b > 30) return 2;
  const kmd::TableView t = shape(k, canonical, 1u << log2b);
  for (int i = 4; i < argc; ++i) show(t, strtoull(argv[i], nullptr, 0));
  if (argc == 4) {
    char line[64];
    while (fgets(line, sizeof line, stdin)) {
      if (line[0] == '\n' || line[0] == 0) continue;
      show(t, strtoull(line, nullptr, 0));
    }
  }
  return 0;
}
