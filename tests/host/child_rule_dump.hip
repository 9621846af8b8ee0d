// Host dump of the integer form of Jellyfish.get_child's keep rule (km/utils/Jellyfish.py:69-72) as
// km_amd/csrc/device_common.h states it: for every "sum ratio n_cutoff" line on stdin (ratio as a hex
// float, so that nothing is rounded again on the way in) one line
//     T none below thr_T
// with T / none from child_threshold (threshold_of behind it) and below / thr_T from
// threshold_shortcut.  tests/test_child_rule.py compares them with the rule written out in Python.
// No GPU is touched.
#include <cinttypes>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include "../../km_amd/csrc/device_common.h"

using namespace kmd;

int main() {
  char line[256];
  while (fgets(line, sizeof line, stdin)) {
    char* p = line;
    const uint64_t sum = strtoull(p, &p, 10);
    const double ratio = strtod(p, &p);
    const int64_t n_cutoff = strtoll(p, &p, 10);
    bool none = false;
    const uint32_t T = child_threshold(sum, ratio, n_cutoff, &none);
    uint64_t below = 0;
    uint32_t thr_T = 0;
    threshold_shortcut(ratio, n_cutoff, &below, &thr_T);
    printf("%" PRIu32 " %d %" PRIu64 " %" PRIu32 "\n", T, none ? 1 : 0, below, thr_T);
  }
  return 0;
}
