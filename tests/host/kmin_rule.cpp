// kmin_rule.cpp — km_amd/csrc/kmin_rule.h on the CPU (built with AddressSanitizer + UBSan by
// tests/test_linear_kmin_edges.py): the closed form that turns (n, start, R, flag) into the k `km linear_kmin` prints.
//
//   kmin_rule < lines of "n start R flag"  >  lines of "k flag" (the flag as the call reports it), then "KMIN RULE OK"
#include <cstdio>
#include <cstdlib>

#include "../../km_amd/csrc/kmin_rule.h"

int main() {
  unsigned long long n, R;
  long long start;
  unsigned flag;
  int got;
  while ((got = scanf("%llu %lld %llu %u", &n, &start, &R, &flag)) == 4) {
    if (start < INT32_MIN || start > INT32_MAX || flag > 1) {
      fprintf(stderr, "kmin_rule: start or flag out of range\n");
      return 2;
    }
    uint8_t f = (uint8_t)flag;
    const int32_t k = kmlin::kmin_closed_form(n, (int32_t)start, R, &f);
    printf("%d %u\n", k, (unsigned)f);
  }
  if (got != EOF) {
    fprintf(stderr, "kmin_rule: a line that is not four numbers\n");
    return 2;
  }
  printf("KMIN RULE OK\n");
  return 0;
}
