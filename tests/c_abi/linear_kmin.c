/* A plain-C client of libkmgpu.so's km_linear_kmin: `km linear_kmin -s START FILE..` for plain FASTA files
 * (records joined, upper-cased), one call for all files.  Built and run by
 * tests/test_linear_kmin.py::test_gpu_plain_c_consumer (gcc, no Python, no torch in the process). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kmgpu.h"

/* appends the sequence lines of a FASTA file, upper-cased, to *buf */
static int read_fasta(const char* path, char** buf, size_t* len, size_t* cap) {
  FILE* f = fopen(path, "r");
  if (!f) return -1;
  char line[4096];
  int in_record = 0, at_line_start = 1;
  while (fgets(line, sizeof line, f)) {
    if (at_line_start && line[0] == '>') in_record = 1;
    else if (in_record && !(at_line_start && line[0] == '>'))
      for (char* p = line; *p && *p != '\n' && *p != '\r'; ++p) {
        if (*len + 1 >= *cap) *buf = (char*)realloc(*buf, *cap *= 2);
        (*buf)[(*len)++] = (*p >= 'a' && *p <= 'z') ? (char)(*p - 32) : *p;
      }
    at_line_start = strchr(line, '\n') != NULL;
  }
  fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s <start> <target.fa>..\n", argv[0]); return 2; }
  const int32_t start = (int32_t)atoi(argv[1]);
  const uint32_t n = (uint32_t)(argc - 2);
  size_t len = 0, cap = 1 << 16;
  char* bases = (char*)malloc(cap);
  uint64_t* off = (uint64_t*)calloc(n + 1, sizeof *off);
  int32_t* kmin = (int32_t*)calloc(n, sizeof *kmin);
  for (uint32_t t = 0; t < n; ++t) {
    if (read_fasta(argv[2 + t], &bases, &len, &cap)) { fprintf(stderr, "cannot read %s\n", argv[2 + t]); return 2; }
    off[t + 1] = len;
  }
  int rc = km_linear_kmin(0, (const uint8_t*)bases, off, n, start, kmin, NULL, NULL, NULL);
  if (rc != KM_OK) { fprintf(stderr, "km_linear_kmin: %s (%s)\n", km_strerror(rc), km_last_error()); return 1; }
  printf("target_name\tlinear_kmin\n");
  for (uint32_t t = 0; t < n; ++t) {
    const char* name = strrchr(argv[2 + t], '/');
    name = name ? name + 1 : argv[2 + t];
    const char* dot = strrchr(name, '.');
    printf("%.*s\t%d\n", (int)(dot && dot != name ? dot - name : (long)strlen(name)), name, kmin[t]);
  }
  free(bases); free(off); free(kmin);
  return 0;
}
