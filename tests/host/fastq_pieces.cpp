// fastq_pieces.cpp — the piece cutter of km_amd/csrc/fastq_cut.h on the CPU (built with AddressSanitizer + UBSan by
// tests/test_fastq_pieces_cpu.py): kmcut::call_end and kmcut::next_piece, the two functions by which every consumer of
// raw FASTQ text (km_counter_add_fastq, km_select_add_fastq, kmjf_fastq_hits, km_select_pair_add_fastq) cuts a call
// into pieces of whole records.  Texts come in as a file; each is cut as a non-final and as a final call at every
// staging size from 6 bytes to its length + 1, in the loop the library runs, out of a buffer of exactly the text's
// size.  The pieces go to standard output, where the test compares them with its own model.
//
//   fastq_pieces <input file>
//   input: "n_texts", then per text "len" on a line of its own and len raw bytes
//   output: "TEXT i", then per staging size and kind of call "S stage F final END end P len len ..." and, where no
//           record ends within a staging buffer, " X offset" behind the pieces before it
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../km_amd/csrc/fastq_cut.h"

namespace {
void die(const char* what) {
  fprintf(stderr, "fastq_pieces: %s\n", what);
  exit(2);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) die("usage: fastq_pieces <input>");
  FILE* fh = fopen(argv[1], "rb");
  if (!fh) die("cannot open the input");
  unsigned long long n_texts = 0;
  if (fscanf(fh, "%llu", &n_texts) != 1) die("header");
  for (unsigned long long t = 0; t < n_texts; ++t) {
    unsigned long long len = 0;
    if (fscanf(fh, "%llu", &len) != 1 || fgetc(fh) != '\n') die("length");
    std::vector<char> text(len);
    if (len && fread(text.data(), 1, len, fh) != len) die("text");
    printf("TEXT %llu\n", t);
    for (uint64_t stage = 6; stage <= len + 1; ++stage)
      for (int final = 0; final < 2; ++final) {
        const uint64_t end = kmcut::call_end(text.data(), len, final != 0);
        if (end > len) die("a call ends behind its text");
        printf("S %llu F %d END %llu P", (unsigned long long)stage, final, (unsigned long long)end);
        for (uint64_t pos = 0; pos < end;) {
          const uint64_t take = kmcut::next_piece(text.data(), pos, end, stage);
          if (take == 0) {
            printf(" X %llu", (unsigned long long)pos);
            break;
          }
          if (take > end - pos) die("a piece ends behind its call");
          printf(" %llu", (unsigned long long)take);
          pos += take;
        }
        printf("\n");
      }
  }
  fclose(fh);
  printf("FASTQ PIECES OK\n");
  return 0;
}
