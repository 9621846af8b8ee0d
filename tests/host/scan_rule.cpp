// scan_rule.cpp — km_amd/csrc/scan_rule.h on the CPU (built with AddressSanitizer + UBSan by tests/test_scan_cpu.py):
// a batch of sequences and a table come in as a file, the batch is cut into pieces for each given staging size, every
// lane of every piece walks its 64 bytes exactly as the kernels' lanes do (kmscan::lane_walk, with the sequence of its
// first byte from kmscan::seq_of over the piece's slice of the offsets), and the statistics per sequence and the text
// go to standard output, where the test compares them with its own model.  The staged piece is copied into a buffer
// of exactly the size the device buffer has, and what lies behind the piece's bytes is filled with bases: a lane that
// looked at them would count windows that do not exist.
//
//   scan_rule <input file>
//   input: "k canonical n_seqs n_table n_stages text_len", the n_seqs + 1 offsets, the staging sizes, n_table lines
//          "key count", the line "TEXT", then text_len raw bytes
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../km_amd/csrc/dump_text.h"
#include "../../km_amd/csrc/scan_rule.h"

namespace {
int g_k = 0, g_canonical = 0;
std::unordered_map<uint64_t, uint32_t> g_table;

uint32_t lookup(uint64_t fwd, uint64_t rev) {
  const auto it = g_table.find(g_canonical && rev < fwd ? rev : fwd);
  return it == g_table.end() ? 0u : it->second;
}

struct StatsSink {
  std::vector<kmscan::Acc>& cells;
  kmscan::Acc a;
  void flush(uint64_t q) {                               // what the atomics do to a cell
    kmscan::Acc& c = cells[q];
    c.total += a.total;
    c.n_kmers += a.n_kmers;
    c.n_zero += a.n_zero;
    c.n_skipped += a.n_skipped;
    c.n_nonbase += a.n_nonbase;
    if (a.n_kmers) {
      c.min = std::min(c.min, a.min);
      c.max = std::max(c.max, a.max);
    }
    kmscan::acc_clear(a);
  }
  void leave(uint64_t q) { flush(q); }
  void nonbase() { ++a.n_nonbase; }
  void window(uint32_t, uint64_t fwd, uint64_t rev, bool valid) {
    if (valid) kmscan::acc_count(a, lookup(fwd, rev));
    else ++a.n_skipped;
  }
};

struct TextSink {
  uint64_t* keys;
  uint32_t* counts;
  uint32_t lines;
  void leave(uint64_t) {}
  void nonbase() {}
  void window(uint32_t j, uint64_t fwd, uint64_t rev, bool valid) {
    if (!valid) return;
    keys[j] = kmscan::printed_key(fwd, rev, g_canonical);
    counts[j] = lookup(fwd, rev);
    lines |= 1u << j;
  }
};

void die(const char* what) {
  fprintf(stderr, "scan_rule: %s\n", what);
  exit(2);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) die("usage: scan_rule <input>");
  FILE* fh = fopen(argv[1], "rb");
  if (!fh) die("cannot open the input");
  unsigned long long n_seqs = 0, n_table = 0, n_stages = 0, text_len = 0;
  if (fscanf(fh, "%d %d %llu %llu %llu %llu", &g_k, &g_canonical, &n_seqs, &n_table, &n_stages, &text_len) != 6) die("header");
  std::vector<uint64_t> off(n_seqs + 1), stages(n_stages);
  for (auto& v : off) { unsigned long long x; if (fscanf(fh, "%llu", &x) != 1) die("offsets"); v = x; }
  for (auto& v : stages) { unsigned long long x; if (fscanf(fh, "%llu", &x) != 1) die("stages"); v = x; }
  for (unsigned long long i = 0; i < n_table; ++i) {
    unsigned long long key; unsigned count;
    if (fscanf(fh, "%llu %u", &key, &count) != 2) die("table");
    g_table[key] = count;
  }
  char word[8] = {0};
  if (fscanf(fh, "%7s", word) != 1 || strcmp(word, "TEXT") != 0 || fgetc(fh) != '\n') die("TEXT");
  std::vector<uint8_t> text(text_len);
  if (text_len && fread(text.data(), 1, text_len, fh) != text_len) die("text");
  fclose(fh);
  const int k = g_k;
  const uint64_t begin = off[0], end = off[n_seqs];
  if (end > text_len) die("offsets beyond the text");

  // ---- the rule's small parts against brute force
  uint64_t windows = 0, by_position = 0;
  for (uint64_t q = 0; q < n_seqs; ++q) windows += kmscan::n_windows(off[q + 1] - off[q], k);
  {
    uint64_t q = 0;
    for (uint64_t p = begin; p < end; ++p) {
      while (off[q + 1] <= p) ++q;                       // the sequence of p by stepping
      if (kmscan::seq_of(off.data(), 0, n_seqs - 1, p) != q) die("seq_of disagrees with stepping");
      by_position += kmscan::window_in_seq(p, k, off[q], off[q + 1]) ? 1 : 0;
      if (q > 0 && kmscan::window_in_seq(p, k, off[q - 1], off[q])) die("a window of the sequence before");
    }
  }
  if (by_position != windows) die("window_in_seq disagrees with n_windows");
  printf("WINDOWS %llu\n", (unsigned long long)windows);

  // ---- per staging size: pieces, lanes, statistics and text
  for (const uint64_t stage : stages) {
    if (stage < (uint64_t)k) die("a staging size below k");
    const uint64_t per = kmscan::starts_per_piece(stage, k);
    const uint64_t pieces = end > begin ? kmscan::n_pieces(begin, end, per) : 0;
    std::vector<kmscan::Acc> cells(n_seqs);
    for (auto& c : cells) kmscan::acc_clear(c);
    std::string out;
    uint64_t next_start = begin;
    for (uint64_t i = 0; i < pieces; ++i) {
      const kmscan::Piece p = kmscan::piece(begin, end, per, k, i);
      if (p.first != next_start || p.n_starts == 0 || p.n_bytes > stage || p.first + p.n_bytes > end) die("piece arithmetic");
      next_start = p.first + p.n_starts;
      // every window whose start the piece owns is complete in its bytes
      if (p.n_bytes < p.n_starts || (p.first + p.n_bytes < end && p.n_bytes != p.n_starts + (uint64_t)k - 1)) die("piece overlap");
      std::vector<uint8_t> staged(stage + kmscan::PAD, (uint8_t)'A');        // exactly the device buffer
      memcpy(staged.data(), text.data() + p.first, p.n_bytes);
      const uint64_t q_lo = (uint64_t)(std::upper_bound(off.begin(), off.end() - 1, p.first) - off.begin()) - 1;
      const uint64_t q_hi = (uint64_t)(std::upper_bound(off.begin(), off.end() - 1, p.first + p.n_starts - 1) - off.begin()) - 1;
      std::vector<uint64_t> keys(p.n_starts);
      std::vector<uint32_t> counts(p.n_starts), lines((p.n_starts + kmscan::RUN - 1) / kmscan::RUN);
      for (uint64_t s = 0; s < p.n_starts; s += kmscan::RUN) {
        uint32_t w[16];
        for (int d = 0; d < 16; ++d) {                   // four aligned 16-byte loads: 64 bytes from s, inside the buffer
          const uint8_t* b = &staged.at(s + 4 * d + 3) - 3;
          w[d] = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
        }
        const uint64_t g0 = p.first + s;
        const uint32_t own = (uint32_t)std::min<uint64_t>(kmscan::RUN, p.n_starts - s);
        const uint64_t q = kmscan::seq_of(off.data(), q_lo, q_hi, g0);
        StatsSink stats{cells, {}};
        kmscan::acc_clear(stats.a);
        stats.flush(kmscan::lane_walk(w, g0, own, end, off.data(), q, k, stats));
        TextSink ts{keys.data() + s, counts.data() + s, 0u};
        (void)kmscan::lane_walk(w, g0, own, end, off.data(), q, k, ts);
        lines[s / kmscan::RUN] = ts.lines;
      }
      for (uint64_t j = 0; j < p.n_starts; ++j) {
        if (!((lines[j >> 5] >> (j & 31)) & 1u)) continue;
        char line[64];
        const uint32_t n = kmdump::put_record(line, keys[j], counts[j], k, KM_DUMP_COLUMN);
        out.append(line, n);
      }
    }
    if (pieces && next_start != end) die("the pieces do not cover the text");
    printf("STAGE %llu PIECES %llu\n", (unsigned long long)stage, (unsigned long long)pieces);
    for (const auto& c : cells)
      printf("%llu %u %u %u %u %u %u\n", (unsigned long long)c.total, c.n_kmers, c.n_zero, c.n_skipped, c.n_nonbase, c.min, c.max);
    printf("TEXT %zu\n", out.size());
    fwrite(out.data(), 1, out.size(), stdout);
  }
  printf("SCAN RULE OK\n");
  return 0;
}
