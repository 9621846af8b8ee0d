// select_pair_rule.cpp — km_amd/csrc/select_pair_rule.h on the CPU (built with AddressSanitizer + UBSan by
// tests/test_select_pair_cpu.py): two FASTQ texts (mate 1, mate 2) and a table come in as a file; for each given staging
// size the two texts go the way km_select_pair_add_fastq sends two final streams: a piece of whole records from each
// (kmcut::next_piece), per mate a line table, a masked copy and every lane's hit walk as tests/host/select_rule.cpp makes
// them, then for R = min(records 1, records 2) the pair's lengths (kmpair::pair_lens), the name comparison
// (kmpair::names_agree), the two scans, every word of both gathers (kmsel::gather_word with R, not the piece's own record
// count) and the consumed offsets (kmpair::consumed), by which either stream advances: the surplus records of the longer
// side are sent again with the next piece.  Every array has exactly the size of its device buffer, reads and writes go
// through at(), and what lies behind a piece's bytes is filled with bases and '@'.
//
//   select_pair_rule <input file>
//   input: "k canonical min_hits invert min_qual rule check_names n_table n_stages len1 len2", the staging sizes, n_table
//          lines "key count", the line "TEXT", then len1 + len2 raw bytes
//   output per staging size: "STAGE s PIECES p PAIRS n KEPT m RESENT a b", then either "NAMES r" (the first pair whose
//          names differ), "COUNT mate r" (the mate with more records, the first pair without a partner) or nothing, then
//          "OUT1 len", the bytes, "OUT2 len", the bytes: what the pieces before a failure left
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../km_amd/csrc/fastq_cut.h"
#include "../../km_amd/csrc/select_pair_rule.h"

namespace {
constexpr uint32_t SCAN_CHUNK = 4096;    // table_kernels.h
int g_k = 0, g_canonical = 0;
unsigned g_min_qual = 0;
std::unordered_map<uint64_t, uint32_t> g_table;

void die(const char* what) {
  fprintf(stderr, "select_pair_rule: %s\n", what);
  exit(2);
}

struct Env {
  std::vector<uint32_t>& hits;
  uint32_t count(uint64_t fwd, uint64_t rev) const {
    const auto it = g_table.find(g_canonical && rev < fwd ? rev : fwd);
    return it == g_table.end() ? 0u : it->second;
  }
  void add(uint32_t r, uint32_t c) { hits.at(r) += c; }
};

struct Load {
  const std::vector<uint8_t>& text;
  kmsel::U128 operator()(uint32_t a) const {
    if (a & 15u) die("unaligned source load");
    kmsel::U128 x{0, 0};
    for (int j = 0; j < 8; ++j) x.lo |= (uint64_t)text.at(a + j) << (8 * j);
    for (int j = 0; j < 8; ++j) x.hi |= (uint64_t)text.at(a + 8 + j) << (8 * j);
    return x;
  }
};

struct Byte {
  const std::vector<uint8_t>& text;
  uint32_t n;
  uint32_t operator()(uint32_t i) const {
    if (i >= n) die("a name read behind its piece");
    return text.at(i);
  }
};

// one mate's piece with the buffers the device has for it, after the front half, k_sel_clear and k_sel_hits
struct Side {
  uint32_t n = 0, n_rec = 0;
  std::vector<uint8_t> text, masked, out;
  std::vector<uint32_t> line_start, hits, len;
  Side(uint64_t stage, const char* src, uint32_t n_) : n(n_), text(stage + kmscan::PAD, (uint8_t)'@'),
      masked(stage + kmscan::PAD, (uint8_t)'A'), out(stage + kmsel::OUT_PAD, 0xEE), line_start(stage + 2, 0xFFFFFFFFu),
      hits(kmsel::hit_cells(stage), 0xDEADu), len(kmsel::len_chunks(stage, SCAN_CHUNK) * SCAN_CHUNK, 0xDEADu) {
    memcpy(text.data(), src, n);
    uint32_t newlines = 0;
    line_start.at(0) = 0;
    for (uint32_t i = 0; i < n; ++i)
      if (text[i] == '\n') line_start.at(++newlines) = i + 1;
    line_start.at(newlines + 1) = n + 1;
    const uint32_t n_lines = kmsel::line_count(newlines, text[n - 1] == '\n');
    for (uint32_t l = 0; l < n_lines; ++l) {
      const uint32_t s = line_start[l], e = std::min(line_start[l + 1] - 1, n);
      for (uint32_t i = s; i < std::min(e + 1, n); ++i) masked[i] = '\n';
      if ((l & 3u) != 1u) continue;
      for (uint32_t i = s; i < e; ++i) {
        const uint8_t ch = text[i];
        if (ch == '\r') continue;
        const uint64_t qp = l + 2 < n_lines ? (uint64_t)line_start[l + 2] + (i - s) : n;
        if (g_min_qual == 0 || (qp < n && text[qp] >= g_min_qual)) masked[i] = ch;
      }
    }
    n_rec = kmsel::record_count(n_lines, n);
    if ((n_lines & 3u) || n_rec != n_lines / 4 || n_rec == 0) die("the piece is not whole records");
    for (uint32_t i = 0; i < (n_lines >> 2) + 1u; ++i) hits.at(i) = 0;
    Env env{hits};
    for (uint32_t s = 0; s < n; s += kmscan::RUN) {
      uint32_t w[16];
      for (int d = 0; d < 16; ++d) {
        const uint8_t* b = &masked.at(s + 4 * d + 3) - 3;
        w[d] = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
      }
      kmsel::lane_hits(w, s, n, line_start.data(), n_lines, g_k, env);
    }
  }
  uint32_t n_pad() const { return (uint32_t)(kmsel::len_chunks(n, SCAN_CHUNK) * SCAN_CHUNK); }
  // k_scan_*, then every word of the gather with n_pairs as the bound -> the mate's total
  uint32_t scan_and_gather(uint32_t n_pairs, uint32_t total) {
    uint32_t run = 0;
    for (uint32_t r = 0; r < n_pad(); ++r) {
      const uint32_t l = len.at(r);
      len[r] = run;
      run += l;
    }
    if (len.at(n_pairs) != total || total > n) die("the scanned lengths do not end in the total");
    Load load{text};
    for (uint32_t w = 0; (uint64_t)w * kmsel::WORD < total; ++w) {
      const kmsel::U128 x = kmsel::gather_word(load, line_start.data(), len.data(), n_pairs, total, w);
      for (int j = 0; j < 8; ++j) {
        out.at((uint64_t)w * 16 + j) = (uint8_t)(x.lo >> (8 * j));
        out.at((uint64_t)w * 16 + 8 + j) = (uint8_t)(x.hi >> (8 * j));
      }
    }
    for (uint64_t i = total; i < ((uint64_t)total + 15) / 16 * 16; ++i)
      if (out[i] != 0) die("bytes behind the total are not zero");
    for (uint64_t i = ((uint64_t)total + 15) / 16 * 16; i < out.size(); ++i)
      if (out[i] != 0xEE) die("a byte behind the last word was written");
    return total;
  }
};
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) die("usage: select_pair_rule <input>");
  FILE* fh = fopen(argv[1], "rb");
  if (!fh) die("cannot open the input");
  unsigned min_hits = 0, rule = 0;
  int invert = 0, check_names = 0;
  unsigned long long n_table = 0, n_stages = 0, len[2] = {0, 0};
  if (fscanf(fh, "%d %d %u %d %u %u %d %llu %llu %llu %llu", &g_k, &g_canonical, &min_hits, &invert, &g_min_qual, &rule,
             &check_names, &n_table, &n_stages, &len[0], &len[1]) != 11) die("header");
  std::vector<uint64_t> stages(n_stages);
  for (auto& v : stages) { unsigned long long x; if (fscanf(fh, "%llu", &x) != 1) die("stages"); v = x; }
  for (unsigned long long i = 0; i < n_table; ++i) {
    unsigned long long key; unsigned count;
    if (fscanf(fh, "%llu %u", &key, &count) != 2) die("table");
    g_table[key] = count;
  }
  char word[8] = {0};
  if (fscanf(fh, "%7s", word) != 1 || strcmp(word, "TEXT") != 0 || fgetc(fh) != '\n') die("TEXT");
  std::vector<char> all[2];
  for (int m = 0; m < 2; ++m) {
    all[m].resize(len[m]);
    if (len[m] && fread(all[m].data(), 1, len[m], fh) != len[m]) die("text");
  }
  fclose(fh);

  // ---- the score at its edges
  if (kmpair::score(0xFFFFFFFFu, 1u, kmpair::RULE_SUM) != 0xFFFFFFFFu || kmpair::score(0x80000000u, 0x80000000u, kmpair::RULE_SUM) != 0xFFFFFFFFu ||
      kmpair::score(0x7FFFFFFFu, 0x80000000u, kmpair::RULE_SUM) != 0xFFFFFFFFu || kmpair::score(3u, 4u, kmpair::RULE_SUM) != 7u ||
      kmpair::score(3u, 4u, kmpair::RULE_ANY) != 4u || kmpair::score(3u, 4u, kmpair::RULE_BOTH) != 3u) die("score");

  for (const uint64_t stage : stages) {
    uint64_t pieces = 0, pairs = 0, kept_all = 0, pos[2] = {0, 0}, resent[2] = {0, 0};
    std::string out_all[2], failure;
    while (pos[0] < len[0] && pos[1] < len[1]) {
      uint32_t take[2];
      for (int m = 0; m < 2; ++m) {
        take[m] = (uint32_t)kmcut::next_piece(all[m].data(), pos[m], len[m], stage);
        if (take[m] == 0) die("no record ends within a staging buffer");
      }
      ++pieces;
      Side a(stage, all[0].data() + pos[0], take[0]), b(stage, all[1].data() + pos[1], take[1]);
      // ---- k_pair_sizes
      const uint32_t n_pairs = kmpair::pair_count(a.n_rec, b.n_rec);
      uint32_t total[2] = {0, 0}, kept = 0;
      for (uint32_t r = 0; r < std::max(a.n_pad(), b.n_pad()); ++r) {
        kmpair::Lens l{0u, 0u, false};
        if (r < n_pairs)
          l = kmpair::pair_lens(a.line_start.data(), a.n, b.line_start.data(), b.n, r, a.hits.at(r), b.hits.at(r), rule,
                                min_hits, invert != 0);
        if (r < a.n_pad()) a.len.at(r) = l.len1;
        if (r < b.n_pad()) b.len.at(r) = l.len2;
        total[0] += l.len1;
        total[1] += l.len2;
        kept += l.kept;
      }
      const uint32_t used[2] = {kmpair::consumed(a.line_start.data(), n_pairs, a.n), kmpair::consumed(b.line_start.data(), n_pairs, b.n)};
      if (n_pairs == 0 || used[0] == 0 || used[1] == 0 || used[0] > a.n || used[1] > b.n) die("a piece made no pair");
      if ((a.n_rec == n_pairs) != (used[0] == a.n) || (b.n_rec == n_pairs) != (used[1] == b.n)) die("consumed offsets");
      // ---- k_pair_names
      if (check_names) {
        Byte b1{a.text, a.n}, b2{b.text, b.n};
        uint32_t r = 0;
        while (r < n_pairs && kmpair::names_agree(b1, kmsel::record_begin(a.line_start.data(), r), a.n, b2,
                                                  kmsel::record_begin(b.line_start.data(), r), b.n)) ++r;
        if (r < n_pairs) {
          failure = "NAMES " + std::to_string(pairs + r) + "\n";
          break;
        }
      }
      // ---- k_scan_*, k_pair_gather
      a.scan_and_gather(n_pairs, total[0]);
      b.scan_and_gather(n_pairs, total[1]);
      Side* side[2] = {&a, &b};
      for (int m = 0; m < 2; ++m) {
        out_all[m].append(reinterpret_cast<const char*>(side[m]->out.data()), total[m]);
        if (pos[m] + used[m] == len[m] && total[m] && side[m]->out[total[m] - 1] != '\n') out_all[m].push_back('\n');
        resent[m] += take[m] - used[m];
        pos[m] += used[m];
      }
      pairs += n_pairs;
      kept_all += kept;
    }
    if (failure.empty() && (pos[0] < len[0]) != (pos[1] < len[1]))
      failure = "COUNT " + std::to_string(pos[0] < len[0] ? 1 : 2) + " " + std::to_string(pairs) + "\n";
    printf("STAGE %llu PIECES %llu PAIRS %llu KEPT %llu RESENT %llu %llu\n", (unsigned long long)stage, (unsigned long long)pieces,
           (unsigned long long)pairs, (unsigned long long)kept_all, (unsigned long long)resent[0], (unsigned long long)resent[1]);
    fputs(failure.c_str(), stdout);
    for (int m = 0; m < 2; ++m) {
      printf("OUT%d %zu\n", m + 1, out_all[m].size());
      fwrite(out_all[m].data(), 1, out_all[m].size(), stdout);
    }
  }
  printf("SELECT PAIR RULE OK\n");
  return 0;
}
