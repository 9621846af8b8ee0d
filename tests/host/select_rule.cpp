// select_rule.cpp — km_amd/csrc/select_rule.h on the CPU (built with AddressSanitizer + UBSan by
// tests/test_select_cpu.py): a FASTQ text and a table come in as a file; for each given staging size the text is cut into
// pieces of whole records by the library's own cutter (kmcut::next_piece), and every piece goes the way it goes on the
// device: a line table and a masked copy (made here from the rule of fastq_kernel.h's header comment, byte by byte),
// then every lane's hit walk (kmsel::lane_hits), the sizes, their exclusive scan, and every word of the gather
// (kmsel::gather_word).  Every array has exactly the size of its device buffer, reads and writes go through at(), and
// what lies behind a piece's bytes is filled with bases and '@': a lane that looked there would count or copy them.
// Hits per record and the gathered bytes go to standard output, where the test compares them with its own model.
//
//   select_rule <input file>
//   input: "k canonical min_hits invert min_qual n_table n_stages text_len", the staging sizes, n_table lines
//          "key count", the line "TEXT", then text_len raw bytes
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../km_amd/csrc/fastq_cut.h"
#include "../../km_amd/csrc/select_rule.h"

namespace {
constexpr uint32_t SCAN_CHUNK = 4096;    // table_kernels.h
int g_k = 0, g_canonical = 0;
std::unordered_map<uint64_t, uint32_t> g_table;

void die(const char* what) {
  fprintf(stderr, "select_rule: %s\n", what);
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
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) die("usage: select_rule <input>");
  FILE* fh = fopen(argv[1], "rb");
  if (!fh) die("cannot open the input");
  unsigned min_hits = 0, min_qual = 0;
  int invert = 0;
  unsigned long long n_table = 0, n_stages = 0, text_len = 0;
  if (fscanf(fh, "%d %d %u %d %u %llu %llu %llu", &g_k, &g_canonical, &min_hits, &invert, &min_qual, &n_table, &n_stages,
             &text_len) != 8) die("header");
  std::vector<uint64_t> stages(n_stages);
  for (auto& v : stages) { unsigned long long x; if (fscanf(fh, "%llu", &x) != 1) die("stages"); v = x; }
  for (unsigned long long i = 0; i < n_table; ++i) {
    unsigned long long key; unsigned count;
    if (fscanf(fh, "%llu %u", &key, &count) != 2) die("table");
    g_table[key] = count;
  }
  char word[8] = {0};
  if (fscanf(fh, "%7s", word) != 1 || strcmp(word, "TEXT") != 0 || fgetc(fh) != '\n') die("TEXT");
  std::vector<char> all(text_len);
  if (text_len && fread(all.data(), 1, text_len, fh) != text_len) die("text");
  fclose(fh);
  const int k = g_k;

  // ---- the byte shifts against a plain byte loop
  for (uint32_t s = 0; s <= 16; ++s) {
    uint8_t b[16];
    for (int j = 0; j < 16; ++j) b[j] = (uint8_t)(0x11 * j + 7);
    kmsel::U128 x{0, 0};
    for (int j = 0; j < 8; ++j) { x.lo |= (uint64_t)b[j] << (8 * j); x.hi |= (uint64_t)b[8 + j] << (8 * j); }
    auto byte = [](kmsel::U128 v, uint32_t j) { return (uint8_t)((j < 8 ? v.lo >> (8 * j) : v.hi >> (8 * (j - 8))) & 0xFF); };
    const kmsel::U128 up = kmsel::bytes_up(x, s);
    for (uint32_t j = 0; j < 16; ++j)
      if (byte(up, j) != (j >= s ? b[j - s] : 0)) die("bytes_up");
    if (s < 16) {
      const kmsel::U128 down = kmsel::bytes_down(x, s);
      for (uint32_t j = 0; j < 16; ++j)
        if (byte(down, j) != (j + s < 16 ? b[j + s] : 0)) die("bytes_down");
    }
    if (s >= 1) {
      const kmsel::U128 first = kmsel::bytes_first(x, s);
      for (uint32_t j = 0; j < 16; ++j)
        if (byte(first, j) != (j < s ? b[j] : 0)) die("bytes_first");
    }
  }

  for (const uint64_t stage : stages) {
    uint64_t pieces = 0;
    std::vector<uint32_t> all_hits;
    std::string out_all;
    for (uint64_t pos = 0; pos < text_len;) {
      const uint64_t take = kmcut::next_piece(all.data(), pos, text_len, stage);
      if (take == 0) die("no record ends within a staging buffer");
      ++pieces;
      const uint32_t n = (uint32_t)take;
      // ---- the buffers, as the device has them
      std::vector<uint8_t> text(stage + kmscan::PAD, (uint8_t)'@'), masked(stage + kmscan::PAD, (uint8_t)'A');
      memcpy(text.data(), all.data() + pos, n);
      std::vector<uint32_t> line_start(stage + 2, 0xFFFFFFFFu);
      std::vector<uint32_t> hits(kmsel::hit_cells(stage), 0xDEADu);
      std::vector<uint32_t> len(kmsel::len_chunks(stage, SCAN_CHUNK) * SCAN_CHUNK, 0xDEADu);
      std::vector<uint8_t> out(stage + kmsel::OUT_PAD, 0xEE);
      // ---- the front half: line table and mask, from the rule
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
          if (min_qual == 0 || (qp < n && text[qp] >= min_qual)) masked[i] = ch;
        }
      }
      // ---- record bounds from the line table
      const uint32_t n_rec = kmsel::record_count(n_lines, n);
      if ((n_lines & 3u) || n_rec != n_lines / 4) die("the piece is not whole records");
      if (n_rec == 0 || kmsel::record_begin(line_start.data(), 0) != 0 || kmsel::record_end(line_start.data(), n_rec - 1, n) != n)
        die("record bounds do not cover the piece");
      for (uint32_t r = 0; r + 1 < n_rec; ++r)
        if (kmsel::record_end(line_start.data(), r, n) != kmsel::record_begin(line_start.data(), r + 1)) die("record bounds");
      // ---- k_sel_clear, k_sel_hits
      for (uint32_t i = 0; i < (n_lines >> 2) + 1u; ++i) hits.at(i) = 0;
      Env env{hits};
      for (uint32_t s = 0; s < n; s += kmscan::RUN) {
        uint32_t w[16];
        for (int d = 0; d < 16; ++d) {                   // four aligned 16-byte loads: 64 bytes from s, inside the buffer
          const uint8_t* b = &masked.at(s + 4 * d + 3) - 3;
          w[d] = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
        }
        kmsel::lane_hits(w, s, n, line_start.data(), n_lines, k, env);
      }
      // ---- k_sel_sizes, k_scan_*
      const uint64_t n_pad = kmsel::len_chunks(n, SCAN_CHUNK) * SCAN_CHUNK;
      uint32_t total = 0;
      for (uint64_t r = 0; r < n_pad; ++r) {
        const uint32_t l = r < n_rec ? kmsel::record_len(line_start.data(), (uint32_t)r, n, hits.at(r), min_hits, invert != 0) : 0u;
        len.at(r) = l;
        total += l;
      }
      uint32_t run = 0;
      for (uint64_t r = 0; r < n_pad; ++r) {
        const uint32_t l = len[r];
        len[r] = run;
        run += l;
      }
      if (len.at(n_rec) != total || total > n) die("the scanned lengths do not end in the total");
      // ---- k_sel_gather: every word
      Load load{text};
      for (uint32_t w = 0; (uint64_t)w * kmsel::WORD < total; ++w) {
        const kmsel::U128 x = kmsel::gather_word(load, line_start.data(), len.data(), n_rec, total, w);
        for (int j = 0; j < 8; ++j) {
          out.at((uint64_t)w * 16 + j) = (uint8_t)(x.lo >> (8 * j));
          out.at((uint64_t)w * 16 + 8 + j) = (uint8_t)(x.hi >> (8 * j));
        }
      }
      for (uint64_t i = total; i < ((uint64_t)total + 15) / 16 * 16; ++i)
        if (out[i] != 0) die("bytes behind the total are not zero");
      for (uint64_t i = ((uint64_t)total + 15) / 16 * 16; i < out.size(); ++i)
        if (out[i] != 0xEE) die("a byte behind the last word was written");
      all_hits.insert(all_hits.end(), hits.begin(), hits.begin() + n_rec);
      out_all.append(reinterpret_cast<const char*>(out.data()), total);
      if (pos + take == text_len && total && out[total - 1] != '\n') out_all.push_back('\n');   // (the host's newline)
      pos += take;
    }
    printf("STAGE %llu PIECES %llu RECORDS %zu\n", (unsigned long long)stage, (unsigned long long)pieces, all_hits.size());
    for (const uint32_t h : all_hits) printf("%u\n", h);
    printf("OUT %zu\n", out_all.size());
    fwrite(out_all.data(), 1, out_all.size(), stdout);
  }
  printf("SELECT RULE OK\n");
  return 0;
}
