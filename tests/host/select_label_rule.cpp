// select_label_rule.cpp — km_amd/csrc/select_label_rule.h on the CPU (built with AddressSanitizer + UBSan by
// tests/test_select_label_cpu.py): a FASTQ text and a label table come in as a file; for each given staging size the
// text is cut into pieces of whole records by the library's own cutter (kmcut::next_piece), and every piece goes the
// way it goes on the device: a line table and a masked copy (made here from the rule of fastq_kernel.h's header
// comment, byte by byte, as tests/host/select_rule.cpp makes them), then every lane's label walk
// (kmlab::lane_label_hits), the sizes of every label (kmlab::keep_mask), the exclusive scan of all planes as one
// array, the label offsets, and every word of every gather pass (kmlab::stream_word with its first word w0) into an
// output buffer of exactly the device buffer's size, cut at the label offsets as the host cuts it.  Every array has
// exactly the size of its device buffer and reads and writes go through at().  Hits per label and record, the figures
// and the outputs go to standard output, where the test compares them with its own model.
//
//   select_label_rule <input file>
//   input: "k canonical min_hits min_qual n_labels n_table n_stages text_len", the staging sizes, n_table lines
//          "key mask", the line "TEXT", then text_len raw bytes
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../km_amd/csrc/fastq_cut.h"
#include "../../km_amd/csrc/select_label_rule.h"

namespace {
constexpr uint32_t SCAN_CHUNK = 4096;    // table_kernels.h
int g_k = 0, g_canonical = 0;
std::unordered_map<uint64_t, uint32_t> g_table;

void die(const char* what) {
  fprintf(stderr, "select_label_rule: %s\n", what);
  exit(2);
}

struct Env {
  std::vector<uint32_t>& hits;
  uint64_t hit_stride;
  uint32_t mask(uint64_t fwd, uint64_t rev) const {
    const auto it = g_table.find(g_canonical && rev < fwd ? rev : fwd);
    return it == g_table.end() ? 0u : it->second;
  }
  void add(uint32_t l, uint32_t r, uint32_t c) {
    if (r >= hit_stride) die("a hit lands outside its plane");
    hits.at(l * hit_stride + r) += c;
  }
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
  if (argc != 2) die("usage: select_label_rule <input>");
  FILE* fh = fopen(argv[1], "rb");
  if (!fh) die("cannot open the input");
  unsigned min_hits = 0, min_qual = 0, n_labels = 0;
  unsigned long long n_table = 0, n_stages = 0, text_len = 0;
  if (fscanf(fh, "%d %d %u %u %u %llu %llu %llu", &g_k, &g_canonical, &min_hits, &min_qual, &n_labels, &n_table, &n_stages,
             &text_len) != 8) die("header");
  if (n_labels < 1 || n_labels > kmlab::MAX_LABELS) die("n_labels");
  std::vector<uint64_t> stages(n_stages);
  for (auto& v : stages) { unsigned long long x; if (fscanf(fh, "%llu", &x) != 1) die("stages"); v = x; }
  for (unsigned long long i = 0; i < n_table; ++i) {
    unsigned long long key; unsigned mask;
    if (fscanf(fh, "%llu %u", &key, &mask) != 2) die("table");
    g_table[key] = mask;
  }
  char word[8] = {0};
  if (fscanf(fh, "%7s", word) != 1 || strcmp(word, "TEXT") != 0 || fgetc(fh) != '\n') die("TEXT");
  std::vector<char> all(text_len);
  if (text_len && fread(all.data(), 1, text_len, fh) != text_len) die("text");
  fclose(fh);
  const int k = g_k;

  for (const uint64_t stage : stages) {
    if ((uint64_t)n_labels * stage >= (1ull << 32)) die("n_labels * stage does not fit 32 bits");
    uint64_t pieces = 0, passes = 0, any = 0, multi = 0;
    std::vector<std::vector<uint32_t>> all_hits(n_labels);
    std::vector<std::string> out_all(n_labels);
    std::vector<uint64_t> kept(n_labels, 0);
    const uint64_t cap = kmlab::pass_bytes(stage + kmsel::OUT_PAD);
    const uint64_t hit_stride = kmsel::hit_cells(stage);
    for (uint64_t pos = 0; pos < text_len;) {
      const uint64_t take = kmcut::next_piece(all.data(), pos, text_len, stage);
      if (take == 0) die("no record ends within a staging buffer");
      ++pieces;
      const uint32_t n = (uint32_t)take;
      // ---- the buffers, as the device has them
      std::vector<uint8_t> text(stage + kmscan::PAD, (uint8_t)'@'), masked(stage + kmscan::PAD, (uint8_t)'A');
      memcpy(text.data(), all.data() + pos, n);
      std::vector<uint32_t> line_start(stage + 2, 0xFFFFFFFFu);
      std::vector<uint32_t> hits(hit_stride * n_labels, 0xDEADu);
      std::vector<uint32_t> len(kmsel::len_chunks(stage, SCAN_CHUNK) * SCAN_CHUNK * n_labels, 0xDEADu);
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
      const uint32_t n_rec = kmsel::record_count(n_lines, n);
      if ((n_lines & 3u) || n_rec != n_lines / 4 || n_rec == 0) die("the piece is not whole records");
      // ---- k_lab_clear, k_lab_hits
      for (uint32_t l = 0; l < n_labels; ++l)
        for (uint32_t i = 0; i < (n_lines >> 2) + 1u; ++i) hits.at(l * hit_stride + i) = 0;
      Env env{hits, hit_stride};
      for (uint32_t s = 0; s < n; s += kmscan::RUN) {
        uint32_t w[16];
        for (int d = 0; d < 16; ++d) {                   // four aligned 16-byte loads: 64 bytes from s, inside the buffer
          const uint8_t* b = &masked.at(s + 4 * d + 3) - 3;
          w[d] = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
        }
        kmlab::lane_label_hits(w, s, n, line_start.data(), n_lines, k, n_labels, env);
      }
      // ---- k_lab_sizes, k_scan_*, k_lab_offsets
      const uint32_t stride = kmlab::len_stride(n, SCAN_CHUNK);
      if ((uint64_t)stride * n_labels > len.size()) die("the planes of a piece do not fit the length array");
      for (uint32_t r = 0; r < stride; ++r) {
        const uint32_t keep = r < n_rec ? kmlab::keep_mask(hits.data(), hit_stride, r, n_labels, min_hits) : 0u;
        const uint32_t bytes = r < n_rec ? kmlab::record_bytes(line_start.data(), r, n) : 0u;
        for (uint32_t l = 0; l < n_labels; ++l) {
          len.at((uint64_t)l * stride + r) = (keep >> l) & 1u ? bytes : 0u;
          kept[l] += (keep >> l) & 1u;
        }
        any += keep != 0u;
        multi += (keep & (keep - 1u)) != 0u;
      }
      uint32_t run = 0;
      for (uint64_t v = 0; v < (uint64_t)stride * n_labels; ++v) {
        const uint32_t l = len[v];
        len[v] = run;
        if (run + l < run) die("the scan wraps");
        run += l;
      }
      const uint32_t total = run;
      std::vector<uint32_t> label_off(n_labels + 1);
      for (uint32_t l = 0; l <= n_labels; ++l) label_off[l] = kmlab::label_begin(len.data(), n_labels, stride, l);
      if (label_off[0] != 0 || label_off[n_labels] != total) die("label_off does not span the stream");
      // ---- k_lab_gather: every pass, every word; the host's cut at the label offsets
      Load load{text};
      const uint64_t n_pass = kmlab::pass_count(total, cap);
      passes += n_pass;
      const bool close = pos + take == text_len && text[n - 1] != '\n';
      for (uint64_t p = 0; p < n_pass; ++p) {
        std::fill(out.begin(), out.end(), 0xEE);
        const uint64_t lo = p * cap, hi = std::min<uint64_t>(total, lo + cap);
        const uint32_t w0 = (uint32_t)(lo / kmsel::WORD);
        for (uint32_t w = 0; (uint64_t)(w0 + w) * kmsel::WORD < hi; ++w) {
          const kmsel::U128 x = kmlab::stream_word(load, line_start.data(), len.data(), n_labels, stride, total, w0 + w);
          for (int j = 0; j < 8; ++j) {
            out.at((uint64_t)w * 16 + j) = (uint8_t)(x.lo >> (8 * j));
            out.at((uint64_t)w * 16 + 8 + j) = (uint8_t)(x.hi >> (8 * j));
          }
        }
        const uint64_t got = hi - lo, padded = (got + 15) / 16 * 16;
        if (hi == total)
          for (uint64_t i = got; i < padded; ++i)
            if (out[i] != 0) die("bytes behind the total are not zero");
        for (uint64_t i = padded; i < out.size(); ++i)
          if (out[i] != 0xEE) die("a byte behind the last word was written");
        for (uint32_t l = 0; l < n_labels; ++l) {
          const uint64_t a = std::max<uint64_t>(label_off[l], lo), b = std::min<uint64_t>(label_off[l + 1], hi);
          if (a >= b) continue;
          out_all[l].append(reinterpret_cast<const char*>(out.data()) + (a - lo), b - a);
          if (close && b == label_off[l + 1] && out[b - lo - 1] != '\n') out_all[l].push_back('\n');   // (the host's newline)
        }
      }
      for (uint32_t l = 0; l < n_labels; ++l)
        all_hits[l].insert(all_hits[l].end(), hits.begin() + l * hit_stride, hits.begin() + l * hit_stride + n_rec);
      pos += take;
    }
    printf("STAGE %llu PIECES %llu RECORDS %zu PASSES %llu ANY %llu MULTI %llu\n", (unsigned long long)stage,
           (unsigned long long)pieces, all_hits[0].size(), (unsigned long long)passes, (unsigned long long)any,
           (unsigned long long)multi);
    for (uint32_t l = 0; l < n_labels; ++l) {
      printf("LABEL %u KEPT %llu OUT %zu HITS", l, (unsigned long long)kept[l], out_all[l].size());
      for (const uint32_t h : all_hits[l]) printf(" %u", h);
      printf("\n");
      fwrite(out_all[l].data(), 1, out_all[l].size(), stdout);
    }
  }
  printf("SELECT LABEL RULE OK\n");
  return 0;
}
