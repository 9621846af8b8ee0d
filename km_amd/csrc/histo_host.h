// histo_host.h — km_histo_layout, km_counter_histo, km_jf_histo, km_histo_kernel_ms, the two text exports (host part
// of kmgpu.hip; device side: histo_kernel.h; the bin rule, its checks and the text: histo_layout.h)
// ------------------------------------------------------------------ histogram of counts and table statistics
// One streaming pass over counts that already sit in HBM — the counting table of a live counter, the kept counts of a
// finished one — or over the record area of a file as it comes, piece by piece (merge_pieces.h), out of a RecordFile
// (db_host.h) through a Staging of the call's own (host_common.h) on a CallStream.  Nothing is changed: a live counter
// takes further add_* and finish afterwards.
namespace {
thread_local float g_histo_kernel_ms = 0.f;

// (low, high, increment) and the cut as the kernels take them; KM_E_ARG as histo_layout.h words it
int histo_rule(uint64_t low, uint64_t high, uint64_t inc, uint32_t lower_count, uint32_t upper_count, kmhisto::Layout* lay,
               HistoRule* r) {
  char why[160];
  if (kmhisto::make(low, high, inc, lay, why, sizeof why)) return fail(KM_E_ARG, "%s", why);
  r->base = lay->base;
  r->ceil = lay->ceil;
  r->inc = (uint32_t)std::min<uint64_t>(inc, 0xFFFFFFFFull);
  r->n_bins = (uint32_t)lay->n_bins;
  r->lo = std::max<uint32_t>(lower_count, 1);
  r->hi = upper_count;
  r->rounds = HISTO_ROUNDS;
  return KM_OK;
}

// The aggregation depth of the two calls that launch kernels: KM_HISTO_ROUNDS (include/kmgpu.h; the tests, and the runs
// that chose the default) or HISTO_ROUNDS.
uint32_t histo_rounds() {
  if (const char* e = getenv("KM_HISTO_ROUNDS")) return (uint32_t)std::min<unsigned long long>(strtoull(e, nullptr, 10), 64);
  return HISTO_ROUNDS;
}

uint32_t histo_grid(uint64_t items) {
  const uint64_t per_block = (uint64_t)HISTO_THREADS * HISTO_ITEMS_PER_THREAD;
  return (uint32_t)std::min<uint64_t>((items + per_block - 1) / per_block, HISTO_GRID);
}

int histo_capacity(const kmhisto::Layout& lay, const uint64_t* bins, uint64_t cap) {
  if (bins && cap < lay.n_bins)
    return fail(KM_E_CAPACITY, "%llu bins, room for %llu", (unsigned long long)lay.n_bins, (unsigned long long)cap);
  return KM_OK;
}

// The device side of one call: bins[n_bins] and, from the next 128-byte line on, the sets of four cells
// (histo_kernel.h), zeroed on `st`; the spans of its kernels.
struct HistoRun {
  static constexpr uint64_t CELL_WORDS = (uint64_t)HISTO_CELL_SETS * HISTO_CELL_STRIDE;
  DevBuf<unsigned long long> out;         // [cells_at + CELL_WORDS]
  KernelSpans spans;
  uint32_t n_bins = 0;
  uint64_t cells_at = 0;                  // n_bins rounded up to a line (hipMalloc aligns the buffer itself)
  int begin(uint32_t bins, hipStream_t st) {
    n_bins = bins;
    cells_at = ((uint64_t)bins + HISTO_CELL_STRIDE - 1) / HISTO_CELL_STRIDE * HISTO_CELL_STRIDE;
    spans.timed = true;
    KMCHK(out.alloc(cells_at + CELL_WORDS));
    HIPCHK(hipMemsetAsync(out, 0, (cells_at + CELL_WORDS) * 8, st));
    return KM_OK;
  }
  unsigned long long* bins() const { return out.p; }
  unsigned long long* cells() const { return out.p + cells_at; }
};

// n items in launches of at most HISTO_CHUNK (histo_kernel.h: the bound that keeps a block's LDS bins inside 32
// bits); launch(first item, items, grid).
template <typename Launch>
int histo_launch(HistoRun& run, hipStream_t st, uint64_t n, Launch launch) {
  KMCHK(run.spans.open(st));
  for (uint64_t at = 0; at < n; at += HISTO_CHUNK) {
    const uint64_t m = std::min(HISTO_CHUNK, n - at);
    launch(at, m, histo_grid(m));
  }
  HIPCHK(hipGetLastError());
  return run.spans.close(st);
}

// Waits for `st`; bins / stats as the caller asked for them (either may be null), `extra` = one more key that never
// was on the device (0: none).
int histo_collect(HistoRun& run, hipStream_t st, const HistoRule& r, const kmhisto::Layout& lay, uint64_t extra,
                  uint64_t* bins, km_histo_stats_t* stats) {
  std::vector<unsigned long long> host(run.cells_at + HistoRun::CELL_WORDS);
  HIPCHK(hipMemcpyAsync(host.data(), run.out, host.size() * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  KMCHK(run.spans.drain(&g_histo_kernel_ms));
  unsigned long long cells[HS_WORDS] = {0, 0, 0, 0};
  for (uint32_t s = 0; s < HISTO_CELL_SETS; ++s) {
    const unsigned long long* set = host.data() + run.cells_at + (uint64_t)s * HISTO_CELL_STRIDE;
    cells[HS_UNIQUE] += set[HS_UNIQUE];
    cells[HS_DISTINCT] += set[HS_DISTINCT];
    cells[HS_TOTAL] += set[HS_TOTAL];
    cells[HS_MAX] = std::max(cells[HS_MAX], set[HS_MAX]);
  }
  if (extra >= r.lo && extra <= r.hi) {
    ++host[kmhisto::bin(lay, extra)];
    cells[HS_UNIQUE] += extra == 1 ? 1 : 0;
    ++cells[HS_DISTINCT];
    cells[HS_TOTAL] += extra;
    cells[HS_MAX] = std::max<unsigned long long>(cells[HS_MAX], extra);
  }
  if (bins) memcpy(bins, host.data(), (uint64_t)run.n_bins * 8);
  if (stats) {
    memset(stats, 0, sizeof *stats);
    stats->unique = cells[HS_UNIQUE];
    stats->distinct = cells[HS_DISTINCT];
    stats->total = cells[HS_TOTAL];
    stats->max_count = cells[HS_MAX];
  }
  return KM_OK;
}

void histo_zeros(const kmhisto::Layout& lay, uint64_t* bins, km_histo_stats_t* stats) {
  if (bins) memset(bins, 0, lay.n_bins * 8);
  if (stats) memset(stats, 0, sizeof *stats);
}
}  // namespace

extern "C" int km_histo_layout(uint64_t low, uint64_t high, uint64_t increment, uint64_t* base, uint64_t* n_bins) {
  kmhisto::Layout lay;
  HistoRule r;
  KMCHK(histo_rule(low, high, increment, 1, 0xFFFFFFFFu, &lay, &r));
  if (base) *base = lay.base;
  if (n_bins) *n_bins = lay.n_bins;
  return KM_OK;
}

extern "C" int km_histo_kernel_ms(float* ms) {
  if (!ms) return fail(KM_E_ARG, "null argument");
  *ms = g_histo_kernel_ms;
  return KM_OK;
}

extern "C" int km_histo_text(uint64_t base, uint64_t increment, const uint64_t* bins, uint64_t n_bins, int full, char* out,
                             uint64_t cap, uint64_t* len) {
  if (!len || (n_bins && !bins)) return fail(KM_E_ARG, "null argument");
  if (increment == 0) return fail(KM_E_ARG, "increment 0");
  if (!kmhisto::write_histo(base, increment, bins, n_bins, full != 0, out, cap, len))
    return fail(KM_E_CAPACITY, "text of %llu bytes, room for %llu", (unsigned long long)*len, (unsigned long long)cap);
  return KM_OK;
}

extern "C" int km_histo_stats_text(const km_histo_stats_t* stats, char* out, uint64_t cap, uint64_t* len) {
  if (!stats || !len) return fail(KM_E_ARG, "null argument");
  if (!kmhisto::write_stats(stats->unique, stats->distinct, stats->total, stats->max_count, out, cap, len))
    return fail(KM_E_CAPACITY, "text of %llu bytes, room for %llu", (unsigned long long)*len, (unsigned long long)cap);
  return KM_OK;
}

extern "C" int km_counter_histo(km_counter_t* c, uint64_t low, uint64_t high, uint64_t increment, uint32_t lower_count,
                                uint32_t upper_count, uint64_t* bins, uint64_t cap, km_histo_stats_t* stats) {
  if (!c) return fail(KM_E_ARG, "null argument");
  kmhisto::Layout lay;
  HistoRule r;
  KMCHK(histo_rule(low, high, increment, lower_count, upper_count, &lay, &r));
  KMCHK(histo_capacity(lay, bins, cap));
  if (c->fq_error != FQ_NO_ERROR) return counter_format_failed(c);
  KMCHK(counter_sketch_settled(c));
  KMCHK(counter_holds_counts(c, "km_counter_histo"));
  if (!c->finished && c->feed == FEED_SET)              // (setops_host.h) the live table holds keys that do not survive
    return fail(KM_E_STATE, "the counter holds the inputs of a set operation: km_counter_finish comes before its histogram");
  r.rounds = histo_rounds();
  g_histo_kernel_ms = 0.f;
  HIPCHK(hipSetDevice(c->device));
  HistoRun run;
  if (c->finished) {                                    // the kept records; T^32 of a k = 32 table is among them
    if (c->n_out == 0) { histo_zeros(lay, bins, stats); return KM_OK; }
    KMCHK(run.begin(r.n_bins, c->st));
    const uint32_t* counts = c->out_counts.p;
    const uint64_t n = c->n_out, quads = n / 4;
    // (whole quads per launch; the last launch takes the tail, and a launch of the tail alone when n < 4)
    KMCHK(histo_launch(run, c->st, std::max<uint64_t>(quads, 1), [&](uint64_t at, uint64_t m, uint32_t grid) {
      const uint64_t upto = at + m >= quads ? n : (at + m) * 4;
      hipLaunchKernelGGL(k_histo_counts, dim3(grid), dim3(HISTO_THREADS), 0, c->st, counts + at * 4, upto - at * 4, r,
                         run.bins(), run.cells());
    }));
    return histo_collect(run, c->st, r, lay, 0, bins, stats);
  }
  KMCHK(counter_flush(c));
  unsigned long long m[CM_WORDS];
  KMCHK(counter_read_meta(c, m));
  KMCHK(run.begin(r.n_bins, c->st));
  const CountSlot* tab = c->table.p;
  KMCHK(histo_launch(run, c->st, c->slots, [&](uint64_t at, uint64_t n, uint32_t grid) {
    hipLaunchKernelGGL(k_histo_table, dim3(grid), dim3(HISTO_THREADS), 0, c->st, tab + at, n, r, run.bins(), run.cells());
  }));
  // T^32 of a non-canonical k = 32 table lives in a cell of its own (count_kernel.h), clamped as finish clamps it
  return histo_collect(run, c->st, r, lay, std::min<unsigned long long>(m[CM_ALLT], 0xFFFFFFFFull), bins, stats);
}

extern "C" int km_jf_histo(int device, const char* path, uint64_t low, uint64_t high, uint64_t increment,
                           uint32_t lower_count, uint32_t upper_count, uint64_t* bins, uint64_t cap,
                           km_histo_stats_t* stats, int32_t* k, uint64_t* n_records, void* stream) {
  if (!path) return fail(KM_E_ARG, "null argument");
  if (device < 0) return fail(KM_E_ARG, "device %d", device);
  kmhisto::Layout lay;
  HistoRule r;
  KMCHK(histo_rule(low, high, increment, lower_count, upper_count, &lay, &r));
  RecordFile file;
  KMCHK(file.open(path));
  KMCHK(histo_capacity(lay, bins, cap));
  const uint64_t n = file.lay.n_records, rec = file.rec;
  if (k) *k = file.lay.k;
  if (n_records) *n_records = n;
  r.rounds = histo_rounds();
  g_histo_kernel_ms = 0.f;
  if (n == 0) { histo_zeros(lay, bins, stats); return KM_OK; }
  const uint32_t kb = file.lay.key_bytes, cb = file.lay.counter_bytes;
  Staging s;
  // (a piece is ONE launch: at most HISTO_CHUNK records, the bound of histo_kernel.h on the items of a launch)
  const uint64_t per = std::min(kmpiece::per_piece(s.bytes, rec), HISTO_CHUNK);
  if (per == 0) return fail(KM_E_ARG, "records of %llu bytes do not fit a staging buffer", (unsigned long long)rec);
  CallStream st;                                        // (declared before what runs on the stream: released after it)
  KMCHK(st.get(device, stream));
  struct Drain {                                        // no early return leaves a copy out of a freed buffer in flight
    hipStream_t st;
    ~Drain() { (void)hipStreamSynchronize(st); }
  };
  DevBuf<uint8_t> d_raw;
  HistoRun run;
  KMCHK(s.alloc(0));
  KMCHK(d_raw.alloc(s.bytes));
  Drain drain{st};
  KMCHK(run.begin(r.n_bins, st));
  const uint64_t pieces = kmpiece::n_pieces(n, per);
  for (uint64_t i = 0; i < pieces; ++i) {
    const kmpiece::Piece p = kmpiece::piece(n, per, rec, i);
    KMCHK(s.claim());                                   // the copy out of this buffer, two pieces ago, is done
    KMCHK(file.read(p, s.mine));
    KMCHK(s.ship(d_raw, p.bytes, st));
    const uint64_t items = (kb == 8 && cb == 4) ? std::max<uint64_t>(p.records / 4, 1) : p.records;
    KMCHK(run.spans.open(st));
    hipLaunchKernelGGL(k_histo_records, dim3(histo_grid(items)), dim3(HISTO_THREADS), 0, st, d_raw.p, p.records, kb, cb, r,
                       run.bins(), run.cells());
    HIPCHK(hipGetLastError());
    KMCHK(run.spans.close(st));
  }
  return histo_collect(run, st, r, lay, 0, bins, stats);
}
