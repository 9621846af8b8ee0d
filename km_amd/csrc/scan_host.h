// scan_host.h — kmjf_cov_seqs, kmjf_scan_text, km_scan_kernel_ms (host part of kmgpu.hip; device side: scan_kernel.h;
// the window rule and the pieces: scan_rule.h)
// ------------------------------------------------------------------ scan: the k-mers of sequences, cut on the device
// The text of a call goes to the device piece by piece through a Staging of the call's own; the offsets go once, whole.
// A piece owns the starts [first, first + n_starts) and stages the k - 1 bytes behind them as well (kmscan::piece), so
// every window is complete in the piece that owns its start.  Statistics: the cells of all sequences stay in HBM for
// the whole call and come back in one copy.  Text: a piece's starts are the records of one DumpPipe piece.
namespace {
thread_local float g_scan_kernel_ms = 0.f;

// What both calls check alike, in this order.  *total: the bytes of all sequences.
int scan_check(const kmjf* h, const uint8_t* text, const uint64_t* seq_off, uint64_t n_seqs, uint64_t* total) {
  if (!h->d_slots) return fail(KM_E_STATE, "table not uploaded");
  *total = 0;
  if (n_seqs == 0) return KM_OK;
  if (!seq_off) return fail(KM_E_ARG, "null argument");
  if (n_seqs > kmscan::MAX_SEQS)
    return fail(KM_E_ARG, "%llu sequences: a call takes at most %llu", (unsigned long long)n_seqs,
                (unsigned long long)kmscan::MAX_SEQS);
  for (uint64_t q = 0; q < n_seqs; ++q)
    if (seq_off[q + 1] < seq_off[q])
      return fail(KM_E_ARG, "seq_off[%llu] = %llu is below seq_off[%llu] = %llu: the offsets must ascend",
                  (unsigned long long)(q + 1), (unsigned long long)seq_off[q + 1], (unsigned long long)q,
                  (unsigned long long)seq_off[q]);
  *total = seq_off[n_seqs] - seq_off[0];
  if (*total && !text) return fail(KM_E_ARG, "null argument");
  return KM_OK;
}

// The device side both calls share: the staged piece, the offsets, and the timing of the scan kernels.
struct ScanRun {
  Staging in;
  DevBuf<uint8_t> d_text;
  DevBuf<uint64_t> d_off;
  KernelSpans spans;
  const uint8_t* text = nullptr;
  const uint64_t* off = nullptr;
  uint64_t n_seqs = 0;
  int k = 0;
  // the buffers; nothing is enqueued
  int begin(const uint8_t* text_, const uint64_t* seq_off, uint64_t n, int k_) {
    text = text_;
    off = seq_off;
    n_seqs = n;
    k = k_;
    spans.timed = true;
    if (in.bytes < (uint64_t)k) return fail(KM_E_ARG, "staging buffers of %llu bytes hold no window of k = %d",
                                            (unsigned long long)in.bytes, k);
    KMCHK(in.alloc(0));
    KMCHK(d_text.alloc(in.bytes + kmscan::PAD));
    KMCHK(d_off.alloc(n + 1));
    return KM_OK;
  }
  int send_offsets(hipStream_t st) {
    HIPCHK(hipMemcpyAsync(d_off, off, (n_seqs + 1) * 8, hipMemcpyHostToDevice, st));
    return KM_OK;
  }
  // piece p to the device on st -> what the kernel is launched with
  int ship(const kmscan::Piece& p, hipStream_t st, ScanPiece* out) {
    KMCHK(in.claim());
    memcpy(in.mine, text + p.first, p.n_bytes);
    KMCHK(in.ship(d_text, p.n_bytes, st));
    out->text = d_text;
    out->first = p.first;
    out->n_starts = p.n_starts;
    out->end_all = off[n_seqs];
    out->off = d_off;
    // the sequences of the piece's first and last start: the last q with off[q] <= position
    out->q_lo = (uint64_t)(std::upper_bound(off, off + n_seqs, p.first) - off) - 1;
    out->q_hi = (uint64_t)(std::upper_bound(off, off + n_seqs, p.first + p.n_starts - 1) - off) - 1;
    return KM_OK;
  }
  static dim3 grid(const kmscan::Piece& p) {
    const uint64_t lanes = (p.n_starts + kmscan::RUN - 1) / kmscan::RUN;
    return dim3((uint32_t)((lanes + kmscan::THREADS - 1) / kmscan::THREADS));
  }
};
}  // namespace

extern "C" int km_scan_kernel_ms(float* ms) {
  if (!ms) return fail(KM_E_ARG, "null argument");
  *ms = g_scan_kernel_ms;
  return KM_OK;
}

extern "C" int kmjf_cov_seqs(kmjf_t* h, const uint8_t* text, const uint64_t* seq_off, uint64_t n_seqs, km_cov_t* out,
                             void* stream) {
  if (!h || (n_seqs && !out)) return fail(KM_E_ARG, "null argument");
  uint64_t total = 0;
  KMCHK(scan_check(h, text, seq_off, n_seqs, &total));
  g_scan_kernel_ms = 0.f;
  if (total == 0) return KM_OK;
  CallStream st;                                        // (declared before what runs on it: released after it)
  KMCHK(st.get(h->device, stream));
  ScanRun run;
  DevBuf<km_cov_t> cells;
  StreamDrain drain{st};
  KMCHK(run.begin(text, seq_off, n_seqs, h->k));
  KMCHK(cells.alloc(n_seqs));
  KMCHK(run.send_offsets(st));
  hipLaunchKernelGGL(k_scan_init, dim3(grid_for(n_seqs, 256)), dim3(256), 0, st, cells.p, n_seqs);
  HIPCHK(hipGetLastError());
  const TableView tv = view_of(h);
  const uint64_t begin = seq_off[0], end = seq_off[n_seqs];
  const uint64_t per = kmscan::starts_per_piece(run.in.bytes, h->k);
  const uint64_t pieces = kmscan::n_pieces(begin, end, per);
  for (uint64_t i = 0; i < pieces; ++i) {
    const kmscan::Piece p = kmscan::piece(begin, end, per, h->k, i);
    ScanPiece sp;
    KMCHK(run.ship(p, st, &sp));
    KMCHK(run.spans.open(st));
    hipLaunchKernelGGL(k_scan_stats, ScanRun::grid(p), dim3(kmscan::THREADS), 0, st, tv, sp, cells.p);
    HIPCHK(hipGetLastError());
    KMCHK(run.spans.close(st));
    if ((i & 63) == 63) {                               // a call of many pieces holds a bounded number of event pairs
      HIPCHK(hipStreamSynchronize(st));
      KMCHK(run.spans.drain(&g_scan_kernel_ms));
    }
  }
  HIPCHK(hipMemcpyAsync(out, cells.p, n_seqs * sizeof(km_cov_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return run.spans.drain(&g_scan_kernel_ms);
}

extern "C" int kmjf_scan_text(kmjf_t* h, const uint8_t* text, const uint64_t* seq_off, uint64_t n_seqs, int out_fd,
                              km_dump_stats_t* stats, void* stream) {
  if (!h) return fail(KM_E_ARG, "null argument");
  KMCHK(dump_check_fd(out_fd));
  uint64_t total = 0;
  KMCHK(scan_check(h, text, seq_off, n_seqs, &total));
  g_scan_kernel_ms = 0.f;
  g_dump_kernel_ms = 0.f;
  if (stats) memset(stats, 0, sizeof *stats);
  if (total == 0) return KM_OK;
  Staging out;
  CallStream st, cs;
  KMCHK(st.get(h->device, stream));
  KMCHK(cs.get(h->device, nullptr));
  ScanRun run;
  DevBuf<uint64_t> d_keys;
  DevBuf<uint32_t> d_counts, d_lines;
  KMCHK(run.begin(text, seq_off, n_seqs, h->k));
  const uint64_t per = std::min(kmscan::starts_per_piece(run.in.bytes, h->k), dump_text_records(out.bytes, h->k));
  KMCHK(out.alloc(0));
  KMCHK(d_keys.alloc(per));
  KMCHK(d_counts.alloc(per));
  KMCHK(d_lines.alloc((per + kmscan::RUN - 1) / kmscan::RUN));
  DumpPipe pipe;                                        // (after the buffers: its destructor drains both streams first)
  pipe.open(&out, st, cs, out_fd);
  KMCHK(pipe.run.begin(DumpRule{h->k, KM_DUMP_COLUMN, 0u, 0xFFFFFFFFu}, out.bytes, 2));   // no filter: a 0 is printed
  KMCHK(run.send_offsets(st));
  const TableView tv = view_of(h);
  const uint64_t begin = seq_off[0], end = seq_off[n_seqs];
  const uint64_t pieces = kmscan::n_pieces(begin, end, per);
  for (uint64_t i = 0; i < pieces; ++i) {
    const kmscan::Piece p = kmscan::piece(begin, end, per, h->k, i);
    ScanPiece sp;
    KMCHK(run.ship(p, st, &sp));
    KMCHK(run.spans.open(st));
    hipLaunchKernelGGL(k_scan_text, ScanRun::grid(p), dim3(kmscan::THREADS), 0, st, tv, sp, d_keys.p, d_counts.p,
                       d_lines.p);
    HIPCHK(hipGetLastError());
    KMCHK(run.spans.close(st));
    KMCHK(pipe.piece(DumpScan{d_keys.p, d_counts.p, d_lines.p}, p.n_starts));   // (waits for the piece: the three
    KMCHK(run.spans.drain(&g_scan_kernel_ms));                                  // arrays are free for the next one)
  }
  KMCHK(pipe.finish(stats));
  if (stats) {                                          // records_in: the windows of the sequences, not the starts
    uint64_t windows = 0;
    for (uint64_t q = 0; q < n_seqs; ++q) windows += kmscan::n_windows(seq_off[q + 1] - seq_off[q], h->k);
    stats->records_in = windows;
  }
  return KM_OK;
}
