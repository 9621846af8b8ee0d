// dump_host.h — km_dump_text, km_jf_dump, km_counter_dump, kmjf_query_text, km_dump_kernel_ms (host part of kmgpu.hip;
// device side: dump_kernel.h; the text rule: dump_text.h)
// ------------------------------------------------------------------ records as text: dump and query
// Records that are in HBM or on their way there leave as text: one piece of records is formatted on the device
// (sizes, scan, write: dump_kernel.h) into one of two text buffers, its byte total is read back, and exactly that
// many bytes cross to a pinned buffer of a Staging on a copy stream of the call's own while the launch stream takes
// the next piece; the host only calls write().  A piece holds at most bytes / (k + 13) records (the worst line), so
// its text always fits one staging buffer, and at most DUMP_MAX_RECORDS (one scan chunk).
#include <fcntl.h>

namespace {
thread_local float g_dump_kernel_ms = 0.f;

int dump_check_format(int format) {
  if (!kmdump::format_known(format)) return fail(KM_E_ARG, "format %d is none of KM_DUMP_FASTA / _COLUMN / _TAB", format);
  return KM_OK;
}

int dump_check_fd(int fd) {
  if (fcntl(fd, F_GETFL) == -1) return fail(KM_E_IO, "output descriptor %d: %s", fd, strerror(errno));
  return KM_OK;
}

// n bytes to fd in as many writes as that takes; 0 or the errno of the write that failed
int dump_write_all(int fd, const unsigned char* p, uint64_t n) {
  while (n) {
    const ssize_t w = write(fd, p, n);
    if (w < 0 && errno == EINTR) continue;
    if (w < 0) return errno;
    p += w;
    n -= (uint64_t)w;
  }
  return 0;
}

// records per piece whose text fits `text_bytes`, within one scan chunk
uint64_t dump_text_records(uint64_t text_bytes, int k) {
  return std::min<uint64_t>(text_bytes / kmdump::worst_line(k), DUMP_MAX_RECORDS);
}

// The device side of one call: the two tile tables of a piece (bytes, scanned in place; kept records), their chunk
// sums, two text buffers, and per text buffer the two totals on the host and the event "formatted, totals there".
struct DumpRun {
  DevBuf<uint32_t> tab;                   // [2 * SCAN_CHUNK] tile tables, [2] sums
  DevBuf<uint8_t> text[2];
  Pinned totals;                          // uint32 [2 buffers][bytes, kept]
  Event done[2];
  KernelSpans spans;
  DumpRule rule;
  uint64_t text_bytes = 0;
  int begin(const DumpRule& r, uint64_t bytes_per_text, int n_text) {
    rule = r;
    text_bytes = bytes_per_text;
    spans.timed = true;
    KMCHK(tab.alloc(2ull * SCAN_CHUNK + 2));
    for (int i = 0; i < n_text; ++i) {
      KMCHK(text[i].alloc(bytes_per_text + 16));
      HIPCHK(hipEventCreateWithFlags(&done[i].h, hipEventDisableTiming));
    }
    return pinned_alloc(&totals, 16, "pinned totals");
  }
  uint32_t* sums() const { return tab.p + 2ull * SCAN_CHUNK; }
  const volatile uint32_t* total_of(int buf) const { return reinterpret_cast<const uint32_t*>(totals.h) + 2 * buf; }

  // The n records of `src` (on the device, ready in stream order) as text into text[buf], on st; with write == false
  // only the totals are computed.  done[buf] follows.
  template <typename Src>
  int format(const Src& src, uint64_t n, int buf, bool write, hipStream_t st) {
    if (n == 0 || n > DUMP_MAX_RECORDS || n * kmdump::worst_line(rule.k) > text_bytes)
      return fail(KM_E_ARG, "a piece of %llu records does not fit %llu text bytes", (unsigned long long)n,
                  (unsigned long long)text_bytes);
    const uint32_t tiles = (uint32_t)((n + DUMP_TILE - 1) / DUMP_TILE);      // tiles + 1 <= SCAN_CHUNK
    KMCHK(spans.open(st));
    HIPCHK(hipMemsetAsync(tab, 0, 2ull * SCAN_CHUNK * 4, st));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dump_sizes<Src>), dim3(tiles), dim3(DUMP_THREADS), 0, st, src, (uint32_t)n, rule,
                       tab.p, tab.p + SCAN_CHUNK);
    // both tables' totals at once: sums[0] = bytes, sums[1] = kept records; they leave before k_scan_sums turns
    // sums[0] into the (only) chunk's offset, 0
    hipLaunchKernelGGL(k_scan_reduce, dim3(2), dim3(SCAN_THREADS), 0, st, tab.p, sums());
    HIPCHK(hipMemcpyAsync(totals.h + 8 * buf, sums(), 8, hipMemcpyDeviceToHost, st));
    if (write) {
      hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(SCAN_THREADS), 0, st, sums(), 1u);
      hipLaunchKernelGGL(k_scan_apply, dim3(1), dim3(SCAN_THREADS), 0, st, tab.p, sums());
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dump_write<Src>), dim3(tiles), dim3(DUMP_THREADS), 0, st, src, (uint32_t)n, rule,
                         tab.p, text[buf].p);
    }
    HIPCHK(hipGetLastError());
    KMCHK(spans.close(st));
    HIPCHK(hipEventRecord(done[buf], st));
    return KM_OK;
  }
  // Waits for format(.., buf, ..), the last piece enqueued: the bytes and the kept records of that piece.  Every
  // span recorded so far is complete then and is drained at once, so a call of many pieces holds one event pair.
  int wait(int buf, uint64_t* bytes, uint64_t* kept) {
    HIPCHK(hipEventSynchronize(done[buf]));
    float so_far;
    KMCHK(spans.drain(&so_far));
    *bytes = total_of(buf)[0];
    *kept = total_of(buf)[1];
    return KM_OK;
  }
};

// The last leg of every call that writes device-made text to a descriptor (here and in select_host.h): per pinned
// buffer of a Staging the bytes of the copy in flight into it; put() waits for that copy and writes them, short writes
// and EINTR handled in dump_write_all, any other failure (EPIPE: the reader went away) is KM_E_IO.  The two buffers
// take turns piece by piece: begin() hands out this piece's, put_before() writes the piece before it while this one is
// made on the device, fetch() starts this piece's copy, and flush() ends a call.
struct TextDrain {
  Staging* out = nullptr;
  hipStream_t cs = nullptr;               // the copy stream
  int fd = -1;
  int turn = 0;                           // the buffer of the next piece
  uint64_t pending[2] = {0, 0};           // bytes of the copy in flight into out->pin[i]
  bool close_line[2] = {false, false};    // the text in out->pin[i] gets a newline behind it unless it ends in one
  uint64_t closed = 0;                    // (the buffers have a byte of padding for it) ... and how often that happened
  int begin() {
    turn ^= 1;
    return turn ^ 1;
  }
  // bytes of d_src (ready: the host has waited for what wrote them) on their way into out->pin[buf]
  int fetch(int buf, const void* d_src, uint64_t bytes) {
    if (bytes) KMCHK(out->fetch(buf, d_src, bytes, cs));
    pending[buf] = bytes;
    return KM_OK;
  }
  int put(int buf) {                      // the text copied into out->pin[buf] goes to fd
    if (!pending[buf]) return KM_OK;
    unsigned char* got = nullptr;
    KMCHK(out->wait(buf, &got));
    uint64_t n = pending[buf];
    pending[buf] = 0;
    if (close_line[buf] && got[n - 1] != '\n') {
      got[n++] = '\n';
      ++closed;
    }
    close_line[buf] = false;
    if (const int e = dump_write_all(fd, got, n)) return fail(KM_E_IO, "writing the text failed: %s", strerror(e));
    return KM_OK;
  }
  int put_before(int buf) { return put(buf ^ 1); }
  // What is still on its way is written, the older of the two first; the newlines that closed a last line count as
  // bytes of the caller's.
  int flush(uint64_t* bytes_out) {
    int rc = put(turn);
    if (rc == KM_OK) rc = put(turn ^ 1);
    *bytes_out += closed;
    closed = 0;
    return rc;
  }
};

// The way out of the calls that write records as text: piece after piece, formatted on `st` into the text buffer
// whose turn it is, copied on `cs` into the pinned buffer of the same number, written to `fd` one piece later.
struct DumpPipe : TextDrain {
  DumpRun run;
  hipStream_t st = nullptr;
  km_dump_stats_t stats;
  StreamDrain sync;                       // (last: both streams are waited for before the tables and texts of `run` go)
  DumpPipe() { memset(&stats, 0, sizeof stats); }
  void open(Staging* text_out, hipStream_t launch, hipStream_t copy, int out_fd) {
    out = text_out;
    st = sync.st = launch;
    cs = sync.cs = copy;
    fd = out_fd;
  }
  template <typename Src>
  int piece(const Src& src, uint64_t n) {
    const int buf = begin();
    KMCHK(run.format(src, n, buf, true, st));
    KMCHK(put_before(buf));               // while this one is formatted
    uint64_t bytes = 0, kept = 0;
    KMCHK(run.wait(buf, &bytes, &kept));
    stats.records_in += n;
    stats.records_out += kept;
    stats.bytes_out += bytes;
    ++stats.pieces;
    return fetch(buf, run.text[buf].p, bytes);
  }
  int finish(km_dump_stats_t* to) {
    KMCHK(flush(&stats.bytes_out));       // (adds nothing: no piece of records leaves a line open)
    HIPCHK(hipStreamSynchronize(st));
    KMCHK(run.spans.drain(&g_dump_kernel_ms));
    if (to) *to = stats;
    return KM_OK;
  }
};
}  // namespace

extern "C" int km_dump_kernel_ms(float* ms) {
  if (!ms) return fail(KM_E_ARG, "null argument");
  *ms = g_dump_kernel_ms;
  return KM_OK;
}

extern "C" int km_dump_text(int device, const uint64_t* keys, const uint32_t* counts, uint64_t n, int k, int format,
                            uint32_t lower, uint32_t upper, char* out, uint64_t cap, uint64_t* len, void* stream) {
  if (!len || (n && (!keys || !counts)) || (cap && !out)) return fail(KM_E_ARG, "null argument");
  if (device < 0) return fail(KM_E_ARG, "device %d", device);
  if (k < 2 || k > 32) return fail(KM_E_ARG, "k=%d outside 2..32", k);
  KMCHK(dump_check_format(format));
  *len = 0;
  g_dump_kernel_ms = 0.f;
  if (n == 0) return KM_OK;
  const DumpRule rule{k, format, lower, upper};
  Staging sized;                                        // (only its size: KM_COUNT_STAGE_BYTES cuts the pieces here too)
  const uint64_t per = dump_text_records(sized.bytes, k);
  CallStream st;
  KMCHK(st.get(device, stream));
  DevBuf<uint64_t> d_keys;
  DevBuf<uint32_t> d_counts;
  DumpRun run;
  KMCHK(d_keys.alloc(n));
  KMCHK(d_counts.alloc(n));
  KMCHK(run.begin(rule, sized.bytes, 1));
  StreamDrain drain{st};
  HIPCHK(hipMemcpyAsync(d_keys, keys, n * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_counts, counts, n * 4, hipMemcpyHostToDevice, st));
  // first the length of the whole text, so that a buffer too small is left untouched; then the text
  for (int pass = 0; pass < 2; ++pass) {
    uint64_t at_byte = 0;
    for (uint64_t first = 0; first < n; first += per) {
      const uint64_t m = std::min(per, n - first);
      uint64_t bytes = 0, kept = 0;
      KMCHK(run.format(DumpArrays{d_keys.p + first, d_counts.p + first}, m, 0, pass == 1, st));
      KMCHK(run.wait(0, &bytes, &kept));
      if (pass == 1 && bytes) {
        HIPCHK(hipMemcpyAsync(out + at_byte, run.text[0].p, bytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
      }
      at_byte += bytes;
    }
    if (pass == 0) {
      *len = at_byte;
      if (!out || at_byte > cap) {                      // the length alone, or a buffer too small
        HIPCHK(hipStreamSynchronize(st));
        KMCHK(run.spans.drain(&g_dump_kernel_ms));
        if (!out) return KM_OK;
        return fail(KM_E_CAPACITY, "text of %llu bytes, room for %llu", (unsigned long long)at_byte, (unsigned long long)cap);
      }
    }
  }
  HIPCHK(hipStreamSynchronize(st));
  return run.spans.drain(&g_dump_kernel_ms);
}

extern "C" int km_jf_dump(int device, const char* path, int out_fd, int format, uint32_t lower, uint32_t upper,
                          km_dump_stats_t* stats, void* stream) {
  if (!path) return fail(KM_E_ARG, "null argument");
  if (device < 0) return fail(KM_E_ARG, "device %d", device);
  KMCHK(dump_check_format(format));
  KMCHK(dump_check_fd(out_fd));
  RecordFile file;
  KMCHK(file.open(path));
  const uint64_t n = file.lay.n_records, rec = file.rec;
  const int k = file.lay.k;
  g_dump_kernel_ms = 0.f;
  if (stats) memset(stats, 0, sizeof *stats);
  if (n == 0) return KM_OK;
  const uint32_t kb = file.lay.key_bytes, cb = file.lay.counter_bytes;
  if (kb < 1 || kb > 8 || cb < 1 || cb > 4)
    return fail(KM_E_FORMAT, "%s: records of %u key bytes and %u count bytes", path, kb, cb);
  Staging in, out;
  const uint64_t per = std::min(kmpiece::per_piece(in.bytes, rec), dump_text_records(out.bytes, k));
  if (per == 0) return fail(KM_E_ARG, "records of %llu bytes do not fit a staging buffer", (unsigned long long)rec);
  CallStream st, cs;                                    // (declared before what runs on them: released after it)
  KMCHK(st.get(device, stream));
  KMCHK(cs.get(device, nullptr));
  DevBuf<uint8_t> d_raw;
  KMCHK(in.alloc(0));
  KMCHK(out.alloc(0));
  KMCHK(d_raw.alloc(in.bytes));
  DumpPipe pipe;                                        // (after the buffers: its destructor drains both streams first)
  pipe.open(&out, st, cs, out_fd);
  KMCHK(pipe.run.begin(DumpRule{k, format, lower, upper}, out.bytes, 2));
  const uint64_t pieces = kmpiece::n_pieces(n, per);
  for (uint64_t i = 0; i < pieces; ++i) {
    const kmpiece::Piece p = kmpiece::piece(n, per, rec, i);
    KMCHK(in.claim());                                  // the copy out of this buffer, two pieces ago, is done
    KMCHK(file.read(p, in.mine));
    KMCHK(in.ship(d_raw, p.bytes, st));
    KMCHK(pipe.piece(DumpRaw{d_raw.p, kb, cb}, p.records));
  }
  return pipe.finish(stats);
}

extern "C" int km_counter_dump(km_counter_t* c, int out_fd, int format, uint32_t lower, uint32_t upper,
                               km_dump_stats_t* stats) {
  if (!c) return fail(KM_E_ARG, "null argument");
  KMCHK(dump_check_format(format));
  KMCHK(dump_check_fd(out_fd));
  KMCHK(counter_holds_counts(c, "km_counter_dump"));
  if (!c->finished) return fail(KM_E_STATE, "km_counter_finish comes first");
  g_dump_kernel_ms = 0.f;
  if (stats) memset(stats, 0, sizeof *stats);
  const uint64_t n = c->n_out;
  if (n == 0) return KM_OK;
  const uint64_t per = dump_text_records(c->stg.bytes, c->k);
  CallStream cs;
  KMCHK(cs.get(c->device, nullptr));
  DumpPipe pipe;
  pipe.open(&c->stg, c->st, cs, out_fd);                // (idle once the counter has finished, as for write_jf)
  KMCHK(pipe.run.begin(DumpRule{c->k, format, lower, upper}, c->stg.bytes, 2));
  for (uint64_t first = 0; first < n; first += per)     // T^32 of a non-canonical k = 32 table is among the records
    KMCHK(pipe.piece(DumpArrays{c->out_keys.p + first, c->out_counts.p + first}, std::min(per, n - first)));
  return pipe.finish(stats);
}

extern "C" int kmjf_query_text(kmjf_t* h, const uint64_t* kmers, uint64_t n, int out_fd, km_dump_stats_t* stats,
                               void* stream) {
  if (!h || (n && !kmers)) return fail(KM_E_ARG, "null argument");
  KMCHK(dump_check_fd(out_fd));
  if (!h->d_slots) return fail(KM_E_STATE, "table not uploaded");
  g_dump_kernel_ms = 0.f;
  if (stats) memset(stats, 0, sizeof *stats);
  if (n == 0) return KM_OK;
  Staging in, out;
  const uint64_t per = std::min(in.bytes / 8, dump_text_records(out.bytes, h->k));
  CallStream st, cs;
  KMCHK(st.get(h->device, stream));
  KMCHK(cs.get(h->device, nullptr));
  DevBuf<uint64_t> d_kmers;
  DevBuf<uint32_t> d_counts;
  KMCHK(in.alloc(0));
  KMCHK(out.alloc(0));
  KMCHK(d_kmers.alloc(per));
  KMCHK(d_counts.alloc(per));
  DumpPipe pipe;
  pipe.open(&out, st, cs, out_fd);
  KMCHK(pipe.run.begin(DumpRule{h->k, KM_DUMP_COLUMN, 0u, 0xFFFFFFFFu}, out.bytes, 2));   // no filter: a 0 is printed
  for (uint64_t first = 0; first < n; first += per) {
    const uint64_t m = std::min(per, n - first);
    KMCHK(in.claim());
    memcpy(in.mine, kmers + first, m * 8);
    KMCHK(in.ship(d_kmers, m * 8, st));
    KMCHK(kmjf_query_batch_dev(h, d_kmers, m, d_counts, st));
    KMCHK(pipe.piece(DumpArrays{d_kmers.p, d_counts.p}, m));
  }
  return pipe.finish(stats);
}
