// select_host.h — km_select_*, kmjf_fastq_hits, km_select_kernel_ms (host part of kmgpu.hip; device side:
// select_kernel.h after fastq_kernel.h's front half; the rule: select_rule.h)
// ------------------------------------------------------------------ select: the FASTQ records that hit a table
// Raw FASTQ text goes to the device in pieces of whole records through a Staging, as for km_counter_add_fastq, and
// through the same front half (fastq_front: line table, mask, validation).  Then per piece: the hits per record, the
// kept records' lengths and their scan, and the gather into one of two dense output buffers.  The piece's totals and
// the format-error cell come back in one small copy; exactly `total` bytes cross to a pinned buffer on the copy stream
// while the launch stream takes the next piece, and dump_host.h's TextDrain writes them a piece later.
namespace {
static_assert(COUNT_PAD == kmscan::PAD && COUNT_PAD >= kmsel::SRC_PAD, "the raw and the masked piece are padded for both readers");
thread_local float g_select_ms[4] = {0.f, 0.f, 0.f, 0.f};

// Device side of one piece, shared by the selector and kmjf_fastq_hits.
struct SelDev {
  FastqDev fq;
  DevBuf<uint8_t> d_text;                 // the raw piece (one: copy and kernels are stream-ordered)
  DevBuf<uint32_t> hits, len, sums;       // per record; len is scanned in place
  DevBuf<unsigned long long> meta;        // [0] the format-error cell (sticky), [1..2] the piece's SEL_* cells
  Pinned back;                            // 24 bytes of meta per output buffer
  KernelSpans spans[4];                   // KM_SELECT_TIME: front half, clear + hits, sizes + scan, gather
  uint64_t stage = 0;
  uint32_t n_tiles = 0;
  uint32_t* cells() const { return reinterpret_cast<uint32_t*>(meta.p + 1); }
  int alloc(uint64_t stage_bytes, bool gather, hipStream_t st) {
    stage = stage_bytes;
    KMCHK(fastq_dev_alloc(&fq, stage));
    KMCHK(d_text.alloc(stage + COUNT_PAD));
    KMCHK(hits.alloc(kmsel::hit_cells(stage)));
    KMCHK(meta.alloc(3));
    if (gather) {
      const uint64_t chunks = len_chunks(stage);
      KMCHK(len.alloc(chunks * SCAN_CHUNK));
      KMCHK(sums.alloc(chunks));
    }
    KMCHK(pinned_alloc(&back, 64, "pinned totals"));
    if (const char* e = getenv("KM_SELECT_TIME"))
      for (KernelSpans& s : spans) s.timed = atoi(e) != 0;
    HIPCHK(hipMemsetAsync(meta.p, 0xFF, 8, st));            // FQ_NO_ERROR
    HIPCHK(hipMemsetAsync(meta.p + 1, 0, 16, st));
    return KM_OK;
  }
  // scan chunks of the lengths of a piece of n bytes: its records and the entry behind them
  static uint64_t len_chunks(uint64_t n) { return kmsel::len_chunks(n, SCAN_CHUNK); }
  // d_text[0 .. n) is there in stream order -> hits[r] of its records, cells()[SEL_RECORDS]
  int front_hits(const TableView& tv, uint64_t n, uint64_t base, uint32_t min_qual, hipStream_t st) {
    KMCHK(spans[0].open(st));
    KMCHK(fastq_front(fq, d_text.p, n, base, min_qual, meta.p, st, &n_tiles));
    KMCHK(spans[0].close(st));
    KMCHK(spans[1].open(st));
    hipLaunchKernelGGL(k_sel_clear, dim3(grid_for(n / 4 + 2, kmsel::THREADS)), dim3(kmsel::THREADS), 0, st, d_text.p, n,
                       fq.tiles.p, n_tiles, hits.p, cells());
    const uint64_t lanes = (n + kmscan::RUN - 1) / kmscan::RUN;
    hipLaunchKernelGGL(k_sel_hits, dim3((uint32_t)((lanes + kmscan::THREADS - 1) / kmscan::THREADS)), dim3(kmscan::THREADS),
                       0, st, tv, d_text.p, fq.masked.p, (uint32_t)n, fq.tiles.p, n_tiles, fq.line_start.p, hits.p);
    HIPCHK(hipGetLastError());
    return spans[1].close(st);
  }
  // ... -> the kept records of the piece end to end in d_out, cells()[SEL_BYTES], [SEL_KEPT]
  int gather(uint64_t n, uint32_t min_hits, int invert, uint8_t* d_out, hipStream_t st) {
    const uint32_t chunks = (uint32_t)len_chunks(n);
    const uint64_t words = (n + kmsel::WORD - 1) / kmsel::WORD;
    KMCHK(spans[2].open(st));
    hipLaunchKernelGGL(k_sel_sizes, dim3(chunks * (SCAN_CHUNK / kmsel::THREADS)), dim3(kmsel::THREADS), 0, st,
                       fq.line_start.p, (uint32_t)n, hits.p, min_hits, invert ? 1u : 0u, len.p, cells());
    scan_in_place(len.p, sums.p, chunks, st);
    HIPCHK(hipGetLastError());
    KMCHK(spans[2].close(st));
    KMCHK(spans[3].open(st));
    hipLaunchKernelGGL(k_sel_gather, dim3((uint32_t)((words + kmsel::THREADS - 1) / kmsel::THREADS)), dim3(kmsel::THREADS),
                       0, st, d_text.p, fq.line_start.p, len.p, cells(), d_out);
    HIPCHK(hipGetLastError());
    return spans[3].close(st);
  }
  // the error cell and the cells into back[buf], in stream order
  int read_back(int buf, hipStream_t st) {
    HIPCHK(hipMemcpyAsync(back.h + 32 * buf, meta.p, 24, hipMemcpyDeviceToHost, st));
    return KM_OK;
  }
  unsigned long long error_of(int buf) const { return *reinterpret_cast<const volatile unsigned long long*>(back.h + 32 * buf); }
  const volatile uint32_t* cells_of(int buf) const { return reinterpret_cast<const volatile uint32_t*>(back.h + 32 * buf + 8); }
  // (the stream has been waited for)
  int drain_spans() {
    for (int i = 0; i < 4; ++i) KMCHK(spans[i].drain(&g_select_ms[i]));
    return KM_OK;
  }
};

int select_format_failed(unsigned long long error) {
  return fail(KM_E_FORMAT, "%s at byte offset %llu", fastq_error_text((unsigned)(error & 0xFF)),
              (unsigned long long)(error >> 8));
}

int select_check_qual(int min_qual_char) {
  if (min_qual_char < 0 || min_qual_char > 255) return fail(KM_E_ARG, "min_qual_char %d outside 0..255", min_qual_char);
  return KM_OK;
}

// What km_select_create and km_select_pair_create check of their arguments, in this order.  The single selector is the
// rule "any" (0) over one descriptor.
int select_check_create(const kmjf* h, const void* out, uint32_t min_hits, int min_qual_char, int rule, const int* fds,
                        int n_fds) {
  if (!h || !out) return fail(KM_E_ARG, "null argument");
  if (min_hits == 0) return fail(KM_E_ARG, "min_hits must be at least 1");
  KMCHK(select_check_qual(min_qual_char));
  if (rule < 0 || rule >= (int)kmpair::RULE_COUNT) return fail(KM_E_ARG, "pair rule %d is none of any (0), both (1), sum (2)", rule);
  if (n_fds == 2 && fds[0] == fds[1]) return fail(KM_E_ARG, "the two mates need two descriptors, both are %d", fds[0]);
  if (!h->d_slots) return fail(KM_E_STATE, "table not uploaded");
  for (int i = 0; i < n_fds; ++i) KMCHK(dump_check_fd(fds[i]));
  return KM_OK;
}

// What km_select and km_select_pair share: the table and the numbers of the rule, the two streams with the events of
// the two output buffers, and the end of a call.  The owner declares it first (the streams are released last) and a
// StreamDrain last (both are waited for before any buffer goes).
struct SelCore {
  kmjf_t* h = nullptr;
  uint32_t min_hits = 1, min_qual = 0;
  int invert = 0;
  CallStream st, cs;                      // launch and copy
  Event done[2];                          // the piece gathered into output buffer i is done, its totals are there
  int dead = KM_OK;                       // the code a call failed with: every further call fails the same way
  std::string dead_msg;
  int open(kmjf_t* table, uint32_t hits, int inv, int min_qual_char, void* stream, StreamDrain* sync) {
    h = table;
    min_hits = hits;
    invert = inv ? 1 : 0;
    min_qual = (uint32_t)min_qual_char;
    KMCHK(st.get(h->device, stream));
    KMCHK(cs.get(h->device, nullptr));
    sync->st = st;
    sync->cs = cs;
    sync->device = h->device;
    for (Event& e : done) HIPCHK(hipEventCreateWithFlags(&e.h, hipEventDisableTiming));
    return KM_OK;
  }
  int alive() const { return dead == KM_OK ? KM_OK : fail(dead, "%s", dead_msg.c_str()); }
  // The end of every add_fastq: rc and msg are what the pieces came to, rc_flush what writing the text they kept came
  // to (the flush comes whatever rc is: what the pieces before a failure kept is written).  Whatever failed, nothing
  // stays in flight and the selector fails from now on: its offsets and the descriptor's content no longer match what
  // a caller who went on would assume.
  int end_call(int rc, std::string msg, int rc_flush) {
    if (rc == KM_OK && rc_flush != KM_OK) {
      rc = rc_flush;
      msg = g_last_error;
    }
    if (rc == KM_OK) return KM_OK;
    (void)hipStreamSynchronize(st);
    (void)hipStreamSynchronize(cs);
    dead = rc;
    dead_msg = msg;
    return fail(rc, "%s", msg.c_str());
  }
};
}  // namespace

struct km_select : SelCore {
  Staging in, out;
  SelDev dev;
  DevBuf<uint8_t> d_out[2];
  TextDrain drain;
  uint64_t offset = 0;                    // bytes consumed by the earlier calls of this stream
  km_select_stats_t stats;
  StreamDrain sync;
  km_select() { memset(&stats, 0, sizeof stats); }
  // One piece of whole records; ends: the stream ends with it.
  int piece(const char* text, uint64_t n, uint64_t base, bool ends) {
    const int buf = drain.begin();
    KMCHK(in.claim());
    memcpy(in.mine, text, n);
    KMCHK(in.ship(dev.d_text, n, st));
    KMCHK(dev.front_hits(view_of(h), n, base, min_qual, st));
    KMCHK(dev.gather(n, min_hits, invert, d_out[buf].p, st));
    KMCHK(dev.read_back(buf, st));
    HIPCHK(hipEventRecord(done[buf], st));
    KMCHK(drain.put_before(buf));         // while this one is scanned
    HIPCHK(hipEventSynchronize(done[buf]));
    KMCHK(dev.drain_spans());
    if (dev.error_of(buf) != FQ_NO_ERROR) return select_format_failed(dev.error_of(buf));
    const volatile uint32_t* c = dev.cells_of(buf);
    stats.records_in += c[SEL_RECORDS];
    stats.records_out += c[SEL_KEPT];
    stats.bytes_in += n;
    stats.bytes_out += c[SEL_BYTES];
    ++stats.pieces;
    drain.close_line[buf] = ends && text[n - 1] != '\n';
    return drain.fetch(buf, d_out[buf].p, c[SEL_BYTES]);
  }
  int flush() { return drain.flush(&stats.bytes_out); }
};

extern "C" int km_select_kernel_ms(float* ms) {
  if (!ms) return fail(KM_E_ARG, "null argument");
  for (int i = 0; i < 4; ++i) ms[i] = g_select_ms[i];
  return KM_OK;
}

extern "C" int km_select_create(kmjf_t* h, uint32_t min_hits, int invert, int min_qual_char, int out_fd, void* stream,
                                km_select_t** out) {
  KMCHK(select_check_create(h, out, min_hits, min_qual_char, 0, &out_fd, 1));
  std::unique_ptr<km_select> s(new (std::nothrow) km_select);
  if (!s) return fail(KM_E_NOMEM, "host allocation failed");
  KMCHK(s->open(h, min_hits, invert, min_qual_char, stream, &s->sync));
  KMCHK(s->in.alloc(0));
  KMCHK(s->out.alloc(1));                               // (room for the newline behind an open last line)
  KMCHK(s->dev.alloc(s->in.bytes, true, s->st));
  for (int i = 0; i < 2; ++i) KMCHK(s->d_out[i].alloc(s->in.bytes + kmsel::OUT_PAD));
  HIPCHK(hipStreamSynchronize(s->st));
  s->drain.out = &s->out;
  s->drain.cs = s->cs;
  s->drain.fd = out_fd;
  for (float& v : g_select_ms) v = 0.f;
  *out = s.release();
  return KM_OK;
}

extern "C" int km_select_add_fastq(km_select_t* s, const char* text, uint64_t n, int final, uint64_t* consumed) {
  if (!s || !consumed || (n && !text)) return fail(KM_E_ARG, "null argument");
  KMCHK(s->alive());
  *consumed = 0;
  if (n == 0) {                                         // nothing for the device or the descriptor; an empty final
    if (final) s->offset = 0;                           // call still ends the stream: the next one's offsets start at 0
    return KM_OK;
  }
  const uint64_t end = kmcut::call_end(text, n, final);
  if (end) HIPCHK(hipSetDevice(s->h->device));
  int rc = KM_OK;
  for (uint64_t pos = 0; pos < end && rc == KM_OK;) {
    uint64_t take = 0;
    rc = fastq_take(text, pos, end, s->in.bytes, s->offset, &take);
    if (rc == KM_OK) rc = s->piece(text + pos, take, s->offset + pos, final && pos + take == end);
    if (rc == KM_OK) {
      pos += take;
      *consumed = pos;
    }
  }
  const std::string msg = rc != KM_OK ? g_last_error : std::string();
  KMCHK(s->end_call(rc, msg, s->flush()));
  s->offset = final ? 0 : s->offset + end;
  return KM_OK;
}

extern "C" int km_select_stats(km_select_t* s, km_select_stats_t* stats) {
  if (!s || !stats) return fail(KM_E_ARG, "null argument");
  *stats = s->stats;
  return KM_OK;
}

extern "C" int km_select_destroy(km_select_t* s) {
  delete s;
  return KM_OK;
}

extern "C" int kmjf_fastq_hits(kmjf_t* h, const char* text, uint64_t n, int min_qual_char, uint32_t* hits, uint64_t cap,
                               uint64_t* n_records, void* stream) {
  if (!h || !n_records || (n && !text) || (cap && !hits)) return fail(KM_E_ARG, "null argument");
  KMCHK(select_check_qual(min_qual_char));
  if (!h->d_slots) return fail(KM_E_STATE, "table not uploaded");
  *n_records = 0;
  if (n == 0) return KM_OK;
  CallStream st;                                        // (declared before what runs on it: released after it)
  KMCHK(st.get(h->device, stream));
  Staging in;
  SelDev dev;
  StreamDrain drain{st};
  KMCHK(in.alloc(0));
  KMCHK(dev.alloc(in.bytes, false, st));
  for (float& v : g_select_ms) v = 0.f;
  const TableView tv = view_of(h);
  uint64_t done = 0;
  for (uint64_t pos = 0; pos < n;) {
    uint64_t take = 0;
    KMCHK(fastq_take(text, pos, n, in.bytes, 0, &take));
    KMCHK(in.claim());
    memcpy(in.mine, text + pos, take);
    KMCHK(in.ship(dev.d_text, take, st));
    KMCHK(dev.front_hits(tv, take, pos, (uint32_t)min_qual_char, st));
    KMCHK(dev.read_back(0, st));
    HIPCHK(hipStreamSynchronize(st));
    KMCHK(dev.drain_spans());
    if (dev.error_of(0) != FQ_NO_ERROR) return select_format_failed(dev.error_of(0));
    const uint64_t records = dev.cells_of(0)[SEL_RECORDS];
    if (done + records > cap)
      return fail(KM_E_CAPACITY, "more than the %llu records there is room for", (unsigned long long)cap);
    if (records) {
      HIPCHK(hipMemcpyAsync(hits + done, dev.hits.p, records * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
    }
    done += records;
    *n_records = done;
    pos += take;
  }
  return KM_OK;
}
