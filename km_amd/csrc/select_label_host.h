// select_label_host.h — km_select_labels_*, kmjf_fastq_label_hits (host part of kmgpu.hip; device side:
// select_label_kernel.h after fastq_kernel.h's front half; the rule: select_label_rule.h)
// ------------------------------------------------------------------ select, labels: one output per label of a table
// A piece goes to the device as in select_host.h and through the same front half.  Then per piece: the hits per record
// and label, the kept records' lengths per label, ONE scan over all the labels' planes, and the gather of the virtual
// stream (label 0's bytes, then label 1's, ...) into one of two output buffers of the single selector's size, `cap`
// bytes of it per pass.  Pass 0 is launched behind the scan without a host round trip; the totals and label_off come
// back with it, and only a piece whose stream is longer than `cap` takes further passes.  LabelDrain cuts each pass's
// bytes at the label_off boundaries and writes every range to its label's descriptor a pass (or piece) later.
namespace {

// TextDrain's sibling for several descriptors: the bytes in flight into out->pin[i] are ranges of labels.
struct LabelDrain {
  struct Range {
    uint32_t label;
    uint64_t at, bytes;                   // within the pinned buffer
    bool ends_label;                      // its last byte is the last of the label's bytes of the piece
  };
  Staging* out = nullptr;
  hipStream_t cs = nullptr;               // the copy stream
  std::vector<int> fds;
  int turn = 0;                           // the buffer of the next pass
  uint64_t pending[2] = {0, 0};           // bytes of the copy in flight into out->pin[i]
  std::vector<Range> ranges[2];
  bool close_line[2] = {false, false};    // a range of out->pin[i] that ends without a newline gets one behind it
  std::vector<uint64_t> closed;           // ... and how often that happened, per label
  int begin() {
    turn ^= 1;
    return turn ^ 1;
  }
  // Bytes [lo, hi) of a piece's virtual stream (ready in d_src: the host has waited for what wrote them) on their way
  // into out->pin[buf]; label_off[0 .. n_labels] cuts them.
  int fetch(int buf, const void* d_src, uint64_t lo, uint64_t hi, const volatile uint32_t* label_off, bool close) {
    ranges[buf].clear();
    pending[buf] = hi - lo;
    close_line[buf] = close;
    if (hi == lo) return KM_OK;
    KMCHK(out->fetch(buf, d_src, hi - lo, cs));
    for (uint32_t l = 0; l < fds.size(); ++l) {
      const uint64_t a = std::max<uint64_t>(label_off[l], lo), b = std::min<uint64_t>(label_off[l + 1], hi);
      if (a < b) ranges[buf].push_back(Range{l, a - lo, b - a, b == label_off[l + 1]});
    }
    return KM_OK;
  }
  int put(int buf) {                      // the text copied into out->pin[buf] goes to the descriptors
    if (!pending[buf]) return KM_OK;
    unsigned char* got = nullptr;
    KMCHK(out->wait(buf, &got));
    pending[buf] = 0;
    for (const Range& r : ranges[buf]) {
      int e = dump_write_all(fds[r.label], got + r.at, r.bytes);
      // only the last record of a stream can lack its newline: a label's bytes of the stream's last piece end in it
      if (!e && close_line[buf] && r.ends_label && got[r.at + r.bytes - 1] != '\n') {
        const unsigned char nl = '\n';
        e = dump_write_all(fds[r.label], &nl, 1);
        ++closed[r.label];
      }
      if (e) return fail(KM_E_IO, "writing the text of label %u failed: %s", r.label, strerror(e));
    }
    return KM_OK;
  }
  int put_before(int buf) { return put(buf ^ 1); }
  int flush(uint64_t* bytes_out) {
    int rc = put(turn);
    if (rc == KM_OK) rc = put(turn ^ 1);
    for (size_t l = 0; l < closed.size(); ++l) {
      bytes_out[l] += closed[l];
      closed[l] = 0;
    }
    return rc;
  }
};

// Device side of one piece, shared by the label selector and kmjf_fastq_label_hits.
struct LabDev {
  FastqDev fq;
  DevBuf<uint8_t> d_text;
  DevBuf<uint32_t> hits, len, sums;       // n_labels planes each; len is scanned in place as one array
  DevBuf<unsigned long long> meta;        // [0] the format-error cell (sticky), behind it the piece's LAB_* cells
  Pinned back;                            // BACK bytes of meta per output buffer
  KernelSpans spans[4];                   // KM_SELECT_TIME: front half, clear + hits, sizes + scan + offsets, gather
  static constexpr uint64_t BACK = 8 + 4 * LAB_CELLS;
  uint64_t stage = 0, hit_stride = 0;
  uint32_t n_labels = 0, n_tiles = 0;
  uint32_t* cells() const { return reinterpret_cast<uint32_t*>(meta.p + 1); }
  int alloc(uint64_t stage_bytes, uint32_t labels, bool gather, hipStream_t st) {
    stage = stage_bytes;
    n_labels = labels;
    hit_stride = kmsel::hit_cells(stage);
    KMCHK(fastq_dev_alloc(&fq, stage));
    KMCHK(d_text.alloc(stage + COUNT_PAD));
    KMCHK(hits.alloc(hit_stride * n_labels));
    KMCHK(meta.alloc(1 + LAB_CELLS / 2));
    if (gather) {
      const uint64_t chunks = SelDev::len_chunks(stage) * n_labels;
      KMCHK(len.alloc(chunks * SCAN_CHUNK));
      KMCHK(sums.alloc(chunks));
    }
    KMCHK(pinned_alloc(&back, 2 * BACK, "pinned totals"));
    if (const char* e = getenv("KM_SELECT_TIME"))
      for (KernelSpans& s : spans) s.timed = atoi(e) != 0;
    HIPCHK(hipMemsetAsync(meta.p, 0xFF, 8, st));            // FQ_NO_ERROR
    HIPCHK(hipMemsetAsync(meta.p + 1, 0, 4 * LAB_CELLS, st));
    return KM_OK;
  }
  // d_text[0 .. n) is there in stream order -> hits[l * hit_stride + r] of its records, cells()[LAB_RECORDS]
  int front_hits(const TableView& tv, uint64_t n, uint64_t base, uint32_t min_qual, hipStream_t st) {
    KMCHK(spans[0].open(st));
    KMCHK(fastq_front(fq, d_text.p, n, base, min_qual, meta.p, st, &n_tiles));
    KMCHK(spans[0].close(st));
    KMCHK(spans[1].open(st));
    hipLaunchKernelGGL(k_lab_clear, dim3(grid_for(n / 4 + 2, kmsel::THREADS)), dim3(kmsel::THREADS), 0, st, d_text.p, n,
                       fq.tiles.p, n_tiles, n_labels, hit_stride, hits.p, cells());
    const uint64_t lanes = (n + kmscan::RUN - 1) / kmscan::RUN;
    hipLaunchKernelGGL(k_lab_hits, dim3((uint32_t)((lanes + kmscan::THREADS - 1) / kmscan::THREADS)), dim3(kmscan::THREADS),
                       0, st, tv, d_text.p, fq.masked.p, (uint32_t)n, fq.tiles.p, n_tiles, fq.line_start.p, n_labels,
                       hit_stride, hits.p);
    HIPCHK(hipGetLastError());
    return spans[1].close(st);
  }
  static uint32_t stride_of(uint64_t n) { return kmlab::len_stride(n, SCAN_CHUNK); }
  // ... -> the scanned planes of the piece, cells()[LAB_BYTES ..], and pass 0 of the gather in d_out (cap bytes of room)
  int sizes_gather(uint64_t n, uint32_t min_hits, uint64_t cap, uint8_t* d_out, hipStream_t st) {
    const uint32_t stride = stride_of(n);
    KMCHK(spans[2].open(st));
    hipLaunchKernelGGL(k_lab_sizes, dim3(stride / kmsel::THREADS), dim3(kmsel::THREADS), 0, st, fq.line_start.p, (uint32_t)n,
                       hits.p, hit_stride, n_labels, min_hits, len.p, stride, cells());
    scan_in_place(len.p, sums.p, n_labels * (stride / SCAN_CHUNK), st);
    hipLaunchKernelGGL(k_lab_offsets, dim3(1), dim3(64), 0, st, len.p, n_labels, stride, cells());
    HIPCHK(hipGetLastError());
    KMCHK(spans[2].close(st));
    return gather_pass(n, 0, cap, d_out, st);
  }
  // pass p of the piece's gather: bytes [p * cap, (p + 1) * cap) of its virtual stream, as far as they exist
  int gather_pass(uint64_t n, uint64_t p, uint64_t cap, uint8_t* d_out, hipStream_t st) {
    const uint64_t all = (n * n_labels + kmsel::WORD - 1) / kmsel::WORD, first = p * (cap / kmsel::WORD);   // (total <= n * n_labels)
    const uint32_t words = (uint32_t)std::min<uint64_t>(cap / kmsel::WORD, all > first ? all - first : 1);
    KMCHK(spans[3].open(st));
    hipLaunchKernelGGL(k_lab_gather, dim3((words + kmsel::THREADS - 1) / kmsel::THREADS), dim3(kmsel::THREADS), 0, st,
                       d_text.p, fq.line_start.p, len.p, n_labels, stride_of(n), (uint32_t)(p * (cap / kmsel::WORD)), words,
                       d_out);
    HIPCHK(hipGetLastError());
    return spans[3].close(st);
  }
  int read_back(int buf, hipStream_t st) {
    HIPCHK(hipMemcpyAsync(back.h + BACK * buf, meta.p, BACK, hipMemcpyDeviceToHost, st));
    return KM_OK;
  }
  unsigned long long error_of(int buf) const { return *reinterpret_cast<const volatile unsigned long long*>(back.h + BACK * buf); }
  const volatile uint32_t* cells_of(int buf) const { return reinterpret_cast<const volatile uint32_t*>(back.h + BACK * buf + 8); }
  int drain_spans() {
    for (int i = 0; i < 4; ++i) KMCHK(spans[i].drain(&g_select_ms[i]));
    return KM_OK;
  }
};

int select_check_labels(uint32_t n_labels) {
  if (n_labels == 0 || n_labels > kmlab::MAX_LABELS)
    return fail(KM_E_ARG, "n_labels %u outside 1..%u", n_labels, kmlab::MAX_LABELS);
  return KM_OK;
}
}  // namespace

struct km_select_labels : SelCore {
  uint32_t n_labels = 0;
  Staging in, out;
  LabDev dev;
  DevBuf<uint8_t> d_out[2];
  LabelDrain drain;
  uint64_t cap = 0;                       // bytes of the virtual stream per gather pass
  uint64_t offset = 0;                    // bytes consumed by the earlier calls of this stream
  km_select_labels_stats_t stats;
  std::vector<uint64_t> records_out, bytes_out;
  StreamDrain sync;
  km_select_labels() { memset(&stats, 0, sizeof stats); }
  // One piece of whole records; ends: the stream ends with it.
  int piece(const char* text, uint64_t n, uint64_t base, bool ends) {
    int buf = drain.begin();
    KMCHK(in.claim());
    memcpy(in.mine, text, n);
    KMCHK(in.ship(dev.d_text, n, st));
    KMCHK(dev.front_hits(view_of(h), n, base, min_qual, st));
    KMCHK(dev.sizes_gather(n, min_hits, cap, d_out[buf].p, st));
    KMCHK(dev.read_back(buf, st));
    HIPCHK(hipEventRecord(done[buf], st));
    KMCHK(drain.put_before(buf));         // while this one is scanned
    HIPCHK(hipEventSynchronize(done[buf]));
    KMCHK(dev.drain_spans());
    if (dev.error_of(buf) != FQ_NO_ERROR) return select_format_failed(dev.error_of(buf));
    uint32_t c[LAB_CELLS];
    for (uint32_t i = 0; i < LAB_CELLS; ++i) c[i] = dev.cells_of(buf)[i];
    stats.records_in += c[LAB_RECORDS];
    stats.records_any += c[LAB_ANY];
    stats.records_multi += c[LAB_MULTI];
    stats.bytes_in += n;
    ++stats.pieces;
    for (uint32_t l = 0; l < n_labels; ++l) {
      records_out[l] += c[LAB_KEPT + l];
      bytes_out[l] += c[LAB_BYTES + l];
    }
    const uint64_t total = c[LAB_TOTAL];
    const bool close = ends && text[n - 1] != '\n';
    const uint64_t passes = kmlab::pass_count(total, cap);
    stats.gather_passes += passes;
    KMCHK(drain.fetch(buf, d_out[buf].p, 0, std::min(total, cap), c + LAB_OFF, close));
    for (uint64_t p = 1; p < passes; ++p) {
      buf = drain.begin();
      KMCHK(dev.gather_pass(n, p, cap, d_out[buf].p, st));
      HIPCHK(hipEventRecord(done[buf], st));
      KMCHK(drain.put_before(buf));       // while this pass is gathered
      HIPCHK(hipEventSynchronize(done[buf]));
      KMCHK(dev.drain_spans());
      KMCHK(drain.fetch(buf, d_out[buf].p, p * cap, std::min(total, (p + 1) * cap), c + LAB_OFF, close));
    }
    return KM_OK;
  }
  int flush() { return drain.flush(bytes_out.data()); }
};

extern "C" int km_select_labels_create(kmjf_t* h, uint32_t n_labels, const int* out_fds, uint32_t min_hits,
                                       int min_qual_char, void* stream, km_select_labels_t** out) {
  if (!h || !out || !out_fds) return fail(KM_E_ARG, "null argument");
  if (min_hits == 0) return fail(KM_E_ARG, "min_hits must be at least 1");
  KMCHK(select_check_qual(min_qual_char));
  KMCHK(select_check_labels(n_labels));
  for (uint32_t i = 0; i < n_labels; ++i)
    for (uint32_t j = 0; j < i; ++j)
      if (out_fds[i] == out_fds[j])
        return fail(KM_E_ARG, "every label needs a descriptor of its own, labels %u and %u both have %d", j, i, out_fds[i]);
  if (!h->d_slots) return fail(KM_E_STATE, "table not uploaded");
  for (uint32_t i = 0; i < n_labels; ++i) KMCHK(dump_check_fd(out_fds[i]));
  std::unique_ptr<km_select_labels> s(new (std::nothrow) km_select_labels);
  if (!s) return fail(KM_E_NOMEM, "host allocation failed");
  if ((uint64_t)n_labels * s->in.bytes >= (1ull << 32))
    return fail(KM_E_CAPACITY, "%u labels times staging buffers of %llu bytes: the offsets of a piece's outputs are 32-bit",
                n_labels, (unsigned long long)s->in.bytes);
  KMCHK(s->open(h, min_hits, 0, min_qual_char, stream, &s->sync));
  s->n_labels = n_labels;
  s->records_out.assign(n_labels, 0);
  s->bytes_out.assign(n_labels, 0);
  KMCHK(s->in.alloc(0));
  KMCHK(s->out.alloc(kmsel::OUT_PAD));
  KMCHK(s->dev.alloc(s->in.bytes, n_labels, true, s->st));
  s->cap = kmlab::pass_bytes(s->in.bytes + kmsel::OUT_PAD);
  for (int i = 0; i < 2; ++i) KMCHK(s->d_out[i].alloc(s->in.bytes + kmsel::OUT_PAD));
  HIPCHK(hipStreamSynchronize(s->st));
  s->drain.out = &s->out;
  s->drain.cs = s->cs;
  s->drain.fds.assign(out_fds, out_fds + n_labels);
  s->drain.closed.assign(n_labels, 0);
  for (float& v : g_select_ms) v = 0.f;
  *out = s.release();
  return KM_OK;
}

extern "C" int km_select_labels_add_fastq(km_select_labels_t* s, const char* text, uint64_t n, int final, uint64_t* consumed) {
  if (!s || !consumed || (n && !text)) return fail(KM_E_ARG, "null argument");
  KMCHK(s->alive());
  *consumed = 0;
  if (n == 0) {                                         // as km_select_add_fastq: an empty final call ends the stream
    if (final) s->offset = 0;
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

extern "C" int km_select_labels_stats(km_select_labels_t* s, km_select_labels_stats_t* stats, uint64_t* records_out,
                                      uint64_t* bytes_out) {
  if (!s || !stats || !records_out || !bytes_out) return fail(KM_E_ARG, "null argument");
  *stats = s->stats;
  for (uint32_t l = 0; l < s->n_labels; ++l) {
    records_out[l] = s->records_out[l];
    bytes_out[l] = s->bytes_out[l];
  }
  return KM_OK;
}

extern "C" int km_select_labels_destroy(km_select_labels_t* s) {
  delete s;
  return KM_OK;
}

extern "C" int kmjf_fastq_label_hits(kmjf_t* h, uint32_t n_labels, const char* text, uint64_t n, int min_qual_char,
                                     uint32_t* hits, uint64_t cap, uint64_t* n_records, void* stream) {
  if (!h || !n_records || (n && !text) || (cap && !hits)) return fail(KM_E_ARG, "null argument");
  KMCHK(select_check_qual(min_qual_char));
  KMCHK(select_check_labels(n_labels));
  if (!h->d_slots) return fail(KM_E_STATE, "table not uploaded");
  *n_records = 0;
  if (n == 0) return KM_OK;
  CallStream st;                                        // (declared before what runs on it: released after it)
  KMCHK(st.get(h->device, stream));
  Staging in;
  LabDev dev;
  StreamDrain drain{st};
  KMCHK(in.alloc(0));
  KMCHK(dev.alloc(in.bytes, n_labels, false, st));
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
    const uint64_t records = dev.cells_of(0)[LAB_RECORDS];
    if (done + records > cap)
      return fail(KM_E_CAPACITY, "more than the %llu records there is room for", (unsigned long long)cap);
    if (records) {
      for (uint32_t l = 0; l < n_labels; ++l)
        HIPCHK(hipMemcpyAsync(hits + l * cap + done, dev.hits.p + l * dev.hit_stride, records * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
    }
    done += records;
    *n_records = done;
    pos += take;
  }
  return KM_OK;
}
