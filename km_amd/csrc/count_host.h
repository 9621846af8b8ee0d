// count_host.h — km_counter_*, km_text_strip, km_fastq_cut (host part of kmgpu.hip; device side: count_kernel.h,
// fastq_kernel.h, and filter_kernel.h / sketch_kernel.h for the counter's other modes, all launched by launch_insert;
// host helpers: fastx_strip.h, fastq_cut.h; records of existing tables: merge_host.h)
// ------------------------------------------------------------------ counting k-mers from reads
// km_counter (include/kmgpu.h): text or bases are staged in two pinned buffers that take turns,
// copied and inserted (count_kernel.h) on the counter's own stream, so the host strips the next block while the
// device inserts the last.  What is staged is ONE byte stream (bases and breaks); it is cut into pieces of the
// staging size that overlap by exactly k - 1 bytes, and a piece counts the windows that lie wholly inside it:
// piece i covers [i (S - k + 1), i (S - k + 1) + S), so a window of k bytes lies wholly inside exactly one piece.
// km_counter_add_fastq stages raw FASTQ text instead, in pieces of whole records that overlap by nothing, and the
// device turns each piece into such a byte stream of its own (fastq_kernel.h) in front of the same insert kernel.
// Whatever is staged, text, FASTQ or the records of merge_host.h, takes one way to the device, that of Staging
// (host_common.h, with the rule that holds the buffers together): claim, fill `mine`, counter_reserve, ship to d_text
// on the counter's stream, then the producer's own kernels.
namespace {
constexpr uint64_t COUNT_DEFAULT_SLOTS = 1ull << 16;
uint64_t key_space(int k) { return k >= 32 ? ~0ull : (1ull << (2 * k)); }

// What km_counter_add_fastq needs on the device beside d_text, allocated by its first call.
struct FastqDev {
  DevBuf<uint8_t> masked;                 // the piece as k_count_insert reads it (k_fq_mask's output)
  DevBuf<uint32_t> tiles, sums;           // newlines per tile, scanned in place (k_scan_*), and the chunk sums
  DevBuf<uint32_t> line_start;
};

const char* fastq_error_text(unsigned kind) {
  switch (kind) {
    case FQ_NO_AT: return "FASTQ record does not start with '@'";
    case FQ_NO_PLUS: return "FASTQ record lacks its '+' line";
    case FQ_QUAL_LEN: return "FASTQ quality line is not as long as its sequence";
    case FQ_TRUNCATED: return "FASTQ record is incomplete";
  }
  return "FASTQ text is malformed";
}
}  // namespace

// What a counter has been fed: text, FASTQ and sum / max records (plain), the inputs of one set operation, or the
// inputs of a comparison (mark_host.h), whose count cells are membership masks.
enum { FEED_NONE = 0, FEED_PLAIN = 1, FEED_SET = 2, FEED_MARK = 3 };

// What a counter does with the windows of its text, i.e. which kernel launch_insert launches: every key inserted; only
// the keys of a filter counted, probed in LDS or in HBM (filter_host.h); or, with a sketch (sketch_host.h), every key
// noted in the first pass and the admitted ones inserted in the second.
enum CountMode { COUNT_PLAIN = 0, COUNT_FILTER_LDS, COUNT_FILTER_HBM, COUNT_SKETCH_NOTE, COUNT_SKETCH_COUNT };

struct km_counter {
  int device = 0, k = 0, canonical = 0;
  Stream st;                              // (declared first: destroyed last)
  DevBuf<CountSlot> table;
  uint64_t slots = 0;
  DevBuf<unsigned long long> meta;        // CM_* cells
  DevBuf<uint8_t> d_text;                 // the staged piece on the device (one: copy and kernel are stream-ordered)
  Staging stg;
  uint64_t fill = 0;                      // bytes of add_bases / add_text in stg.mine
  uint32_t own_from = 0;                  // of those, carried over from the piece before
  uint64_t occ_ub = 0;                    // upper bound of the occupied slots once everything enqueued has run
  uint32_t n_grow = 0;
  bool finished = false;
  km_text_state_t text = {0, 0, 0, 0, 0};
  std::unique_ptr<FastqDev> fq;
  KernelSpans fq_spans;                   // KM_COUNT_TIME_FASTQ: around every piece's line-table and mask kernels
  uint64_t fq_offset = 0;                 // bytes km_counter_add_fastq consumed in the earlier calls of this stream
  unsigned long long fq_error = FQ_NO_ERROR;   // what the device found, once read: (stream offset << 8) | kind
  KernelSpans merge_spans;                // KM_COUNT_TIME_MERGE: around every piece's record kernel (merge_host.h)
  km_counter_stats_t last = {0, 0, 0, 0, 0, 0};
  int feed = FEED_NONE;                   // what the counter has taken: the two kinds do not mix (setops_host.h)
  int set_op = 0;                         // FEED_SET: KM_SET_INTERSECT / KM_SET_SUBTRACT
  uint32_t set_inputs = 0;                // FEED_SET: inputs so far, the empty ones too
  uint32_t mark_inputs = 0;               // FEED_MARK: inputs so far, the empty ones too (mark_host.h)
  KernelSpans cooc_spans;                 // KM_COUNT_TIME_MERGE: around every pass of k_cooc_table (mark_host.h)
  DevBuf<unsigned long long> cooc_cells;  // FEED_MARK: what k_cooc_table adds to, allocated by the first call
  CountMode mode = COUNT_PLAIN;           // set by km_counter_set_filter, km_counter_set_sketch, km_counter_sketch_done
  uint32_t grid_cap = 0;                  // the most blocks of a launch with a bounded grid (filtered, noting)
  KernelSpans insert_spans;               // KM_COUNT_TIME_FILTER: around every insert launch, filtered or not
  DevBuf<uint64_t> sketch;                // sketch_host.h: the words of the sketch (sketch_rule.h)
  uint64_t sketch_words = 0;
  float sketch_note_ms = 0.f;             // ... what insert_spans held when the noting pass ended
  DevBuf<uint64_t> out_keys;
  DevBuf<uint32_t> out_counts;
  uint64_t n_out = 0;
  ~km_counter() {
    (void)hipSetDevice(device);
    if (st) (void)hipStreamSynchronize(st);
  }
};

// A format error the device found (km_counter_add_fastq) stays with the counter: every call from then on fails.
static int counter_format_failed(const km_counter* c) {
  return fail(KM_E_FORMAT, "%s at byte offset %llu", fastq_error_text((unsigned)(c->fq_error & 0xFF)),
              (unsigned long long)(c->fq_error >> 8));
}

// What every call that feeds or ends a counter checks once its arguments are in order.
static int counter_usable(const km_counter* c) {
  if (c->finished) return fail(KM_E_STATE, "counter already finished");
  if (c->fq_error != FQ_NO_ERROR) return counter_format_failed(c);
  return KM_OK;
}

// ... and every call that feeds text, FASTQ or sum / max records
static int counter_takes_plain(const km_counter* c) {
  KMCHK(counter_usable(c));
  if (c->feed == FEED_SET)
    return fail(KM_E_STATE, "counter holds the inputs of a set operation (%s): it takes no text, FASTQ or sum / max records",
                c->set_op == KM_SET_INTERSECT ? "intersect" : "subtract");
  if (c->feed == FEED_MARK)
    return fail(KM_E_STATE, "counter holds the inputs of a comparison (mark): it takes no text, FASTQ or sum / max records");
  return KM_OK;
}

// ... and every call that reads count cells as counts (finish, records, write_jf, histo, dump): those of a counter
// that holds the inputs of a comparison are membership masks (mark_host.h)
static int counter_holds_counts(const km_counter* c, const char* what) {
  if (c->feed == FEED_MARK)
    return fail(KM_E_STATE, "counter holds the inputs of a comparison (mark): its count cells are membership masks, and %s "
                "has nothing to read; km_counter_cooccurrence is its result", what);
  return KM_OK;
}

static bool counter_has_filter(const km_counter* c) { return c->mode == COUNT_FILTER_LDS || c->mode == COUNT_FILTER_HBM; }
static bool counter_has_sketch(const km_counter* c) { return c->mode == COUNT_SKETCH_NOTE || c->mode == COUNT_SKETCH_COUNT; }

// ... and every call that feeds records, of either kind: a filter restricts what is counted from reads, and a
// record brings a count of its own (filter_host.h)
static int counter_takes_records(const km_counter* c) {
  if (counter_has_filter(c))
    return fail(KM_E_STATE, "counter has a filter: it counts reads (add_bases, add_text, add_fastq) and takes no records");
  if (counter_has_sketch(c))
    return fail(KM_E_STATE, "counter has a sketch: it counts reads (add_bases, add_text, add_fastq) and takes no records");
  return KM_OK;
}

// ... and every call that reads the table or ends the counter: while a sketch is in its noting pass there is no table
// to speak of (sketch_host.h)
static int counter_sketch_settled(const km_counter* c) {
  if (c->mode == COUNT_SKETCH_NOTE) return fail(KM_E_STATE, "the counter's sketch is in its first pass: km_counter_sketch_done comes first");
  return KM_OK;
}

// nothing claims a slot: a filter's table never grows, and the noting pass of a sketch does not touch the table
static bool counter_table_fixed(const km_counter* c) { return counter_has_filter(c) || c->mode == COUNT_SKETCH_NOTE; }

// waits for everything enqueued
static int counter_read_meta(km_counter* c, unsigned long long* m) {
  HIPCHK(hipMemcpyAsync(m, c->meta, CM_WORDS * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  if (m[CM_ERROR]) return fail(KM_E_HIP, "counting table ran full (%llu keys not placed)", m[CM_ERROR]);
  if (m[CM_FORMAT] != FQ_NO_ERROR) {
    c->fq_error = m[CM_FORMAT];
    return counter_format_failed(c);
  }
  c->last.bases = m[CM_BASES];
  c->last.kmers = m[CM_KMERS];
  c->last.distinct = m[CM_DISTINCT] + (m[CM_ALLT] || m[CM_ALLT_HAVE] ? 1 : 0);
  c->last.slots = c->slots;
  c->last.n_grow = c->n_grow;
  return KM_OK;
}

// Room for `windows` more keys, every one of them new: the load limit (1/2) is checked against that worst case
// BEFORE the piece is inserted, so an insert kernel never meets a full table.  The bound kept on the host only
// grows; when it no longer fits, the exact occupancy is read (one wait for the pieces in flight) and, if that
// does not fit either, the table is rehashed into one of 2^d times the capacity.
static int counter_reserve(km_counter* c, uint64_t windows) {
  const uint64_t space = key_space(c->k);
  auto need_of = [&](uint64_t occ) { return std::min(occ + windows, space); };
  if (need_of(c->occ_ub) <= c->slots / 2) { c->occ_ub = need_of(c->occ_ub); return KM_OK; }
  unsigned long long m[CM_WORDS];
  KMCHK(counter_read_meta(c, m));
  const uint64_t need = need_of(m[CM_DISTINCT]);
  uint64_t ns = c->slots;
  uint32_t d = 0;
  while (need > ns / 2) {
    if (ns >> 62) return fail(KM_E_CAPACITY, "counting table would exceed 2^62 slots");
    ns <<= 1;
    ++d;
  }
  if (d) {
    DevBuf<CountSlot> grown;
    KMCHK(grown.alloc(ns));
    hipLaunchKernelGGL(k_count_init, dim3(grid_for(ns, 256)), dim3(256), 0, c->st, grown.p, ns);
    hipLaunchKernelGGL(k_count_rehash, dim3(grid_for(c->slots, 256)), dim3(256), 0, c->st, c->table.p, c->slots,
                       grown.p, ns - 1, c->meta.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->st));
    c->table = std::move(grown);
    c->slots = ns;
    c->n_grow += d;
  }
  c->occ_ub = need;
  return KM_OK;
}

// text[0 .. n) on the device into the table; the windows that start before own_from belong to the piece before.
// A lane per 32 bytes, 256 lanes per block.  A counter with a filter only looks its keys up (filter_kernel.h); one with
// a sketch notes the keys in its first pass and counts the admitted ones in its second (sketch_kernel.h).  The filtered
// and the noting kernel take a bounded grid: a block makes as many trips over the text as it takes.
static int launch_insert(km_counter* c, const uint8_t* text, uint64_t n, uint32_t own_from) {
  const uint64_t lanes = (n + COUNT_RUN - 1) / COUNT_RUN;
  const dim3 block(256), full((uint32_t)((lanes + 255) / 256)), capped(std::min(full.x, c->grid_cap));
  const uint32_t shift = 64u - kmsketch::log2_words(c->sketch_words);      // (of a sketch; unused otherwise)
  KMCHK(c->insert_spans.open(c->st));
  switch (c->mode) {
    case COUNT_PLAIN:
      hipLaunchKernelGGL(k_count_insert, full, block, 0, c->st, text, n, own_from, c->k, c->canonical, c->table.p,
                         c->slots - 1, c->meta.p);
      break;
    case COUNT_FILTER_LDS:
      hipLaunchKernelGGL(k_count_filtered<true>, capped, block, 0, c->st, text, n, own_from, c->k, c->canonical,
                         c->table.p, c->slots - 1, c->meta.p);
      break;
    case COUNT_FILTER_HBM:
      hipLaunchKernelGGL(k_count_filtered<false>, capped, block, 0, c->st, text, n, own_from, c->k, c->canonical,
                         c->table.p, c->slots - 1, c->meta.p);
      break;
    case COUNT_SKETCH_NOTE:
      hipLaunchKernelGGL(k_sketch_note, capped, block, 0, c->st, text, n, own_from, c->k, c->canonical, c->sketch.p,
                         shift, c->meta.p);
      break;
    case COUNT_SKETCH_COUNT:
      hipLaunchKernelGGL(k_count_solid, full, block, 0, c->st, text, n, own_from, c->k, c->canonical, c->table.p,
                         c->slots - 1, c->sketch.p, shift, c->meta.p);
      break;
  }
  HIPCHK(hipGetLastError());
  return c->insert_spans.close(c->st);
}
static_assert(FILTER_THREADS == 256 && SKETCH_THREADS == 256, "launch_insert: one block size for the five kernels");

// Enqueue the piece of add_bases / add_text (copy + insert) and turn to the other buffer, which starts with the
// last k - 1 bytes of this one.  Nothing to do while the buffer holds only such carried bytes.
static int counter_flush(km_counter* c) {
  if (c->fill <= c->own_from) return KM_OK;
  const uint64_t n = c->fill;
  const unsigned char* sent = c->stg.mine;            // (a buffer whose copy is in flight may still be read)
  if (!counter_table_fixed(c)) KMCHK(counter_reserve(c, n >= (uint64_t)c->k ? n - c->k + 1 : 0));
  KMCHK(c->stg.ship(c->d_text, n, c->st));
  KMCHK(launch_insert(c, c->d_text, n, c->own_from));
  KMCHK(c->stg.claim());
  const uint64_t keep = std::min<uint64_t>((uint64_t)c->k - 1, n);
  memcpy(c->stg.mine, sent + n - keep, keep);
  c->fill = keep;
  c->own_from = (uint32_t)keep;
  return KM_OK;
}

// In front of a run of whole pieces (FASTQ records, records of a table): what add_bases / add_text left goes first,
// and the k - 1 bytes it would carry over are dropped, since no k-mer spans a change between the kinds of calls.
// Every piece of the run claims its own buffer, and so does counter_append when its turn comes again.
static int counter_begin_pieces(km_counter* c) {
  KMCHK(counter_flush(c));
  c->fill = 0;
  c->own_from = 0;
  return KM_OK;
}

static int counter_append(km_counter* c, const uint8_t* p, uint64_t n) {
  while (n) {
    if (c->fill == c->stg.bytes) {
      KMCHK(counter_flush(c));
    }
    if (!c->stg.mine) KMCHK(c->stg.claim());            // the first bytes, or the first after a run of whole pieces
    const uint64_t take = std::min(n, c->stg.bytes - c->fill);
    memcpy(c->stg.mine + c->fill, p, take);
    c->fill += take;
    p += take;
    n -= take;
  }
  return KM_OK;
}

extern "C" int km_counter_create(int device, int k, int canonical, uint64_t expected_distinct, km_counter_t** out) {
  if (!out) return fail(KM_E_ARG, "null argument");
  if (k < 2 || k > 32) return fail(KM_E_K, "k=%d unsupported", k);
  if (device < 0) return fail(KM_E_ARG, "device %d", device);
  if (expected_distinct >> 60) return fail(KM_E_ARG, "expected_distinct too large");
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<km_counter> c(new (std::nothrow) km_counter);
  if (!c) return fail(KM_E_NOMEM, "host allocation failed");
  c->device = device;
  c->k = k;
  c->canonical = canonical ? 1 : 0;
  if (const char* e = getenv("KM_COUNT_TIME_MERGE")) c->merge_spans.timed = c->cooc_spans.timed = atoi(e) != 0;
  if (const char* e = getenv("KM_COUNT_TIME_FILTER")) c->insert_spans.timed = atoi(e) != 0;
  c->slots = COUNT_DEFAULT_SLOTS;
  if (expected_distinct) {
    c->slots = 64;
    while (c->slots / 2 < expected_distinct) c->slots <<= 1;
  }
  HIPCHK(hipStreamCreateWithFlags(&c->st.h, hipStreamNonBlocking));
  int rc = c->table.alloc(c->slots);
  if (rc == KM_OK) rc = c->meta.alloc(CM_WORDS);
  if (rc == KM_OK) rc = c->d_text.alloc(c->stg.bytes + COUNT_PAD);
  if (rc == KM_OK) rc = c->stg.alloc(COUNT_PAD);
  if (rc != KM_OK) return rc;
  HIPCHK(hipMemsetAsync(c->meta, 0, CM_WORDS * 8, c->st));
  HIPCHK(hipMemsetAsync(c->meta.p + CM_FORMAT, 0xFF, 8, c->st));        // FQ_NO_ERROR
  hipLaunchKernelGGL(k_count_init, dim3(grid_for(c->slots, 256)), dim3(256), 0, c->st, c->table.p, c->slots);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->st));
  c->last.slots = c->slots;
  *out = c.release();
  return KM_OK;
}

extern "C" int km_counter_add_bases(km_counter_t* c, const uint8_t* bytes, uint64_t n) {
  if (!c || (n && !bytes)) return fail(KM_E_ARG, "null argument");
  KMCHK(counter_takes_plain(c));
  if (n == 0) return KM_OK;
  HIPCHK(hipSetDevice(c->device));
  c->feed = FEED_PLAIN;
  int rc = counter_append(c, bytes, n);
  const uint8_t brk = kmstrip::BREAK;                 // k-mers never span two calls
  if (rc == KM_OK) rc = counter_append(c, &brk, 1);
  return rc;
}

namespace {
struct CounterSink {
  km_counter* c;
  int rc = KM_OK;
  void bytes(const uint8_t* p, uint64_t n) { if (rc == KM_OK) rc = counter_append(c, p, n); }
  void brk() { const uint8_t b = kmstrip::BREAK; bytes(&b, 1); }
};
struct BufferSink {
  uint8_t* out;
  uint64_t n = 0;
  void bytes(const uint8_t* p, uint64_t len) { memcpy(out + n, p, len); n += len; }
  void brk() { out[n++] = kmstrip::BREAK; }
};
int strip_failed(const kmstrip::Result& r) {
  return fail(KM_E_FORMAT, "%s at byte offset %llu", kmstrip::error_text(r.error), (unsigned long long)r.error_offset);
}
}  // namespace

extern "C" int km_counter_add_text(km_counter_t* c, const char* text, uint64_t n, int final, uint64_t* consumed) {
  if (!c || !consumed || (n && !text)) return fail(KM_E_ARG, "null argument");
  KMCHK(counter_takes_plain(c));
  *consumed = 0;
  if (n == 0 && !final) return KM_OK;
  HIPCHK(hipSetDevice(c->device));
  c->feed = FEED_PLAIN;
  CounterSink sink{c};
  const kmstrip::Result r = kmstrip::strip(&c->text, text, n, final, sink);
  *consumed = r.consumed;
  if (sink.rc != KM_OK) return sink.rc;
  if (r.error) return strip_failed(r);
  return KM_OK;
}

// ---- raw FASTQ text, parsed on the device
// The buffers of the front half for pieces of at most `stage` bytes (also select_host.h's).
static int fastq_dev_alloc(FastqDev* f, uint64_t stage) {
  if (stage >= 0xFFFFFFF0ull) return fail(KM_E_ARG, "staging buffers of %llu bytes: the line table is 32-bit",
                                          (unsigned long long)stage);
  const uint64_t max_tiles = (stage + FQ_TILE - 1) / FQ_TILE;
  const uint64_t max_chunks = (max_tiles + 1 + SCAN_CHUNK - 1) / SCAN_CHUNK;
  KMCHK(f->masked.alloc(stage + COUNT_PAD));
  KMCHK(f->tiles.alloc(max_chunks * SCAN_CHUNK));
  KMCHK(f->sums.alloc(max_chunks));
  KMCHK(f->line_start.alloc(stage + 2));                // a piece of n bytes has at most n newlines
  return KM_OK;
}

static int fastq_prepare(km_counter* c) {
  if (c->fq) return KM_OK;
  std::unique_ptr<FastqDev> f(new (std::nothrow) FastqDev);
  if (!f) return fail(KM_E_NOMEM, "host allocation failed");
  KMCHK(fastq_dev_alloc(f.get(), c->stg.bytes));
  if (const char* e = getenv("KM_COUNT_TIME_FASTQ")) c->fq_spans.timed = atoi(e) != 0;
  c->fq = std::move(f);
  return KM_OK;
}

// The front half of a FASTQ piece, d_text[0 .. n) on the device in stream order: line table -> mask into f.masked,
// validation into error_cell.  base: the piece's offset in the stream (for what the validation reports).
static int fastq_front(FastqDev& f, const uint8_t* d_text, uint64_t n, uint64_t base, uint32_t min_qual,
                       unsigned long long* error_cell, hipStream_t st, uint32_t* tiles_out) {
  const uint32_t n_tiles = (uint32_t)((n + FQ_TILE - 1) / FQ_TILE);
  const uint32_t n_chunks = (uint32_t)(((uint64_t)n_tiles + 1 + SCAN_CHUNK - 1) / SCAN_CHUNK);
  HIPCHK(hipMemsetAsync(f.tiles, 0, (uint64_t)n_chunks * SCAN_CHUNK * 4, st));
  hipLaunchKernelGGL(k_fq_count_lines, dim3(n_tiles), dim3(FQ_THREADS), 0, st, d_text, n, f.tiles.p);
  scan_in_place(f.tiles.p, f.sums.p, n_chunks, st);
  hipLaunchKernelGGL(k_fq_line_starts, dim3(n_tiles), dim3(FQ_THREADS), 0, st, d_text, n, f.tiles.p, n_tiles,
                     f.line_start.p);
  hipLaunchKernelGGL(k_fq_mask, dim3(n_tiles), dim3(FQ_THREADS), 0, st, d_text, n, f.tiles.p, n_tiles,
                     f.line_start.p, min_qual, base, f.masked.p, error_cell);
  HIPCHK(hipGetLastError());
  if (tiles_out) *tiles_out = n_tiles;
  return KM_OK;
}

// The next piece of text[pos .. end) for every caller that sends FASTQ pieces (kmcut::next_piece), or KM_E_CAPACITY:
// a record longer than a staging buffer.  stream_offset: where text[0] lies in the stream.
static int fastq_take(const char* text, uint64_t pos, uint64_t end, uint64_t stage, uint64_t stream_offset, uint64_t* take) {
  *take = kmcut::next_piece(text, pos, end, stage);
  if (*take == 0)
    return fail(KM_E_CAPACITY, "no FASTQ record ends within the %llu bytes of a staging buffer from byte offset %llu",
                (unsigned long long)stage, (unsigned long long)(stream_offset + pos));
  return KM_OK;
}

// One piece of whole records, text[0 .. n) with n <= stage: copy -> line table -> mask -> insert, all on the
// counter's stream.  base: the piece's offset in the stream (for what the validation reports).
static int fastq_enqueue(km_counter* c, const char* text, uint64_t n, uint64_t base, uint32_t min_qual) {
  FastqDev& f = *c->fq;
  KMCHK(c->stg.claim());
  memcpy(c->stg.mine, text, n);
  if (!counter_table_fixed(c)) KMCHK(counter_reserve(c, n));   // every byte taken as a window: a bound, and a loose one
  KMCHK(c->stg.ship(c->d_text, n, c->st));
  KMCHK(c->fq_spans.open(c->st));
  KMCHK(fastq_front(f, c->d_text.p, n, base, min_qual, c->meta.p + CM_FORMAT, c->st, nullptr));
  KMCHK(c->fq_spans.close(c->st));
  return launch_insert(c, f.masked, n, 0);
}

extern "C" int km_fastq_cut(const char* text, uint64_t n, uint64_t* cut) {
  if (!cut || (n && !text)) return fail(KM_E_ARG, "null argument");
  *cut = kmcut::cut(text, n);
  return KM_OK;
}

extern "C" int km_counter_add_fastq(km_counter_t* c, const char* text, uint64_t n, int final, int min_qual_char,
                                    uint64_t* consumed) {
  if (!c || !consumed || (n && !text)) return fail(KM_E_ARG, "null argument");
  if (min_qual_char < 0 || min_qual_char > 255) return fail(KM_E_ARG, "min_qual_char %d outside 0..255", min_qual_char);
  KMCHK(counter_takes_plain(c));
  *consumed = 0;
  const uint64_t end = kmcut::call_end(text, n, final);
  if (end) {
    HIPCHK(hipSetDevice(c->device));
    KMCHK(fastq_prepare(c));
    c->feed = FEED_PLAIN;
    KMCHK(counter_begin_pieces(c));
  }
  for (uint64_t pos = 0; pos < end;) {
    uint64_t take = 0;
    KMCHK(fastq_take(text, pos, end, c->stg.bytes, c->fq_offset, &take));
    KMCHK(fastq_enqueue(c, text + pos, take, c->fq_offset + pos, (uint32_t)min_qual_char));
    pos += take;
    *consumed = pos;
  }
  c->fq_offset = final ? 0 : c->fq_offset + end;
  return KM_OK;
}

extern "C" int km_counter_fastq_kernel_ms(km_counter_t* c, float* ms) {
  if (!c || !ms) return fail(KM_E_ARG, "null argument");
  *ms = 0.f;
  if (!c->fq_spans.timed) return KM_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->st));
  return c->fq_spans.drain(ms);
}

extern "C" int km_text_strip(km_text_state_t* st, const char* text, uint64_t n, int final, uint8_t* out, uint64_t cap,
                             uint64_t* n_out, uint64_t* consumed) {
  if (!st || !out || !n_out || !consumed || (n && !text)) return fail(KM_E_ARG, "null argument");
  *n_out = *consumed = 0;
  if (cap < n + 1) return fail(KM_E_CAPACITY, "output buffer too small (%llu bytes of text need %llu)",
                               (unsigned long long)n, (unsigned long long)n + 1);
  BufferSink sink{out};
  const kmstrip::Result r = kmstrip::strip(st, text, n, final, sink);
  *n_out = sink.n;
  *consumed = r.consumed;
  if (r.error) return strip_failed(r);
  return KM_OK;
}

extern "C" int km_counter_stats(km_counter_t* c, km_counter_stats_t* s) {
  if (!c || !s) return fail(KM_E_ARG, "null argument");
  if (c->fq_error != FQ_NO_ERROR) return counter_format_failed(c);
  if (!c->finished) {
    HIPCHK(hipSetDevice(c->device));
    int rc = counter_flush(c);
    unsigned long long m[CM_WORDS];
    if (rc == KM_OK) rc = counter_read_meta(c, m);
    if (rc != KM_OK) return rc;
  }
  *s = c->last;
  return KM_OK;
}

// km_counter_finish / km_counter_finish_range: the slots that survived (every slot unless the counter holds a set
// operation) with lower <= count <= upper into the record arrays, then the lookup table from those.  `ranged` = the
// compaction of setops_kernel.h; without it, the one of count_kernel.h that km_counter_finish has always used.
static int counter_finish_cut(km_counter* c, uint32_t lower_count, uint32_t upper_count, bool ranged, kmjf_t** out,
                              const char* caller = "km_counter_finish") {
  KMCHK(counter_usable(c));
  KMCHK(counter_sketch_settled(c));
  KMCHK(counter_holds_counts(c, caller));
  HIPCHK(hipSetDevice(c->device));
  int rc = counter_flush(c);
  unsigned long long m[CM_WORDS];
  if (rc == KM_OK) rc = counter_read_meta(c, m);
  if (rc != KM_OK) return rc;
  const uint64_t cap = m[CM_DISTINCT] + 1;
  rc = c->out_keys.alloc(cap);
  if (rc == KM_OK) rc = c->out_counts.alloc(cap);
  if (rc != KM_OK) return rc;
  const bool intersect = c->feed == FEED_SET && c->set_op == KM_SET_INTERSECT;
  const uint32_t want = intersect ? c->set_inputs - 1 : 0;      // of the spare word (setops_kernel.h)
  HIPCHK(hipMemsetAsync(c->meta.p + CM_OUT, 0, 8, c->st));
  if (ranged)
    hipLaunchKernelGGL(k_set_compact, dim3(grid_for(c->slots, 256)), dim3(256), 0, c->st, c->table.p, c->slots, want,
                       intersect ? 1 : 0, lower_count, upper_count, c->out_keys.p, c->out_counts.p, c->meta.p);
  else
    hipLaunchKernelGGL(k_count_compact, dim3(grid_for(c->slots, 256)), dim3(256), 0, c->st, c->table.p, c->slots,
                       lower_count, c->out_keys.p, c->out_counts.p, c->meta.p);
  HIPCHK(hipGetLastError());
  KMCHK(counter_read_meta(c, m));
  uint64_t n = m[CM_OUT];
  if (n > m[CM_DISTINCT]) return fail(KM_E_HIP, "compaction wrote %llu records for %llu keys", m[CM_OUT], m[CM_DISTINCT]);
  // T^32 of a non-canonical k = 32 table (count_kernel.h; under a set operation its cells are those of setops_kernel.h,
  // and a filter that holds it lists it with whatever count it has, 0 too)
  const bool have = intersect || counter_has_filter(c) ? m[CM_ALLT_HAVE] != 0 : m[CM_ALLT] != 0;
  const uint32_t allt = intersect ? ~(uint32_t)m[CM_ALLT] : (uint32_t)std::min<unsigned long long>(m[CM_ALLT], 0xFFFFFFFFull);
  if (have && m[CM_ALLT_MATCH] == want && allt >= lower_count && allt <= upper_count) {
    const uint64_t key = EMPTY;
    HIPCHK(hipMemcpyAsync(c->out_keys.p + n, &key, 8, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemcpyAsync(c->out_counts.p + n, &allt, 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    ++n;
  }
  kmjf_t* h = nullptr;
  KMCHK(kmjf_create(c->k, c->canonical, &h));
  rc = kmjf_upload_from_device(h, c->device, c->out_keys, c->out_counts, n, c->st);
  if (rc != KM_OK) { kmjf_close(h); return rc; }
  c->n_out = n;
  c->table.release();
  c->d_text.release();
  c->sketch.release();
  c->fq.reset();
  c->finished = true;
  *out = h;
  return KM_OK;
}

extern "C" int km_counter_finish(km_counter_t* c, uint32_t lower_count, kmjf_t** out) {
  if (!c || !out) return fail(KM_E_ARG, "null argument");
  return counter_finish_cut(c, lower_count, 0xFFFFFFFFu, c->feed == FEED_SET, out);
}

extern "C" int km_counter_records(km_counter_t* c, uint64_t* keys, uint32_t* counts, uint64_t cap, uint64_t* n) {
  if (!c || !n) return fail(KM_E_ARG, "null argument");
  KMCHK(counter_sketch_settled(c));
  KMCHK(counter_holds_counts(c, "km_counter_records"));
  if (!c->finished) return fail(KM_E_STATE, "km_counter_finish comes first");
  *n = c->n_out;
  if (!keys && !counts) return KM_OK;
  if (!keys || !counts) return fail(KM_E_ARG, "null argument");
  if (cap < c->n_out) return fail(KM_E_CAPACITY, "%llu records, room for %llu", (unsigned long long)c->n_out,
                                  (unsigned long long)cap);
  if (c->n_out == 0) return KM_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(keys, c->out_keys, c->n_out * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipMemcpyAsync(counts, c->out_counts, c->n_out * 4, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return KM_OK;
}

extern "C" int km_counter_destroy(km_counter_t* c) {
  delete c;
  return KM_OK;
}
