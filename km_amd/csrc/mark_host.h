// mark_host.h — km_counter_mark_records, km_counter_mark_jf, km_counter_cooccurrence (host part of kmgpu.hip; device
// side: mark_kernel.h, cooc_kernel.h; the arithmetic: cooc_rule.h; the way of a piece through the counter's Staging:
// merge_host.h)
// ------------------------------------------------------------------ comparing the inputs of a counter
// Every mark call is ONE input: it takes the next ordinal g (0-based), and all its pieces carry it.  Any input may
// bring new keys, so counter_reserve stands in front of every piece of every input (the set operations reserve for
// their first input only) and the table grows between pieces; k_count_rehash carries the count cell, which here is the
// membership mask.  km_counter_cooccurrence reads the table in one pass and leaves it as it was, so it may be called
// between inputs and again.
namespace {
// What both mark calls check first, in this order; nothing is changed.
int mark_check(const km_counter* c) {
  KMCHK(counter_usable(c));
  KMCHK(counter_takes_records(c));
  if (c->feed == FEED_PLAIN)
    return fail(KM_E_STATE, "counter has taken text, FASTQ or sum / max records: a comparison (mark) needs a counter of its own");
  if (c->feed == FEED_SET)
    return fail(KM_E_STATE, "counter holds the inputs of a set operation (%s): it cannot take one of a comparison (mark)",
                c->set_op == KM_SET_INTERSECT ? "intersect" : "subtract");
  if (c->mark_inputs >= kmcooc::MAX_INPUTS)
    return fail(KM_E_CAPACITY, "counter holds %u inputs already: a comparison takes at most %u", c->mark_inputs,
                kmcooc::MAX_INPUTS);
  return KM_OK;
}

// The call has passed every check: it is the next input, with or without records.
uint32_t mark_begin_input(km_counter* c) {
  c->feed = FEED_MARK;
  return c->mark_inputs++;
}

// n records of kb + cb bytes as input g; fill(dst, piece) writes piece.bytes bytes of them to a pinned buffer.
template <typename Fill>
int mark_enqueue(km_counter* c, uint64_t n, uint32_t kb, uint32_t cb, uint32_t lower, uint32_t upper, uint32_t g, Fill fill) {
  const uint64_t rec = (uint64_t)kb + cb, per = kmpiece::per_piece(c->stg.bytes, rec);
  HIPCHK(hipSetDevice(c->device));
  const uint64_t pieces = kmpiece::n_pieces(n, per);
  for (uint64_t i = 0; i < pieces; ++i) {
    const kmpiece::Piece p = kmpiece::piece(n, per, rec, i);
    KMCHK(c->stg.claim());
    KMCHK(fill(c->stg.mine, p));
    KMCHK(counter_reserve(c, p.records));               // any input may bring new keys
    KMCHK(c->stg.ship(c->d_text, p.bytes, c->st));
    KMCHK(c->merge_spans.open(c->st));
    hipLaunchKernelGGL(k_mark_records, dim3(grid_for(p.records, 256)), dim3(256), 0, c->st, c->d_text.p, p.records, kb, cb,
                       lower, upper, g, c->table.p, c->slots - 1, c->meta.p);
    HIPCHK(hipGetLastError());
    KMCHK(c->merge_spans.close(c->st));
  }
  return KM_OK;
}
}  // namespace

extern "C" int km_counter_mark_records(km_counter_t* c, const uint64_t* keys, const uint32_t* counts, uint64_t n,
                                       uint32_t lower, uint32_t upper) {
  if (!c || (n && (!keys || !counts))) return fail(KM_E_ARG, "null argument");
  KMCHK(mark_check(c));
  const uint32_t g = mark_begin_input(c);
  if (n == 0) return KM_OK;
  return mark_enqueue(c, n, (uint32_t)kmpiece::PACKED_KEY_BYTES, (uint32_t)kmpiece::PACKED_COUNT_BYTES, lower, upper, g,
                      [&](unsigned char* dst, const kmpiece::Piece& p) {
                        kmpiece::pack(keys, counts, p.first, p.records, dst);
                        return KM_OK;
                      });
}

extern "C" int km_counter_mark_jf(km_counter_t* c, const char* path, uint32_t lower, uint32_t upper, uint64_t* n_records) {
  if (!c || !path) return fail(KM_E_ARG, "null argument");
  KMCHK(mark_check(c));
  RecordFile file;
  KMCHK(file.open(path));
  const jfio::Layout& lay = file.lay;
  if (lay.k != c->k || lay.canonical != c->canonical)
    return fail(KM_E_ARG, "%s holds k=%d canonical=%d, the counter k=%d canonical=%d", path, lay.k, lay.canonical, c->k,
                c->canonical);
  if (n_records) *n_records = lay.n_records;
  const uint32_t g = mark_begin_input(c);
  if (lay.n_records == 0) return KM_OK;
  return mark_enqueue(c, lay.n_records, lay.key_bytes, lay.counter_bytes, lower, upper, g,
                      [&](unsigned char* dst, const kmpiece::Piece& p) { return file.read(p, dst); });
}

extern "C" int km_counter_cooccurrence(km_counter_t* c, km_cooc_t* out) {
  if (!c || !out) return fail(KM_E_ARG, "null argument");
  KMCHK(counter_usable(c));
  if (c->feed != FEED_MARK && c->feed != FEED_NONE)
    return fail(KM_E_STATE, "counter does not hold the inputs of a comparison: km_counter_mark_records / _mark_jf feed one");
  // (cooc_kernel.h) a block's 32-bit bins count the slots it visits: slots / COOC_GRID + 256 of them
  if (c->slots >> 42) return fail(KM_E_CAPACITY, "a table of %llu slots is beyond what one pass counts", (unsigned long long)c->slots);
  HIPCHK(hipSetDevice(c->device));
  const uint32_t n = c->mark_inputs;
  const uint64_t words = (uint64_t)COOC_SETS * kmcooc::CELLS;
  std::vector<unsigned long long> host(words, 0ull);
  if (n) {
    KMCHK(c->cooc_cells.alloc(words));
    HIPCHK(hipMemsetAsync(c->cooc_cells, 0, words * 8, c->st));
    KMCHK(c->cooc_spans.open(c->st));
    hipLaunchKernelGGL(k_cooc_table, dim3(std::min<uint32_t>((uint32_t)grid_for(c->slots, COOC_THREADS), COOC_GRID)),
                       dim3(COOC_THREADS), 0, c->st, c->table.p, c->slots, n, c->cooc_cells.p);
    HIPCHK(hipGetLastError());
    KMCHK(c->cooc_spans.close(c->st));
    HIPCHK(hipMemcpyAsync(host.data(), c->cooc_cells, words * 8, hipMemcpyDeviceToHost, c->st));
  }
  unsigned long long m[CM_WORDS];
  KMCHK(counter_read_meta(c, m));                         // waits for the marks, the pass and the copy
  float ms = 0.f;
  KMCHK(c->cooc_spans.drain(&ms));
  uint64_t cells[kmcooc::CELLS] = {0};
  for (uint32_t s = 0; s < COOC_SETS; ++s)
    for (uint32_t i = 0; i < kmcooc::CELLS; ++i) cells[i] += host[(uint64_t)s * kmcooc::CELLS + i];
  static_assert(sizeof out->shared == sizeof(kmcooc::Result::shared) && sizeof out->in_exactly == sizeof(kmcooc::Result::in_exactly) &&
                    sizeof out->private_to == sizeof(kmcooc::Result::priv),
                "km_cooc_t is laid out as kmcooc::Result");
  kmcooc::Result r;
  kmcooc::fold(cells, n, (uint32_t)m[CM_ALLT], &r);       // the key ~0 has no slot: its mask joins every number here
  memset(out, 0, sizeof *out);
  out->n_inputs = n;
  out->n_union = r.n_union;
  memcpy(out->shared, r.shared, sizeof r.shared);
  memcpy(out->in_exactly, r.in_exactly, sizeof r.in_exactly);
  memcpy(out->private_to, r.priv, sizeof r.priv);
  out->kernel_ms = ms;
  return KM_OK;
}
