// setops_host.h — km_counter_set_records, km_counter_set_jf, km_counter_finish_range (host part of kmgpu.hip; device
// side: setops_kernel.h; the way of a piece through the counter's Staging: merge_host.h)
// ------------------------------------------------------------------ set operations over the inputs of a counter
// Every call is ONE input: it takes the next ordinal g, and all its pieces carry it.  Input 1 is enqueued as
// merge_enqueue enqueues (counter_reserve in front of every piece: its records may all be new keys); later inputs only
// look keys up, so nothing is reserved for them and the table keeps the size input 1 left it with.
namespace {
const char* set_name(int op) { return op == KM_SET_INTERSECT ? "intersect" : "subtract"; }

// What both set calls check first, in this order; nothing is changed.
int set_check(const km_counter* c, int op) {
  if (op != KM_SET_INTERSECT && op != KM_SET_SUBTRACT)
    return fail(KM_E_ARG, "op %d is neither KM_SET_INTERSECT nor KM_SET_SUBTRACT", op);
  KMCHK(counter_usable(c));
  KMCHK(counter_takes_records(c));
  if (c->feed == FEED_PLAIN)
    return fail(KM_E_STATE, "counter has taken text, FASTQ or sum / max records: a set operation (%s) needs a counter of its own",
                set_name(op));
  if (c->feed == FEED_MARK)
    return fail(KM_E_STATE, "counter holds the inputs of a comparison (mark): a set operation (%s) needs a counter of its own",
                set_name(op));
  if (c->feed == FEED_SET && c->set_op != op)
    return fail(KM_E_STATE, "counter holds the inputs of %s: it cannot take one of %s", set_name(c->set_op), set_name(op));
  return KM_OK;
}

// The call has passed every check: it is the next input, with or without records.
uint32_t set_begin_input(km_counter* c, int op) {
  c->feed = FEED_SET;
  c->set_op = op;
  return ++c->set_inputs;
}

// n records of kb + cb bytes as input g; fill(dst, piece) writes piece.bytes bytes of them to a pinned buffer.
template <typename Fill>
int set_enqueue(km_counter* c, uint64_t n, uint32_t kb, uint32_t cb, int op, uint32_t g, Fill fill) {
  const uint64_t rec = (uint64_t)kb + cb, per = kmpiece::per_piece(c->stg.bytes, rec);
  HIPCHK(hipSetDevice(c->device));
  const uint64_t pieces = kmpiece::n_pieces(n, per);
  for (uint64_t i = 0; i < pieces; ++i) {
    const kmpiece::Piece p = kmpiece::piece(n, per, rec, i);
    KMCHK(c->stg.claim());
    KMCHK(fill(c->stg.mine, p));
    if (g == 1) KMCHK(counter_reserve(c, p.records));   // only input 1 claims slots
    KMCHK(c->stg.ship(c->d_text, p.bytes, c->st));
    KMCHK(c->merge_spans.open(c->st));
    hipLaunchKernelGGL(k_set_records, dim3(grid_for(p.records, 256)), dim3(256), 0, c->st, c->d_text.p, p.records, kb, cb,
                       op, g, c->table.p, c->slots - 1, c->meta.p);
    HIPCHK(hipGetLastError());
    KMCHK(c->merge_spans.close(c->st));
  }
  return KM_OK;
}
}  // namespace

extern "C" int km_counter_set_records(km_counter_t* c, const uint64_t* keys, const uint32_t* counts, uint64_t n, int op) {
  if (!c || (n && (!keys || !counts))) return fail(KM_E_ARG, "null argument");
  KMCHK(set_check(c, op));
  const uint32_t g = set_begin_input(c, op);
  if (n == 0) return KM_OK;
  return set_enqueue(c, n, (uint32_t)kmpiece::PACKED_KEY_BYTES, (uint32_t)kmpiece::PACKED_COUNT_BYTES, op, g,
                     [&](unsigned char* dst, const kmpiece::Piece& p) {
                       kmpiece::pack(keys, counts, p.first, p.records, dst);
                       return KM_OK;
                     });
}

extern "C" int km_counter_set_jf(km_counter_t* c, const char* path, int op, uint64_t* n_records) {
  if (!c || !path) return fail(KM_E_ARG, "null argument");
  KMCHK(set_check(c, op));
  RecordFile file;
  KMCHK(file.open(path));
  const jfio::Layout& lay = file.lay;
  if (lay.k != c->k || lay.canonical != c->canonical)
    return fail(KM_E_ARG, "%s holds k=%d canonical=%d, the counter k=%d canonical=%d", path, lay.k, lay.canonical, c->k,
                c->canonical);
  if (n_records) *n_records = lay.n_records;
  const uint32_t g = set_begin_input(c, op);
  if (lay.n_records == 0) return KM_OK;
  return set_enqueue(c, lay.n_records, lay.key_bytes, lay.counter_bytes, op, g,
                     [&](unsigned char* dst, const kmpiece::Piece& p) { return file.read(p, dst); });
}

extern "C" int km_counter_finish_range(km_counter_t* c, uint32_t lower_count, uint32_t upper_count, kmjf_t** out) {
  if (!c || !out) return fail(KM_E_ARG, "null argument");
  return counter_finish_cut(c, lower_count, upper_count, true, out, "km_counter_finish_range");
}
