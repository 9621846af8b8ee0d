// merge_host.h — km_jf_file_info, km_counter_add_records, km_counter_add_jf, km_counter_merge_stats (host part of
// kmgpu.hip; device side: merge_kernel.h; the piece arithmetic: merge_pieces.h; a file's records: db_host.h)
// ------------------------------------------------------------------ records of existing tables into a counter
// A record area, of a file or packed from host arrays, goes through the counter's Staging (host_common.h) into d_text
// in pieces of whole records (the staging size rounded down to a multiple of the record size), each followed by
// k_count_add_records on the counter's stream: copy, event, kernel.  The host fills the next piece while the last
// one runs; nothing waits except counter_reserve when it has to read the occupancy.
namespace {
// What every add_* checks first, in their order.
int merge_check(const km_counter* c, int mode) {
  if (mode != KM_MERGE_SUM && mode != KM_MERGE_MAX) return fail(KM_E_ARG, "mode %d is neither KM_MERGE_SUM nor KM_MERGE_MAX", mode);
  KMCHK(counter_takes_plain(c));
  return counter_takes_records(c);
}

// n records of kb + cb bytes; fill(dst, piece) writes piece.bytes bytes of them to a pinned buffer.
template <typename Fill>
int merge_enqueue(km_counter* c, uint64_t n, uint32_t kb, uint32_t cb, int mode, Fill fill) {
  const uint64_t rec = (uint64_t)kb + cb, per = kmpiece::per_piece(c->stg.bytes, rec);
  HIPCHK(hipSetDevice(c->device));
  KMCHK(counter_begin_pieces(c));
  c->feed = FEED_PLAIN;
  const uint64_t pieces = kmpiece::n_pieces(n, per);
  for (uint64_t i = 0; i < pieces; ++i) {
    const kmpiece::Piece p = kmpiece::piece(n, per, rec, i);
    KMCHK(c->stg.claim());
    KMCHK(fill(c->stg.mine, p));
    KMCHK(counter_reserve(c, p.records));               // every record a new key: the insert never meets a full table
    KMCHK(c->stg.ship(c->d_text, p.bytes, c->st));
    KMCHK(c->merge_spans.open(c->st));
    hipLaunchKernelGGL(k_count_add_records, dim3(grid_for(p.records, 256)), dim3(256), 0, c->st, c->d_text.p, p.records,
                       kb, cb, mode, c->table.p, c->slots - 1, c->meta.p);
    HIPCHK(hipGetLastError());
    KMCHK(c->merge_spans.close(c->st));
  }
  return KM_OK;
}
}  // namespace

extern "C" int km_jf_file_info(const char* path, int32_t* k, int32_t* canonical, uint64_t* n_records, int32_t* key_bytes,
                               int32_t* counter_len) {
  if (!path) return fail(KM_E_ARG, "null argument");
  RecordFile file;
  KMCHK(file.open(path));
  const jfio::Layout& lay = file.lay;
  if (k) *k = lay.k;
  if (canonical) *canonical = lay.canonical;
  if (n_records) *n_records = lay.n_records;
  if (key_bytes) *key_bytes = (int32_t)lay.key_bytes;
  if (counter_len) *counter_len = (int32_t)lay.counter_bytes;
  return KM_OK;
}

extern "C" int km_counter_add_records(km_counter_t* c, const uint64_t* keys, const uint32_t* counts, uint64_t n, int mode) {
  if (!c || (n && (!keys || !counts))) return fail(KM_E_ARG, "null argument");
  KMCHK(merge_check(c, mode));
  if (n == 0) return KM_OK;
  return merge_enqueue(c, n, (uint32_t)kmpiece::PACKED_KEY_BYTES, (uint32_t)kmpiece::PACKED_COUNT_BYTES, mode,
                       [&](unsigned char* dst, const kmpiece::Piece& p) {
                         kmpiece::pack(keys, counts, p.first, p.records, dst);
                         return KM_OK;
                       });
}

extern "C" int km_counter_add_jf(km_counter_t* c, const char* path, int mode, uint64_t* n_records) {
  if (!c || !path) return fail(KM_E_ARG, "null argument");
  KMCHK(merge_check(c, mode));
  RecordFile file;
  KMCHK(file.open(path));
  const jfio::Layout& lay = file.lay;
  if (lay.k != c->k || lay.canonical != c->canonical)
    return fail(KM_E_ARG, "%s holds k=%d canonical=%d, the counter k=%d canonical=%d", path, lay.k, lay.canonical, c->k,
                c->canonical);
  if (n_records) *n_records = lay.n_records;
  if (lay.n_records == 0) return KM_OK;
  return merge_enqueue(c, lay.n_records, lay.key_bytes, lay.counter_bytes, mode,
                       [&](unsigned char* dst, const kmpiece::Piece& p) { return file.read(p, dst); });
}

extern "C" int km_counter_merge_stats(km_counter_t* c, uint64_t* records_in, float* kernel_ms) {
  if (!c) return fail(KM_E_ARG, "null argument");
  if (c->fq_error != FQ_NO_ERROR) return counter_format_failed(c);
  HIPCHK(hipSetDevice(c->device));
  unsigned long long m[CM_WORDS];
  KMCHK(counter_read_meta(c, m));
  float ms = 0.f;
  KMCHK(c->merge_spans.drain(&ms));
  if (records_in) *records_in = m[CM_RECORDS];
  if (kernel_ms) *kernel_ms = ms;
  return KM_OK;
}
