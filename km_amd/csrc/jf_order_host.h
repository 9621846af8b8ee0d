// jf_order_host.h — km_jf_*, km_counter_write_jf (host part of kmgpu.hip; device side: jf_order_kernel.h)
// ------------------------------------------------------------------ files in Jellyfish's own record order
// A `binary/sorted` file of real Jellyfish is ordered by pos = M · key over GF(2) (M: the header's matrix1, r rows,
// c = 2k columns), ties by key, and is binary-searched in that order (DESIGN.md §10 "File, Jellyfish order").
// The records are sorted on the device: positions and a histogram of their top bits (k_jf_position), an exclusive
// scan (the k_scan_* kernels of the table build), a scatter into buckets of about 1 K records and one block per
// bucket that sorts in LDS and writes the finished file records.
namespace {
thread_local uint64_t g_jf_stats[4] = {0, 0, 0, 0};
thread_local float g_jf_kernel_ms = 0.f;

uint64_t jf_mix(uint64_t x) {                       // splitmix64's output function
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// rank over GF(2) of the c column vectors (r bits each): the matrix has full row rank iff it is r
int jf_rank(const uint64_t* columns, int c) {
  uint64_t basis[64] = {0};                         // basis[b]: a vector whose highest set bit is b
  int rank = 0;
  for (int i = 0; i < c; ++i) {
    uint64_t v = columns[i];
    while (v) {
      const int b = 63 - __builtin_clzll(v);
      if (!basis[b]) { basis[b] = v; ++rank; break; }
      v ^= basis[b];
    }
  }
  return rank;
}

int jf_check_shape(int k, int size_log2) {
  if (k < 2 || k > 32) return fail(KM_E_K, "k=%d unsupported", k);
  if (size_log2 < 1 || size_log2 > 2 * k) return fail(KM_E_ARG, "size_log2=%d outside 1..%d", size_log2, 2 * k);
  return KM_OK;
}

// (device current)  d_keys / d_counts [n] are only read; records receives n * (ceil(2k/8) + 4) bytes, d_pos_out
// (or null) the n positions in output order.  Waits for the kernels: the bucket figures are read back.
int jf_sort_device(const uint64_t* columns, int k, int size_log2, const uint64_t* d_keys, const uint32_t* d_counts,
                   uint64_t n, uint8_t* d_records, uint64_t* d_pos_out, hipStream_t st) {
  const int c = 2 * k, r = size_log2;
  const uint64_t mask = r >= 64 ? ~0ull : (1ull << r) - 1;
  int bits = 0;
  while ((n >> bits) > 1024 && bits < r && bits < 30) ++bits;
  const int shift = r - bits;
  const uint32_t n_buckets = 1u << bits;
  const uint32_t n_chunks = (uint32_t)(((uint64_t)n_buckets + 1 + SCAN_CHUNK - 1) / SCAN_CHUNK);
  const uint64_t dir_words = (uint64_t)n_chunks * SCAN_CHUNK;
  DevBuf<uint64_t> d_cols, pos, pos2, keys2;
  DevBuf<uint32_t> counts2, dir, cursor, sums;
  DevBuf<unsigned long long> d_stats;
  KMCHK(d_cols.alloc(c));
  KMCHK(pos.alloc(n));
  KMCHK(pos2.alloc(n));
  KMCHK(keys2.alloc(n));
  KMCHK(counts2.alloc(n));
  KMCHK(dir.alloc(dir_words));
  KMCHK(cursor.alloc(n_buckets));
  KMCHK(sums.alloc(n_chunks));
  KMCHK(d_stats.alloc(2));
  KernelSpans span;
  span.timed = true;
  HIPCHK(hipMemcpyAsync(d_cols, columns, (size_t)c * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(dir, 0, dir_words * 4, st));
  HIPCHK(hipMemsetAsync(cursor, 0, (uint64_t)n_buckets * 4, st));
  HIPCHK(hipMemsetAsync(d_stats, 0, 16, st));
  KMCHK(span.open(st));
  const int grid = grid_for(n, JF_THREADS);
  hipLaunchKernelGGL(k_jf_position, dim3(grid), dim3(JF_THREADS), 0, st, d_cols.p, c, mask, d_keys, n, pos.p, dir.p,
                     shift, bits);
  scan_in_place(dir.p, sums.p, n_chunks, st);
  hipLaunchKernelGGL(k_jf_bucket_stats, dim3(grid_for(n_buckets, 256)), dim3(256), 0, st, dir.p, n_buckets, d_stats.p);
  hipLaunchKernelGGL(k_jf_scatter, dim3(grid), dim3(JF_THREADS), 0, st, pos.p, d_keys, d_counts, n, dir.p, cursor.p,
                     shift, bits, pos2.p, keys2.p, counts2.p);
  hipLaunchKernelGGL(k_jf_sort_buckets, dim3(std::min<uint32_t>(n_buckets, 1u << 20)), dim3(JF_THREADS), 0, st, dir.p,
                     n_buckets, pos2.p, keys2.p, counts2.p, (uint32_t)((c + 7) / 8), d_records, d_pos_out);
  HIPCHK(hipGetLastError());
  KMCHK(span.close(st));
  unsigned long long stats[2];
  HIPCHK(hipMemcpyAsync(stats, d_stats, 16, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  KMCHK(span.drain(&g_jf_kernel_ms));
  g_jf_stats[0] = n_buckets;
  g_jf_stats[1] = stats[0];
  g_jf_stats[2] = stats[1];
  g_jf_stats[3] = 0;
  return KM_OK;
}

void jf_put(std::string& s, const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  s += buf;
}

// The whole file header (length prefix, JSON with sorted keys, padding to 8), the matrix and the size it names.
// The keys are those of a header written by Jellyfish 2.2.3 minus hostname / pwd / time / exe_path, so the same
// records give the same file; max_reprobe, reprobes and val_len carry that header's values.
int jf_make_header(int k, int canonical, uint64_t n, uint64_t seed, const char* cmdline_json, std::string* out,
                   uint64_t* columns, int* size_log2) {
  if (cmdline_json) {                               // pasted as it is: its brackets at least
    const size_t len = strlen(cmdline_json);
    if (len < 2 || cmdline_json[0] != '[' || cmdline_json[len - 1] != ']')
      return fail(KM_E_ARG, "cmdline_json is not a JSON array");
  }
  int s = 4;
  while (s < 2 * k && s < 63 && (1ull << s) < 2 * n) ++s;
  s = std::min(s, 2 * k);
  KMCHK(km_jf_matrix(k, s, seed, columns));
  std::string j = "{\"alignment\":8,\"canonical\":";
  j += canonical ? "true" : "false";
  j += ",\"cmdline\":";
  j += cmdline_json ? cmdline_json : "[\"km_amd\",\"count\"]";
  jf_put(j, ",\"counter_len\":4,\"format\":\"binary/sorted\",\"key_len\":%d,\"matrix1\":{\"c\":%d,\"columns\":[", 2 * k, 2 * k);
  for (int i = 0; i < 2 * k; ++i) jf_put(j, i ? ",%llu" : "%llu", (unsigned long long)columns[i]);
  jf_put(j, "],\"r\":%d},\"max_reprobe\":126,\"reprobes\":[1", s);
  for (int i = 1; i <= 126; ++i) jf_put(j, ",%d", i * (i + 1) / 2);
  jf_put(j, "],\"size\":%llu,\"val_len\":12}", 1ull << s);
  j.append((8 - (9 + j.size()) % 8) % 8, '\0');
  char len[16];
  snprintf(len, sizeof len, "%09llu", (unsigned long long)j.size());
  *out = len + j;
  *size_log2 = s;
  return KM_OK;
}
}  // namespace

extern "C" int km_jf_matrix(int k, int size_log2, uint64_t seed, uint64_t* columns) {
  if (!columns) return fail(KM_E_ARG, "null argument");
  KMCHK(jf_check_shape(k, size_log2));
  const int c = 2 * k, r = size_log2;
  const uint64_t mask = r >= 64 ? ~0ull : (1ull << r) - 1;
  for (uint64_t attempt = 0;; ++attempt) {            // (a random r x c matrix, c >= r, has full rank with p > 0.28)
    for (int i = 0; i < c; ++i)
      columns[i] = jf_mix(jf_mix(seed + 0x9E3779B97F4A7C15ull * (attempt + 1)) + 0x9E3779B97F4A7C15ull * (uint64_t)(i + 1)) & mask;
    if (jf_rank(columns, c) == r) return KM_OK;
  }
}

extern "C" int km_jf_header(int k, int canonical, uint64_t n, uint64_t seed, const char* cmdline_json, char* out,
                            uint64_t cap, uint64_t* len, uint64_t* columns, int* size_log2) {
  if (!len || !columns || !size_log2) return fail(KM_E_ARG, "null argument");
  if (k < 2 || k > 32) return fail(KM_E_K, "k=%d unsupported", k);
  std::string h;
  KMCHK(jf_make_header(k, canonical, n, seed, cmdline_json, &h, columns, size_log2));
  *len = h.size();
  if (!out) return KM_OK;
  if (cap < h.size()) return fail(KM_E_CAPACITY, "header of %llu bytes, room for %llu", (unsigned long long)h.size(),
                                  (unsigned long long)cap);
  memcpy(out, h.data(), h.size());
  return KM_OK;
}

extern "C" int km_jf_sort_stats(uint64_t* out4) {
  if (!out4) return fail(KM_E_ARG, "null argument");
  memcpy(out4, g_jf_stats, sizeof g_jf_stats);
  return KM_OK;
}

extern "C" int km_jf_sort_kernel_ms(float* ms) {
  if (!ms) return fail(KM_E_ARG, "null argument");
  *ms = g_jf_kernel_ms;
  return KM_OK;
}

extern "C" int km_jf_sort_records(int device, const uint64_t* columns, int k, int size_log2, const uint64_t* keys,
                                  const uint32_t* counts, uint64_t n, uint8_t* records, uint64_t* pos_or_null,
                                  void* stream) {
  if (!columns || (n && (!keys || !counts || !records))) return fail(KM_E_ARG, "null argument");
  KMCHK(jf_check_shape(k, size_log2));
  if (device < 0) return fail(KM_E_ARG, "device %d", device);
  if (n >> 32) return fail(KM_E_ARG, "%llu records: the bucket directory is 32-bit", (unsigned long long)n);
  memset(g_jf_stats, 0, sizeof g_jf_stats);
  g_jf_kernel_ms = 0.f;
  if (n == 0) return KM_OK;
  CallStream st;
  KMCHK(st.get(device, stream));
  const uint64_t rec = (uint64_t)(2 * k + 7) / 8 + 4;
  DevBuf<uint64_t> d_keys, d_pos;
  DevBuf<uint32_t> d_counts;
  DevBuf<uint8_t> d_records;
  KMCHK(d_keys.alloc(n));
  KMCHK(d_counts.alloc(n));
  KMCHK(d_records.alloc(n * rec));
  if (pos_or_null) KMCHK(d_pos.alloc(n));
  HIPCHK(hipMemcpyAsync(d_keys, keys, n * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_counts, counts, n * 4, hipMemcpyHostToDevice, st));
  KMCHK(jf_sort_device(columns, k, size_log2, d_keys, d_counts, n, d_records, pos_or_null ? d_pos.p : nullptr, st));
  HIPCHK(hipMemcpyAsync(records, d_records, n * rec, hipMemcpyDeviceToHost, st));
  if (pos_or_null) HIPCHK(hipMemcpyAsync(pos_or_null, d_pos, n * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return KM_OK;
}

// The sorted records leave the device through the counter's Staging (fetch and wait: host_common.h), which is idle
// once the counter has finished: the copy of one piece runs while the piece before it is written to the file.
extern "C" int km_counter_write_jf(km_counter_t* c, const char* path, const char* cmdline_json, uint64_t seed) {
  if (!c || !path) return fail(KM_E_ARG, "null argument");
  KMCHK(counter_holds_counts(c, "km_counter_write_jf"));
  if (!c->finished) return fail(KM_E_STATE, "km_counter_finish comes first");
  const uint64_t n = c->n_out;
  if (n >> 32) return fail(KM_E_ARG, "%llu records: the bucket directory is 32-bit", (unsigned long long)n);
  memset(g_jf_stats, 0, sizeof g_jf_stats);
  g_jf_kernel_ms = 0.f;
  std::string header;
  uint64_t columns[64];
  int size_log2 = 0;
  KMCHK(jf_make_header(c->k, c->canonical, n, seed, cmdline_json, &header, columns, &size_log2));
  const uint64_t total = n * ((uint64_t)(2 * c->k + 7) / 8 + 4);
  File f(fopen(path, "wb"));                          // before the sort: a path that cannot be had costs nothing
  if (!f) return fail(KM_E_IO, "cannot create %s: %s", path, strerror(errno));
  struct Partial {                                    // whatever ends the call early takes the partial file along
    const char* path; bool keep;
    ~Partial() { if (!keep) (void)remove(path); }
  } partial{path, false};
  DevBuf<uint8_t> d_records;
  if (n) {
    HIPCHK(hipSetDevice(c->device));
    KMCHK(d_records.alloc(total));
    KMCHK(jf_sort_device(columns, c->k, size_log2, c->out_keys, c->out_counts, n, d_records, nullptr, c->st));
  }
  int io_errno = 0;                                   // errno of the first write that failed
  auto put = [&](const void* p, uint64_t len) {
    if (fwrite(p, 1, len, f) == len) return true;
    io_errno = errno;
    return false;
  };
  bool ok = put(header.data(), header.size());
  Staging& s = c->stg;
  const uint64_t piece = s.bytes;
  auto fetch = [&](uint64_t at, int buf) { return s.fetch(buf, d_records.p + at, std::min(piece, total - at), c->st); };
  int cur = 0;
  if (total) KMCHK(fetch(0, 0));
  for (uint64_t at = 0; at < total && ok; at += piece, cur ^= 1) {
    if (at + piece < total) KMCHK(fetch(at + piece, cur ^ 1));
    unsigned char* got = nullptr;
    KMCHK(s.wait(cur, &got));
    ok = put(got, std::min(piece, total - at));
  }
  if (total) HIPCHK(hipStreamSynchronize(c->st));
  if (fclose(f.take()) != 0 && ok) {
    io_errno = errno;
    ok = false;
  }
  if (!ok) return fail(KM_E_IO, "writing %s failed: %s", path, strerror(io_errno));
  partial.keep = true;
  return KM_OK;
}
