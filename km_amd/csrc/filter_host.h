// filter_host.h — km_counter_set_filter, km_counter_filter_stats (host part of kmgpu.hip; device side: filter_kernel.h;
// where a filtered counter differs on its way through count_host.h: its CountMode in launch_insert, counter_table_fixed
// in counter_flush and fastq_enqueue)
// ------------------------------------------------------------------ counting only a given set of k-mers
// The filter replaces the counter's table by one that holds exactly the filter's keys, each with count 0, at the
// smallest power of two >= max(64, 2 * distinct) slots.  How many keys are distinct is known only once the device has
// canonicalised and claimed them, so they are seeded into a table sized for n distinct keys first and, when fewer
// were, rehashed into the smaller one (k_count_rehash: keys and their counts of 0).  Nothing claims a slot afterwards:
// counter_reserve never runs for such a counter, and slots / n_grow stay what they are here.
namespace {
uint64_t filter_slots_for(uint64_t distinct) {
  uint64_t s = 64;
  while (s < 2 * distinct) s <<= 1;
  return s;
}

// The most blocks of a bounded grid (km_counter::grid_cap): KM_COUNT_FILTER_BLOCKS, or what fills the device.  The LDS
// tier's 64 KiB let two blocks share a CU's 160 KiB; the HBM tier's blocks, and those of a sketch's noting pass, are
// bounded by their waves alone (eight of four waves each).
int filter_grid_cap(int device, CountMode mode, uint32_t* blocks) {
  if (const char* e = getenv("KM_COUNT_FILTER_BLOCKS")) {
    const unsigned long long v = strtoull(e, nullptr, 10);
    if (v) { *blocks = (uint32_t)std::min<unsigned long long>(v, 1u << 20); return KM_OK; }
  }
  int cus = 0;
  HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
  *blocks = (uint32_t)std::max(cus, 1) * (mode == COUNT_FILTER_LDS ? 2u : 8u);
  return KM_OK;
}
}  // namespace

extern "C" int km_counter_set_filter(km_counter_t* c, const uint64_t* keys, uint64_t n) {
  if (!c || (n && !keys)) return fail(KM_E_ARG, "null argument");
  KMCHK(counter_usable(c));
  if (counter_has_filter(c)) return fail(KM_E_STATE, "counter already has a filter");
  if (counter_has_sketch(c)) return fail(KM_E_STATE, "counter has a sketch: it takes no filter");
  if (c->feed != FEED_NONE) return fail(KM_E_STATE, "counter has been fed: the filter comes before the first add_* or set_* call");
  if (n >> 60) return fail(KM_E_ARG, "%llu filter keys: too many", (unsigned long long)n);
  if (c->k < 32)
    for (uint64_t i = 0; i < n; ++i)
      if (keys[i] >> (2 * c->k))
        return fail(KM_E_ARG, "filter key %llu (0x%llx) is no k-mer of k=%d", (unsigned long long)i,
                    (unsigned long long)keys[i], c->k);
  HIPCHK(hipSetDevice(c->device));
  DevBuf<uint64_t> d_keys;
  DevBuf<CountSlot> seeded;
  const uint64_t wide = filter_slots_for(n);
  KMCHK(d_keys.alloc(n));
  KMCHK(seeded.alloc(wide));
  if (n) HIPCHK(hipMemcpyAsync(d_keys.p, keys, n * 8, hipMemcpyHostToDevice, c->st));
  hipLaunchKernelGGL(k_count_init, dim3(grid_for(wide, 256)), dim3(256), 0, c->st, seeded.p, wide);
  if (n)
    hipLaunchKernelGGL(k_filter_seed, dim3(grid_for(n, 256)), dim3(256), 0, c->st, d_keys.p, n, c->k, c->canonical,
                       seeded.p, wide - 1, c->meta.p);
  HIPCHK(hipGetLastError());
  unsigned long long m[CM_WORDS];
  KMCHK(counter_read_meta(c, m));                       // (waits: d_keys and `keys` are done with)
  const uint64_t slots = filter_slots_for(c->last.distinct);
  if (slots != wide) {
    DevBuf<CountSlot> tight;
    KMCHK(tight.alloc(slots));
    hipLaunchKernelGGL(k_count_init, dim3(grid_for(slots, 256)), dim3(256), 0, c->st, tight.p, slots);
    hipLaunchKernelGGL(k_count_rehash, dim3(grid_for(wide, 256)), dim3(256), 0, c->st, seeded.p, wide, tight.p, slots - 1,
                       c->meta.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->st));
    seeded = std::move(tight);
  }
  CountMode mode = slots <= FILTER_LDS_SLOTS ? COUNT_FILTER_LDS : COUNT_FILTER_HBM;
  if (const char* e = getenv("KM_COUNT_FILTER_LDS"))
    if (atoi(e) == 0) mode = COUNT_FILTER_HBM;
  KMCHK(filter_grid_cap(c->device, mode, &c->grid_cap));
  c->table = std::move(seeded);
  c->slots = slots;
  c->occ_ub = m[CM_DISTINCT];
  c->last.slots = slots;
  c->mode = mode;
  return KM_OK;
}

extern "C" int km_counter_filter_stats(km_counter_t* c, uint64_t* n_keys, uint64_t* kmers_hit, int* tier,
                                       uint64_t* lds_keys, float* kernel_ms) {
  if (!c) return fail(KM_E_ARG, "null argument");
  if (c->fq_error != FQ_NO_ERROR) return counter_format_failed(c);
  HIPCHK(hipSetDevice(c->device));
  if (!c->finished) KMCHK(counter_flush(c));
  unsigned long long m[CM_WORDS];
  KMCHK(counter_read_meta(c, m));
  float ms = 0.f;
  KMCHK(c->insert_spans.drain(&ms));
  if (n_keys) *n_keys = counter_has_filter(c) ? c->last.distinct : 0;
  if (kmers_hit) *kmers_hit = m[CM_HITS];
  if (tier) *tier = c->mode == COUNT_FILTER_LDS ? 1 : c->mode == COUNT_FILTER_HBM ? 2 : 0;
  if (lds_keys) *lds_keys = FILTER_LDS_SLOTS / 2;
  if (kernel_ms) *kernel_ms = ms;
  return KM_OK;
}
