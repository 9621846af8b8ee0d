// db_host.h — the database: kmjf_* open / upload / broadcast / load and the lookups; RecordFile, the one reader of a
// file's record area (host part of kmgpu.hip; device side: table_kernels.h)
#include <dlfcn.h>
#include <rccl/rccl.h>

// ------------------------------------------------------------------------ database
struct kmjf {
  int k = 0;
  int canonical = 0;
  std::vector<uint64_t> keys;
  std::vector<uint32_t> counts;
  uint64_t n_records = 0;
  // device table
  int device = -1;
  DevBuf<Slot> d_slots;
  uint64_t n_slots = 0;
  DevBuf<uint32_t> d_dir;        // [n_buckets + 1] (+ padding) exclusive prefix of bucket sizes
  uint32_t n_buckets = 0;
  uint32_t unit = 2;
  uint32_t max_probe = 2;
  DevBuf<OvfSlot> d_ovf;
  uint64_t n_ovf = 0;
  uint64_t n_groups = 0;

  ~kmjf() { free_table(); }
  void free_table() {
    if (d_slots) {
      (void)hipSetDevice(device);
      d_slots.release();
      d_ovf.release();
      d_dir.release();
    }
    n_slots = n_groups = n_ovf = 0;
    n_buckets = 0;
    device = -1;
  }
};

static uint64_t mask_bits(int nbases) { return nbases >= 32 ? ~0ull : ((1ull << (2 * nbases)) - 1); }

// A table's geometry over its directory: what the build kernels see before there are slots
static TableView table_shape(int k, int canonical, uint32_t n_buckets, uint32_t unit, const uint32_t* dir) {
  TableView t;
  t.slots = nullptr;
  t.dir = dir;
  t.n_slots = 0;
  t.ovf = nullptr;
  t.n_ovf = 0;
  t.kmask = mask_bits(k);
  t.pmask = mask_bits(k - 1);
  t.n_buckets = n_buckets;
  t.bshift = 31;                                    // (n_buckets: a power of two, 2^4 .. 2^30; 0 before the build)
  while (t.bshift > 1 && (1ull << (32 - t.bshift)) < n_buckets) --t.bshift;
  t.unit = unit;
  t.max_probe = 2;
  t.k = k;
  t.canonical = canonical;
  t.m = minimizer_len(k);
  t.w = k - t.m;
  t.mmask = (uint32_t)mask_bits(t.m);
  t.inv32 = (uint32_t)((1ull << 32) / ((uint64_t)2 * t.w * 256));
  t.cshift = 1;
  while ((1u << t.cshift) < 2u * (uint32_t)t.w) ++t.cshift;
  return t;
}

static TableView view_of(const kmjf* h) {
  TableView t = table_shape(h->k, h->canonical, h->n_buckets, h->unit, h->d_dir);
  t.slots = h->d_slots;
  t.n_slots = h->n_slots;
  t.ovf = h->d_ovf;
  t.n_ovf = h->n_ovf;
  t.max_probe = h->max_probe;
  return t;
}

// What jfio's readers return, as the library's codes under the reader's own message; then the k this library takes.
static int reader_result(int rc, const std::string& err, int k) {
  if (rc != 0) return fail(rc == 1 ? KM_E_IO : rc == 2 ? KM_E_FORMAT : KM_E_K, "%s", err.c_str());
  if (k < 2 || k > 32) return fail(KM_E_K, "k=%d unsupported", k);
  return KM_OK;
}

// The record area of a file, for the calls that take it in as it is stored, whole or piece by piece.
struct RecordFile {
  jfio::Layout lay;
  File f;                                 // left open by open(), positioned anywhere
  const char* path = nullptr;             // (the caller's, for the messages)
  uint64_t rec = 0;                       // bytes per record
  int open(const char* p) {               // the header of `p` as kmjf_open judges it
    std::string err;
    void* file = nullptr;
    const int rc = jfio::read_layout(path = p, &lay, &file, &err);
    f.h = static_cast<FILE*>(file);
    rec = (uint64_t)lay.key_bytes + lay.counter_bytes;
    return reader_result(rc, err, lay.k);
  }
  int read(const kmpiece::Piece& p, unsigned char* dst) const {   // the records of piece p into dst[p.bytes]
    const int e = kmpiece::read_exact(fileno(f), dst, p.bytes, lay.body_offset + p.first * rec);
    if (e == 0) return KM_OK;
    return fail(KM_E_IO, "reading the records of %s failed: %s", path, e < 0 ? "the file ends early" : strerror(e));
  }
};

extern "C" int kmjf_open(const char* path, kmjf_t** out) {
  if (!path || !out) return fail(KM_E_ARG, "null argument");
  jfio::Records rec;
  std::string err;
  const int rc = jfio::read_file(path, &rec, &err);
  KMCHK(reader_result(rc, err, rec.k));
  kmjf* h = new (std::nothrow) kmjf;
  if (!h) return fail(KM_E_NOMEM, "host allocation failed");
  h->k = rec.k;
  h->canonical = rec.canonical;
  h->keys.swap(rec.keys);
  h->counts.swap(rec.counts);
  h->n_records = h->keys.size();
  *out = h;
  return KM_OK;
}

extern "C" int kmjf_from_records(const uint64_t* keys, const uint32_t* counts, uint64_t n, int k,
                                 int canonical, kmjf_t** out) {
  if (!out || (n && (!keys || !counts))) return fail(KM_E_ARG, "null argument");
  if (k < 2 || k > 32) return fail(KM_E_K, "k=%d unsupported", k);
  kmjf* h = new (std::nothrow) kmjf;
  if (!h) return fail(KM_E_NOMEM, "host allocation failed");
  h->k = k;
  h->canonical = canonical ? 1 : 0;
  try {
    h->keys.assign(keys, keys + n);
    h->counts.assign(counts, counts + n);
  } catch (...) {
    delete h;
    return fail(KM_E_NOMEM, "host allocation failed");
  }
  h->n_records = n;
  *out = h;
  return KM_OK;
}

extern "C" int kmjf_create(int k, int canonical, kmjf_t** out) {
  return kmjf_from_records(nullptr, nullptr, 0, k, canonical, out);
}

extern "C" int kmjf_close(kmjf_t* h) {
  delete h;
  return KM_OK;
}

extern "C" int kmjf_info(const kmjf_t* h, kmjf_info_t* info) {
  if (!h || !info) return fail(KM_E_ARG, "null argument");
  info->k = h->k;
  info->canonical = h->canonical;
  info->n_records = h->n_records;
  info->n_slots = h->n_slots;
  info->n_groups = h->n_groups;
  info->table_bytes = h->n_slots * sizeof(Slot) + h->n_ovf * sizeof(OvfSlot) +
                      (h->d_dir ? ((uint64_t)h->n_buckets + 1) * 4 : 0);
  info->device = h->device;
  info->max_probe = h->d_slots ? (int32_t)h->max_probe : 0;
  return KM_OK;
}

extern "C" int kmjf_records(const kmjf_t* h, const uint64_t** keys, const uint32_t** counts,
                            uint64_t* n) {
  if (!h || !keys || !counts || !n) return fail(KM_E_ARG, "null argument");
  *keys = h->keys.data();
  *counts = h->counts.data();
  *n = h->keys.size();
  return KM_OK;
}

// Build, all on the device from device-resident records: count the entries of every minimizer
// bucket -> capacities -> exclusive scan (= the directory) -> insert every key into its home
// pair.  Buckets where some key found its pair taken are doubled and the table is rebuilt
// (a handful of rounds); the result is a table in which every lookup reads exactly one
// aligned 32-byte pair.
extern "C" int kmjf_upload_from_device(kmjf_t* h, int device, const uint64_t* d_keys,
                                       const uint32_t* d_counts, uint64_t n, void* stream) {
  if (!h || (n && (!d_keys || !d_counts))) return fail(KM_E_ARG, "null argument");
  hipStream_t st = (hipStream_t)stream;
  h->free_table();
  HIPCHK(hipSetDevice(device));
  // every record enters at most two groups
  const uint64_t max_entries = (h->canonical ? 2 : 1) * n;
  if (max_entries >= (1ull << 31)) return fail(KM_E_CAPACITY, "more than 2^31 table entries");
  // the build's environment, read once per call.  (KM_TABLE_LEAN_CROWDED=0: round 3's rule, a second doubling
  // before a bucket becomes a two-choice table)
  const bool verbose = getenv("KM_BUILD_VERBOSE") != nullptr;
  const bool settle = getenv("KM_TABLE_NO_SETTLE") == nullptr;
  const char* lean_env = getenv("KM_TABLE_LEAN_CROWDED");
  const int lean_crowded = lean_env ? atoi(lean_env) : 1;
  // KM_TABLE_LOAD: initial load factor of every bucket (HBM capacity is plentiful): unit = 1/load
  uint32_t unit = 2;
  if (const char* lf = getenv("KM_TABLE_LOAD")) {
    double v = atof(lf);
    if (v >= 0.05 && v <= 0.5) unit = (uint32_t)(1.0 / v + 0.5);
  }
  // KM_DIR_LOG2: log2 of the bucket count (default: about one bucket per 2 entries; a
  // super-k-mer brings ~w entries of its own, so most buckets of real data are empty)
  uint32_t n_buckets = 1024;
  // (at most 1.5 entries per bucket: with 1.9 — a 500 M-k-mer sample under the old rule of 2 — half as many more buckets
  // double and the table takes 144 B per k-mer instead of ~105)
  while ((uint64_t)n_buckets * 3 < max_entries * 2 && n_buckets < (1u << 30)) n_buckets <<= 1;
  if (const char* dl = getenv("KM_DIR_LOG2")) { int v = atoi(dl); if (v >= 4 && v <= 30) n_buckets = 1u << v; }
  const uint32_t n_chunks = (uint32_t)(((uint64_t)n_buckets + 1 + SCAN_CHUNK - 1) / SCAN_CHUNK);
  const uint64_t dir_words = (uint64_t)n_chunks * SCAN_CHUNK;
  // the table (dir, slots, ovf) goes to h once built; the rest is build scratch
  DevBuf<uint32_t> dir, caps, sums;
  DevBuf<unsigned long long> d_meta;   // [0] occupied slots, [1] error, [2] flagged buckets, [3] max probe distance,
                                       // [4] big counts, [5] total capacity (pairs)
  DevBuf<Slot> slots;
  DevBuf<OvfSlot> ovf;
  DevBuf<uint32_t> settle_bits;         // one bit per bucket: on the list below
  DevBuf<uint32_t> settle_list;         // buckets holding a key outside its home pair (k_table_settle)
  const uint32_t SETTLE_CAP = 1u << 22;
  const uint64_t settle_words = ((uint64_t)n_buckets + 31) / 32 + 1;
  int rc = dir.alloc(dir_words);
  if (rc == KM_OK) rc = caps.alloc(dir_words);
  if (rc == KM_OK) rc = settle_bits.alloc(settle_words);
  if (rc == KM_OK) rc = settle_list.alloc(SETTLE_CAP);
  if (rc == KM_OK) rc = sums.alloc(n_chunks);
  if (rc == KM_OK) rc = d_meta.alloc(8);
  if (rc != KM_OK) return rc;
  (void)hipMemsetAsync(dir, 0, dir_words * 4, st);
  (void)hipMemsetAsync(caps, 0, dir_words * 4, st);
  (void)hipMemsetAsync(d_meta, 0, 64, st);

  const TableView tv = table_shape(h->k, h->canonical, n_buckets, unit, dir);

  if (n) {
    hipLaunchKernelGGL(k_count_big, dim3(grid_for(n, 256)), dim3(256), 0, st, d_counts, n, d_meta + 4);
    hipLaunchKernelGGL(k_dir_count, dim3(grid_for(n, 256)), dim3(256), 0, st, tv, d_keys, d_counts, n, caps);
  }
  hipLaunchKernelGGL(k_dir_capacity, dim3(grid_for((uint64_t)n_buckets, 256)), dim3(256), 0, st, caps,
                     (uint64_t)n_buckets, unit, tv.cshift);
  const int MAX_ROUNDS = 5;             // CAP_MAX_GEN dry rounds, up to two more doublings found by the real
                                        // insert, then one final round that places every key wherever it fits
  unsigned long long meta[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t n_slots = 0;
  uint32_t max_probe = 2;
  int rounds = 0, dry_rounds = 0;
  DevBuf<uint32_t> ctr;             // dry rounds: entries per home pair, one byte each
  hipError_t e;
  for (;; ++rounds) {
    const int final_round = rounds >= MAX_ROUNDS;
    (void)hipMemsetAsync(d_meta, 0, 32, st);          // [0..3]
    (void)hipMemsetAsync(d_meta + 5, 0, 8, st);
    hipLaunchKernelGGL(k_dir_copy, dim3(grid_for((uint64_t)n_buckets, 256)), dim3(256), 0, st, caps, dir,
                       (uint64_t)n_buckets, d_meta + 5);
    scan_in_place(dir, sums, n_chunks, st);
    e = hipMemcpyAsync(meta, d_meta, 48, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail_hip(KM_E_HIP, "directory pass failed", e);
    if (meta[5] >= (1ull << 32))
      return fail_hip(KM_E_CAPACITY, "table needs more than 2^33 slots (32-bit directory)", hipSuccess);
    n_slots = std::max<uint64_t>(64, 2ull * meta[5]);
    if (n && dry_rounds < (int)CAP_MAX_GEN) {
      // dry round (cheap: one byte per pair instead of the slots): find the buckets to double
      const uint64_t words = meta[5] / 4 + 2;
      if (words > ctr.n) {
        KMCHK(ctr.alloc(words + words / 2));
      }
      (void)hipMemsetAsync(ctr, 0, words * 4, st);
      hipLaunchKernelGGL(k_table_dry, dim3(grid_for(n, 256)), dim3(256), 0, st, tv, d_keys, d_counts, n, caps,
                         ctr, d_meta);
      e = hipMemcpyAsync(meta, d_meta, 32, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      if (e != hipSuccess) return fail_hip(KM_E_HIP, "table build failed", e);
      ++dry_rounds;
      if (verbose)
        fprintf(stderr, "libkmgpu: dry round %d: %llu slots, %llu buckets to grow\n", dry_rounds,
                (unsigned long long)n_slots, meta[2]);
      if (meta[2]) {
        hipLaunchKernelGGL(k_dir_grow, dim3(grid_for((uint64_t)n_buckets, 256)), dim3(256), 0, st, caps,
                           (uint64_t)n_buckets, tv.cshift, lean_crowded);
        continue;
      }
      dry_rounds = (int)CAP_MAX_GEN;               // nothing to grow: go straight to the insert
    }
    if (n_slots + 16 > slots.n) {
      KMCHK(slots.alloc(n_slots + n_slots / 4 + 16));   // head room for the following rounds
    }
    hipLaunchKernelGGL(k_table_init, dim3(grid_for(n_slots, 256)), dim3(256), 0, st, slots, n_slots);
    (void)hipMemsetAsync(settle_bits, 0, settle_words * 4, st);
    (void)hipMemsetAsync(d_meta + 6, 0, 16, st);
    if (n)
      hipLaunchKernelGGL(k_table_insert, dim3(grid_for(n, 256)), dim3(256), 0, st, tv, slots, d_keys,
                         d_counts, n, caps, final_round, d_meta, settle_bits, settle_list, SETTLE_CAP);
    e = hipMemcpyAsync(meta, d_meta, 64, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail_hip(KM_E_HIP, "table build failed", e);
    if (meta[1] & 0xFFFFFFFFull) return fail_hip(KM_E_HIP, "table build overflowed", hipSuccess);
    max_probe = std::max<uint32_t>(2, (uint32_t)meta[3] + 1);
    // ---- settle: the buckets in which the race of the insert decided who sits where are laid out again as a
    // function of their keys alone (k_table_settle); that layout also decides which of them double once more
    if (n && meta[6] && meta[6] <= SETTLE_CAP && settle) {
      const uint32_t n_list = (uint32_t)meta[6];
      const uint32_t lds = 128u << 10;
      // (per device and cheap: set on every build rather than remembered per process)
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_table_settle), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return fail_hip(KM_E_HIP, "table settle pass: 128 KB of dynamic LDS refused", e);
      const uint32_t race_probe = max_probe;
      const unsigned long long n_slots_total = meta[5];
      (void)hipMemsetAsync(d_meta + 3, 0, 8, st);
      (void)hipMemsetAsync(d_meta + 5, 0, 8, st);
      hipLaunchKernelGGL(k_table_settle, dim3(n_list), dim3(256), lds, st, tv, slots, settle_list, n_list, lds, caps,
                         final_round, d_meta);
      // (a rejected launch would leave meta[3] = 0, i.e. max_probe 2 with keys further out: lookups would miss them)
      e = hipGetLastError();
      if (e == hipSuccess) e = hipMemcpyAsync(meta, d_meta, 64, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      if (e != hipSuccess) return fail_hip(KM_E_HIP, "table settle pass failed", e);
      max_probe = std::max<uint32_t>(2, (uint32_t)meta[3] + 1);
      if (verbose)
        fprintf(stderr, "libkmgpu: settle pass: %u buckets laid out again by their keys alone (%llu too large: measured only); "
                "max_probe %u (the race had %u)\n", n_list, meta[5], max_probe, race_probe);
      meta[5] = n_slots_total;
    }
    if (verbose)
      fprintf(stderr, "libkmgpu: build round %d: %llu slots, %llu buckets to grow, max distance %llu; %llu buckets (%llu slots) hold a key outside its home pair\n", rounds,
              (unsigned long long)n_slots, meta[2], meta[3], meta[6], meta[7]);
    if (final_round) break;
    if (meta[2] == 0) break;
    hipLaunchKernelGGL(k_dir_grow, dim3(grid_for((uint64_t)n_buckets, 256)), dim3(256), 0, st, caps,
                       (uint64_t)n_buckets, tv.cshift, lean_crowded);
  }
  // the buckets the last insert did not list for k_table_settle: which of two groups took the first slot of their home
  // pair is all the race decided there; tag order takes that out as well (settle_bits: as that insert left them)
  if (n) {
    TableView tv_slots = tv;
    tv_slots.slots = slots;
    hipLaunchKernelGGL(k_table_order_pairs, dim3(grid_for((uint64_t)n_buckets, 256)), dim3(256), 0, st, tv_slots, slots,
                       settle_bits);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail_hip(KM_E_HIP, "table order pass failed", e);
  }
  if (verbose)
    fprintf(stderr, "libkmgpu: table built in %d round(s): %llu slots for %llu groups, max_probe %u\n",
            rounds + 1, (unsigned long long)n_slots, meta[0], max_probe);
  // side table for the (rare) counts that do not fit 16 bits
  const uint64_t n_big = meta[4];
  const uint64_t n_ovf = n_big ? (n_big * 2 + 64) : 0;
  if (n_ovf) {
    KMCHK(ovf.alloc(n_ovf));
    (void)hipMemsetAsync(ovf, 0, n_ovf * sizeof(OvfSlot), st);
    (void)hipMemsetAsync(d_meta + 1, 0, 8, st);
    hipLaunchKernelGGL(k_ovf_insert, dim3(grid_for(n, 256)), dim3(256), 0, st, d_keys, d_counts, n, h->k,
                       h->canonical, ovf, n_ovf, reinterpret_cast<unsigned int*>(d_meta + 1));
    unsigned long long err = 0;
    e = hipMemcpyAsync(&err, d_meta + 1, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail_hip(KM_E_HIP, "side table build failed", e);
    if (err & 0xFFFFFFFFull) return fail_hip(KM_E_HIP, "side table overflowed", hipSuccess);
  }
  h->d_slots = std::move(slots);
  h->d_dir = std::move(dir);
  h->n_buckets = n_buckets;
  h->unit = unit;
  h->max_probe = max_probe;
  h->d_ovf = std::move(ovf);
  h->n_ovf = n_ovf;
  h->n_slots = n_slots;
  h->n_groups = meta[0];
  h->device = device;
  if (h->keys.empty()) h->n_records = n;
  return KM_OK;
}

extern "C" int kmjf_upload(kmjf_t* h, int device) {
  if (!h) return fail(KM_E_ARG, "null argument");
  HIPCHK(hipSetDevice(device));
  const uint64_t n = h->keys.size();
  DevBuf<uint64_t> d_keys;
  DevBuf<uint32_t> d_counts;
  if (n) {
    int rc = d_keys.alloc(n);
    if (rc == KM_OK) rc = d_counts.alloc(n);
    if (rc != KM_OK) return rc;
    hipError_t e = hipMemcpy(d_keys, h->keys.data(), n * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_counts, h->counts.data(), n * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(KM_E_HIP, "record upload failed: %s", hipGetErrorString(e));
  }
  return kmjf_upload_from_device(h, device, d_keys, d_counts, n, nullptr);
}

// ---- kmjf_broadcast: one process, several GPUs.  RCCL is looked up at run time (dlopen) so that the library
// has no link-time dependency on it; only its types come from the header.
namespace {
struct RcclApi {
  void* lib = nullptr;
  ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  ncclResult_t (*Broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
const RcclApi* rccl_api() {
  static RcclApi api;
  static std::once_flag once;
  std::call_once(once, [] {
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      api.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
      if (api.lib) break;
    }
    if (!api.lib) return;
    api.CommInitAll = reinterpret_cast<decltype(api.CommInitAll)>(dlsym(api.lib, "ncclCommInitAll"));
    api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(dlsym(api.lib, "ncclCommDestroy"));
    api.GroupStart = reinterpret_cast<decltype(api.GroupStart)>(dlsym(api.lib, "ncclGroupStart"));
    api.GroupEnd = reinterpret_cast<decltype(api.GroupEnd)>(dlsym(api.lib, "ncclGroupEnd"));
    api.Broadcast = reinterpret_cast<decltype(api.Broadcast)>(dlsym(api.lib, "ncclBroadcast"));
    api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(dlsym(api.lib, "ncclGetErrorString"));
  });
  const bool ok = api.lib && api.CommInitAll && api.CommDestroy && api.GroupStart && api.GroupEnd && api.Broadcast;
  return ok ? &api : nullptr;
}
}  // namespace

extern "C" int kmjf_broadcast(kmjf_t* h, const int* devices, int n, kmjf_t** replicas) {
  if (!h || !devices || !replicas || n < 1) return fail(KM_E_ARG, "bad argument");
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < i; ++j)
      if (devices[i] == devices[j]) return fail(KM_E_ARG, "device %d named twice", devices[i]);
  int n_dev = 0;
  HIPCHK(hipGetDeviceCount(&n_dev));
  for (int i = 0; i < n; ++i)
    if (devices[i] < 0 || devices[i] >= n_dev) return fail(KM_E_ARG, "no device %d (this process sees %d)", devices[i], n_dev);
  for (int i = 0; i < n; ++i) replicas[i] = nullptr;
  if (n == 1) {
    int rc = kmjf_upload(h, devices[0]);
    if (rc == KM_OK) replicas[0] = h;
    return rc;
  }
  const RcclApi* api = rccl_api();
  if (!api) {
    const char* why = dlerror();                       // (a second call returns NULL)
    return fail(KM_E_HIP, "RCCL (librccl.so.1) cannot be loaded: %s", why ? why : "symbols missing");
  }
  const uint64_t cnt = h->keys.size();
  const uint64_t bytes = cnt * 12;                     // keys, then counts: one buffer, one broadcast
  struct Peer {                                        // one device's share, released under that device
    int device = 0;
    unsigned char* buf = nullptr;
    hipStream_t st = nullptr;
    ncclComm_t comm = nullptr;
    const RcclApi* api = nullptr;                      // set once the communicators are up
    Peer() = default;
    Peer(const Peer&) = delete;
    ~Peer() {
      (void)hipSetDevice(device);
      if (buf) (void)hipFree(buf);
      if (st) (void)hipStreamDestroy(st);
      if (api && comm) (void)api->CommDestroy(comm);
    }
  };
  std::vector<std::unique_ptr<kmjf>> made(n);         // the tables of devices[1..]: handed out once all are built
  std::vector<Peer> peer(n);
  for (int i = 0; i < n; ++i) peer[i].device = devices[i];
  for (int i = 0; i < n; ++i) {
    hipError_t e = hipSetDevice(devices[i]);
    if (e == hipSuccess) e = hipMalloc((void**)&peer[i].buf, bytes ? bytes : 16);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&peer[i].st, hipStreamNonBlocking);
    if (e != hipSuccess) return fail_hip(KM_E_NOMEM, "record buffer", e);
  }
  {
    hipError_t e = hipSetDevice(devices[0]);
    if (e == hipSuccess && cnt) e = hipMemcpy(peer[0].buf, h->keys.data(), cnt * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess && cnt) e = hipMemcpy(peer[0].buf + cnt * 8, h->counts.data(), cnt * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail_hip(KM_E_HIP, "record upload", e);
  }
  std::vector<ncclComm_t> comm(n, nullptr);
  ncclResult_t nr = api->CommInitAll(comm.data(), n, devices);
  if (nr != ncclSuccess) return fail(KM_E_HIP, "ncclCommInitAll: %s", api->GetErrorString ? api->GetErrorString(nr) : "failed");
  for (int i = 0; i < n; ++i) { peer[i].comm = comm[i]; peer[i].api = api; }
  if (bytes) {
    nr = api->GroupStart();
    for (int i = 0; i < n && nr == ncclSuccess; ++i) {
      (void)hipSetDevice(devices[i]);
      nr = api->Broadcast(peer[i].buf, peer[i].buf, bytes, ncclUint8, 0, peer[i].comm, peer[i].st);
    }
    const ncclResult_t ne = api->GroupEnd();
    if (nr == ncclSuccess) nr = ne;
    if (nr != ncclSuccess) return fail(KM_E_HIP, "ncclBroadcast: %s", api->GetErrorString ? api->GetErrorString(nr) : "failed");
  }
  for (int i = 0; i < n; ++i) {
    hipError_t e = hipSetDevice(devices[i]);
    if (e == hipSuccess) e = hipStreamSynchronize(peer[i].st);
    if (e != hipSuccess) return fail_hip(KM_E_HIP, "broadcast did not complete", e);
  }
  // every device builds its own table from its copy of the records
  for (int i = 0; i < n; ++i) {
    kmjf_t* r = h;
    if (i > 0) {
      int rc = kmjf_create(h->k, h->canonical, &r);
      if (rc != KM_OK) { const std::string why = km_last_error(); return fail(rc, "replica: %s", why.c_str()); }
      made[i].reset(r);
    }
    int rc = kmjf_upload_from_device(r, devices[i], reinterpret_cast<const uint64_t*>(peer[i].buf),
                                     reinterpret_cast<const uint32_t*>(peer[i].buf + cnt * 8), cnt, peer[i].st);
    if (rc != KM_OK) { const std::string why = km_last_error(); return fail(rc, "table build: %s", why.c_str()); }
  }
  replicas[0] = h;
  for (int i = 1; i < n; ++i) replicas[i] = made[i].release();
  return KM_OK;
}

// Direct ingestion: header parsed on the host, the record area of the (memory-mapped) file is
// copied to HBM as it is, unpacked there (k_unpack_records) and the table is built from the
// device-resident records.  No host copy of the records is made or kept (kmjf_records()
// reports none).  Measured (bench.py `jf_ingestion`) against the host reader + upload.
extern "C" int kmjf_load(const char* path, int device, kmjf_t** out) {
  if (!path || !out) return fail(KM_E_ARG, "null argument");
  RecordFile file;
  int rc = file.open(path);
  if (rc != KM_OK) return rc;
  const jfio::Layout& lay = file.lay;
  const uint64_t n = lay.n_records;
  const uint64_t rec = file.rec;
  const uint64_t body = n * rec;
  // map the whole file (the record area does not start on a page boundary)
  const uint64_t map_len = lay.body_offset + body;
  Mapping map(nullptr, Unmap{map_len});
  if (body) {
    void* m = mmap(nullptr, map_len, PROT_READ, MAP_PRIVATE | MAP_POPULATE, fileno(file.f), 0);   // populate: no per-page faults during the copy
    if (m == MAP_FAILED) return fail(KM_E_IO, "cannot map %s", path);
    map.reset(m);
    (void)madvise(m, map_len, MADV_SEQUENTIAL);
  }
  file.f.reset();                              // the mapping stays valid

  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return fail_hip(KM_E_HIP, "device setup failed", e);
  // KM_LOAD_CHUNK_KB: copy granularity (default 256 MB; tests use small chunks)
  uint64_t chunk_target = 256ull << 20;
  if (const char* ck = getenv("KM_LOAD_CHUNK_KB")) { long v = atol(ck); if (v >= 1) chunk_target = (uint64_t)v << 10; }
  const uint64_t chunk_recs = std::max<uint64_t>(1, chunk_target / rec);
  DevBuf<uint64_t> d_keys;
  DevBuf<uint32_t> d_counts;
  DevBuf<unsigned long long> d_meta;
  unsigned long long nz = 0;
  {
    DevBuf<unsigned char> d_raw;               // one chunk of the records as stored: freed before the table build
    if (n) {
      rc = d_raw.alloc(std::min(n, chunk_recs) * rec);
      if (rc == KM_OK) rc = d_keys.alloc(n);
      if (rc == KM_OK) rc = d_counts.alloc(n);
    }
    if (rc == KM_OK) rc = d_meta.alloc(1);
    if (rc != KM_OK) return rc;
    (void)hipMemset(d_meta, 0, 8);
    const unsigned char* src = static_cast<const unsigned char*>(map.get()) + lay.body_offset;
    for (uint64_t done = 0; done < n;) {
      const uint64_t m = std::min(chunk_recs, n - done);
      e = hipMemcpy(d_raw, src + done * rec, m * rec, hipMemcpyHostToDevice);   // pageable: staged by the runtime
      if (e != hipSuccess) return fail_hip(KM_E_HIP, "ingestion failed", e);
      hipLaunchKernelGGL(k_unpack_records, dim3(grid_for(m, 256)), dim3(256), 0, nullptr, d_raw, m, lay.key_bytes,
                         lay.counter_bytes, d_keys + done, d_counts + done, d_meta);
      done += m;
    }
    e = hipMemcpy(&nz, d_meta, 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail_hip(KM_E_HIP, "ingestion failed", e);
  }
  kmjf* h = new (std::nothrow) kmjf;
  if (!h) return fail(KM_E_NOMEM, "host allocation failed");
  h->k = lay.k;
  h->canonical = lay.canonical;
  rc = kmjf_upload_from_device(h, device, d_keys, d_counts, n, nullptr);
  if (rc != KM_OK) { delete h; return rc; }
  h->n_records = nz;
  *out = h;
  return KM_OK;
}

// Diagnostics: the directory and the slots of an uploaded table as they lie in HBM (tests classify the buckets)
extern "C" int kmjf_debug_table(kmjf_t* h, uint32_t* dir, uint64_t dir_cap, void* slots, uint64_t slots_cap_bytes,
                                uint64_t* n_buckets, uint64_t* n_slots) {
  if (!h || !n_buckets || !n_slots) return fail(KM_E_ARG, "null argument");
  if (!h->d_slots) return fail(KM_E_STATE, "table not uploaded");
  *n_buckets = h->n_buckets;
  *n_slots = h->n_slots;
  if (!dir && !slots) return KM_OK;
  if (dir && dir_cap < (uint64_t)h->n_buckets + 1) return fail(KM_E_ARG, "directory buffer too small");
  if (slots && slots_cap_bytes < h->n_slots * sizeof(Slot)) return fail(KM_E_ARG, "slot buffer too small");
  HIPCHK(hipSetDevice(h->device));
  if (dir) HIPCHK(hipMemcpy(dir, h->d_dir, ((uint64_t)h->n_buckets + 1) * 4, hipMemcpyDeviceToHost));
  if (slots) HIPCHK(hipMemcpy(slots, h->d_slots, h->n_slots * sizeof(Slot), hipMemcpyDeviceToHost));
  return KM_OK;
}

// -------------------------------------------------------------------------- lookups
extern "C" int kmjf_query_batch_dev(kmjf_t* h, const uint64_t* d_kmers, uint64_t n,
                                    uint32_t* d_counts, void* stream) {
  if (!h || (n && (!d_kmers || !d_counts))) return fail(KM_E_ARG, "null argument");
  if (!h->d_slots) return fail(KM_E_STATE, "table not uploaded");
  if (!n) return KM_OK;
  HIPCHK(hipSetDevice(h->device));
  hipLaunchKernelGGL(k_query, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream,
                     view_of(h), d_kmers, n, d_counts);
  HIPCHK(hipGetLastError());
  return KM_OK;
}

extern "C" int kmjf_children_batch_dev(kmjf_t* h, const uint64_t* d_kmers, uint64_t n, double ratio,
                                       int64_t n_cutoff, int forward, uint8_t* d_mask,
                                       uint32_t* d_counts4, void* stream) {
  if (!h || (n && !d_kmers)) return fail(KM_E_ARG, "null argument");
  if (!h->d_slots) return fail(KM_E_STATE, "table not uploaded");
  if (!n) return KM_OK;
  HIPCHK(hipSetDevice(h->device));
  hipLaunchKernelGGL(k_children, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream,
                     view_of(h), d_kmers, n, ratio, n_cutoff, forward, d_mask, d_counts4);
  HIPCHK(hipGetLastError());
  return KM_OK;
}

extern "C" int kmjf_query_batch(kmjf_t* h, const uint64_t* kmers, uint64_t n, uint32_t* counts) {
  if (!h || (n && (!kmers || !counts))) return fail(KM_E_ARG, "null argument");
  if (!h->d_slots) return fail(KM_E_STATE, "table not uploaded");
  if (!n) return KM_OK;
  HIPCHK(hipSetDevice(h->device));
  DevBuf<uint64_t> dk;
  DevBuf<uint32_t> dc;
  int rc = dk.alloc(n);
  if (rc == KM_OK) rc = dc.alloc(n);
  if (rc != KM_OK) return rc;
  hipError_t e = hipMemcpy(dk, kmers, n * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    rc = kmjf_query_batch_dev(h, dk, n, dc, nullptr);
    if (rc == KM_OK) e = hipMemcpy(counts, dc, n * 4, hipMemcpyDeviceToHost);
  }
  if (rc != KM_OK) return rc;
  if (e != hipSuccess) return fail(KM_E_HIP, "query batch failed: %s", hipGetErrorString(e));
  return KM_OK;
}

extern "C" int kmjf_children_batch(kmjf_t* h, const uint64_t* kmers, uint64_t n, double ratio,
                                   int64_t n_cutoff, int forward, uint8_t* mask, uint32_t* counts4) {
  if (!h || (n && !kmers)) return fail(KM_E_ARG, "null argument");
  if (!h->d_slots) return fail(KM_E_STATE, "table not uploaded");
  if (!n) return KM_OK;
  HIPCHK(hipSetDevice(h->device));
  DevBuf<uint64_t> dk;
  DevBuf<uint8_t> dm;
  DevBuf<uint32_t> dc;
  int rc = dk.alloc(n);
  if (rc != KM_OK) return rc;
  if (dm.alloc(n) != KM_OK || dc.alloc(4 * n) != KM_OK) {
    const std::string why = km_last_error();
    return fail(KM_E_HIP, "children batch failed: %s", why.c_str());
  }
  hipError_t e = hipMemcpy(dk, kmers, n * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    rc = kmjf_children_batch_dev(h, dk, n, ratio, n_cutoff, forward, dm, dc, nullptr);
    if (rc == KM_OK && mask) e = hipMemcpy(mask, dm, n, hipMemcpyDeviceToHost);
    if (rc == KM_OK && e == hipSuccess && counts4) e = hipMemcpy(counts4, dc, n * 16, hipMemcpyDeviceToHost);
  }
  if (rc != KM_OK) return rc;
  if (e != hipSuccess) return fail(KM_E_HIP, "children batch failed: %s", hipGetErrorString(e));
  return KM_OK;
}
