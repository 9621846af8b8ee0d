// host_common.h — what every host part of kmgpu.hip shares: error plumbing, the in-place scan, owned resources, Staging, the stream pool
// ------------------------------------------------------------------ error plumbing
static thread_local std::string g_last_error;

static int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

#define HIPCHK(expr)                                                                   \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess)                                                              \
      return fail(e_ == hipErrorOutOfMemory ? KM_E_NOMEM : KM_E_HIP, "%s failed: %s (%s:%d)", \
                  #expr, hipGetErrorString(e_), __FILE__, __LINE__);                   \
  } while (0)

// ... and for the library's own codes: pass a failure on to the caller
#define KMCHK(expr) do { const int rc_ = (expr); if (rc_ != KM_OK) return rc_; } while (0)

extern "C" const char* km_strerror(int code) {
  switch (code) {
    case KM_OK: return "ok";
    case KM_E_IO: return "I/O error";
    case KM_E_FORMAT: return "not a Jellyfish binary/sorted file";
    case KM_E_K: return "unsupported k (need 2 <= k <= 32)";
    case KM_E_ARG: return "bad argument";
    case KM_E_HIP: return "HIP runtime error";
    case KM_E_NOMEM: return "out of memory";
    case KM_E_STATE: return "call order violated";
    case KM_E_CAPACITY: return "output buffer too small";
  }
  return "unknown error";
}
extern "C" const char* km_last_error(void) { return g_last_error.c_str(); }
extern "C" const char* km_version(void) { return "km_amd 0.1.0 (gfx950)"; }
extern "C" int km_device_count(int* n) {
  if (!n) return fail(KM_E_ARG, "null argument");
  HIPCHK(hipGetDeviceCount(n));
  return KM_OK;
}

static int fail_hip(int code, const char* what, hipError_t e) { return fail(code, "%s: %s", what, hipGetErrorString(e)); }

static int grid_for(uint64_t n, int block) {
  uint64_t g = (n + block - 1) / block;
  if (g < 1) g = 1;
  if (g > 256 * 32) g = 256 * 32;      // grid-stride the rest
  return (int)g;
}

static double host_now_us() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// The scan of table_kernels.h: data[0 .. chunks * SCAN_CHUNK) becomes its exclusive prefix sums on `stream`, sums[0 ..
// chunks) is its scratch.  (Launches only: the caller asks hipGetLastError with its own.)
static void scan_in_place(uint32_t* data, uint32_t* sums, uint32_t chunks, hipStream_t stream) {
  hipLaunchKernelGGL(k_scan_reduce, dim3(chunks), dim3(SCAN_THREADS), 0, stream, data, sums);
  hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(SCAN_THREADS), 0, stream, sums, chunks);
  hipLaunchKernelGGL(k_scan_apply, dim3(chunks), dim3(SCAN_THREADS), 0, stream, data, sums);
}

// ------------------------------------------------------------------ owned resources
// Every buffer, event, graph and file the library makes belongs to one of these, which releases it when the owner goes
// and reads as the raw handle it holds.  A release happens under the device current at that moment: an owner of another
// device's resource sets that device first (kmjf::free_table, kmjf_broadcast's Peer).  None lives in static storage
// (the pool's streams below are plain handles that last as long as the process).
namespace {
template <typename T>
struct DevBuf {
  T* p = nullptr;
  uint64_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(DevBuf&& o) noexcept {   // frees what this held, takes what o held
    release();
    std::swap(p, o.p);
    std::swap(n, o.n);
    return *this;
  }
  ~DevBuf() { release(); }
  operator T*() const { return p; }
  int alloc(uint64_t count) {
    if (count <= n && p) return KM_OK;
    release();
    if (count == 0) count = 1;
    hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
    if (e != hipSuccess) { p = nullptr; n = 0; return fail(KM_E_NOMEM, "hipMalloc of %llu bytes failed",
                                                          (unsigned long long)(count * sizeof(T))); }
    n = count;
    return KM_OK;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};

template <typename H, auto Free>
struct Owned {
  H h;
  explicit Owned(H v = nullptr) : h(v) {}
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  Owned(Owned&& o) noexcept : h(o.take()) {}
  ~Owned() { reset(); }
  operator H() const { return h; }
  void reset() { if (h) (void)Free(h); h = nullptr; }
  H take() { H v = h; h = nullptr; return v; }     // the handle, from now on the caller's to free
};
using Event = Owned<hipEvent_t, hipEventDestroy>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Graph = Owned<hipGraph_t, hipGraphDestroy>;
using GraphExec = Owned<hipGraphExec_t, hipGraphExecDestroy>;
using Pinned = Owned<unsigned char*, hipHostFree>;
using File = Owned<FILE*, fclose>;
struct Unmap { size_t len; void operator()(void* p) const { munmap(p, len); } };
using Mapping = std::unique_ptr<void, Unmap>;

// bytes of pinned host memory into an (empty) owner
static int pinned_alloc(Pinned* to, uint64_t bytes, const char* what) {
  hipError_t e = hipHostMalloc((void**)&to->h, bytes, hipHostMallocDefault);
  if (e != hipSuccess) { to->h = nullptr; return fail(KM_E_NOMEM, "%s: %s", what, hipGetErrorString(e)); }
  return KM_OK;
}

// Timing of kernels that an environment variable asks for: an event pair around each run of them on one stream.
// Does nothing unless `timed`.  The owner declares it after its stream: the events go before the stream.
struct KernelSpans {
  bool timed = false;
  std::vector<std::pair<Event, Event>> pairs;      // recorded and not yet drained
  float ms = 0.f;                                  // of the pairs drained so far
  int open(hipStream_t st) {
    if (!timed) return KM_OK;
    Event t0, t1;
    HIPCHK(hipEventCreate(&t0.h));
    HIPCHK(hipEventCreate(&t1.h));
    pairs.emplace_back(std::move(t0), std::move(t1));
    HIPCHK(hipEventRecord(pairs.back().first, st));
    return KM_OK;
  }
  int close(hipStream_t st) {
    if (timed) HIPCHK(hipEventRecord(pairs.back().second, st));
    return KM_OK;
  }
  // (the stream has been waited for)  *total = the time of every pair so far
  int drain(float* total) {
    for (auto& p : pairs) {
      float t = 0.f;
      HIPCHK(hipEventElapsedTime(&t, p.first, p.second));
      ms += t;
    }
    pairs.clear();
    *total = ms;
    return KM_OK;
  }
};

// Two pinned buffers that take turns between the host and a stream, and an event per buffer: the copy that last
// used it is done.  One rule holds them together, in either direction: the host touches a buffer only once that
// copy is done.  It therefore gets a buffer's address from claim() or wait() alone, which wait for the event first.
// Host to device (a counter's text, FASTQ and record pieces; km_jf_histo): producers write through `mine`, which
// claim() sets to the buffer whose turn it is and ship() takes away again, so it is null in between and no producer
// can write under a copy.  Device to host (km_counter_write_jf, once the counter has finished): fetch(buf) enqueues
// the copy into a buffer and wait(buf) hands it out to be read.
constexpr uint64_t COUNT_STAGE_BYTES = 16ull << 20;     // per pinned buffer
struct Staging {
  Pinned pin[2];
  Event copied[2];                        // the copy out of, or into, pin[i] is done
  uint64_t bytes = COUNT_STAGE_BYTES;     // per buffer (KM_COUNT_STAGE_BYTES: tests reach many pieces with small inputs)
  int cur = 0;                            // whose turn it is
  unsigned char* mine = nullptr;          // pin[cur] while it is the host's to write
  Staging() { if (const char* e = getenv("KM_COUNT_STAGE_BYTES")) bytes = std::max<uint64_t>(256, strtoull(e, nullptr, 10)); }
  int alloc(uint64_t pad) {               // the buffers, of bytes + pad each, and their events
    for (int i = 0; i < 2; ++i) {
      KMCHK(pinned_alloc(&pin[i], bytes + pad, "pinned staging buffer"));
      HIPCHK(hipEventCreateWithFlags(&copied[i].h, hipEventDisableTiming));
    }
    return KM_OK;
  }
  int claim() { return wait(cur, &mine); }
  // The n bytes the host wrote to the claimed buffer go to d_dst on st, and the turn passes to the other buffer.
  int ship(void* d_dst, uint64_t n, hipStream_t st) {
    HIPCHK(hipMemcpyAsync(d_dst, mine, n, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(copied[cur], st));
    mine = nullptr;
    cur ^= 1;
    return KM_OK;
  }
  int fetch(int buf, const void* d_src, uint64_t n, hipStream_t st) {
    HIPCHK(hipMemcpyAsync(pin[buf], d_src, n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(copied[buf], st));
    return KM_OK;
  }
  int wait(int buf, unsigned char** ready) {
    HIPCHK(hipEventSynchronize(copied[buf]));
    *ready = pin[buf];
    return KM_OK;
  }
};
}  // namespace

// ---- streams.  A pipelined consumer runs a few batches at a time, each on its own launch stream.  How
// those streams fall onto the GPU's hardware queues decides how well the batches overlap.  Measured on
// MI355X, four batches in flight (tools/pump_min.py): with the runtime's default of 4 hardware queues and
// k_graph_pure on a per-batch side stream (round 2's arrangement) 0.30 ms per step — every side stream
// shares a queue with ANOTHER batch's launch stream; 0.34 when launch streams themselves end up pairwise
// on one queue; 0.21 with 8 queues and the side streams on queues of their own; 0.19 with 8 queues and no
// side stream at all: a batch's kernels in ONE stream, every launch stream on a queue of its own.  So
// (1) there is no side stream any more — the overlap of k_graph_pure with k_dfs it was there for comes from ONE
// launch that holds the blocks of both (graph_kernel.h: k_dfs_pure), which needs no stream or queue of its
// own —, (2) the library asks for 8 hardware queues unless the environment
// says otherwise — when it is loaded, i.e. before the HIP runtime reads its settings — and (3) launch
// streams come from a per-device pool created once.
namespace {
__attribute__((constructor)) void km_default_hw_queues() { setenv("GPU_MAX_HW_QUEUES", "8", 0); }

// Seven: with the null stream one per hardware queue of the library's default of 8 — and what a consumer that keeps
// four batches in flight on four pool streams (bench.py, kmclient) leaves km_batch_pump are the three it takes for its
// paired steps (chain, tail, front: result_host.h), so no stream is created or destroyed inside a pump call.
constexpr int POOL_STREAMS = 7;
struct StreamPool {
  std::vector<hipStream_t> launch;
  std::vector<char> in_use;                        // handed out by km_stream_create and not yet given back
};
std::mutex g_pool_mu;
std::map<int, StreamPool> g_pools;

// (device already current)  A pooled stream that nobody holds; once all are out, a fresh stream of the caller's
// own (two consumers never share a launch stream: a capture on it, or a wait for its last batch, would see the
// other's work).
int pool_get(int device, hipStream_t* out) {
  std::lock_guard<std::mutex> lk(g_pool_mu);
  StreamPool& p = g_pools[device];
  if (p.launch.empty()) {
    Stream made[POOL_STREAMS];                     // the pool takes them once all exist
    for (Stream& s : made) HIPCHK(hipStreamCreateWithFlags(&s.h, hipStreamNonBlocking));
    for (Stream& s : made) p.launch.push_back(s.take());
    p.in_use.assign(p.launch.size(), 0);
  }
  for (size_t i = 0; i < p.launch.size(); ++i)
    if (!p.in_use[i]) { p.in_use[i] = 1; *out = p.launch[i]; return KM_OK; }
  hipStream_t st = nullptr;
  HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  *out = st;
  return KM_OK;
}
// true: a pool stream (now free again); false: not ours to keep
bool pool_give_back(hipStream_t st) {
  std::lock_guard<std::mutex> lk(g_pool_mu);
  for (auto& kv : g_pools)
    for (size_t i = 0; i < kv.second.launch.size(); ++i)
      if (kv.second.launch[i] == st) { kv.second.in_use[i] = 0; return true; }
  return false;
}

// The stream of one call, read as the handle like the owners above: the caller's, or one of the pool's for as long as
// the call lasts.  Declared before whatever runs on the stream, so that it is released after it.
struct CallStream {
  hipStream_t st = nullptr;
  bool own = false;
  ~CallStream() { if (own && !pool_give_back(st)) (void)hipStreamDestroy(st); }
  operator hipStream_t() const { return st; }
  int get(int device, void* stream) {      // makes `device` current
    HIPCHK(hipSetDevice(device));
    st = (hipStream_t)stream;
    if (!st) { KMCHK(pool_get(device, &st)); own = true; }
    return KM_OK;
  }
};

// Declared after what its streams (a launch stream; a copy stream, if there is one) work on, in a call or in an owner:
// waits for both before any of that is freed, so no copy into a freed buffer and no kernel on one stays in flight.
// device >= 0: made current first (an owner that may go on another thread than the one that made it).
struct StreamDrain {
  hipStream_t st = nullptr, cs = nullptr;
  int device = -1;
  ~StreamDrain() {
    if (device >= 0) (void)hipSetDevice(device);
    if (st) (void)hipStreamSynchronize(st);
    if (cs) (void)hipStreamSynchronize(cs);
  }
};
}  // namespace

extern "C" int km_stream_create(int device, void** stream) {
  if (!stream) return fail(KM_E_ARG, "null argument");
  HIPCHK(hipSetDevice(device));
  hipStream_t st = nullptr;
  int rc = pool_get(device, &st);
  if (rc != KM_OK) return rc;
  *stream = st;
  return KM_OK;
}
// (pool streams live as long as the process: one handed back is free for the next km_stream_create; a stream made
// beyond the pool is destroyed)
extern "C" int km_stream_destroy(void* stream) {
  if (stream && !pool_give_back((hipStream_t)stream)) HIPCHK(hipStreamDestroy((hipStream_t)stream));
  return KM_OK;
}
