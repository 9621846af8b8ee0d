// batch_host.h — km_batch (host part of kmgpu.hip).  In reading order: the knobs, LaunchHints (how each grid is sized
// and when a captured step is stale), what a batch owns by group, set_targets, the geometry, the launches, the step
// (km_batch_run), the large tier and km_batch_sync.  What reads a delivered step is in result_host.h.
// ---------------------------------------------------------------------------- environment knobs
// Read once per process.  The ones that make results INVALID (timing ablations) exist only in a
// diagnostics build of the library (-DKM_DIAGNOSTICS, what tools/_diag.py compiles): the product
// library cannot be talked into returning KM_OK over undelivered or partial data.
namespace {
struct Knobs {
  uint32_t debug_flags = 0;     // KM_DEBUG_FLAGS      (diagnostics build) stage cuts of k_dfs / k_graph
  int debug_deliver = 0;        // KM_DEBUG_DELIVER    (diagnostics build) skip delivery kernels / copy
  bool zero_copy = false;       // KM_DELIVER_ZEROCOPY (diagnostics build) pack straight into pinned memory
  int dfs_replay = 0;           // KM_DFS_REPLAY       (diagnostics build) k_dfs twice per step
  bool epilogue = true;         // KM_EPILOGUE=0: every flagged target through k_graph (results unchanged)
  bool seed_stamps = false;     // KM_SEED_STAMPS: in-kernel time stamps (results unchanged, slower)
  bool host_trace = false;      // KM_TRACE_HOST: host time of the sections of km_batch_run on stderr
  long spin_us = 0;             // KM_SPIN_US: poll the delivery event this long before sleeping on it
  uint32_t graph_grid = 0;      // KM_GRAPH_GRID: blocks of k_graph when the epilogue of k_dfs is on (tests: force the overflow path)
  bool speculate = true;        // KM_SPECULATE=0: k_dfs walks every chain one lookup after the other (results unchanged)
  bool dfs_grid_full = false;   // KM_DFS_GRID_FULL=1: one block of k_dfs per target of the batch, as before round 4
  bool fuse_pure = true;        // KM_FUSE_PURE=0: k_dfs and k_graph_pure as two launches, as before round 6 (results unchanged)
  int pair_seed = 1;            // KM_PAIR_SEED=0: km_batch_pump never runs a batch's k_seed in another batch's walk launch; 2: wherever it can, also where it does not pay (results unchanged)
  bool seed_waves = false;      // KM_SEED_WAVES=1: k_seed as single-wave blocks (k_seed_waves: what seed_body costs alone; results unchanged)
  bool pump_front = true;       // KM_PUMP_FRONT=0: paired steps run k_pack of the next batch on the chain, in front of the paired launch, as in round 7; default: on a third stream of the pump (results unchanged)
  bool pair_pure_last = true;   // KM_PAIR_PURE_LAST=0: the paired launch's blocks in round 7's order walk, pure-chain, seeds; default: walk, seeds, pure-chain (pair_roles.h; results unchanged)
};
Knobs read_knobs() {
  Knobs q;
  auto num = [](const char* name, long dflt) { const char* v = getenv(name); return v ? strtol(v, nullptr, 0) : dflt; };
#ifdef KM_DIAGNOSTICS
  q.debug_flags = (uint32_t)num("KM_DEBUG_FLAGS", 0);
  q.debug_deliver = (int)num("KM_DEBUG_DELIVER", 0);
  q.zero_copy = num("KM_DELIVER_ZEROCOPY", 0) != 0;
  q.dfs_replay = (int)num("KM_DFS_REPLAY", 0);
#endif
  q.epilogue = num("KM_EPILOGUE", 1) != 0;
  q.seed_stamps = getenv("KM_SEED_STAMPS") != nullptr;
  q.host_trace = getenv("KM_TRACE_HOST") != nullptr;
  q.spin_us = num("KM_SPIN_US", 0);
  q.graph_grid = (uint32_t)std::max<long>(0, num("KM_GRAPH_GRID", 0));
  q.speculate = num("KM_SPECULATE", 1) != 0;
  q.dfs_grid_full = num("KM_DFS_GRID_FULL", 0) != 0;
  q.fuse_pure = num("KM_FUSE_PURE", 1) != 0;
  q.pair_seed = (int)num("KM_PAIR_SEED", 1);
  q.seed_waves = num("KM_SEED_WAVES", 0) != 0;
  q.pump_front = num("KM_PUMP_FRONT", 1) != 0;
  q.pair_pure_last = num("KM_PAIR_PURE_LAST", 1) != 0;
  return q;
}
const Knobs& knobs() {
#ifdef KM_DIAGNOSTICS
  static thread_local Knobs k;      // the diagnostics tools change the ablation flags between runs
  k = read_knobs();
  return k;
#else
  static const Knobs k = read_knobs();
  return k;
#endif
}

// What km_batch_create takes from the environment.  Read at EVERY km_batch_create, not once per process like the
// Knobs: the tests set KM_TEST_SMALL_POOLS inside the running process, between two batches.
//   KM_BIG_DEVICE_OFF: no large tier of the device's own (every such target: the host's); KM_BIG_DEVICE=1: that tier
//   armed from the first run; KM_TEST_SMALL_POOLS (tests): force the pool-overflow path of km_batch_sync
struct CreateOptions { bool big_device_off, big_device_armed, small_pools; };
CreateOptions read_create_options() {
  const char* armed = getenv("KM_BIG_DEVICE");
  return {getenv("KM_BIG_DEVICE_OFF") != nullptr, armed && atoi(armed) != 0, getenv("KM_TEST_SMALL_POOLS") != nullptr};
}
}  // namespace

// ---------------------------------------------------------------------------- batch
namespace {

// (FAST_EXTRA, FAST_LDS_LIMIT, FAST_BCAP_MAX, FAST_FCAP_MAX, what fits the fast tier and its sizes, and round_up:
// tier_geometry.h)
constexpr uint32_t LOOP_LOG_CAP = 4096;       // loop breaks of a batch kept for km_batch_graph_log (the rest is counted only)
constexpr uint32_t BIG_DEV_SLOTS = 32;        // targets per run the device's own large tier takes (the rest: the host's)
constexpr uint64_t BIG_DEV_MAX_BYTES = 1ull << 30;   // ... unless their node storage would exceed this (huge -n)

// Region A of the delivery buffer (deliver_kernel.h): offsets from n_targets alone.
struct OutLayout { uint64_t totals, status, n_ref, probes, node_off, extra_off, path_off, ref_max, esc_node, esc_value, a_bytes; };
OutLayout out_layout(uint32_t n) {
  auto al = [](uint64_t v) { return (v + 63) & ~63ull; };
  OutLayout L;
  uint64_t o = 0;
  L.totals = o;    o = al(o + 8ull * OT_WORDS);
  L.status = o;    o = al(o + 4ull * n);
  L.n_ref = o;     o = al(o + 4ull * n);
  L.probes = o;    o = al(o + 8ull * n);
  L.node_off = o;  o = al(o + 8ull * ((uint64_t)n + 1));
  L.extra_off = o; o = al(o + 8ull * ((uint64_t)n + 1));
  L.path_off = o;  o = al(o + 4ull * ((uint64_t)n + 1));
  L.ref_max = o;   o = al(o + 4ull * n);
  L.esc_node = o;  o = al(o + 8ull * OUT_ESC_CAP);
  L.esc_value = o; o = al(o + 4ull * OUT_ESC_CAP);
  L.a_bytes = o;
  return L;
}

// The first failure of a run of allocations.  All of them are attempted, in the order written (a braced list is
// evaluated left to right).
int first_error(std::initializer_list<int> rcs) {
  for (int r : rcs) if (r != KM_OK) return r;
  return KM_OK;
}

// ---- launch hints: the grids of k_dfs and k_graph follow what the last DELIVERED run of this batch reported, and a
// captured step (which holds its grids) is stale once the report has moved away from them.  A new target set does
// not reset them.
struct LaunchHints {
  static constexpr uint32_t NONE = 0xFFFFFFFFu;   // nothing seen yet: the default grid
  uint32_t flagged_seen = NONE;      // flagged targets of the last delivered run: the grid of k_dfs
  uint32_t graph_list_seen = NONE;   // entries of k_graph's work list in it

  // k_dfs, one single-wave block per FLAGGED target: x 1.25 + 64 of what was seen (the whole batch until then, or with
  // KM_DFS_GRID_FULL=1) — 6 000 of the headline batch's 10 000 blocks used to leave after one load, each having claimed
  // its LDS first.  More flagged targets than blocks: the kernel hands the rest to the large tier (walk_kernel.h).
  uint32_t dfs_grid(uint32_t n_targets) const {
    uint32_t grid = n_targets;
    if (flagged_seen != NONE && !knobs().dfs_grid_full)
      grid = (uint32_t)std::min<uint64_t>(grid, (uint64_t)flagged_seen + flagged_seen / 4 + 64);
    return grid;
  }
  // k_graph, one block per entry of the work list.  When the epilogue of k_dfs answers the regular targets
  // (`short_list`) the list is a percent of the batch: an eighth of the batch (at least 1 024 blocks; KM_GRAPH_GRID
  // sets it) and at most 4x + 64 of what was seen — with nothing left to it, the headline batch's 1 250 blocks cost
  // 8.6 us alone and 31 us inside the pipeline.  More entries than blocks go to the large tier (graph_kernel.h).
  uint32_t graph_grid(uint32_t n_targets, bool short_list) const {
    if (!short_list) return n_targets;
    uint32_t cap = knobs().graph_grid ? knobs().graph_grid : std::max<uint32_t>(1024u, n_targets / 8);
    if (!knobs().graph_grid && graph_list_seen != NONE)
      cap = std::min<uint32_t>(cap, (uint32_t)std::min<uint64_t>(4ull * graph_list_seen + 64, 0x7FFFFFFFull));
    return std::min<uint32_t>(n_targets, cap);
  }
  // The totals of a delivered run (`graph_list`: NULL unless the graph stage ran in full).  True: a step captured
  // under the old hints is stale — the flagged targets outgrew their grid's margin or fell to a quarter; the work
  // list outgrew a quarter of its grid or shrank to a 16th.
  bool observe(unsigned long long flagged, const unsigned long long* graph_list) {
    bool stale = false;
    const uint32_t fl = (uint32_t)std::min<unsigned long long>(flagged, 0x7FFFFFFFull);
    if (flagged_seen != NONE && (fl > flagged_seen + flagged_seen / 8 + 32 || 4 * fl + 256 < flagged_seen)) stale = true;
    flagged_seen = fl;
    if (graph_list) {
      const uint32_t seen = (uint32_t)std::min<unsigned long long>(*graph_list, 0x7FFFFFFFull);
      if (graph_list_seen != NONE && (seen > 2 * graph_list_seen + 16 || 16 * seen + 64 < graph_list_seen)) stale = true;
      graph_list_seen = seen;
    }
    return stale;
  }
};

// ---- what a batch owns, by what it serves.  Every group allocates its own buffers; km_batch_create calls them in
// the order the allocations have always had.
struct Inputs {                    // the targets as given, packed, and cut into k_seed's work items
  DevBuf<uint8_t> d_bases;
  DevBuf<uint64_t> d_toff, d_woff, d_packed;   // offsets; 2-bit packed targets (k_pack) and theirs
  DevBuf<uint64_t> d_items, d_fw_off;          // k_seed work items and flag bitmaps
  DevBuf<uint32_t> d_item_off, d_flagbits;
  std::vector<uint64_t> h_toff, h_woff, h_fw_off;
  std::vector<uint32_t> h_item_off;
  uint32_t n_items = 0;
  std::vector<uint64_t> h_packed;    // km_batch_fetch: packed targets, when node_kmer is asked for
  DevBuf<float> d_tref;              // shared reference-chain distances (push_layout: grows with the longest target)
  int alloc(uint32_t n, uint64_t max_bases) {
    return first_error({d_bases.alloc(max_bases + 64), d_toff.alloc((uint64_t)n + 1), d_woff.alloc((uint64_t)n + 1),
                        d_packed.alloc(max_bases / 32 + 2 * (uint64_t)n + 2),
                        d_items.alloc(16 * (max_bases / SEED_BLOCK + (uint64_t)n + 1)),
                        d_item_off.alloc((uint64_t)n + 1), d_flagbits.alloc(max_bases / 32 + (uint64_t)n + 1),
                        d_fw_off.alloc((uint64_t)n + 1)});
  }
};

struct PerTarget {                 // what the walk and the graph stage keep per target, and the lists between them
  DevBuf<uint32_t> d_tflag, d_flagged, d_nflagged;
  DevBuf<uint4> d_flag_rec;          // k_seed -> k_dfs: one 32-byte record per flagged target
  DevBuf<uint32_t> d_left;           // k_dfs -> k_graph: flagged targets the epilogue did not answer
  DevBuf<EpiArgs> d_epi;             // where that epilogue writes (device copy of h_epi)
  EpiArgs h_epi{};
  bool epi_valid = false;
  DevBuf<unsigned long long> d_dfs_probes;
  DevBuf<uint64_t> d_node_base;
  DevBuf<uint32_t> d_node_cap;
  std::vector<uint64_t> h_node_base, h_node_base0;   // ...0: the fast-tier layout of layout_targets
  std::vector<uint32_t> h_node_cap, h_node_cap0;
  uint64_t node_pool0 = 0;
  bool layout_moved = false;         // the large tier re-homed some targets: restore before the next run
  DevBuf<uint32_t> d_n_nodes, d_n_ref, d_status, d_gstatus, d_npaths, d_pathbase, d_need_full, d_t_nruns, d_t_refmax;
  std::vector<uint32_t> h_status, h_gstatus, h_n_nodes, h_n_ref, h_npaths, h_pathbase;   // host mirrors after sync
  DevBuf<unsigned char> d_frames;    // fast-tier DFS stack frames, one slice per target (km_batch_run: by the geometry)
  int alloc(uint32_t n) {
    return first_error({d_tflag.alloc(n), d_flagged.alloc(n), d_flag_rec.alloc(2ull * n), d_left.alloc(n),
                        d_epi.alloc(1), d_nflagged.alloc(4), d_dfs_probes.alloc(n), d_node_base.alloc(n),
                        d_node_cap.alloc(n), d_n_nodes.alloc(n), d_n_ref.alloc(n), d_status.alloc(n),
                        d_gstatus.alloc(n), d_npaths.alloc(n), d_pathbase.alloc(n), d_need_full.alloc(n),
                        d_t_nruns.alloc(n), d_t_refmax.alloc(n)});
  }
};

struct Delivery {                  // deliver_kernel.h: device buffer in its final host layout + its pinned host twin
  DevBuf<unsigned long long> d_loc, d_blk_tot, d_blk_base;
  DevBuf<unsigned int> d_scan_ticket;
  DevBuf<uint32_t> d_cnt4;
  DevBuf<unsigned char> d_out;       // (d_out, h_out: ensure_out)
  Pinned h_out;
  uint64_t out_cap = 0;
  Event ev_out;
  bool deliver_pending = false, result_ready = false;
  bool lean = false;                 // the pending / ready delivery omits bare-reference node counts
  bool count16 = false;              // ... and carries 16-bit counts + escape list (KM_DELIVER_COUNT16)
  uint64_t copied_tail = 0, tail_guess = 0;
  unsigned long long serial = 0;
  int alloc_scan(uint32_t n) {
    return first_error({d_loc.alloc(4ull * n), d_cnt4.alloc(4ull * n),
                        d_blk_tot.alloc(8ull * (n / OUT_SCAN_THREADS + 1)),
                        d_blk_base.alloc(4ull * (n / OUT_SCAN_THREADS + 1) + 8), d_scan_ticket.alloc(1)});
  }
};

struct Probes {                    // what a run counts beside its results
  DevBuf<uint64_t> d_probes, d_fetches;
  bool count_fetches = false;        // the last run counted table slots read (KM_RUN_COUNT_FETCHES)
  DevBuf<unsigned long long> d_stamps;   // diagnostics: k_seed time stamps (KM_SEED_STAMPS; km_batch_run)
  int alloc(uint32_t n) { return first_error({d_probes.alloc(n), d_fetches.alloc(n)}); }
};

struct LargeTier {
  DevBuf<uint32_t> d_big_ids;        // the host's large tier (km_batch_sync): its list and its workspace
  DevBuf<unsigned char> d_big_ws;
  uint32_t n_big = 0;                // targets it took in the last synchronised run
  // the device's own large tier (walk_kernel.h: WalkArgs::big_ctl)
  DevBuf<uint64_t> d_node_base0;
  DevBuf<uint32_t> d_big_ctl, d_big_walk, d_big_graph;
  DevBuf<unsigned char> d_bigdev_walk_ws, d_bigdev_graph_ws;   // (ensure_bigdev_ws)
  uint32_t big_entry = 0;            // nodes per slot of the region (0: tier off)
  uint64_t big_region = 0;           // its first node (the region sits in front of the fast-tier layout)
  // Its two launches cost a step ~9 us when every kernel runs alone, needed or not.  They are launched once a
  // delivery of this batch has reported a target for the large tier (the first such target of a workspace's life
  // takes the host's path, as every one used to; KM_BIG_DEVICE=1 arms the tier from the first run)
  bool bigdev_armed = false;
  bool bigdev_ran = false;           // the last run launched it
  // BIG_DEV_SLOTS slots of the reference's own bound on a walk (MutationFinder.py:140-156)
  void configure(const km_params_t& p, const CreateOptions& opt) {
    const uint64_t entry = (uint64_t)p.max_node + p.max_stack + 1;
    if (!opt.big_device_off && entry < 0x7FFFFFFFull && entry * BIG_DEV_SLOTS * 12 <= BIG_DEV_MAX_BYTES) big_entry = (uint32_t)entry;
    bigdev_armed = opt.big_device_armed;
  }
  int alloc(uint32_t n) {
    return first_error({d_node_base0.alloc(n), d_big_ctl.alloc(8), d_big_walk.alloc(BIG_DEV_SLOTS),
                        d_big_graph.alloc(BIG_DEV_SLOTS)});
  }
};

struct VerboseLog {                // -v (km_batch_graph_log): reference edges stripped / edges kept per target, the walk's loop breaks
  DevBuf<uint32_t> d_t_eremoved, d_t_enonref, d_loop_list, d_loop_ctl;
  int alloc(uint32_t n) {
    return first_error({d_t_eremoved.alloc(n), d_t_enonref.alloc(n), d_loop_list.alloc(2ull * LOOP_LOG_CAP),
                        d_loop_ctl.alloc(4)});
  }
};

struct NodePools {
  DevBuf<uint64_t> d_node_kmer;
  DevBuf<uint32_t> d_node_cnt;
  uint64_t node_pool_used = 0;
  int alloc(uint64_t pool) { return first_error({d_node_kmer.alloc(pool), d_node_cnt.alloc(pool)}); }
};

struct PathPools {                 // paths and their runs, claimed by the graph kernels through d_counters
  DevBuf<unsigned long long> d_counters;
  DevBuf<uint32_t> d_p_target, d_p_nruns, d_p_len, d_p_mincov, d_r_start, d_r_len;
  DevBuf<uint64_t> d_p_runbase;
  DevBuf<unsigned long long> d_psort;   // (delivery's sort keys: one per path)
  uint64_t path_pool = 0, run_pool = 0;
  unsigned long long h_overflow = 0;
  int alloc(uint32_t n, bool small_pools) {
    path_pool = small_pools ? 2 * POOL_GROUPS : (((uint64_t)n * 4 + 8192) / POOL_GROUPS + 1) * POOL_GROUPS;
    run_pool = small_pools ? 4 * POOL_GROUPS : (((uint64_t)n * 16 + 32768) / POOL_GROUPS + 1) * POOL_GROUPS;
    return first_error({d_counters.alloc(POOL_GROUPS * POOL_CTR_STRIDE + 16), alloc_pools()});
  }
  int grow() {                       // (km_batch_sync: the pools overflowed)
    path_pool = (path_pool * 4 / POOL_GROUPS + 1) * POOL_GROUPS;
    run_pool = (run_pool * 4 / POOL_GROUPS + 1) * POOL_GROUPS;
    return alloc_pools();
  }
  int alloc_pools() {
    return first_error({d_p_target.alloc(path_pool), d_p_runbase.alloc(path_pool), d_p_nruns.alloc(path_pool),
                        d_p_len.alloc(path_pool), d_p_mincov.alloc(path_pool), d_psort.alloc(path_pool),
                        d_r_start.alloc(run_pool), d_r_len.alloc(run_pool)});
  }
};

struct Timing {
  Event ev[7];
  float ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool timed = false;                // the last run recorded its timing events
  bool timed_fine = false;           // ... those between the kernels of the walk stage as well
  bool timed_deliver = false;
};

struct Pairing {                   // the paired pump (result_host.h): this batch's step ran on the pump's own streams
  Event ev_walked;                   // recorded behind its walk launch on the chain; the tail waits for it (made on first use)
  Event ev_packed;                   // recorded behind its k_pack on the front; the chain waits for it (made on first use)
  bool borrowed = false;             // last_stream is one of the pump's streams (until the pump returns)
  uint32_t n_seeded = 0;             // diagnostics (km_batch_debug_counts): paired launches that seeded this batch so far
};

struct CapturedStep {              // KM_RUN_HIPGRAPH: km_batch_run captures, km_batch::drop_graph() forgets
  Graph graph;
  GraphExec gexec;
  int stages = 0;
  hipStream_t stream = nullptr;
};

}  // namespace

struct km_batch {
  kmjf* db = nullptr;
  km_params_t p{};
  uint32_t max_targets = 0;
  uint64_t max_bases = 0;
  int device = 0;
  // the target set (layout_targets)
  uint32_t n_targets = 0, max_len = 0;
  uint64_t total_bases = 0, total_ref = 0;
  // the last run
  bool ran_walk = false, ran_graph = false, synced = true;
  hipStream_t last_stream = nullptr;
  int graph_mode = 0;                  // 1 = duplicate check only (walk stage run alone)
  WalkArgs wa{};                       // geometry of the last launch
  GraphArgs ga{};
  uint32_t walk_lds = 0, graph_lds = 0, pure_lds = 0;

  Inputs in;
  PerTarget t;
  Delivery out;
  Probes probes;
  LargeTier big;
  VerboseLog log;
  NodePools nodes;
  PathPools paths;
  Timing tm;
  LaunchHints hints;
  Pairing pair;
  CapturedStep cap;                    // the last member: it goes before the buffers it uses

  void drop_graph() { cap.gexec.reset(); cap.graph.reset(); }
};

static uint64_t default_tail_bytes(const km_batch* b, uint64_t nodes, uint64_t extra) {
  return out_align(4 * nodes) + out_align(8 * extra) + 2 * out_align(4 * b->paths.path_pool) +
         out_align(8 * (b->paths.path_pool + 1)) + 2 * out_align(4 * b->paths.run_pool) + 256;
}

// Delivery buffers: region A for max_targets + `tail_need` bytes of tail.
static int ensure_out(km_batch* b, uint64_t tail_need) {
  const uint64_t need = out_layout(b->max_targets).a_bytes + tail_need;
  if (b->out.d_out && b->out.h_out && need <= b->out.out_cap) return KM_OK;
  b->out.h_out.reset();
  b->out.out_cap = 0;
  const uint64_t cap = need + need / 8;
  if (b->out.d_out.alloc(cap) != KM_OK) return fail(KM_E_NOMEM, "hipMalloc of the delivery buffer failed");
  if (hipHostMalloc((void**)&b->out.h_out.h, cap, hipHostMallocDefault) != hipSuccess) {
    b->out.h_out.h = nullptr;
    return fail(KM_E_NOMEM, "pinned allocation of %llu bytes failed", (unsigned long long)cap);
  }
  b->out.out_cap = cap;
  return KM_OK;
}

extern "C" int km_batch_create(kmjf_t* h, const km_params_t* params, uint32_t max_targets,
                               uint64_t max_total_bases, km_batch_t** out) {
  if (!h || !params || !out || !max_targets) return fail(KM_E_ARG, "bad argument");
  if (!h->d_slots) return fail(KM_E_STATE, "table not uploaded");
  // word offsets of the packed targets and of the flag bitmaps travel as 32-bit halves of one record word
  if (max_total_bases / 32 + 2ull * max_targets + 2 >= (1ull << 32)) return fail(KM_E_ARG, "batch too large (more than 2^37 bases)");
  HIPCHK(hipSetDevice(h->device));
  km_batch* b = new (std::nothrow) km_batch;
  if (!b) return fail(KM_E_NOMEM, "host allocation failed");
  b->db = h;
  b->p = *params;
  b->max_targets = max_targets;
  b->max_bases = max_total_bases;
  b->device = h->device;
  const CreateOptions opt = read_create_options();
  int rc = KM_OK;
  auto A = [&](int r) { if (rc == KM_OK) rc = r; };
  A(b->in.alloc(max_targets, max_total_bases));
  A(b->t.alloc(max_targets));
  A(b->out.alloc_scan(max_targets));
  if (rc == KM_OK && hipMemset(b->out.d_scan_ticket.p, 0, 4) != hipSuccess) rc = fail(KM_E_HIP, "hipMemset failed");
  A(b->probes.alloc(max_targets));
  b->big.configure(*params, opt);
  A(b->big.alloc(max_targets));
  A(b->log.alloc(max_targets));
  if (rc == KM_OK && hipMemset(b->log.d_loop_ctl.p, 0, 16) != hipSuccess) rc = fail(KM_E_HIP, "hipMemset failed");
  if (rc == KM_OK && hipMemset(b->big.d_big_ctl.p, 0, 32) != hipSuccess) rc = fail(KM_E_HIP, "hipMemset failed");
  A(b->nodes.alloc(max_total_bases + (uint64_t)max_targets * FAST_EXTRA + (uint64_t)b->big.big_entry * BIG_DEV_SLOTS));
  A(b->paths.alloc(max_targets, opt.small_pools));
  // the walk rarely adds more than a few nodes per target: the tail grows on demand
  if (rc == KM_OK) rc = ensure_out(b, default_tail_bytes(b, max_total_bases + 16ull * max_targets, 16ull * max_targets));
  if (rc == KM_OK) {
    if (hipEventCreateWithFlags(&b->out.ev_out.h, hipEventDisableTiming) != hipSuccess)
      rc = fail(KM_E_HIP, "stream/event creation failed");
  }
  if (rc == KM_OK) {
    for (int i = 0; i < 7; ++i)
      if (hipEventCreate(&b->tm.ev[i].h) != hipSuccess) rc = fail(KM_E_HIP, "hipEventCreate failed");
  }
  if (rc != KM_OK) { delete b; return rc; }
  *out = b;
  return KM_OK;
}

extern "C" int km_batch_destroy(km_batch_t* b) {
  if (!b) return KM_OK;
  (void)hipSetDevice(b->device);
  (void)hipDeviceSynchronize();
  delete b;
  return KM_OK;
}

// Every check of a new target set, before anything of the batch is touched: a rejected set leaves the
// batch as it was (same targets, same results on the next run).
static int check_targets(const km_batch* b, const uint64_t* offsets, uint32_t n) {
  if (n > b->max_targets) return fail(KM_E_ARG, "too many targets for this batch (%u > %u)", n, b->max_targets);
  for (uint32_t t = 0; t < n; ++t) {
    if (offsets[t + 1] < offsets[t]) return fail(KM_E_ARG, "offsets must be non-decreasing");
    if (offsets[t + 1] - offsets[t] > 0x7FFFFFFFull) return fail(KM_E_ARG, "target too long");
  }
  if (offsets[n] - offsets[0] > b->max_bases) return fail(KM_E_ARG, "too many bases for this batch");
  return KM_OK;
}

// A step of the old set may still be running (an un-awaited km_batch_run): its kernels and its delivery copy
// read the inputs and the layout that the new set overwrites.  The batch's streams are non-blocking, so
// neither hipMemcpy nor a synchronisation of the NULL stream orders against them: wait for the last one.
// After an awaited delivery (result_ready) nothing of this batch is left in that stream.
static int wait_in_flight(km_batch* b) {
  if (b->out.deliver_pending || (!b->synced && !b->out.result_ready)) HIPCHK(hipStreamSynchronize(b->last_stream));
  return KM_OK;
}

// Per-batch geometry + per-target node storage layout (offsets passed check_targets).
static int layout_targets(km_batch* b, const uint64_t* offsets, uint32_t n) {
  const uint64_t total = offsets[n] - offsets[0];
  const int k = b->db->k;
  b->in.h_toff.assign(n + 1, 0);
  b->in.h_woff.assign(n + 1, 0);
  b->in.h_fw_off.assign(n + 1, 0);
  b->in.h_item_off.assign(n + 1, 0);
  b->t.h_node_base.assign(n, 0);
  b->t.h_node_cap.assign(n, 0);
  uint64_t pool = (uint64_t)b->big.big_entry * BIG_DEV_SLOTS, total_ref = 0;   // (the large tier's region comes first)
  b->big.big_region = 0;
  uint32_t max_len = 0;
  for (uint32_t t = 0; t < n; ++t) {
    const uint64_t L = offsets[t + 1] - offsets[t];
    b->in.h_toff[t] = offsets[t] - offsets[0];
    b->in.h_woff[t + 1] = b->in.h_woff[t] + (L + 31) / 32 + 1;
    const uint32_t n_ref = (L >= (uint64_t)k) ? (uint32_t)(L - k + 1) : 0;
    b->in.h_fw_off[t + 1] = b->in.h_fw_off[t] + (n_ref + 31) / 32;
    b->in.h_item_off[t + 1] = b->in.h_item_off[t] + (n_ref + SEED_BLOCK - 1) / SEED_BLOCK;
    b->t.h_node_base[t] = pool;
    b->t.h_node_cap[t] = n_ref + FAST_EXTRA;
    pool += (uint64_t)n_ref + FAST_EXTRA;
    total_ref += n_ref;
    max_len = std::max<uint32_t>(max_len, (uint32_t)L);
  }
  b->in.h_toff[n] = total;
  b->t.h_node_base0 = b->t.h_node_base;
  b->t.h_node_cap0 = b->t.h_node_cap;
  b->t.node_pool0 = b->nodes.node_pool_used = pool;
  b->t.layout_moved = false;
  b->in.n_items = b->in.h_item_off[n];
  b->n_targets = n;
  b->total_bases = total;
  b->total_ref = total_ref;
  b->max_len = max_len;
  b->out.tail_guess = 4 * total_ref + total_ref / 2 + (64u << 10);
  b->in.h_packed.clear();
  return KM_OK;
}

static int push_layout(km_batch* b, hipStream_t st) {
  const uint32_t n = b->n_targets;
  b->drop_graph();                     // geometry and pointers may change with the targets
  {
    // tref[j] = distance of reference node j from the source along the reference chain,
    // accumulated exactly as Graph.py does: float32 0 + 0.01f, then + 0.01f per hop
    const uint32_t need = b->max_len + 2;
    if (b->in.d_tref.n < need) {
      KMCHK(b->in.d_tref.alloc(std::max<uint64_t>(need, 4096)));
      std::vector<float> h(b->in.d_tref.n);
      volatile float acc = 0.0f;
      for (size_t j = 0; j < h.size(); ++j) { acc = acc + 0.01f; h[j] = acc; }
      HIPCHK(hipMemcpy(b->in.d_tref.p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    }
  }
  HIPCHK(hipMemcpyAsync(b->in.d_toff.p, b->in.h_toff.data(), (uint64_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(b->in.d_woff.p, b->in.h_woff.data(), (uint64_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(b->in.d_fw_off.p, b->in.h_fw_off.data(), (uint64_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(b->in.d_item_off.p, b->in.h_item_off.data(), (uint64_t)(n + 1) * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(b->t.d_node_base.p, b->t.h_node_base.data(), (uint64_t)n * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(b->big.d_node_base0.p, b->t.h_node_base.data(), (uint64_t)n * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(b->t.d_node_cap.p, b->t.h_node_cap.data(), (uint64_t)n * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  b->ran_walk = b->ran_graph = false;
  b->synced = true;
  b->out.deliver_pending = b->out.result_ready = false;
  return KM_OK;
}

extern "C" int km_batch_set_targets(km_batch_t* b, const uint8_t* bases, const uint64_t* offsets,
                                    uint32_t n_targets) {
  if (!b || !offsets || (!bases && n_targets)) return fail(KM_E_ARG, "null argument");
  KMCHK(check_targets(b, offsets, n_targets));
  HIPCHK(hipSetDevice(b->device));
  KMCHK(wait_in_flight(b));
  KMCHK(layout_targets(b, offsets, n_targets));
  if (b->total_bases)
    HIPCHK(hipMemcpy(b->in.d_bases.p, bases + offsets[0], b->total_bases, hipMemcpyHostToDevice));
  return push_layout(b, nullptr);
}

extern "C" int km_batch_set_targets_dev(km_batch_t* b, const uint8_t* d_bases,
                                        const uint64_t* offsets_host, uint32_t n_targets, void* stream) {
  if (!b || !offsets_host || (!d_bases && n_targets)) return fail(KM_E_ARG, "null argument");
  KMCHK(check_targets(b, offsets_host, n_targets));
  HIPCHK(hipSetDevice(b->device));
  KMCHK(wait_in_flight(b));
  KMCHK(layout_targets(b, offsets_host, n_targets));
  hipStream_t st = (hipStream_t)stream;
  if (b->total_bases)
    HIPCHK(hipMemcpyAsync(b->in.d_bases.p, d_bases + offsets_host[0], b->total_bases,
                          hipMemcpyDeviceToDevice, st));
  return push_layout(b, st);
}

static void fill_walk_args(km_batch* b, WalkArgs& a) {
  memset(&a, 0, sizeof a);
  a.tab = view_of(b->db);
  a.bases = b->in.d_bases.p;
  a.toff = b->in.d_toff.p;
  a.packed = b->in.d_packed.p;
  a.woff = b->in.d_woff.p;
  a.n_targets = b->n_targets;
  a.ratio = b->p.ratio;
  a.n_cutoff = b->p.count;
  a.nc = (double)b->p.count;
  threshold_shortcut(a.ratio, a.n_cutoff, &a.thr_below, &a.thr_T);
  a.max_stack = b->p.max_stack;
  a.max_break = b->p.max_break;
  a.max_node = b->p.max_node;
  a.items = b->in.d_items.p;
  a.item_off = b->in.d_item_off.p;
  a.n_items = b->in.n_items;
  a.flagbits = b->in.d_flagbits.p;
  a.fw_off = b->in.d_fw_off.p;
  a.tflag = b->t.d_tflag.p;
  a.flagged = b->t.d_flagged.p;
  a.flag_rec = b->t.d_flag_rec.p;
  a.fast_extra = FAST_EXTRA;
  a.epi = nullptr;
  a.n_flagged = b->t.d_nflagged.p;
  a.list = b->t.d_flagged.p;
  a.n_list_dev = b->t.d_nflagged.p;
  a.n_list_host = 0;
  a.node_kmer = b->nodes.d_node_kmer.p;
  a.node_cnt = b->nodes.d_node_cnt.p;
  a.node_base = b->t.d_node_base.p;
  a.node_cap = b->t.d_node_cap.p;
  a.node_base0 = b->big.d_node_base0.p;
  a.big_ctl = b->big.big_entry ? b->big.d_big_ctl.p : nullptr;
  a.big_walk = b->big.d_big_walk.p;
  a.big_slots = BIG_DEV_SLOTS;
  a.big_entry = b->big.big_entry;
  a.big_region = b->big.big_region;
  a.big_prep = 0;
  a.loop_list = b->log.d_loop_list.p;
  a.loop_ctl = b->log.d_loop_ctl.p;
  a.loop_cap = LOOP_LOG_CAP;
  a.t_eremoved = b->log.d_t_eremoved.p;
  a.t_enonref = b->log.d_t_enonref.p;
  a.n_nodes = b->t.d_n_nodes.p;
  a.n_ref = b->t.d_n_ref.p;
  a.status = b->t.d_status.p;
  a.probes = reinterpret_cast<unsigned long long*>(b->probes.d_probes.p);
  a.dfs_probes = b->t.d_dfs_probes.p;
  a.fetches = reinterpret_cast<unsigned long long*>(b->probes.d_fetches.p);
  a.g_ws = nullptr;
  a.g_stride = 0;
  a.dbg = knobs().debug_flags & 0xFFu;          // timing ablations (diagnostics build only); results are invalid
  a.spec = knobs().speculate ? 1u : 0u;
  a.pool_counters = b->paths.d_counters.p;
}

static void fill_graph_args(km_batch* b, GraphArgs& g) {
  g.k = b->db->k;
  g.kmask = mask_bits(b->db->k);
  g.pmask = mask_bits(b->db->k - 1);
  g.tids = nullptr;
  g.work_list = b->t.d_flagged.p;
  g.work_n = b->t.d_nflagged.p;
  g.left = b->t.d_left.p;
  g.dfs_answers = 0;
  g.big_ctl = b->big.big_entry ? b->big.d_big_ctl.p : nullptr;
  g.big_graph = b->big.d_big_graph.p;
  g.big_slots = BIG_DEV_SLOTS;
  g.tids_n = nullptr;
  g.n_targets = b->n_targets;
  g.node_kmer = b->nodes.d_node_kmer.p;
  g.node_cnt = b->nodes.d_node_cnt.p;
  g.node_base = b->t.d_node_base.p;
  g.packed = b->in.d_packed.p;
  g.woff = b->in.d_woff.p;
  g.words_cap = 0;
  g.n_nodes = b->t.d_n_nodes.p;
  g.n_ref = b->t.d_n_ref.p;
  g.status = b->t.d_status.p;
  g.tflag = b->t.d_tflag.p;
  g.need_full = b->t.d_need_full.p;
  g.use_need_full = 0;
  g.hcap_pure = 0;
  g.g_status = b->t.d_gstatus.p;
  g.t_npaths = b->t.d_npaths.p;
  g.t_pathbase = b->t.d_pathbase.p;
  g.t_nruns = b->t.d_t_nruns.p;
  g.t_refmax = b->t.d_t_refmax.p;
  g.t_eremoved = b->log.d_t_eremoved.p;
  g.t_enonref = b->log.d_t_enonref.p;
  g.counters = b->paths.d_counters.p;
  g.path_pool = b->paths.path_pool;
  g.run_pool = b->paths.run_pool;
  g.p_target = b->paths.d_p_target.p;
  g.p_runbase = b->paths.d_p_runbase.p;
  g.p_nruns = b->paths.d_p_nruns.p;
  g.p_len = b->paths.d_p_len.p;
  g.p_mincov = b->paths.d_p_mincov.p;
  g.r_start = b->paths.d_r_start.p;
  g.r_len = b->paths.d_r_len.p;
  g.tref = b->in.d_tref.p;
  g.tref_len = (uint32_t)std::min<uint64_t>(b->in.d_tref.n, 0xFFFFFFFFull);
  g.g_ws = nullptr;
  g.g_stride = 0;
  g.dbg = knobs().debug_flags >> 8;
  if (b->graph_mode == 1) g.dbg = 1;       // duplicate check only
  if (g.dbg && !(g.dbg & 0x80u)) g.work_list = nullptr;   // every target goes through k_graph: no list
}

// ---- fast-tier geometry.  The LDS-resident kernels are sized for the longest target of the
// batch that still fits FAST_LDS_LIMIT; longer targets (and walks that outgrow the extra-node,
// branch-frame or stack-frame allowance) are flagged T_NEEDS_BIG by the kernels themselves, one
// by one, and finished by the large tier in km_batch_sync.  One long target does not demote the
// rest of its batch.
static void fast_geometry(km_batch* b) {
  const int k = b->db->k;
  const uint32_t max_nref = b->max_len >= (uint32_t)k ? b->max_len - k + 1 : 1;
  const FastGeometry fg = fast_tier_geometry(k, max_nref, b->p.max_stack, b->p.max_break);
  const uint32_t nref = fg.nref;
  WalkArgs& wa = b->wa;
  fill_walk_args(b, wa);
  wa.hs_cap = fg.hs_cap;
  wa.pcap = fg.pcap;
  wa.words_cap = fg.words_cap;
  wa.fcap = fg.fcap;
  wa.bcap = fg.bcap;
  wa.f_stride = walk_frame_bytes(wa.fcap);
  b->walk_lds = (uint32_t)walk_lds_bytes(wa.hs_cap, wa.words_cap, wa.bcap, wa.pcap, 2);
  GraphArgs& ga = b->ga;
  fill_graph_args(b, ga);
  ga.ncap = fg.ncap;
  ga.hcap = fg.hcap;
  ga.words_cap = wa.words_cap;
  b->graph_lds = (uint32_t)graph_ws_bytes<uint16_t>(ga.ncap, ga.hcap, ga.words_cap);
  ga.hcap_pure = 64;                                             // position table at load <= 1/4 (graph_kernel.h: k_graph_pure)
  while (ga.hcap_pure < 4 * (nref + 2)) ga.hcap_pure <<= 1;
  b->pure_lds = (uint32_t)pure_lds_bytes(ga.hcap_pure, ga.words_cap);
  if (b->pure_lds > FAST_LDS_LIMIT) {                            // all -> need_full
    ga.hcap_pure = 64;
    b->pure_lds = (uint32_t)pure_lds_bytes(64, ga.words_cap);
  }
  // the epilogue of k_dfs answers the regular flagged targets when the graph stage is wanted in full
  // (KM_EPILOGUE=0: diagnostics, everything through k_graph as in round 2)
  if (knobs().epilogue && b->graph_mode == 0 && ga.dbg == 0 && ga.work_list != nullptr) {
    EpiArgs e;
    memset(&e, 0, sizeof e);
    e.counters = ga.counters; e.path_pool = ga.path_pool; e.run_pool = ga.run_pool;
    e.p_target = ga.p_target; e.p_runbase = ga.p_runbase; e.p_nruns = ga.p_nruns; e.p_len = ga.p_len;
    e.p_mincov = ga.p_mincov; e.r_start = ga.r_start; e.r_len = ga.r_len;
    e.g_status = ga.g_status; e.t_npaths = ga.t_npaths; e.t_pathbase = ga.t_pathbase; e.t_nruns = ga.t_nruns;
    e.t_refmax = ga.t_refmax;
    e.t_eremoved = ga.t_eremoved; e.t_enonref = ga.t_enonref;
    e.left = b->t.d_left.p; e.n_left = b->t.d_nflagged.p + 2;
    if (!b->t.epi_valid || memcmp(&e, &b->t.h_epi, sizeof e) != 0) {
      if (hipMemcpy(b->t.d_epi.p, &e, sizeof e, hipMemcpyHostToDevice) == hipSuccess) { b->t.h_epi = e; b->t.epi_valid = true; }
      else b->t.epi_valid = false;
    }
    if (b->t.epi_valid) { wa.epi = b->t.d_epi.p; ga.dfs_answers = 1; }
  }
}

// LDS-tier graph kernels, instantiated for k = 31 where that is the database's k
static void launch_pure(km_batch* b, hipStream_t st, const GraphArgs& ga) {
  if (ga.k == 31) hipLaunchKernelGGL((k_graph_pure<31>), dim3(b->n_targets), dim3(64), b->pure_lds, st, ga);
  else hipLaunchKernelGGL((k_graph_pure<0>), dim3(b->n_targets), dim3(64), b->pure_lds, st, ga);
}
static void launch_graph(km_batch* b, hipStream_t st, const GraphArgs& ga) {
  const uint32_t grid = b->hints.graph_grid(b->n_targets, ga.work_list && ga.dfs_answers);
  if (ga.k == 31) hipLaunchKernelGGL((k_graph<false, 31>), dim3(grid), dim3(GRAPH_THREADS), b->graph_lds, st, ga);
  else hipLaunchKernelGGL((k_graph<false, 0>), dim3(grid), dim3(GRAPH_THREADS), b->graph_lds, st, ga);
}

// Graph stage on one stream: pure-chain pass, then the general kernel for the rest.
static int launch_graph_fast(km_batch* b, hipStream_t st) {
  HIPCHK(hipMemsetAsync(b->paths.d_counters.p, 0, (POOL_GROUPS * POOL_CTR_STRIDE + 16) * sizeof(unsigned long long), st));
  b->ga.use_need_full = 1;
  b->ga.dfs_answers = 0;                  // no k_dfs in this pass: every flagged target goes through k_graph
  HIPCHK(hipMemsetAsync(b->t.d_nflagged.p + 1, 0, sizeof(uint32_t), st));   // k_graph_pure appends its hand-overs again
  launch_pure(b, st, b->ga);
  launch_graph(b, st, b->ga);
  HIPCHK(hipGetLastError());
  return KM_OK;
}

static void launch_seed(uint32_t n_items, hipStream_t st, const WalkArgs& wa, bool count_fetches) {
  if (wa.stamps) hipLaunchKernelGGL((k_seed<true, 0, true>), dim3(n_items), dim3(SEED_BLOCK), 0, st, wa);   // KM_SEED_STAMPS diagnostics
  else if (knobs().seed_waves && !count_fetches && n_items < (1u << 29)) {
    const dim3 g((4 / SEED_WAVE_RUNS) * n_items), blk(64);
    if (wa.tab.k == 31) hipLaunchKernelGGL((k_seed_waves<31>), g, blk, SEED_WAVE_LDS, st, wa);
    else hipLaunchKernelGGL((k_seed_waves<0>), g, blk, SEED_WAVE_LDS, st, wa);
  }
  else if (wa.tab.k == 31) {
    if (count_fetches) hipLaunchKernelGGL((k_seed<false, 31, true>), dim3(n_items), dim3(SEED_BLOCK), 0, st, wa);
    else hipLaunchKernelGGL((k_seed<false, 31, false>), dim3(n_items), dim3(SEED_BLOCK), 0, st, wa);
  } else {
    if (count_fetches) hipLaunchKernelGGL((k_seed<false, 0, true>), dim3(n_items), dim3(SEED_BLOCK), 0, st, wa);
    else hipLaunchKernelGGL((k_seed<false, 0, false>), dim3(n_items), dim3(SEED_BLOCK), 0, st, wa);
  }
}

static void launch_dfs(km_batch* b, hipStream_t st, const WalkArgs& wa) {
  const uint32_t grid = b->hints.dfs_grid(b->n_targets);
  if (wa.tab.k == 31) hipLaunchKernelGGL((k_dfs<false, 31>), dim3(grid), dim3(64), b->walk_lds, st, wa);
  else hipLaunchKernelGGL((k_dfs<false, 0>), dim3(grid), dim3(64), b->walk_lds, st, wa);
}

// k_dfs and k_graph_pure as ONE launch (graph_kernel.h: k_dfs_pure): k_dfs's blocks first, then one block per target
// for the pure-chain pass, every block with k_dfs's LDS.  Only where that holds the pure-chain pass as well
// (fuses_pure): its position table has the power of two >= 4 (n_ref + 2) slots, k_dfs's the one >= 4 n_ref, so for a
// longest target of 511-512, 1 023-1 024, ... k-mers the pure pass needs MORE than the walk (10 384 against 9 712
// bytes at 512) and one launch would cost the walk blocks LDS, i.e. resident waves: such a batch keeps two launches.
static bool fuses_pure(const km_batch* b) { return b->pure_lds <= b->walk_lds; }
static void launch_dfs_pure(km_batch* b, hipStream_t st, const WalkArgs& wa, const GraphArgs& ga) {
  const uint32_t dfs_grid = b->hints.dfs_grid(b->n_targets);
  const uint32_t lds = b->walk_lds;
  if (wa.tab.k == 31) hipLaunchKernelGGL((k_dfs_pure<31>), dim3(dfs_grid + b->n_targets), dim3(64), lds, st, wa, ga, dfs_grid);
  else hipLaunchKernelGGL((k_dfs_pure<0>), dim3(dfs_grid + b->n_targets), dim3(64), lds, st, wa, ga, dfs_grid);
}

// Compaction kernels + ONE asynchronous copy of region A and the expected part of the tail into
// the pinned twin; km_batch_result() waits for ev_out and fetches what the guess left behind.
static int enqueue_deliver(km_batch* b, hipStream_t st, bool lean, bool count16 = false) {
  const double h_in = host_now_us();
  const uint32_t n = b->n_targets;
  b->out.lean = lean;
  b->out.count16 = count16;
  const OutLayout L = out_layout(n);
  b->out.result_ready = false;
  if (n == 0) {
    memset(b->out.h_out, 0, L.a_bytes + 64);
    reinterpret_cast<unsigned long long*>(b->out.h_out.h)[OT_TAIL_BYTES] = 16;
    reinterpret_cast<unsigned long long*>(b->out.h_out.h)[OT_SERIAL] = ++b->out.serial;
    b->out.copied_tail = 16;
    b->out.deliver_pending = true;
    HIPCHK(hipEventRecord(b->out.ev_out, st));
    return KM_OK;
  }
  OutArgs oa;
  memset(&oa, 0, sizeof oa);
  oa.n_targets = n;
  oa.ran_graph = (b->ran_graph && b->graph_mode == 0) ? 1u : 0u;
  oa.lean = lean ? 1u : 0u;
  oa.count16 = count16 ? 1u : 0u;
  oa.count_fetches = b->probes.count_fetches ? 1u : 0u;
  oa.serial = ++b->out.serial;
  oa.big_ctl = b->big.big_entry ? b->big.d_big_ctl.p : nullptr;
  oa.big_slots = BIG_DEV_SLOTS;
  oa.status = b->t.d_status.p; oa.g_status = b->t.d_gstatus.p; oa.n_nodes = b->t.d_n_nodes.p; oa.n_ref = b->t.d_n_ref.p;
  oa.t_npaths = b->t.d_npaths.p; oa.t_pathbase = b->t.d_pathbase.p; oa.t_nruns = b->t.d_t_nruns.p;
  oa.t_refmax = b->t.d_t_refmax.p;
  oa.probes = reinterpret_cast<unsigned long long*>(b->probes.d_probes.p);
  oa.dfs_probes = b->t.d_dfs_probes.p;
  oa.fetches = reinterpret_cast<unsigned long long*>(b->probes.d_fetches.p);
  oa.pool_overflow = b->paths.d_counters.p + POOL_GROUPS * POOL_CTR_STRIDE;
  oa.n_flagged = b->t.d_nflagged.p;
  oa.node_base = b->t.d_node_base.p; oa.node_kmer = b->nodes.d_node_kmer.p; oa.node_cnt = b->nodes.d_node_cnt.p;
  oa.p_runbase = b->paths.d_p_runbase.p; oa.p_nruns = b->paths.d_p_nruns.p; oa.p_len = b->paths.d_p_len.p;
  oa.p_mincov = b->paths.d_p_mincov.p; oa.r_start = b->paths.d_r_start.p; oa.r_len = b->paths.d_r_len.p;
  oa.loc = b->out.d_loc.p; oa.cnt = b->out.d_cnt4.p; oa.blk_tot = b->out.d_blk_tot.p; oa.psort = b->paths.d_psort.p;
  oa.blk_base = b->out.d_blk_base.p; oa.scan_ticket = b->out.d_scan_ticket.p;
  // KM_DELIVER_ZEROCOPY=1: the delivery kernels store straight into the pinned host buffer
  // (PCIe writes from the CUs, no copy command on the stream); default: device buffer + one DMA
  const bool zero_copy = knobs().zero_copy;
  unsigned char* dst = zero_copy ? b->out.h_out : b->out.d_out;
  oa.totals = reinterpret_cast<unsigned long long*>(dst + L.totals);
  oa.o_status = reinterpret_cast<uint32_t*>(dst + L.status);
  oa.o_nref = reinterpret_cast<uint32_t*>(dst + L.n_ref);
  oa.o_probes = reinterpret_cast<uint64_t*>(dst + L.probes);
  oa.o_node_off = reinterpret_cast<uint64_t*>(dst + L.node_off);
  oa.o_extra_off = reinterpret_cast<uint64_t*>(dst + L.extra_off);
  oa.o_path_off = reinterpret_cast<uint32_t*>(dst + L.path_off);
  oa.o_refmax = reinterpret_cast<uint32_t*>(dst + L.ref_max);
  oa.o_esc_node = reinterpret_cast<uint64_t*>(dst + L.esc_node);
  oa.o_esc_value = reinterpret_cast<uint32_t*>(dst + L.esc_value);
  oa.tail = dst + L.a_bytes;
  oa.tail_cap = b->out.out_cap - L.a_bytes;
  const int dbg_deliver = knobs().debug_deliver;   // timing ablations (diagnostics build only)
  const bool host_trace = knobs().host_trace;      // diagnostics: host time of the calls below
  const double h0 = host_trace ? host_now_us() : 0;
  if (!(dbg_deliver & 2)) {
    hipLaunchKernelGGL(k_out_scan, dim3((n + OUT_SCAN_THREADS - 1) / OUT_SCAN_THREADS), dim3(OUT_SCAN_THREADS), 0, st, oa);
    hipLaunchKernelGGL(k_out_pack, dim3(n), dim3(64), 0, st, oa);
  }
  HIPCHK(hipGetLastError());
  const double h1 = host_trace ? host_now_us() : 0;
  if (b->tm.timed) HIPCHK(hipEventRecord(b->tm.ev[5], st));
  uint64_t guess = std::min<uint64_t>(oa.tail_cap, b->out.tail_guess);
  if (zero_copy) guess = oa.tail_cap;            // everything is already where it belongs
  else if (!(dbg_deliver & 1)) {
    HIPCHK(hipMemcpyAsync(b->out.h_out, b->out.d_out, L.a_bytes + guess, hipMemcpyDeviceToHost, st));
  }
  const double h2 = host_trace ? host_now_us() : 0;
  if (b->tm.timed) HIPCHK(hipEventRecord(b->tm.ev[6], st));
  b->tm.timed_deliver = b->tm.timed;
  HIPCHK(hipEventRecord(b->out.ev_out, st));
  if (host_trace) fprintf(stderr, "[km host] deliver: kernels %.1f us, memcpyAsync %.1f us, event %.1f us, whole %.1f\n", h1 - h0, h2 - h1, host_now_us() - h2, host_now_us() - h_in);
  b->out.copied_tail = guess;
  b->out.deliver_pending = true;
  return KM_OK;
}

// The large tier of an earlier run moved some targets to bigger node storage: back to the layout of
// layout_targets (a step replayed on the same targets starts from the same state).  The device arrays are reset
// by k_pack itself (node_base0); this is the host's mirror of them.
static void restore_layout(km_batch* b) {
  if (!b->t.layout_moved) return;
  b->drop_graph();
  b->t.h_node_base = b->t.h_node_base0;
  b->t.h_node_cap = b->t.h_node_cap0;
  b->nodes.node_pool_used = b->t.node_pool0;
  b->t.layout_moved = false;
}

// Geometry of the large-tier walk (global-memory workspaces sized for the reference's own bound on a walk)
static int big_walk_geometry(km_batch* b, WalkArgs& a) {
  const int k = b->db->k;
  const uint32_t max_nref = b->max_len >= (uint32_t)k ? b->max_len - k + 1 : 1;
  const uint64_t max_nodes = std::max<uint64_t>(max_nref, (uint64_t)b->p.max_node + b->p.max_stack) + 1;
  const uint64_t hs = 2 * (max_nodes + b->p.max_stack + 64);
  if (hs > 0x7FFFFF00ull) return fail(KM_E_ARG, "node limit too large");
  a.hs_cap = round_up((uint32_t)hs, 64);
  a.pcap = walk_pcap(max_nref);
  a.words_cap = words_cap_for(b->max_len);
  a.fcap = round_up(b->p.max_stack + 2, 2);
  a.bcap = b->p.max_break + 1;
  a.g_stride = walk_ws_bytes(a.hs_cap, a.words_cap, a.fcap, a.bcap, a.pcap);
  return KM_OK;
}

// ... and of its graph kernel, for targets of up to `ncap` nodes
static void big_graph_geometry(const km_batch* b, GraphArgs& g, uint32_t ncap) {
  g.ncap = ncap;
  g.hcap = graph_hcap(ncap);
  g.words_cap = words_cap_for(b->max_len);
  g.g_stride = graph_ws_bytes<uint32_t>(g.ncap, g.hcap, g.words_cap);
}

// Workspaces of the device's own large tier (allocated before a step is launched or captured; they grow with the
// longest target of the batch)
static int ensure_bigdev_ws(km_batch* b) {
  if (!b->big.big_entry || !b->big.bigdev_armed) return KM_OK;
  WalkArgs a;
  memset(&a, 0, sizeof a);
  KMCHK(big_walk_geometry(b, a));
  KMCHK(b->big.d_bigdev_walk_ws.alloc((uint64_t)BIG_DEV_SLOTS * a.g_stride));
  GraphArgs g{};
  big_graph_geometry(b, g, b->big.big_entry + 2);
  return b->big.d_bigdev_graph_ws.alloc((uint64_t)BIG_DEV_SLOTS * g.g_stride);
}

// The device's own large tier, walk: one more launch behind the fast k_dfs, in its stream — BIG_DEV_SLOTS single-wave
// blocks that leave at once unless the fast kernel appended targets to the list (WalkArgs::big_ctl).
static int launch_big_walk_dev(km_batch* b, hipStream_t st) {
  if (!b->big.big_entry || !b->big.bigdev_armed) return KM_OK;
  WalkArgs a;
  fill_walk_args(b, a);
  KMCHK(big_walk_geometry(b, a));
  if (b->big.d_bigdev_walk_ws.n < (uint64_t)BIG_DEV_SLOTS * a.g_stride) return fail(KM_E_STATE, "large-tier workspace missing");
  a.g_ws = b->big.d_bigdev_walk_ws.p;
  a.list = b->big.d_big_walk.p;
  a.n_list_dev = b->big.d_big_ctl.p;
  a.n_list_host = 0;
  a.big_prep = 1;
  a.stamps = nullptr;
  hipLaunchKernelGGL((k_dfs<true, 0>), dim3(BIG_DEV_SLOTS), dim3(64), 0, st, a);
  return KM_OK;
}
// ... and graph: behind the fast k_graph, over what it (or the large-tier walk's results) could not hold
static int launch_big_graph_dev(km_batch* b, hipStream_t st) {
  if (!b->big.big_entry || !b->big.bigdev_armed) return KM_OK;
  GraphArgs g;
  fill_graph_args(b, g);
  big_graph_geometry(b, g, b->big.big_entry + 2);
  if (b->big.d_bigdev_graph_ws.n < (uint64_t)BIG_DEV_SLOTS * g.g_stride) return fail(KM_E_STATE, "large-tier workspace missing");
  g.g_ws = b->big.d_bigdev_graph_ws.p;
  g.tids = b->big.d_big_graph.p;
  g.tids_n = b->big.d_big_ctl.p + 1;
  hipLaunchKernelGGL((k_graph<true, 0>), dim3(BIG_DEV_SLOTS), dim3(GRAPH_THREADS), 0, st, g);
  return KM_OK;
}

// What km_batch_run's `stages` asks for, decoded once.  (What is left of KM_RUN_SERIAL: a cached captured step is
// not replayed.)
struct RunFlags {
  int stages;                          // KM_STAGE_WALK | KM_STAGE_GRAPH
  bool hipgraph, serial, deliver, lean, count16, count_fetches, timed, timed_fine;
  explicit RunFlags(int s)
      : stages(s & (KM_STAGE_WALK | KM_STAGE_GRAPH)), hipgraph(s & KM_RUN_HIPGRAPH), serial(s & KM_RUN_SERIAL),
        deliver(s & KM_RUN_DELIVER), lean(s & KM_DELIVER_LEAN), count16(s & KM_DELIVER_COUNT16),
        count_fetches(s & KM_RUN_COUNT_FETCHES), timed(s & KM_RUN_TIMED), timed_fine(timed && !(s & KM_RUN_TIMED_STAGES)) {}
};

// ---- the step in pieces.  km_batch_run calls them in order on one stream; the paired pump (result_host.h) enqueues
// them at different moments and on different streams: front (step_open: restore_layout, geometry; step_pack: k_pack), middle
// (step_seed: k_seed; step_walk: k_dfs_pure) and back (step_back: the large-tier launches, k_graph, the delivery).
// What every run resets first.
static void step_begin(km_batch* b, hipStream_t st, const RunFlags& f) {
  b->last_stream = st;
  if (f.stages & KM_STAGE_WALK) b->probes.count_fetches = f.count_fetches;
  b->out.deliver_pending = b->out.result_ready = false;
  b->tm.timed_deliver = false;
  b->big.n_big = 0;
}
// Geometry of the step and the workspaces that follow from it.
static int step_geometry(km_batch* b, const RunFlags& f) {
  b->graph_mode = (f.stages & KM_STAGE_GRAPH) ? 0 : 1;
  fast_geometry(b);
  WalkArgs& wa = b->wa;
  KMCHK(b->t.d_frames.alloc((uint64_t)b->n_targets * wa.f_stride));
  KMCHK(ensure_bigdev_ws(b));
  wa.f_ws = b->t.d_frames.p;
  wa.stamps = nullptr;
  if (knobs().seed_stamps) {
    KMCHK(b->probes.d_stamps.alloc(16ull * (SEED_BLOCK / 64) * (b->in.n_items + 4)));
    wa.stamps = b->probes.d_stamps.p;
  }
  b->tm.timed = f.timed;
  b->tm.timed_fine = f.timed_fine;
  return KM_OK;
}
// k_pack, the first kernel of a step (it also zeroes the path-pool counters of the graph kernels: no fill command)
static int step_pack(km_batch* b, hipStream_t st) {
  if (b->tm.timed) HIPCHK(hipEventRecord(b->tm.ev[0], st));
  hipLaunchKernelGGL(k_pack, dim3((b->n_targets + PACK_WAVES - 1) / PACK_WAVES), dim3(64 * PACK_WAVES), 0, st, b->wa);
  if (b->tm.timed && b->tm.timed_fine) HIPCHK(hipEventRecord(b->tm.ev[3], st));
  return KM_OK;
}
// what a plain step (non-empty batch, walk stage) does before its first launch: afterwards its geometry is known
static int step_open(km_batch* b, hipStream_t st, const RunFlags& f) {
  step_begin(b, st, f);
  restore_layout(b);
  return step_geometry(b, f);
}
// front of a plain step on `st`
static int step_front(km_batch* b, hipStream_t st, const RunFlags& f) {
  KMCHK(step_open(b, st, f));
  return step_pack(b, st);
}
static int step_seed(km_batch* b, hipStream_t st) {
  if (b->in.n_items)
    launch_seed(b->in.n_items, st, b->wa, b->probes.count_fetches);
  if (b->tm.timed && b->tm.timed_fine) HIPCHK(hipEventRecord(b->tm.ev[4], st));
  return KM_OK;
}
// May this step's k_dfs and k_graph_pure be one launch?  (the walk-only run's k_graph_pure answers nothing, ga.dbg;
// the diagnostics measure k_dfs by itself)
static bool step_fuses(const km_batch* b, const RunFlags& f) {
  return knobs().fuse_pure && !f.serial && (f.stages & KM_STAGE_GRAPH) && b->ga.dbg == 0 && !knobs().dfs_replay &&
         b->wa.stamps == nullptr && b->wa.dbg == 0 && fuses_pure(b);
}
// k_dfs (with k_graph_pure in its launch where step_fuses): *fused says which
static int step_walk(km_batch* b, hipStream_t st, const RunFlags& f, bool* fused) {
  WalkArgs& wa = b->wa;
  GraphArgs& ga = b->ga;
  // a batch's kernels run in ONE stream, in order: batches overlap with each other, every launch stream on a
  // hardware queue of its own (see "streams" in host_common.h).  k_graph_pure needs nothing of k_dfs and runs
  // beside it — rounds 2-3 on a side stream per batch, since round 6 as blocks of k_dfs's own launch;
  // KM_RUN_SERIAL selects one launch each, k_graph_pure behind k_dfs.
  ga.use_need_full = 1;
  // diagnostics (KM_DFS_REPLAY=1|2): k_dfs twice, the SECOND launch is the one timed — its instruction
  // cache is warm; with 2 a 1 GiB memset in between flushes L2 / Infinity Cache (data cold again)
  const int dfs_replay = knobs().dfs_replay;
  if (dfs_replay) {
    launch_dfs(b, st, wa);
    if (dfs_replay == 2) {
      static void* scratch = nullptr;
      if (!scratch) HIPCHK(hipMalloc(&scratch, 1ull << 30));
      HIPCHK(hipMemsetAsync(scratch, 0, 1ull << 30, st));
    }
    if (b->tm.timed) HIPCHK(hipEventRecord(b->tm.ev[4], st));
  }
  *fused = step_fuses(b, f);
  if (*fused) launch_dfs_pure(b, st, wa, ga);
  else launch_dfs(b, st, wa);
  HIPCHK(hipGetLastError());
  if (b->tm.timed) HIPCHK(hipEventRecord(b->tm.ev[1], st));
  return KM_OK;
}
// what follows the walk launch up to the end of the graph stage: [k_dfs of the device's large tier], k_graph_pure
// unless it ran in k_dfs's launch, k_graph, [k_graph of the device's large tier]
static int step_graph(km_batch* b, hipStream_t st, bool fused) {
  b->big.bigdev_ran = b->big.big_entry && b->big.bigdev_armed;
  KMCHK(launch_big_walk_dev(b, st));
  if (!fused) launch_pure(b, st, b->ga);
  launch_graph(b, st, b->ga);
  KMCHK(launch_big_graph_dev(b, st));
  HIPCHK(hipGetLastError());
  b->ran_walk = true;
  b->ran_graph = false;
  return KM_OK;
}
// back of a plain step: step_graph and the delivery
static int step_back(km_batch* b, hipStream_t st, const RunFlags& f, bool fused) {
  KMCHK(step_graph(b, st, fused));
  b->ran_graph = true;
  b->synced = false;
  return f.deliver ? enqueue_deliver(b, st, f.lean, f.count16) : KM_OK;
}
// middle and back of a plain step on `st`, its front enqueued there
static int step_rest(km_batch* b, hipStream_t st, const RunFlags& f) {
  bool fused = false;
  KMCHK(step_seed(b, st));
  KMCHK(step_walk(b, st, f, &fused));
  return step_back(b, st, f, fused);
}

// The middle of TWO steps in one launch (graph_kernel.h: k_dfs_pure_seed): k_dfs and k_graph_pure of `prev`, whose
// k_seed has run, and k_seed of `next`, whose k_pack is in front of this launch on `st` (or `st` waits for its event).
// The caller has checked that the two may share it (result_host.h: pairs_with).  The grid's order: walk blocks, seed
// blocks, pure-chain blocks (pair_roles.h; KM_PAIR_PURE_LAST=0: walk, pure-chain, seeds as in round 7).
static int launch_dfs_pure_seed(km_batch* prev, km_batch* next, hipStream_t st) {
  prev->ga.use_need_full = 1;
  const uint32_t dfs_grid = prev->hints.dfs_grid(prev->n_targets), n_pure = prev->n_targets;
  const uint64_t grid = (uint64_t)dfs_grid + n_pure + (uint64_t)(4 / SEED_WAVE_RUNS) * next->in.n_items;
  if (grid > 0x7FFFFFFFull || prev->walk_lds < SEED_WAVE_LDS) return fail(KM_E_STATE, "paired launch out of range");
  const uint32_t pure_last = knobs().pair_pure_last ? 1u : 0u;
  if (prev->wa.tab.k == 31)
    hipLaunchKernelGGL((k_dfs_pure_seed<31>), dim3((uint32_t)grid), dim3(64), prev->walk_lds, st, prev->wa, prev->ga, dfs_grid, n_pure, next->wa, pure_last);
  else
    hipLaunchKernelGGL((k_dfs_pure_seed<0>), dim3((uint32_t)grid), dim3(64), prev->walk_lds, st, prev->wa, prev->ga, dfs_grid, n_pure, next->wa, pure_last);
  HIPCHK(hipGetLastError());
  return KM_OK;
}

// One step.  In stream order: k_pack (which also zeroes the path-pool counters), k_seed, k_dfs_pure (k_dfs and
// k_graph_pure in one launch), [k_dfs of the device's large tier], k_graph, [k_graph of the device's large tier], then
// the delivery (enqueue_deliver) when asked for.  With KM_RUN_SERIAL ("every kernel alone"), KM_FUSE_PURE=0, a
// walk-only run or the k_dfs diagnostics: k_dfs, [large-tier k_dfs], k_graph_pure, k_graph, ... as before round 6.
// With KM_RUN_HIPGRAPH everything before the delivery is captured once and replayed.  A graph-only run (no k_pack)
// zeroes the counters with a fill command of its own (launch_graph_fast).
extern "C" int km_batch_run(km_batch_t* b, int stages, void* stream) {
  if (!b) return fail(KM_E_ARG, "null argument");
  const bool host_trace = knobs().host_trace;      // diagnostics: host time of the sections
  double ht[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  ht[0] = host_trace ? host_now_us() : 0;
  HIPCHK(hipSetDevice(b->device));
  hipStream_t st = (hipStream_t)stream;
  const RunFlags f(stages);
  step_begin(b, st, f);
  if (!b->n_targets) {
    b->ran_walk = true;
    b->ran_graph = (f.stages & KM_STAGE_GRAPH) != 0;
    b->graph_mode = b->ran_graph ? 0 : 1;
    b->synced = true;
    return f.deliver ? enqueue_deliver(b, st, f.lean, f.count16) : KM_OK;
  }
  if (f.stages & KM_STAGE_WALK) restore_layout(b);
  ht[1] = host_trace ? host_now_us() : 0;
  if (f.hipgraph && !f.serial && b->cap.gexec && b->cap.stages == f.stages && b->cap.stream == st) {
    HIPCHK(hipGraphLaunch(b->cap.gexec, st));
    b->big.bigdev_ran = b->big.big_entry && b->big.bigdev_armed;      // (a flip of that state drops the captured step)
    b->ran_walk = true;
    b->ran_graph = true;
    b->synced = false;
    b->tm.timed = false;
    return f.deliver ? enqueue_deliver(b, st, f.lean, f.count16) : KM_OK;
  }

  KMCHK(step_geometry(b, f));
  bool graph_launched = false;
  // a captured step has no host round trips inside
  const bool capturing = f.hipgraph && st != nullptr && (f.stages & KM_STAGE_WALK);   // the NULL stream cannot be captured
  if (capturing) {
    b->tm.timed = false;
    b->drop_graph();
    HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  }
  ht[2] = host_trace ? host_now_us() : 0;
  if (f.stages & KM_STAGE_WALK) {
    bool fused = false;
    KMCHK(step_pack(b, st));
    KMCHK(step_seed(b, st));
    KMCHK(step_walk(b, st, f, &fused));
    KMCHK(step_graph(b, st, fused));
    graph_launched = true;
  } else if (!b->ran_walk) {
    return fail(KM_E_STATE, "graph stage requested before the walk stage");
  } else {
    for (int i : {0, 3, 4, 1})
      if (b->tm.timed) HIPCHK(hipEventRecord(b->tm.ev[i], st));
  }
  // the graph kernels also host the duplicate-k-mer check, so they always run
  // (graph_mode 1 = stop after that check)
  if (!graph_launched) KMCHK(launch_graph_fast(b, st));
  b->ran_graph = true;                      // graph_mode says how far it went
  if (b->tm.timed) HIPCHK(hipEventRecord(b->tm.ev[2], st));
  if (capturing) {
    HIPCHK(hipStreamEndCapture(st, &b->cap.graph.h));
    HIPCHK(hipGraphInstantiate(&b->cap.gexec.h, b->cap.graph, nullptr, nullptr, 0));
    b->cap.stages = f.stages;
    b->cap.stream = st;
    HIPCHK(hipGraphLaunch(b->cap.gexec, st));
  }
  b->synced = false;
  if (host_trace) ht[4] = host_now_us();
  const int rc_deliver = f.deliver ? enqueue_deliver(b, st, f.lean, f.count16) : KM_OK;
  if (host_trace)
    fprintf(stderr, "[km host] run: setdevice+layout %.1f us, geometry %.1f, launches %.1f, delivery %.1f, whole call %.1f\n",
            ht[1] - ht[0], ht[2] - ht[1], ht[4] - ht[2], host_now_us() - ht[4], host_now_us() - ht[0]);
  return rc_deliver;
}

static int pull_status(km_batch* b, hipStream_t st) {
  const uint32_t n = b->n_targets;
  b->t.h_status.resize(n); b->t.h_gstatus.assign(n, 0); b->t.h_n_nodes.resize(n); b->t.h_n_ref.resize(n);
  b->t.h_npaths.assign(n, 0); b->t.h_pathbase.assign(n, 0);
  HIPCHK(hipMemcpyAsync(b->t.h_status.data(), b->t.d_status.p, (uint64_t)n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(b->t.h_n_nodes.data(), b->t.d_n_nodes.p, (uint64_t)n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(b->t.h_n_ref.data(), b->t.d_n_ref.p, (uint64_t)n * 4, hipMemcpyDeviceToHost, st));
  if (b->ran_graph) {
    HIPCHK(hipMemcpyAsync(b->t.h_gstatus.data(), b->t.d_gstatus.p, (uint64_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(b->t.h_npaths.data(), b->t.d_npaths.p, (uint64_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(b->t.h_pathbase.data(), b->t.d_pathbase.p, (uint64_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&b->paths.h_overflow, b->paths.d_counters.p + POOL_GROUPS * POOL_CTR_STRIDE, 8, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  return KM_OK;
}

// The host's large tier runs its `nb` targets in slices, so that the workspace (`stride` bytes per target) stays
// bounded: launch(ws, first, count) enqueues one slice, which is then checked and awaited.
template <typename Launch>
static int run_in_slices(km_batch* b, uint32_t nb, uint64_t stride, hipStream_t st, Launch launch) {
  const uint64_t budget = 8ull << 30;
  const uint32_t per = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(nb, budget / stride));
  KMCHK(b->big.d_big_ws.alloc((uint64_t)per * stride));
  for (uint32_t s = 0; s < nb; s += per) {
    launch(b->big.d_big_ws.p, s, std::min(per, nb - s));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
  }
  return KM_OK;
}

// Large tier: rerun the listed targets with global-memory workspaces.
static int run_big_walk(km_batch* b, const std::vector<uint32_t>& ids, hipStream_t st) {
  const uint32_t nb = (uint32_t)ids.size();
  const int k = b->db->k;
  b->drop_graph();                    // a captured step holds the addresses that change below
  b->t.layout_moved = true;
  if (b->big.big_entry) {                 // the device's own large tier may have re-homed targets of this run
    HIPCHK(hipMemcpyAsync(b->t.h_node_base.data(), b->t.d_node_base.p, (uint64_t)b->n_targets * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(b->t.h_node_cap.data(), b->t.d_node_cap.p, (uint64_t)b->n_targets * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  // per-target node storage big enough for the reference's own bound
  uint64_t extra = 0;
  std::vector<uint64_t> old_base;
  for (uint32_t t : ids) old_base.push_back(b->t.h_node_base[t]);
  for (uint32_t t : ids) {
    const uint64_t L = b->in.h_toff[t + 1] - b->in.h_toff[t];
    const uint32_t n_ref = (L >= (uint64_t)k) ? (uint32_t)(L - k + 1) : 0;
    const uint64_t cap = std::max<uint64_t>(n_ref, (uint64_t)b->p.max_node + b->p.max_stack) + 1;
    if (cap > 0x7FFFFFFFull) return fail(KM_E_ARG, "node limit too large");
    b->t.h_node_base[t] = b->nodes.node_pool_used + extra;
    b->t.h_node_cap[t] = (uint32_t)cap;
    extra += cap;
  }
  const uint64_t need = b->nodes.node_pool_used + extra;
  if (need > b->nodes.d_node_kmer.n) {
    // grow the pools, keeping the fast-tier results (the old pools go right after the copy)
    DevBuf<uint64_t> nk; DevBuf<uint32_t> nc;
    KMCHK(nk.alloc(need));
    KMCHK(nc.alloc(need));
    HIPCHK(hipMemcpyAsync(nk.p, b->nodes.d_node_kmer.p, b->nodes.node_pool_used * 8, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(nc.p, b->nodes.d_node_cnt.p, b->nodes.node_pool_used * 4, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    b->nodes.d_node_kmer = std::move(nk); b->nodes.d_node_cnt = std::move(nc);
  }
  b->nodes.node_pool_used = need;
  // the seed kernel's results (the counts of the target's own k-mers) move to the new storage
  for (size_t q = 0; q < ids.size(); ++q) {
    const uint32_t t = ids[q];
    const uint64_t nref = b->t.h_n_ref[t];
    if (!nref) continue;
    HIPCHK(hipMemcpyAsync(b->nodes.d_node_cnt.p + b->t.h_node_base[t], b->nodes.d_node_cnt.p + old_base[q], nref * 4,
                          hipMemcpyDeviceToDevice, st));
  }
  HIPCHK(hipMemcpyAsync(b->t.d_node_base.p, b->t.h_node_base.data(), (uint64_t)b->n_targets * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(b->t.d_node_cap.p, b->t.h_node_cap.data(), (uint64_t)b->n_targets * 4, hipMemcpyHostToDevice, st));
  KMCHK(b->big.d_big_ids.alloc(nb));
  HIPCHK(hipMemcpyAsync(b->big.d_big_ids.p, ids.data(), (uint64_t)nb * 4, hipMemcpyHostToDevice, st));

  WalkArgs a;
  fill_walk_args(b, a);
  a.n_list_dev = nullptr;
  a.big_ctl = nullptr;                // (this pass IS the fallback)
  KMCHK(big_walk_geometry(b, a));
  return run_in_slices(b, nb, a.g_stride, st, [&](unsigned char* ws, uint32_t first, uint32_t cnt) {
    a.g_ws = ws;
    a.list = b->big.d_big_ids.p + first;
    a.n_list_host = cnt;
    hipLaunchKernelGGL((k_dfs<true, 0>), dim3(cnt), dim3(64), 0, st, a);
  });
}

// `by_edges`: workspaces sized by the most edges a target can have, 4 per node + 2, not by its nodes.  k_graph keeps
// one candidate edge per path in a list of ncap entries; a dense graph (small k: most of the 4^k k-mers are nodes,
// every node has several successors) has more of them than nodes and gets T_INTERNAL from the first pass.
static int run_big_graph(km_batch* b, const std::vector<uint32_t>& ids, hipStream_t st, bool by_edges = false) {
  const uint32_t nb = (uint32_t)ids.size();
  KMCHK(b->big.d_big_ids.alloc(nb));
  HIPCHK(hipMemcpyAsync(b->big.d_big_ids.p, ids.data(), (uint64_t)nb * 4, hipMemcpyHostToDevice, st));
  uint32_t max_nodes = 0;
  for (uint32_t t : ids) max_nodes = std::max(max_nodes, b->t.h_n_nodes[t]);
  GraphArgs g;
  fill_graph_args(b, g);
  if (by_edges && max_nodes > 0x0FFFFFF0u) return fail(KM_E_NOMEM, "graph too large");
  big_graph_geometry(b, g, by_edges ? 4 * (max_nodes + 2) : max_nodes + 2);
  return run_in_slices(b, nb, g.g_stride, st, [&](unsigned char* ws, uint32_t first, uint32_t cnt) {
    g.g_ws = ws;
    g.tids = b->big.d_big_ids.p + first;
    hipLaunchKernelGGL((k_graph<true, 0>), dim3(cnt), dim3(GRAPH_THREADS), 0, st, g);
  });
}

static int relaunch_fast_graph(km_batch* b, hipStream_t st) {
  // same geometry as the run, new pool sizes / addresses
  const GraphArgs old = b->ga;
  fill_graph_args(b, b->ga);
  b->ga.ncap = old.ncap; b->ga.hcap = old.hcap; b->ga.words_cap = old.words_cap; b->ga.hcap_pure = old.hcap_pure;
  KMCHK(launch_graph_fast(b, st));
  HIPCHK(hipStreamSynchronize(st));
  return KM_OK;
}

static void read_timings(km_batch* b) {
  for (float& v : b->tm.ms) v = 0.0f;
  if (!b->tm.timed) return;
  (void)hipEventElapsedTime(&b->tm.ms[0], b->tm.ev[0], b->tm.ev[1]);
  (void)hipEventElapsedTime(&b->tm.ms[1], b->tm.ev[1], b->tm.ev[2]);
  (void)hipEventElapsedTime(&b->tm.ms[2], b->tm.ev[0], b->tm.ev[2]);
  if (b->tm.timed_fine) {
    (void)hipEventElapsedTime(&b->tm.ms[3], b->tm.ev[3], b->tm.ev[4]);
    (void)hipEventElapsedTime(&b->tm.ms[4], b->tm.ev[0], b->tm.ev[3]);
    (void)hipEventElapsedTime(&b->tm.ms[5], b->tm.ev[4], b->tm.ev[1]);
  }
  if (b->tm.timed_deliver) {
    (void)hipEventElapsedTime(&b->tm.ms[6], b->tm.ev[2], b->tm.ev[5]);
    (void)hipEventElapsedTime(&b->tm.ms[7], b->tm.ev[5], b->tm.ev[6]);
  }
  (void)hipGetLastError();
}

// From the next run on, the device's own large tier is launched (a captured step does not contain its launches).
static void arm_big_device(km_batch* b) {
  if (!b->big.big_entry || b->big.bigdev_armed) return;
  b->big.bigdev_armed = true;
  b->drop_graph();
}

// Wait for the launched kernels, then finish the rare work that needs the host:
// targets that outgrew the LDS-resident tier are rerun with global workspaces,
// and the path pools are enlarged if they overflowed.
extern "C" int km_batch_sync(km_batch_t* b) {
  if (!b) return fail(KM_E_ARG, "null argument");
  if (b->synced) return KM_OK;
  HIPCHK(hipSetDevice(b->device));
  hipStream_t st = b->last_stream;
  HIPCHK(hipStreamSynchronize(st));
  read_timings(b);
  if (!b->n_targets) { b->synced = true; return KM_OK; }
  KMCHK(pull_status(b, st));
  const uint32_t n = b->n_targets;

  std::vector<uint32_t> big;
  for (uint32_t t = 0; t < n; ++t) if (b->t.h_status[t] == T_NEEDS_BIG) big.push_back(t);
  b->big.n_big = (uint32_t)big.size();
  std::vector<char> force_big(n, 0);
  bool changed = false;
  if (!big.empty()) {
    arm_big_device(b);
    KMCHK(run_big_walk(b, big, st));
    for (uint32_t t : big) force_big[t] = 1;     // the fast graph pass skipped them
    KMCHK(pull_status(b, st));
    changed = true;
  }
  if (b->ran_graph) {
    for (int pass = 0;; ++pass) {
      if (pass > 0) {
        if (pass > 8) return fail(KM_E_NOMEM, "path pools keep overflowing");
        b->drop_graph();                  // a captured step holds the old pool addresses and sizes
        KMCHK(b->paths.grow());
        KMCHK(relaunch_fast_graph(b, st));
        KMCHK(pull_status(b, st));
        std::fill(force_big.begin(), force_big.end(), 0);   // the relaunch saw their final walk status
        changed = true;
      }
      std::vector<uint32_t> todo;
      for (uint32_t t = 0; t < n; ++t)
        if (b->t.h_status[t] == T_OK && (force_big[t] || b->t.h_gstatus[t] == T_NEEDS_BIG)) todo.push_back(t);
      if (!todo.empty()) {
        KMCHK(run_big_graph(b, todo, st));
        KMCHK(pull_status(b, st));
        std::vector<uint32_t> dense;          // more candidate edges than nodes: once more, sized by the edges
        for (uint32_t t : todo) if (b->t.h_status[t] == T_OK && b->t.h_gstatus[t] == T_INTERNAL) dense.push_back(t);
        if (!dense.empty()) {
          KMCHK(run_big_graph(b, dense, st, true));
          KMCHK(pull_status(b, st));
        }
        changed = true;
      }
      if (!b->paths.h_overflow) break;
    }
  }
  if (changed) b->out.deliver_pending = b->out.result_ready = false;   // any earlier delivery is stale
  b->synced = true;
  return KM_OK;
}
