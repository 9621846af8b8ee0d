// result_host.h — what reads a delivered step: finish_result and the exports over it (km_batch_result, _pump, _sizes,
// _fetch), the diagnostics exports and the measurement helpers (host part of kmgpu.hip; the step itself: batch_host.h)
// Wait for an event; KM_SPIN_US=n polls it for the first n microseconds instead of putting the
// thread to sleep at once (default 0: on the boxes measured a polling consumer gained nothing,
// 0.315 against 0.312 ms per delivered step).
static hipError_t wait_event_hot(hipEvent_t ev) {
  const long spin_us = knobs().spin_us;
  if (spin_us > 0) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      const hipError_t e = hipEventQuery(ev);
      if (e != hipErrorNotReady) return e;
      if (std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > spin_us) break;
    }
  }
  return hipEventSynchronize(ev);
}

// Results of the last run in the pinned delivery buffer (delivering now if the run did not).
// `need_full`: a lean delivery (pending or ready) is replaced by a full one.
static int finish_result(km_batch* b, bool need_full) {
  if (!b->ran_walk) return fail(KM_E_STATE, "nothing has run yet");
  const bool partial = b->out.lean || b->out.count16;       // the pending / ready delivery is not the full 32-bit form
  if (b->out.result_ready && !(need_full && partial)) return KM_OK;
  HIPCHK(hipSetDevice(b->device));
  hipStream_t st = b->last_stream;
  if (need_full && partial && (b->out.deliver_pending || b->out.result_ready)) {
    HIPCHK(hipEventSynchronize(b->out.ev_out));
    b->out.deliver_pending = b->out.result_ready = false;
  }
  if (!b->out.deliver_pending) {
    KMCHK(km_batch_sync(b));
    KMCHK(enqueue_deliver(b, st, false));
  }
  const OutLayout L = out_layout(b->n_targets);
  const unsigned long long* T = reinterpret_cast<const unsigned long long*>(b->out.h_out + L.totals);
  for (int attempt = 0;; ++attempt) {
    HIPCHK(wait_event_hot(b->out.ev_out));
    if (knobs().debug_deliver) {                      // timing ablation (diagnostics build only): nothing valid arrived
      b->out.deliver_pending = false; b->out.result_ready = true;
      return KM_OK;
    }
    if (T[OT_SERIAL] != b->out.serial) return fail(KM_E_HIP, "delivery buffer out of step");
    const unsigned long long nh = T[OT_NEEDS_HOST];
    if (b->hints.observe(T[OT_N_FLAGGED], b->ran_graph && b->graph_mode == 0 ? &T[OT_N_GRAPH_LIST] : nullptr)) b->drop_graph();
    if ((nh & 1ull) || T[OT_N_BIG_DEV]) arm_big_device(b);
    if (!nh && b->out.count16 && T[OT_N_ESC] > OUT_ESC_CAP) {
      // more counts >= 65535 than the escape list holds: this batch is delivered with 32-bit counts
      if (attempt >= 4) return fail(KM_E_NOMEM, "result delivery keeps failing");
      KMCHK(enqueue_deliver(b, st, b->out.lean, false));
      continue;
    }
    if (!nh) break;
    if (attempt >= 4) return fail(KM_E_NOMEM, "result delivery keeps failing");
    if (nh & 1ull) {
      b->synced = false;
      KMCHK(km_batch_sync(b));
    }
    HIPCHK(hipStreamSynchronize(st));
    // (2: everything is final, only the tail is larger than the buffer.  A tail of 16-bit counts is sized for the
    // 32-bit form, 2 more bytes per node and at most 16 of alignment: should the escape list overflow, that form
    // follows, and a buffer grown by an eighth would send it round this loop once more)
    KMCHK(ensure_out(b, nh == 2ull ? T[OT_TAIL_BYTES] + (b->out.count16 ? 2 * T[OT_N_NODES] + 16 : 0) + 4096
                                   : default_tail_bytes(b, b->nodes.node_pool_used, b->nodes.node_pool_used)));
    T = reinterpret_cast<const unsigned long long*>(b->out.h_out + L.totals);
    KMCHK(enqueue_deliver(b, st, b->out.lean, b->out.count16));
  }
  const uint64_t tail = T[OT_TAIL_BYTES];
  if (tail > b->out.copied_tail)
    HIPCHK(hipMemcpy(b->out.h_out + L.a_bytes + b->out.copied_tail, b->out.d_out + L.a_bytes + b->out.copied_tail,
                     tail - b->out.copied_tail, hipMemcpyDeviceToHost));
  b->out.tail_guess = tail + tail / 16 + 4096;
  if (b->out.count16 && T[OT_N_ESC] > 1) {
    // the escape list in node order (the delivery kernel appends as its waves come)
    const uint32_t ne = (uint32_t)T[OT_N_ESC];
    uint64_t* en = reinterpret_cast<uint64_t*>(b->out.h_out + L.esc_node);
    uint32_t* ev = reinterpret_cast<uint32_t*>(b->out.h_out + L.esc_value);
    std::vector<std::pair<uint64_t, uint32_t>> tmp(ne);
    for (uint32_t i = 0; i < ne; ++i) tmp[i] = {en[i], ev[i]};
    std::sort(tmp.begin(), tmp.end());
    for (uint32_t i = 0; i < ne; ++i) { en[i] = tmp[i].first; ev[i] = tmp[i].second; }
  }
  b->out.deliver_pending = false;
  b->out.result_ready = true;
  return KM_OK;
}

static void view_of_result(const km_batch* b, km_batch_out_t* v) {
  const OutLayout L = out_layout(b->n_targets);
  unsigned char* h = b->out.h_out;
  const unsigned long long* T = reinterpret_cast<const unsigned long long*>(h + L.totals);
  unsigned char* tail = h + L.a_bytes;
  memset(v, 0, sizeof *v);
  v->status = reinterpret_cast<uint32_t*>(h + L.status);
  v->n_ref = reinterpret_cast<uint32_t*>(h + L.n_ref);
  v->probes = reinterpret_cast<uint64_t*>(h + L.probes);
  v->node_off = reinterpret_cast<uint64_t*>(h + L.node_off);
  v->extra_off = reinterpret_cast<uint64_t*>(h + L.extra_off);
  v->path_off = reinterpret_cast<uint32_t*>(h + L.path_off);
  v->ref_max_cov = reinterpret_cast<uint32_t*>(h + L.ref_max);
  if (b->out.count16) {
    v->node_count16 = reinterpret_cast<uint16_t*>(tail + T[OT_OFF_COUNT]);
    v->count_esc_node = reinterpret_cast<uint64_t*>(h + L.esc_node);
    v->count_esc_value = reinterpret_cast<uint32_t*>(h + L.esc_value);
  } else {
    v->node_count = reinterpret_cast<uint32_t*>(tail + T[OT_OFF_COUNT]);
  }
  v->extra_kmer = reinterpret_cast<uint64_t*>(tail + T[OT_OFF_EXTRA]);
  v->path_len = reinterpret_cast<uint32_t*>(tail + T[OT_OFF_PLEN]);
  v->path_min_cov = reinterpret_cast<uint32_t*>(tail + T[OT_OFF_PMIN]);
  v->run_off = reinterpret_cast<uint64_t*>(tail + T[OT_OFF_RUNOFF]);
  v->run_start = reinterpret_cast<uint32_t*>(tail + T[OT_OFF_RSTART]);
  v->run_len = reinterpret_cast<uint32_t*>(tail + T[OT_OFF_RLEN]);
}

static void sizes_of_result(const km_batch* b, km_batch_sizes_t* s) {
  const unsigned long long* T = reinterpret_cast<const unsigned long long*>(b->out.h_out + out_layout(b->n_targets).totals);
  memset(s, 0, sizeof *s);
  s->n_targets = b->n_targets;
  s->n_paths = (uint32_t)T[OT_N_PATHS];
  s->n_nodes = T[OT_N_NODES];
  s->n_runs = T[OT_N_RUNS];
  s->n_extra = T[OT_N_EXTRA];
  s->logical_probes = T[OT_PROBES];
  s->table_fetches = T[OT_FETCHES];
  s->n_big_tier = b->big.n_big + (b->big.bigdev_ran ? (uint32_t)T[OT_N_BIG_DEV] : 0u);
  s->n_flagged = (uint32_t)T[OT_N_FLAGGED];
  s->seed_probes = T[OT_SEED_PROBES];
  s->n_count_escapes = b->out.count16 ? (uint32_t)T[OT_N_ESC] : 0;
}

extern "C" int km_batch_result(km_batch_t* b, km_batch_out_t* view, km_batch_sizes_t* sizes) {
  if (!b) return fail(KM_E_ARG, "null argument");
  KMCHK(finish_result(b, false));
  if (view) view_of_result(b, view);
  if (sizes) sizes_of_result(b, sizes);
  return KM_OK;
}

// `steps` runs over `n` batches in flight, round robin: before a batch is run again its last
// delivery is awaited (km_batch_result), at the end every batch's.  The loop a pipelined consumer
// writes, kept on the library's side of the ABI so that an interpreter between two launches does
// not sit in the timed region (diagnostics / bench; tools/launch_cost.py).
//
// Consecutive steps are PAIRED where they can be: k_seed of the next batch runs as blocks of the previous batch's
// k_dfs_pure launch (graph_kernel.h: k_dfs_pure_seed), so that the two kernels that are three quarters of a step's
// chain — one bound by memory, one by its slowest wave — overlap whatever the streams' hardware queues do.  The
// paired steps use THREE streams of the pump's own (pool streams held for the call), whatever n is.  The chain — the
// paired launch, the paired launch, ... — goes to one, where each launch follows the last without waiting for a
// command that was enqueued after it; behind every paired launch an event is recorded, and the second stream, the
// tail, waits for it and takes the back of the walked batch's step (large tier, k_graph, delivery), off the chain.
// k_pack of the next batch needs nothing of the launch in front of it, only that the host has awaited the last
// delivery of its workspace: it goes to the third stream, the front, with an event behind it that the chain waits for
// before the launch that seeds that batch (KM_PUMP_FRONT=0: k_pack on the chain, in front of that launch, as in
// round 7).  What that wins is small, 2 % of a step: in the timeline k_pack does not run beside the launch that was
// enqueued before it, on either stream.  It starts as that launch drains, together with the tail's kernels — while
// the launch's single-wave blocks keep the wave slots full, the blocks of another queue's kernel hardly get one —
// and the next launch starts some 13 us after k_pack's end instead of at it.
// (With the chain on the batches' own streams, each paired launch behind an event of the stream before it, the GPU
// stood idle a fifth of the time; with the backs on the batches' own streams the chain shared hardware queues with
// their copies: DESIGN.md section 5, round 7.  The delivery copy on a fourth stream, and the front or the tail at a
// higher stream priority, lost: round 8.)  The front waits once for what the caller has put on a batch's stream
// before the call (the first step of a run of paired steps: the chain), and the chain gets that wait through
// k_pack's event; when the pump returns every delivery has been awaited and a batch's stream is its own again.
// The first step of a run of paired steps packs and seeds on the chain, with the block k_seed; the last one walks
// with k_dfs_pure.  A step
// that cannot be paired is km_batch_run's sequence on the batch's own stream; KM_PUMP_UNPAIRED or KM_PAIR_SEED=0:
// every step is.
//
// One chain gives up the overlap of n streams, so by default a step is paired only where that trade pays
// (pairing_pays, seeds_fill_device below; the figures: DESIGN.md section 5, round 7): at most PAIR_MAX_BATCHES batches
// in flight, a lean delivery, and seeds of the next batch for PAIR_MIN_SEED_ROUNDS rounds of the device.
// KM_PUMP_PAIRED or KM_PAIR_SEED=2 pairs every step that CAN be paired (tests, measurements).

// May steps with these flags be paired at all?  Plain walk + graph + delivery, no diagnostics.
static bool pairing_allowed(int n, int stages) {
  const int plain = KM_STAGE_WALK | KM_STAGE_GRAPH | KM_RUN_DELIVER | KM_DELIVER_LEAN | KM_DELIVER_COUNT16;
  const int must = KM_STAGE_WALK | KM_STAGE_GRAPH | KM_RUN_DELIVER;
  return n >= 2 && (stages & ~plain) == 0 && (stages & must) == must && knobs().pair_seed != 0 && knobs().fuse_pure &&
         !knobs().seed_stamps && !knobs().dfs_replay && knobs().debug_flags == 0;
}
// May k_seed of `next` run in the walk launch of `prev`?  (What does not change between two km_batch_set_targets.)
static bool pairs_with(const km_batch* prev, const km_batch* next) {
  // (the paired launch's grid: at most n_targets walk blocks + n_targets pure-chain blocks + the seed blocks)
  const uint64_t grid_max = 2ull * prev->n_targets + (uint64_t)(4 / SEED_WAVE_RUNS) * next->in.n_items;
  return prev != next && prev->device == next->device && prev->n_targets && next->n_targets && next->in.n_items &&
         (prev->db->k == 31) == (next->db->k == 31) && grid_max <= 0x7FFFFFFFull;
}

// Does the walk launch of `b` (front enqueued: its geometry is known) take another batch's seeds?  Its k_dfs and
// k_graph_pure must share a launch, and its walk blocks — the grid follows the flagged targets of b's last delivery —
// must all be resident at once (CU_SIMDS x KM_DFS_WAVES_PER_EU = 16 waves per CU at 128 registers, fewer where a block's
// share of the CU's LDS says so): every seed block then starts as soon as a walk wave retires.  A walk that needs several rounds of the device has no idle slot
// before its last round; the seeds would only be appended to it, and the one chain of the paired steps would cost the
// overlap of the batches' walks on their own streams (measured on the workload whose every target is flagged, 10 000
// walk blocks: 0.71 ms per step unpaired, 1.15 paired: DESIGN.md section 5, round 7).
constexpr uint32_t CU_SIMDS = 4;               // SIMDs of a CDNA compute unit
constexpr uint32_t CU_LDS_BYTES = 160u << 10;  // LDS of a gfx950 compute unit
static bool takes_seeds(const km_batch* b, const RunFlags& f, int cus) {
  const uint64_t per_cu = std::min<uint64_t>(CU_SIMDS * KM_DFS_WAVES_PER_EU, CU_LDS_BYTES / std::max<uint32_t>(b->walk_lds, 1u));
  return step_fuses(b, f) && b->walk_lds >= SEED_WAVE_LDS &&      // (a seed wave's key windows are part of the launch's LDS)
         (uint64_t)b->hints.dfs_grid(b->n_targets) <= per_cu * (uint64_t)cus;
}

// Does pairing pay for a pump of n batches with these flags?  The paired steps share ONE chain stream and one tail
// stream.  That is a gain where the GPU is the limit and the chain's two long kernels are what a step costs; it is a
// loss where the consumer answers a latency-bound step with more batches in flight than the four the gain was
// measured with (8 batches of 1 250-5 000 targets: 1.4-2.1 x slower paired), and where the delivery copy is
// what a step costs (a full delivery, 20 MB per step: every copy and the delivery kernels of the step behind it
// follow each other on the tail, 0.454 -> 0.488 ms per step paired).
constexpr int PAIR_MAX_BATCHES = 4;
static bool pairing_pays(int n, const RunFlags& f) { return n <= PAIR_MAX_BATCHES && f.lean; }
// ... and for this next batch?  Its seed blocks must fill the wave slots of the walk launch (CU_SIMDS x
// KM_DFS_WAVES_PER_EU per compute unit) PAIR_MIN_SEED_ROUNDS times over: only then is the seed role bound by the
// memory system, whose idle share under the walk is what the paired launch wins.  Fewer seed waves wait for their own
// dependent loads like the walk beside them, the step is bound by the latency of its chain of kernels, and n chains on
// n streams are shorter than one (4 batches of 1 250 targets x 500 nt, 0.6 rounds: 0.070 -> 0.077 ms per step paired).
constexpr uint32_t PAIR_MIN_SEED_ROUNDS = 2;
static bool seeds_fill_device(const km_batch* next, int cus) {
  return (uint64_t)(4 / SEED_WAVE_RUNS) * next->in.n_items >=
         (uint64_t)PAIR_MIN_SEED_ROUNDS * CU_SIMDS * KM_DFS_WAVES_PER_EU * (uint64_t)cus;
}

extern "C" int km_batch_pump(km_batch_t* const* bs, void* const* streams, int n, int steps, int stages) {
  if (!bs || n <= 0 || steps < 0) return fail(KM_E_ARG, "bad argument");
  const bool deliver = (stages & KM_RUN_DELIVER) != 0;
  const bool wherever = (stages & KM_PUMP_PAIRED) || knobs().pair_seed == 2;   // not only where it pays
  const bool unpaired = (stages & KM_PUMP_UNPAIRED) != 0;
  stages &= ~(KM_PUMP_UNPAIRED | KM_PUMP_PAIRED);
  const RunFlags f(stages);
  const bool may_pair = !unpaired && pairing_allowed(n, stages) && (wherever || pairing_pays(n, f));
  CallStream chain, tail, front;         // the streams of the paired steps (taken at the first such step)
  const bool use_front = knobs().pump_front;
  int chain_device = -1;                 // their device
  int cus = 0, cus_device = -1;          // the compute units of the device of the batch at hand
  auto learn_cus = [&](int device) -> int {
    if (device != cus_device) HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    cus_device = device;
    return KM_OK;
  };
  // may k_seed of `next` run in the walk launch of `prev`, and is it worth it?
  auto pairs = [&](const km_batch* prev, const km_batch* next) {
    return pairs_with(prev, next) && (wherever || seeds_fill_device(next, cus));
  };
  km_batch* prev = nullptr;              // front and k_seed enqueued on the chain, the rest of its step not yet
  // However the call ends, no batch keeps a stream of the pump's as its last_stream: on success every delivery has
  // been awaited; on an error return the pump's streams are waited for first.  (Declared behind them: it runs before
  // they are given back.)
  struct GiveBack {
    km_batch_t* const* bs; void* const* streams; int n; const CallStream &chain, &tail, &front; bool ok = false;
    ~GiveBack() {
      for (int q = 0; q < n; ++q) {
        km_batch* b = bs[q];
        if (!b || !b->pair.borrowed) continue;
        if (!ok) {
          (void)hipSetDevice(b->device);
          for (const CallStream* s : {&front, &chain, &tail})
            if (s->st) (void)hipStreamSynchronize(*s);
        }
        b->last_stream = (hipStream_t)(streams ? streams[q] : nullptr);
        b->pair.borrowed = false;
      }
    }
  } give_back{bs, streams, n, chain, tail, front};
  // prev's walk launch is on the chain: the tail takes the back of its step behind it
  auto back_of_prev = [&](bool fused) -> int {
    if (!prev->pair.ev_walked) HIPCHK(hipEventCreateWithFlags(&prev->pair.ev_walked.h, hipEventDisableTiming));
    HIPCHK(hipEventRecord(prev->pair.ev_walked, chain));
    HIPCHK(hipStreamWaitEvent(tail, prev->pair.ev_walked, 0));
    prev->last_stream = tail;
    return step_back(prev, tail, f, fused);
  };
  // the rest of prev's step without another batch's seeds: k_dfs_pure, the back
  auto finish_alone = [&]() -> int {
    bool fused = false;
    HIPCHK(hipSetDevice(prev->device));
    KMCHK(step_walk(prev, chain, f, &fused));
    KMCHK(back_of_prev(fused));
    prev = nullptr;
    return KM_OK;
  };
  // b's step goes to the pump's streams: behind its un-awaited run of before this pump, if any, and behind what
  // the caller has put on its stream (`first`: the stream of the pump that gets b's first command, its k_pack)
  auto borrow = [&](km_batch* b, hipStream_t st, bool first_round, hipStream_t first) -> int {
    KMCHK(wait_in_flight(b));
    if (first_round) {
      if (!b->pair.ev_walked) HIPCHK(hipEventCreateWithFlags(&b->pair.ev_walked.h, hipEventDisableTiming));
      HIPCHK(hipEventRecord(b->pair.ev_walked, st));
      HIPCHK(hipStreamWaitEvent(first, b->pair.ev_walked, 0));
    }
    b->pair.borrowed = true;
    return KM_OK;
  };
  for (int i = 0; i < steps; ++i) {
    km_batch_t* b = bs[i % n];
    hipStream_t st = (hipStream_t)(streams ? streams[i % n] : nullptr);
    if (i >= n && deliver) KMCHK(finish_result(b, false));
    if (may_pair) KMCHK(learn_cus(b->device));
    if (prev && pairs(prev, b)) {
      HIPCHK(hipSetDevice(b->device));
      if (use_front) {
        // k_pack(b) needs nothing of the launch in front of it on the chain, only that b's last delivery has been
        // awaited (above): it goes to the front, and the chain waits for its event (what orders b's seeds behind
        // whatever the caller put on b's stream, too)
        KMCHK(borrow(b, st, i < n, front));
        KMCHK(step_open(b, chain, f));
        KMCHK(step_pack(b, front));
        if (!b->pair.ev_packed) HIPCHK(hipEventCreateWithFlags(&b->pair.ev_packed.h, hipEventDisableTiming));
        HIPCHK(hipEventRecord(b->pair.ev_packed, front));
        HIPCHK(hipStreamWaitEvent(chain, b->pair.ev_packed, 0));
      } else {
        KMCHK(borrow(b, st, i < n, chain));
        KMCHK(step_front(b, chain, f));
      }
      KMCHK(launch_dfs_pure_seed(prev, b, chain));
      ++b->pair.n_seeded;
      KMCHK(back_of_prev(true));
      // (can b, in its turn, take the seeds of the step after it?  Its geometry is known now.)
      prev = b;
      if (!takes_seeds(b, f, cus)) KMCHK(finish_alone());
      continue;
    }
    if (prev) KMCHK(finish_alone());
    const bool first_of_pair = may_pair && i + 1 < steps && pairs(b, bs[(i + 1) % n]) &&
                               (chain_device < 0 || chain_device == b->device);
    if (!first_of_pair) {
      KMCHK(km_batch_run(b, stages, st));
      continue;
    }
    HIPCHK(hipSetDevice(b->device));
    KMCHK(wait_in_flight(b));              // (an un-awaited run of before this pump, on whichever stream)
    KMCHK(step_open(b, st, f));
    if (!takes_seeds(b, f, cus)) {         // its walk takes nobody's seeds: the whole step on its own stream
      KMCHK(step_pack(b, st));
      KMCHK(step_rest(b, st, f));
      continue;
    }
    if (chain_device < 0) {
      KMCHK(chain.get(b->device, nullptr));
      KMCHK(tail.get(b->device, nullptr));
      if (use_front) KMCHK(front.get(b->device, nullptr));
      chain_device = b->device;
    }
    KMCHK(borrow(b, st, i < n, chain));
    b->last_stream = chain;
    KMCHK(step_pack(b, chain));
    KMCHK(step_seed(b, chain));
    prev = b;
  }
  if (prev) KMCHK(finish_alone());
  for (int q = 0; q < std::min(n, steps); ++q) {
    KMCHK(deliver ? finish_result(bs[q], false) : km_batch_sync(bs[q]));
  }
  give_back.ok = true;                   // nothing of any batch is left on the pump's streams
  return KM_OK;
}

extern "C" int km_batch_debug_stamps(km_batch_t* b, uint64_t* dst, uint64_t cap_words, uint64_t* n_words) {
  if (!b || !n_words) return fail(KM_E_ARG, "null argument");
  KMCHK(km_batch_sync(b));
  const uint64_t n = b->probes.d_stamps.p ? 16ull * (SEED_BLOCK / 64) * b->in.n_items : 0;
  *n_words = n;
  if (!dst || !n) return KM_OK;
  if (cap_words < n) return fail(KM_E_CAPACITY, "stamp buffer too small");
  HIPCHK(hipMemcpy(dst, b->probes.d_stamps.p, n * 8, hipMemcpyDeviceToHost));
  return KM_OK;
}

// ---- measurement helpers for consumers that hold no device buffers of their own (bench.py at N = 1
// runs without PyTorch in the process: the library is then served by the ROCm installation's HIP runtime,
// as it is for a C consumer)
extern "C" int km_device_sync(int device) {
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipDeviceSynchronize());
  return KM_OK;
}

// Device-to-device copy of `bytes` bytes, `reps` times: read + write bandwidth in GB/s (the box's
// large-copy rate beside the 8 TB/s spec).
extern "C" int km_device_copy_GBs(int device, uint64_t bytes, int reps, double* gbs) {
  if (!gbs || !bytes || reps < 1) return fail(KM_E_ARG, "bad argument");
  HIPCHK(hipSetDevice(device));
  DevBuf<unsigned char> a, b;
  if (a.alloc(bytes) != KM_OK || b.alloc(bytes) != KM_OK) return fail(KM_E_NOMEM, "hipMalloc failed");
  Event e0, e1;
  hipError_t e = hipEventCreate(&e0.h);
  if (e == hipSuccess) e = hipEventCreate(&e1.h);
  if (e == hipSuccess) e = hipMemcpy(b, a, bytes, hipMemcpyDeviceToDevice);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipEventRecord(e0, nullptr);
  for (int i = 0; i < reps && e == hipSuccess; ++i) e = hipMemcpyAsync(b, a, bytes, hipMemcpyDeviceToDevice, nullptr);
  if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
  if (e == hipSuccess) e = hipEventSynchronize(e1);
  float ms = 0;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  if (e != hipSuccess) return fail(KM_E_HIP, "copy bandwidth measurement failed: %s", hipGetErrorString(e));
  *gbs = 2.0 * (double)reps * (double)bytes / ((double)ms * 1e-3) / 1e9;
  return KM_OK;
}

// k_query and k_children alone over `n` k-mers given on the host: average kernel time over `reps`
// launches each (HIP events), and how many of the k-mers have count 0.
extern "C" int km_probe_bench(kmjf_t* h, const uint64_t* kmers, uint64_t n, int reps, double ratio, int64_t n_cutoff,
                              double* query_ms, double* children_ms, uint64_t* n_zero) {
  if (!h || !kmers || !n || reps < 1 || !query_ms || !children_ms) return fail(KM_E_ARG, "bad argument");
  if (!h->d_slots) return fail(KM_E_STATE, "table not uploaded");
  HIPCHK(hipSetDevice(h->device));
  DevBuf<uint64_t> dk;
  DevBuf<uint32_t> dq, dc;
  DevBuf<uint8_t> dm;
  Event ev[3];
  if (dk.alloc(n) != KM_OK || dq.alloc(n) != KM_OK || dm.alloc(n) != KM_OK || dc.alloc(4 * n) != KM_OK) {
    const std::string why = km_last_error();
    return fail(KM_E_HIP, "probe benchmark failed: %s", why.c_str());
  }
  int rc = KM_OK;
  hipError_t e = hipSuccess;
  for (int i = 0; i < 3 && e == hipSuccess; ++i) e = hipEventCreate(&ev[i].h);
  if (e == hipSuccess) e = hipMemcpy(dk, kmers, n * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    for (int w = 0; w < 2 && rc == KM_OK; ++w) {
      rc = kmjf_query_batch_dev(h, dk, n, dq, nullptr);
      if (rc == KM_OK) rc = kmjf_children_batch_dev(h, dk, n, ratio, n_cutoff, 1, dm, dc, nullptr);
    }
    if (rc == KM_OK) e = hipDeviceSynchronize();
    if (rc == KM_OK && e == hipSuccess) e = hipEventRecord(ev[0], nullptr);
    for (int i = 0; i < reps && rc == KM_OK; ++i) rc = kmjf_query_batch_dev(h, dk, n, dq, nullptr);
    if (rc == KM_OK && e == hipSuccess) e = hipEventRecord(ev[1], nullptr);
    for (int i = 0; i < reps && rc == KM_OK; ++i) rc = kmjf_children_batch_dev(h, dk, n, ratio, n_cutoff, 1, dm, dc, nullptr);
    if (rc == KM_OK && e == hipSuccess) e = hipEventRecord(ev[2], nullptr);
    if (rc == KM_OK && e == hipSuccess) e = hipEventSynchronize(ev[2]);
    float q = 0, c = 0;
    if (rc == KM_OK && e == hipSuccess) e = hipEventElapsedTime(&q, ev[0], ev[1]);
    if (rc == KM_OK && e == hipSuccess) e = hipEventElapsedTime(&c, ev[1], ev[2]);
    *query_ms = q / reps;
    *children_ms = c / reps;
    if (rc == KM_OK && e == hipSuccess && n_zero) {
      std::vector<uint32_t> hq(n);
      e = hipMemcpy(hq.data(), dq, n * 4, hipMemcpyDeviceToHost);
      uint64_t z = 0;
      for (uint32_t v : hq) z += v == 0;
      *n_zero = z;
    }
  }
  if (rc != KM_OK) return rc;
  if (e != hipSuccess) return fail(KM_E_HIP, "probe benchmark failed: %s", hipGetErrorString(e));
  return KM_OK;
}

// Diagnostics: the device counters of the last run — [0] flagged targets (k_seed), [1] unflagged
// targets k_graph_pure handed to k_graph, [2] flagged targets the epilogue of k_dfs left to k_graph.
// What the reference logs with -v from inside the walk and the graph (km/utils/MutationFinder.py:160-161,
// km/utils/Graph.py:198, 231), for the last run: per target the reference edges stripped and the edges kept, and the
// walk's loop breaks as {target, node index} pairs in walk order.  Any output may be NULL.
extern "C" int km_batch_graph_log(km_batch_t* b, uint32_t* removed_ref_edges, uint32_t* nonref_edges,
                                  uint32_t* n_loop_breaks, uint32_t* loop_pairs, uint32_t loop_cap) {
  if (!b) return fail(KM_E_ARG, "null argument");
  if (!b->ran_walk) return fail(KM_E_STATE, "no run to report on");
  // a delivered run: finish it (large tier, pools) first
  KMCHK(b->out.deliver_pending || b->out.result_ready ? finish_result(b, false) : km_batch_sync(b));
  HIPCHK(hipSetDevice(b->device));
  hipStream_t st = b->last_stream;
  HIPCHK(hipStreamSynchronize(st));
  const uint32_t n = b->n_targets;
  if (removed_ref_edges && n) HIPCHK(hipMemcpy(removed_ref_edges, b->log.d_t_eremoved.p, 4ull * n, hipMemcpyDeviceToHost));
  if (nonref_edges && n) HIPCHK(hipMemcpy(nonref_edges, b->log.d_t_enonref.p, 4ull * n, hipMemcpyDeviceToHost));
  uint32_t n_loops = 0;
  if (n) HIPCHK(hipMemcpy(&n_loops, b->log.d_loop_ctl.p, 4, hipMemcpyDeviceToHost));
  if (n_loop_breaks) *n_loop_breaks = n_loops;
  const uint32_t have = std::min<uint32_t>(std::min<uint32_t>(n_loops, LOOP_LOG_CAP), loop_cap);
  if (loop_pairs && have) HIPCHK(hipMemcpy(loop_pairs, b->log.d_loop_list.p, 8ull * have, hipMemcpyDeviceToHost));
  return KM_OK;
}

extern "C" int km_batch_debug_counts(km_batch_t* b, uint32_t* out4) {
  if (!b || !out4) return fail(KM_E_ARG, "null argument");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize(b->last_stream));
  HIPCHK(hipMemcpy(out4, b->t.d_nflagged.p, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
  out4[3] = b->pair.n_seeded;
  return KM_OK;
}

extern "C" int km_batch_timings(km_batch_t* b, float* ms8) {
  float* ms3 = ms8;
  if (!b || !ms3) return fail(KM_E_ARG, "null argument");
  if (!b->synced) {
    // timing events only: no status pull, no large tier (finish_result does that when asked)
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipStreamSynchronize(b->last_stream));
    read_timings(b);
  }
  for (int i = 0; i < 8; ++i) ms3[i] = b->tm.ms[i];
  return KM_OK;
}

extern "C" int km_batch_sizes(km_batch_t* b, km_batch_sizes_t* s) {
  if (!b || !s) return fail(KM_E_ARG, "null argument");
  KMCHK(finish_result(b, true));          // the sizes km_batch_fetch fills: a full delivery
  sizes_of_result(b, s);
  return KM_OK;
}

// Copying variant of km_batch_result: fills caller-allocated arrays (sizes from km_batch_sizes).
// node_kmer, when asked for, is rebuilt here: the target's own k-mers from the packed targets,
// the walk-discovered ones from extra_kmer.
extern "C" int km_batch_fetch(km_batch_t* b, const km_batch_out_t* out) {
  if (!b || !out) return fail(KM_E_ARG, "null argument");
  KMCHK(finish_result(b, true));          // the copying API always returns every node
  km_batch_out_t v;
  km_batch_sizes_t s;
  view_of_result(b, &v);
  sizes_of_result(b, &s);
  const uint32_t n = b->n_targets;
  if (out->status) memcpy(out->status, v.status, 4ull * n);
  if (out->aux) memset(out->aux, 0, 4ull * n);
  if (out->n_ref) memcpy(out->n_ref, v.n_ref, 4ull * n);
  if (out->probes) memcpy(out->probes, v.probes, 8ull * n);
  if (out->node_off) memcpy(out->node_off, v.node_off, 8ull * (n + 1));
  if (out->extra_off) memcpy(out->extra_off, v.extra_off, 8ull * (n + 1));
  if (out->node_count) memcpy(out->node_count, v.node_count, 4 * s.n_nodes);
  if (out->extra_kmer) memcpy(out->extra_kmer, v.extra_kmer, 8 * s.n_extra);
  if (out->path_off) memcpy(out->path_off, v.path_off, 4ull * (n + 1));
  if (out->ref_max_cov) memcpy(out->ref_max_cov, v.ref_max_cov, 4ull * n);
  if (out->run_off) memcpy(out->run_off, v.run_off, 8ull * (s.n_paths + 1));
  if (out->run_start) memcpy(out->run_start, v.run_start, 4 * s.n_runs);
  if (out->run_len) memcpy(out->run_len, v.run_len, 4 * s.n_runs);
  if (out->path_len) memcpy(out->path_len, v.path_len, 4ull * s.n_paths);
  if (out->path_min_cov) memcpy(out->path_min_cov, v.path_min_cov, 4ull * s.n_paths);
  if (out->node_kmer && n) {
    HIPCHK(hipSetDevice(b->device));
    if (b->in.h_packed.empty()) {
      b->in.h_packed.resize(b->in.h_woff[n]);
      HIPCHK(hipMemcpy(b->in.h_packed.data(), b->in.d_packed.p, b->in.h_woff[n] * 8, hipMemcpyDeviceToHost));
    }
    const int k = b->db->k;
    for (uint32_t t = 0; t < n; ++t) {
      const uint64_t a0 = v.node_off[t], cnt = v.node_off[t + 1] - a0;
      if (!cnt) continue;
      const uint64_t ne = v.extra_off[t + 1] - v.extra_off[t], nr = cnt - ne;
      const uint64_t* words = b->in.h_packed.data() + b->in.h_woff[t];
      uint64_t* dst = out->node_kmer + a0;
      for (uint64_t i = 0; i < nr; ++i) {
        const uint64_t w = i >> 5, sh = (i & 31) * 2;
        const uint64_t x = sh ? ((words[w] << sh) | (words[w + 1] >> (64 - sh))) : words[w];
        dst[i] = x >> (64 - 2 * k);
      }
      memcpy(dst + nr, v.extra_kmer + v.extra_off[t], 8 * ne);
    }
  }
  return KM_OK;
}
