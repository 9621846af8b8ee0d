/* kmgpu.h — C-ABI of libkmgpu.so: the MI355X (gfx950) implementation of km's
 * `find_mutation` hot path.  Plain pointers and sizes only; every function
 * returns an int status (KM_OK == 0) and never throws across the boundary.
 *
 * The reference (iric-soft/km, pure Python) has no FFI of its own: its seam is
 * the duck-type of km/utils/Jellyfish.py plus the SWIG surface of the
 * third-party Jellyfish binding beneath it.  Each entry point below names the
 * reference interface it replaces (file:line into the reference tree).  The
 * ctypes binding a km maintainer would add is shown in INTEGRATION.md and
 * shipped as km_amd/lib.py.
 *
 * Threading: a handle is used from one host thread at a time.  Device work is
 * issued on the caller's HIP stream where a `stream` argument exists
 * (a hipStream_t passed as void*; NULL = the default stream).
 *
 * k-mer encoding (same as Jellyfish keys): A=0 C=1 G=2 T=3, two bits per base,
 * first base in the most significant used bits of a uint64_t (k <= 32).
 */
#ifndef KMGPU_H
#define KMGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------- */
#define KM_OK          0
#define KM_E_IO        1   /* cannot open / read the file                          */
#define KM_E_FORMAT    2   /* not a Jellyfish `binary/sorted` file, bad header     */
#define KM_E_K         3   /* k > 32 (key does not fit a uint64_t) or k < 2        */
#define KM_E_ARG       4   /* NULL / out-of-range argument                         */
#define KM_E_HIP       5   /* a HIP runtime call failed (see km_last_error)        */
#define KM_E_NOMEM     6   /* host or device allocation failed                     */
#define KM_E_STATE     7   /* call order violated (e.g. table not uploaded)        */
#define KM_E_CAPACITY  8   /* a caller-provided output buffer is too small         */

/* ---- per-target status written by the walk ------------------------------ */
#define KM_T_OK          0
#define KM_T_NODE_LIMIT  1  /* len(node_data) > max_node at an extension call:
                               km/utils/MutationFinder.py:143-148 (host turns it
                               back into the same sys.exit message)              */
#define KM_T_REPEAT_KMER 2  /* a k-mer occurs twice in the target: ValueError of
                               km/utils/common.py:55-59                          */
#define KM_T_EMPTY       3  /* target shorter than k: `assert len(ref_mer)`,
                               km/utils/Sequence.py:46                           */
#define KM_T_BAD_BASE    4  /* a character outside ACGTacgt                      */
#define KM_T_INTERNAL    5  /* workspace exhausted even in the large tier        */

typedef struct kmjf kmjf_t;         /* one k-mer count database (host records + device table) */
typedef struct km_batch km_batch_t; /* device workspace for a batch of targets                */

typedef struct {
  int32_t  k;            /* k-mer length (key_len / 2)                        */
  int32_t  canonical;    /* header["canonical"]  (km/utils/Jellyfish.py:45)   */
  uint64_t n_records;    /* records held (count > 0)                          */
  uint64_t n_slots;      /* device table capacity in 16-byte slots (0 = not uploaded) */
  uint64_t n_groups;     /* occupied slots                                    */
  uint64_t table_bytes;  /* n_slots * 16 + bucket directory + side table of counts >= 65535 */
  int32_t  device;       /* HIP device ordinal of the table, -1 if none       */
  int32_t  max_probe;    /* slots a lookup may read: 2 (the home pair) unless a minimizer
                            bucket was too heavy to keep that bound; like n_slots a function of
                            the record SET (any order of the records gives the same table
                            geometry: the build's settle pass)    */
} kmjf_info_t;

/* Walk parameters = the CLI flags of km/argparser/find_mutation.py:5-39 as they
 * reach Jellyfish(cutoff=ratio, n_cutoff=count) and
 * MutationFinder(refpath, jf, steps, branchs, nodes)
 * (km/tools/find_mutation.py:29,49-51). */
typedef struct {
  double   ratio;      /* -p/--ratio   : child kept iff count >= max(sum*ratio, count) */
  int64_t  count;      /* -c/--count                                                   */
  uint32_t max_stack;  /* -s/--steps                                                   */
  uint32_t max_break;  /* -b/--branchs                                                 */
  uint32_t max_node;   /* -n/--nodes                                                   */
  uint32_t reserved;
} km_params_t;

typedef struct {
  uint32_t n_targets;
  uint32_t n_paths;        /* over all targets                                 */
  uint64_t n_nodes;        /* over all targets, caps excluded                  */
  uint64_t n_runs;         /* path run-length records over all paths           */
  uint64_t logical_probes; /* reference-semantics Jellyfish.query calls        */
  uint64_t table_fetches;  /* 16-byte table slots actually read by the walk (KM_RUN_COUNT_FETCHES; else 0) */
  uint32_t n_big_tier;     /* targets that needed the large-workspace pass     */
  uint32_t n_flagged;      /* targets with at least one non-trivial seed       */
  uint64_t seed_probes;    /* logical probes answered by the k_seed kernel     */
  uint64_t n_extra;        /* walk-discovered nodes over all targets (n_nodes minus the targets' own k-mers) */
  uint32_t n_count_escapes;/* entries of count_esc_node / count_esc_value (KM_DELIVER_COUNT16), else 0            */
  uint32_t reserved;
} km_batch_sizes_t;

/* Host-side result arrays.  km_batch_fetch() fills caller-allocated arrays (numpy; any
 * pointer may be NULL to skip that output; sizes come from km_batch_sizes());
 * km_batch_result() instead points them into the batch's pinned delivery buffer (no copy;
 * node_kmer is NULL there: a target's own k-mers are not shipped back to the caller who
 * supplied them, node i < n_ref is the k-mer at base i of the target, and the
 * walk-discovered nodes n_ref.. are in extra_kmer).
 *
 * Node order per target (canonical order): the target's own
 * k-mers in target order (node i == k-mer at position i), then walk-discovered
 * k-mers in registration order.  The two capping nodes of
 * km/utils/MutationFinder.py:97-98,122-123 are implicit: BigBang == n_nodes,
 * BigCrunch == n_nodes + 1.
 *
 * A path (km/utils/Graph.py:220-240, caps stripped as in
 * km/utils/MutationFinder.py:562) is a list of node indices, delivered
 * run-length encoded: consecutive indices (i, i+1, ...) collapse into one
 * (start, length) run.  Paths of one target are sorted by their index sequence. */
typedef struct {
  uint32_t* status;        /* [n_targets]   KM_T_*                                      */
  uint32_t* aux;           /* [n_targets]   REPEAT_KMER: unused (host re-derives pos)   */
  uint32_t* n_ref;         /* [n_targets]   k-mers in the target                        */
  uint64_t* probes;        /* [n_targets]   logical probes                              */
  uint64_t* node_off;      /* [n_targets+1] CSR offsets into node_kmer/node_count       */
  uint64_t* node_kmer;     /* [n_nodes]     packed k-mers                               */
  uint32_t* node_count;    /* [n_nodes]     counts (Jellyfish.query)                    */
  uint32_t* path_off;      /* [n_targets+1] CSR offsets into the per-path arrays        */
  uint64_t* run_off;       /* [n_paths+1]   CSR offsets into run_start/run_len          */
  uint32_t* run_start;     /* [n_runs]                                                  */
  uint32_t* run_len;       /* [n_runs]                                                  */
  uint32_t* path_len;      /* [n_paths]     nodes on the path                           */
  uint32_t* path_min_cov;  /* [n_paths]     min count along the path
                                            (km/utils/MutationFinder.py:639,802)        */
  uint64_t* extra_off;     /* [n_targets+1] CSR offsets into extra_kmer
                                            (extra_off[t+1]-extra_off[t] == nodes of t - n_ref[t]) */
  uint64_t* extra_kmer;    /* [n_extra]     packed k-mers of the walk-discovered nodes     */
  uint32_t* ref_max_cov;   /* [n_targets]   bare-reference targets (the only path is the target's own
                                            k-mer chain, no walk-discovered node): max count over
                                            the target's k-mers; 0xFFFFFFFF for every other target */
  /* KM_DELIVER_COUNT16 (km_batch_result only): node_count is NULL and the counts arrive as 16-bit values,
   * same indexing (node_off); a count >= 65535 reads 0xFFFF there and its exact value is in the escape
   * list, sorted by node index (global index into node_count16).  Half the bytes of a delivery are counts. */
  uint16_t* node_count16;    /* [n_nodes]                                                 */
  uint64_t* count_esc_node;  /* [n_count_escapes] ascending                               */
  uint32_t* count_esc_value; /* [n_count_escapes]                                         */
} km_batch_out_t;

/* ---- database: replaces Jellyfish.__init__ (km/utils/Jellyfish.py:23-45) and
 *      the binding's QueryMerFile / MerDNA.k() (km/utils/Jellyfish.py:24-25) --- */
int kmjf_open(const char* path, kmjf_t** out);
/* Build a database from in-memory records (synthetic workloads, tests, the
 * receiving side of a broadcast).  keys/counts are copied. */
int kmjf_from_records(const uint64_t* keys, const uint32_t* counts, uint64_t n,
                      int k, int canonical, kmjf_t** out);
/* An empty handle whose records live only on a device (multi-GPU receive side). */
int kmjf_create(int k, int canonical, kmjf_t** out);
int kmjf_close(kmjf_t* h);
int kmjf_info(const kmjf_t* h, kmjf_info_t* info);
/* Borrow the host record arrays (valid until kmjf_close). */
int kmjf_records(const kmjf_t* h, const uint64_t** keys, const uint32_t** counts, uint64_t* n);

/* Open + upload in one go, without a host copy of the records: the record area of the
 * memory-mapped file is copied to HBM as it is, unpacked and inserted there (the path for
 * sample-after-sample runs, example/run_leucegene.sh:29-35).  kmjf_records() then reports none. */
int kmjf_load(const char* path, int device, kmjf_t** out);

/* Build the HBM-resident table on `device` from the host records. */
int kmjf_upload(kmjf_t* h, int device);
/* Build the table from record arrays that already sit in device memory
 * (e.g. received through an RCCL broadcast).  The arrays are only read. */
int kmjf_upload_from_device(kmjf_t* h, int device, const uint64_t* d_keys,
                            const uint32_t* d_counts, uint64_t n, void* stream);

/* One database on several GPUs of this process (BASELINE config 4: targets sharded, table replicated; the
 * read-only handle every target of km/tools/find_mutation.py:29,47-58 shares).  `h` holds host records
 * (kmjf_open / kmjf_from_records).  They are uploaded to devices[0], cross the links ONCE as one RCCL
 * broadcast of the 12-byte records (not of the 8.8x larger table), and every device builds its own table:
 * replicas[0] = h (now uploaded on devices[0]), replicas[1..n-1] = new handles for devices[1..n-1]
 * (kmjf_close each).  n == 1 is kmjf_upload.  RCCL is loaded when first needed (librccl.so.1), the library
 * does not link against it; KM_E_HIP if it is missing or a collective fails, KM_E_ARG for n < 1, a null
 * argument or a device named twice.  One process per GPU (torch.distributed, MPI): broadcast the records
 * with the launcher's own collective and call kmjf_upload_from_device (km_amd/dist.py does). */
int kmjf_broadcast(kmjf_t* h, const int* devices, int n, kmjf_t** replicas);

/* ---- lookups: replace Jellyfish.query (km/utils/Jellyfish.py:47-53; also the
 *      loop of common.get_cov, km/utils/common.py:73-92) and
 *      Jellyfish.get_child (km/utils/Jellyfish.py:55-72) ---------------------- */
/* Host arrays in / out. */
int kmjf_query_batch(kmjf_t* h, const uint64_t* kmers, uint64_t n, uint32_t* counts);
/* mask bit c (A=0..T=3) set <=> child `kmer[1:]+c` (forward) or `c+kmer[:-1]`
 * (forward == 0) is kept; counts4[4*i+c] = its count. */
int kmjf_children_batch(kmjf_t* h, const uint64_t* kmers, uint64_t n, double ratio,
                        int64_t n_cutoff, int forward, uint8_t* mask, uint32_t* counts4);
/* Same, device arrays, asynchronous on `stream`. */
int kmjf_query_batch_dev(kmjf_t* h, const uint64_t* d_kmers, uint64_t n, uint32_t* d_counts,
                         void* stream);
int kmjf_children_batch_dev(kmjf_t* h, const uint64_t* d_kmers, uint64_t n, double ratio,
                            int64_t n_cutoff, int forward, uint8_t* d_mask,
                            uint32_t* d_counts4, void* stream);

/* ---- batched walk + path search: replaces, for many targets at once, the loop
 *      body of km/tools/find_mutation.py:47-53:
 *        MutationFinder.__init__ / __extend (km/utils/MutationFinder.py:87-165)
 *        MutationFinder.graph_analysis     (km/utils/MutationFinder.py:496-572)
 *        Graph.init_paths / all_shortest   (km/utils/Graph.py:63-240)
 *        get_counts + min                  (km/utils/MutationFinder.py:490-494,639) */
int km_batch_create(kmjf_t* h, const km_params_t* params, uint32_t max_targets,
                    uint64_t max_total_bases, km_batch_t** out);
int km_batch_destroy(km_batch_t* b);
/* Targets as concatenated ASCII bases (ACGT, either case); offsets[n+1]. Copies H2D.
 * Failure: every argument is checked first (n_targets <= max_targets, offsets non-decreasing, no target
 * longer than 2^31 - 1 bases, offsets[n] - offsets[0] <= max_total_bases); a rejected call (KM_E_ARG)
 * changes nothing: the batch keeps its targets, and the next run gives the results it gave before.
 * In flight: the call may follow a km_batch_run whose results were never awaited (any stream): it first
 * waits for that run and its delivery, then discards them.  Either way, views handed out by an earlier
 * km_batch_result of this batch are invalid once the call has succeeded. */
int km_batch_set_targets(km_batch_t* b, const uint8_t* bases, const uint64_t* offsets,
                         uint32_t n_targets);
/* Same with device-resident arrays (copied device-to-device, async on stream; the call returns once the
 * copy is done).  Same failure guarantee and in-flight behaviour. */
int km_batch_set_targets_dev(km_batch_t* b, const uint8_t* d_bases, const uint64_t* offsets_host,
                             uint32_t n_targets, void* stream);
#define KM_STAGE_WALK  1
#define KM_STAGE_GRAPH 2
/* OR into `stages`: capture the step into a hipGraph on first use and replay it with one
 * launch afterwards (until the targets change).  Per-kernel HIP-event timings are not
 * available for replayed steps. */
#define KM_RUN_HIPGRAPH 4
/* OR into `stages`: also enqueue result delivery behind the kernels, on the same stream — the
 * results are compacted on the device into their final layout (CSR, paths sorted) and cross
 * PCIe with one asynchronous copy into the batch's pinned buffer; km_batch_result() then only
 * waits for that copy.  Without this flag km_batch_result() / km_batch_fetch() deliver on
 * demand. */
#define KM_RUN_DELIVER 8
/* With KM_RUN_DELIVER: lean delivery.  A bare-reference target (ref_max_cov[t] != 0xFFFFFFFF;
 * typically 70 % of a batch) prints one `Reference` row whose only data are path_min_cov and
 * whether every count is 0 (km/utils/MutationFinder.py:575-648, km/utils/PathQuant.py:144-154):
 * its node_count rows are omitted (node_off[t+1] == node_off[t]) and do not cross PCIe.  Every
 * other target is delivered in full.  km_report_rows accepts both forms; km_batch_fetch always
 * returns every node (re-delivering if the last delivery was lean). */
#define KM_DELIVER_LEAN 16
/* With KM_RUN_DELIVER: node counts cross PCIe as 16-bit values + a short list of the exact counts >= 65535
 * (km_batch_out_t.node_count16 / count_esc_*; at most 2048 of those per delivery, else the library quietly
 * delivers the 32-bit form).  km_report_rows reads either form; km_batch_fetch always fills 32-bit counts. */
#define KM_DELIVER_COUNT16 128
/* Count the 16-byte table slots the walk reads (km_batch_sizes_t.table_fetches; 0 without this flag): a
 * diagnostic — two ballots and one more atomic per wave of k_seed, 2 % of a pipelined step. */
#define KM_RUN_COUNT_FETCHES 256
/* Record the HIP events km_batch_timings reads (seven event records per run; off by default). */
#define KM_RUN_TIMED 32
/* With KM_RUN_TIMED: record the STAGE boundaries only (walk start / end, graph end, delivery) — the walk stage as it
 * runs in production, without the two event records between its three kernels; km_batch_timings [3], [4], [5] are 0. */
#define KM_RUN_TIMED_STAGES 512
/* Every kernel alone: a batch's kernels always run in `stream`, in order, and by default the pass over the unflagged
 * targets (k_graph_pure) runs as blocks of k_dfs's own launch (k_dfs_pure; rounds 2-3: beside k_dfs on a side stream).
 * With this flag k_dfs and k_graph_pure are one launch each, k_graph_pure behind k_dfs and inside the graph stage of
 * km_batch_timings — what per-kernel measurements want.  (The environment's KM_FUSE_PURE=0 selects the same two
 * launches for every run.)  Results are the same either way. */
#define KM_RUN_SERIAL 64
/* Launch the kernels asynchronously on `stream` (no host synchronisation unless
 * a target overflows the fast tier, in which case the large-tier pass needs one). */
int km_batch_run(km_batch_t* b, int stages, void* stream);
int km_batch_sync(km_batch_t* b);
/* Sizes of the arrays km_batch_fetch fills (a full delivery; km_batch_result reports the sizes
 * of the delivery it returns, which may be lean).  NOTE: after a LEAN km_batch_result both
 * km_batch_sizes and km_batch_fetch deliver again, in full, into the same pinned buffer (which may
 * be reallocated): views handed out by that km_batch_result are invalid afterwards — copy what is
 * still needed first, or ask for the full form only. */
int km_batch_sizes(km_batch_t* b, km_batch_sizes_t* sizes);
int km_batch_fetch(km_batch_t* b, const km_batch_out_t* out);
/* Zero-copy variant: waits for the delivery of the last run (finishing, if some target needed
 * it, the large-workspace tier first) and points `view` into the batch's pinned host buffer;
 * the arrays stay valid until the next km_batch_run / km_batch_set_targets on this batch.
 * Either output may be NULL.  This is what `km find_mutation` needs per target
 * (km/tools/find_mutation.py:49-58) and what km_report_rows consumes. */
int km_batch_result(km_batch_t* b, km_batch_out_t* view, km_batch_sizes_t* sizes);
/* `steps` runs over `n` batches in flight, round robin (batch i % n on streams[i % n]): before a
 * batch is run again its previous delivery is awaited, at the end every batch's.  The loop of a
 * pipelined consumer (km/tools/find_mutation.py:47-58 over successive batches) without an
 * interpreter between the launches.
 * Consecutive steps are PAIRED where they can be: k_seed of the next batch runs as blocks of the previous batch's
 * k_dfs_pure launch (one kernel, k_dfs_pure_seed), so that the memory-bound k_seed fills what the latency-bound walk
 * leaves idle.  Paired steps do NOT run on streams[]: the pump takes three streams of the library's pool for the call.
 * One, the chain, gets the paired launch of every step, in order; the second, the tail, waits for an event
 * behind each paired launch and gets the rest of the walked batch's step (large tier, k_graph, delivery kernels, the
 * copy) — so those copies follow each other on one stream; the third, the front, gets k_pack of every next batch, and
 * the chain waits for an event behind it (KM_PUMP_FRONT=0 in the environment: k_pack on the chain, two streams).
 * During paired steps the callers' streams carry nothing: the front (for the first step of a run of paired steps, the
 * chain) first waits for whatever the caller has put on a batch's own stream — a km_batch_set_targets_dev just before
 * the call is seen by that batch's k_pack —, and when the call returns (also with an error) no batch refers to the
 * pump's streams any more and nothing of any batch is left on them.
 * A step CAN be paired when n >= 2, both batches have targets and the next one a walkable k-mer, both databases have
 * k = 31 or neither, the previous batch's k_dfs and k_graph_pure share a launch, its walk blocks (as many as its last
 * delivery reported flagged targets, + 25 %) are all resident on the device at once, and `stages` is plain walk +
 * graph + delivery (no KM_RUN_SERIAL, KM_RUN_HIPGRAPH, KM_RUN_TIMED*, KM_RUN_COUNT_FETCHES); every other step is
 * km_batch_run's own sequence on streams[i % n].  Results are the same either way.
 * One chain gives up the overlap of n streams, so by default such a step IS paired only where that pays: n <= 4
 * (more batches in flight is how a consumer hides the latency of small steps, and that needs their chains side by
 * side: paired, 8 batches of 1 250-5 000 targets ran 1.4-2.1 x slower), a lean delivery (KM_DELIVER_LEAN: a full
 * one is bound by its copies, which the tail would put one behind the other), and at least two seed blocks of the
 * next batch (one per 256 k-mers of a target, rounded up per target) for each of the device's 16 wave slots per
 * compute unit — 8 192 on 256 compute units, about 4 100 targets of 500 nt; below that the seeds are bound by latency
 * like the walk beside them and nothing is won.
 * KM_PUMP_UNPAIRED in `stages` (km_batch_run ignores both flags) or KM_PAIR_SEED=0 in the environment: no step is
 * paired.  KM_PUMP_PAIRED or KM_PAIR_SEED=2: every step that can be paired is, whether it pays or not (tests,
 * measurements); KM_PUMP_UNPAIRED wins over it. */
#define KM_PUMP_UNPAIRED 1024
#define KM_PUMP_PAIRED 2048
int km_batch_pump(km_batch_t* const* batches, void* const* streams, int n, int steps, int stages);
/* What the reference logs with -v from inside the walk and the graph, for the last run of `b` (any output may be
 * NULL): removed_ref_edges[n_targets] / nonref_edges[n_targets] — "Removed %d ref edges." (km/utils/Graph.py:198)
 * and "%d edges in non-ref edge set." (km/utils/Graph.py:231), in this library's node order (the reference's own
 * numbers move by one with its hash seed: its `if last_cur` skips whichever node happens to have index 0);
 * *n_loop_breaks — how often the walk met a k-mer on its stack that was not yet a node ("Broke loop at kmer",
 * km/utils/MutationFinder.py:160-161); loop_pairs[2 * min(*n_loop_breaks, 4096, loop_cap)] — {target, node index
 * of that k-mer} in walk order per target.  Waits for the run (and finishes what it left to the host). */
int km_batch_graph_log(km_batch_t* b, uint32_t* removed_ref_edges, uint32_t* nonref_edges,
                       uint32_t* n_loop_breaks, uint32_t* loop_pairs, uint32_t loop_cap);
/* Durations (ms) of the last run (it must have carried KM_RUN_TIMED; zeros otherwise) measured
 * with HIP events on the launch stream:
 * [0] walk stage (k_pack + k_seed + k_dfs), [1] graph stage, [2] walk + graph,
 * [3] k_seed, [4] k_pack, [5] k_dfs, [6] the delivery kernels (k_out_scan + k_out_pack),
 * [7] the device-to-host copy ([6], [7]: 0 unless the run carried KM_RUN_DELIVER).
 * Without KM_RUN_SERIAL a walk + graph run launches k_dfs and k_graph_pure as one kernel: [0] and [5] then contain
 * the pure-chain pass and [1] is that much shorter; with KM_RUN_SERIAL (or KM_FUSE_PURE=0) the pass counts in [1]. */
int km_batch_timings(km_batch_t* b, float* ms8);

/* ---- host reporting: replaces, for all targets of a fetched batch at once, the per-target
 *      tail of km/tools/find_mutation.py:53-58 — MutationFinder.graph_analysis' naming and
 *      quantification (km/utils/MutationFinder.py:190-373, 405-488, 575-833), PathQuant
 *      (km/utils/PathQuant.py:37-49, 93-154) and the row order.  Pure host code. */
typedef struct {
  uint32_t n_targets;
  const uint8_t* bases;          /* target sequences as given (ASCII), concatenated           */
  const uint64_t* base_off;      /* [n_targets+1]                                             */
  const char* const* names;      /* [n_targets] NUL-terminated query names                    */
  const char* db_name;           /* the Database column                                       */
  int32_t k;
  int32_t reserved;
  const km_batch_out_t* res;     /* arrays of km_batch_fetch or km_batch_result: everything but
                                    aux / probes / path_len; node_kmer may be NULL when
                                    extra_off / extra_kmer are given                          */
  const km_batch_sizes_t* sizes; /* the lengths of those arrays (km_batch_sizes / km_batch_result), or NULL.
                                    With them every offset array is checked against its array's length
                                    before anything is read (KM_E_ARG on a mismatch); without them the
                                    offsets are taken at their word.  Either way every node index of
                                    a path is checked against its target's node count: a target
                                    whose view is inconsistent gets err 5 and no rows, it is never
                                    read or written out of bounds.                                */
} km_report_in_t;
/* text: the TSV rows of every KM_T_OK target, each row terminated by '\n' (the text as a whole is
 * what `km find_mutation` prints between its header and its trailer);
 * row_off[t] .. row_off[t+1] is the block of target t (empty for other statuses);
 * err[t] != 0 where the reference would have raised while naming a variant
 * (1 IndexError, 2 "mutation identification could be incorrect", 3 AssertionError,
 * 4 ValueError, 5 = the view of this target is inconsistent — offsets not monotone, a path node
 * beyond the target's nodes, counts missing for a target that has variant paths; no rows then), or
 * 100 = rows delivered, but a printed rVAF / expression sits
 * within 1e-6 of a %.3f / %.1f rounding tie, where the last bits of the least-squares solver
 * decide the digit: a caller that needs the reference's exact text recomputes that target with
 * numpy (km_amd.lib.report_rows does).  Release the three arrays with km_report_free.
 * Threads: a team of KM_REPORT_THREADS workers (default min(cores, 16)) kept between calls; each worker places
 * itself on its own CPU once, when it is started, and keeps the process's affinity mask (KM_REPORT_SPREAD=0:
 * placement is left to the scheduler). */
int km_report_rows(const km_report_in_t* in, char** text, uint64_t** row_off, int32_t** err);
void km_report_free(char* text, uint64_t* row_off, int32_t* err);

/* Diagnostics: with KM_SEED_STAMPS set in the environment k_seed records, per wave, eight
 * s_memtime stamps (start, header, bases, minimizer scan, directory words, slots, resolved,
 * end), two s_memrealtime stamps (start, end) and the HW_ID placement, 16 words per wave.
 * dst == NULL only reports the size.  Stamped runs are slower; never use them for timing. */
int km_batch_debug_stamps(km_batch_t* b, uint64_t* dst, uint64_t cap_words, uint64_t* n_words);
/* Diagnostics: device counters of the last run — out4[0] flagged targets (k_seed), [1] unflagged targets
 * the pure-chain pass handed to k_graph, [2] flagged targets the epilogue of k_dfs left to k_graph, [3] a host counter: how
 * often, since the batch was made, its k_seed has run in another batch's walk launch (km_batch_pump's paired steps). */
int km_batch_debug_counts(km_batch_t* b, uint32_t* out4);
/* Diagnostics: a read-only look at an uploaded table — its directory (n_buckets + 1 words: bucket b owns the slots
 * [2 dir[b], 2 dir[b+1])) to dir[dir_cap words] and its slots (16 bytes each: u64 tag, ~0 if empty, then four u16
 * counts) to slots[slots_cap_bytes], copied synchronously.  *n_buckets / *n_slots always report the sizes; with dir
 * and slots both NULL nothing else happens.  KM_E_STATE before the upload, KM_E_ARG if a capacity is too small. */
int kmjf_debug_table(kmjf_t* h, uint32_t* dir, uint64_t dir_cap, void* slots, uint64_t slots_cap_bytes,
                     uint64_t* n_buckets, uint64_t* n_slots);

/* ---- linear_kmin -------------------------------------------------------------------------------
 * `km linear_kmin` (km/tools/linear_kmin.py:7-46) for a catalog: per target, the smallest k >= start at
 * which the target's k-mers are unique (km/utils/common.py:48-63: the ValueError / KM_T_REPEAT_KMER of
 * find_mutation) and their (k-1)-overlap graph is linear; as in the reference's loop, k is at most the
 * target's length unless start - 1 is larger (then k = start - 1).  Target t is bases[base_off[t] .. base_off[t+1]), ASCII, already upper-cased (any byte
 * is compared as is, N included).  Optional per-target outputs: longest_repeat = R, the longest repeated
 * substring (overlaps allowed), and nonexempt = some repeat of length R is not one of the pairs the
 * linearity test lets pass.  Blocks until the results are in host memory; device buffers
 * are sized to the call and freed before it returns; large inputs are staged in chunks.  KM_E_ARG, before
 * any HIP call, for NULL pointers, decreasing offsets or a target longer than 2^31 - 1; n_targets == 0
 * returns KM_OK without a launch.  stream: a hipStream_t, NULL = one of the library's own. */
int km_linear_kmin(int device, const uint8_t* bases, const uint64_t* base_off, uint32_t n_targets,
                   int32_t start, int32_t* kmin, int32_t* longest_repeat, uint8_t* nonexempt, void* stream);

/* ---- counting k-mers from reads -----------------------------------------------------------------
 * What `jellyfish count -m k [-C] -L lower_count -s expected_distinct` does in front of every km tool, on the
 * GPU: reads go into a counting hash table in HBM, and km_counter_finish turns that table into an ordinary
 * kmjf_t without the records visiting the host.  A byte of A C G T a c g t is a base, any other
 * byte a break (N, the newline between two reads); every window of k consecutive bases is one k-mer, stored
 * as min(key, revcomp(key)) when canonical.  Counts are exact up to 2^32 - 1; an input that repeats one k-mer
 * more often than that is out of scope (the count wraps).  One counter lives on one device and is used from
 * one host thread at a time; its copies and kernels run on a stream of its own. */
typedef struct km_counter km_counter_t;
typedef struct {
  uint64_t bases;        /* bytes accepted as bases                                    */
  uint64_t kmers;        /* windows counted (sum of all counts)                        */
  uint64_t distinct;     /* occupied slots                                             */
  uint64_t slots;        /* current capacity                                           */
  uint32_t n_grow;       /* how often the table doubled                                */
  uint32_t reserved;
} km_counter_stats_t;
/* state of the text stripper between calls: all zero before the first call of a stream */
typedef struct {
  int32_t  format;       /* 0 not known yet, 1 FASTA, 2 FASTQ                          */
  int32_t  line;         /* FASTQ: line of the record the next line is (0..3)          */
  int32_t  open;         /* FASTA: bases were written since the last break             */
  int32_t  reserved;
  uint64_t offset;       /* bytes consumed by the earlier calls of this stream         */
} km_text_state_t;

/* expected_distinct plays the part of Jellyfish's -s: the table starts with the next power of two at or above
 * twice that many slots (the load limit is 1/2); 0 = a small default (65 536 slots).  The table doubles when
 * it has to, so a wrong guess costs time, never correctness.  KM_E_K for k outside 2..32. */
int km_counter_create(int device, int k, int canonical, uint64_t expected_distinct, km_counter_t** out);
/* bases and breaks as described above; k-mers never span two calls.  n == 0 is KM_OK without a launch. */
int km_counter_add_bases(km_counter_t* c, const uint8_t* bytes, uint64_t n);
/* FASTA (multi-line records) or 4-line FASTQ text, chosen by the first byte ('>' or '@'); "\r\n" is accepted.
 * Whole lines are taken: a call may end in mid-line, *consumed says how much was taken, and the caller passes
 * the rest again in front of the next block; final != 0 on the last call of a stream (the last line then needs
 * no newline, and the next call may start a stream of the other format).  KM_E_FORMAT for a first byte that is
 * neither, a FASTQ record that does not start with '@' or lacks its '+' line; km_last_error names the byte
 * offset within the stream. */
int km_counter_add_text(km_counter_t* c, const char* text, uint64_t n, int final, uint64_t* consumed);
/* 4-line FASTQ text as it is, parsed on the GPU, with the quality masking of `jellyfish count -Q CHAR`
 * (--min-qual-char; km's own counting command, example/run_leucegene.sh:22, passes '-Q+'): a base whose quality
 * byte is below min_qual_char is read as N.  The comparison is strict and on the raw byte (no Phred offset), which
 * is this project's reading of Jellyfish 2's option, not checked against a run of it; 0 masks nothing and then
 * counts what km_counter_add_text counts.  The text is strict: line 4r starts with '@', line 4r+2 with '+', line
 * 4r+3 is as long as line 4r+1 (a '\r' before the newline is dropped from both first), and — unlike
 * km_counter_add_text — no blank lines between or behind records.  Whole records are taken, up to km_fastq_cut
 * of the text; *consumed says how much, and the caller passes the rest again in front of the next block; with
 * final != 0 everything is taken and the last line needs no newline.  The text goes to the device in pieces of
 * whole records (no k-mer spans two pieces, or a change between this call and add_bases / add_text), where kernels
 * find the lines, pair every base with its quality byte and hand a stream of bases and breaks to the insert kernel.
 * KM_E_ARG for min_qual_char outside 0..255; KM_E_CAPACITY, naming the offset, for a record longer than a staging
 * buffer (16 MiB).  A malformed record is found ASYNCHRONOUSLY, by the device: KM_E_FORMAT comes from the next
 * call on this counter that waits for the device (a later add_* that has to grow the table, km_counter_stats,
 * km_counter_finish), km_last_error names the kind and the smallest offending byte offset within the stream (all
 * calls since the last final one), and every further call on the counter returns KM_E_FORMAT too. */
int km_counter_add_fastq(km_counter_t* c, const char* text, uint64_t n, int final, int min_qual_char,
                         uint64_t* consumed);
/* Host only.  *cut = the largest offset <= n at which a record of 4-line FASTQ text ends: one past the newline of
 * a quality line whose record is all there, 0 if no record is complete.  A header is told from a quality line that
 * starts with '@' by the line two below it, which starts with '+' only below a header.  Found by walking back from
 * the end over a handful of lines, not by a pass over the text. */
int km_fastq_cut(const char* text, uint64_t n, uint64_t* cut);
/* With KM_COUNT_TIME_FASTQ=1 in the environment of the first km_counter_add_fastq call: the time of the line-table
 * and mask kernels of all pieces so far, by HIP events on the counter's stream (waits for it); 0 otherwise. */
int km_counter_fastq_kernel_ms(km_counter_t* c, float* ms);
/* waits for everything added so far */
int km_counter_stats(km_counter_t* c, km_counter_stats_t* s);
/* compacts (count >= lower_count), builds the lookup table on the counter's device through the same path
 * as kmjf_upload_from_device, frees the counting table; *out is an ordinary kmjf_t (kmjf_info, batches,
 * queries, kmjf_close).  The counter may only be destroyed afterwards (and asked for its stats and records):
 * KM_E_STATE for add_* after finish or a second finish. */
int km_counter_finish(km_counter_t* c, uint32_t lower_count, kmjf_t** out);
/* after finish: copy the compacted records to the host (for writing a file), in no particular order;
 * keys / counts may be NULL to ask for *n only; KM_E_CAPACITY if cap < n */
int km_counter_records(km_counter_t* c, uint64_t* keys, uint32_t* counts, uint64_t cap, uint64_t* n);
int km_counter_destroy(km_counter_t* c);
/* The text stripper of km_counter_add_text alone, host only (no device is touched): writes the byte stream the
 * counter would stage — sequence bytes, one '\n' where a read ends — to out[cap]; n bytes of text give at most
 * n + 1 (KM_E_CAPACITY if cap is smaller, before anything is written). */
int km_text_strip(km_text_state_t* st, const char* text, uint64_t n, int final, uint8_t* out, uint64_t cap,
                  uint64_t* n_out, uint64_t* consumed);

/* ---- files in Jellyfish's own record order ------------------------------------------------------
 * Real Jellyfish orders the records of a `binary/sorted` file by pos(key) = M . key over GF(2) — M is the
 * header's matrix1: r rows, c = 2k columns, bit i of the key (0 = least significant) selects columns[c-1-i],
 * the result is masked with size - 1 — and binary-searches that order; ties are ordered by key (DESIGN.md 10,
 * "File, Jellyfish order").  The functions below sort records that way on the GPU and write such files. */
/* Host only.  A deterministic matrix of r = size_log2 rows and 2k columns with full row rank, made from a seeded
 * mixer (reseeded until the rank is full).  KM_E_K for k outside 2..32, KM_E_ARG unless 1 <= size_log2 <= 2k. */
int km_jf_matrix(int k, int size_log2, uint64_t seed, uint64_t* columns /* [2k] */);
/* Host arrays in and out: records[n * (ceil(2k/8) + 4)] receives the file records ([little-endian key bytes]
 * [4 count bytes]) in (pos, key) order under the caller's matrix, pos_or_null[n] their positions in that order.
 * The keys are expected to be distinct (records with one key have no defined order among themselves).  n == 0
 * returns KM_OK without a launch; KM_E_ARG for n >= 2^32 (32-bit bucket directory) and, like KM_E_K, for the
 * shapes km_jf_matrix refuses, before any HIP call.  stream: a hipStream_t, NULL = one of the library's own. */
int km_jf_sort_records(int device, const uint64_t* columns, int k, int size_log2, const uint64_t* keys,
                       const uint32_t* counts, uint64_t n, uint8_t* records, uint64_t* pos_or_null, void* stream);
/* The last sort of the calling thread (km_jf_sort_records, km_counter_write_jf): out4[0] buckets, [1] entries of
 * the largest bucket, [2] buckets too large for the sort in LDS (sorted in global memory instead), [3] 0. */
int km_jf_sort_stats(uint64_t* out4);
/* ... and the time of its kernels (position, scan, scatter, sort), measured with HIP events on its stream. */
int km_jf_sort_kernel_ms(float* ms);
/* Host only.  The header of a file of n records in this order — 9 digits, JSON with sorted keys, padding to 8
 * bytes — with size = the power of two >= max(16, 2n), at most 4^k, and matrix1 = km_jf_matrix(k, log2 size,
 * seed), both also returned.  cmdline_json: a JSON array, NULL = ["km_amd","count"]; it is pasted into the header
 * as it is, so the caller answers for its being valid JSON — only its brackets are checked (KM_E_ARG unless it
 * begins with '[' and ends with ']').  out == NULL asks for *len only; KM_E_CAPACITY if cap < *len. */
int km_jf_header(int k, int canonical, uint64_t n, uint64_t seed, const char* cmdline_json, char* out,
                 uint64_t cap, uint64_t* len, uint64_t* columns /* [2k] */, int* size_log2);
/* After km_counter_finish (KM_E_STATE before): sort the device-resident records, write the km_jf_header of
 * (k, canonical, n, seed, cmdline_json) and the records to `path`.  The records never visit the host as arrays:
 * the finished file bytes are drained through the counter's pinned staging buffers piece by piece.  The file is
 * created before anything runs on the device: KM_E_IO if it cannot be created or written, and whenever the call
 * fails after that the partial file is removed. */
int km_counter_write_jf(km_counter_t* c, const char* path, const char* cmdline_json, uint64_t seed);

/* ---- merging tables that already exist ------------------------------------------------------------
 * Records of `binary/sorted` files, or of host arrays, go into a counter's table with their counts (DESIGN.md 10,
 * "Merging tables"): per key the counts are summed, saturating at 2^32 - 1 (KM_MERGE_SUM), or their maximum is
 * kept (KM_MERGE_MAX); the result does not depend on the order of arrival.  Saturation belongs to this record path
 * only: counting from reads (add_bases / add_text / add_fastq) keeps its wrapping add.  Reads and records may feed
 * one counter; km_counter_stats' bases / kmers tally text only, distinct stays exact.  These are this project's own
 * semantics of "merge", not checked against a run of `jellyfish merge`. */
#define KM_MERGE_SUM 0
#define KM_MERGE_MAX 1
/* Host only, header only: no device is touched, no record is read.  *n_records = the record area's length divided by
 * the record size (key_bytes + counter_len); any output may be NULL.  KM_E_IO / KM_E_FORMAT / KM_E_K as kmjf_open
 * gives them for the same file. */
int km_jf_file_info(const char* path, int32_t* k, int32_t* canonical, uint64_t* n_records, int32_t* key_bytes,
                    int32_t* counter_len);
/* n (key, count) pairs; a pair with count 0 is skipped, a key may occur more than once (combined by the mode), and
 * keys are stored as given: a non-canonical key in a canonical counter stays unreachable by lookups.  Text staged
 * by an earlier add_bases / add_text is flushed first.  The pairs are packed into file records inside the pinned
 * staging buffers and enqueued piece by piece; the call returns without waiting for the device.  Before any device
 * work, the counter left as it was: KM_E_ARG for NULL arguments or a mode other than the two, KM_E_STATE after
 * km_counter_finish, a sticky FASTQ format error as every add_* returns it.  n == 0 is KM_OK without a launch. */
int km_counter_add_records(km_counter_t* c, const uint64_t* keys, const uint32_t* counts, uint64_t n, int mode);
/* The same for the record area of a file, read with pread into the pinned staging buffers piece by piece (whole
 * records; the file is never in HBM as a whole).  *n_records (may be NULL): the records in the file.  Besides the
 * above, before any device work: KM_E_IO / KM_E_FORMAT / KM_E_K from the header as kmjf_open gives them, KM_E_ARG
 * for a file whose k or canonical differs from the counter's (km_last_error names both and the path).  A file
 * without records is KM_OK without a launch.  KM_E_IO if the file ends before its records do (what was enqueued
 * before stays added). */
int km_counter_add_jf(km_counter_t* c, const char* path, int mode, uint64_t* n_records);
/* Waits for everything added so far.  *records_in: records taken with count > 0 by the two calls above since the
 * counter was made; *kernel_ms: with KM_COUNT_TIME_MERGE=1 in the environment of km_counter_create, the time of
 * their kernels by HIP events on the counter's stream, 0 otherwise.  Either may be NULL. */
int km_counter_merge_stats(km_counter_t* c, uint64_t* records_in, float* kernel_ms);

/* ---- set operations over tables that already exist ---------------------------------------------------
 * The opposite kind of merge ("Set operations").  Every call below that feeds records is ONE input,
 * however many staging pieces it spans, and an input without records is an input too:
 *   KM_SET_INTERSECT  the keys present, with count > 0, in every input; the count is the minimum over all their
 *                     records (a key that repeats inside one input takes part with the minimum of its records there
 *                     and still is one input);
 *   KM_SET_SUBTRACT   the records of the FIRST input whose key occurs, with count > 0, in no later input; the count is
 *                     the first input's, a key that repeats inside it summed with saturation as by KM_MERGE_SUM.
 * A record with count 0 is absent: in a later input of subtract it removes nothing.  With one input both are filters.
 * The first input claims slots and may grow the table; later inputs only look keys up, so the table never grows after
 * the first, whatever its size.  The result depends neither on the order of the records nor on the piece size, and,
 * inputs 2..N being interchangeable by definition, not on their order.  These are THIS PROJECT'S OWN definitions, not
 * checked against a run of `jellyfish merge --min` or any other tool.
 * State (each refusal before any device work, the counter left as it was): a counter that has taken text, FASTQ or
 * sum / max records refuses the set calls, a counter that has taken a set call refuses those and the other operation
 * (KM_E_STATE, km_last_error names which); KM_E_ARG for NULL arguments or an op other than the two.  km_counter_stats'
 * distinct counts the keys of the first input; km_counter_merge_stats tallies the records and kernels of these calls
 * too.  km_counter_histo of such a counter is refused (KM_E_STATE) until it has finished: its live table holds keys that
 * do not survive.  km_counter_finish keeps lower_count <= count, as km_counter_finish_range with upper 2^32 - 1. */
#define KM_SET_INTERSECT 0
#define KM_SET_SUBTRACT 1
/* n (key, count) pairs as one input, packed and enqueued as km_counter_add_records does; n == 0 is an empty input. */
int km_counter_set_records(km_counter_t* c, const uint64_t* keys, const uint32_t* counts, uint64_t n, int op);
/* The record area of a file as one input, read as km_counter_add_jf reads it, with its checks of the header and of k /
 * canonical and their messages; *n_records (may be NULL): the records in the file. */
int km_counter_set_jf(km_counter_t* c, const char* path, int op, uint64_t* n_records);
/* km_counter_finish with a cut on both sides: keeps lower_count <= count <= upper_count (upper < lower keeps nothing
 * and is no error).  For every counter: reads, sum / max records, set operations.  Everything after finish
 * (km_counter_records, km_counter_write_jf, km_counter_histo, km_counter_dump) works on what was kept. */
int km_counter_finish_range(km_counter_t* c, uint32_t lower_count, uint32_t upper_count, kmjf_t** out);

/* ---- comparing tables that already exist -----------------------------------------------------------
 * How several tables relate to each other ("Compare"): every call below that feeds records is ONE input,
 * however many staging pieces it spans; inputs are numbered 0 .. n - 1 in the order of the calls, an input without
 * records is an input too, and a counter takes at most 32.  All inputs are of the counter's k and canonical setting.
 *   Set of an input.  Input i is the set S_i of the keys of its records with lower <= count <= upper.  A record with
 *     count 0 is absent whatever lower is.  The cut is applied per record: a key that appears in several records of one
 *     input is in S_i if ANY of them passes the cut, and feeding a record twice changes nothing (membership is
 *     idempotent).  upper < lower is an empty set and no error.
 *   Result.  shared[i][j] = |S_i & S_j|, symmetric, shared[i][i] = |S_i|.  union = |S_0 | .. | S_n-1|.
 *     in_exactly[m], 1 <= m <= n, = the keys held by exactly m inputs; in_exactly[n] is the core.  private[i] = the keys
 *     held by input i alone.  All values are 64-bit integers and exact.
 * The result depends neither on the order of the records nor on the piece size.  On the device a key's count cell holds
 * the 32-bit mask of the inputs that have it, so every input crosses to the device once, whatever the number of pairs,
 * and any input may grow the table (the mask moves with the key).  These are THIS PROJECT'S OWN definitions.
 * State (each refusal before any device work, the counter left as it was and still usable; KM_E_STATE unless said
 * otherwise, km_last_error names which): a counter that has taken text, FASTQ, sum / max or set records refuses the mark
 * calls, and a counter that has taken a mark call refuses all of those; a 33rd mark call is KM_E_CAPACITY; a counter
 * with a filter or a sketch takes no records.  km_counter_finish / _finish_range, _records, _write_jf, _histo and _dump
 * of such a counter are refused: its count cells are not counts.  km_counter_stats' distinct counts the union so far;
 * km_counter_merge_stats tallies the records that passed the cut and, with KM_COUNT_TIME_MERGE=1, the marking kernels. */
typedef struct {
  uint32_t n_inputs;              /* mark calls so far                                                          */
  float kernel_ms;                /* with KM_COUNT_TIME_MERGE=1 when the counter was made: the time of every pass
                                     of km_counter_cooccurrence over the table so far, by HIP events; 0 otherwise */
  uint64_t n_union;               /* union                                                                      */
  uint64_t shared[32 * 32];       /* shared[i * 32 + j], the full symmetric matrix; 0 at i or j >= n_inputs     */
  uint64_t in_exactly[33];        /* [m], 1 <= m <= n_inputs; [0] is 0                                          */
  uint64_t private_to[32];        /* private[i]                                                                 */
} km_cooc_t;
/* n (key, count) pairs as the next input, packed and enqueued as km_counter_add_records does; n == 0 is an empty input. */
int km_counter_mark_records(km_counter_t* c, const uint64_t* keys, const uint32_t* counts, uint64_t n, uint32_t lower,
                            uint32_t upper);
/* The record area of a file as the next input, read as km_counter_add_jf reads it, with its checks of the header and of
 * k / canonical and their messages (a refused file is no input); *n_records (may be NULL): the records in the file.
 * A call that fails AFTER those checks (KM_E_IO because the file ends before its records do, KM_E_NOMEM / KM_E_CAPACITY
 * because the table cannot grow; the same holds for km_counter_mark_records) has taken its ordinal: it is an input, one
 * of the 32, whose set is the records of the pieces enqueued before the failure.  The counter stays usable, but its
 * result then speaks of that partial input: start over with a new counter for the numbers of the whole files. */
int km_counter_mark_jf(km_counter_t* c, const char* path, uint32_t lower, uint32_t upper, uint64_t* n_records);
/* The result over the inputs so far, in one streaming pass over the table, which is left as it was: it may be called
 * between inputs and more than once (waits for everything enqueued).  T^32 of a non-canonical k = 32 table, which has
 * no slot, is folded into every number on the host.  Without any input every number is 0. */
int km_counter_cooccurrence(km_counter_t* c, km_cooc_t* out);

/* ---- counting only a given set of k-mers -----------------------------------------------------------
 * What `jellyfish count --if FILE` is for ("Filtered counting"): a counter may be given a FILTER once,
 * before it has been fed anything.  The filter is a set of k-mers in the counter's key encoding; for a canonical
 * counter a key is replaced by min(key, reverse complement) on the device, so the caller need not canonicalise.  Keys
 * may repeat; an empty set is a valid filter and counts nothing.  From then on km_counter_add_bases / _add_text /
 * _add_fastq (with its quality masking as before) add 1 to a window's key ONLY IF THAT KEY IS IN THE FILTER.  Every
 * key of the filter is in the table from the start with count 0, so km_counter_finish with lower_count 0 lists the
 * keys that never occurred with count 0 (T^32 of a non-canonical k = 32 counter too, when the filter holds it), and the
 * kmjf_t finished that way answers 0 for them, as for an absent key.  km_counter_stats_t keeps its meaning: bases and
 * kmers are all bases and all valid windows seen, distinct is the number of distinct filter keys, slots is fixed by
 * this call at the smallest power of two >= max(64, 2 * distinct), and n_grow stays 0: the table never grows.
 * km_counter_finish / _finish_range, _records, _write_jf, _dump and _histo work as on any counter.
 * State (each refusal before any device work, the counter left as it was and still usable): a counter that has been
 * fed refuses a filter, a second filter is refused, and a counter with a filter refuses km_counter_add_records,
 * _add_jf, _set_records and _set_jf (all KM_E_STATE).  KM_E_ARG for NULL arguments and for a key >= 4^k.
 * The counting pass runs in one of two tiers over the same table: while slots <= 8192 (at most 4096 distinct keys) a
 * block keeps the table's keys in LDS and touches HBM for a hit alone; a larger set is looked up in HBM.  Either tier
 * leaves the same table.  KM_COUNT_FILTER_LDS=0 in the environment of this call forces the HBM tier and
 * KM_COUNT_FILTER_BLOCKS=n caps the grid; neither changes a result.
 * These semantics are THIS PROJECT'S READING of `--if`, not checked against a run of Jellyfish. */
int km_counter_set_filter(km_counter_t* c, const uint64_t* keys, uint64_t n);
/* Waits for everything added so far.  *n_keys: the distinct keys of the filter (0 without one); *kmers_hit: the
 * windows counted, i.e. the sum of all counts; *tier: 0 no filter, 1 LDS, 2 HBM; *lds_keys: the most distinct keys the
 * LDS tier takes (a constant of the library, answered with or without a filter); *kernel_ms: with
 * KM_COUNT_TIME_FILTER=1 in the environment of km_counter_create, the time of the counting kernels (filtered, or the
 * plain insert kernel of a counter without a filter) by HIP events on the counter's stream, 0 otherwise.  Any output
 * may be NULL. */
int km_counter_filter_stats(km_counter_t* c, uint64_t* n_keys, uint64_t* kmers_hit, int* tier /* 0 none, 1 LDS, 2 HBM */,
                            uint64_t* lds_keys /* most distinct keys the LDS tier takes */, float* kernel_ms);

/* ---- solid k-mers: keeping the k-mers seen once out of the table, in two passes ------------------
 * What `jellyfish bc` + `jellyfish count --bc` are for ("Solid k-mers, two passes"): in real reads most
 * distinct k-mers are sequencing errors that occur once, and every user of a table cuts them away.  A counter may be
 * given a SKETCH once, before it has been fed anything and instead of a filter.  It is then fed TWICE: everything fed
 * until km_counter_sketch_done (pass 1) is only noted in the sketch, everything fed after it (pass 2) is counted, but
 * a window adds 1 to its key ONLY IF THE SKETCH ADMITS THE KEY.  The sketch admits every key that pass 1 saw at least
 * twice (no false negatives) and a few that it saw once or never (false positives, counted exactly like any key).
 * So when pass 2 is fed what pass 1 was fed, the records of km_counter_finish with lower_count >= 2 are exactly those
 * of a plain counter, while the table holds, and grows for, the admitted keys alone.  With lower_count < 2 the records
 * are a subset: the caller of this interface wants lower_count >= 2.  If pass 2 is fed OTHER text than pass 1, the
 * result is "the counts, in the second text, of the k-mers the first text admitted"; that is no error.
 * The rule (km_amd/csrc/sketch_rule.h; km_sketch_slot and km_sketch_words state it on the host):
 *   the sketch is `words` 64-bit words, a power of two, 64 <= words <= 2^40; the low 32 bits of a word are plane 1
 *   ("seen"), the high 32 bits plane 2 ("seen again");
 *   a key's slot: h = mix64(key ^ 0x9E3779B97F4A7C15) (the MurmurHash3 finalizer), word = h >> (64 - log2 words),
 *   mask = 1 << (h & 31) | 1 << (h >> 5 & 31) | 1 << (h >> 10 & 31), one to three bits;
 *   noting a key: if plane 2 of its word holds the mask already, nothing; otherwise the mask is OR-ed into plane 1
 *   atomically, and if plane 1 held it before, into plane 2 as well;
 *   the sketch admits a key iff plane 2 of its word holds its mask;
 *   km_sketch_words(n) = the smallest power of two >= max(64, ceil(n / 2)): two expected distinct k-mers per word.
 * T^32 of a non-canonical k = 32 counter (the key ~0) has no sketch entry: pass 2 always counts it, in its own cell.
 * Pass 1: km_counter_add_bases / _add_text / _add_fastq (with its quality masking) work as on any counter, and a
 * malformed FASTQ record is reported by this pass (km_counter_sketch_done at the latest).  bases and kmers of
 * km_counter_stats_t are tallied by pass 2 alone; distinct, slots and n_grow speak of the admitted keys.
 * State (each refusal before any device work, the counter left as it was and still usable; all KM_E_STATE):
 * km_counter_set_sketch on a counter that has been fed, has a sketch or has a filter; km_counter_set_filter,
 * _add_records, _add_jf, _set_records, _set_jf on a counter with a sketch; km_counter_finish / _finish_range, _records,
 * _histo, _dump, _write_jf before km_counter_sketch_done; km_counter_sketch_done twice or without a sketch.  KM_E_ARG
 * for a `words` that is no power of two or out of range.  KM_COUNT_FILTER_BLOCKS=n caps the grid of pass 1 too.
 * The flag and these semantics are THIS PROJECT'S OWN, not checked against a run of Jellyfish. */
int km_sketch_words(uint64_t expected_distinct, uint64_t* words);
int km_sketch_slot(uint64_t key, uint64_t words, uint64_t* word, uint32_t* mask);
int km_counter_set_sketch(km_counter_t* c, uint64_t words);
/* Ends pass 1: everything fed is enqueued and waited for, and the next add_* call starts a fresh stream (no k-mer
 * spans the two passes, a FASTQ stream's offsets start at 0 again). */
int km_counter_sketch_done(km_counter_t* c);
/* Waits for everything added so far.  *words: the sketch's size (0 without one); *bits_1 / *bits_2: the set bits of
 * plane 1 / plane 2 (final once pass 1 has ended); *kmers_noted: the windows pass 1 noted (all valid windows but those
 * of the key ~0); *kmers_admitted: the windows pass 2 counted in the table; kernel_ms[0], kernel_ms[1]: with
 * KM_COUNT_TIME_FILTER=1 in the environment of km_counter_create, the time of the kernels of pass 1 and of pass 2 by
 * HIP events on the counter's stream, 0 otherwise.  Any output may be NULL. */
int km_counter_sketch_stats(km_counter_t* c, uint64_t* words, uint64_t* bits_1, uint64_t* bits_2, uint64_t* kmers_noted,
                            uint64_t* kmers_admitted, float* kernel_ms /* [2] */);

/* ---- histogram of counts and table statistics -----------------------------------------------------
 * What `jellyfish histo` and `jellyfish stats` print, from counts that are already in HBM or from a file streamed
 * through it ("Histogram and statistics").  Both definitions are THIS PROJECT'S READING of the two
 * Jellyfish commands, not checked against a run of Jellyfish.
 * Keys looked at: a record or slot with count c takes part iff max(lower_count, 1) <= c <= upper_count (a count of 0
 * is not a key); bins and statistics see exactly those.
 * Bins, with 64-bit low <= high and increment >= 1:
 *   base   = low > 1 ? (increment >= low ? 1 : low - increment) : 1
 *   ceil   = high + increment
 *   n_bins = (ceil + increment - base) / increment                 (integer division)
 *   bin(c) = c < base ? 0 : c > ceil ? n_bins - 1 : (c - base) / increment
 * bin i is labelled base + i * increment; the defaults (1, 10000, 1) give 10 001 bins, the last one labelled 10001
 * and holding every count of 10 001 and above.
 * Statistics: unique = keys with count 1, distinct = keys, total = the 64-bit sum of their counts, max_count = the
 * largest count (0 if no key). */
typedef struct { uint64_t unique, distinct, total, max_count, reserved[2]; } km_histo_stats_t;

/* host only: the bin layout of (low, high, increment); either output may be NULL.  KM_E_ARG, km_last_error naming the
 * value, for increment == 0, low > high, high + 2 * increment beyond 64 bits, more than 2^24 bins. */
int km_histo_layout(uint64_t low, uint64_t high, uint64_t increment, uint64_t* base, uint64_t* n_bins);
/* A counter BEFORE finish (the counting table: everything added so far, waits for it, changes nothing the table
 * holds — the counter takes further add_* and finish afterwards) or AFTER finish (the kept records).  Before finish the
 * call enqueues what is staged, as km_counter_stats does: the pieces end where they would not have without the call,
 * so km_counter_stats_t.slots and n_grow (WHEN the table doubles) may differ from those of a counter never asked;
 * bases, kmers, distinct, the finished database and the records do not.  bins[cap] receives
 * n_bins values, KM_E_CAPACITY if cap is smaller; bins or stats may be NULL.  Before any device work: KM_E_ARG as
 * km_histo_layout, KM_E_CAPACITY; a sticky FASTQ format error as every call on the counter returns it. */
int km_counter_histo(km_counter_t* c, uint64_t low, uint64_t high, uint64_t increment, uint32_t lower_count,
                     uint32_t upper_count, uint64_t* bins, uint64_t cap, km_histo_stats_t* stats);
/* The record area of a binary/sorted file, read with pread into pinned staging piece by piece (whole records);
 * the file is never in host memory or HBM as a whole.  No counter is needed.  *k, *n_records (may be NULL): from the
 * header.  Before any device work: KM_E_ARG, KM_E_IO / KM_E_FORMAT / KM_E_K as kmjf_open gives them, KM_E_CAPACITY.
 * A file without records returns zeros without a launch.  stream: a hipStream_t, NULL = one of the library's own. */
int km_jf_histo(int device, const char* path, uint64_t low, uint64_t high, uint64_t increment, uint32_t lower_count,
                uint32_t upper_count, uint64_t* bins, uint64_t cap, km_histo_stats_t* stats, int32_t* k,
                uint64_t* n_records, void* stream);
/* Environment, read by the two calls above: KM_HISTO_ROUNDS = how many rounds a wave spends adding the lanes that hold
 * one bin as a single LDS atomic before the rest add on their own (0..64; the results are the same at any value; for
 * tests and measurement, the default is the measured choice of DESIGN.md 10); KM_COUNT_STAGE_BYTES sizes the pinned
 * buffers of km_jf_histo as it sizes a counter's. */
/* the time of the histogram kernels of the calling thread's last km_counter_histo / km_jf_histo, by HIP events */
int km_histo_kernel_ms(float* ms);
/* Host only, the text of the two commands.  km_histo_text: one line "<label> <n>\n" per bin with n > 0, or per bin
 * with full != 0; km_histo_stats_text: "Unique:    <n>\nDistinct:  <n>\nTotal:     <n>\nMax_count: <n>\n".
 * out == NULL asks for *len only; KM_E_CAPACITY if cap < *len (nothing is written). */
int km_histo_text(uint64_t base, uint64_t increment, const uint64_t* bins, uint64_t n_bins, int full, char* out,
                  uint64_t cap, uint64_t* len);
int km_histo_stats_text(const km_histo_stats_t* stats, char* out, uint64_t cap, uint64_t* len);

/* ---- dump and query: records as text ----------------------------------------------------------------
 * What `jellyfish dump [-c [-t]] [-L lower] [-U upper]` and `jellyfish query` print, the text built on the device
 * from records that are in HBM or streamed through it ("Dump and query").  The rule below is THIS
 * PROJECT'S READING of the two commands, not checked against a run of Jellyfish: no Jellyfish binary was available.
 *   KM_DUMP_FASTA   ">COUNT\nMER\n"     the default of `jellyfish dump`
 *   KM_DUMP_COLUMN  "MER COUNT\n"       -c, and every line of `query`
 *   KM_DUMP_TAB     "MER\tCOUNT\n"      -c -t
 * MER: k letters, ACGT for 0..3, the first base from the most significant used bit pair (bits above 2k of a file's
 * key bytes are ignored).  COUNT: decimal, no padding, "0" for zero.  A record is printed iff lower <= count <= upper
 * (0 and 2^32 - 1 print all of them, a zero-count record of a file too; lower > upper prints nothing and is no error).
 * Lines come in the order of the input: file order, the order of km_counter_records, query order.  Nothing is sorted.
 * The longest line has k + 13 bytes. */
#ifndef KM_DUMP_FASTA
#define KM_DUMP_FASTA 0
#define KM_DUMP_COLUMN 1
#define KM_DUMP_TAB 2
#endif
/* records_in: records looked at; records_out: lines written; bytes_out: their bytes; pieces: how many pieces the
 * records were cut into (a piece's text fits one staging buffer: KM_COUNT_STAGE_BYTES / (k + 13) records at most) */
typedef struct { uint64_t records_in, records_out, bytes_out, pieces, reserved[4]; } km_dump_stats_t;

/* Host arrays in, text into out[cap].  *len is always the length of the whole text; KM_E_CAPACITY, naming both
 * numbers, if cap is smaller (out is then left untouched); out == NULL with cap 0 asks for *len only.  Before any
 * device work: KM_E_ARG for null arguments, a format other than the three, device < 0, k outside 2..32. */
int km_dump_text(int device, const uint64_t* keys, const uint32_t* counts, uint64_t n, int k, int format,
                 uint32_t lower, uint32_t upper, char* out, uint64_t cap, uint64_t* len, void* stream);
/* The record area of a binary/sorted file, read piece by piece as km_jf_histo reads it, as text to the descriptor
 * out_fd (short writes and EINTR are handled; any other failure of write is KM_E_IO with the system's message, and
 * nothing of the call is left running on the device).  Before any device work: KM_E_ARG as above, KM_E_IO for a
 * descriptor that is not open, KM_E_IO / KM_E_FORMAT / KM_E_K for the file as kmjf_open gives them.  A file without
 * records writes nothing.  stats may be NULL.  stream: a hipStream_t, NULL = one of the library's own. */
int km_jf_dump(int device, const char* path, int out_fd, int format, uint32_t lower, uint32_t upper,
               km_dump_stats_t* stats, void* stream);
/* After km_counter_finish (KM_E_STATE before): the kept records, in the order of km_counter_records, straight out of
 * HBM; the counter stays usable for km_counter_write_jf, km_counter_records and km_counter_histo. */
int km_counter_dump(km_counter_t* c, int out_fd, int format, uint32_t lower, uint32_t upper, km_dump_stats_t* stats);
/* `query`: one KM_DUMP_COLUMN line per k-mer with its count in the uploaded table (KM_E_STATE without one), 0 for a
 * k-mer that is not there, in the order given; duplicates repeat.  The k-mers are looked up and printed as they are
 * given: for a canonical database the caller passes min(k-mer, reverse complement). */
int kmjf_query_text(kmjf_t* h, const uint64_t* kmers, uint64_t n, int out_fd, km_dump_stats_t* stats, void* stream);
/* the time of the sizes / scan / write kernels of the calling thread's last call of the four above, by HIP events */
int km_dump_kernel_ms(float* ms);

/* ---- scan: the k-mers of sequences, cut and looked up on the device ------------------------- */
/* Sequences go to the device as text; their k-mers are cut there and looked up in the uploaded table.  The rule:
 *   A sequence is a run of bytes.  ACGTacgt are bases; every other byte is a non-base.
 *   A window is k consecutive bytes of ONE sequence.  Windows never span two sequences; a sequence shorter than k
 *   has none.
 *   A window is valid iff all k bytes are bases.  A window with a non-base is skipped.
 *   The count of a valid window is what kmjf_query_batch returns for its packed k-mer (A 0, C 1, G 2, T 3, the first
 *   base in the most significant used bits): that of the canonical form for a canonical table, 0 for an absent k-mer.
 *   The k-mer printed is what `query` prints: min(k-mer, reverse complement) for a canonical table, the k-mer as
 *   given otherwise.
 * text holds the sequences end to end with nothing between them: sequence q is text[seq_off[q] .. seq_off[q + 1]).
 * seq_off has n_seqs + 1 entries and ascends; equal neighbours are an empty sequence.  No byte value is reserved.
 * A call takes at most KM_SCAN_MAX_SEQS sequences (KM_E_ARG beyond); the text has no limit of its own: it crosses
 * in pieces of KM_COUNT_STAGE_BYTES, and a sequence may span any number of them.
 * Both calls: KM_E_ARG for null pointers and for offsets that do not ascend, KM_E_STATE without an uploaded table;
 * with n_seqs == 0 or no bytes at all they return KM_OK and touch neither out nor the descriptor.
 * stream: a hipStream_t, NULL = one of the library's own.  Nothing of a call is left running on the device. */
#define KM_SCAN_MAX_SEQS (1ull << 26)
typedef struct {
  uint64_t total;      /* sum of the counts of the valid windows                      */
  uint64_t n_kmers;    /* valid windows                                               */
  uint64_t n_zero;     /* valid windows with count 0                                  */
  uint64_t n_skipped;  /* windows of this sequence with a non-base                    */
  uint64_t n_nonbase;  /* bytes of this sequence that are not ACGTacgt                */
  uint32_t min, max;   /* over the valid windows; 0xFFFFFFFF and 0 when n_kmers == 0  */
} km_cov_t;
/* out[n_seqs]: the statistics of every sequence (an empty one: zeros, min 0xFFFFFFFF).  All fields are integer sums,
 * minima and maxima: the result does not depend on how the work was spread. */
int kmjf_cov_seqs(kmjf_t* h, const uint8_t* text, const uint64_t* seq_off, uint64_t n_seqs, km_cov_t* out, void* stream);
/* One KM_DUMP_COLUMN line ("MER COUNT\n") per valid window to the descriptor out_fd, sequence after sequence, windows
 * in text order; a skipped window has no line.  stats (may be NULL): records_in = the windows of all sequences,
 * records_out = the lines written.  The descriptor is treated as kmjf_query_text treats it: KM_E_IO when it is not
 * open or a write fails, and the library goes on. */
int kmjf_scan_text(kmjf_t* h, const uint8_t* text, const uint64_t* seq_off, uint64_t n_seqs, int out_fd,
                   km_dump_stats_t* stats, void* stream);
/* the time of the scan kernels (extraction + lookup) of the calling thread's last call of the two above, by HIP events */
int km_scan_kernel_ms(float* ms);

/* ---- select: the FASTQ reads that hit a table, extracted on the device ---------------------- */
/* The rule:
 *   The input is strict 4-line FASTQ text as km_counter_add_fastq takes it, validated the same way (the same four
 *   kinds: no '@', no '+', quality line not as long as the sequence, incomplete record).  A '\r' in front of a newline
 *   is tolerated and is no base.
 *   Record r is lines 4r .. 4r + 3; its bytes run from the first byte of its header to the newline of its quality
 *   line, newlines included.
 *   hits(r) is the number of windows of k consecutive bytes of record r's sequence line whose k bytes are all ACGTacgt
 *   and whose k-mer has a count > 0 in the table (looked up as kmjf_cov_seqs does: the canonical form in a canonical
 *   table).  With min_qual_char != 0 a base whose quality byte is below it is a non-base first (`count -Q`'s rule).
 *   keep(r) = (hits(r) >= min_hits) != invert, with min_hits >= 1.
 *   The output is the kept records in input order, byte for byte as they came in: header, '+' line, qualities and
 *   '\r' untouched, the bases unmasked.  If the last record of a stream (final != 0) lacks its final newline and is
 *   kept, one '\n' is written behind it, so that two streams written to one descriptor do not run together.
 * Not covered: FASTA reads; more than one device.  (Mates of a pair kept together: km_select_pair_* below.) */
typedef struct km_select km_select_t;
typedef struct { uint64_t records_in, records_out, bytes_in, bytes_out, pieces, reserved[3]; } km_select_stats_t;
/* A selector over the uploaded table of h (which must outlive it) that writes to the descriptor out_fd.  stream: a
 * hipStream_t for all of its work, NULL = one of the library's own.  Before any device work: KM_E_ARG for null
 * pointers, min_hits == 0 or min_qual_char outside 0..255, KM_E_STATE without an uploaded table, KM_E_IO for a
 * descriptor that is not open. */
int km_select_create(kmjf_t* h, uint32_t min_hits, int invert, int min_qual_char, int out_fd, void* stream,
                     km_select_t** out);
/* text, n, final, *consumed as for km_counter_add_fastq: whole records are taken, the caller passes the rest again.
 * The text crosses in pieces of whole records of at most KM_COUNT_STAGE_BYTES; the kept records of a piece are
 * gathered on the device and only their bytes come back, while the next piece is staged and scanned; the host only
 * calls write().  When the call returns, everything it kept has been written.  n == 0 returns KM_OK and touches
 * nothing, except that an empty final call ends the stream: the offsets of the next one start at 0 again.
 * KM_E_CAPACITY, naming the stream offset, when no record ends within a staging buffer.  A malformed record:
 * KM_E_FORMAT from this very call, with the kind and the smallest offending stream offset (bytes since the last final
 * call) in km_last_error; the piece that holds it is not written, the pieces before it are.  KM_E_IO when a write
 * fails (EPIPE: the reader went away).  After any of these failures nothing of the call is left running on the
 * device and every further call on the selector fails with the same code and text. */
int km_select_add_fastq(km_select_t* s, const char* text, uint64_t n, int final, uint64_t* consumed);
/* bytes_out counts a newline written behind a last record without one */
int km_select_stats(km_select_t* s, km_select_stats_t* stats);
int km_select_destroy(km_select_t* s);
/* hits[r] = hits(r) for every record of text[0 .. n), whole records of any length (cut into pieces internally, the
 * last line needs no newline): the first half of the selection without the gather, for callers with a rule of their
 * own (mates of a pair, thresholds per read length).  *n_records: how many there are; KM_E_CAPACITY if more than cap.
 * Errors as above; n == 0 returns KM_OK with *n_records = 0. */
int kmjf_fastq_hits(kmjf_t* h, const char* text, uint64_t n, int min_qual_char, uint32_t* hits, uint64_t cap,
                    uint64_t* n_records, void* stream);
/* With KM_SELECT_TIME=1 in the environment of km_select_create / kmjf_fastq_hits (else no event is made and all are
 * 0): ms[4], the kernel time by HIP events of the selector, or the kmjf_fastq_hits call, that last finished a piece on
 * the calling thread, over all its pieces so far: [0] line table and mask, [1] clear and hits, [2] sizes and scan,
 * [3] the gather alone */
int km_select_kernel_ms(float* ms);

/* ---- select, pairs: the mates of a paired-end run kept together ----------------------------- */
/* The rule (this project's own definition: the reference has no paired selection to compare with):
 *   Two FASTQ streams, mate 1 and mate 2, whose records correspond one to one: record r of either is pair r.  Each
 *   stream is taken and validated as km_select_add_fastq takes one.
 *   h1(r), h2(r) are hits(r) of record r of mate 1 and of mate 2 exactly as defined above; the same table, k, canonical
 *   setting and quality masking apply to both mates.
 *   score(r) depends on the pair rule:
 *     KM_PAIR_ANY  (0, the default of the callers): max(h1, h2)
 *     KM_PAIR_BOTH (1): min(h1, h2)
 *     KM_PAIR_SUM  (2): h1 + h2, saturating at 2^32 - 1
 *   keep(r) = (score(r) >= min_hits) != invert.  A pair is kept or dropped whole; invert inverts the pair's decision.
 *   Mate 1's kept records go to one descriptor and mate 2's to another, both byte for byte and in input order, so record
 *   i of one output is the mate of record i of the other.
 *   The name check (on unless check_names == 0): the name of a record is the bytes of its header line behind '@', up to
 *   but not including the first space, tab, '\r' or '\n'.  If that name is at least two bytes long and ends in "/1" or
 *   "/2", those two bytes are dropped.  Mates agree iff their names are byte-equal.  The first pair that disagrees is a
 *   format error that names the pair's index within the stream (from 0, over all calls since the last final one) and the
 *   byte offsets of both headers within their streams.  With the check off, names are not looked at.
 *   When the final call arrives and one stream still holds a record while the other has none, that is a format error
 *   ("mate files differ in their number of records") that names the mate with more and the index of the first pair
 *   without a partner.
 *   A malformed record in either mate is reported as by km_select_add_fastq, with "mate 1" or "mate 2" in front.
 *   After any error, the whole pieces before the failing one are on both descriptors and the failing piece leaves nothing
 *   on either: each output is a prefix of what a fault-free run would write, and both prefixes end at the same pair.  The
 *   selector is dead afterwards, as a km_select_t is.  Where a stream holds several faults, which one is reported is
 *   not specified.
 *   A kept last record without a final newline gets one, decided in each output independently.
 * Not covered: interleaved input or output, orphan files for half-matching pairs, FASTA reads, more than one device. */
enum { KM_PAIR_ANY = 0, KM_PAIR_BOTH = 1, KM_PAIR_SUM = 2 };
typedef struct km_select_pair km_select_pair_t;
/* bytes_in: consumed, not counting bytes sent again; resent_bytes: the bytes of whole records that went to the device in
 * a piece, found no partner there and went again at the head of the next piece */
typedef struct {
  uint64_t pairs_in, pairs_out, bytes_in[2], bytes_out[2], pieces, resent_bytes[2], reserved[3];
} km_select_pair_stats_t;
/* As km_select_create, with the pair rule, the name check and a descriptor per mate.  KM_E_ARG in addition for an
 * unknown rule and for out_fd1 == out_fd2. */
int km_select_pair_create(kmjf_t* h, uint32_t min_hits, int invert, int min_qual_char, int rule, int check_names,
                          int out_fd1, int out_fd2, void* stream, km_select_pair_t** out);
/* text1/n1 and text2/n2 as text/n of km_select_add_fastq, one per mate; *consumed1, *consumed2 follow its protocol:
 * the caller passes the rest of either stream again in front of its next block.  A piece is one staging buffer's worth
 * of whole records from each stream; the device pairs the first R = min(records of the two) of them, the host advances
 * each stream by what those took, and the longer side's surplus records go to the device again with the next piece.
 * A non-final call in which either side holds no whole record consumes nothing of either and succeeds.  A final call
 * ends both streams: offsets and pair indices of the next ones start at 0.  Errors as above and as for
 * km_select_add_fastq. */
int km_select_pair_add_fastq(km_select_pair_t* s, const char* text1, uint64_t n1, const char* text2, uint64_t n2, int final,
                             uint64_t* consumed1, uint64_t* consumed2);
/* bytes_out counts a newline written behind a last record without one.  KM_SELECT_TIME=1 fills km_select_kernel_ms for a
 * pair selector too, both mates summed: [2] holds the pair's sizes, the name check and the scans, [3] the one gather. */
int km_select_pair_stats(km_select_pair_t* s, km_select_pair_stats_t* stats);
int km_select_pair_destroy(km_select_pair_t* s);

/* ---- select, labels: one output per label of a table, split on the device ------------------- */
/* The rule (this project's own definition: the reference has no labelled selection to compare with):
 *   A label table is an uploaded kmjf_t whose "count" of a k-mer is a 32-bit mask: bit l is set when the k-mer belongs to
 *   label l, 0 <= l < n_labels <= 32.  Bits at or above n_labels are ignored.  A mask of 0xFFFF or more lives in the
 *   table's overflow side table like any count of that size; kmjf_from_records sizes that table from the records, so any
 *   number of such keys is fine.
 *   The input, its validation, record r, the quality masking and the windows of a record are those of km_select above.
 *   hits_l(r) is the number of windows of k bytes of record r's sequence line that are all ACGTacgt after the masking and
 *   whose k-mer's mask has bit l.
 *   keep_l(r) = hits_l(r) >= min_hits, with min_hits >= 1.  There is no invert.
 *   Output l is the records with keep_l, byte for byte from the unmasked text, in input order.  A record kept by several
 *   labels is in each of their outputs.
 *   If the last record of a stream (final != 0) lacks its final newline, every output that ends with that record gets one
 *   '\n' behind it: km_select's rule, applied per output.
 *   The virtual stream of a piece is label 0's bytes of the piece, then label 1's, and so on; its length is the piece's
 *   total.  The device gathers it into an output buffer of km_select's size, cap bytes (the buffer rounded down to 16) per
 *   pass: pass p holds bytes [p * cap, min((p + 1) * cap, total)).  A piece takes max(1, ceil(total / cap)) passes;
 *   gather_passes counts them over all pieces.
 * Limits: n_labels * KM_COUNT_STAGE_BYTES < 2^32 (all offsets of a piece are 32-bit); device memory grows with n_labels:
 *   one hit plane of stage / 4 and one length plane of about stage / 6 entries per label.
 * Not covered: more than 32 labels (class ids instead of masks), pairs, invert, FASTA reads, more than one device. */
typedef struct km_select_labels km_select_labels_t;
/* records_any: records kept by at least one label, records_multi: by at least two */
typedef struct { uint64_t records_in, records_any, records_multi, bytes_in, pieces, gather_passes; } km_select_labels_stats_t;
/* As km_select_create, with out_fds[0 .. n_labels), label l's descriptor.  The checks come in km_select_create's order:
 * KM_E_ARG for null pointers, min_hits == 0, min_qual_char outside 0..255, n_labels == 0 or > 32 and two equal
 * descriptors; KM_E_STATE without an uploaded table; KM_E_IO for a descriptor that is not open; then KM_E_CAPACITY,
 * naming both numbers, when n_labels * KM_COUNT_STAGE_BYTES >= 2^32. */
int km_select_labels_create(kmjf_t* h, uint32_t n_labels, const int* out_fds, uint32_t min_hits, int min_qual_char,
                            void* stream, km_select_labels_t** out);
/* text, n, final, *consumed and every error as for km_select_add_fastq: a malformed record is KM_E_FORMAT with kind and
 * byte offset, a record longer than a staging buffer KM_E_CAPACITY, a failed write KM_E_IO; what the pieces before the
 * failing one kept is on the descriptors, and the selector is dead afterwards. */
int km_select_labels_add_fastq(km_select_labels_t* s, const char* text, uint64_t n, int final, uint64_t* consumed);
/* records_out[l], bytes_out[l] for l < n_labels; bytes_out counts a newline written behind a last record without one */
int km_select_labels_stats(km_select_labels_t* s, km_select_labels_stats_t* stats, uint64_t* records_out, uint64_t* bytes_out);
int km_select_labels_destroy(km_select_labels_t* s);
/* hits[l * cap + r] = hits_l(r) for every record of text[0 .. n), as kmjf_fastq_hits gives hits(r); KM_E_ARG in addition
 * for n_labels == 0 or > 32.  KM_SELECT_TIME=1 fills km_select_kernel_ms for both calls of this section, with the same
 * four spans: [2] holds the sizes of all labels, the one scan and the offsets, [3] every gather pass. */
int kmjf_fastq_label_hits(kmjf_t* h, uint32_t n_labels, const char* text, uint64_t n, int min_qual_char, uint32_t* hits,
                          uint64_t cap, uint64_t* n_records, void* stream);

/* ---- measurement helpers (bench.py at N = 1 holds no device buffers of its own) ------------- */
int km_device_sync(int device);                                    /* hipDeviceSynchronize on `device`          */
/* device-to-device copy of `bytes` bytes, `reps` times: read + write GB/s (the box's large-copy
 * rate beside the 8 TB/s spec) */
int km_device_copy_GBs(int device, uint64_t bytes, int reps, double* gbs);
/* the two probe kernels alone (rows A2 / A3: Jellyfish.query, get_child — km/utils/Jellyfish.py:47-72)
 * over `n` host k-mers: average launch time over `reps` launches each, and how many have count 0 */
int km_probe_bench(kmjf_t* h, const uint64_t* kmers, uint64_t n, int reps, double ratio, int64_t n_cutoff,
                   double* query_ms, double* children_ms, uint64_t* n_zero);

/* ---- misc ---------------------------------------------------------------- */
const char* km_strerror(int code);
const char* km_last_error(void);   /* thread-local detail of the last failure */
int km_device_count(int* n);
/* A non-blocking HIP stream on `device` for callers that do not bring their own. */
int km_stream_create(int device, void** stream);
int km_stream_destroy(void* stream);
const char* km_version(void);

#ifdef __cplusplus
}
#endif
#endif /* KMGPU_H */
