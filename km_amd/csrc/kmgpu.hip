// kmgpu.hip — libkmgpu.so: C-ABI (include/kmgpu.h) over the HIP kernels.
// Build: hipcc --offload-arch=gfx950 -O3 -fPIC -shared (see __graft_entry__.build()).
// One translation unit; the host code is in the parts included at the bottom, one per subsystem:
//   host_common.h  error plumbing, owners of device memory / events / streams, KernelSpans (timing by event pairs),
//                  Staging (two pinned buffers taking turns, either direction, and the one rule that governs them),
//                  the stream pool, CallStream (the caller's stream or one of the pool's), km_stream_*
//   db_host.h      the database: kmjf_* open / upload / broadcast / load, the lookups; what the file readers return
//                  as the library's codes (reader_result); RecordFile, the one reader of a file's record area
//   tier_geometry.h  what the LDS tier can hold (constants, fast_tier_fits)
//   batch_host.h   knobs, km_batch (what a batch owns), set_targets, one step: km_batch_run, km_batch_sync
//   result_host.h  reading a delivered step: km_batch_result / _pump / _fetch, diagnostics and measurement exports
//   kmin_host.h    km_linear_kmin
//   count_host.h   km_counter_*, km_text_strip, km_fastq_cut; the one way of text, FASTQ and record pieces through the
//                  counter's Staging (claim, counter_reserve, ship; counter_begin_pieces); the counter's mode (plain,
//                  filter in LDS / in HBM, sketch noting / counting) and launch_insert, the one switch over it
//   jf_order_host.h  km_jf_*, km_counter_write_jf: files in Jellyfish's own record order (out through the same Staging)
//   merge_host.h   km_jf_file_info, km_counter_add_records, km_counter_add_jf: records of existing tables, as pieces
//                  on the counter's staging
//   setops_host.h  km_counter_set_records, km_counter_set_jf, km_counter_finish_range: intersect / subtract over the
//                  inputs of one counter, as pieces on the counter's staging
//   histo_host.h   km_histo_*, km_counter_histo, km_jf_histo: the count histogram and the four statistics of a counter
//                  or a file in one streaming pass (a file: RecordFile, a Staging of the call's own, CallStream)
//   dump_host.h    km_dump_text, km_jf_dump, km_counter_dump, kmjf_query_text: records as the text of `dump` / `query`,
//                  formatted on the device piece by piece and written to a descriptor (a Staging in, a Staging out)
//   scan_host.h    kmjf_cov_seqs, kmjf_scan_text: the k-mers of sequences cut and looked up on the device, as per-sequence
//                  coverage statistics or as the text of `query` (a Staging in; the text through dump_host.h's DumpPipe)
//   select_host.h  km_select_*, kmjf_fastq_hits: the FASTQ records that hit the table, found and gathered on the device
//                  (count_host.h's front half of a FASTQ piece, a Staging in, the kept bytes out through TextDrain)
//   select_pair_host.h  km_select_pair_*: the same for the two mate streams of a paired-end run, kept or dropped as
//                  pairs (select_host.h's SelDev per mate, a Staging in and a TextDrain out per mate)
//   select_label_host.h  km_select_labels_*, kmjf_fastq_label_hits: the FASTQ records sorted into one output per label
//                  of a table whose counts are label masks (the same front half, a Staging in, one Staging out whose
//                  bytes LabelDrain cuts at the label boundaries; the last with templated kernels of its own)
//   filter_host.h  km_counter_set_filter, km_counter_filter_stats: a counter that counts only a given set of k-mers
//                  (the seed of its table, the tier and the cap of its bounded grid)
//   sketch_host.h  km_sketch_words, km_sketch_slot, km_counter_set_sketch, km_counter_sketch_done,
//                  km_counter_sketch_stats: a counter fed twice, whose table takes only the k-mers a first pass saw
//                  again (the sketch, the end of its first pass, its statistics)
//   mark_host.h    km_counter_mark_records, km_counter_mark_jf, km_counter_cooccurrence: the inputs of a comparison as
//                  membership masks in the count cells, pieces on the counter's staging, and the one pass over the table
//                  that counts what every pair of inputs shares (included last; its two kernels are not templates, and the
//                  compiler emits those ahead of the template instances: every existing kernel keeps its instructions)
// Their order is load-bearing: the templated kernels enter the code object in the order in which the host code
// first instantiates them, and the code object is compared byte for byte across host-only changes.  The two instances
// of k_count_filtered are instantiated by count_host.h's launch_insert since all counting kernels are launched from
// that one switch: they moved from the end of the code object, behind dump_host.h's six k_dump_* instances, to in
// front of those six (behind the walk kernels of batch_host.h).  No other kernel changed its place.
#include <hip/hip_runtime.h>
#include <chrono>
#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <map>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/kmgpu.h"
#include "count_kernel.h"
#include "deliver_kernel.h"
#include "device_common.h"
#include "dump_kernel.h"
#include "dump_text.h"
#include "fastq_cut.h"
#include "fastq_kernel.h"
#include "fastx_strip.h"
#include "graph_kernel.h"
#include "histo_kernel.h"
#include "histo_layout.h"
#include "jf_order_kernel.h"
#include "jf_reader.h"
#include "kmin_kernel.h"
#include "merge_kernel.h"
#include "merge_pieces.h"
#include "table_kernels.h"
#include "walk_kernel.h"
#include "setops_kernel.h"      // (after those above: the kernels before it keep their places in the code object)
#include "scan_kernel.h"
#include "scan_rule.h"
#include "select_kernel.h"
#include "select_rule.h"
#include "select_pair_kernel.h"
#include "select_pair_rule.h"
#include "filter_kernel.h"      // (behind those above: every kernel before it keeps its place in the code object)
#include "sketch_kernel.h"      // (behind filter_kernel.h, for the same reason)
#include "select_label_kernel.h"   // (behind sketch_kernel.h, for the same reason)
#include "select_label_rule.h"
#include "mark_kernel.h"        // (behind all others, with cooc_kernel.h: no existing kernel changes its instructions)
#include "cooc_kernel.h"
#include "cooc_rule.h"

using namespace kmd;

#include "host_common.h"
#include "db_host.h"
#include "tier_geometry.h"
#include "batch_host.h"
#include "result_host.h"
#include "kmin_host.h"
#include "count_host.h"
#include "jf_order_host.h"
#include "merge_host.h"
#include "setops_host.h"
#include "histo_host.h"
#include "dump_host.h"
#include "scan_host.h"
#include "select_host.h"
#include "select_pair_host.h"
#include "filter_host.h"
#include "sketch_host.h"        // (behind filter_host.h: it uses its grid cap)
#include "select_label_host.h"  // (behind select_host.h: its SelCore and span cells)
#include "mark_host.h"          // (behind all others: it instantiates no templated kernel)
