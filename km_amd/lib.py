"""ctypes binding of libkmgpu.so (include/kmgpu.h).

This is the whole Python<->native boundary: plain pointers and sizes, numpy
arrays own every in/out buffer.  There is NO CPU fallback — if the HIP library
is missing or cannot be loaded, :func:`load` raises.
"""

import atexit
import ctypes as C
import json
import os
import sys
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# KM_LIBRARY: another build of the same library (diagnostics builds of tools/); it must exist
LIB_PATH = os.environ.get("KM_LIBRARY") or os.path.join(_HERE, "libkmgpu.so")

KM_OK = 0
KM_STAGE_WALK, KM_STAGE_GRAPH, KM_RUN_HIPGRAPH, KM_RUN_DELIVER, KM_DELIVER_LEAN, KM_RUN_TIMED = 1, 2, 4, 8, 16, 32
KM_DELIVER_COUNT16 = 128        # node counts cross PCIe as 16-bit values + the list of the exact counts >= 65535
KM_RUN_COUNT_FETCHES = 256      # count the table slots read (sizes.table_fetches; a diagnostic, 2 % of a step)
KM_RUN_SERIAL = 64
KM_RUN_TIMED_STAGES = 512       # with KM_RUN_TIMED: stage boundaries only (no event records between the walk stage's kernels)
KM_PUMP_UNPAIRED = 1024         # km_batch_pump: every step is km_batch_run's own sequence (no k_seed in another batch's walk launch)
KM_PUMP_PAIRED = 2048           # km_batch_pump: pair every step that can be paired, not only where it pays (<= 4 batches, lean delivery, large batches)
T_OK, T_NODE_LIMIT, T_REPEAT_KMER, T_EMPTY, T_BAD_BASE, T_INTERNAL = range(6)

# every symbol include/kmgpu.h declares (tests check the library exports them all)
SYMBOLS = [
    "kmjf_open", "kmjf_load", "kmjf_from_records", "kmjf_create", "kmjf_close", "kmjf_info", "kmjf_records",
    "kmjf_upload", "kmjf_upload_from_device", "kmjf_broadcast", "kmjf_query_batch", "kmjf_children_batch",
    "kmjf_query_batch_dev", "kmjf_children_batch_dev", "km_batch_create", "km_batch_destroy",
    "km_batch_set_targets", "km_batch_set_targets_dev", "km_batch_run", "km_batch_sync",
    "km_batch_sizes", "km_batch_fetch", "km_batch_result", "km_batch_timings", "km_batch_graph_log", "km_batch_pump", "km_batch_debug_stamps", "km_batch_debug_counts",
    "kmjf_debug_table",
    "km_device_sync", "km_device_copy_GBs", "km_probe_bench",
    "km_report_rows", "km_report_free", "km_linear_kmin", "km_strerror", "km_last_error",
    "km_counter_create", "km_counter_add_bases", "km_counter_add_text", "km_counter_stats", "km_counter_finish",
    "km_counter_records", "km_counter_destroy", "km_text_strip",
    "km_counter_add_fastq", "km_fastq_cut", "km_counter_fastq_kernel_ms",
    "km_jf_matrix", "km_jf_sort_records", "km_jf_sort_stats", "km_jf_sort_kernel_ms", "km_jf_header",
    "km_counter_write_jf",
    "km_jf_file_info", "km_counter_add_records", "km_counter_add_jf", "km_counter_merge_stats",
    "km_counter_set_records", "km_counter_set_jf", "km_counter_finish_range",
    "km_counter_mark_records", "km_counter_mark_jf", "km_counter_cooccurrence",
    "km_counter_set_filter", "km_counter_filter_stats",
    "km_sketch_words", "km_sketch_slot", "km_counter_set_sketch", "km_counter_sketch_done", "km_counter_sketch_stats",
    "km_histo_layout", "km_counter_histo", "km_jf_histo", "km_histo_kernel_ms", "km_histo_text", "km_histo_stats_text",
    "km_dump_text", "km_jf_dump", "km_counter_dump", "kmjf_query_text", "km_dump_kernel_ms",
    "kmjf_cov_seqs", "kmjf_scan_text", "km_scan_kernel_ms",
    "km_select_create", "km_select_add_fastq", "km_select_stats", "km_select_destroy", "kmjf_fastq_hits",
    "km_select_kernel_ms",
    "km_select_pair_create", "km_select_pair_add_fastq", "km_select_pair_stats", "km_select_pair_destroy",
    "km_select_labels_create", "km_select_labels_add_fastq", "km_select_labels_stats", "km_select_labels_destroy",
    "kmjf_fastq_label_hits",
    "km_device_count", "km_stream_create", "km_stream_destroy", "km_version",
]


class KmError(RuntimeError):
    def __init__(self, code, detail):
        self.code = code
        self.detail = detail
        super().__init__("libkmgpu: %s" % detail)


class JfInfo(C.Structure):
    _fields_ = [("k", C.c_int32), ("canonical", C.c_int32), ("n_records", C.c_uint64),
                ("n_slots", C.c_uint64), ("n_groups", C.c_uint64), ("table_bytes", C.c_uint64),
                ("device", C.c_int32), ("max_probe", C.c_int32)]


class Params(C.Structure):
    _fields_ = [("ratio", C.c_double), ("count", C.c_int64), ("max_stack", C.c_uint32),
                ("max_break", C.c_uint32), ("max_node", C.c_uint32), ("reserved", C.c_uint32)]


class BatchSizes(C.Structure):
    _fields_ = [("n_targets", C.c_uint32), ("n_paths", C.c_uint32), ("n_nodes", C.c_uint64),
                ("n_runs", C.c_uint64), ("logical_probes", C.c_uint64),
                ("table_fetches", C.c_uint64), ("n_big_tier", C.c_uint32), ("n_flagged", C.c_uint32),
                ("seed_probes", C.c_uint64), ("n_extra", C.c_uint64),
                ("n_count_escapes", C.c_uint32), ("reserved", C.c_uint32)]


class CounterStats(C.Structure):
    """km_counter_stats_t (include/kmgpu.h)."""
    _fields_ = [("bases", C.c_uint64), ("kmers", C.c_uint64), ("distinct", C.c_uint64), ("slots", C.c_uint64),
                ("n_grow", C.c_uint32), ("reserved", C.c_uint32)]


class Cooc(C.Structure):
    """km_cooc_t"""
    _fields_ = [("n_inputs", C.c_uint32), ("kernel_ms", C.c_float), ("n_union", C.c_uint64),
                ("shared", C.c_uint64 * (32 * 32)), ("in_exactly", C.c_uint64 * 33), ("private_to", C.c_uint64 * 32)]


class HistoStats(C.Structure):
    """km_histo_stats_t (include/kmgpu.h)."""
    _fields_ = [("unique", C.c_uint64), ("distinct", C.c_uint64), ("total", C.c_uint64), ("max_count", C.c_uint64),
                ("reserved", C.c_uint64 * 2)]


class DumpStats(C.Structure):
    """km_dump_stats_t (include/kmgpu.h)."""
    _fields_ = [("records_in", C.c_uint64), ("records_out", C.c_uint64), ("bytes_out", C.c_uint64),
                ("pieces", C.c_uint64), ("reserved", C.c_uint64 * 4)]


class SelectStats(C.Structure):
    """km_select_stats_t (include/kmgpu.h)."""
    _fields_ = [("records_in", C.c_uint64), ("records_out", C.c_uint64), ("bytes_in", C.c_uint64),
                ("bytes_out", C.c_uint64), ("pieces", C.c_uint64), ("reserved", C.c_uint64 * 3)]


class SelectPairStats(C.Structure):
    """km_select_pair_stats_t (include/kmgpu.h)."""
    _fields_ = [("pairs_in", C.c_uint64), ("pairs_out", C.c_uint64), ("bytes_in", C.c_uint64 * 2),
                ("bytes_out", C.c_uint64 * 2), ("pieces", C.c_uint64), ("resent_bytes", C.c_uint64 * 2),
                ("reserved", C.c_uint64 * 3)]


class SelectLabelsStats(C.Structure):
    """km_select_labels_stats_t (include/kmgpu.h)."""
    _fields_ = [("records_in", C.c_uint64), ("records_any", C.c_uint64), ("records_multi", C.c_uint64),
                ("bytes_in", C.c_uint64), ("pieces", C.c_uint64), ("gather_passes", C.c_uint64)]


class TextState(C.Structure):
    """km_text_state_t (include/kmgpu.h)."""
    _fields_ = [("format", C.c_int32), ("line", C.c_int32), ("open", C.c_int32), ("reserved", C.c_int32),
                ("offset", C.c_uint64)]


# km_cov_t (include/kmgpu.h): the coverage statistics of one sequence
COV_DTYPE = np.dtype([("total", "<u8"), ("n_kmers", "<u8"), ("n_zero", "<u8"), ("n_skipped", "<u8"),
                      ("n_nonbase", "<u8"), ("min", "<u4"), ("max", "<u4")])
assert COV_DTYPE.itemsize == 48

_P16 = C.POINTER(C.c_uint16)
_P32 = C.POINTER(C.c_uint32)
_P64 = C.POINTER(C.c_uint64)


class BatchOut(C.Structure):
    _fields_ = [("status", _P32), ("aux", _P32), ("n_ref", _P32), ("probes", _P64),
                ("node_off", _P64), ("node_kmer", _P64), ("node_count", _P32),
                ("path_off", _P32), ("run_off", _P64), ("run_start", _P32), ("run_len", _P32),
                ("path_len", _P32), ("path_min_cov", _P32), ("extra_off", _P64), ("extra_kmer", _P64),
                ("ref_max_cov", _P32),
                ("node_count16", _P16), ("count_esc_node", _P64), ("count_esc_value", _P32)]


class ReportIn(C.Structure):
    """km_report_in_t (include/kmgpu.h)."""
    _fields_ = [("n_targets", C.c_uint32), ("bases", C.c_void_p), ("base_off", C.c_void_p),
                ("names", C.POINTER(C.c_char_p)), ("db_name", C.c_char_p), ("k", C.c_int32),
                ("reserved", C.c_int32), ("res", C.POINTER(BatchOut)), ("sizes", C.POINTER(BatchSizes))]


_lib = None

# Live native handles, closed at interpreter exit while the HIP runtime is still up: batches first
# (they reference their database), then databases.  Without this a handle that is still alive when
# Python tears its modules down is destroyed by __del__ in arbitrary order, possibly after the HIP
# runtime has unloaded its state (round 2: a SIGSEGV inside __cxa_finalize under rocprofv3).
_LIVE_COUNTERS = weakref.WeakSet()
_LIVE_BATCHES = weakref.WeakSet()
_LIVE_DATABASES = weakref.WeakSet()


def close_all_handles():
    for live in (_LIVE_COUNTERS, _LIVE_BATCHES, _LIVE_DATABASES):
        for handle in list(live):
            try:
                handle.close()
            except Exception:
                pass


class _Handle:
    """The life of one native handle, for every class that owns one: `_slot` names the attribute that holds it (a
    c_void_p; None once closed), `_destroy` the library call that frees it and `_live` the set close_all_handles walks.
    A subclass sets self._lib and the slot, makes the handle and calls _opened(); close() is safe to repeat, and runs
    from a `with` block, from the collector and at interpreter exit."""
    _slot = _destroy = _live = None

    def _opened(self):
        self._live.add(self)

    def close(self):
        h = getattr(self, self._slot, None)
        if h is not None and h.value:
            getattr(self._lib, self._destroy)(h)
        setattr(self, self._slot, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _records(keys, counts):
    """(keys, counts) as the contiguous uint64 / uint32 arrays the library takes, 1-d and of one length."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    if keys.shape != counts.shape or keys.ndim != 1:
        raise ValueError("keys and counts must be 1-d arrays of one length")
    return keys, counts


atexit.register(close_all_handles)


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so.7 (same
    SONAME as /opt/rocm's): whichever is loaded first serves both libkmgpu.so and torch, and torch
    finds no GPU when it is the system one.  So when torch is installed but not imported yet (a later
    `import torch` — km_amd.dist, bench.py — must keep working) ITS runtime is loaded first.
    KM_HIP_RUNTIME=system keeps the ROCm installation's (a process that will never import torch: a
    single-GPU `km find_mutation`, a C consumer); KM_HIP_RUNTIME=torch insists on torch's and fails
    loudly without it.  Returns a short description of what was bound (KM_VERBOSE_LOAD=1 prints it)."""
    import importlib.util
    want = os.environ.get("KM_HIP_RUNTIME", "")
    if "torch" in sys.modules:
        return "torch already imported: its HIP runtime serves libkmgpu.so"
    if want == "system":
        return "system HIP runtime (KM_HIP_RUNTIME=system)"
    try:
        spec = importlib.util.find_spec("torch")
    except Exception:
        spec = None
    if spec is None or not spec.origin:
        if want == "torch":
            raise ImportError("km_amd: KM_HIP_RUNTIME=torch but torch is not installed")
        return "system HIP runtime (no torch installed)"
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if not os.path.exists(cand):
        if want == "torch":
            raise ImportError("km_amd: KM_HIP_RUNTIME=torch but %s does not exist" % cand)
        return "system HIP runtime (torch ships no libamdhip64.so)"
    try:
        C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except OSError as exc:
        if want == "torch":
            raise ImportError("km_amd: cannot load %s: %s" % (cand, exc))
        sys.stderr.write("km_amd: could not preload torch's HIP runtime (%s): %s — libkmgpu.so binds the system one; "
                         "a later `import torch` may then find no GPU (KM_HIP_RUNTIME=system silences this)\n" % (cand, exc))
        return "system HIP runtime (preload of torch's failed)"
    return "torch's bundled HIP runtime %s (KM_HIP_RUNTIME=system to use the ROCm installation's)" % cand


HIP_RUNTIME_BOUND = None


def load():
    """Load libkmgpu.so (built in-tree by ``__graft_entry__.build()``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("km_amd: %s is missing — run `python -c 'import __graft_entry__ as g; "
                          "g.build()'` (there is no CPU fallback)" % LIB_PATH)
    global HIP_RUNTIME_BOUND
    HIP_RUNTIME_BOUND = _share_hip_runtime_with_torch()
    if os.environ.get("KM_VERBOSE_LOAD"):
        sys.stderr.write("km_amd: %s; library %s\n" % (HIP_RUNTIME_BOUND, LIB_PATH))
    lib = C.CDLL(LIB_PATH)
    vp, cp = C.c_void_p, C.c_char_p
    u32, u64, i32, i64, dbl = C.c_uint32, C.c_uint64, C.c_int, C.c_int64, C.c_double
    sig = {
        "kmjf_open": [cp, C.POINTER(vp)],
        "kmjf_load": [cp, i32, C.POINTER(vp)],
        "kmjf_from_records": [vp, vp, u64, i32, i32, C.POINTER(vp)],
        "kmjf_create": [i32, i32, C.POINTER(vp)],
        "kmjf_close": [vp],
        "kmjf_info": [vp, C.POINTER(JfInfo)],
        "kmjf_records": [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)],
        "kmjf_upload": [vp, i32],
        "kmjf_upload_from_device": [vp, i32, vp, vp, u64, vp],
        "kmjf_broadcast": [vp, C.POINTER(i32), i32, C.POINTER(vp)],
        "kmjf_query_batch": [vp, vp, u64, vp],
        "kmjf_children_batch": [vp, vp, u64, dbl, i64, i32, vp, vp],
        "kmjf_query_batch_dev": [vp, vp, u64, vp, vp],
        "kmjf_children_batch_dev": [vp, vp, u64, dbl, i64, i32, vp, vp, vp],
        "km_batch_create": [vp, C.POINTER(Params), u32, u64, C.POINTER(vp)],
        "km_batch_destroy": [vp],
        "km_batch_set_targets": [vp, vp, vp, u32],
        "km_batch_set_targets_dev": [vp, vp, vp, u32, vp],
        "km_batch_run": [vp, i32, vp],
        "km_batch_sync": [vp],
        "km_batch_sizes": [vp, C.POINTER(BatchSizes)],
        "km_batch_fetch": [vp, C.POINTER(BatchOut)],
        "km_batch_result": [vp, C.POINTER(BatchOut), C.POINTER(BatchSizes)],
        "km_batch_timings": [vp, C.POINTER(C.c_float)],
        "km_batch_graph_log": [vp, vp, vp, C.POINTER(u32), vp, u32],
        "km_batch_pump": [C.POINTER(vp), C.POINTER(vp), i32, i32, i32],
        "km_batch_debug_stamps": [vp, vp, C.c_uint64, C.POINTER(C.c_uint64)],
        "km_batch_debug_counts": [vp, C.POINTER(C.c_uint32)],
        "kmjf_debug_table": [vp, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64)],
        "km_report_rows": [C.POINTER(ReportIn), C.POINTER(vp), C.POINTER(C.POINTER(C.c_uint64)),
                           C.POINTER(C.POINTER(C.c_int32))],
        "km_linear_kmin": [i32, vp, vp, u32, i32, vp, vp, vp, vp],
        "km_counter_create": [i32, i32, i32, u64, C.POINTER(vp)],
        "km_counter_add_bases": [vp, vp, u64],
        "km_counter_add_text": [vp, vp, u64, i32, C.POINTER(u64)],
        "km_counter_add_fastq": [vp, vp, u64, i32, i32, C.POINTER(u64)],
        "km_fastq_cut": [vp, u64, C.POINTER(u64)],
        "km_counter_fastq_kernel_ms": [vp, C.POINTER(C.c_float)],
        "km_counter_stats": [vp, C.POINTER(CounterStats)],
        "km_counter_finish": [vp, u32, C.POINTER(vp)],
        "km_counter_records": [vp, vp, vp, u64, C.POINTER(u64)],
        "km_counter_destroy": [vp],
        "km_text_strip": [C.POINTER(TextState), vp, u64, i32, vp, u64, C.POINTER(u64), C.POINTER(u64)],
        "km_jf_matrix": [i32, i32, u64, vp],
        "km_jf_sort_records": [i32, vp, i32, i32, vp, vp, u64, vp, vp, vp],
        "km_jf_sort_stats": [vp],
        "km_jf_sort_kernel_ms": [C.POINTER(C.c_float)],
        "km_jf_header": [i32, i32, u64, u64, cp, vp, u64, C.POINTER(u64), vp, C.POINTER(i32)],
        "km_counter_write_jf": [vp, cp, cp, u64],
        "km_jf_file_info": [cp, C.POINTER(i32), C.POINTER(i32), C.POINTER(u64), C.POINTER(i32), C.POINTER(i32)],
        "km_counter_add_records": [vp, vp, vp, u64, i32],
        "km_counter_add_jf": [vp, cp, i32, C.POINTER(u64)],
        "km_counter_merge_stats": [vp, C.POINTER(u64), C.POINTER(C.c_float)],
        "km_counter_set_records": [vp, vp, vp, u64, i32],
        "km_counter_set_jf": [vp, cp, i32, C.POINTER(u64)],
        "km_counter_finish_range": [vp, u32, u32, C.POINTER(vp)],
        "km_counter_mark_records": [vp, vp, vp, u64, u32, u32],
        "km_counter_mark_jf": [vp, cp, u32, u32, C.POINTER(u64)],
        "km_counter_cooccurrence": [vp, C.POINTER(Cooc)],
        "km_counter_set_filter": [vp, vp, u64],
        "km_counter_filter_stats": [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(i32), C.POINTER(u64),
                                    C.POINTER(C.c_float)],
        "km_sketch_words": [u64, C.POINTER(u64)],
        "km_sketch_slot": [u64, u64, C.POINTER(u64), C.POINTER(u32)],
        "km_counter_set_sketch": [vp, u64],
        "km_counter_sketch_done": [vp],
        "km_counter_sketch_stats": [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64),
                                    C.POINTER(C.c_float)],
        "km_histo_layout": [u64, u64, u64, C.POINTER(u64), C.POINTER(u64)],
        "km_counter_histo": [vp, u64, u64, u64, u32, u32, vp, u64, C.POINTER(HistoStats)],
        "km_jf_histo": [i32, cp, u64, u64, u64, u32, u32, vp, u64, C.POINTER(HistoStats), C.POINTER(C.c_int32),
                        C.POINTER(u64), vp],
        "km_histo_kernel_ms": [C.POINTER(C.c_float)],
        "km_histo_text": [u64, u64, vp, u64, i32, vp, u64, C.POINTER(u64)],
        "km_histo_stats_text": [C.POINTER(HistoStats), vp, u64, C.POINTER(u64)],
        "km_dump_text": [i32, vp, vp, u64, i32, i32, u32, u32, vp, u64, C.POINTER(u64), vp],
        "km_jf_dump": [i32, cp, i32, i32, u32, u32, C.POINTER(DumpStats), vp],
        "km_counter_dump": [vp, i32, i32, u32, u32, C.POINTER(DumpStats)],
        "kmjf_query_text": [vp, vp, u64, i32, C.POINTER(DumpStats), vp],
        "km_dump_kernel_ms": [C.POINTER(C.c_float)],
        "kmjf_cov_seqs": [vp, vp, vp, u64, vp, vp],
        "kmjf_scan_text": [vp, vp, vp, u64, i32, C.POINTER(DumpStats), vp],
        "km_scan_kernel_ms": [C.POINTER(C.c_float)],
        "km_select_create": [vp, u32, i32, i32, i32, vp, C.POINTER(vp)],
        "km_select_add_fastq": [vp, vp, u64, i32, C.POINTER(u64)],
        "km_select_stats": [vp, C.POINTER(SelectStats)],
        "km_select_destroy": [vp],
        "kmjf_fastq_hits": [vp, vp, u64, i32, vp, u64, C.POINTER(u64), vp],
        "km_select_kernel_ms": [C.POINTER(C.c_float)],
        "km_select_pair_create": [vp, u32, i32, i32, i32, i32, i32, i32, vp, C.POINTER(vp)],
        "km_select_pair_add_fastq": [vp, vp, u64, vp, u64, i32, C.POINTER(u64), C.POINTER(u64)],
        "km_select_pair_stats": [vp, C.POINTER(SelectPairStats)],
        "km_select_pair_destroy": [vp],
        "km_select_labels_create": [vp, u32, C.POINTER(i32), u32, i32, vp, C.POINTER(vp)],
        "km_select_labels_add_fastq": [vp, vp, u64, i32, C.POINTER(u64)],
        "km_select_labels_stats": [vp, C.POINTER(SelectLabelsStats), C.POINTER(u64), C.POINTER(u64)],
        "km_select_labels_destroy": [vp],
        "kmjf_fastq_label_hits": [vp, u32, vp, u64, i32, vp, u64, C.POINTER(u64), vp],
        "km_device_count": [C.POINTER(i32)],
        "km_device_sync": [i32],
        "km_device_copy_GBs": [i32, u64, i32, C.POINTER(dbl)],
        "km_probe_bench": [vp, vp, u64, i32, dbl, i64, C.POINTER(dbl), C.POINTER(dbl), C.POINTER(u64)],
        "km_stream_create": [i32, C.POINTER(vp)],
        "km_stream_destroy": [vp],
    }
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = i32
    for name in ("km_strerror", "km_last_error", "km_version"):
        getattr(lib, name).restype = cp
    lib.km_strerror.argtypes = [i32]
    lib.km_report_free.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]
    lib.km_report_free.restype = None
    _lib = lib
    return lib


def pump(batches, streams, steps, stages):
    """km_batch_pump: `steps` runs over the batches in flight, round robin, deliveries awaited."""
    lib = load()
    n = len(batches)
    bs = (C.c_void_p * n)(*[b._b for b in batches])
    sts = (C.c_void_p * n)(*[C.c_void_p(s or 0) for s in streams])
    check(lib.km_batch_pump(bs, sts, n, int(steps), int(stages)))


def device_sync(device=0):
    check(load().km_device_sync(int(device)))


def device_copy_GBs(device=0, nbytes=1 << 30, reps=10):
    out = C.c_double()
    check(load().km_device_copy_GBs(int(device), int(nbytes), int(reps), C.byref(out)))
    return float(out.value)


def probe_bench(db, kmers, reps=10, ratio=0.05, n_cutoff=5):
    """(query_ms, children_ms, n_zero): k_query / k_children alone over `kmers` (numpy uint64)."""
    kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
    q, c, z = C.c_double(), C.c_double(), C.c_uint64()
    check(load().km_probe_bench(db._h, ptr(kmers), kmers.size, int(reps), float(ratio), int(n_cutoff),
                                C.byref(q), C.byref(c), C.byref(z)))
    return float(q.value), float(c.value), int(z.value)


def stream_create(device=0):
    """A non-blocking HIP stream handle (int) from the library."""
    st = C.c_void_p()
    check(load().km_stream_create(int(device), C.byref(st)))
    return st.value


def stream_destroy(stream):
    check(load().km_stream_destroy(C.c_void_p(stream)))


def check(rc):
    if rc != KM_OK:
        lib = load()
        detail = lib.km_last_error().decode() or lib.km_strerror(rc).decode()
        raise KmError(rc, detail)


def ptr(arr):
    """Raw pointer of a C-contiguous numpy array (or None)."""
    if arr is None:
        return None
    assert arr.flags["C_CONTIGUOUS"]
    return arr.ctypes.data_as(C.c_void_p)


def typed_ptr(arr, ctype):
    return None if arr is None else arr.ctypes.data_as(C.POINTER(ctype))


class Database(_Handle):
    """One k-mer count database: host records + HBM-resident table.

    Replaces the ``QueryMerFile`` handle of km/utils/Jellyfish.py:24."""
    _slot, _destroy, _live = "_h", "kmjf_close", _LIVE_DATABASES

    def __init__(self, handle):
        self._h = handle
        self._lib = load()
        self._opened()

    @classmethod
    def open(cls, path):
        lib = load()
        h = C.c_void_p()
        check(lib.kmjf_open(os.fsencode(path), C.byref(h)))
        return cls(h)

    @classmethod
    def load(cls, path, device=0):
        """Open + upload without a host copy of the records (direct file -> HBM ingestion)."""
        lib = load()
        h = C.c_void_p()
        check(lib.kmjf_load(os.fsencode(path), int(device), C.byref(h)))
        return cls(h)

    @classmethod
    def from_records(cls, keys, counts, k, canonical=True):
        lib = load()
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        assert keys.shape == counts.shape
        h = C.c_void_p()
        check(lib.kmjf_from_records(ptr(keys), ptr(counts), keys.size, int(k), int(bool(canonical)),
                                    C.byref(h)))
        return cls(h)

    @classmethod
    def empty(cls, k, canonical=True):
        lib = load()
        h = C.c_void_p()
        check(lib.kmjf_create(int(k), int(bool(canonical)), C.byref(h)))
        return cls(h)

    @property
    def info(self):
        inf = JfInfo()
        check(self._lib.kmjf_info(self._h, C.byref(inf)))
        return inf

    def records(self):
        """(keys, counts) copies of the host records."""
        kp, cp_, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        check(self._lib.kmjf_records(self._h, C.byref(kp), C.byref(cp_), C.byref(n)))
        if n.value == 0:
            return np.zeros(0, np.uint64), np.zeros(0, np.uint32)
        keys = np.ctypeslib.as_array(C.cast(kp, _P64), shape=(n.value,)).copy()
        counts = np.ctypeslib.as_array(C.cast(cp_, _P32), shape=(n.value,)).copy()
        return keys, counts

    def upload(self, device=0):
        check(self._lib.kmjf_upload(self._h, int(device)))
        return self

    def broadcast(self, devices):
        """One process, several GPUs (kmjf_broadcast): the host records go to devices[0], cross the links once as
        one RCCL broadcast and every device builds its own table.  Returns one Database per device; the first is
        this one."""
        devices = [int(d) for d in devices]
        arr = (C.c_int * len(devices))(*devices)
        out = (C.c_void_p * max(1, len(devices)))()
        check(self._lib.kmjf_broadcast(self._h, arr, len(devices), out))
        return [self] + [Database(C.c_void_p(out[i])) for i in range(1, len(devices))]

    def upload_from_device(self, device, d_keys_ptr, d_counts_ptr, n, stream=None):
        check(self._lib.kmjf_upload_from_device(self._h, int(device), C.c_void_p(d_keys_ptr),
                                                C.c_void_p(d_counts_ptr), int(n),
                                                C.c_void_p(stream or 0)))
        return self

    def query_dev(self, d_kmers_ptr, n, d_counts_ptr, stream=None):
        """Device arrays in / out, asynchronous on `stream`."""
        check(self._lib.kmjf_query_batch_dev(self._h, C.c_void_p(d_kmers_ptr), int(n),
                                             C.c_void_p(d_counts_ptr), C.c_void_p(stream or 0)))

    def children_dev(self, d_kmers_ptr, n, ratio, n_cutoff, d_mask_ptr, d_counts4_ptr, forward=True,
                     stream=None):
        check(self._lib.kmjf_children_batch_dev(self._h, C.c_void_p(d_kmers_ptr), int(n), float(ratio),
                                                int(n_cutoff), int(bool(forward)),
                                                C.c_void_p(d_mask_ptr), C.c_void_p(d_counts4_ptr),
                                                C.c_void_p(stream or 0)))

    def query(self, kmers):
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        out = np.zeros(kmers.size, dtype=np.uint32)
        check(self._lib.kmjf_query_batch(self._h, ptr(kmers), kmers.size, ptr(out)))
        return out

    def children(self, kmers, ratio, n_cutoff, forward=True):
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        mask = np.zeros(kmers.size, dtype=np.uint8)
        counts4 = np.zeros((kmers.size, 4), dtype=np.uint32)
        check(self._lib.kmjf_children_batch(self._h, ptr(kmers), kmers.size, float(ratio),
                                            int(n_cutoff), int(bool(forward)), ptr(mask),
                                            ptr(counts4)))
        return mask, counts4

    def debug_table(self):
        """kmjf_debug_table: the uploaded table as it lies in HBM -> (dir uint32[n_buckets + 1], tag uint64[n_slots],
        counts uint16[n_slots, 4]); bucket b owns the slots [2 dir[b], 2 dir[b + 1]), an empty slot has tag ~0."""
        nb, ns = C.c_uint64(), C.c_uint64()
        check(self._lib.kmjf_debug_table(self._h, None, 0, None, 0, C.byref(nb), C.byref(ns)))
        dir_ = np.zeros(nb.value + 1, np.uint32)
        slots = np.zeros(ns.value, np.dtype([("tag", np.uint64), ("c", np.uint16, (4,))]))
        check(self._lib.kmjf_debug_table(self._h, ptr(dir_), dir_.size, ptr(slots), slots.nbytes, C.byref(nb), C.byref(ns)))
        return dir_, slots["tag"].copy(), slots["c"].copy()

    def query_text(self, kmers, out_fd, stream=None):
        """kmjf_query_text: one "MER COUNT" line per k-mer (uint64, as given: canonicalised by the caller for a
        canonical database) to the descriptor out_fd, in the order given, 0 for an absent k-mer; the lookups and
        the text are made on the device -> the dict of km_dump_stats_t."""
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        st = DumpStats()
        check(self._lib.kmjf_query_text(self._h, ptr(kmers) if kmers.size else None, kmers.size, out_descriptor(out_fd),
                                        C.byref(st), C.c_void_p(stream or 0)))
        return _dump_stats_dict(st)

    def cov_seqs(self, seqs, stream=None):
        """kmjf_cov_seqs: the coverage statistics of every sequence of `seqs` (str, bytes or uint8 arrays) over its
        windows of k bases, cut and looked up on the device -> a structured array of km_cov_t (COV_DTYPE), one cell
        per sequence.  A window with a byte outside ACGTacgt is skipped and counted in n_skipped; a sequence
        without a valid window has n_kmers 0, min 0xFFFFFFFF and max 0."""
        text, off = pack_sequences(seqs)
        out = np.zeros(off.size - 1, COV_DTYPE)
        out["min"] = 0xFFFFFFFF                             # (a call without bytes touches nothing)
        check(self._lib.kmjf_cov_seqs(self._h, ptr(text) if text.size else None, ptr(off), off.size - 1,
                                      ptr(out) if out.size else None, C.c_void_p(stream or 0)))
        return out

    def scan_text(self, seqs, out_fd, stream=None):
        """kmjf_scan_text: one "MER COUNT" line per valid window of every sequence of `seqs`, in order, to the
        descriptor out_fd: what `query -s` prints; the k-mers are cut, looked up and printed on the device -> the
        dict of km_dump_stats_t (records_in: all windows, records_out: the lines)."""
        text, off = pack_sequences(seqs)
        st = DumpStats()
        check(self._lib.kmjf_scan_text(self._h, ptr(text) if text.size else None, ptr(off), off.size - 1,
                                       out_descriptor(out_fd), C.byref(st), C.c_void_p(stream or 0)))
        return _dump_stats_dict(st)

    def fastq_hits(self, text, min_qual_char=None, stream=None):
        """kmjf_fastq_hits: per record of the 4-line FASTQ text (whole records, the last line needs no newline) the
        number of windows of k bases of its sequence line whose k-mer this table holds with a count > 0; with
        min_qual_char a base whose quality byte is below it is no base -> np.uint32[n_records].  Cut, masked and looked
        up on the device; a malformed record raises KmError (KM_E_FORMAT)."""
        buf = _byte_view(text)
        hits = np.zeros(buf.size // 6 + 1, np.uint32)          # the smallest record has six bytes
        n = C.c_uint64()
        check(self._lib.kmjf_fastq_hits(self._h, ptr(buf) if buf.size else None, buf.size,
                                        _qual_byte(min_qual_char or 0), ptr(hits), hits.size, C.byref(n),
                                        C.c_void_p(stream or 0)))
        return hits[:n.value].copy()

    def fastq_label_hits(self, n_labels, text, min_qual_char=None, stream=None):
        """kmjf_fastq_label_hits: this table's counts read as label masks (bit l = label l, l < n_labels <= 32); per
        label and record of the 4-line FASTQ text the number of windows of k bases whose k-mer's mask has the label's
        bit -> np.uint32[n_labels, n_records].  Otherwise as fastq_hits."""
        buf = _byte_view(text)
        cap = buf.size // 6 + 1
        hits = np.zeros((max(int(n_labels), 1), cap), np.uint32)
        n = C.c_uint64()
        check(self._lib.kmjf_fastq_label_hits(self._h, int(n_labels), ptr(buf) if buf.size else None, buf.size,
                                              _qual_byte(min_qual_char or 0), ptr(hits), cap, C.byref(n),
                                              C.c_void_p(stream or 0)))
        return hits[:, :n.value].copy()


def _byte_view(data):
    """A C-contiguous uint8 view of a bytes-like object (no copy for bytes, bytearray, memoryview, numpy)."""
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    return np.frombuffer(data, dtype=np.uint8)


def strip_text(text, final=True, state=None):
    """km_text_strip: the FASTA / FASTQ stripper of Counter.add_text alone, on the host (no GPU).
    -> (stream bytes, consumed, state); pass `state` back in with the next block of the same stream."""
    st = TextState() if state is None else state
    buf = _byte_view(text)
    out = np.empty(buf.size + 1, np.uint8)
    n_out, consumed = C.c_uint64(), C.c_uint64()
    check(load().km_text_strip(C.byref(st), ptr(buf) if buf.size else None, buf.size, int(bool(final)), ptr(out),
                               out.size, C.byref(n_out), C.byref(consumed)))
    return out[:n_out.value].tobytes(), int(consumed.value), st


def fastq_cut(data):
    """km_fastq_cut: the largest offset at which a record of the 4-line FASTQ text `data` ends (0: no complete
    record).  Host only."""
    buf = _byte_view(data)
    cut = C.c_uint64()
    check(load().km_fastq_cut(ptr(buf) if buf.size else None, buf.size, C.byref(cut)))
    return int(cut.value)


def sketch_words(expected_distinct):
    """km_sketch_words: the size, in 64-bit words, of Counter.set_sketch's sketch for that many expected distinct
    k-mers: the smallest power of two >= max(64, ceil(n / 2)).  Host only."""
    words = C.c_uint64()
    check(load().km_sketch_words(int(expected_distinct), C.byref(words)))
    return int(words.value)


def sketch_slot(key, words):
    """km_sketch_slot: (word index, 32-bit mask of one to three bits) of `key` in a sketch of `words` words
    (include/kmgpu.h has the rule).  Host only."""
    word, mask = C.c_uint64(), C.c_uint32()
    check(load().km_sketch_slot(int(key), int(words), C.byref(word), C.byref(mask)))
    return int(word.value), int(mask.value)


def _qual_byte(min_qual_char):
    """0..255 from an int, or from a str / bytes of one character."""
    if isinstance(min_qual_char, str):
        min_qual_char = min_qual_char.encode("latin-1")
    if isinstance(min_qual_char, (bytes, bytearray)):
        if len(min_qual_char) != 1:
            raise ValueError("min_qual_char must be one character")
        return min_qual_char[0]
    return int(min_qual_char)


class Counter(_Handle):
    """k-mers counted from reads on the GPU (km_counter_*, include/kmgpu.h): what `jellyfish count -m k [-C]
    -s expected_distinct` does.  add_bases / add_text / add_fastq feed it, finish() hands back a Database whose table was
    built on the device from the counted records."""
    _slot, _destroy, _live = "_c", "km_counter_destroy", _LIVE_COUNTERS

    def __init__(self, k=31, canonical=True, device=0, expected_distinct=0):
        self._lib = load()
        self._c = C.c_void_p()
        self.k, self.canonical, self.device = int(k), bool(canonical), int(device)
        check(self._lib.km_counter_create(self.device, self.k, int(self.canonical), int(expected_distinct),
                                          C.byref(self._c)))
        self._opened()

    def add_bases(self, data):
        """Bases (ACGTacgt) and breaks (any other byte); k-mers never span two calls."""
        buf = _byte_view(data)
        check(self._lib.km_counter_add_bases(self._c, ptr(buf) if buf.size else None, buf.size))

    def add_text(self, data, final=False):
        """FASTA or 4-line FASTQ text; returns how many bytes were taken (whole lines): pass the rest again in
        front of the next block."""
        buf = _byte_view(data)
        consumed = C.c_uint64()
        check(self._lib.km_counter_add_text(self._c, ptr(buf) if buf.size else None, buf.size, int(bool(final)),
                                            C.byref(consumed)))
        return int(consumed.value)

    def add_fastq(self, data, final=False, min_qual_char=0):
        """4-line FASTQ text, parsed on the GPU; a base whose quality byte is below min_qual_char (an int, or one
        character; 0 masks nothing) is read as N, as by `jellyfish count -Q`.  Returns how many bytes were taken
        (whole records): pass the rest again in front of the next block.  A malformed record raises KmError
        (KM_E_FORMAT) from a LATER call that waits for the device: stats(), finish()."""
        buf = _byte_view(data)
        consumed = C.c_uint64()
        check(self._lib.km_counter_add_fastq(self._c, ptr(buf) if buf.size else None, buf.size, int(bool(final)),
                                             _qual_byte(min_qual_char), C.byref(consumed)))
        return int(consumed.value)

    def fastq_kernel_ms(self):
        """km_counter_fastq_kernel_ms: time of add_fastq's own kernels so far (needs KM_COUNT_TIME_FASTQ=1)."""
        ms = C.c_float()
        check(self._lib.km_counter_fastq_kernel_ms(self._c, C.byref(ms)))
        return float(ms.value)

    def add_records(self, keys, counts, mode="sum"):
        """km_counter_add_records: (key, count) pairs into the table, per key summed (saturating at 2^32 - 1) or
        the maximum kept (mode "sum" / "max"); pairs with count 0 are skipped, keys may repeat."""
        keys, counts = _records(keys, counts)
        check(self._lib.km_counter_add_records(self._c, ptr(keys) if keys.size else None,
                                               ptr(counts) if counts.size else None, keys.size, _merge_mode(mode)))

    def add_jf(self, path, mode="sum"):
        """km_counter_add_jf: the records of a `binary/sorted` file of the counter's k and canonical into the
        table, combined as by add_records; returns the number of records in the file."""
        n = C.c_uint64()
        check(self._lib.km_counter_add_jf(self._c, os.fsencode(path), _merge_mode(mode), C.byref(n)))
        return int(n.value)

    def set_records(self, keys, counts, op="intersect"):
        """km_counter_set_records: (key, count) pairs as ONE input of a set operation over the counter's inputs.
        "intersect": the keys with count > 0 in every input, with the minimum over all their records; "subtract": the
        records of the first input whose key is, with count > 0, in no later one.  Pairs with count 0 are absent, keys
        may repeat (one input all the same), an empty call is an empty input.  This project's own definitions."""
        keys, counts = _records(keys, counts)
        check(self._lib.km_counter_set_records(self._c, ptr(keys) if keys.size else None,
                                               ptr(counts) if counts.size else None, keys.size, _set_op(op)))

    def set_jf(self, path, op="intersect"):
        """km_counter_set_jf: the records of a `binary/sorted` file of the counter's k and canonical as one input of
        the set operation, as by set_records; returns the number of records in the file."""
        n = C.c_uint64()
        check(self._lib.km_counter_set_jf(self._c, os.fsencode(path), _set_op(op), C.byref(n)))
        return int(n.value)

    def mark_records(self, keys, counts, lower_count=1, upper_count=0xFFFFFFFF):
        """km_counter_mark_records: (key, count) pairs as the NEXT input of a comparison (at most 32).  The input is the
        set of the keys of its pairs with lower_count <= count <= upper_count; pairs with count 0 are absent, keys may
        repeat (a key is in the set if any of its pairs passes the cut), an empty call is an empty input.  This
        project's own definitions (include/kmgpu.h)."""
        keys, counts = _records(keys, counts)
        check(self._lib.km_counter_mark_records(self._c, ptr(keys) if keys.size else None,
                                                ptr(counts) if counts.size else None, keys.size, int(lower_count),
                                                int(upper_count)))

    def mark_jf(self, path, lower_count=1, upper_count=0xFFFFFFFF):
        """km_counter_mark_jf: the records of a `binary/sorted` file of the counter's k and canonical as the next
        input of the comparison, as by mark_records; returns the number of records in the file."""
        n = C.c_uint64()
        check(self._lib.km_counter_mark_jf(self._c, os.fsencode(path), int(lower_count), int(upper_count), C.byref(n)))
        return int(n.value)

    def cooccurrence(self):
        """km_counter_cooccurrence (waits for everything marked so far; the counter is left as it was): dict(n_inputs,
        union, shared = uint64[n, n] with |S_i & S_j|, in_exactly = uint64[n + 1] indexed by m (entry 0 is 0), private =
        uint64[n], kernel_ms = the time of the passes over the table so far, needs KM_COUNT_TIME_MERGE=1 when the
        counter is made)."""
        r = Cooc()
        check(self._lib.km_counter_cooccurrence(self._c, C.byref(r)))
        n = int(r.n_inputs)
        shared = np.ctypeslib.as_array(r.shared).reshape(32, 32)[:n, :n].copy()
        return {"n_inputs": n, "union": int(r.n_union), "shared": shared,
                "in_exactly": np.ctypeslib.as_array(r.in_exactly)[:n + 1].copy(),
                "private": np.ctypeslib.as_array(r.private_to)[:n].copy(), "kernel_ms": float(r.kernel_ms)}

    def set_filter(self, keys):
        """km_counter_set_filter: from now on only the k-mers of `keys` (uint64, the counter's key encoding; a
        canonical counter canonicalises them on the device; repeats allowed, empty allowed) are counted, and each of
        them is in the table from the start with count 0.  Once, and before anything has been fed.  This project's
        reading of `jellyfish count --if`."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
        check(self._lib.km_counter_set_filter(self._c, ptr(keys) if keys.size else None, keys.size))

    def filter_stats(self):
        """km_counter_filter_stats (waits for everything added so far): dict(n_keys = distinct filter keys, kmers_hit
        = windows counted, tier = "none" / "lds" / "hbm", lds_keys = the most distinct keys the LDS tier takes,
        kernel_ms = the time of the counting kernels, needs KM_COUNT_TIME_FILTER=1 when the counter is made)."""
        n, hit, tier, cap, ms = C.c_uint64(), C.c_uint64(), C.c_int(), C.c_uint64(), C.c_float()
        check(self._lib.km_counter_filter_stats(self._c, C.byref(n), C.byref(hit), C.byref(tier), C.byref(cap),
                                                C.byref(ms)))
        return {"n_keys": int(n.value), "kmers_hit": int(hit.value), "tier": FILTER_TIERS[tier.value],
                "lds_keys": int(cap.value), "kernel_ms": float(ms.value)}

    def set_sketch(self, words):
        """km_counter_set_sketch: the counter is fed twice from now on.  What is fed until sketch_done() is only noted
        in a two-plane Bloom sketch of `words` 64-bit words (a power of two, 64 .. 2^40; sketch_words(n) sizes it for n
        expected distinct k-mers); what is fed afterwards is counted only if the sketch saw its k-mer at least twice in
        the first pass, or falsely says so.  With both passes over the same reads, finish(2) gives exactly the records
        of a plain counter while the table holds the admitted k-mers alone.  Once, before anything has been fed, and
        not beside a filter.  This project's own semantics (what `jellyfish bc` + `count --bc` are for)."""
        check(self._lib.km_counter_set_sketch(self._c, int(words)))

    def sketch_done(self):
        """km_counter_sketch_done: ends the first pass (waits for it; a malformed FASTQ record of that pass raises
        here at the latest).  The next add_* call starts a fresh stream."""
        check(self._lib.km_counter_sketch_done(self._c))

    def sketch_stats(self):
        """km_counter_sketch_stats (waits for everything added so far): dict(words, bits_1 / bits_2 = set bits of the
        planes "seen" / "seen again", kmers_noted = windows of the first pass, kmers_admitted = windows the second pass
        counted, note_ms / count_ms = the time of the kernels of either pass, needs KM_COUNT_TIME_FILTER=1 when the
        counter is made)."""
        w, b1, b2, noted, adm = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        ms = (C.c_float * 2)()
        check(self._lib.km_counter_sketch_stats(self._c, C.byref(w), C.byref(b1), C.byref(b2), C.byref(noted),
                                                C.byref(adm), ms))
        return {"words": int(w.value), "bits_1": int(b1.value), "bits_2": int(b2.value),
                "kmers_noted": int(noted.value), "kmers_admitted": int(adm.value), "note_ms": float(ms[0]),
                "count_ms": float(ms[1])}

    def merge_stats(self):
        """km_counter_merge_stats (waits for everything added so far): dict(records_in = records with count > 0
        taken by add_records / add_jf / set_records / set_jf, kernel_ms = the time of their kernels, needs
        KM_COUNT_TIME_MERGE=1)."""
        n, ms = C.c_uint64(), C.c_float()
        check(self._lib.km_counter_merge_stats(self._c, C.byref(n), C.byref(ms)))
        return {"records_in": int(n.value), "kernel_ms": float(ms.value)}

    def stats(self):
        """dict of km_counter_stats_t (waits for everything added so far)."""
        s = CounterStats()
        check(self._lib.km_counter_stats(self._c, C.byref(s)))
        return {"bases": int(s.bases), "kmers": int(s.kmers), "distinct": int(s.distinct), "slots": int(s.slots),
                "n_grow": int(s.n_grow)}

    def finish(self, lower_count=1, upper_count=0xFFFFFFFF):
        """Keep the k-mers with lower_count <= count <= upper_count (of a set operation: those that survived it) and
        build the lookup table from them -> Database.  Without an upper cut this is km_counter_finish, with one
        km_counter_finish_range."""
        h = C.c_void_p()
        if int(upper_count) == 0xFFFFFFFF:
            check(self._lib.km_counter_finish(self._c, int(lower_count), C.byref(h)))
        else:
            check(self._lib.km_counter_finish_range(self._c, int(lower_count), int(upper_count), C.byref(h)))
        return Database(h)

    def n_records(self):
        """How many records the finished counter kept."""
        n = C.c_uint64()
        check(self._lib.km_counter_records(self._c, None, None, 0, C.byref(n)))
        return int(n.value)

    def records(self):
        """(keys, counts) of the finished counter, as compacted on the device: in no particular order."""
        n = C.c_uint64()
        check(self._lib.km_counter_records(self._c, None, None, 0, C.byref(n)))
        keys = np.zeros(n.value, np.uint64)
        counts = np.zeros(n.value, np.uint32)
        if n.value:
            check(self._lib.km_counter_records(self._c, ptr(keys), ptr(counts), n.value, C.byref(n)))
        return keys, counts

    def write_jf(self, path, cmdline=None, seed=0):
        """km_counter_write_jf: the finished counter's records as a file in Jellyfish's own record order, sorted
        on the device and written natively (the records are not copied to the host as arrays)."""
        check(self._lib.km_counter_write_jf(self._c, os.fsencode(path), _cmdline_json(cmdline), int(seed)))


    def histo(self, low=1, high=10000, increment=1, lower_count=1, upper_count=0xFFFFFFFF):
        """km_counter_histo: the histogram of the counts and the four statistics, before finish() (everything added
        so far; the counter is left as it was) or after it (the kept records) -> (base, bins uint64[n_bins], stats
        dict).  A key takes part iff max(lower_count, 1) <= count <= upper_count; bin i is labelled
        base + i * increment (include/kmgpu.h has the rule: this project's reading of `jellyfish histo`)."""
        base, n_bins = histo_layout(low, high, increment)
        bins = np.zeros(n_bins, np.uint64)
        st = HistoStats()
        check(self._lib.km_counter_histo(self._c, int(low), int(high), int(increment), int(lower_count),
                                         int(upper_count), ptr(bins), bins.size, C.byref(st)))
        return base, bins, _histo_stats_dict(st)

    def dump(self, out, fmt="fasta", lower_count=0, upper_count=0xFFFFFFFF):
        """km_counter_dump: the finished counter's records with lower_count <= count <= upper_count as text to `out`
        (a descriptor, or a file object, which is flushed first), in the order of records(), formatted on the device
        -> the dict of km_dump_stats_t."""
        st = DumpStats()
        check(self._lib.km_counter_dump(self._c, out_descriptor(out), _dump_format(fmt), int(lower_count), int(upper_count),
                                        C.byref(st)))
        return _dump_stats_dict(st)


def _histo_stats_dict(st):
    return {"unique": int(st.unique), "distinct": int(st.distinct), "total": int(st.total),
            "max_count": int(st.max_count)}


def histo_layout(low=1, high=10000, increment=1):
    """km_histo_layout -> (base, n_bins) of `histo -l low -h high -i increment` (host only)."""
    base, n = C.c_uint64(), C.c_uint64()
    check(load().km_histo_layout(int(low), int(high), int(increment), C.byref(base), C.byref(n)))
    return int(base.value), int(n.value)


def jf_histo(path, low=1, high=10000, increment=1, lower_count=1, upper_count=0xFFFFFFFF, device=0, stream=None):
    """km_jf_histo: the same for the records of a `binary/sorted` file, streamed through the GPU piece by piece
    -> (base, bins, stats dict with k and n_records of the header added)."""
    base, n_bins = histo_layout(low, high, increment)
    bins = np.zeros(n_bins, np.uint64)
    st, k, n = HistoStats(), C.c_int32(), C.c_uint64()
    check(load().km_jf_histo(int(device), os.fsencode(path), int(low), int(high), int(increment), int(lower_count),
                             int(upper_count), ptr(bins), bins.size, C.byref(st), C.byref(k), C.byref(n),
                             C.c_void_p(stream or 0)))
    stats = _histo_stats_dict(st)
    stats.update(k=int(k.value), n_records=int(n.value))
    return base, bins, stats


def histo_kernel_ms():
    """km_histo_kernel_ms: the time of the histogram kernels of this thread's last Counter.histo / jf_histo."""
    ms = C.c_float()
    check(load().km_histo_kernel_ms(C.byref(ms)))
    return float(ms.value)


def histo_text(base, increment, bins, full=False):
    """km_histo_text: "<label> <n>\\n" per bin with n > 0 (per bin with full), as str."""
    lib = load()
    bins = np.ascontiguousarray(bins, dtype=np.uint64)
    ln = C.c_uint64()
    args = (int(base), int(increment), ptr(bins) if bins.size else None, bins.size, int(bool(full)))
    check(lib.km_histo_text(*args, None, 0, C.byref(ln)))
    out = np.zeros(max(ln.value, 1), np.uint8)
    check(lib.km_histo_text(*args, ptr(out), out.size, C.byref(ln)))
    return out[:ln.value].tobytes().decode("ascii")


def histo_stats_text(stats):
    """km_histo_stats_text: the four lines of `jellyfish stats` for a stats dict of Counter.histo / jf_histo."""
    lib = load()
    st = HistoStats(int(stats["unique"]), int(stats["distinct"]), int(stats["total"]), int(stats["max_count"]))
    ln = C.c_uint64()
    check(lib.km_histo_stats_text(C.byref(st), None, 0, C.byref(ln)))
    out = np.zeros(max(ln.value, 1), np.uint8)
    check(lib.km_histo_stats_text(C.byref(st), ptr(out), out.size, C.byref(ln)))
    return out[:ln.value].tobytes().decode("ascii")


DUMP_FORMATS = {"fasta": 0, "column": 1, "tab": 2}         # KM_DUMP_FASTA, KM_DUMP_COLUMN, KM_DUMP_TAB


def _dump_format(fmt):
    """The library's code of "fasta" / "column" / "tab"; anything else goes through as an int for it to refuse."""
    return DUMP_FORMATS[fmt] if fmt in DUMP_FORMATS else int(fmt)


def out_descriptor(out):
    """The descriptor the library writes to: `out` itself, or that of a file object, flushed before it is handed over
    so that what Python buffered comes first."""
    if isinstance(out, int):
        return out
    out.flush()
    return out.fileno()


def _dump_stats_dict(st):
    return {"records_in": int(st.records_in), "records_out": int(st.records_out), "bytes_out": int(st.bytes_out),
            "pieces": int(st.pieces)}


def dump_text(keys, counts, k, fmt="fasta", lower_count=0, upper_count=0xFFFFFFFF, device=0):
    """km_dump_text: the records (keys, counts) with lower_count <= count <= upper_count as the text of `dump`, in
    the order given -> bytes.  fmt "fasta" is ">COUNT\nMER\n", "column" "MER COUNT\n", "tab" "MER\tCOUNT\n"
    (include/kmgpu.h has the rule: this project's reading of `jellyfish dump`)."""
    keys, counts = _records(keys, counts)
    out = np.empty(max(keys.size * (max(int(k), 0) + 13), 1), np.uint8)          # the longest line is k + 13 bytes
    ln = C.c_uint64()
    check(load().km_dump_text(int(device), ptr(keys) if keys.size else None, ptr(counts) if counts.size else None,
                              keys.size, int(k), _dump_format(fmt), int(lower_count), int(upper_count), ptr(out),
                              out.size, C.byref(ln), None))
    return out[:ln.value].tobytes()


def jf_dump(path, out_fd, fmt="fasta", lower_count=0, upper_count=0xFFFFFFFF, device=0, stream=None):
    """km_jf_dump: the records of a `binary/sorted` file as text to the descriptor out_fd, in file order, streamed
    through the GPU piece by piece -> the dict of km_dump_stats_t."""
    st = DumpStats()
    check(load().km_jf_dump(int(device), os.fsencode(path), out_descriptor(out_fd), _dump_format(fmt), int(lower_count),
                            int(upper_count), C.byref(st), C.c_void_p(stream or 0)))
    return _dump_stats_dict(st)


def dump_kernel_ms():
    """km_dump_kernel_ms: the time of the text kernels of this thread's last dump_text / jf_dump / Counter.dump /
    Database.query_text."""
    ms = C.c_float()
    check(load().km_dump_kernel_ms(C.byref(ms)))
    return float(ms.value)


def scan_kernel_ms():
    """km_scan_kernel_ms: the time of the scan kernels (extraction + lookup) of this thread's last Database.cov_seqs /
    Database.scan_text."""
    ms = C.c_float()
    check(load().km_scan_kernel_ms(C.byref(ms)))
    return float(ms.value)


class Selector(_Handle):
    """The FASTQ reads that hit a table, extracted on the GPU (km_select_*, include/kmgpu.h): a read is kept iff
    (its windows of k bases with a count > 0 in `db` number at least min_hits) != invert, and the kept records go to
    `out` (a descriptor, or a file object with fileno()) byte for byte, in input order.  `db` must stay open for as long
    as the selector lives.  A context manager; close() releases the device side."""
    _slot, _destroy, _live = "_s", "km_select_destroy", _LIVE_COUNTERS

    def __init__(self, db, out, min_hits=1, invert=False, min_qual_char=None, stream=None):
        self._lib = load()
        self._s = C.c_void_p()
        self._db = db
        check(self._lib.km_select_create(db._h, int(min_hits), int(bool(invert)), _qual_byte(min_qual_char or 0),
                                         out_descriptor(out), C.c_void_p(stream or 0), C.byref(self._s)))
        self._opened()

    def add_fastq(self, data, final=False):
        """4-line FASTQ text; returns how many bytes were taken (whole records): pass the rest again in front of the
        next block.  What the call kept is on the descriptor when it returns.  A malformed record raises KmError
        (KM_E_FORMAT) from this call; the pieces before it are written."""
        buf = _byte_view(data)
        consumed = C.c_uint64()
        check(self._lib.km_select_add_fastq(self._s, ptr(buf) if buf.size else None, buf.size, int(bool(final)),
                                            C.byref(consumed)))
        return int(consumed.value)

    def stats(self):
        st = SelectStats()
        check(self._lib.km_select_stats(self._s, C.byref(st)))
        return {name: int(getattr(st, name)) for name in ("records_in", "records_out", "bytes_in", "bytes_out", "pieces")}


def select_kernel_ms():
    """km_select_kernel_ms (needs KM_SELECT_TIME=1 when the selector is made, else zeros): the kernel time of the
    Selector, or the Database.fastq_hits call, that last finished a piece on this thread -> {"front": line table and
    mask, "hits": clear and hits, "sizes": sizes and scan, "gather": the gather alone}, ms."""
    ms = (C.c_float * 4)()
    check(load().km_select_kernel_ms(ms))
    return {"front": float(ms[0]), "hits": float(ms[1]), "sizes": float(ms[2]), "gather": float(ms[3])}


class LabelSelector(_Handle):
    """The FASTQ reads sorted into one output per label on the GPU (km_select_labels_*, include/kmgpu.h): the counts of
    `db` are label masks (count.label_table), read r goes to outs[l] iff its windows of k bases whose k-mer's mask has
    bit l number at least min_hits, byte for byte and in input order; a read kept by several labels is in each of their
    outputs.  `outs`: one descriptor, or file object with fileno(), per label, at most 32.  `db` must stay open for as
    long as the selector lives.  A context manager; close() releases the device side."""
    _slot, _destroy, _live = "_s", "km_select_labels_destroy", _LIVE_COUNTERS

    def __init__(self, db, outs, min_hits=1, min_qual_char=None, stream=None):
        self._lib = load()
        self._s = C.c_void_p()
        self._db = db
        fds = [out_descriptor(o) for o in outs]
        self.n_labels = len(fds)
        arr = (C.c_int32 * max(len(fds), 1))(*fds)
        check(self._lib.km_select_labels_create(db._h, len(fds), arr, int(min_hits), _qual_byte(min_qual_char or 0),
                                                C.c_void_p(stream or 0), C.byref(self._s)))
        self._opened()

    def add_fastq(self, data, final=False):
        """As Selector.add_fastq: returns how many bytes were taken (whole records); what the call kept is on the
        descriptors when it returns."""
        buf = _byte_view(data)
        consumed = C.c_uint64()
        check(self._lib.km_select_labels_add_fastq(self._s, ptr(buf) if buf.size else None, buf.size, int(bool(final)),
                                                   C.byref(consumed)))
        return int(consumed.value)

    def stats(self):
        """km_select_labels_stats_t as a dict, with records_out and bytes_out as lists, one entry per label."""
        st = SelectLabelsStats()
        rec, byt = (C.c_uint64 * self.n_labels)(), (C.c_uint64 * self.n_labels)()
        check(self._lib.km_select_labels_stats(self._s, C.byref(st), rec, byt))
        out = {name: int(getattr(st, name)) for name, _ in SelectLabelsStats._fields_}
        out["records_out"] = [int(v) for v in rec]
        out["bytes_out"] = [int(v) for v in byt]
        return out


PAIR_RULES = {"any": 0, "both": 1, "sum": 2}     # KM_PAIR_ANY, KM_PAIR_BOTH, KM_PAIR_SUM


class PairSelector(_Handle):
    """The mates of a paired-end run that hit a table, kept together on the GPU (km_select_pair_*, include/kmgpu.h):
    record r of `data1` and record r of `data2` are pair r, kept iff (score >= min_hits) != invert with score =
    max(h1, h2) for rule "any", min(h1, h2) for "both" and h1 + h2 for "sum"; mate 1's kept records go to `out1` and
    mate 2's to `out2` (descriptors, or file objects with fileno()) byte for byte and in input order.  With check_names
    the mates' names (without a "/1" or "/2" at the end) must agree.  `db` must stay open for as long as the selector
    lives.  A context manager; close() releases the device side."""
    _slot, _destroy, _live = "_s", "km_select_pair_destroy", _LIVE_COUNTERS

    def __init__(self, db, out1, out2, min_hits=1, invert=False, min_qual_char=None, rule="any", check_names=True,
                 stream=None):
        self._lib = load()
        self._s = C.c_void_p()
        self._db = db
        if isinstance(rule, str) and rule not in PAIR_RULES:
            raise KmError(4, "pair rule %r is none of 'any', 'both', 'sum'" % (rule,))       # KM_E_ARG
        code = PAIR_RULES[rule] if isinstance(rule, str) else int(rule)
        check(self._lib.km_select_pair_create(db._h, int(min_hits), int(bool(invert)), _qual_byte(min_qual_char or 0),
                                              code, int(bool(check_names)), out_descriptor(out1), out_descriptor(out2),
                                              C.c_void_p(stream or 0), C.byref(self._s)))
        self._opened()

    def add_fastq(self, data1, data2, final=False):
        """4-line FASTQ text of mate 1 and of mate 2; returns (used1, used2), how many bytes of either were taken (whole
        records that found their partner): pass the rest of each again in front of its next block.  What the call kept
        is on the descriptors when it returns.  A malformed record, mates whose names differ and, at the final call,
        streams of unequal record counts raise KmError (KM_E_FORMAT); the pieces before it are written."""
        buf1, buf2 = _byte_view(data1), _byte_view(data2)
        used1, used2 = C.c_uint64(), C.c_uint64()
        check(self._lib.km_select_pair_add_fastq(self._s, ptr(buf1) if buf1.size else None, buf1.size,
                                                 ptr(buf2) if buf2.size else None, buf2.size, int(bool(final)),
                                                 C.byref(used1), C.byref(used2)))
        return int(used1.value), int(used2.value)

    def stats(self):
        st = SelectPairStats()
        check(self._lib.km_select_pair_stats(self._s, C.byref(st)))
        out = {"pairs_in": int(st.pairs_in), "pairs_out": int(st.pairs_out), "pieces": int(st.pieces)}
        for name in ("bytes_in", "bytes_out", "resent_bytes"):
            out[name] = [int(v) for v in getattr(st, name)]
        return out


MERGE_MODES = {"sum": 0, "max": 1}         # KM_MERGE_SUM, KM_MERGE_MAX


def _merge_mode(mode):
    """The library's code of "sum" / "max"; anything else goes through as an int for the library to refuse."""
    return MERGE_MODES[mode] if mode in MERGE_MODES else int(mode)


SET_OPS = {"intersect": 0, "subtract": 1}   # KM_SET_INTERSECT, KM_SET_SUBTRACT
FILTER_TIERS = ("none", "lds", "hbm")       # km_counter_filter_stats' tier


def _set_op(op):
    """The library's code of "intersect" / "subtract"; anything else goes through as an int for it to refuse."""
    return SET_OPS[op] if op in SET_OPS else int(op)


def jf_file_info(path):
    """km_jf_file_info: dict(k, canonical, n_records, key_bytes, counter_len) from the header and the size of a
    `binary/sorted` file (host only: no record is read)."""
    k, canonical, kb, cb, n = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_uint64()
    check(load().km_jf_file_info(os.fsencode(path), C.byref(k), C.byref(canonical), C.byref(n), C.byref(kb),
                                 C.byref(cb)))
    return {"k": int(k.value), "canonical": bool(canonical.value), "n_records": int(n.value),
            "key_bytes": int(kb.value), "counter_len": int(cb.value)}


def _cmdline_json(cmdline):
    return None if cmdline is None else json.dumps([str(a) for a in cmdline], separators=(",", ":")).encode("ascii")


def jf_matrix(k, size_log2, seed=0):
    """km_jf_matrix: the 2k column words of a deterministic full-rank matrix with size_log2 rows (host only)."""
    columns = np.zeros(64, np.uint64)                 # (room whatever k is: a bad k is the library's to refuse)
    check(load().km_jf_matrix(int(k), int(size_log2), int(seed), ptr(columns)))
    return columns[:2 * int(k)].copy()


def jf_header(k, canonical, n, cmdline=None, seed=0):
    """km_jf_header -> (header bytes, columns, size_log2) of a file of n records in Jellyfish's order."""
    lib = load()
    columns = np.zeros(64, np.uint64)
    ln, s = C.c_uint64(), C.c_int()
    args = (int(k), int(bool(canonical)), int(n), int(seed), _cmdline_json(cmdline))
    check(lib.km_jf_header(*args, None, 0, C.byref(ln), ptr(columns), C.byref(s)))
    out = np.zeros(ln.value, np.uint8)
    check(lib.km_jf_header(*args, ptr(out), out.size, C.byref(ln), ptr(columns), C.byref(s)))
    return out.tobytes(), columns[:2 * int(k)].copy(), int(s.value)


def jf_sort_records(columns, k, size_log2, keys, counts, device=0, want_pos=False):
    """km_jf_sort_records: the file records (uint8[n, ceil(2k/8) + 4]) of (keys, counts) in (pos, key) order under
    the matrix `columns` (2k words, r = size_log2 rows), sorted on the GPU; with want_pos also their positions."""
    columns = np.ascontiguousarray(columns, dtype=np.uint64)
    keys, counts = _records(keys, counts)
    if 2 <= int(k) <= 32 and columns.size != 2 * int(k):
        raise ValueError("%d columns for k=%d" % (columns.size, k))
    rec = (2 * int(k) + 7) // 8 + 4
    out = np.zeros((keys.size, rec), np.uint8)
    pos = np.zeros(keys.size, np.uint64) if want_pos else None
    check(load().km_jf_sort_records(int(device), ptr(columns), int(k), int(size_log2), ptr(keys), ptr(counts),
                                    keys.size, ptr(out), ptr(pos), None))
    return (out, pos) if want_pos else out


def jf_sort_stats():
    """km_jf_sort_stats of this thread's last sort: dict(buckets, largest, oversized, kernel_ms)."""
    v = np.zeros(4, np.uint64)
    ms = C.c_float()
    check(load().km_jf_sort_stats(ptr(v)))
    check(load().km_jf_sort_kernel_ms(C.byref(ms)))
    return {"buckets": int(v[0]), "largest": int(v[1]), "oversized": int(v[2]), "kernel_ms": float(ms.value)}


class Batch(_Handle):
    """Device workspace that walks + path-searches many targets per launch."""
    _slot, _destroy, _live = "_b", "km_batch_destroy", _LIVE_BATCHES

    def __init__(self, db, ratio=0.05, count=5, max_stack=500, max_break=10, max_node=10000,
                 max_targets=1024, max_total_bases=1 << 20):
        self._lib = load()
        self.db = db
        self.params = Params(float(ratio), int(count), int(max_stack), int(max_break),
                             int(max_node), 0)
        self._b = C.c_void_p()
        check(self._lib.km_batch_create(db._h, C.byref(self.params), int(max_targets),
                                        int(max_total_bases), C.byref(self._b)))
        self.n_targets = 0
        self._opened()

    def set_targets(self, seqs):
        """seqs: list of str/bytes (ACGT)."""
        blob, offs = pack_sequences(seqs)
        self.set_targets_packed(blob, offs)

    def set_targets_packed(self, blob, offsets):
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        check(self._lib.km_batch_set_targets(self._b, ptr(blob), ptr(offsets), offsets.size - 1))
        self.n_targets = offsets.size - 1

    def set_targets_dev(self, d_bases_ptr, offsets, stream=None):
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        check(self._lib.km_batch_set_targets_dev(self._b, C.c_void_p(d_bases_ptr), ptr(offsets),
                                                 offsets.size - 1, C.c_void_p(stream or 0)))
        self.n_targets = offsets.size - 1

    def run(self, stages=KM_STAGE_WALK | KM_STAGE_GRAPH, stream=None):
        check(self._lib.km_batch_run(self._b, int(stages), C.c_void_p(stream or 0)))

    def sync(self):
        check(self._lib.km_batch_sync(self._b))

    def timings(self):
        """km_batch_timings: (walk, graph, walk + graph, k_seed, k_pack, k_dfs, delivery kernels, copy) in ms.  Without
        KM_RUN_SERIAL k_dfs and k_graph_pure are one launch: walk and k_dfs contain the pure-chain pass, graph does not."""
        ms = (C.c_float * 8)()
        check(self._lib.km_batch_timings(self._b, ms))
        return tuple(float(x) for x in ms)

    def graph_log(self, n_targets):
        """What the reference logs with -v from inside the walk and the graph (km_batch_graph_log): per target the
        reference edges stripped and the edges kept, and per target the node indices at which the walk broke a
        loop, in walk order.  -> (removed uint32[n], nonref uint32[n], {target: [node index, ...]}, n_loop_breaks)."""
        n = int(n_targets)
        removed = np.zeros(max(1, n), dtype=np.uint32)
        nonref = np.zeros(max(1, n), dtype=np.uint32)
        cap = 4096
        pairs = np.zeros(2 * cap, dtype=np.uint32)
        n_loops = C.c_uint32(0)
        check(self._lib.km_batch_graph_log(self._b, ptr(removed), ptr(nonref), C.byref(n_loops), ptr(pairs), cap))
        loops = {}
        for t, node in pairs[:2 * min(cap, n_loops.value)].reshape(-1, 2).tolist():
            if node == 0xFFFFFFFF:               # the large tier starts this target's walk over
                loops.pop(t, None)
            else:
                loops.setdefault(t, []).append(node)
        n_real = sum(len(v) for v in loops.values())
        return removed[:n], nonref[:n], loops, n_real

    def debug_counts(self):
        """(flagged targets, unflagged ones handed to k_graph, flagged ones the epilogue of k_dfs left to k_graph)."""
        out = (C.c_uint32 * 4)()
        check(self._lib.km_batch_debug_counts(self._b, out))
        return int(out[0]), int(out[1]), int(out[2])

    def paired_steps(self):
        """How often, since the batch was made, its k_seed has run in another batch's walk launch (km_batch_pump)."""
        out = (C.c_uint32 * 4)()
        check(self._lib.km_batch_debug_counts(self._b, out))
        return int(out[3])

    def debug_stamps(self):
        """k_seed time stamps (KM_SEED_STAMPS diagnostics): uint64 array [n_waves, 16]."""
        n = C.c_uint64(0)
        check(self._lib.km_batch_debug_stamps(self._b, None, 0, C.byref(n)))
        out = np.zeros(int(n.value), dtype=np.uint64)
        if n.value:
            check(self._lib.km_batch_debug_stamps(self._b, out.ctypes.data_as(C.c_void_p), n, C.byref(n)))
        return out.reshape(-1, 16)

    def sizes(self):
        """Sizes of a FULL delivery.  After a lean result() this (like fetch()) delivers again into the
        same pinned buffer: arrays returned by that result() must not be used afterwards."""
        s = BatchSizes()
        check(self._lib.km_batch_sizes(self._b, C.byref(s)))
        return s

    def wait_result(self):
        """Wait for the delivery of the last run (km_batch_result without building views);
        returns the batch sizes."""
        s = BatchSizes()
        check(self._lib.km_batch_result(self._b, None, C.byref(s)))
        return s

    def result(self):
        """Results of the last run as numpy views INTO the batch's pinned delivery buffer (no
        copy; valid until the next run / set_targets on this batch).  `node_kmer` is absent:
        node i < n_ref of a target is the k-mer at base i of the target, the walk-discovered
        nodes are in `extra_kmer` (CSR `extra_off`)."""
        out, s = BatchOut(), BatchSizes()
        check(self._lib.km_batch_result(self._b, C.byref(out), C.byref(s)))
        n = s.n_targets

        def view(p, count, dtype):
            if count == 0:
                return np.zeros(0, dtype)
            return np.ctypeslib.as_array(p, shape=(int(count),))

        extra = {}
        if not out.node_count and out.node_count16:
            # KM_DELIVER_COUNT16: the 16-bit form as delivered, and the counts as every consumer here reads them
            c16 = view(out.node_count16, s.n_nodes, np.uint16)
            esc_n = view(out.count_esc_node, s.n_count_escapes, np.uint64)
            esc_v = view(out.count_esc_value, s.n_count_escapes, np.uint32)
            counts = c16.astype(np.uint32)
            if s.n_count_escapes:
                counts[esc_n.astype(np.int64)] = esc_v
            extra = {"node_count16": c16, "count_esc_node": esc_n, "count_esc_value": esc_v, "node_count": counts}
        res = {
            "status": view(out.status, n, np.uint32), "n_ref": view(out.n_ref, n, np.uint32),
            "probes": view(out.probes, n, np.uint64), "node_off": view(out.node_off, n + 1, np.uint64),
            "extra_off": view(out.extra_off, n + 1, np.uint64),
            "ref_max_cov": view(out.ref_max_cov, n, np.uint32),
            "node_count": extra["node_count"] if extra else view(out.node_count, s.n_nodes, np.uint32),
            "extra_kmer": view(out.extra_kmer, s.n_extra, np.uint64),
            "path_off": view(out.path_off, n + 1, np.uint32),
            "run_off": view(out.run_off, s.n_paths + 1, np.uint64),
            "run_start": view(out.run_start, s.n_runs, np.uint32),
            "run_len": view(out.run_len, s.n_runs, np.uint32),
            "path_len": view(out.path_len, s.n_paths, np.uint32),
            "path_min_cov": view(out.path_min_cov, s.n_paths, np.uint32),
            "logical_probes": int(s.logical_probes), "table_fetches": int(s.table_fetches),
            "n_big_tier": int(s.n_big_tier), "n_flagged": int(s.n_flagged),
        }
        res.update(extra)
        return res

    def fetch(self, nodes=True, paths=True):
        """Copy results to host numpy arrays (dict), node k-mers rebuilt in full."""
        s = self.sizes()
        n = s.n_targets
        r = {
            "status": np.zeros(n, np.uint32), "n_ref": np.zeros(n, np.uint32),
            "probes": np.zeros(n, np.uint64), "node_off": np.zeros(n + 1, np.uint64),
            "logical_probes": int(s.logical_probes), "table_fetches": int(s.table_fetches),
            "n_big_tier": int(s.n_big_tier),
        }
        out = BatchOut()
        out.status = typed_ptr(r["status"], C.c_uint32)
        out.n_ref = typed_ptr(r["n_ref"], C.c_uint32)
        out.probes = typed_ptr(r["probes"], C.c_uint64)
        out.node_off = typed_ptr(r["node_off"], C.c_uint64)
        if nodes:
            r["node_kmer"] = np.zeros(max(1, s.n_nodes), np.uint64)
            r["node_count"] = np.zeros(max(1, s.n_nodes), np.uint32)
            out.node_kmer = typed_ptr(r["node_kmer"], C.c_uint64)
            out.node_count = typed_ptr(r["node_count"], C.c_uint32)
        if paths:
            r["path_off"] = np.zeros(n + 1, np.uint32)
            r["run_off"] = np.zeros(s.n_paths + 1, np.uint64)
            r["run_start"] = np.zeros(max(1, s.n_runs), np.uint32)
            r["run_len"] = np.zeros(max(1, s.n_runs), np.uint32)
            r["path_len"] = np.zeros(max(1, s.n_paths), np.uint32)
            r["path_min_cov"] = np.zeros(max(1, s.n_paths), np.uint32)
            out.path_off = typed_ptr(r["path_off"], C.c_uint32)
            out.run_off = typed_ptr(r["run_off"], C.c_uint64)
            out.run_start = typed_ptr(r["run_start"], C.c_uint32)
            out.run_len = typed_ptr(r["run_len"], C.c_uint32)
            out.path_len = typed_ptr(r["path_len"], C.c_uint32)
            out.path_min_cov = typed_ptr(r["path_min_cov"], C.c_uint32)
        check(self._lib.km_batch_fetch(self._b, C.byref(out)))
        if nodes:
            r["node_kmer"] = r["node_kmer"][: s.n_nodes]
            r["node_count"] = r["node_count"][: s.n_nodes]
        if paths:
            r["run_start"] = r["run_start"][: s.n_runs]
            r["run_len"] = r["run_len"][: s.n_runs]
            r["path_len"] = r["path_len"][: s.n_paths]
            r["path_min_cov"] = r["path_min_cov"][: s.n_paths]
        return r


def expand_path(res, p):
    """Node indices of path `p` (global path number) from the run-length records."""
    a, b = int(res["run_off"][p]), int(res["run_off"][p + 1])
    if b == a:
        return np.zeros(0, np.int64)
    return np.concatenate([np.arange(s, s + l, dtype=np.int64)
                           for s, l in zip(res["run_start"][a:b].tolist(),
                                           res["run_len"][a:b].tolist())])


REPORT_ERRORS = {1: IndexError("list index out of range"),
                 2: Exception("mutation identification could be incorrect"),
                 3: AssertionError(), 4: ValueError("min() arg is an empty sequence"),
                 5: RuntimeError("km_report_rows: the result view of this target is inconsistent")}


def _python_rows(res, t, name, seq, k, db_name):
    """Rows of target t through the Python restatement (km_amd/report.py)."""
    from . import report
    a, e = int(res["node_off"][t]), int(res["node_off"][t + 1])
    p0, p1 = int(res["path_off"][t]), int(res["path_off"][t + 1])
    paths = [expand_path(res, p) for p in range(p0, p1)]
    seq = seq if isinstance(seq, str) else bytes(seq).decode("ascii")
    if "node_kmer" in res:
        kmers = np.asarray(res["node_kmer"][a:e])
    else:                                              # delivery view: own k-mers from the sequence
        from . import kmer as km
        x0, x1 = int(res["extra_off"][t]), int(res["extra_off"][t + 1])
        kmers = np.concatenate([km.sliding_kmers(km.encode(seq), k)[:int(res["n_ref"][t])],
                                np.asarray(res["extra_kmer"][x0:x1])])
    tr = report.TargetResult(name, seq, k, int(res["n_ref"][t]), kmers,
                             np.asarray(res["node_count"][a:e]), paths,
                             np.asarray(res["path_min_cov"][p0:p1]).tolist())
    return report.target_rows(tr, db_name)


def pack_sequences(seqs):
    """(blob, offsets): the sequences as one uint8 array + uint64 offsets[n+1]."""
    enc = [s.encode("ascii") if isinstance(s, str) else bytes(s) for s in seqs]
    offs = np.zeros(len(enc) + 1, dtype=np.uint64)
    np.cumsum([len(e) for e in enc], out=offs[1:])
    return np.frombuffer(b"".join(enc) or b"\0", dtype=np.uint8), offs


def linear_kmin(seqs, start=10, device=0, stream=None, detail=False):
    """`km linear_kmin` (km/tools/linear_kmin.py:7-46) of every sequence (ASCII str or bytes, upper-cased)
    in one km_linear_kmin call: an int32 array of k.  detail=True also returns R (the longest repeated
    substring, int32) and the flag (uint8: some repeat of length R is not exempt), DESIGN.md §9."""
    lib = load()
    blob, offs = pack_sequences(seqs)
    n = len(offs) - 1
    kmin = np.zeros(n, np.int32)
    rep = np.zeros(n, np.int32)
    flag = np.zeros(n, np.uint8)
    check(lib.km_linear_kmin(device, ptr(blob), ptr(offs), n, start, ptr(kmin), ptr(rep), ptr(flag), stream))
    return (kmin, rep, flag) if detail else kmin


def report_rows(res, names, seqs, k, db_name, packed=None):
    """TSV rows of every target of a fetched batch (dict from Batch.fetch) through the C++
    reporting path: returns a list with, per target, a list of row strings (empty unless the
    target's status is KM_T_OK) or the exception the reference would have raised.
    `packed` = pack_sequences(seqs) when the caller already has it."""
    text, row_off, special = report_text(res, names, seqs, k, db_name, packed)
    result = []
    for t in range(len(names)):
        if t in special:
            result.append(special[t])
        else:
            a, e = int(row_off[t]), int(row_off[t + 1])
            result.append(text[a:e].splitlines() if e > a else [])
    return result


def report_text(res, names, seqs, k, db_name, packed=None):
    """The same as one string: (text, row_off, special).  text[row_off[t]:row_off[t+1]] is the block
    of target t, every row terminated by a newline; `special` maps the few targets that are NOT
    served by the text to their row list (numpy recomputation on a rounding tie) or to the exception
    the reference would have raised.  When `special` is empty, `text` is the whole TSV body."""
    lib = load()
    n = len(names)
    blob, offs = packed if packed is not None else pack_sequences(seqs)
    out = BatchOut()
    keep = []
    for field, ctype in (("status", C.c_uint32), ("n_ref", C.c_uint32), ("probes", C.c_uint64),
                         ("node_off", C.c_uint64), ("node_kmer", C.c_uint64), ("node_count", C.c_uint32),
                         ("path_off", C.c_uint32), ("run_off", C.c_uint64), ("run_start", C.c_uint32),
                         ("run_len", C.c_uint32), ("path_len", C.c_uint32), ("path_min_cov", C.c_uint32),
                         ("extra_off", C.c_uint64), ("extra_kmer", C.c_uint64), ("ref_max_cov", C.c_uint32)):
        if field not in res:
            continue                                   # a delivery view has no node_kmer, a fetch no extra_*
        if field == "node_count" and "node_count16" in res:
            continue                                   # the 16-bit form goes to the library as it came
        arr = np.ascontiguousarray(res[field], dtype=np.dtype(ctype))
        if arr.size == 0:
            arr = np.zeros(1, dtype=arr.dtype)
        keep.append(arr)
        setattr(out, field, typed_ptr(arr, ctype))
    n_esc = 0
    if "node_count16" in res:
        n_esc = int(np.asarray(res["count_esc_node"]).size)
        for field, ctype in (("node_count16", C.c_uint16), ("count_esc_node", C.c_uint64), ("count_esc_value", C.c_uint32)):
            arr = np.ascontiguousarray(res[field], dtype=np.dtype(ctype))
            if arr.size == 0:
                arr = np.zeros(1, dtype=arr.dtype)
            keep.append(arr)
            setattr(out, field, typed_ptr(arr, ctype))
    inp = ReportIn()
    inp.n_targets = n
    inp.bases = blob.ctypes.data
    inp.base_off = offs.ctypes.data
    name_arr = (C.c_char_p * max(1, n))(*[nm.encode() for nm in names])
    inp.names = name_arr
    inp.db_name = str(db_name).encode()
    inp.k = int(k)
    inp.res = C.pointer(out)
    # the lengths of the arrays, so that the library checks every offset against them first
    sz = BatchSizes()
    sz.n_targets = n
    sz.n_nodes = int(np.asarray(res["node_count"]).size)
    sz.n_paths = int(np.asarray(res["path_min_cov"]).size)
    sz.n_runs = int(np.asarray(res["run_start"]).size)
    sz.n_extra = int(np.asarray(res["extra_kmer"]).size) if "extra_kmer" in res else 0
    sz.n_count_escapes = n_esc
    inp.sizes = C.pointer(sz)
    text = C.c_void_p()
    row_off = C.POINTER(C.c_uint64)()
    err = C.POINTER(C.c_int32)()
    check(lib.km_report_rows(C.byref(inp), C.byref(text), C.byref(row_off), C.byref(err)))
    try:
        total = int(row_off[n])
        blob_out = C.string_at(text, total).decode("ascii")
        offs_out = np.ctypeslib.as_array(row_off, shape=(n + 1,)).copy()
        errs = np.ctypeslib.as_array(err, shape=(max(1, n),))[:n]
        special = {}
        for t in np.nonzero(errs)[0].tolist():
            if errs[t] == 100:
                # a printed value sits on a %.1f / %.3f rounding tie: the digit depends on the
                # last bits of the least-squares solver — recompute with numpy, like the reference
                special[t] = _python_rows(res, t, names[t], seqs[t], k, db_name)
            else:
                special[t] = REPORT_ERRORS.get(int(errs[t]), RuntimeError("report error %d" % errs[t]))
    finally:
        lib.km_report_free(text, row_off, err)
    return blob_out, offs_out, special
