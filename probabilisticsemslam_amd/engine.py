"""ctypes binding of include/kbest_c.h.  No compute happens in Python and there
is no fallback: if the HIP library is missing or no GPU is present, calls fail
loudly (KBestError)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

KBEST_FLAG_NO_PRUNE = 1
KBEST_FLAG_COUNT_PUSHED = 2
KBEST_FLAG_TABLES_I8 = 64
KBEST_FLAG_NO_REORDER = 128
KBEST_FLAG_NO_TIE_CHECK = 512
KBEST_FLAG_NO_TIE_RESOLVE = 1024
KBEST_FLAG_REFERENCE_ORDER = 2048
KBEST_FLAG_REFERENCE_TIES = 4096
KBEST_FLAG_CANONICAL_TIES = 8192
# per-problem tie flags (kbest_c.h, "Order of exact ties")
KBEST_TIE_INSIDE, KBEST_TIE_BOUNDARY, KBEST_TIE_RESOLVED, KBEST_TIE_REFERENCE = 1, 2, 4, 8
KBEST_TIE_UNCHECKED, KBEST_TIE_UNORDERED, KBEST_TIE_UNRESOLVED = 1 << 28, 1 << 29, 1 << 30
KBEST_ROUTE_LANE, KBEST_ROUTE_SMALL, KBEST_ROUTE_FAST, KBEST_ROUTE_WIDE, KBEST_ROUTE_RELAY, KBEST_ROUTE_EXTRA = 1, 2, 4, 8, 16, 32
KBEST_ROUTE_EXACT = 64
KBEST_ROUTE_SPLIT = 128  # (KBEST_SPLIT: several workgroups per matrix of the 64-row kernel, then the merge)
KBEST_TIE_CAP = 4096
KBEST_MAX_DIM = 64        # rows handled by the LDS-resident kernel
KBEST_MAX_DIM_WIDE = 1024  # rows of the general-size kernel (beyond KBEST_MAX_DIM)
KBEST_MAX_DIM_EXACT = 16384  # rows handled at all (the reference-order kernel beyond KBEST_MAX_DIM_WIDE)
KBEST_PERM_MAX_COLS = 16     # measurements per frame of the exact (permanent) association probabilities
KBEST_LBP_MAX_COLS = 128     # measurements per frame of the belief-propagation association probabilities
KBEST_CLUSTER_MAX_COLS = 128  # measurements per frame of the clustered exact association probabilities
KBEST_CLUSTER_MAX_SIZE = 16   # ... and per cluster
KBEST_BIGCLUSTER_MAX_SIZE = 20  # ... and per cluster of the big-cluster tier (one cluster over the whole chip)
KBEST_FRONTIER_MAX_COLS = 64    # ... and per cluster of the frontier tier (one workgroup per cluster)
KBEST_FRONTIER_MAX_WIDTH = 16   # ... whose rows, in the greedy order, keep at most this many columns open
KBEST_FRONTIER_SLOT = 4 << 20   # ... and whose layers fit this many bytes
KBEST_QUADRIC_MAP_MAX = 1 << 22  # landmarks a frame of the quadric-map entries sees at the most
KBEST_QUADRIC_MAP_TILE = 256     # ... and landmark rows per workgroup of their passes over the map

# every symbol include/kbest_c.h declares
C_ABI_SYMBOLS = (
    "kbest_default_opts", "kbest_create", "kbest_destroy", "kbest_strerror", "kbest_last_error",
    "kbest_device_count", "kbest_batch_f64_dev", "kbest_batch_f64", "kbest_reserve", "kbest_weights_batch_f64",
    "kbest_set_profile_buffer", "kbest_condition_costs_f64", "kbest_assoc_probs_batch_f64",
    "kbest_quadric_costs_f64", "kbest_quadric_assoc_probs_batch_f64", "kbest_bb_match_batch_f64",
    "kbest_bruteforce_probs_batch_f64", "kbest_assign_batch_f64", "kbest_to_probs_f64",
    "kbest_assoc_probs_batch_f64_dev", "kbest_reserve_assoc",
    "kbest_create_multi", "kbest_destroy_multi", "kbest_multi_size", "kbest_multi_last_error", "kbest_batch_f64_multi",
    "kbest_multi_tables_agree", "kbest_batch_f64_multi_ex", "kbest_merge_topk_f64_dev", "kbest_register_host_buffer",
    "kbest_unregister_host_buffer", "kbest_multi_timeline", "kbest_last_tie_flags", "kbest_set_assoc_tie_flags_dev",
    "kbest_relay_launches", "kbest_merge_topk_i8_f64_dev", "kbest_merge_gains_f64_dev", "kbest_multi_exchange_bytes",
    "kbest_last_route", "kbest_resolve_ties_dev", "kbest_multi_last_tie_flags", "kbest_reserve_exact",
    "kbest_set_reference_order", "kbest_permanent_probs_batch_f64", "kbest_permanent_probs_batch_f64_dev",
    "kbest_reserve_permanent", "kbest_set_permanent_work_cap", "kbest_last_permanent_grid",
    "kbest_sample_assoc_batch_f64", "kbest_sample_assoc_batch_f64_dev", "kbest_reserve_sample",
    "kbest_belief_probs_batch_f64", "kbest_belief_probs_batch_f64_dev", "kbest_reserve_belief", "kbest_set_belief_lds_limit",
    "kbest_clustered_probs_batch_f64", "kbest_clustered_probs_batch_f64_dev", "kbest_reserve_clustered",
    "kbest_set_clustered_slot_cap", "kbest_set_clustered_work_cap", "kbest_last_clustered_grid",
    "kbest_clustered_sample_assoc_batch_f64", "kbest_clustered_sample_assoc_batch_f64_dev", "kbest_reserve_clustered_sample",
    "kbest_clustered_partial_batch_f64_dev", "kbest_hybrid_probs_batch_f64",
    "kbest_reserve_bigcluster", "kbest_set_bigcluster_work_cap", "kbest_bigcluster_probs_f64_dev",
    "kbest_hybrid_exact_probs_batch_f64",
    "kbest_reserve_frontier", "kbest_set_frontier_work_cap", "kbest_set_frontier_slot", "kbest_frontier_probs_f64_dev",
    "kbest_hybrid_frontier_probs_batch_f64",
    "kbest_reserve_hybrid_dev", "kbest_hybrid_frontier_probs_batch_f64_dev",
    "kbest_reserve_frontier_sample", "kbest_frontier_sample_f64_dev", "kbest_hybrid_frontier_sample_assoc_batch_f64",
    "kbest_reserve_hybrid_sample_dev", "kbest_hybrid_frontier_sample_assoc_batch_f64_dev",
    "kbest_table_sample_f64_dev", "kbest_hybrid_sample_assoc_batch_f64",
    "kbest_bb_costs_f64",
    "kbest_reserve_quadric_map_dev", "kbest_quadric_map_probs_batch_f64_dev", "kbest_quadric_map_probs_batch_f64",
    "kbest_quadric_map_kernel_usage",
    "kbest_reserve_quadric_map_sample_dev", "kbest_quadric_map_sample_assoc_batch_f64_dev", "kbest_quadric_map_sample_assoc_batch_f64",
    "kbest_quadric_map_sample_kernel_usage",
    "kbest_reserve_assoc_factors_dev", "kbest_assoc_factors_f64_dev", "kbest_reserve_quadric_map_factors_dev",
    "kbest_quadric_map_factors_batch_f64_dev", "kbest_assoc_factors_batch_f64", "kbest_factors_kernel_usage",
)
KBEST_MULTI_STAMPS = 6
KBEST_MULTI_BATCH, KBEST_MULTI_SUBTREE = 0, 1


class KBestError(RuntimeError):
    pass


class KBestOpts(C.Structure):
    _fields_ = [("maximize", C.c_int32), ("use_cutoff", C.c_int32), ("cutoff", C.c_double), ("flags", C.c_uint32),
                ("root_col_offset", C.c_int32), ("root_col_stride", C.c_int32), ("tie_flags", C.c_void_p)]


def lib_path() -> str:
    # KBEST_LIB selects another in-tree build of the same library (the diagnostic libkbest_amd_prof.so)
    return os.path.join(_HERE, os.environ.get("KBEST_LIB", "libkbest_amd.so"))


_lib = None


def load_library():
    """Load the in-tree HIP library; raises KBestError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise KBestError(f"{path} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                         "(there is no CPU fallback)")
    lib = C.CDLL(path)
    vp, i32p, i64p, dp = C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p
    lib.kbest_default_opts.argtypes = [C.POINTER(KBestOpts)]
    lib.kbest_default_opts.restype = None
    lib.kbest_create.argtypes = [C.POINTER(vp), C.c_int]
    lib.kbest_destroy.argtypes = [vp]
    lib.kbest_strerror.argtypes = [C.c_int]
    lib.kbest_strerror.restype = C.c_char_p
    lib.kbest_last_error.argtypes = [vp]
    lib.kbest_last_error.restype = C.c_char_p
    lib.kbest_device_count.restype = C.c_int
    lib.kbest_reserve.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    if hasattr(lib, "kbest_reserve_exact"):
        lib.kbest_reserve_exact.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.kbest_set_profile_buffer.argtypes = [vp, vp]
    lib.kbest_batch_f64_dev.argtypes = [vp, C.POINTER(KBestOpts), C.c_int, C.c_int, C.c_int, i32p, i32p, dp, i64p,
                                        C.c_int, i32p, i32p, dp, i32p, i64p, vp]
    lib.kbest_batch_f64.argtypes = [vp, C.POINTER(KBestOpts), C.c_int, C.c_int, C.c_int, i32p, i32p, dp, i64p,
                                    C.c_int, i32p, i32p, dp, i32p, i64p]
    lib.kbest_weights_batch_f64.argtypes = [vp, C.c_int, i32p, i32p, dp, i64p, C.c_int, dp, i64p, i32p]
    lib.kbest_assoc_probs_batch_f64.argtypes = [vp, C.c_int, i32p, i32p, dp, i64p, C.c_int, dp, i64p, i32p]
    lib.kbest_bruteforce_probs_batch_f64.argtypes = [vp, C.c_int, i32p, i32p, dp, i64p, C.c_int, dp, i64p, i32p]
    lib.kbest_condition_costs_f64.argtypes = [vp, C.c_int, i32p, i32p, dp, i64p, dp, i32p, i32p, C.c_int]
    lib.kbest_quadric_costs_f64.argtypes = [vp, C.c_int, i32p, i32p, dp, dp, dp, dp, C.c_double, dp]
    lib.kbest_quadric_assoc_probs_batch_f64.argtypes = [vp, C.c_int, i32p, i32p, dp, dp, dp, dp, C.c_double, C.c_int,
                                                        dp, i64p, i32p]
    lib.kbest_bb_match_batch_f64.argtypes = [vp, C.c_int, i32p, i32p, dp, dp, C.c_double, i32p]
    lib.kbest_bb_costs_f64.argtypes = [vp, C.c_int, i32p, i32p, dp, dp, C.c_double, dp]
    lib.kbest_assign_batch_f64.argtypes = [vp, C.c_int, C.c_int, C.c_int, i32p, i32p, dp, i64p, C.c_int, C.c_int, C.c_int,
                                           i32p, i32p, dp, dp, dp, i32p]
    lib.kbest_to_probs_f64.argtypes = [vp, dp, C.c_int64]
    lib.kbest_assoc_probs_batch_f64_dev.argtypes = [vp, C.c_int, C.c_int, C.c_int, i32p, i32p, i32p, dp, i64p, C.c_int, C.c_int,
                                                    dp, i64p, i32p, vp]
    lib.kbest_reserve_assoc.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.kbest_create_multi.argtypes = [C.POINTER(vp), i32p, C.c_int]
    lib.kbest_destroy_multi.argtypes = [vp]
    lib.kbest_multi_size.argtypes = [vp]
    lib.kbest_multi_last_error.argtypes = [vp]
    lib.kbest_multi_last_error.restype = C.c_char_p
    lib.kbest_batch_f64_multi.argtypes = [vp, C.POINTER(KBestOpts), C.c_int, C.c_int, C.c_int, i32p, i32p, dp, C.c_int, i32p,
                                          i32p, dp, i32p]
    lib.kbest_multi_tables_agree.argtypes = [vp]
    lib.kbest_batch_f64_multi_ex.argtypes = [vp, C.POINTER(KBestOpts), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, i32p, i32p, dp,
                                             C.c_int, i32p, i32p, dp, i32p]
    lib.kbest_merge_topk_f64_dev.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int64, dp, i32p,
                                             i32p, vp]
    if hasattr(lib, "kbest_merge_gains_f64_dev"):
        lib.kbest_merge_topk_i8_f64_dev.argtypes = lib.kbest_merge_topk_f64_dev.argtypes
        lib.kbest_merge_gains_f64_dev.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, dp, i32p, C.c_int, vp, dp, vp, i32p, i32p, vp]
        lib.kbest_multi_exchange_bytes.argtypes = [vp, C.POINTER(C.c_int)]
        lib.kbest_multi_exchange_bytes.restype = C.c_longlong
    if hasattr(lib, "kbest_multi_timeline"):  # (absent from older in-tree builds selected with KBEST_LIB for A/B runs)
        lib.kbest_multi_timeline.argtypes = [vp, dp, C.c_int]
    if hasattr(lib, "kbest_relay_launches"):
        lib.kbest_relay_launches.argtypes = [vp]
        lib.kbest_relay_launches.restype = C.c_longlong
    if hasattr(lib, "kbest_last_route"):
        lib.kbest_last_route.argtypes = [vp]
        lib.kbest_resolve_ties_dev.argtypes = [vp, C.POINTER(KBestOpts), C.c_int, C.c_int, C.c_int, i32p, i32p, dp, i64p, C.c_int, i32p, i32p, dp,
                                               i32p, i32p, vp]
        lib.kbest_multi_last_tie_flags.argtypes = [vp, i32p, C.c_int]
    if hasattr(lib, "kbest_last_tie_flags"):
        lib.kbest_last_tie_flags.argtypes = [vp, i32p, C.c_int]
        lib.kbest_set_assoc_tie_flags_dev.argtypes = [vp, vp]
    if hasattr(lib, "kbest_permanent_probs_batch_f64"):
        lib.kbest_permanent_probs_batch_f64.argtypes = [vp, C.c_int, i32p, i32p, dp, i64p, C.c_int, dp, i64p, dp]
        lib.kbest_permanent_probs_batch_f64_dev.argtypes = [vp, C.c_int, C.c_int, C.c_int, i32p, i32p, dp, i64p, C.c_int, dp, i64p, dp, vp]
        lib.kbest_reserve_permanent.argtypes = [vp, C.c_int, C.c_int, C.c_int]
        lib.kbest_set_permanent_work_cap.argtypes = [vp, C.c_size_t]
        lib.kbest_last_permanent_grid.argtypes = [vp]
    if hasattr(lib, "kbest_sample_assoc_batch_f64"):
        lib.kbest_sample_assoc_batch_f64.argtypes = [vp, C.c_int, i32p, i32p, dp, i64p, C.c_int, C.c_int, C.c_uint64, C.c_uint32, i64p,
                                                     i32p, i64p, dp, i64p, dp]
        lib.kbest_sample_assoc_batch_f64_dev.argtypes = [vp, C.c_int, C.c_int, C.c_int, i32p, i32p, dp, i64p, C.c_int, C.c_int,
                                                         C.c_uint64, C.c_uint32, i64p, i32p, i64p, dp, i64p, dp, vp]
        lib.kbest_reserve_sample.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    if hasattr(lib, "kbest_belief_probs_batch_f64"):
        lib.kbest_belief_probs_batch_f64.argtypes = [vp, C.c_int, i32p, i32p, dp, i64p, C.c_int, C.c_double, C.c_int, dp, i64p, i32p, dp]
        lib.kbest_belief_probs_batch_f64_dev.argtypes = [vp, C.c_int, C.c_int, C.c_int, i32p, i32p, dp, i64p, C.c_int, C.c_double,
                                                         C.c_int, dp, i64p, i32p, dp, vp]
        lib.kbest_reserve_belief.argtypes = [vp, C.c_int, C.c_int, C.c_int]
        lib.kbest_set_belief_lds_limit.argtypes = [vp, C.c_size_t]
    if hasattr(lib, "kbest_clustered_probs_batch_f64"):
        lib.kbest_clustered_probs_batch_f64.argtypes = [vp, C.c_int, i32p, i32p, dp, i64p, C.c_int, dp, i64p, dp, i32p, i32p, i32p,
                                                        C.c_int]
        lib.kbest_clustered_probs_batch_f64_dev.argtypes = [vp, C.c_int, C.c_int, C.c_int, i32p, i32p, dp, i64p, C.c_int, dp, i64p,
                                                            dp, i32p, i32p, i32p, C.c_int, vp]
        lib.kbest_reserve_clustered.argtypes = [vp, C.c_int, C.c_int, C.c_int]
        lib.kbest_set_clustered_slot_cap.argtypes = [vp, C.c_size_t]
        lib.kbest_set_clustered_work_cap.argtypes = [vp, C.c_size_t]
        lib.kbest_last_clustered_grid.argtypes = [vp]
    if hasattr(lib, "kbest_clustered_sample_assoc_batch_f64"):
        lib.kbest_clustered_sample_assoc_batch_f64.argtypes = [vp, C.c_int, i32p, i32p, dp, i64p, C.c_int, C.c_int, C.c_uint64, C.c_uint32,
                                                               i64p, i32p, i64p, dp, i64p, dp, i32p, i32p]
        lib.kbest_clustered_sample_assoc_batch_f64_dev.argtypes = [vp, C.c_int, C.c_int, C.c_int, i32p, i32p, dp, i64p, C.c_int, C.c_int,
                                                                   C.c_uint64, C.c_uint32, i64p, i32p, i64p, dp, i64p, dp, i32p, i32p, vp]
        lib.kbest_reserve_clustered_sample.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    if hasattr(lib, "kbest_hybrid_probs_batch_f64"):
        lib.kbest_clustered_partial_batch_f64_dev.argtypes = [vp, C.c_int, C.c_int, C.c_int, i32p, i32p, dp, i64p, C.c_int, C.c_int,
                                                              dp, i64p, dp, i32p, i32p, i32p, C.c_int, i32p, i32p, C.c_int, i32p,
                                                              C.c_int, dp, vp]
        lib.kbest_hybrid_probs_batch_f64.argtypes = [vp, C.c_int, i32p, i32p, dp, i64p, C.c_int, C.c_int, C.c_int, dp, i64p, i32p,
                                                     i32p, i32p]
    if hasattr(lib, "kbest_hybrid_exact_probs_batch_f64"):
        lib.kbest_reserve_bigcluster.argtypes = [vp, C.c_int, C.c_int]
        lib.kbest_set_bigcluster_work_cap.argtypes = [vp, C.c_size_t]
        lib.kbest_bigcluster_probs_f64_dev.argtypes = [vp, C.c_int, i32p, i32p, i64p, i64p, dp, dp, dp, i32p, vp]
        lib.kbest_hybrid_exact_probs_batch_f64.argtypes = [vp, C.c_int, i32p, i32p, dp, i64p, C.c_int, C.c_int, C.c_int, C.c_int, dp,
                                                           i64p, dp, i32p, i32p, i32p, i32p]
    if hasattr(lib, "kbest_hybrid_frontier_probs_batch_f64"):
        lib.kbest_reserve_frontier.argtypes = [vp, C.c_int, C.c_int, C.c_int]
        lib.kbest_set_frontier_work_cap.argtypes = [vp, C.c_size_t]
        lib.kbest_set_frontier_slot.argtypes = [vp, C.c_size_t]
        lib.kbest_frontier_probs_f64_dev.argtypes = [vp, C.c_int, i32p, i32p, i64p, i64p, dp, dp, dp, i32p, i32p, vp]
        lib.kbest_hybrid_frontier_probs_batch_f64.argtypes = [vp, C.c_int, i32p, i32p, dp, i64p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                              C.c_int, dp, i64p, dp, i32p, i32p, i32p, i32p, i32p]
    if hasattr(lib, "kbest_hybrid_frontier_probs_batch_f64_dev"):
        lib.kbest_reserve_hybrid_dev.argtypes = [vp, C.c_int, C.c_int, C.c_int]
        lib.kbest_hybrid_frontier_probs_batch_f64_dev.argtypes = [vp, C.c_int, C.c_int, C.c_int, i32p, i32p, dp, i64p, C.c_int, C.c_int,
                                                                  C.c_int, dp, dp, i64p, dp, i32p, i32p, i32p, i32p, vp]
    if hasattr(lib, "kbest_frontier_sample_f64_dev"):
        lib.kbest_reserve_frontier_sample.argtypes = [vp, C.c_int, C.c_int, C.c_int]
        lib.kbest_frontier_sample_f64_dev.argtypes = [vp, C.c_int, i32p, i32p, i64p, dp, i32p, i64p, i64p, C.c_int, C.c_uint64,
                                                      C.c_uint32, i32p, i64p, dp, i64p, dp, i32p, i32p, vp]
        lib.kbest_hybrid_frontier_sample_assoc_batch_f64.argtypes = [vp, C.c_int, i32p, i32p, dp, i64p, C.c_int, C.c_int, C.c_int,
                                                                     C.c_int, C.c_uint64, C.c_uint32, i64p, i32p, i64p, dp, i64p, dp,
                                                                     i32p, i32p, i32p, i32p]
    if hasattr(lib, "kbest_hybrid_frontier_sample_assoc_batch_f64_dev"):
        lib.kbest_reserve_hybrid_sample_dev.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
        lib.kbest_hybrid_frontier_sample_assoc_batch_f64_dev.argtypes = [vp, C.c_int, C.c_int, C.c_int, i32p, i32p, dp, i64p, C.c_int,
                                                                         C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint32, i64p, dp,
                                                                         i32p, i64p, dp, i64p, dp, i32p, i32p, i32p, i32p, vp]
    if hasattr(lib, "kbest_table_sample_f64_dev"):
        lib.kbest_table_sample_f64_dev.argtypes = [vp, C.c_int, C.c_int, C.c_int, i32p, i32p, dp, i32p, C.c_double, i32p, i64p, C.c_int,
                                                   C.c_uint64, C.c_uint32, i32p, i64p, dp, i64p, i32p, i32p, vp]
        lib.kbest_hybrid_sample_assoc_batch_f64.argtypes = [vp, C.c_int, i32p, i32p, dp, i64p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                            C.c_int, C.c_uint64, C.c_uint32, i64p, i32p, i64p, dp, i64p, dp, i32p,
                                                            i32p, i32p, i32p, i32p]
    if hasattr(lib, "kbest_quadric_map_probs_batch_f64_dev"):
        lib.kbest_reserve_quadric_map_dev.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
        lib.kbest_quadric_map_probs_batch_f64_dev.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, i64p, i32p, dp, dp, i64p,
                                                              i32p, C.c_double, C.c_int, C.c_int, i32p, i32p, dp, dp, dp, i64p, dp,
                                                              i32p, i32p, i32p, i32p, vp]
        lib.kbest_quadric_map_probs_batch_f64.argtypes = [vp, C.c_int, C.c_int, dp, dp, i64p, i32p, i32p, dp, dp, C.c_double, C.c_int,
                                                          C.c_int, C.c_int, C.c_int, dp, i64p, dp, i32p, i32p, i32p, i32p, i32p, i32p]
        lib.kbest_quadric_map_kernel_usage.argtypes = [C.c_int, i32p, i32p, i32p]
    if hasattr(lib, "kbest_quadric_map_sample_assoc_batch_f64_dev"):
        lib.kbest_reserve_quadric_map_sample_dev.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        lib.kbest_quadric_map_sample_assoc_batch_f64_dev.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, i64p, i32p, dp, dp,
                                                                     i64p, i32p, C.c_double, C.c_int, C.c_int, C.c_int, C.c_uint64,
                                                                     C.c_uint32, i64p, i32p, i32p, dp, i32p, i64p, dp, i64p, dp, i32p,
                                                                     i32p, i32p, i32p, vp]
        lib.kbest_quadric_map_sample_assoc_batch_f64.argtypes = [vp, C.c_int, C.c_int, dp, dp, i64p, i32p, i32p, dp, dp, C.c_double,
                                                                 C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint32, i64p, i32p,
                                                                 i64p, dp, i64p, dp, i32p, i32p, i32p, i32p, i32p, i32p]
        lib.kbest_quadric_map_sample_kernel_usage.argtypes = [i32p, i32p, i32p]
    if hasattr(lib, "kbest_assoc_factors_f64_dev"):
        i64 = C.c_int64
        # thresholds, capacities, lists, counts, support: the factor arguments every entry ends with (before the stream)
        fargs = [C.c_double, C.c_double, C.c_double, i64, i32p, i32p, i32p, i64p, dp, dp, i64, i32p, i32p, dp, dp, i32p, i64p, i32p,
                 i64p, i64p, i32p, i64]
        lib.kbest_reserve_assoc_factors_dev.argtypes = [vp, C.c_int, C.c_int]
        lib.kbest_assoc_factors_f64_dev.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp, i64p, i32p, i32p, i32p, i64, i64p, i32p] + fargs + [vp]
        lib.kbest_reserve_quadric_map_factors_dev.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
        lib.kbest_quadric_map_factors_batch_f64_dev.argtypes = lib.kbest_quadric_map_probs_batch_f64_dev.argtypes[:-1] + fargs + [vp]
        lib.kbest_assoc_factors_batch_f64.argtypes = [vp, C.c_int, dp, i64p, i32p, i32p, i64p, i32p] + fargs
        lib.kbest_factors_kernel_usage.argtypes = [C.c_int, i32p, i32p, i32p]
    lib.kbest_register_host_buffer.argtypes = [vp, vp, C.c_size_t]
    lib.kbest_unregister_host_buffer.argtypes = [vp, vp]
    _lib = lib
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _dptr(t):
    """Device pointer of a torch CUDA tensor (or a raw address, or None)."""
    return None if t is None else C.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else int(t))


def _stream(s):
    return C.c_void_p(s) if s else None


def _pack_frames(costs, nL, nM, who):
    """The frame batch of the probability entries: costs is a list of 1-D column-major (nL+nM) x nM blocks.  Returns (nL, nM
    as int32 arrays, B, the blocks end to end, costOff[B], probOff[B], psizes[B]: doubles of every frame's [nM, nL+1] slice,
    probs: the zeroed slices end to end)."""
    nL = np.ascontiguousarray(nL, dtype=np.int32)
    nM = np.ascontiguousarray(nM, dtype=np.int32)
    B = len(nL)
    sizes = (nL.astype(np.int64) + nM) * nM
    psizes = nM.astype(np.int64) * (nL.astype(np.int64) + 1)
    costOff = np.zeros(B, np.int64)
    probOff = np.zeros(B, np.int64)
    costOff[1:] = np.cumsum(sizes)[:-1]
    probOff[1:] = np.cumsum(psizes)[:-1]
    flat = np.concatenate([np.zeros(0, np.float64)] + [np.ascontiguousarray(c, dtype=np.float64).reshape(-1) for c in costs])
    if flat.size != int(sizes.sum()):
        raise KBestError(f"{who}: a cost block is not (nL + nM) x nM")
    probs = np.zeros(int(psizes.sum()), np.float64)
    return nL, nM, B, flat, costOff, probOff, psizes, probs


def _split_probs(probs, probOff, psizes, nL, nM):
    """The frames' [nM, nL+1] views of probs."""
    return [probs[probOff[b]: probOff[b] + psizes[b]].reshape(int(nM[b]), int(nL[b]) + 1) for b in range(len(nL))]


def _pack_draws(nM, B, n_sample, frame_key, who):
    """The draw buffers of the sampling entries, frame after frame: n_sample as int, asgOff[B], lpOff[B], assign (int32, every
    frame's [n_sample, nM]), logp (float64, every frame's [n_sample]), both zeroed, and the keys as uint64[B] (None: no keys)."""
    n_sample = int(n_sample)
    sizes = nM.astype(np.int64) * max(n_sample, 0)
    asgOff = np.zeros(B, np.int64)
    asgOff[1:] = np.cumsum(sizes)[:-1]
    lpOff = np.arange(B, dtype=np.int64) * n_sample
    key = None if frame_key is None else np.ascontiguousarray(frame_key, dtype=np.uint64)
    if key is not None and key.shape != (B,):
        raise KBestError(f"{who}: frame_key must hold one key per frame")
    return n_sample, asgOff, lpOff, np.zeros(int(sizes.sum()), np.int32), np.zeros(B * max(n_sample, 0), np.float64), key


def _split_draws(assign, asgOff, logp, lpOff, nM, n_sample):
    """The frames' [n_sample, nM] views of assign and [n_sample] views of logp."""
    return ([assign[asgOff[b]: asgOff[b] + n_sample * int(nM[b])].reshape(n_sample, int(nM[b])) for b in range(len(nM))],
            [logp[lpOff[b]: lpOff[b] + n_sample] for b in range(len(nM))])


class KBestEngine:
    """One engine context = one GPU, one stream, one hypothesis-state workspace."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        self.ctx = C.c_void_p()
        rc = self.lib.kbest_create(C.byref(self.ctx), device)
        if rc != 0:
            raise KBestError(f"kbest_create(device={device}): {self.lib.kbest_strerror(rc).decode()}")

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.kbest_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise KBestError(f"{self.lib.kbest_strerror(rc).decode()}: {self.lib.kbest_last_error(self.ctx).decode()}")

    def _opts(self, maximize, cutoff, flags=0, root_shard=None):
        o = KBestOpts()
        self.lib.kbest_default_opts(C.byref(o))
        o.maximize = int(bool(maximize))
        o.use_cutoff = int(cutoff is not None)
        o.cutoff = float(cutoff) if cutoff is not None else 0.0
        o.flags = flags
        if root_shard is not None:
            o.root_col_offset, o.root_col_stride = root_shard
        return o

    # ---- host buffers -----------------------------------------------------------------
    def kbest(self, costs, N, M, k, maximize=False, cutoff=None, nRow=None, nCol=None, costOff=None,
              count_pushed=False, prune=True, root_shard=None, tables_i8=False, reorder=True, tie_flags=False,
              tie_check=True, tie_resolve=True, reference_order=False, reference_ties=False, canonical_ties=False):
        """Batched kBest2D / kBest2DCutoff.  costs: (B, N*M) for uniform shapes, or a flat packed
        array with per-problem nRow/nCol/costOff (N, M are then the maxima).
        Returns (nf[B], row4col[B,k,M], col4row[B,k,N], gain[B,k]) (+ pushed[B] if count_pushed).
        tables_i8: the two tables come back as int8 (KBEST_FLAG_TABLES_I8; N <= 127).
        tie_flags: also return the per-problem KBEST_TIE_* flags (last element of the tuple).
        reference_order: KBEST_FLAG_REFERENCE_ORDER -- the reference's own order of operations (exact ties in its heap's order,
        col4row on padded columns as the reference names them; slow).
        reference_ties: KBEST_FLAG_REFERENCE_TIES -- the fast kernels, and every problem with an exact tie among its k + 1 best gains
        again on the reference-order kernel (KBEST_TIE_REFERENCE): the reference's answer everywhere, fast where nothing ties.  This
        is the DEFAULT of the synchronous entries (the flag is accepted and changes nothing).
        canonical_ties: KBEST_FLAG_CANONICAL_TIES -- the engine's own rule on exact ties instead ((gain, row4col) lexicographic; a
        level that straddles slot k completed in steps of up to 4 096 solutions)."""
        costs = np.ascontiguousarray(costs, dtype=np.float64)
        if nRow is None:
            costs = costs.reshape(-1, N * M)
            B = costs.shape[0]
        else:
            nRow = np.ascontiguousarray(nRow, dtype=np.int32)
            nCol = np.ascontiguousarray(nCol, dtype=np.int32)
            costOff = np.ascontiguousarray(costOff, dtype=np.int64)
            B = len(nRow)
        tdt = np.int8 if tables_i8 else np.int32
        r4c = np.empty((B, k, M), tdt)
        c4r = np.empty((B, k, N), tdt)
        gain = np.empty((B, k), np.float64)
        nf = np.empty(B, np.int32)
        pushed = np.zeros(B, np.int64) if count_pushed else None
        flags = ((KBEST_FLAG_COUNT_PUSHED if count_pushed else 0) | (0 if prune else KBEST_FLAG_NO_PRUNE) |
                 (KBEST_FLAG_TABLES_I8 if tables_i8 else 0) | (0 if reorder else KBEST_FLAG_NO_REORDER) |
                 (0 if tie_check else KBEST_FLAG_NO_TIE_CHECK) | (0 if tie_resolve else KBEST_FLAG_NO_TIE_RESOLVE) |
                 (KBEST_FLAG_REFERENCE_ORDER if reference_order else 0) | (KBEST_FLAG_REFERENCE_TIES if reference_ties else 0) |
                 (KBEST_FLAG_CANONICAL_TIES if canonical_ties else 0))
        o = self._opts(maximize, cutoff, flags, root_shard)
        tf = np.zeros(B, np.int32) if tie_flags else None
        if tf is not None:
            o.tie_flags = tf.ctypes.data
        self._check(self.lib.kbest_batch_f64(self.ctx, C.byref(o), B, N, M, _ptr(nRow), _ptr(nCol), _ptr(costs),
                                             _ptr(costOff), k, _ptr(r4c), _ptr(c4r), _ptr(gain), _ptr(nf),
                                             _ptr(pushed)))
        out = (nf, r4c, c4r, gain) + ((pushed,) if count_pushed else ()) + ((tf,) if tie_flags else ())
        return out

    def assign(self, costs, N, M, maximize=False, shift=True, gain_cols=0):
        """Batched assign2D (shift=True) / shortestPathCPP (shift=False) on uniform N x M problems, costs (B, N*M).
        Returns (feasible[B], row4col[B,M], col4row[B,N] (-1 = unassigned), gain[B], u[B,M], v[B,N])."""
        costs = np.ascontiguousarray(costs, dtype=np.float64).reshape(-1, N * M)
        B = costs.shape[0]
        r4c = np.empty((B, M), np.int32); c4r = np.empty((B, N), np.int32)
        g = np.empty(B); u = np.empty((B, M)); v = np.empty((B, N)); ok = np.empty(B, np.int32)
        self._check(self.lib.kbest_assign_batch_f64(self.ctx, B, N, M, None, None, _ptr(costs), None, int(bool(maximize)),
                                                    int(bool(shift)), int(gain_cols), _ptr(r4c), _ptr(c4r), _ptr(g), _ptr(u),
                                                    _ptr(v), _ptr(ok)))
        return ok, r4c, c4r, g, u, v

    def to_probs(self, x):
        """toProbs (assignment.h:19): returns exp(min - x) with the 42 gate."""
        x = np.array(x, dtype=np.float64).reshape(-1)
        self._check(self.lib.kbest_to_probs_f64(self.ctx, _ptr(x), x.size))
        return x

    def condition_costs(self, costs, nRows, nCols):
        """Batched conditionCosts.  Returns (list of conditioned 1-D blocks, list of rowIdx arrays)."""
        nRows = np.ascontiguousarray(nRows, dtype=np.int32)
        nCols = np.ascontiguousarray(nCols, dtype=np.int32)
        B = len(nRows)
        sizes = nRows.astype(np.int64) * nCols
        off = np.zeros(B, np.int64)
        off[1:] = np.cumsum(sizes)[:-1]
        flat = np.concatenate([np.ascontiguousarray(c, dtype=np.float64).reshape(-1) for c in costs])
        out = np.zeros_like(flat)
        good = np.zeros(B, np.int32)
        maxRow = int(nRows.max())
        ridx = np.zeros((B, maxRow), np.int32)
        self._check(self.lib.kbest_condition_costs_f64(self.ctx, B, _ptr(nRows), _ptr(nCols), _ptr(flat), _ptr(off),
                                                       _ptr(out), _ptr(good), _ptr(ridx), maxRow))
        return ([out[off[b]: off[b] + int(good[b]) * int(nCols[b])].copy() for b in range(B)],
                [ridx[b, : good[b]].copy() for b in range(B)])

    def relay_launches(self):
        """Launches of the 64-row kernel this context has made as a relay (diagnostic, kbest_relay_launches)."""
        return int(self.lib.kbest_relay_launches(self.ctx))

    def set_reference_order(self, on=True):
        """kbest_set_reference_order: the host-buffer association entries enumerate in the reference's own order of operations
        (on = 1 / True), or only their frames with a tie at slot k do (on = 2: the same answer, fused kernels wherever nothing ties)."""
        self.lib.kbest_set_reference_order.argtypes = [C.c_void_p, C.c_int]
        self._check(self.lib.kbest_set_reference_order(self.ctx, int(on)))

    def last_route(self):
        """KBEST_ROUTE_* bits of the kernel(s) this context's last k-best launch went to (diagnostic, kbest_last_route)."""
        return int(self.lib.kbest_last_route(self.ctx))

    def last_tie_flags(self):
        """KBEST_TIE_* flags of the problems of this context's last synchronous call (kbest_last_tie_flags)."""
        n = self.lib.kbest_last_tie_flags(self.ctx, None, 0)
        out = np.zeros(max(n, 0), np.int32)
        if n > 0:
            self.lib.kbest_last_tie_flags(self.ctx, _ptr(out), n)
        return out

    def set_assoc_tie_flags_dev(self, d_flags):
        """Where assoc_probs_dev writes its frames' KBEST_TIE_* flags (an int32 [B] torch CUDA tensor, or None)."""
        self._check(self.lib.kbest_set_assoc_tie_flags_dev(self.ctx, None if d_flags is None else C.c_void_p(d_flags.data_ptr())))

    def weights(self, costs, nL, nM, k, condition=False, brute_force=False):
        """Batched assignmentProb (condition=False) or, with condition=True, the whole
        conditionCosts -> assignmentProb -> scatter chain of getAssignmentProbs on raw cost blocks.
        costs: list of 1-D column-major (nL+nM) x nM blocks.  Returns (list of [nM, nL+1] arrays, nf[B])."""
        nL, nM, B, flat, costOff, probOff, psizes, probs = _pack_frames(costs, nL, nM, "weights")
        nf = np.zeros(B, np.int32)
        fn = (self.lib.kbest_bruteforce_probs_batch_f64 if brute_force else
              self.lib.kbest_assoc_probs_batch_f64 if condition else self.lib.kbest_weights_batch_f64)
        self._check(fn(self.ctx, B, _ptr(nL), _ptr(nM), _ptr(flat), _ptr(costOff), k, _ptr(probs), _ptr(probOff),
                       _ptr(nf)))
        out = _split_probs(probs, probOff, psizes, nL, nM)
        return out, nf

    def permanent_probs(self, costs, nL, nM, condition=False):
        """Batched permanentProb (assignment.h:13): the EXACT association probabilities, nM <= 16 (kbest_perm.hip).  Packing as
        weights(); condition=True: raw blocks, conditionCosts -> permanentProb -> scatter back (getAssignmentProbs with usePerm).
        Returns (list of [nM, nL+1] arrays, perm[B]: the permanent of every frame's toProbs matrix, the normaliser)."""
        nL, nM, B, flat, costOff, probOff, psizes, probs = _pack_frames(costs, nL, nM, "permanent_probs")
        perm = np.zeros(B, np.float64)
        self._check(self.lib.kbest_permanent_probs_batch_f64(self.ctx, B, _ptr(nL), _ptr(nM), _ptr(flat), _ptr(costOff),
                                                             int(bool(condition)), _ptr(probs), _ptr(probOff), _ptr(perm)))
        out = _split_probs(probs, probOff, psizes, nL, nM)
        return out, perm

    def set_permanent_work_cap(self, nbytes=0):
        """Diagnostic (kbest_set_permanent_work_cap): cap of the permanent work space in bytes, 0 = the default; a lower cap means
        fewer frames in flight and the same results."""
        self._check(self.lib.kbest_set_permanent_work_cap(self.ctx, int(nbytes)))

    def last_permanent_grid(self):
        """Diagnostic (kbest_last_permanent_grid): workgroups -- frames in flight -- of this context's last permanent launch."""
        return int(self.lib.kbest_last_permanent_grid(self.ctx))

    def sample_assoc(self, costs, nL, nM, n_sample, seed=0, condition=False, frame_key=None, sample_base=0):
        """Joint associations drawn from the exact posterior, nM <= 16 (kbest_sample.hip): n_sample independent draws per frame.
        Packing and condition as permanent_probs().  frame_key: one uint64 per frame (None: the frame's index) -- with it a frame's
        draws do not depend on the batch; sample_base: the index of the first draw.  Returns (list of int32 [n_sample, nM] arrays:
        the raw row of the frame's block every measurement takes, a row >= nL is a miss; list of logProb [n_sample] arrays; perm[B]).
        A frame whose permanent is 0 has assign -1 and logProb NaN."""
        nL, nM, B, flat, costOff, _, _, _ = _pack_frames(costs, nL, nM, "sample_assoc")
        n_sample, asgOff, lpOff, assign, logp, key = _pack_draws(nM, B, n_sample, frame_key, "sample_assoc")
        perm = np.zeros(B, np.float64)
        self._check(self.lib.kbest_sample_assoc_batch_f64(self.ctx, B, _ptr(nL), _ptr(nM), _ptr(flat), _ptr(costOff), int(bool(condition)),
                                                          n_sample, int(seed), int(sample_base), _ptr(key), _ptr(assign), _ptr(asgOff),
                                                          _ptr(logp), _ptr(lpOff), _ptr(perm)))
        return (*_split_draws(assign, asgOff, logp, lpOff, nM, n_sample), perm)

    def belief_probs(self, costs, nL, nM, condition=False, tol=1e-12, max_iter=10000):
        """Batched beliefProb (kbest_lbp.hip): the association probabilities by loopy belief propagation, nM <= 128 and
        nL + nM <= 1024.  Packing and condition as permanent_probs().  Stops after the sweep whose resid <= tol or after max_iter
        sweeps (tol <= 0: exactly max_iter).  Returns (list of [nM, nL+1] arrays, iters[B]: sweeps run, -2 for an infeasible frame
        (all zeros), resid[B]: the last sweep's max |nu' - nu|)."""
        nL, nM, B, flat, costOff, probOff, psizes, probs = _pack_frames(costs, nL, nM, "belief_probs")
        iters = np.zeros(B, np.int32)
        resid = np.zeros(B, np.float64)
        self._check(self.lib.kbest_belief_probs_batch_f64(self.ctx, B, _ptr(nL), _ptr(nM), _ptr(flat), _ptr(costOff),
                                                          int(bool(condition)), float(tol), int(max_iter), _ptr(probs),
                                                          _ptr(probOff), _ptr(iters), _ptr(resid)))
        out = _split_probs(probs, probOff, psizes, nL, nM)
        return out, iters, resid

    def set_belief_lds_limit(self, nbytes=0):
        """Diagnostic (kbest_set_belief_lds_limit): LDS bytes the belief-propagation launches may plan with, 0 = the device's limit;
        a low value keeps a and nu of small frames in the HBM work space -- the same results."""
        self._check(self.lib.kbest_set_belief_lds_limit(self.ctx, int(nbytes)))

    def clustered_probs(self, costs, nL, nM, condition=False, labels=False):
        """Batched clusterProb (kbest_cluster.hip): the EXACT association probabilities by gated clusters, nM <= 128 and
        nL + nM <= 1024, clusters of at most 16 measurements.  Packing and condition as permanent_probs().  Returns (list of
        [nM, nL+1] arrays, logPerm[B]: the sum of log Z_k over the clusters (-inf: infeasible, NaN: refused), info[B]: the number of
        clusters, 0 for an infeasible frame, -2 / -3 for a refused one (all zeros), maxCluster[B]: measurements of the largest
        cluster) and, with labels=True, label[B, max nM]: the lowest column of every column's cluster, -1 beyond the frame's nM."""
        nL, nM, B, flat, costOff, probOff, psizes, probs = _pack_frames(costs, nL, nM, "clustered_probs")
        logPerm = np.zeros(B, np.float64)
        info = np.zeros(B, np.int32)
        maxCluster = np.zeros(B, np.int32)
        stride = int(nM.max()) if B else 1
        lab = np.full((B, stride), -1, np.int32) if labels else None
        self._check(self.lib.kbest_clustered_probs_batch_f64(self.ctx, B, _ptr(nL), _ptr(nM), _ptr(flat), _ptr(costOff),
                                                             int(bool(condition)), _ptr(probs), _ptr(probOff), _ptr(logPerm),
                                                             _ptr(info), _ptr(maxCluster), _ptr(lab), stride))
        out = _split_probs(probs, probOff, psizes, nL, nM)
        return (out, logPerm, info, maxCluster, lab) if labels else (out, logPerm, info, maxCluster)

    def clustered_sample_assoc(self, costs, nL, nM, n_sample, seed=0, condition=False, frame_key=None, sample_base=0):
        """Joint associations drawn from the exact posterior by gated clusters (kbest_cluster_sample.hip): sample_assoc() for the
        frames clustered_probs() takes -- nM <= 128, nL + nM <= 1024, clusters of at most 16 measurements; on a frame sample_assoc()
        takes, the same draws.  Packing, condition, frame_key and sample_base as sample_assoc().  Returns (list of int32
        [n_sample, nM] arrays: the raw row of the frame's block every measurement takes, a row >= nL is a miss; list of logProb
        [n_sample] arrays; logPerm[B], info[B], maxCluster[B] as clustered_probs()).  A refused (info -2 / -3) or infeasible
        (info 0) frame has assign -1 and logProb NaN."""
        nL, nM, B, flat, costOff, _, _, _ = _pack_frames(costs, nL, nM, "clustered_sample_assoc")
        n_sample, asgOff, lpOff, assign, logp, key = _pack_draws(nM, B, n_sample, frame_key, "clustered_sample_assoc")
        logPerm = np.zeros(B, np.float64)
        info = np.zeros(B, np.int32)
        maxCluster = np.zeros(B, np.int32)
        self._check(self.lib.kbest_clustered_sample_assoc_batch_f64(self.ctx, B, _ptr(nL), _ptr(nM), _ptr(flat), _ptr(costOff),
                                                                    int(bool(condition)), n_sample, int(seed), int(sample_base),
                                                                    _ptr(key), _ptr(assign), _ptr(asgOff), _ptr(logp), _ptr(lpOff),
                                                                    _ptr(logPerm), _ptr(info), _ptr(maxCluster)))
        return (*_split_draws(assign, asgOff, logp, lpOff, nM, n_sample), logPerm, info, maxCluster)

    def exact_or_belief_probs(self, costs, nL, nM, condition=False, tol=1e-12, max_iter=10000):
        """The exact probabilities wherever the gate leaves clusters of at most 16 measurements, belief propagation elsewhere:
        clustered_probs() once, then belief_probs() on the refused frames only.  Returns (list of [nM, nL+1] arrays, method[B]:
        0 exact, 1 belief propagation, -2 infeasible (all zeros)).  hybrid_probs() is the better answer for the refused frames:
        it keeps every cluster it can take exact and spends a k-best enumeration on the oversized one alone."""
        out, _, info, _ = self.clustered_probs(costs, nL, nM, condition=condition)
        method = np.where(info > 0, 0, np.where(info == 0, -2, 1)).astype(np.int32)
        refused = [b for b in range(len(info)) if info[b] < 0]
        if refused:
            bp, iters, _ = self.belief_probs([costs[b] for b in refused], [int(nL[b]) for b in refused],
                                             [int(nM[b]) for b in refused], condition=condition, tol=tol, max_iter=max_iter)
            for j, b in enumerate(refused):
                out[b] = bp[j]
                if iters[j] == -2:
                    method[b] = -2
        return out, method

    def hybrid_probs(self, costs, nL, nM, k, condition=False, max_exact=16):
        """Batched hybridProb (kbest_hybrid_probs_batch_f64): exact on every gated cluster of at most max_exact (1 .. 16, 0 = 16)
        measurements, assignmentProb(k) -- kBest2DCutoff(k, 42) -> weights -- on each larger cluster alone; nM <= 128 and
        nL + nM <= 1024.  Packing and condition as permanent_probs().  Returns (list of [nM, nL+1] arrays, method[B]: 0 every
        cluster exact (the bits of clustered_probs), 1 some clusters enumerated and every enumeration ended before k, 2 some
        enumeration cut at k, -2 infeasible (all zeros), -1 refused (all zeros), nOpen[B]: clusters enumerated, maxCluster[B])."""
        nL, nM, B, flat, costOff, probOff, psizes, probs = _pack_frames(costs, nL, nM, "hybrid_probs")
        method = np.zeros(B, np.int32)
        nOpen = np.zeros(B, np.int32)
        maxCluster = np.zeros(B, np.int32)
        self._check(self.lib.kbest_hybrid_probs_batch_f64(self.ctx, B, _ptr(nL), _ptr(nM), _ptr(flat), _ptr(costOff),
                                                          int(bool(condition)), int(k), int(max_exact), _ptr(probs), _ptr(probOff),
                                                          _ptr(method), _ptr(nOpen), _ptr(maxCluster)))
        out = _split_probs(probs, probOff, psizes, nL, nM)
        return out, method, nOpen, maxCluster

    def hybrid_exact_probs(self, costs, nL, nM, k=0, condition=False, max_exact=16, max_big=20):
        """Batched hybridExactProb (kbest_hybrid_exact_probs_batch_f64): hybrid_probs() with the big-cluster tier between its two --
        every cluster of more than max_exact and at most max_big (0 .. 20) measurements whose layers fit the work cap is answered
        EXACTLY, one cluster over the whole chip; what is still open goes through assignmentProb(k) when k >= 1 and refuses its
        frame when k = 0.  Returns (list of [nM, nL+1] arrays, method[B]: 0 every cluster exact, 1 / 2 some cluster enumerated
        (complete / cut at k), -2 infeasible (all zeros), -1 refused (all zeros), nOpen[B]: clusters beyond max_exact, nBig[B]: those
        of them answered exactly, maxCluster[B], logPerm[B]: the sum of log Z_k over the exactly answered clusters)."""
        nL, nM, B, flat, costOff, probOff, psizes, probs = _pack_frames(costs, nL, nM, "hybrid_exact_probs")
        method = np.zeros(B, np.int32)
        nOpen = np.zeros(B, np.int32)
        nBig = np.zeros(B, np.int32)
        maxCluster = np.zeros(B, np.int32)
        logPerm = np.zeros(B, np.float64)
        self._check(self.lib.kbest_hybrid_exact_probs_batch_f64(self.ctx, B, _ptr(nL), _ptr(nM), _ptr(flat), _ptr(costOff),
                                                                int(bool(condition)), int(k), int(max_exact), int(max_big),
                                                                _ptr(probs), _ptr(probOff), _ptr(logPerm), _ptr(method), _ptr(nOpen),
                                                                _ptr(nBig), _ptr(maxCluster)))
        out = _split_probs(probs, probOff, psizes, nL, nM)
        return out, method, nOpen, nBig, maxCluster, logPerm

    def reserve_bigcluster(self, maxM, maxRows):
        """kbest_reserve_bigcluster: the work space of bigcluster_probs_dev for clusters of up to maxM measurements and maxRows
        (nL_k + m_k) rows."""
        self._check(self.lib.kbest_reserve_bigcluster(self.ctx, int(maxM), int(maxRows)))

    def set_bigcluster_work_cap(self, nbytes=0):
        """For tests (kbest_set_bigcluster_work_cap): the layers of the big clusters in flight at the most, 0 = the default again."""
        self._check(self.lib.kbest_set_bigcluster_work_cap(self.ctx, int(nbytes)))

    def bigcluster_probs_dev(self, m, nLk, subOff, probOff, d_sub, d_probs, d_logZ=None, d_info=None, stream=None, reserve=True):
        """kbest_bigcluster_probs_f64_dev, asynchronous on `stream`: m, nLk, subOff, probOff are HOST sequences (one entry per
        cluster), d_sub / d_probs / d_logZ / d_info torch CUDA tensors: cluster k is the (nLk + m) x m column-major block at
        d_sub[subOff[k]:] (the format the partial clustered kernel hands out) and gets [m][nLk + 1] probabilities at
        d_probs[probOff[k]:], log Z_k and info (1 answered, 0 no complete assignment, -5 declined: Z' below 2^-970 although there is
        one, -3 beyond the work cap; after -5 and -3 the outputs are untouched)."""
        m = np.ascontiguousarray(m, dtype=np.int32)
        nLk = np.ascontiguousarray(nLk, dtype=np.int32)
        subOff = np.ascontiguousarray(subOff, dtype=np.int64)
        probOff = np.ascontiguousarray(probOff, dtype=np.int64)
        if reserve and len(m):
            self.reserve_bigcluster(int(m.max()), int((m + nLk).max()))
        self._check(self.lib.kbest_bigcluster_probs_f64_dev(self.ctx, len(m), _ptr(m), _ptr(nLk), _ptr(subOff), _ptr(probOff),
                                                            _dptr(d_sub), _dptr(d_probs), _dptr(d_logZ), _dptr(d_info),
                                                            _stream(stream)))

    def hybrid_frontier_probs(self, costs, nL, nM, k=0, condition=False, max_exact=16, max_big=20, max_width=16):
        """Batched hybridFrontierProb (kbest_hybrid_frontier_probs_batch_f64): hybrid_exact_probs() with the frontier tier first
        among the open clusters -- every cluster of more than max_exact and at most 64 measurements whose rows, in the greedy
        order, keep at most max_width (0 .. 16; 0: the tier is off) columns open is answered EXACTLY, one workgroup per cluster in
        one launch; what the tier refuses goes to the big-cluster tier (at most max_big measurements), then to assignmentProb(k)
        when k >= 1, and refuses its frame when k = 0.  Returns (list of [nM, nL+1] arrays, method[B], nOpen[B], nBig[B],
        maxCluster[B], logPerm[B] as hybrid_exact_probs(), nFrontier[B]: the open clusters this tier answered)."""
        nL, nM, B, flat, costOff, probOff, psizes, probs = _pack_frames(costs, nL, nM, "hybrid_frontier_probs")
        method = np.zeros(B, np.int32)
        nOpen = np.zeros(B, np.int32)
        nBig = np.zeros(B, np.int32)
        nFrontier = np.zeros(B, np.int32)
        maxCluster = np.zeros(B, np.int32)
        logPerm = np.zeros(B, np.float64)
        self._check(self.lib.kbest_hybrid_frontier_probs_batch_f64(self.ctx, B, _ptr(nL), _ptr(nM), _ptr(flat), _ptr(costOff),
                                                                   int(bool(condition)), int(k), int(max_exact), int(max_big),
                                                                   int(max_width), _ptr(probs), _ptr(probOff), _ptr(logPerm),
                                                                   _ptr(method), _ptr(nOpen), _ptr(nBig), _ptr(maxCluster),
                                                                   _ptr(nFrontier)))
        out = _split_probs(probs, probOff, psizes, nL, nM)
        return out, method, nOpen, nBig, maxCluster, logPerm, nFrontier

    def reserve_frontier(self, n, maxM, maxRows):
        """kbest_reserve_frontier: the work space of frontier_probs_dev for n clusters of up to maxM measurements and maxRows
        (nL_k + m_k) rows."""
        self._check(self.lib.kbest_reserve_frontier(self.ctx, int(n), int(maxM), int(maxRows)))

    def set_frontier_work_cap(self, nbytes=0):
        """For tests (kbest_set_frontier_work_cap): the slots of the frontier tier in flight at the most, 0 = the default again."""
        self._check(self.lib.kbest_set_frontier_work_cap(self.ctx, int(nbytes)))

    def set_frontier_slot(self, nbytes=0):
        """For tests (kbest_set_frontier_slot): the layers of one cluster of the frontier tier at the most, 0 = KBEST_FRONTIER_SLOT
        again; a cluster that needs more is refused (info = -3)."""
        self._check(self.lib.kbest_set_frontier_slot(self.ctx, int(nbytes)))

    def frontier_probs_dev(self, m, nLk, subOff, probOff, d_sub, d_probs, d_logZ=None, d_info=None, d_width=None, stream=None,
                           reserve=True):
        """kbest_frontier_probs_f64_dev, asynchronous on `stream`: arguments as bigcluster_probs_dev() with up to 64 measurements a
        cluster, plus d_width (the cluster's frontier width W).  info: 1 answered, 0 no complete assignment, -5 declined (Z' below
        2^-970 although there is one), -4 W > 16, -3 layers beyond the slot (refused: probabilities and log Z untouched)."""
        m = np.ascontiguousarray(m, dtype=np.int32)
        nLk = np.ascontiguousarray(nLk, dtype=np.int32)
        subOff = np.ascontiguousarray(subOff, dtype=np.int64)
        probOff = np.ascontiguousarray(probOff, dtype=np.int64)
        if reserve and len(m):
            self.reserve_frontier(len(m), int(m.max()), int((m + nLk).max()))
        self._check(self.lib.kbest_frontier_probs_f64_dev(self.ctx, len(m), _ptr(m), _ptr(nLk), _ptr(subOff), _ptr(probOff),
                                                          _dptr(d_sub), _dptr(d_probs), _dptr(d_logZ), _dptr(d_info),
                                                          _dptr(d_width), _stream(stream)))

    def hybrid_frontier_sample_assoc(self, costs, nL, nM, n_sample, seed=0, condition=False, frame_key=None, sample_base=0,
                                     max_exact=16, max_width=16):
        """kbest_hybrid_frontier_sample_assoc_batch_f64: clustered_sample_assoc() for the frames hybrid_frontier_probs(k=0, max_big=0)
        answers -- the clusters of at most max_exact measurements by the clustered sampler's walk (the same draws), every larger one
        of at most 64 measurements and a frontier width of at most max_width by a backward walk over the frontier tier's layers.
        Returns (list of int32 [n_sample, nM] arrays: the raw row every measurement takes, list of logProb [n_sample], logPerm[B],
        method[B]: 0 drawn, -1 refused (assign -1, logProb NaN), -2 infeasible (likewise), nOpen[B], nFrontier[B], maxCluster[B])."""
        nL, nM, B, flat, costOff, _, _, _ = _pack_frames(costs, nL, nM, "hybrid_frontier_sample_assoc")
        n_sample, asgOff, lpOff, assign, logp, key = _pack_draws(nM, B, n_sample, frame_key, "hybrid_frontier_sample_assoc")
        logPerm = np.zeros(B, np.float64)
        method, nOpen, nFrontier, maxCluster = (np.zeros(B, np.int32) for _ in range(4))
        self._check(self.lib.kbest_hybrid_frontier_sample_assoc_batch_f64(
            self.ctx, B, _ptr(nL), _ptr(nM), _ptr(flat), _ptr(costOff), int(bool(condition)), int(max_exact), int(max_width), n_sample,
            int(seed), int(sample_base), _ptr(key), _ptr(assign), _ptr(asgOff), _ptr(logp), _ptr(lpOff), _ptr(logPerm), _ptr(method),
            _ptr(nOpen), _ptr(nFrontier), _ptr(maxCluster)))
        return (*_split_draws(assign, asgOff, logp, lpOff, nM, n_sample), logPerm, method, nOpen, nFrontier, maxCluster)

    def hybrid_sample_assoc(self, costs, nL, nM, n_sample, k, seed=0, condition=False, frame_key=None, sample_base=0, max_exact=16,
                            max_width=16):
        """kbest_hybrid_sample_assoc_batch_f64: hybrid_frontier_sample_assoc() for EVERY gated frame -- with k >= 1 an open cluster
        the frontier sampler does not take is enumerated (kBest2DCutoff(k, 42) on its sub-block) and drawn from its table under
        assignmentProb's weights, instead of refusing the frame; k = 0 is hybrid_frontier_sample_assoc() bit for bit.  Returns
        (list of int32 [n_sample, nM] arrays: the raw row every measurement takes, list of logProb [n_sample], logPerm[B] (the exactly
        answered clusters only), method[B]: 0 all exact, 1 every enumeration complete, 2 some cut at k, -1 refused, -2 infeasible
        (assign -1, logProb NaN), nOpen[B], nFrontier[B], nEnum[B], maxCluster[B])."""
        nL, nM, B, flat, costOff, _, _, _ = _pack_frames(costs, nL, nM, "hybrid_sample_assoc")
        n_sample, asgOff, lpOff, assign, logp, key = _pack_draws(nM, B, n_sample, frame_key, "hybrid_sample_assoc")
        logPerm = np.zeros(B, np.float64)
        method, nOpen, nFrontier, nEnum, maxCluster = (np.zeros(B, np.int32) for _ in range(5))
        self._check(self.lib.kbest_hybrid_sample_assoc_batch_f64(
            self.ctx, B, _ptr(nL), _ptr(nM), _ptr(flat), _ptr(costOff), int(bool(condition)), int(k), int(max_exact), int(max_width),
            n_sample, int(seed), int(sample_base), _ptr(key), _ptr(assign), _ptr(asgOff), _ptr(logp), _ptr(lpOff), _ptr(logPerm),
            _ptr(method), _ptr(nOpen), _ptr(nFrontier), _ptr(nEnum), _ptr(maxCluster)))
        return (*_split_draws(assign, asgOff, logp, lpOff, nM, n_sample), logPerm, method, nOpen, nFrontier, nEnum, maxCluster)

    def table_sample_dev(self, k, maxCol, m, d_row4col, d_gain, d_nf, n_sample, d_assignLocal, asgOff, d_logTerm, ltOff, d_pick=None,
                         d_info=None, cutoff=42.0, cluster_key=None, frame_key=None, seed=0, sample_base=0, stream=None):
        """kbest_table_sample_f64_dev, asynchronous on `stream`: n_sample joint associations of every problem, drawn from its table
        of k best assignments (d_row4col [n][k][maxCol] int32, d_gain [n][k], d_nf [n]: what kbest_batch_f64_dev writes) under
        the weights w_j = exp(gain_0 - gain_j) within the cutoff.  m[i] (host) the columns of problem i; cluster_key[i] < 2^30 and
        frame_key[i] (host, None: 0) the generator's keys.  Out: d_assignLocal at asgOff[i] [n_sample][m_i] = the picked slot's
        rows, d_logTerm at ltOff[i] [n_sample], d_pick (optional) [n][n_sample] the slot.  info 1 drawn, 0 nothing to draw from
        (-1, NaN, -1), -1 m outside 1 .. maxCol (untouched)."""
        m = np.ascontiguousarray(m, dtype=np.int32)
        asgOff = np.ascontiguousarray(asgOff, dtype=np.int64)
        ltOff = np.ascontiguousarray(ltOff, dtype=np.int64)
        ck = None if cluster_key is None else np.ascontiguousarray(cluster_key, dtype=np.uint32)
        fk = None if frame_key is None else np.ascontiguousarray(frame_key, dtype=np.uint64)
        if (ck is not None and len(ck) != len(m)) or (fk is not None and len(fk) != len(m)) or len(asgOff) != len(m) or len(ltOff) != len(m):
            raise ValueError("table_sample_dev: one key and one offset per problem")
        self._check(self.lib.kbest_table_sample_f64_dev(self.ctx, len(m), int(k), int(maxCol), _ptr(m), _dptr(d_row4col), _dptr(d_gain),
                                                        _dptr(d_nf), float(cutoff), _ptr(ck), _ptr(fk), int(n_sample), int(seed),
                                                        int(sample_base), _dptr(d_assignLocal), _ptr(asgOff), _dptr(d_logTerm),
                                                        _ptr(ltOff), _dptr(d_pick), _dptr(d_info), _stream(stream)))

    def reserve_frontier_sample(self, n, maxM, maxRows):
        """kbest_reserve_frontier_sample: the work space of frontier_sample_dev -- exactly what reserve_frontier() reserves."""
        self._check(self.lib.kbest_reserve_frontier_sample(self.ctx, int(n), int(maxM), int(maxRows)))

    def frontier_sample_dev(self, m, nLk, subOff, d_sub, d_rowKey, rowKeyOff, n_sample, d_assignLocal, asgOff, d_logTerm, ltOff,
                            d_logZ=None, d_info=None, d_width=None, seed=0, sample_base=0, frame_key=None, stream=None, reserve=True):
        """kbest_frontier_sample_f64_dev, asynchronous on `stream`: n_sample joint associations of every cluster, drawn from its
        exact posterior by a backward walk over the frontier tier's forward layers.  m, nLk, subOff, d_sub, d_logZ, d_info and
        d_width as frontier_probs_dev() (and with its bits); d_rowKey (int32, device) at rowKeyOff[k] the key q of every row of
        the cluster's sub-block, frame_key[k] (host, None: 0) the key of its frame.  Out: d_assignLocal at asgOff[k]
        [n_sample][m_k] the row of the sub-block every column takes, d_logTerm at ltOff[k] [n_sample] the draw's log-probability
        inside the cluster.  info 0: -1 and NaN; a refused cluster (-3, -4): untouched."""
        m = np.ascontiguousarray(m, dtype=np.int32)
        nLk = np.ascontiguousarray(nLk, dtype=np.int32)
        subOff = np.ascontiguousarray(subOff, dtype=np.int64)
        rowKeyOff = np.ascontiguousarray(rowKeyOff, dtype=np.int64)
        asgOff = np.ascontiguousarray(asgOff, dtype=np.int64)
        ltOff = np.ascontiguousarray(ltOff, dtype=np.int64)
        fk = None if frame_key is None else np.ascontiguousarray(frame_key, dtype=np.uint64)
        if fk is not None and len(fk) != len(m):
            raise ValueError("frontier_sample_dev: one frame key per cluster")
        if reserve and len(m):
            self.reserve_frontier_sample(len(m), int(m.max()), int((m + nLk).max()))
        self._check(self.lib.kbest_frontier_sample_f64_dev(self.ctx, len(m), _ptr(m), _ptr(nLk), _ptr(subOff), _dptr(d_sub),
                                                           _dptr(d_rowKey), _ptr(rowKeyOff), None if fk is None else _ptr(fk),
                                                           int(n_sample), int(seed), int(sample_base), _dptr(d_assignLocal),
                                                           _ptr(asgOff), _dptr(d_logTerm), _ptr(ltOff), _dptr(d_logZ), _dptr(d_info),
                                                           _dptr(d_width), _stream(stream)))

    def set_clustered_slot_cap(self, nbytes=0):
        """For tests (kbest_set_clustered_slot_cap): the layers of one cluster at the most, 0 = KBEST_CLUSTER_SLOT_CAP again; a frame
        with a cluster that needs more is refused (info = -3)."""
        self._check(self.lib.kbest_set_clustered_slot_cap(self.ctx, int(nbytes)))

    def set_clustered_work_cap(self, nbytes=0):
        """For tests (kbest_set_clustered_work_cap): cap of the clustered kernel's work space, 0 = KBEST_CLUSTER_WORK_CAP again."""
        self._check(self.lib.kbest_set_clustered_work_cap(self.ctx, int(nbytes)))

    def last_clustered_grid(self):
        """Diagnostic (kbest_last_clustered_grid): workgroups -- frames in flight -- of this context's last clustered launch."""
        return int(self.lib.kbest_last_clustered_grid(self.ctx))

    @staticmethod
    def _pack_quadrics(frames):
        """frames: list of (landMean (nL,3), landCov (nL,3,3), measMean (nM,3), measCov (nM,3,3))."""
        nL = np.array([len(f[0]) for f in frames], np.int32)
        nM = np.array([len(f[2]) for f in frames], np.int32)
        cat = lambda i, w: np.ascontiguousarray(np.concatenate([np.asarray(f[i], np.float64).reshape(-1, w) for f in frames]))  # noqa: E731
        return nL, nM, cat(0, 3), cat(1, 9), cat(2, 3), cat(3, 9)

    def quadric_costs(self, frames, gate):
        """Batched computeQuadricCostMatrix.  Returns a list of (nL+nM)*nM column-major blocks."""
        nL, nM, lm, lc, mm, mc = self._pack_quadrics(frames)
        sizes = (nL.astype(np.int64) + nM) * nM
        out = np.zeros(int(sizes.sum()))
        self._check(self.lib.kbest_quadric_costs_f64(self.ctx, len(frames), _ptr(nL), _ptr(nM), _ptr(lm), _ptr(lc), _ptr(mm),
                                                     _ptr(mc), float(gate), _ptr(out)))
        off = np.concatenate([[0], np.cumsum(sizes)])
        return [out[off[b]: off[b + 1]] for b in range(len(frames))]

    def quadric_assoc_probs(self, frames, gate, k):
        """getAssignmentProbs from (mean, covariance) pairs: list of [nM, nL+1] arrays, nf."""
        nL, nM, lm, lc, mm, mc = self._pack_quadrics(frames)
        psizes = nM.astype(np.int64) * (nL + 1)
        poff = np.zeros(len(frames), np.int64)
        poff[1:] = np.cumsum(psizes)[:-1]
        probs = np.zeros(int(psizes.sum()))
        nf = np.zeros(len(frames), np.int32)
        self._check(self.lib.kbest_quadric_assoc_probs_batch_f64(self.ctx, len(frames), _ptr(nL), _ptr(nM), _ptr(lm), _ptr(lc),
                                                                 _ptr(mm), _ptr(mc), float(gate), k, _ptr(probs), _ptr(poff),
                                                                 _ptr(nf)))
        return [probs[poff[b]: poff[b] + psizes[b]].reshape(int(nM[b]), int(nL[b]) + 1) for b in range(len(frames))], nf

    def quadric_map_probs(self, map_mean, map_cov, frames, gate, k=0, max_exact=16, max_big=20, max_width=16):
        """getAssignmentProbs' exact branch from quadrics against one map of any size (kbest_quadric_map_probs_batch_f64).
        map_mean (nMap, 3), map_cov (nMap, 3, 3); frames: list of (landOff, nL, measMean (nM, 3), measCov (nM, 3, 3)) -- frame b
        sees landmarks landOff .. landOff + nL of the map.  The cost builder conditions while it builds (the raw block is never
        formed); the compact blocks go through the one-stream exact path, and what that refuses through
        hybrid_frontier_probs(k, max_big, condition=False) when k >= 1 or max_big > 0.  Returns (list of dense [nM, nL+1] arrays,
        method[B], nKeep[B]: landmark rows conditionCosts keeps, nOpen[B], nBig[B], nFrontier[B], maxCluster[B], logPerm[B])."""
        B = len(frames)
        mm = np.ascontiguousarray(np.asarray(map_mean, np.float64).reshape(-1, 3))
        mc = np.ascontiguousarray(np.asarray(map_cov, np.float64).reshape(-1, 9))
        if len(mm) != len(mc):
            raise KBestError("quadric_map_probs: map_mean and map_cov differ in length")
        landOff = np.array([f[0] for f in frames], np.int64)
        nL = np.array([f[1] for f in frames], np.int32)
        nM = np.array([len(f[2]) for f in frames], np.int32)
        cat = lambda i, w: np.ascontiguousarray(np.concatenate([np.zeros((0, w))] + [np.asarray(f[i], np.float64).reshape(-1, w) for f in frames]))  # noqa: E731
        zm, zc = cat(2, 3), cat(3, 9)
        psizes = nM.astype(np.int64) * (nL.astype(np.int64) + 1)
        probOff = np.zeros(B, np.int64)
        probOff[1:] = np.cumsum(psizes)[:-1]
        probs = np.zeros(int(psizes.sum()), np.float64)
        ints = np.zeros((6, max(B, 1)), np.int32)  # method | nKeep | nOpen | nBig | nFrontier | maxCluster
        logPerm = np.zeros(max(B, 1), np.float64)
        self._check(self.lib.kbest_quadric_map_probs_batch_f64(
            self.ctx, B, len(mm), _ptr(mm), _ptr(mc), _ptr(landOff), _ptr(nL), _ptr(nM), _ptr(zm), _ptr(zc), float(gate), int(k),
            int(max_exact), int(max_big), int(max_width), _ptr(probs), _ptr(probOff), _ptr(logPerm), _ptr(ints[0]), _ptr(ints[1]),
            _ptr(ints[2]), _ptr(ints[3]), _ptr(ints[4]), _ptr(ints[5])))
        out = _split_probs(probs, probOff, psizes, nL, nM)
        return (out,) + tuple(ints[i, :B].copy() for i in range(6)) + (logPerm[:B].copy(),)

    def reserve_quadric_map_dev(self, B, maxMap, maxKeep, maxCol):
        """kbest_reserve_quadric_map_dev: everything quadric_map_probs_dev needs besides the caller's buffers, sized from the four
        numbers alone (a reservation never shrinks)."""
        self._check(self.lib.kbest_reserve_quadric_map_dev(self.ctx, int(B), int(maxMap), int(maxKeep), int(maxCol)))

    def quadric_map_probs_dev(self, B, maxMap, maxKeep, maxCol, d_mapMean, d_mapCov, d_landOff, d_nL, d_measMean, d_measCov, d_measOff,
                              d_nM, gate, d_nKeep, d_rowIdx, d_cprobs, d_method, d_ccost=None, d_probs=None, d_probOff=None,
                              d_logPerm=None, d_nOpen=None, d_nFrontier=None, d_maxCluster=None, max_exact=16, max_width=16,
                              stream=None, reserve=True):
        """kbest_quadric_map_probs_batch_f64_dev on torch CUDA tensors (or raw addresses), asynchronous on `stream` (a raw
        hipStream_t integer): from quadrics against one resident map to the exact probabilities without a host read, a synchronise
        or an allocation.  d_landOff, d_measOff, d_probOff int64 [B]; d_nL, d_nM int32 [B]; d_nKeep int32 [B]; d_rowIdx int32
        [B][maxKeep]; d_ccost (None: the context's) frame b's compact block at b (maxKeep + maxCol) maxCol; d_cprobs frame b's
        [nM][nKeep + 1] at b maxCol (maxKeep + 1); d_probs (None: not expanded) the dense [nM][nL + 1] slices at d_probOff.
        reserve=False: the caller has called reserve_quadric_map_dev (timed loops, graph capture; the C entry never allocates)."""
        if reserve:
            self.reserve_quadric_map_dev(B, maxMap, maxKeep, maxCol)
        self._check(self.lib.kbest_quadric_map_probs_batch_f64_dev(
            self.ctx, int(B), int(maxMap), int(maxKeep), int(maxCol), _dptr(d_mapMean), _dptr(d_mapCov), _dptr(d_landOff), _dptr(d_nL),
            _dptr(d_measMean), _dptr(d_measCov), _dptr(d_measOff), _dptr(d_nM), float(gate), int(max_exact), int(max_width),
            _dptr(d_nKeep), _dptr(d_rowIdx), _dptr(d_ccost), _dptr(d_cprobs), _dptr(d_probs), _dptr(d_probOff), _dptr(d_logPerm),
            _dptr(d_method), _dptr(d_nOpen), _dptr(d_nFrontier), _dptr(d_maxCluster), _stream(stream)))

    def quadric_map_sample_assoc(self, map_mean, map_cov, frames, gate, n_sample, k=0, seed=0, frame_key=None, sample_base=0,
                                 max_exact=16, max_width=16):
        """kbest_quadric_map_sample_assoc_batch_f64: n_sample joint associations a frame, drawn from the exact posterior whose
        marginals quadric_map_probs() returns -- map and frames as there.  The compact blocks go through the one-stream sampler, and
        with k >= 1 what that refuses because of an open cluster through hybrid_sample_assoc(k, condition=False).  Returns (list of
        int32 [n_sample, nM] arrays: the row of the notional raw (nL + nM) x nM block every measurement takes -- a landmark of the
        frame's window, or nL + c for the miss of measurement c --, list of logProb [n_sample], logPerm[B], method[B]: 0 all exact,
        1 / 2 enumerated, -1 refused, -2 infeasible (assign -1, logProb NaN), nKeep[B], nOpen[B], nFrontier[B], nEnum[B],
        maxCluster[B])."""
        B = len(frames)
        mm = np.ascontiguousarray(np.asarray(map_mean, np.float64).reshape(-1, 3))
        mc = np.ascontiguousarray(np.asarray(map_cov, np.float64).reshape(-1, 9))
        if len(mm) != len(mc):
            raise KBestError("quadric_map_sample_assoc: map_mean and map_cov differ in length")
        landOff = np.array([f[0] for f in frames], np.int64)
        nL = np.array([f[1] for f in frames], np.int32)
        nM = np.array([len(f[2]) for f in frames], np.int32)
        cat = lambda i, w: np.ascontiguousarray(np.concatenate([np.zeros((0, w))] + [np.asarray(f[i], np.float64).reshape(-1, w) for f in frames]))  # noqa: E731
        zm, zc = cat(2, 3), cat(3, 9)
        n_sample, asgOff, lpOff, assign, logp, key = _pack_draws(nM, B, n_sample, frame_key, "quadric_map_sample_assoc")
        ints = np.zeros((6, max(B, 1)), np.int32)  # method | nKeep | nOpen | nFrontier | nEnum | maxCluster
        logPerm = np.zeros(max(B, 1), np.float64)
        self._check(self.lib.kbest_quadric_map_sample_assoc_batch_f64(
            self.ctx, B, len(mm), _ptr(mm), _ptr(mc), _ptr(landOff), _ptr(nL), _ptr(nM), _ptr(zm), _ptr(zc), float(gate), int(k),
            int(max_exact), int(max_width), n_sample, int(seed), int(sample_base), _ptr(key), _ptr(assign), _ptr(asgOff), _ptr(logp),
            _ptr(lpOff), _ptr(logPerm), _ptr(ints[0]), _ptr(ints[1]), _ptr(ints[2]), _ptr(ints[3]), _ptr(ints[4]), _ptr(ints[5])))
        return (*_split_draws(assign, asgOff, logp, lpOff, nM, n_sample), logPerm[:B].copy()) + tuple(ints[i, :B].copy() for i in range(6))

    def reserve_quadric_map_sample_dev(self, B, maxMap, maxKeep, maxCol, n_sample):
        """kbest_reserve_quadric_map_sample_dev: everything quadric_map_sample_assoc_dev needs besides the caller's buffers, sized
        from the five numbers alone (a reservation never shrinks)."""
        self._check(self.lib.kbest_reserve_quadric_map_sample_dev(self.ctx, int(B), int(maxMap), int(maxKeep), int(maxCol), int(n_sample)))

    def quadric_map_sample_assoc_dev(self, B, maxMap, maxKeep, maxCol, d_mapMean, d_mapCov, d_landOff, d_nL, d_measMean, d_measCov,
                                     d_measOff, d_nM, gate, n_sample, d_nKeep, d_rowIdx, d_assign, d_asgOff, d_logProb, d_lpOff, d_method,
                                     d_ccost=None, d_logPerm=None, d_nOpen=None, d_nFrontier=None, d_maxCluster=None, seed=0,
                                     sample_base=0, d_frameKey=None, max_exact=16, max_width=16, stream=None, reserve=True):
        """kbest_quadric_map_sample_assoc_batch_f64_dev on torch CUDA tensors (or raw addresses), asynchronous on `stream` (a raw
        hipStream_t integer): from quadrics against one resident map to n_sample joint associations a frame without a host read, a
        synchronise or an allocation.  The map, frames, d_nKeep, d_rowIdx and d_ccost as in quadric_map_probs_dev; d_assign (int32)
        at d_asgOff[b] [n_sample][nM]: rows of the notional raw block; d_logProb (float64) at d_lpOff[b] [n_sample]; d_frameKey int64
        / uint64 [B] or None (frame b: b).  d_method int32 [B] is required.  reserve=False: the caller has called
        reserve_quadric_map_sample_dev (timed loops, graph capture; the C entry never allocates)."""
        if reserve:
            self.reserve_quadric_map_sample_dev(B, maxMap, maxKeep, maxCol, n_sample)
        self._check(self.lib.kbest_quadric_map_sample_assoc_batch_f64_dev(
            self.ctx, int(B), int(maxMap), int(maxKeep), int(maxCol), _dptr(d_mapMean), _dptr(d_mapCov), _dptr(d_landOff), _dptr(d_nL),
            _dptr(d_measMean), _dptr(d_measCov), _dptr(d_measOff), _dptr(d_nM), float(gate), int(max_exact), int(max_width),
            int(n_sample), int(seed), int(sample_base), _dptr(d_frameKey), _dptr(d_nKeep), _dptr(d_rowIdx), _dptr(d_ccost),
            _dptr(d_assign), _dptr(d_asgOff), _dptr(d_logProb), _dptr(d_lpOff), _dptr(d_logPerm), _dptr(d_method), _dptr(d_nOpen),
            _dptr(d_nFrontier), _dptr(d_maxCluster), _stream(stream)))

    # ---- factor lists from association probabilities (kbest_factors.hip; the reference's consumer loop, system.cpp:279-346) ----
    @staticmethod
    def _factor_args(ptr, factor_thresh, new_thresh, box_sd, max_factor, factors, max_new, news, counts, total, support, n_support):
        """The factor arguments every C entry ends with.  factors: (fFrame, fMeas, fLand, fMap or None, fProb, fSigma) or None with
        capacity 0; news: (nFrame, nMeas, nProb, nSigma) or None with capacity 0; counts: (nFactor, factorOff, nNew, newOff)."""
        f = tuple(factors) if factors is not None else (None,) * 6
        n = tuple(news) if news is not None else (None,) * 4
        c = tuple(counts) if counts is not None else (None,) * 4
        if len(f) != 6 or len(n) != 4 or len(c) != 4:
            raise KBestError("factor lists: 6 factor arrays, 4 new-landmark arrays, 4 count arrays")
        return (float(factor_thresh), float(new_thresh), float(box_sd), int(max_factor)) + tuple(ptr(x) for x in f) + (int(max_new),) + \
            tuple(ptr(x) for x in n) + tuple(ptr(x) for x in c) + (ptr(total), ptr(support), int(n_support))

    def reserve_assoc_factors_dev(self, B, maxCol):
        """kbest_reserve_assoc_factors_dev: the per-(frame, measurement) counts and scan partials of assoc_factors_dev (never shrinks)."""
        self._check(self.lib.kbest_reserve_assoc_factors_dev(self.ctx, int(B), int(maxCol)))

    def assoc_factors_dev(self, B, maxSlot, maxCol, d_probs, d_probOff, d_nSlot, d_nM, max_factor, d_factors, max_new, d_news, d_counts,
                          d_total, d_rowIdx=None, row_stride=0, d_landOff=None, d_method=None, d_support=None, n_support=0,
                          factor_thresh=0.05, new_thresh=0.33, box_sd=3.0, stream=None, reserve=True):
        """kbest_assoc_factors_f64_dev on torch CUDA tensors (or raw addresses), asynchronous on `stream`: the thresholded, ordered
        factor and new-landmark lists of the probabilities of any entry, without a host read, a synchronise or an allocation.  Frame
        b: [nM][nSlot + 1] at d_probOff[b]; d_rowIdx (None: dense form) int32 [B][row_stride]; d_factors = (fFrame, fMeas, fLand int32,
        fMap int64 or None, fProb, fSigma float64) or None with max_factor 0; d_news = (nFrame, nMeas int32, nProb, nSigma float64) or
        None with max_new 0; d_counts = (nFactor int32, factorOff int64, nNew int32, newOff int64), each [B]; d_total int64 [2];
        d_support int32 [n_support] or None.  reserve=False: the caller has called reserve_assoc_factors_dev."""
        if reserve:
            self.reserve_assoc_factors_dev(B, maxCol)
        self._check(self.lib.kbest_assoc_factors_f64_dev(
            self.ctx, int(B), int(maxSlot), int(maxCol), _dptr(d_probs), _dptr(d_probOff), _dptr(d_nSlot), _dptr(d_nM), _dptr(d_rowIdx),
            int(row_stride), _dptr(d_landOff), _dptr(d_method),
            *self._factor_args(_dptr, factor_thresh, new_thresh, box_sd, max_factor, d_factors, max_new, d_news, d_counts, d_total,
                               d_support, n_support), _stream(stream)))

    def reserve_quadric_map_factors_dev(self, B, maxMap, maxKeep, maxCol):
        """kbest_reserve_quadric_map_factors_dev: reserve_quadric_map_dev and reserve_assoc_factors_dev."""
        self._check(self.lib.kbest_reserve_quadric_map_factors_dev(self.ctx, int(B), int(maxMap), int(maxKeep), int(maxCol)))

    def quadric_map_factors_dev(self, B, maxMap, maxKeep, maxCol, d_mapMean, d_mapCov, d_landOff, d_nL, d_measMean, d_measCov, d_measOff,
                                d_nM, gate, d_nKeep, d_rowIdx, d_cprobs, d_method, max_factor, d_factors, max_new, d_news, d_counts,
                                d_total, d_ccost=None, d_probs=None, d_probOff=None, d_logPerm=None, d_nOpen=None, d_nFrontier=None,
                                d_maxCluster=None, d_support=None, n_support=0, factor_thresh=0.05, new_thresh=0.33, box_sd=3.0,
                                max_exact=16, max_width=16, stream=None, reserve=True):
        """kbest_quadric_map_factors_batch_f64_dev: quadric_map_probs_dev (same arguments, same bits, d_probs may stay None), then
        the factor passes of assoc_factors_dev in compact form on d_cprobs, d_rowIdx and d_nKeep with d_method, all on `stream`.
        reserve=False: the caller has called reserve_quadric_map_factors_dev (timed loops, graph capture)."""
        if reserve:
            self.reserve_quadric_map_factors_dev(B, maxMap, maxKeep, maxCol)
        self._check(self.lib.kbest_quadric_map_factors_batch_f64_dev(
            self.ctx, int(B), int(maxMap), int(maxKeep), int(maxCol), _dptr(d_mapMean), _dptr(d_mapCov), _dptr(d_landOff), _dptr(d_nL),
            _dptr(d_measMean), _dptr(d_measCov), _dptr(d_measOff), _dptr(d_nM), float(gate), int(max_exact), int(max_width),
            _dptr(d_nKeep), _dptr(d_rowIdx), _dptr(d_ccost), _dptr(d_cprobs), _dptr(d_probs), _dptr(d_probOff), _dptr(d_logPerm),
            _dptr(d_method), _dptr(d_nOpen), _dptr(d_nFrontier), _dptr(d_maxCluster),
            *self._factor_args(_dptr, factor_thresh, new_thresh, box_sd, max_factor, d_factors, max_new, d_news, d_counts, d_total,
                               d_support, n_support), _stream(stream)))

    def assoc_factors(self, probs_list, land_off=None, method=None, factor_thresh=0.05, new_thresh=0.33, box_sd=3.0, max_factor=None,
                      max_new=None, n_support=0):
        """kbest_assoc_factors_batch_f64 on the dense [nM, nL + 1] arrays every host probability entry returns.  land_off[B] (None:
        0) gives the map index of a frame's landmark 0, method[B] (None: every frame emits) the method of the probability entry: a
        frame with method < 0 emits nothing.  max_factor / max_new None: a counting call first, then the exact capacities.  Returns
        a dict: factors (per frame a dict meas, land, map, prob, sigma), new (per frame a dict meas, prob, sigma), flat (the lists
        as they are: fFrame, fMeas, fLand, fMap, fProb, fSigma, nFrame, nMeas, nProb, nSigma, cut at min(total, capacity)), nFactor,
        factorOff, nNew, newOff, total (the true totals) and support (int32 [n_support], None with n_support 0)."""
        B = len(probs_list)
        arrs = [np.ascontiguousarray(p, dtype=np.float64) for p in probs_list]
        if any(a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1 for a in arrs):
            raise KBestError("assoc_factors: every frame is an [nM, nL + 1] array with nM >= 1")
        nM = np.array([a.shape[0] for a in arrs], np.int32)
        nL = np.array([a.shape[1] - 1 for a in arrs], np.int32)
        sizes = np.array([a.size for a in arrs], np.int64)
        probOff = np.zeros(B, np.int64)
        probOff[1:] = np.cumsum(sizes)[:-1]
        flat = np.concatenate([np.zeros(0)] + [a.reshape(-1) for a in arrs])
        lo = None if land_off is None else np.ascontiguousarray(land_off, dtype=np.int64)
        me = None if method is None else np.ascontiguousarray(method, dtype=np.int32)
        if (lo is not None and lo.shape != (B,)) or (me is not None and me.shape != (B,)):
            raise KBestError("assoc_factors: land_off and method hold one number per frame")
        counts = (np.zeros(max(B, 1), np.int32), np.zeros(max(B, 1), np.int64), np.zeros(max(B, 1), np.int32), np.zeros(max(B, 1), np.int64))
        total = np.zeros(2, np.int64)
        support = np.zeros(int(n_support), np.int32) if n_support else None

        def call(cf, cn):
            f = (np.zeros(cf, np.int32), np.zeros(cf, np.int32), np.zeros(cf, np.int32), np.zeros(cf, np.int64), np.zeros(cf), np.zeros(cf))
            n = (np.zeros(cn, np.int32), np.zeros(cn, np.int32), np.zeros(cn), np.zeros(cn))
            self._check(self.lib.kbest_assoc_factors_batch_f64(
                self.ctx, B, _ptr(flat), _ptr(probOff), _ptr(nL), _ptr(nM), _ptr(lo), _ptr(me),
                *self._factor_args(_ptr, factor_thresh, new_thresh, box_sd, cf, f if cf else None, cn, n if cn else None, counts, total,
                                   support, n_support)))
            return f, n

        if max_factor is None or max_new is None:
            call(0, 0)
            max_factor = int(total[0]) if max_factor is None else int(max_factor)
            max_new = int(total[1]) if max_new is None else int(max_new)
        f, n = call(int(max_factor), int(max_new))
        gf, gn = min(int(total[0]), int(max_factor)), min(int(total[1]), int(max_new))
        f, n = tuple(a[:gf] for a in f), tuple(a[:gn] for a in n)
        nFactor, factorOff, nNew, newOff = (c[:B].copy() for c in counts)
        cutf = lambda a, b: a[min(int(factorOff[b]), gf): min(int(factorOff[b]) + int(nFactor[b]), gf)]  # noqa: E731
        cutn = lambda a, b: a[min(int(newOff[b]), gn): min(int(newOff[b]) + int(nNew[b]), gn)]  # noqa: E731
        return dict(
            factors=[dict(meas=cutf(f[1], b), land=cutf(f[2], b), map=cutf(f[3], b), prob=cutf(f[4], b), sigma=cutf(f[5], b)) for b in range(B)],
            new=[dict(meas=cutn(n[1], b), prob=cutn(n[2], b), sigma=cutn(n[3], b)) for b in range(B)],
            flat=dict(zip(("fFrame", "fMeas", "fLand", "fMap", "fProb", "fSigma", "nFrame", "nMeas", "nProb", "nSigma"), f + n)),
            nFactor=nFactor, factorOff=factorOff, nNew=nNew, newOff=newOff, total=total.copy(), support=support)

    def quadric_map_factors(self, map_mean, map_cov, frames, gate, factor_thresh=0.05, new_thresh=0.33, box_sd=3.0, k=0, max_exact=16,
                            max_big=20, max_width=16, support=True):
        """From quadrics against one map to the factor lists: quadric_map_probs(map_mean, map_cov, frames, gate, k, ...) and
        assoc_factors on its dense slices with the frames' landOff and method -- the defaults are the reference's
        NEW_FACTOR_PROB_THRESH, NEW_LANDMARK_THRESH and BOX_SD (constsUtils.h:75-78).  Returns the dict of assoc_factors (support
        over the whole map, None with support=False) with method, nKeep and logPerm of the probability entry added."""
        out = self.quadric_map_probs(map_mean, map_cov, frames, gate, k=k, max_exact=max_exact, max_big=max_big, max_width=max_width)
        n_map = len(np.asarray(map_mean, np.float64).reshape(-1, 3))
        r = self.assoc_factors(out[0], land_off=[f[0] for f in frames], method=out[1], factor_thresh=factor_thresh, new_thresh=new_thresh,
                               box_sd=box_sd, n_support=n_map if support else 0)
        r.update(method=out[1], nKeep=out[2], logPerm=out[7])
        return r

    def factors_kernel_usage(self, which):
        """(registers, scratch bytes, static LDS bytes) of a factor pass: 0 count, 1 scan inside a frame, 2 scan over the frames, 3 emit."""
        v = np.zeros(3, np.int32)
        self._check(self.lib.kbest_factors_kernel_usage(int(which), _ptr(v[0:1]), _ptr(v[1:2]), _ptr(v[2:3])))
        return tuple(int(x) for x in v)

    def quadric_map_sample_kernel_usage(self):
        """(registers, scratch bytes, static LDS bytes) of the kernel that maps compact rows to raw rows."""
        v = np.zeros(3, np.int32)
        self._check(self.lib.kbest_quadric_map_sample_kernel_usage(_ptr(v[0:1]), _ptr(v[1:2]), _ptr(v[2:3])))
        return tuple(int(x) for x in v)

    @staticmethod
    def _pack_boxes(boxesL, boxesR):
        """boxesL / boxesR: lists of (n, 5) arrays (xmin, ymin, xmax, ymax, xOffset)."""
        nL = np.array([len(b) for b in boxesL], np.int32)
        nR = np.array([len(b) for b in boxesR], np.int32)
        cat = lambda boxes: np.ascontiguousarray(np.concatenate([np.asarray(b, np.float64).reshape(-1, 5) for b in boxes] + [np.zeros((0, 5))]))  # noqa: E731
        return nL, nR, cat(boxesL), cat(boxesR)

    def bb_costs(self, boxesL, boxesR, gate):
        """Batched computeBBCostMatrix.  Returns a list of (nR+nL)*nL column-major profit blocks."""
        nL, nR, bl, br = self._pack_boxes(boxesL, boxesR)
        sizes = (nR.astype(np.int64) + nL) * nL
        out = np.zeros(int(sizes.sum()))
        self._check(self.lib.kbest_bb_costs_f64(self.ctx, len(boxesL), _ptr(nL), _ptr(nR), _ptr(bl), _ptr(br), float(gate), _ptr(out)))
        off = np.concatenate([[0], np.cumsum(sizes)])
        return [out[off[b]: off[b + 1]] for b in range(len(boxesL))]

    def bb_match(self, boxesL, boxesR, gate):
        """Batched asgnBB.  boxesL / boxesR: lists of (n, 5) arrays (xmin, ymin, xmax, ymax, xOffset)."""
        nL, nR, bl, br = self._pack_boxes(boxesL, boxesR)
        asg = np.full(int(nL.sum()), -9, np.int32)
        self._check(self.lib.kbest_bb_match_batch_f64(self.ctx, len(boxesL), _ptr(nL), _ptr(nR), _ptr(bl), _ptr(br),
                                                      float(gate), _ptr(asg)))
        off = np.concatenate([[0], np.cumsum(nL)])
        return [asg[off[b]: off[b + 1]] for b in range(len(boxesL))]

    # ---- device buffers (torch tensors already resident in HBM) -------------------------
    def register_host(self, *arrays):
        """kbest_register_host_buffer on numpy arrays the caller keeps using (cost blocks, result tables): pinned and mapped,
        so that kbest_batch_f64 moves them without staging copies.  The arrays must stay alive until unregister_host."""
        for a in arrays:
            self._check(self.lib.kbest_register_host_buffer(self.ctx, a.ctypes.data_as(C.c_void_p), a.nbytes))

    def unregister_host(self, *arrays):
        for a in arrays:
            self._check(self.lib.kbest_unregister_host_buffer(self.ctx, a.ctypes.data_as(C.c_void_p)))

    def reserve(self, B, N, k):
        self._check(self.lib.kbest_reserve(self.ctx, B, N, k))

    def kbest_dev(self, d_cost, B, N, M, k, d_row4col, d_col4row, d_gain, d_nf, maximize=False, cutoff=None,
                  d_pushed=None, prune=True, stream=None, root_shard=None, d_nRow=None, d_nCol=None, d_costOff=None,
                  tables_i8=False, d_tie_flags=None, tie_check=True, reference_order=False):
        """Asynchronous launch on `stream` (a raw hipStream_t integer, e.g.
        torch.cuda.current_stream().cuda_stream).  All d_* are torch CUDA tensors (tables_i8: d_row4col / d_col4row int8;
        d_tie_flags: int32 [B], receives the KBEST_TIE_* flags)."""
        flags = ((KBEST_FLAG_COUNT_PUSHED if d_pushed is not None else 0) | (0 if prune else KBEST_FLAG_NO_PRUNE) |
                 (KBEST_FLAG_TABLES_I8 if tables_i8 else 0) | (0 if tie_check else KBEST_FLAG_NO_TIE_CHECK) |
                 (KBEST_FLAG_REFERENCE_ORDER if reference_order else 0))
        o = self._opts(maximize, cutoff, flags, root_shard)
        if d_tie_flags is not None:
            o.tie_flags = d_tie_flags.data_ptr()
        # the C entry never allocates (kbest_c.h): size the workspace here (a no-op once it is large enough)
        if reference_order or N > KBEST_MAX_DIM_WIDE:
            self._check(self.lib.kbest_reserve_exact(self.ctx, B, N, M, k))
        else:
            self.reserve(B, N, k)

        self._check(self.lib.kbest_batch_f64_dev(self.ctx, C.byref(o), B, N, M, _dptr(d_nRow), _dptr(d_nCol), _dptr(d_cost),
                                                 _dptr(d_costOff), k, _dptr(d_row4col), _dptr(d_col4row), _dptr(d_gain), _dptr(d_nf),
                                                 _dptr(d_pushed), _stream(stream)))


    def resolve_ties_dev(self, d_cost, B, N, M, k, d_row4col, d_col4row, d_gain, d_tie_flags, maximize=False, cutoff=None, stream=None,
                         d_nRow=None, d_nCol=None, d_costOff=None, tables_i8=False, reference_ties=False, canonical_ties=False, d_nf=None):
        """kbest_resolve_ties_dev: the synchronous second call behind kbest_dev -- completes the gain levels that straddle slot k
        in the device tables (same arguments as the launch).  By default (reference_ties: the accepted no-op flag) every problem flagged
        with a tie is replaced by the reference-order kernel's tables; canonical_ties: KBEST_FLAG_CANONICAL_TIES -- the engine's own
        rule instead (levels that straddle slot k completed in steps).  d_nf: the launch's nf tensor -- a re-run problem's entry takes
        the re-run's count (without it the launch's count stays, which a cutoff on gains that round apart can make stale)."""
        o = self._opts(maximize, cutoff, (KBEST_FLAG_TABLES_I8 if tables_i8 else 0) | (KBEST_FLAG_REFERENCE_TIES if reference_ties else 0) |
                       (KBEST_FLAG_CANONICAL_TIES if canonical_ties else 0))
        self._check(self.lib.kbest_resolve_ties_dev(self.ctx, C.byref(o), B, N, M, _dptr(d_nRow), _dptr(d_nCol), _dptr(d_cost),
                                                    _dptr(d_costOff), k, _dptr(d_row4col), _dptr(d_col4row), _dptr(d_gain),
                                                    _dptr(d_tie_flags), _dptr(d_nf), _stream(stream)))

    def merge_topk_dev(self, B, n_shard, k, M, d_gain, d_row4col, d_nf, shard_stride_bytes, d_out_gain, d_out_row4col, d_out_nf,
                       maximize=False, stream=None, tables_i8=False):
        """kbest_merge_topk_f64_dev (tables_i8: kbest_merge_topk_i8_f64_dev -- the shards' row4col tables are int8): k-way merge
        of per-shard k-best lists (torch tensors / device pointers)."""
        fn = self.lib.kbest_merge_topk_i8_f64_dev if tables_i8 else self.lib.kbest_merge_topk_f64_dev
        self._check(fn(self.ctx, B, n_shard, k, M, int(bool(maximize)), _dptr(d_gain), _dptr(d_row4col), _dptr(d_nf),
                       int(shard_stride_bytes), _dptr(d_out_gain), _dptr(d_out_row4col), _dptr(d_out_nf), _stream(stream)))

    def merge_gains_dev(self, B, n_shard, k, M, d_gain, d_nf, own_shard, d_own_row4col8, d_out_gain, d_out_row4col8, d_out_nf, d_tied,
                        maximize=False, stream=None):
        """kbest_merge_gains_f64_dev: the global k-best heap from all shards' gains [S,B,k] / nf [S,B] and this rank's own
        rows (int8 [B,k,M]); d_out_row4col8 (zeroed by the caller) receives the own winners' rows, d_tied (zeroed) the tie word."""
        self._check(self.lib.kbest_merge_gains_f64_dev(self.ctx, B, n_shard, k, M, int(bool(maximize)), _dptr(d_gain), _dptr(d_nf),
                                                       int(own_shard), _dptr(d_own_row4col8), _dptr(d_out_gain), _dptr(d_out_row4col8),
                                                       _dptr(d_out_nf), _dptr(d_tied), _stream(stream)))

    def reserve_assoc(self, B, maxRawRow, maxCol, k):
        self._check(self.lib.kbest_reserve_assoc(self.ctx, B, maxRawRow, maxCol, k))

    def assoc_probs_dev(self, B, maxRawRow, maxCol, d_nL, d_nM, d_nRow, d_cost, d_costOff, k, d_probs, d_probOff, d_nf,
                        condition=True, stream=None):
        """Fused association on device buffers (torch CUDA tensors), asynchronous on `stream`: one launch."""
        self._check(self.lib.kbest_assoc_probs_batch_f64_dev(self.ctx, B, maxRawRow, maxCol, _dptr(d_nL), _dptr(d_nM), _dptr(d_nRow),
                                                             _dptr(d_cost), _dptr(d_costOff), k, int(bool(condition)), _dptr(d_probs),
                                                             _dptr(d_probOff), _dptr(d_nf), _stream(stream)))

    def reserve_permanent(self, B, maxRawRow, maxCol):
        self._check(self.lib.kbest_reserve_permanent(self.ctx, B, maxRawRow, maxCol))

    def permanent_probs_dev(self, B, maxRawRow, maxCol, d_nL, d_nM, d_cost, d_costOff, d_probs, d_probOff, d_perm=None,
                            condition=False, stream=None, reserve=True):
        """kbest_permanent_probs_batch_f64_dev on torch CUDA tensors, asynchronous on `stream` (a raw hipStream_t integer): one
        launch.  The work space is sized here (a no-op once it is large enough): the C entry never allocates.  reserve=False: the
        caller has called reserve_permanent (timed loops: nothing but the C entry between two events)."""
        if reserve:
            self.reserve_permanent(B, maxRawRow, maxCol)
        self._check(self.lib.kbest_permanent_probs_batch_f64_dev(self.ctx, B, maxRawRow, maxCol, _dptr(d_nL), _dptr(d_nM), _dptr(d_cost),
                                                                 _dptr(d_costOff), int(bool(condition)), _dptr(d_probs), _dptr(d_probOff),
                                                                 _dptr(d_perm), _stream(stream)))

    def reserve_sample(self, B, maxRawRow, maxCol):
        self._check(self.lib.kbest_reserve_sample(self.ctx, B, maxRawRow, maxCol))

    def sample_assoc_dev(self, B, maxRawRow, maxCol, d_nL, d_nM, d_cost, d_costOff, n_sample, d_assign, d_asgOff, d_logProb, d_lpOff,
                         d_perm=None, seed=0, sample_base=0, d_frameKey=None, condition=False, stream=None, reserve=True):
        """kbest_sample_assoc_batch_f64_dev on torch CUDA tensors, asynchronous on `stream` (a raw hipStream_t integer): one
        launch.  d_frameKey: int64 / uint64 [B] or None.  The work space is sized here (a no-op once it is large enough): the C entry
        never allocates.  reserve=False: the caller has called reserve_sample."""
        if reserve:
            self.reserve_sample(B, maxRawRow, maxCol)
        self._check(self.lib.kbest_sample_assoc_batch_f64_dev(self.ctx, B, maxRawRow, maxCol, _dptr(d_nL), _dptr(d_nM), _dptr(d_cost),
                                                              _dptr(d_costOff), int(bool(condition)), int(n_sample), int(seed),
                                                              int(sample_base), _dptr(d_frameKey), _dptr(d_assign), _dptr(d_asgOff),
                                                              _dptr(d_logProb), _dptr(d_lpOff), _dptr(d_perm), _stream(stream)))

    def reserve_belief(self, B, maxRawRow, maxCol):
        self._check(self.lib.kbest_reserve_belief(self.ctx, B, maxRawRow, maxCol))

    def belief_probs_dev(self, B, maxRawRow, maxCol, d_nL, d_nM, d_cost, d_costOff, d_probs, d_probOff, d_iters=None, d_resid=None,
                         condition=False, tol=1e-12, max_iter=10000, stream=None, reserve=True):
        """kbest_belief_probs_batch_f64_dev on torch CUDA tensors, asynchronous on `stream` (a raw hipStream_t integer): one
        launch.  The work space is sized here (a no-op once it is large enough): the C entry never allocates.  reserve=False: the
        caller has called reserve_belief (timed loops: nothing but the C entry between two events)."""
        if reserve:
            self.reserve_belief(B, maxRawRow, maxCol)
        self._check(self.lib.kbest_belief_probs_batch_f64_dev(self.ctx, B, maxRawRow, maxCol, _dptr(d_nL), _dptr(d_nM), _dptr(d_cost),
                                                              _dptr(d_costOff), int(bool(condition)), float(tol), int(max_iter),
                                                              _dptr(d_probs), _dptr(d_probOff), _dptr(d_iters), _dptr(d_resid),
                                                              _stream(stream)))

    def reserve_clustered(self, B, maxRawRow, maxCol):
        self._check(self.lib.kbest_reserve_clustered(self.ctx, B, maxRawRow, maxCol))

    def clustered_probs_dev(self, B, maxRawRow, maxCol, d_nL, d_nM, d_cost, d_costOff, d_probs, d_probOff, d_logPerm=None,
                            d_info=None, d_maxCluster=None, d_label=None, labelStride=0, condition=False, stream=None,
                            reserve=True):
        """kbest_clustered_probs_batch_f64_dev on torch CUDA tensors, asynchronous on `stream` (a raw hipStream_t integer): one
        launch.  The work space is sized here (a no-op once it is large enough): the C entry never allocates.  reserve=False: the
        caller has called reserve_clustered (timed loops: nothing but the C entry between two events)."""
        if reserve:
            self.reserve_clustered(B, maxRawRow, maxCol)
        self._check(self.lib.kbest_clustered_probs_batch_f64_dev(self.ctx, B, maxRawRow, maxCol, _dptr(d_nL), _dptr(d_nM), _dptr(d_cost),
                                                                 _dptr(d_costOff), int(bool(condition)), _dptr(d_probs), _dptr(d_probOff),
                                                                 _dptr(d_logPerm), _dptr(d_info), _dptr(d_maxCluster), _dptr(d_label),
                                                                 int(labelStride), _stream(stream)))

    def reserve_clustered_sample(self, B, maxRawRow, maxCol):
        self._check(self.lib.kbest_reserve_clustered_sample(self.ctx, B, maxRawRow, maxCol))

    def clustered_sample_assoc_dev(self, B, maxRawRow, maxCol, d_nL, d_nM, d_cost, d_costOff, n_sample, d_assign, d_asgOff, d_logProb,
                                   d_lpOff, d_logPerm=None, d_info=None, d_maxCluster=None, seed=0, sample_base=0, d_frameKey=None,
                                   condition=False, stream=None, reserve=True):
        """kbest_clustered_sample_assoc_batch_f64_dev on torch CUDA tensors, asynchronous on `stream` (a raw hipStream_t integer):
        one launch.  d_frameKey: int64 / uint64 [B] or None.  The work space is sized here (a no-op once it is large enough): the C
        entry never allocates.  reserve=False: the caller has called reserve_clustered_sample."""
        if reserve:
            self.reserve_clustered_sample(B, maxRawRow, maxCol)
        self._check(self.lib.kbest_clustered_sample_assoc_batch_f64_dev(self.ctx, B, maxRawRow, maxCol, _dptr(d_nL), _dptr(d_nM),
                                                                        _dptr(d_cost), _dptr(d_costOff), int(bool(condition)),
                                                                        int(n_sample), int(seed), int(sample_base), _dptr(d_frameKey),
                                                                        _dptr(d_assign), _dptr(d_asgOff), _dptr(d_logProb),
                                                                        _dptr(d_lpOff), _dptr(d_logPerm), _dptr(d_info),
                                                                        _dptr(d_maxCluster), _stream(stream)))

    def clustered_partial_dev(self, B, maxRawRow, maxCol, d_nL, d_nM, d_cost, d_costOff, d_probs, d_probOff, d_nOpen, d_openDesc,
                              descStride, d_openRows, rowStride, d_sub, max_exact=16, d_logPerm=None, d_info=None,
                              d_maxCluster=None, d_label=None, labelStride=0, condition=False, stream=None, reserve=True):
        """kbest_clustered_partial_batch_f64_dev on torch CUDA tensors, asynchronous on `stream`: clustered_probs_dev in the partial
        mode -- clusters of more than max_exact measurements stay open (zeros) and come back as sub-problems: d_nOpen int32 [B],
        d_openDesc int32 [B, descStride, 4] (root, m_k, nL_k, R_k), d_openRows int32 [B, rowStride], d_sub doubles shaped like
        d_cost (include/kbest_c.h has the layout)."""
        if reserve:
            self.reserve_clustered(B, maxRawRow, maxCol)
        self._check(self.lib.kbest_clustered_partial_batch_f64_dev(self.ctx, B, maxRawRow, maxCol, _dptr(d_nL), _dptr(d_nM), _dptr(d_cost),
                                                                   _dptr(d_costOff), int(bool(condition)), int(max_exact), _dptr(d_probs),
                                                                   _dptr(d_probOff), _dptr(d_logPerm), _dptr(d_info), _dptr(d_maxCluster),
                                                                   _dptr(d_label), int(labelStride), _dptr(d_nOpen), _dptr(d_openDesc),
                                                                   int(descStride), _dptr(d_openRows), int(rowStride), _dptr(d_sub),
                                                                   _stream(stream)))

    def reserve_hybrid_dev(self, B, maxRawRow, maxCol):
        """kbest_reserve_hybrid_dev: everything hybrid_frontier_probs_dev needs besides the caller's buffers, sized from the
        three numbers alone."""
        self._check(self.lib.kbest_reserve_hybrid_dev(self.ctx, int(B), int(maxRawRow), int(maxCol)))

    def hybrid_frontier_probs_dev(self, B, maxRawRow, maxCol, d_nL, d_nM, d_cost, d_costOff, d_sub, d_probs, d_probOff, d_method,
                                  d_logPerm=None, d_nOpen=None, d_nFrontier=None, d_maxCluster=None, condition=False, max_exact=16,
                                  max_width=16, stream=None, reserve=True):
        """kbest_hybrid_frontier_probs_batch_f64_dev on torch CUDA tensors, asynchronous on `stream` (a raw hipStream_t integer):
        hybrid_frontier_probs(k=0, max_big=0) -- the partial clustered kernel, the frontier tier on every open cluster, the scatter
        into the frames -- without a host read, a synchronise or an allocation, and with that entry's bits.  d_sub: a work buffer
        shaped like d_cost.  d_method int32 [B] is required; d_logPerm (float64), d_nOpen, d_nFrontier, d_maxCluster (int32) may be
        None.  A frame beyond (maxRawRow, maxCol) is not touched (method -1): zero d_probs first for zeros there.  reserve=False:
        the caller has called reserve_hybrid_dev (timed loops; the C entry never allocates)."""
        if reserve:
            self.reserve_hybrid_dev(B, maxRawRow, maxCol)
        self._check(self.lib.kbest_hybrid_frontier_probs_batch_f64_dev(
            self.ctx, int(B), int(maxRawRow), int(maxCol), _dptr(d_nL), _dptr(d_nM), _dptr(d_cost), _dptr(d_costOff),
            int(bool(condition)), int(max_exact), int(max_width), _dptr(d_sub), _dptr(d_probs), _dptr(d_probOff), _dptr(d_logPerm),
            _dptr(d_method), _dptr(d_nOpen), _dptr(d_nFrontier), _dptr(d_maxCluster), _stream(stream)))

    def reserve_hybrid_sample_dev(self, B, maxRawRow, maxCol, n_sample):
        """kbest_reserve_hybrid_sample_dev: everything hybrid_frontier_sample_assoc_dev needs besides the caller's buffers, sized
        from the four numbers alone."""
        self._check(self.lib.kbest_reserve_hybrid_sample_dev(self.ctx, int(B), int(maxRawRow), int(maxCol), int(n_sample)))

    def hybrid_frontier_sample_assoc_dev(self, B, maxRawRow, maxCol, d_nL, d_nM, d_cost, d_costOff, d_sub, n_sample, d_assign, d_asgOff,
                                         d_logProb, d_lpOff, d_method, d_logPerm=None, d_nOpen=None, d_nFrontier=None,
                                         d_maxCluster=None, seed=0, sample_base=0, d_frameKey=None, condition=False, max_exact=16,
                                         max_width=16, stream=None, reserve=True):
        """kbest_hybrid_frontier_sample_assoc_batch_f64_dev on torch CUDA tensors (or raw addresses), asynchronous on `stream` (a
        raw hipStream_t integer): hybrid_frontier_sample_assoc() -- n_sample whole hypotheses a frame, the clusters of at most
        max_exact measurements by the clustered sampler's walk, every larger one by the walk over the frontier tier's layers --
        without a host read, a synchronise or an allocation, and with that entry's bits.  d_sub: a work buffer shaped like d_cost.
        d_assign (int32) at d_asgOff[b] [n_sample][nM], d_logProb (float64) at d_lpOff[b] [n_sample]; d_frameKey int64 / uint64
        [B] or None (frame b: b).  d_method int32 [B] is required; d_logPerm (float64), d_nOpen, d_nFrontier, d_maxCluster (int32)
        may be None.  A frame beyond (maxRawRow, maxCol): method -1, its draws not touched.  reserve=False: the caller has called
        reserve_hybrid_sample_dev (timed loops; the C entry never allocates)."""
        if reserve:
            self.reserve_hybrid_sample_dev(B, maxRawRow, maxCol, n_sample)
        self._check(self.lib.kbest_hybrid_frontier_sample_assoc_batch_f64_dev(
            self.ctx, int(B), int(maxRawRow), int(maxCol), _dptr(d_nL), _dptr(d_nM), _dptr(d_cost), _dptr(d_costOff),
            int(bool(condition)), int(max_exact), int(max_width), int(n_sample), int(seed), int(sample_base), _dptr(d_frameKey),
            _dptr(d_sub), _dptr(d_assign), _dptr(d_asgOff), _dptr(d_logProb), _dptr(d_lpOff), _dptr(d_logPerm), _dptr(d_method),
            _dptr(d_nOpen), _dptr(d_nFrontier), _dptr(d_maxCluster), _stream(stream)))


class KBestMulti:
    """Multi-device engine of include/kbest_c.h: one context per GPU in ONE process, contiguous block sharding, RCCL
    all-gather of the packed result tables (kbest_multi.cpp)."""

    def __init__(self, device_ids):
        self.lib = load_library()
        ids = np.ascontiguousarray(device_ids, dtype=np.int32)
        self.m = C.c_void_p()
        rc = self.lib.kbest_create_multi(C.byref(self.m), _ptr(ids), len(ids))
        if rc != 0:
            raise KBestError(f"kbest_create_multi({list(ids)}): {self.lib.kbest_strerror(rc).decode()}")

    def close(self):
        if getattr(self, "m", None):
            self.lib.kbest_destroy_multi(self.m)
            self.m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def kbest(self, costs, N, M, k, maximize=False, cutoff=None, nRow=None, nCol=None, subtree=False, n_shard=0, reference_ties=False,
              canonical_ties=False):
        """Batch mode (default): contiguous blocks of the batch per device.  subtree=True: every device enumerates its share
        of the root's subtrees of every matrix (n_shard shards, 0 = one per device), one all-gather of the packed lists,
        k-way merge on the device (kbest_merge.hip)."""
        costs = np.ascontiguousarray(costs, dtype=np.float64).reshape(-1, N * M)
        B = costs.shape[0]
        r4c = np.empty((B, k, M), np.int32); c4r = np.empty((B, k, N), np.int32)
        gain = np.empty((B, k)); nf = np.empty(B, np.int32)
        o = KBestOpts()
        self.lib.kbest_default_opts(C.byref(o))
        o.maximize = int(bool(maximize)); o.use_cutoff = int(cutoff is not None); o.cutoff = float(cutoff or 0.0)
        if reference_ties:  # (batch mode: kbest_c.h, KBEST_FLAG_REFERENCE_TIES -- the default; accepted)
            o.flags |= KBEST_FLAG_REFERENCE_TIES
        if canonical_ties:  # (the engine's own rule on exact ties)
            o.flags |= KBEST_FLAG_CANONICAL_TIES
        if nRow is not None:
            nRow = np.ascontiguousarray(nRow, dtype=np.int32); nCol = np.ascontiguousarray(nCol, dtype=np.int32)
        if subtree:
            rc = self.lib.kbest_batch_f64_multi_ex(self.m, C.byref(o), KBEST_MULTI_SUBTREE, int(n_shard), B, N, M, _ptr(nRow),
                                                   _ptr(nCol), _ptr(costs), k, _ptr(r4c), _ptr(c4r), _ptr(gain), _ptr(nf))
        else:
            rc = self.lib.kbest_batch_f64_multi(self.m, C.byref(o), B, N, M, _ptr(nRow), _ptr(nCol), _ptr(costs), k, _ptr(r4c),
                                                _ptr(c4r), _ptr(gain), _ptr(nf))
        if rc != 0:
            raise KBestError(f"{self.lib.kbest_strerror(rc).decode()}: {self.lib.kbest_multi_last_error(self.m).decode()}")
        return nf, r4c, c4r, gain

    def tables_agree(self):
        return self.lib.kbest_multi_tables_agree(self.m) == 1

    def last_tie_flags(self):
        """KBEST_TIE_* flags of the problems of the last batch-mode call (kbest_multi_last_tie_flags)."""
        n = self.lib.kbest_multi_last_tie_flags(self.m, None, 0)
        out = np.zeros(max(n, 0), np.int32)
        if n > 0:
            self.lib.kbest_multi_last_tie_flags(self.m, _ptr(out), n)
        return out

    def exchange_bytes(self):
        """(bytes that arrived at one device in the exchanges of the last call, path: 0 batch, 1 subtree gains first, 2 subtree whole lists)."""
        path = C.c_int(0)
        n = self.lib.kbest_multi_exchange_bytes(self.m, C.byref(path))
        return int(n), int(path.value)

    def timeline(self):
        """Host times of the last call per device: array [nDev, 6] of seconds since the call was entered (kbest_multi_timeline)."""
        n = self.lib.kbest_multi_size(self.m)
        out = np.zeros((n, KBEST_MULTI_STAMPS))
        self.lib.kbest_multi_timeline(self.m, _ptr(out), n)
        return out


# ---- reference-named conveniences (B = 1), mirroring shortestPathCPP.hpp / assignment.h -------------
_default = None


def _engine():
    global _default
    if _default is None:
        _default = KBestEngine(0)
    return _default


def kBest2D(k, numRow, numCol, maximize, C_):
    """shortestPathCPP.hpp:204-212.  Returns (numFound, col4rowBest[k,numRow], row4colBest[k,numCol], gainBest[k])."""
    nf, r4c, c4r, g = _engine().kbest(np.asarray(C_).reshape(1, -1), numRow, numCol, k, maximize)
    return int(nf[0]), c4r[0], r4c[0], g[0]


def kBest2DCutoff(k, numRow, numCol, maximize, C_, cutoff):
    """shortestPathCPP.hpp:256-265."""
    nf, r4c, c4r, g = _engine().kbest(np.asarray(C_).reshape(1, -1), numRow, numCol, k, maximize, cutoff)
    return int(nf[0]), c4r[0], r4c[0], g[0]


def assignmentProb(costMatrix, nL, nM, k):
    """assignment.h:11.  Returns probs[nM][nL+1]."""
    out, _ = _engine().weights([costMatrix], [nL], [nM], k)
    return out[0]


def permanentProb(costMatrix, nL, nM, permOpt=1):
    """assignment.h:13.  Returns probs[nM][nL+1]; exact for permOpt 0, 1 and 2, any other value raises as the reference throws."""
    if permOpt not in (0, 1, 2):
        raise RuntimeError("Unknown permanent option passed!")
    out, _ = _engine().permanent_probs([costMatrix], [nL], [nM])
    return out[0]


def sampleAssoc(costMatrix, nL, nM, nSample, seed=0):
    """Not in the reference: nSample joint associations drawn from the exact posterior permanentProb gives the marginals of
    (frame key 0).  Returns int32 [nSample][nM]: the row every measurement takes (a row >= nL: unassigned); raises RuntimeError
    when the frame has no consistent association."""
    out, _, perm = _engine().sample_assoc([costMatrix], [nL], [nM], nSample, seed=seed, frame_key=[0])
    if not perm[0] > 0.0:
        raise RuntimeError("sampleAssoc: the frame has no consistent association (permanent 0)")
    return out[0]


def beliefProb(costMatrix, nL, nM):
    """Not in the reference: the association probabilities by loopy belief propagation (tol 1e-12, at most 10 000 sweeps), for
    frames of up to 128 measurements.  Returns probs[nM][nL+1]; an infeasible frame comes back as all zeros."""
    out, _, _ = _engine().belief_probs([costMatrix], [nL], [nM])
    return out[0]


def clusterProb(costMatrix, nL, nM):
    """Not in the reference: the EXACT association probabilities by gated clusters, for frames of up to 128 measurements whose
    clusters have at most 16.  Returns probs[nM][nL+1]; raises RuntimeError naming the largest cluster when the frame is refused;
    an infeasible frame comes back as all zeros."""
    out, _, info, maxCluster = _engine().clustered_probs([costMatrix], [nL], [nM])
    if info[0] < 0:
        raise RuntimeError(f"clusterProb: frame refused (info {int(info[0])}): its largest cluster has {int(maxCluster[0])} measurements")
    return out[0]


def clusterSampleAssoc(costMatrix, nL, nM, nSample, seed=0):
    """Not in the reference: sampleAssoc for the frames clusterProb takes (up to 128 measurements, clusters of at most 16; frame key
    0).  Returns int32 [nSample][nM]: the row every measurement takes (a row >= nL: unassigned); raises RuntimeError naming the
    largest cluster when the frame is refused, and when the frame has no consistent association."""
    out, _, _, info, maxCluster = _engine().clustered_sample_assoc([costMatrix], [nL], [nM], nSample, seed=seed, frame_key=[0])
    if info[0] < 0:
        raise RuntimeError(f"clusterSampleAssoc: frame refused (info {int(info[0])}): its largest cluster has {int(maxCluster[0])} measurements")
    if info[0] == 0:
        raise RuntimeError("clusterSampleAssoc: the frame has no consistent association (some cluster's permanent is 0)")
    return out[0]


def hybridProb(costMatrix, nL, nM, k):
    """Not in the reference: the hybrid association probabilities, for frames of up to 128 measurements: exact on every gated
    cluster of at most 16 measurements, assignmentProb(k) on each larger cluster alone.  Returns probs[nM][nL+1]; raises
    RuntimeError only when the frame is refused (a cluster with more rows >= nL than measurements); an infeasible frame comes back
    as all zeros."""
    out, method, _, _ = _engine().hybrid_probs([costMatrix], [nL], [nM], k)
    if method[0] == -1:
        raise RuntimeError("hybridProb: frame refused: a cluster holds more rows >= nL than measurements")
    return out[0]


def hybridFrontierSampleAssoc(costMatrix, nL, nM, nSample, seed=0):
    """Not in the reference: clusterSampleAssoc for the frames hybridFrontierProb(k = 0) takes: gated clusters of up to 64
    measurements whose rows, in the greedy order, keep at most 16 columns open are drawn too.  Returns int32 [nSample][nM]; raises
    RuntimeError when the frame is refused or has no consistent association."""
    asg, _, _, method, _, _, maxCluster = _engine().hybrid_frontier_sample_assoc([costMatrix], [nL], [nM], nSample, seed=seed,
                                                                                   frame_key=[0])
    if method[0] == -1:
        raise RuntimeError(f"hybridFrontierSampleAssoc: frame refused: its largest cluster has {int(maxCluster[0])} measurements")
    if method[0] == -2:
        raise RuntimeError("hybridFrontierSampleAssoc: the frame has no consistent association (some cluster's permanent is 0)")
    return asg[0]


def hybridSampleAssoc(costMatrix, nL, nM, nSample, k, seed=0):
    """Not in the reference: hybridFrontierSampleAssoc for EVERY gated frame of up to 128 measurements: a cluster no exact tier
    takes is drawn from its k best assignments within the cutoff 42 under assignmentProb's weights (k >= 1; k = 0 refuses such a
    frame).  Returns int32 [nSample][nM]; raises RuntimeError when the frame is refused or has no consistent association."""
    asg, _, _, method, _, _, _, maxCluster = _engine().hybrid_sample_assoc([costMatrix], [nL], [nM], nSample, k, seed=seed, frame_key=[0])
    if method[0] == -1:
        raise RuntimeError(f"hybridSampleAssoc: frame refused: its largest cluster has {int(maxCluster[0])} measurements")
    if method[0] == -2:
        raise RuntimeError("hybridSampleAssoc: the frame has no consistent association (some cluster has no feasible assignment)")
    return asg[0]


def hybridFrontierProb(costMatrix, nL, nM, k):
    """Not in the reference: hybridExactProb with the frontier tier first: exact on every gated cluster of at most 64 measurements
    whose rows, in the greedy order, keep at most 16 columns open, and on every other of at most 20; assignmentProb(k) on what is
    left (k = 0: such a frame is refused).  Returns probs[nM][nL+1]; raises RuntimeError only when the frame is refused; an
    infeasible frame comes back as all zeros."""
    out, method, _, _, maxCluster, _, _ = _engine().hybrid_frontier_probs([costMatrix], [nL], [nM], k)
    if method[0] == -1:
        raise RuntimeError(f"hybridFrontierProb: frame refused: its largest cluster has {int(maxCluster[0])} measurements")
    return out[0]


def hybridExactProb(costMatrix, nL, nM, k):
    """Not in the reference: hybridProb with the exact tier for clusters of 17 .. 20 measurements in between: exact on every gated
    cluster of at most 20 measurements, assignmentProb(k) on each larger one alone (k = 0: such a frame is refused).  Returns
    probs[nM][nL+1]; raises RuntimeError only when the frame is refused; an infeasible frame comes back as all zeros."""
    out, method, _, _, maxCluster, _ = _engine().hybrid_exact_probs([costMatrix], [nL], [nM], k)
    if method[0] == -1:
        raise RuntimeError(f"hybridExactProb: frame refused: its largest cluster has {int(maxCluster[0])} measurements")
    return out[0]
