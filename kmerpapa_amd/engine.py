"""ctypes binding of ``libkmerpapa_hip.so`` (C-ABI in include/kmerpapa_hip.h).

This is the only door from the Python host layer into the GPU.  There is no CPU
fallback: if the HIP library is missing or no GPU is visible, :func:`load` / :class:`Device`
raise, loudly.

Host-side responsibilities kept here:
  * k-mer ordering: count tables go to the device in KmerEnumeration order (position 0
    fastest, nucleotide digit = index in ``code[g]``), see ``kmer_order``;
  * pass planning: lane groups are packed into passes that fit device memory
    (4 bytes per cell per lane: the f32 train score of the value-only sweep, plus a
    per-lane backtrack node pool; ``Plan.info["bytes_per_lane"]``);
  * sharding: groups are spread over the visible GPUs, one host thread per GPU
    (ctypes releases the GIL during every call), no collective needed.
"""
import atexit
import ctypes
import os
import threading
import time

import numpy as np

from .pattern_utils import code_no

_HERE = os.path.dirname(os.path.abspath(__file__))
# KMERPAPA_LIB selects another build of the same C-ABI (e.g. the -DKP_STAMPS diagnostic build)
LIB_PATH = os.environ.get("KMERPAPA_LIB") or os.path.join(_HERE, "libkmerpapa_hip.so")
MAX_GROUP_LANES = 8

_lib = None
_lib_lock = threading.Lock()


class KPError(RuntimeError):
    """Error reported by the C-ABI (carries the KP_E_* code)."""

    def __init__(self, code, msg):
        super().__init__(f"kmerpapa_hip error {code}: {msg}")
        self.code = code


class KPGroup(ctypes.Structure):
    _fields_ = [("fold", ctypes.c_int32), ("n_lanes", ctypes.c_int32), ("alpha", ctypes.c_double),
                ("beta", ctypes.c_double), ("penalty", ctypes.c_double * MAX_GROUP_LANES)]


class KPPlanInfo(ctypes.Structure):
    _fields_ = [("npat", ctypes.c_uint64), ("nblocks", ctypes.c_uint64), ("n_kmers", ctypes.c_uint64),
                ("block", ctypes.c_uint32), ("block_pad", ctypes.c_uint32), ("k", ctypes.c_int32),
                ("low_positions", ctypes.c_int32), ("max_level", ctypes.c_int32),
                ("high_levels", ctypes.c_int32), ("pairs_total", ctypes.c_double),
                ("pairs_high", ctypes.c_double), ("bytes_per_lane", ctypes.c_uint64),
                ("lanes_per_workgroup", ctypes.c_uint32), ("pad_", ctypes.c_uint32)]


class KPPassStats(ctypes.Structure):
    _fields_ = [("dp_ms", ctypes.c_double), ("backtrack_ms", ctypes.c_double), ("total_ms", ctypes.c_double),
                ("units", ctypes.c_uint64), ("dp_launches", ctypes.c_uint64), ("alg_bytes", ctypes.c_double),
                ("gather_bytes", ctypes.c_double)]


class KPGreedyLane(ctypes.Structure):
    _fields_ = [("fold", ctypes.c_int32), ("chain", ctypes.c_int32), ("alpha", ctypes.c_double),
                ("beta", ctypes.c_double), ("penalty", ctypes.c_double)]


class KPGreedyStats(ctypes.Structure):
    _fields_ = [("hist_ms", ctypes.c_double), ("total_ms", ctypes.c_double), ("frontier_kmers", ctypes.c_uint64),
                ("items", ctypes.c_uint64), ("depths", ctypes.c_uint32), ("batches", ctypes.c_uint32)]


class KPApplyStats(ctypes.Structure):
    _fields_ = [("unmatched", ctypes.c_uint64), ("multi", ctypes.c_uint64), ("overlap_pairs", ctypes.c_uint64),
                ("outside_super", ctypes.c_uint64), ("assign_ms", ctypes.c_double), ("tiles", ctypes.c_uint32),
                ("lds_counters", ctypes.c_uint32)]


class KPSeqStats(ctypes.Structure):
    _fields_ = [("windows", ctypes.c_uint64), ("windows_invalid", ctypes.c_uint64), ("sites", ctypes.c_uint64),
                ("sites_skipped", ctypes.c_uint64), ("items", ctypes.c_uint64), ("scan_ms", ctypes.c_double),
                ("tile", ctypes.c_uint32), ("path", ctypes.c_uint32)]


class KPPredStats(ctypes.Structure):
    _fields_ = [("assigned", ctypes.c_uint64), ("unmatched", ctypes.c_uint64), ("invalid", ctypes.c_uint64),
                ("items", ctypes.c_uint64), ("lut_bytes", ctypes.c_uint64), ("lut_ms", ctypes.c_double),
                ("scan_ms", ctypes.c_double), ("tile", ctypes.c_uint32), ("path", ctypes.c_uint32)]


class KPSpecStats(ctypes.Structure):
    _fields_ = list(KPPredStats._fields_)


class KPSpecSimStats(ctypes.Structure):
    _fields_ = [("windows", ctypes.c_uint64), ("hits", ctypes.c_uint64), ("items", ctypes.c_uint64),
                ("count_ms", ctypes.c_double), ("write_ms", ctypes.c_double)]


class KPSpecNullStats(ctypes.Structure):
    _fields_ = [("windows", ctypes.c_uint64), ("draws", ctypes.c_uint64), ("hits", ctypes.c_uint64),
                ("items", ctypes.c_uint64), ("passes", ctypes.c_uint32), ("reps_per_pass", ctypes.c_uint32),
                ("null_ms", ctypes.c_double)]


class KPSpecCodingStats(ctypes.Structure):
    _fields_ = [("items", ctypes.c_uint64), ("positions", ctypes.c_uint64), ("pairs", ctypes.c_uint64),
                ("scan_ms", ctypes.c_double), ("path", ctypes.c_uint32)]


class KPSpecCodingNullStats(ctypes.Structure):
    _fields_ = [("positions", ctypes.c_uint64), ("drawing", ctypes.c_uint64), ("hits", ctypes.c_uint64),
                ("unclassed", ctypes.c_uint64), ("passes", ctypes.c_uint32), ("reps_per_pass", ctypes.c_uint32),
                ("stage_ms", ctypes.c_double), ("draw_ms", ctypes.c_double)]


class KPISpecStats(ctypes.Structure):
    _fields_ = list(KPPredStats._fields_) + [("sites", ctypes.c_uint64), ("sites_skipped", ctypes.c_uint64),
                                             ("sites_ms", ctypes.c_double)]


SEQ_PATH_LDS, SEQ_PATH_GLOBAL = 1, 2  # KPSeqStats.path of a device scan (0: host, or no scan yet)
PRED_PATH_LDS, PRED_PATH_GLOBAL = 1, 2  # KPPredStats.path of a device regions call (0: host, or none yet)
SPEC_PATH_LDS, SPEC_PATH_GLOBAL = 1, 2  # KPSpecStats.path, the same
ISPEC_PATH_LDS, ISPEC_PATH_GLOBAL = 1, 2  # KPISpecStats.path, the same
ISPEC_INS, ISPEC_DEL = 0, 1  # kp_ispec_begin's pattern kinds

EXPORTS = ["kp_last_error", "kp_device_count", "kp_create", "kp_destroy", "kp_device_mem", "kp_plan_create",
           "kp_plan_destroy", "kp_plan_get_info", "kp_plan_host", "kp_plan_host_counts", "kp_set_counts", "kp_counts_begin", "kp_counts_fold", "kp_pass",
           "kp_reserve_lanes", "kp_last_pass_stats", "kp_last_launch_ms", "kp_fit_leaves", "kp_dump_lane", "kp_gather_cells", "kp_fold_split",
           "kp_fold_sample", "kp_math_log", "kp_math_libm", "kp_kmer_parse", "kp_kmer_table_info", "kp_kmer_table_copy", "kp_kmer_table_free",
           "kp_format_long_rows", "kp_py_repr", "kp_device_groups", "kp_allkmers_cv", "kp_block_order_check",
           "kp_plan_block_check", "kp_block_list_host", "kp_greedy", "kp_greedy_leaves", "kp_greedy_host",
           "kp_greedy_last_stats", "kp_apply", "kp_apply_host", "kp_seq_begin", "kp_seq_scan", "kp_seq_sites",
           "kp_seq_end", "kp_seq_last_stats", "kp_seq_host", "kp_pred_begin", "kp_pred_regions", "kp_pred_track",
           "kp_pred_sites", "kp_pred_end", "kp_pred_last_stats", "kp_pred_host", "kp_seq_begin_typed",
           "kp_seq_sites_typed", "kp_seq_end_typed", "kp_spec_begin", "kp_spec_regions", "kp_spec_track",
           "kp_spec_sites", "kp_spec_end", "kp_spec_last_stats", "kp_spec_host", "kp_spec_simulate", "kp_spec_last_sim",
           "kp_spec_null", "kp_spec_last_null", "kp_spec_coding", "kp_spec_coding_sites", "kp_spec_last_coding",
           "kp_spec_coding_null", "kp_spec_last_coding_null", "kp_seq_begin_indel", "kp_seq_begin_strands",
           "kp_seq_indels", "kp_seq_indel_host", "kp_ispec_begin", "kp_ispec_regions", "kp_ispec_track",
           "kp_ispec_sites", "kp_ispec_end", "kp_ispec_last_stats", "kp_ispec_host"]

INDEL_PLACE = {"left": 0, "right": 1, "sample": 2}  # kp_seq_indels' place


def load():
    """Load libkmerpapa_hip.so (built in-tree by __graft_entry__.build())."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                              "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
        L = ctypes.CDLL(LIB_PATH)
        vp = ctypes.c_void_p
        u64p = ctypes.POINTER(ctypes.c_uint64)
        L.kp_last_error.restype = ctypes.c_char_p
        L.kp_device_count.argtypes = [ctypes.POINTER(ctypes.c_int)]
        L.kp_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
        L.kp_destroy.argtypes = [vp]
        L.kp_destroy.restype = None
        L.kp_device_mem.argtypes = [vp, u64p, u64p]
        L.kp_plan_create.argtypes = [vp, ctypes.c_char_p, ctypes.c_uint32, ctypes.POINTER(vp)]
        L.kp_plan_destroy.argtypes = [vp]
        L.kp_plan_destroy.restype = None
        L.kp_plan_get_info.argtypes = [vp, ctypes.POINTER(KPPlanInfo)]
        L.kp_plan_host.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.POINTER(KPPlanInfo)]
        if hasattr(L, "kp_plan_host_counts"):  # (older builds loaded through KMERPAPA_LIB for A/B timing lack it)
            L.kp_plan_host_counts.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_int,
                                              ctypes.POINTER(KPPlanInfo)]
        L.kp_block_order_check.argtypes = [ctypes.c_char_p, ctypes.c_uint32, u64p]
        L.kp_plan_block_check.argtypes = [vp, u64p]
        if hasattr(L, "kp_block_list_host"):  # (older builds loaded through KMERPAPA_LIB lack it)
            L.kp_block_list_host.argtypes = [ctypes.c_char_p, ctypes.c_uint32, vp, vp]
        L.kp_kmer_parse.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_char_p, ctypes.c_int,
                                    ctypes.POINTER(vp)]
        L.kp_kmer_table_info.argtypes = [vp, u64p, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64),
                                         ctypes.POINTER(ctypes.c_int64)]
        L.kp_kmer_table_copy.argtypes = [vp, vp, vp, vp]
        L.kp_kmer_table_free.argtypes = [vp]
        L.kp_kmer_table_free.restype = None
        L.kp_set_counts.argtypes = [vp, vp, vp, ctypes.c_uint64, ctypes.c_int, ctypes.c_int]
        L.kp_counts_begin.argtypes = [vp, vp, vp, ctypes.c_uint64, ctypes.c_int, ctypes.c_int]
        L.kp_counts_fold.argtypes = [vp, ctypes.c_int, vp, vp, ctypes.c_uint64]
        L.kp_pass.argtypes = [vp, ctypes.POINTER(KPGroup), ctypes.c_int, vp, vp, vp]
        L.kp_last_pass_stats.argtypes = [vp, ctypes.POINTER(KPPassStats)]
        L.kp_device_groups.argtypes = [ctypes.POINTER(KPGroup), ctypes.c_int, ctypes.c_int, vp, vp, vp, ctypes.c_int,
                                       ctypes.POINTER(ctypes.c_int)]
        L.kp_last_launch_ms.argtypes = [vp, vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        L.kp_reserve_lanes.argtypes = [vp, ctypes.c_uint32]
        L.kp_fit_leaves.argtypes = [vp, ctypes.c_uint32, vp, ctypes.c_uint64, u64p]
        L.kp_dump_lane.argtypes = [vp, ctypes.c_uint32, vp, vp]
        L.kp_gather_cells.argtypes = [vp, ctypes.c_uint32, vp, ctypes.c_uint64, vp]
        L.kp_fold_split.argtypes = [vp, ctypes.POINTER(ctypes.c_int32), vp, ctypes.c_uint64, ctypes.c_int, vp]
        if hasattr(L, "kp_math_log"):  # (older builds loaded through KMERPAPA_LIB for A/B timing lack it)
            L.kp_math_log.argtypes = [vp, vp, vp, ctypes.c_uint64]
        if hasattr(L, "kp_math_libm"):
            L.kp_math_libm.argtypes = [vp, vp, vp, ctypes.c_uint64, ctypes.c_int]
        L.kp_format_long_rows.argtypes = [vp, ctypes.c_int, vp, vp, vp, ctypes.c_uint64, vp, vp, ctypes.c_uint64, vp,
                                          ctypes.c_uint64, u64p]
        L.kp_py_repr.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_uint64, u64p]
        L.kp_allkmers_cv.argtypes = [vp, vp, vp, ctypes.c_uint64, ctypes.c_int, vp, vp, ctypes.c_int, vp, vp]
        L.kp_fold_sample.argtypes = [vp, ctypes.POINTER(ctypes.c_int32), vp, ctypes.c_uint64, ctypes.c_uint64, vp]
        if hasattr(L, "kp_greedy"):  # (older builds loaded through KMERPAPA_LIB for A/B timing lack it)
            L.kp_greedy.argtypes = [vp, ctypes.c_char_p, vp, vp, ctypes.c_uint64, ctypes.c_int,
                                    ctypes.POINTER(KPGreedyLane), ctypes.c_int, vp, vp, vp]
            L.kp_greedy_leaves.argtypes = [vp, ctypes.c_uint32, vp, ctypes.c_uint64, u64p]
            L.kp_greedy_last_stats.argtypes = [vp, ctypes.POINTER(KPGreedyStats)]
            L.kp_greedy_host.argtypes = [ctypes.c_char_p, vp, vp, ctypes.c_uint64, ctypes.c_int,
                                         ctypes.POINTER(KPGreedyLane), ctypes.c_int, vp, vp, vp]
        if hasattr(L, "kp_apply"):  # (older builds loaded through KMERPAPA_LIB for A/B timing lack it)
            tail = [ctypes.c_int, vp, ctypes.c_uint32, ctypes.c_uint64, vp, vp, vp, ctypes.c_uint64, ctypes.c_int, vp, vp,
                    vp, vp, vp, ctypes.POINTER(KPApplyStats)]
            L.kp_apply.argtypes = [vp] + tail
            L.kp_apply_host.argtypes = tail
        if hasattr(L, "kp_seq_begin"):  # (older builds loaded through KMERPAPA_LIB for A/B timing lack it)
            L.kp_seq_begin.argtypes = [vp, ctypes.c_int, ctypes.c_int]
            L.kp_seq_scan.argtypes = [vp, vp, ctypes.c_uint64, vp, vp, ctypes.c_uint64]
            L.kp_seq_sites.argtypes = [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64]
            L.kp_seq_end.argtypes = [vp, vp, vp]
            L.kp_seq_last_stats.argtypes = [vp, ctypes.POINTER(KPSeqStats)]
            L.kp_seq_host.argtypes = [ctypes.c_int, ctypes.c_int, vp, ctypes.c_uint64, ctypes.c_int, vp, vp,
                                      ctypes.c_uint64, vp, ctypes.c_uint64, vp, vp, ctypes.POINTER(KPSeqStats)]
        if hasattr(L, "kp_pred_begin"):  # (older builds loaded through KMERPAPA_LIB for A/B timing lack it)
            u64 = ctypes.c_uint64
            L.kp_pred_begin.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_uint32, u64]
            L.kp_pred_regions.argtypes = [vp, vp, u64, vp, vp, u64, vp, vp, vp, vp]
            L.kp_pred_track.argtypes = [vp, vp, u64, u64, u64, vp]
            L.kp_pred_sites.argtypes = [vp, vp, u64, vp, u64, vp]
            L.kp_pred_end.argtypes = [vp]
            L.kp_pred_last_stats.argtypes = [vp, ctypes.POINTER(KPPredStats)]
            L.kp_pred_host.argtypes = [ctypes.c_int, ctypes.c_int, vp, ctypes.c_uint32, u64, vp, u64, vp, vp, u64, vp, vp,
                                       vp, vp, u64, u64, vp, vp, u64, vp, ctypes.POINTER(KPPredStats)]
        if hasattr(L, "kp_spec_begin"):  # (older builds loaded through KMERPAPA_LIB for A/B timing lack it)
            u64 = ctypes.c_uint64
            L.kp_seq_begin_typed.argtypes = [vp, ctypes.c_int, ctypes.c_int]
            L.kp_seq_sites_typed.argtypes = [vp, vp, u64, vp, vp, u64]
            L.kp_seq_end_typed.argtypes = [vp, vp, vp]
            L.kp_spec_begin.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_uint32]
            L.kp_spec_regions.argtypes = [vp, vp, u64, vp, vp, u64, vp, vp, vp, vp]
            L.kp_spec_track.argtypes = [vp, vp, u64, u64, u64, vp]
            L.kp_spec_sites.argtypes = [vp, vp, u64, vp, vp, u64, vp]
            L.kp_spec_end.argtypes = [vp]
            L.kp_spec_last_stats.argtypes = [vp, ctypes.POINTER(KPSpecStats)]
            L.kp_spec_host.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_uint32, vp, u64, vp, vp, u64, vp, vp, vp,
                                       vp, u64, u64, vp, vp, vp, u64, vp, ctypes.POINTER(KPSpecStats)]
        if hasattr(L, "kp_spec_simulate"):  # (older builds loaded through KMERPAPA_LIB for A/B timing lack it)
            u64, u32 = ctypes.c_uint64, ctypes.c_uint32
            L.kp_spec_simulate.argtypes = [vp, vp, u64, u32, vp, vp, u64, vp, ctypes.c_double, u64, u32, u64, vp, vp, vp,
                                           u64p]
            L.kp_spec_last_sim.argtypes = [vp, ctypes.POINTER(KPSpecSimStats)]
        if hasattr(L, "kp_spec_null"):  # (older builds loaded through KMERPAPA_LIB for A/B timing lack it)
            u64, u32 = ctypes.c_uint64, ctypes.c_uint32
            L.kp_spec_null.argtypes = [vp, vp, u64, u32, vp, vp, u64, vp, ctypes.c_double, u64, u32, u32, ctypes.c_int, vp]
            L.kp_spec_last_null.argtypes = [vp, ctypes.POINTER(KPSpecNullStats)]
        if hasattr(L, "kp_spec_coding"):  # (older builds loaded through KMERPAPA_LIB for A/B timing lack it)
            u64, u32 = ctypes.c_uint64, ctypes.c_uint32
            table = [vp, vp, u64, vp, vp, u64, vp, vp, u64, u32]  # ctx, the contig and the transcript table, splice
            L.kp_spec_coding.argtypes = table + [vp, vp, vp, vp]
            L.kp_spec_coding_sites.argtypes = table + [vp, vp, vp, u64, vp, vp, vp]
            L.kp_spec_last_coding.argtypes = [vp, ctypes.POINTER(KPSpecCodingStats)]
        if hasattr(L, "kp_spec_coding_null"):  # (older builds loaded through KMERPAPA_LIB for A/B timing lack it)
            u64, u32 = ctypes.c_uint64, ctypes.c_uint32
            L.kp_spec_coding_null.argtypes = [vp, vp, u64, u32, vp, vp, u64, vp, vp, u64, u32, vp, ctypes.c_double, u64, u32,
                                              u32, vp]
            L.kp_spec_last_coding_null.argtypes = [vp, ctypes.POINTER(KPSpecCodingNullStats)]
        if hasattr(L, "kp_seq_indels"):  # (older builds loaded through KMERPAPA_LIB for A/B timing lack it)
            u64, u32 = ctypes.c_uint64, ctypes.c_uint32
            L.kp_seq_begin_indel.argtypes = [vp, ctypes.c_int, ctypes.c_int]
            L.kp_seq_begin_strands.argtypes = [vp, ctypes.c_int, ctypes.c_int]
            sites = [vp, vp, vp, vp, vp, u64, ctypes.c_int, u64]  # pos, del_len, key, ins_off, ins, n, place, seed
            L.kp_seq_indels.argtypes = [vp, vp, u64, u32] + sites + [vp]
            L.kp_seq_indel_host.argtypes = [ctypes.c_int, ctypes.c_int, vp, u64, u32, ctypes.c_int, vp, vp, u64] + sites + \
                [vp, vp, vp, ctypes.POINTER(KPSeqStats)]
        if hasattr(L, "kp_ispec_begin"):  # (older builds loaded through KMERPAPA_LIB for A/B timing lack it)
            u64, u32 = ctypes.c_uint64, ctypes.c_uint32
            sites = [vp, vp, vp, vp, vp, u64, ctypes.c_int, u64]  # pos, del_len, key, ins_off, ins, n, place, seed
            L.kp_ispec_begin.argtypes = [vp, ctypes.c_int, vp, vp, u32]
            L.kp_ispec_regions.argtypes = [vp, vp, u64, vp, vp, u64, vp, vp, vp, vp]
            L.kp_ispec_track.argtypes = [vp, vp, u64, u64, u64, vp]
            L.kp_ispec_sites.argtypes = [vp, vp, u64, u32] + sites + [vp, vp]
            L.kp_ispec_end.argtypes = [vp]
            L.kp_ispec_last_stats.argtypes = [vp, ctypes.POINTER(KPISpecStats)]
            L.kp_ispec_host.argtypes = [ctypes.c_int, vp, vp, u32, vp, u64, u32, vp, vp, u64, vp, vp, vp, vp, u64, u64, vp] + \
                sites + [vp, vp, ctypes.POINTER(KPISpecStats)]
        for name in EXPORTS:
            if not hasattr(L, name):
                continue
            if name not in ("kp_destroy", "kp_plan_destroy", "kp_last_error", "kp_kmer_table_free"):
                getattr(L, name).restype = ctypes.c_int
        _lib = L
        return L


def _check(rc):
    if rc != 0:
        raise KPError(rc, load().kp_last_error().decode(errors="replace"))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


# launch knobs read by the library (csrc/kp_pass.h, kp_plan.h, kp_plan_dev.h; every setting gives the same scores; they change timing)
LAUNCH_KNOBS = ("KP_DP_THREADS", "KP_LANES_PER_WG", "KP_XCD_REMAP", "KP_LANE_SPLIT", "KP_NT_STORE", "KP_NT_SLOW",
                "KP_BLOCK_PERM", "KP_BLOCK_ORDER", "KP_BLOCK_TILE", "KP_BLOCK_CLASS", "KP_LOW_ORDER", "KP_EXACT_LOGS",
               "KP_CLASS_STREAMS", "KP_NT_SLOW_H", "KP_LDS_BUDGET", "KP_WIDE_SPLIT", "KP_HPD")


_toolchain = None


def toolchain_version():
    """``hipcc --version`` of the compiler that built the library, recorded by the build
    (csrc/kp_toolchain.txt; part of kernel_tag)."""
    global _toolchain
    if _toolchain is None:
        try:
            with open(os.path.join(_HERE, "csrc", "kp_toolchain.txt")) as f:
                _toolchain = f.read()
        except OSError:
            _toolchain = "toolchain: not recorded (library not built by csrc/Makefile)"
    return _toolchain


def kernel_tag():
    """Short hash of everything that decides the sweep's launches: the library's tracked
    sources (csrc/kp_*.h, kp_*.hip, gen_logdata.py, Makefile, the C-ABI header), the log
    constants generated into kp_logdata.h (without its comment lines, which name the host
    libm's path), the compiler (``hipcc --version``) and the launch knobs set in the
    environment.  Ties PMC profiles (profiles/*/pmc_*.json) to the exact build and launch
    configuration."""
    import glob
    import hashlib
    h = hashlib.sha1()
    csrc = os.path.join(_HERE, "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "kp_*.h")) + glob.glob(os.path.join(csrc, "kp_*.hip")))
    files = [f for f in files if os.path.basename(f) != "kp_logdata.h"]
    files += [os.path.join(csrc, "gen_logdata.py"), os.path.join(csrc, "Makefile"),
              os.path.join(os.path.dirname(_HERE), "include", "kmerpapa_hip.h")]
    for fn in files:
        if not os.path.isfile(fn):  # (an installed copy may lack a build file: hash its absence)
            h.update(b"missing:" + os.path.basename(fn).encode())
            continue
        with open(fn, "rb") as f:
            h.update(os.path.basename(fn).encode() + b"\0" + f.read())
    gen = os.path.join(csrc, "kp_logdata.h")
    if os.path.isfile(gen):
        with open(gen, "rb") as f:
            h.update(b"kp_logdata.h\0" + b"".join(x for x in f.readlines() if not x.lstrip().startswith(b"//")))
    h.update(toolchain_version().encode())
    for k in LAUNCH_KNOBS:
        h.update(f"{k}={os.environ.get(k, '')}".encode())
    return h.hexdigest()[:12]


def fold_split(colors, n_folds, prng):
    """Fold split of ``colors`` with the caller's numpy ``RandomState`` stream, in C++
    (``kp_fold_split``; bit-identical to CV_tools.py:5-62).  ``prng`` is advanced exactly
    as numpy's own draws would advance it.  Returns uint64 ``[n, n_folds]``."""
    L = load()
    st = prng.get_state(legacy=True)
    if st[0] != "MT19937":
        raise ValueError("fold split needs a legacy MT19937 RandomState")
    key = np.array(st[1], dtype=np.uint32)
    pos = ctypes.c_int32(int(st[2]))
    col = np.ascontiguousarray(colors, dtype=np.uint64)
    out = np.zeros((col.shape[0], int(n_folds)), dtype=np.uint64)
    _check(L.kp_fold_split(_ptr(key), ctypes.byref(pos), _ptr(col), ctypes.c_uint64(col.shape[0]), int(n_folds),
                           _ptr(out)))
    prng.set_state((st[0], key, pos.value, st[3], st[4]))
    return out


def fold_sample(colors, m, prng):
    """One fold of the split: ``m`` balls drawn colour by colour from ``colors``
    (CV_tools.py sample :5-27) with the caller's numpy ``RandomState`` stream, in C++
    (``kp_fold_sample``).  Returns uint64 ``[n]``; ``prng`` advances as numpy's would."""
    L = load()
    st = prng.get_state(legacy=True)
    if st[0] != "MT19937":
        raise ValueError("fold split needs a legacy MT19937 RandomState")
    key = np.array(st[1], dtype=np.uint32)
    pos = ctypes.c_int32(int(st[2]))
    col = np.ascontiguousarray(colors, dtype=np.uint64)
    out = np.zeros(col.shape[0], dtype=np.uint64)
    _check(L.kp_fold_sample(_ptr(key), ctypes.byref(pos), _ptr(col), ctypes.c_uint64(col.shape[0]),
                            ctypes.c_uint64(int(m)), _ptr(out)))
    prng.set_state((st[0], key, pos.value, st[3], st[4]))
    return out


def parse_kmer_counts(text, columns, super_pattern=None, length=0):
    """Parse k-mer count text with the native reader (``kp_kmer_parse``, C++).

    ``text``: bytes of a "kmer count" (``columns=2``) or "kmer positive background"
    (``columns=3``) file.  Returns ``(k, codes uint64, c0 int64, c1 int64, total0,
    total1)`` with codes sorted (2 bits per letter, first letter most significant).
    Input errors raise ``ValueError`` with the parser's message."""
    L = load()
    buf = bytes(text)
    t = ctypes.c_void_p()
    sp = super_pattern.encode("ascii") if super_pattern else None
    rc = L.kp_kmer_parse(buf, ctypes.c_uint64(len(buf)), int(columns), sp, int(length or 0), ctypes.byref(t))
    if rc != 0:
        raise ValueError(L.kp_last_error().decode(errors="replace"))
    try:
        n, k = ctypes.c_uint64(), ctypes.c_int32()
        t0, t1 = ctypes.c_int64(), ctypes.c_int64()
        _check(L.kp_kmer_table_info(t, ctypes.byref(n), ctypes.byref(k), ctypes.byref(t0), ctypes.byref(t1)))
        codes = np.zeros(n.value, np.uint64)
        c0 = np.zeros(n.value, np.int64)
        c1 = np.zeros(n.value, np.int64)
        _check(L.kp_kmer_table_copy(t, _ptr(codes), _ptr(c0), _ptr(c1)))
    finally:
        L.kp_kmer_table_free(t)
    return k.value, codes, c0, c1, t0.value, t1.value


def py_repr(x):
    """Python repr() of every float64 in ``x`` by the native formatter (kp_py_repr); a list
    of str.  Host code, no GPU (a check of kp_format_long_rows' float format)."""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    cap = 40 * x.size + 1
    buf = ctypes.create_string_buffer(cap)
    n = ctypes.c_uint64()
    _check(load().kp_py_repr(_ptr(x), ctypes.c_uint64(x.size), buf, ctypes.c_uint64(cap), ctypes.byref(n)))
    return buf.raw[:n.value].decode("ascii").split("\n")[:-1]


def format_long_rows(kmers, c_neg, c_pos, pid, tails):
    """The -l output rows (kp_format_long_rows): ``kmers`` uint8 ``[n, k]`` letters,
    ``c_neg``/``c_pos`` int64 ``[n]``, ``pid`` ``[n]`` = index into ``tails`` (list of
    str, each " pattern p_neg p_pos p_rate\n").  Returns the text as bytes; a row with no
    counts raises ZeroDivisionError, as the reference's formula does."""
    kmers = np.ascontiguousarray(kmers, dtype=np.uint8)
    n, k = kmers.shape
    c_neg = np.ascontiguousarray(c_neg, dtype=np.int64)
    c_pos = np.ascontiguousarray(c_pos, dtype=np.int64)
    pid = np.ascontiguousarray(pid, dtype=np.uint32)
    tb = [t.encode("ascii") for t in tails]
    off = np.zeros(len(tb) + 1, np.uint64)
    off[1:] = np.cumsum([len(t) for t in tb])
    tail_bytes = b"".join(tb) or b"\0"
    lens = np.array([len(t) for t in tb] or [0], np.int64)
    cap = int(n * (k + 3 * 32) + (lens[pid].sum() if n else 0)) + 1
    out = np.empty(cap, np.uint8)  # (not zeroed: only the w bytes written are returned)
    w = ctypes.c_uint64()
    rc = load().kp_format_long_rows(kmers.ctypes.data_as(ctypes.c_void_p), int(k), _ptr(c_neg), _ptr(c_pos),
                                    _ptr(pid), ctypes.c_uint64(n), tail_bytes, _ptr(off), ctypes.c_uint64(len(tb)),
                                    _ptr(out), ctypes.c_uint64(cap), ctypes.byref(w))
    if rc != 0:
        msg = load().kp_last_error().decode(errors="replace")
        if "division by zero" in msg:
            raise ZeroDivisionError("float division by zero")
        raise KPError(rc, msg)
    return out[:w.value].tobytes()


def plan_info(gen_pat, max_block=0):
    """The plan's info (cells, blocks, device bytes per lane, ...) built on the host only
    (kp_plan_host): no GPU is touched."""
    info = KPPlanInfo()
    _check(load().kp_plan_host(gen_pat.encode(), ctypes.c_uint32(max_block), ctypes.byref(info)))
    return {name: getattr(info, name) for name, _ in KPPlanInfo._fields_}


def shard_width(gen_pat, itype=np.uint32, max_block=0):
    """Lanes one sweep workgroup holds for ``gen_pat``'s lattice at count width ``itype``
    (kp_plan_host_counts, host only): the group size shard.assign_lanes deals whole.  A pure
    function of the lattice and the count width, so every rank of a job computes the same."""
    info = KPPlanInfo()
    _check(load().kp_plan_host_counts(gen_pat.encode(), ctypes.c_uint32(max_block), int(np.dtype(itype).itemsize),
                                      ctypes.byref(info)))
    return int(info.lanes_per_workgroup)


def counts_itype(M):
    """Count width of a run's counts: an array, a FoldFeed, or None (uint32)."""
    if isinstance(M, FoldFeed):
        return M.M_all.dtype
    return np.asarray(M).dtype if M is not None else np.dtype(np.uint32)


def block_order_check(gen_pat, max_block=0):
    """Blocks of ``gen_pat``'s lattice whose closed-form block-list slot (the rule the
    device builds the list by, kp_blocks_kernel) differs from the host's block walk
    (kp_block_order_check, host code): 0 when the two agree."""
    n = ctypes.c_uint64()
    _check(load().kp_block_order_check(gen_pat.encode(), ctypes.c_uint32(max_block), ctypes.byref(n)))
    return n.value


def block_list_host(gen_pat, max_block=0):
    """The block list of ``gen_pat``'s lattice as the host walks it (kp_block_list_host, host
    code; the order the block-list knobs in the environment select): ``(hlist, hoff)``, the
    blocks in list order and the level offsets into that list."""
    info = KPPlanInfo()
    _check(load().kp_plan_host(gen_pat.encode(), ctypes.c_uint32(max_block), ctypes.byref(info)))
    hlist = np.zeros(info.nblocks, dtype=np.uint32)
    hoff = np.zeros(info.high_levels + 1, dtype=np.uint64)
    _check(load().kp_block_list_host(gen_pat.encode(), ctypes.c_uint32(max_block), _ptr(hlist), _ptr(hoff)))
    return hlist, hoff


def _group_array(groups):
    """``groups`` (list of ``(fold, alpha, beta, penalties)``; ``beta`` may be a callable) as
    the C-ABI's kp_group array; returns it and the number of lanes."""
    arr = (KPGroup * len(groups))()
    nl = 0
    for i, (fold, alpha, beta, pens) in enumerate(groups):
        pens = list(pens)
        if not 1 <= len(pens) <= MAX_GROUP_LANES:
            raise ValueError("a group holds 1..8 penalties")
        arr[i].fold = int(fold)
        arr[i].n_lanes = len(pens)
        arr[i].alpha = float(alpha)
        arr[i].beta = float(beta() if callable(beta) else beta)
        for j, c in enumerate(pens):
            arr[i].penalty[j] = float(c)
        nl += len(pens)
    return arr, nl


def device_groups(groups, width):
    """The workgroups (device groups) kp_pass runs ``groups`` as, at ``width`` lanes per
    workgroup (kp_device_groups, host code): a list of ``(lane0, lanes, mixed_lanes)``."""
    arr, nl = _group_array(groups)
    cap = nl
    lane0 = np.zeros(cap, np.int32)
    nls = np.zeros(cap, np.int32)
    nl2 = np.zeros(cap, np.int32)
    n = ctypes.c_int()
    _check(load().kp_device_groups(arr, len(groups), width, _ptr(lane0), _ptr(nls), _ptr(nl2), cap, ctypes.byref(n)))
    return [(int(lane0[i]), int(nls[i]), int(nl2[i])) for i in range(n.value)]


def device_count():
    n = ctypes.c_int(0)
    _check(load().kp_device_count(ctypes.byref(n)))
    return n.value


def visible_devices():
    """GPUs the DP may use: $KMERPAPA_DEVICES (comma list) or every visible device."""
    env = os.environ.get("KMERPAPA_DEVICES")
    if env:
        return [int(x) for x in env.split(",") if x.strip()]
    return list(range(device_count()))


def _seq_bytes(seq):
    seq = np.ascontiguousarray(seq, dtype=np.uint8).reshape(-1)
    return seq, ctypes.c_uint64(seq.shape[0])


def _alt_bytes(alt, n):
    if isinstance(alt, (bytes, bytearray, str)):
        alt = np.frombuffer(alt.encode("latin-1") if isinstance(alt, str) else bytes(alt), np.uint8)
    alt = np.ascontiguousarray(alt, dtype=np.uint8).reshape(-1)
    if alt.shape[0] != n:
        raise ValueError("one ALT base per position")
    return alt


class _SeqCalls:
    """The kp_seq_* session calls on ``self._h``: a :class:`Device`'s context, or None for the
    calling thread's host session (:class:`HostSeq`)."""

    _h = None

    def seq_begin(self, k, fold=True):
        """Open a counting session of ``k``-mers (kp_seq_begin); ``fold``: count a window whose
        centre is G or T as its reverse complement (odd ``k`` only)."""
        _check(load().kp_seq_begin(self._h, int(k), int(bool(fold))))
        self._seq_cells = 4 ** int(k)

    def seq_scan(self, seq, regions=None):
        """Count every window of the contig ``seq`` (uint8, one byte per base) whose centre lies
        in ``regions`` (``[m, 2]`` 0-based half-open, sorted and disjoint; None = the whole
        contig) into the background column (kp_seq_scan)."""
        seq, n = _seq_bytes(seq)
        if regions is None:
            _check(load().kp_seq_scan(self._h, _ptr(seq), n, None, None, ctypes.c_uint64(0)))
            return
        reg = np.asarray(regions, dtype=np.uint64).reshape(-1, 2)
        if reg.shape[0] == 0:
            return  # (no region is not "the whole contig")
        rb, re = np.ascontiguousarray(reg[:, 0]), np.ascontiguousarray(reg[:, 1])
        _check(load().kp_seq_scan(self._h, _ptr(seq), n, _ptr(rb), _ptr(re), ctypes.c_uint64(reg.shape[0])))

    def seq_sites(self, seq, pos):
        """Count the window centred at each 0-based position of ``pos`` on the contig ``seq``
        into the positive column, duplicates as often as they occur (kp_seq_sites)."""
        seq, n = _seq_bytes(seq)
        pos = np.ascontiguousarray(pos, dtype=np.uint64).reshape(-1)
        _check(load().kp_seq_sites(self._h, _ptr(seq), n, _ptr(pos), ctypes.c_uint64(pos.shape[0])))

    def seq_end(self, want_pos=True, want_bg=True):
        """Close the session (kp_seq_end).  Returns ``(pos_counts, bg_counts)``, dense uint64
        ``[4^k]`` in code order (None for a column not wanted)."""
        cells = getattr(self, "_seq_cells", 0)
        pos = np.zeros(cells, np.uint64) if want_pos and cells else None
        bg = np.zeros(cells, np.uint64) if want_bg and cells else None
        self._seq_cells = 0
        _check(load().kp_seq_end(self._h, _ptr(pos), _ptr(bg)))
        return pos, bg

    def seq_begin_typed(self, k, fold=True):
        """Open a typed counting session (kp_seq_begin_typed): three positive columns, one per ALT
        slot (:func:`kmerpapa_amd.spectrum.slot_of`), beside the background column."""
        _check(load().kp_seq_begin_typed(self._h, int(k), int(bool(fold))))
        self._seq_cells = 4 ** int(k)

    def seq_sites_typed(self, seq, pos, alt):
        """Count the window centred at each 0-based position of ``pos`` into the column of its ALT
        base ``alt`` (bytes ``ACGTacgt`` on the forward strand) (kp_seq_sites_typed)."""
        seq, n = _seq_bytes(seq)
        pos = np.ascontiguousarray(pos, dtype=np.uint64).reshape(-1)
        alt = _alt_bytes(alt, pos.shape[0])
        _check(load().kp_seq_sites_typed(self._h, _ptr(seq), n, _ptr(pos), _ptr(alt), ctypes.c_uint64(pos.shape[0])))

    def seq_end_typed(self, want_pos=True, want_bg=True):
        """Close a typed session (kp_seq_end_typed).  Returns ``(pos_counts [3, 4^k], bg_counts
        [4^k])``, dense uint64 in code order (None for what is not wanted)."""
        cells = getattr(self, "_seq_cells", 0)
        pos = np.zeros((3, cells), np.uint64) if want_pos and cells else None
        bg = np.zeros(cells, np.uint64) if want_bg and cells else None
        self._seq_cells = 0
        _check(load().kp_seq_end_typed(self._h, _ptr(pos), _ptr(bg)))
        return pos, bg

    def seq_count_typed(self, k, fold, jobs):
        """One whole typed session.  ``jobs``: one ``(seq, regions, sites)`` per contig as
        :meth:`seq_count`'s, ``sites`` being ``(pos, alt)`` or None.  Returns ``(pos_counts,
        bg_counts, stats)``."""
        self.seq_begin_typed(k, fold)
        try:
            for seq, regions, sites in jobs:
                if regions is not False:
                    self.seq_scan(seq, regions)
                if sites is not None and len(sites[0]):
                    self.seq_sites_typed(seq, *sites)
        except BaseException:
            self.seq_end_typed(False, False)
            raise
        pos, bg = self.seq_end_typed()
        return pos, bg, self.seq_stats()

    def seq_stats(self):
        """Figures of the current or last session (kp_seq_last_stats) as a dict."""
        st = KPSeqStats()
        _check(load().kp_seq_last_stats(self._h, ctypes.byref(st)))
        return {name: getattr(st, name) for name, _ in KPSeqStats._fields_}

    def seq_count(self, k, fold, jobs):
        """One whole session.  ``jobs``: one ``(seq, regions, sites)`` per contig -- ``regions``
        as :meth:`seq_scan` takes them, or False for no scan; ``sites`` positions or None.
        Returns ``(pos_counts, bg_counts, stats)``."""
        self.seq_begin(k, fold)
        try:
            for seq, regions, sites in jobs:
                if regions is not False:
                    self.seq_scan(seq, regions)
                if sites is not None and len(sites):
                    self.seq_sites(seq, sites)
        except BaseException:
            self.seq_end(False, False)
            raise
        pos, bg = self.seq_end()
        return pos, bg, self.seq_stats()


    def seq_begin_indel(self, k, both=True):
        """Open an indel session of even ``k`` (kp_seq_begin_indel): columns ins, del_start and
        del_end beside the background; ``both``: every add comes with its mirror on the other strand."""
        _check(load().kp_seq_begin_indel(self._h, int(k), int(bool(both))))
        self._seq_cells = 4 ** int(k)

    def seq_begin_strands(self, k, both=True):
        """Open a plain, unfolded session whose scan adds on both strands if ``both``
        (kp_seq_begin_strands); :meth:`seq_end` closes it."""
        _check(load().kp_seq_begin_strands(self._h, int(k), int(bool(both))))
        self._seq_cells = 4 ** int(k)

    def seq_indels(self, seq, contig, sites, place="left", seed=0, want_resolved=True):
        """Place and count the indels ``sites`` (:func:`indel_sites`) of the contig ``seq`` with index
        ``contig`` (kp_seq_indels).  Returns ``resolved`` uint64 ``[m, 3]``: lo, hi and the chosen
        breakpoint of every site, or None."""
        seq, n = _seq_bytes(seq)
        pos, del_len, ins, ins_off, key = sites
        res = np.zeros((pos.shape[0], 3), np.uint64) if want_resolved else None
        _check(load().kp_seq_indels(self._h, _ptr(seq), n, int(contig), _ptr(pos), _ptr(del_len), _ptr(key), _ptr(ins_off),
                                    _ptr(ins), ctypes.c_uint64(pos.shape[0]), INDEL_PLACE[place], ctypes.c_uint64(int(seed)),
                                    _ptr(res)))
        return res

    def seq_count_indels(self, k, both, jobs, place="left", seed=0):
        """One whole indel session.  ``jobs``: one ``(seq, regions, contig index, sites)`` per contig,
        ``regions`` as :meth:`seq_count`'s, ``sites`` an :func:`indel_sites` tuple or None.  Returns
        ``(pos_counts [3, 4^k], bg_counts, stats, [resolved or None per job])``."""
        self.seq_begin_indel(k, both)
        resolved = []
        try:
            for seq, regions, contig, sites in jobs:
                if regions is not False:
                    self.seq_scan(seq, regions)
                resolved.append(self.seq_indels(seq, contig, sites, place, seed)
                                if sites is not None and len(sites[0]) else None)
        except BaseException:
            self.seq_end_typed(False, False)
            raise
        pos, bg = self.seq_end_typed()
        return pos, bg, self.seq_stats(), resolved

    def seq_count_strands(self, k, both, jobs):
        """One whole background session of both strands (or, ``both`` False, of the forward strand
        unfolded).  ``jobs``: one ``(seq, regions)`` per contig.  Returns ``(bg_counts, stats)``."""
        self.seq_begin_strands(k, both)
        try:
            for seq, regions in jobs:
                if regions is not False:
                    self.seq_scan(seq, regions)
        except BaseException:
            self.seq_end(False, False)
            raise
        _, bg = self.seq_end(False, True)
        return bg, self.seq_stats()


def indel_sites(pos, del_len, insertions, key=None):
    """The arrays kp_seq_indels takes: ``pos`` and ``del_len`` (0 = an insertion) per site,
    ``insertions`` one bytes / str per site (empty for a deletion) or an ``(ins uint8 pool, ins_off
    uint64 [m + 1])`` pair, ``key`` per site (None: the site's index)."""
    pos = np.ascontiguousarray(pos, dtype=np.uint64).reshape(-1)
    del_len = np.ascontiguousarray(del_len, dtype=np.uint64).reshape(-1)
    if isinstance(insertions, tuple):
        ins, ins_off = insertions
    else:
        parts = [x.encode("latin-1") if isinstance(x, str) else bytes(x) for x in insertions]
        ins = np.frombuffer(b"".join(parts), np.uint8)
        ins_off = np.concatenate([[0], np.cumsum([len(x) for x in parts])])
    ins = np.ascontiguousarray(ins, dtype=np.uint8).reshape(-1)
    ins_off = np.ascontiguousarray(ins_off, dtype=np.uint64).reshape(-1)
    if del_len.shape[0] != pos.shape[0] or ins_off.shape[0] != pos.shape[0] + 1:
        raise ValueError("one deletion length and one insertion per site")
    if int(ins_off[-1]) != ins.shape[0]:
        raise ValueError("the last insertion offset is the size of the pool")
    if key is not None:
        key = np.ascontiguousarray(key, dtype=np.uint64).reshape(-1)
        if key.shape[0] != pos.shape[0]:
            raise ValueError("one key per site")
    return pos, del_len, ins, ins_off, key


class HostSeq(_SeqCalls):
    """The kp_seq_* calls of the calling thread's host session (ctx = NULL): the kernels' per-base
    code run serially on the host (parity and CPU tests, not a product path)."""


def seq_host(k, fold, jobs):
    """:meth:`Device.seq_count` computed serially on the host."""
    return HostSeq().seq_count(k, fold, jobs)


def seq_host_contig(k, fold, seq, regions=None, sites=None):
    """One host session of one contig in one call (kp_seq_host); arguments as
    :meth:`Device.seq_count`'s jobs.  Returns ``(pos_counts, bg_counts, stats)``."""
    seq, n = _seq_bytes(seq)
    rb = re = None
    nr = 0
    scan = regions is not False
    if scan and regions is not None:
        reg = np.asarray(regions, dtype=np.uint64).reshape(-1, 2)
        rb, re, nr = np.ascontiguousarray(reg[:, 0]), np.ascontiguousarray(reg[:, 1]), reg.shape[0]
        scan = nr > 0
    p = np.ascontiguousarray(sites if sites is not None else [], dtype=np.uint64).reshape(-1)
    cells = 4 ** int(k) if 1 <= int(k) <= 15 else 1
    pos, bg = np.zeros(cells, np.uint64), np.zeros(cells, np.uint64)
    st = KPSeqStats()
    _check(load().kp_seq_host(int(k), int(bool(fold)), _ptr(seq), n, int(scan), _ptr(rb), _ptr(re), ctypes.c_uint64(nr),
                              _ptr(p), ctypes.c_uint64(p.shape[0]), _ptr(pos), _ptr(bg), ctypes.byref(st)))
    return pos, bg, {name: getattr(st, name) for name, _ in KPSeqStats._fields_}


def seq_indel_host_contig(k, both, seq, contig, regions=None, sites=None, place="left", seed=0):
    """One host indel session of one contig in one call (kp_seq_indel_host); arguments as
    :meth:`Device.seq_count_indels`'s jobs.  Returns ``(pos_counts [3, 4^k], bg_counts, stats,
    resolved)``."""
    seq, n = _seq_bytes(seq)
    rb = re = None
    nr = 0
    scan = regions is not False
    if scan and regions is not None:
        rb, re, nr = _regions_arrays(regions)
        scan = nr > 0
    pos, del_len, ins, ins_off, key = sites if sites is not None else indel_sites([], [], [])
    cells = 4 ** int(k) if 1 <= int(k) <= 15 else 1
    cols, bg = np.zeros((3, cells), np.uint64), np.zeros(cells, np.uint64)
    res = np.zeros((pos.shape[0], 3), np.uint64)
    st = KPSeqStats()
    _check(load().kp_seq_indel_host(int(k), int(bool(both)), _ptr(seq), n, int(contig), int(scan), _ptr(rb), _ptr(re),
                                    ctypes.c_uint64(nr), _ptr(pos), _ptr(del_len), _ptr(key), _ptr(ins_off), _ptr(ins),
                                    ctypes.c_uint64(pos.shape[0]), INDEL_PLACE[place], ctypes.c_uint64(int(seed)),
                                    _ptr(cols), _ptr(bg), _ptr(res), ctypes.byref(st)))
    return cols, bg, {name: getattr(st, name) for name, _ in KPSeqStats._fields_}, res


def _regions_arrays(regions):
    reg = np.asarray(regions, dtype=np.uint64).reshape(-1, 2)
    return np.ascontiguousarray(reg[:, 0]), np.ascontiguousarray(reg[:, 1]), reg.shape[0]


class _PredCalls:
    """The kp_pred_* session calls on ``self._h``: a :class:`Device`'s context, or None for the
    calling thread's host session (:class:`HostPred`)."""

    _h = None
    _pred_P = 0

    def pred_begin(self, k, patterns, super_word, fold=True):
        """Open a prediction session (kp_pred_begin): ``patterns`` are pattern words
        (:func:`pattern_word`) that must be pairwise disjoint, ``super_word`` the super
        pattern's; ``fold`` as :meth:`seq_begin`'s."""
        pats = np.ascontiguousarray(patterns, dtype=np.uint64).reshape(-1)
        _check(load().kp_pred_begin(self._h, int(k), int(bool(fold)), _ptr(pats), ctypes.c_uint32(pats.shape[0]),
                                    ctypes.c_uint64(int(super_word))))
        self._pred_P = pats.shape[0]

    def pred_regions(self, seq, regions, rates=None, want_hist=True):
        """Per region of the contig ``seq`` (``regions`` ``[m, 2]`` 0-based half-open, in any
        order, overlapping or not): ``(hist, other, expected)`` -- ``hist`` uint64 ``[m, P]``
        positions per pattern (None without ``want_hist``), ``other`` uint64 ``[m, 2]`` positions
        without a pattern and positions without a valid window, ``expected`` float64 ``[m]`` the
        sum of ``hist * rates`` in pattern order (None without ``rates``) (kp_pred_regions)."""
        seq, n = _seq_bytes(seq)
        rb, re, m = _regions_arrays(regions)
        P = self._pred_P
        r = exp = None
        if rates is not None:
            r = np.ascontiguousarray(rates, dtype=np.float64).reshape(-1)
            if r.shape[0] != P:
                raise ValueError("one rate per pattern")
            exp = np.zeros(m, np.float64)
        hist = np.zeros((m, P), np.uint64) if want_hist else None
        other = np.zeros((m, 2), np.uint64)
        _check(load().kp_pred_regions(self._h, _ptr(seq), n, _ptr(rb), _ptr(re), ctypes.c_uint64(m), _ptr(r), _ptr(hist),
                                      _ptr(other), _ptr(exp)))
        return hist, other, exp

    def pred_track(self, seq, begin=0, end=None):
        """int32 ``[end - begin]``: the pattern of the window centred at each position of
        ``[begin, end)`` (default: the whole contig), -1 if none matches, -2 without a valid
        window (kp_pred_track)."""
        seq, n = _seq_bytes(seq)
        end = seq.shape[0] if end is None else int(end)
        pid = np.zeros(max(end - int(begin), 0), np.int32)
        _check(load().kp_pred_track(self._h, _ptr(seq), n, ctypes.c_uint64(int(begin)), ctypes.c_uint64(end), _ptr(pid)))
        return pid

    def pred_sites(self, seq, pos):
        """int32 ``[len(pos)]``: :meth:`pred_track`'s code at each 0-based position (kp_pred_sites)."""
        seq, n = _seq_bytes(seq)
        pos = np.ascontiguousarray(pos, dtype=np.uint64).reshape(-1)
        pid = np.zeros(pos.shape[0], np.int32)
        _check(load().kp_pred_sites(self._h, _ptr(seq), n, _ptr(pos), ctypes.c_uint64(pos.shape[0]), _ptr(pid)))
        return pid

    def pred_end(self):
        """Close the session (kp_pred_end)."""
        _check(load().kp_pred_end(self._h))

    def pred_stats(self):
        """Figures of the current or last session (kp_pred_last_stats) as a dict."""
        st = KPPredStats()
        _check(load().kp_pred_last_stats(self._h, ctypes.byref(st)))
        return {name: getattr(st, name) for name, _ in KPPredStats._fields_}


class HostPred(_PredCalls):
    """The kp_pred_* calls of the calling thread's host session (ctx = NULL): the kernels' per-base
    and per-code functions run serially on the host (parity and CPU tests, not a product path)."""


def pred_host(k, patterns, super_word, fold, seq, regions=None, rates=None, track=None, sites=None):
    """One host session of one contig in one call (kp_pred_host): the ``regions`` (with
    ``rates``), the ``track`` range ``(begin, end)`` and the ``sites`` positions, each optional.
    Returns ``(hist, other, expected, track_pid, site_pid, stats)``."""
    seq, n = _seq_bytes(seq)
    pats = np.ascontiguousarray(patterns, dtype=np.uint64).reshape(-1)
    P = pats.shape[0]
    rb, re, m = _regions_arrays(regions if regions is not None else np.zeros((0, 2)))
    r = exp = None
    if rates is not None:
        r = np.ascontiguousarray(rates, dtype=np.float64).reshape(-1)
        if r.shape[0] != P:
            raise ValueError("one rate per pattern")
        exp = np.zeros(m, np.float64)
    hist, other = np.zeros((m, P), np.uint64), np.zeros((m, 2), np.uint64)
    tb, te = (0, 0) if track is None else (int(track[0]), int(track[1]))
    tpid = None if track is None else np.zeros(max(te - tb, 0) + 1, np.int32)  # (never a null pointer)
    p = np.ascontiguousarray(sites if sites is not None else [], dtype=np.uint64).reshape(-1)
    spid = np.zeros(p.shape[0], np.int32)
    st = KPPredStats()
    u64 = ctypes.c_uint64
    _check(load().kp_pred_host(int(k), int(bool(fold)), _ptr(pats), ctypes.c_uint32(P), u64(int(super_word)), _ptr(seq), n,
                               _ptr(rb), _ptr(re), u64(m), _ptr(r), _ptr(hist), _ptr(other), _ptr(exp), u64(tb), u64(te),
                               _ptr(tpid), _ptr(p), u64(p.shape[0]), _ptr(spid), ctypes.byref(st)))
    return (hist, other, exp, None if tpid is None else tpid[:max(te - tb, 0)], spid,
            {name: getattr(st, name) for name, _ in KPPredStats._fields_})


def _transcript_arrays(transcripts):
    """``(seg_begin, seg_end, tx_first, tx_strand)`` of ``(strand, segments)`` pairs."""
    sb, se, first, strand = [], [], [0], []
    for st, segs in transcripts:
        st = {"+": 0, "-": 1}.get(st, st)
        if st not in (0, 1):
            raise ValueError("a strand is 0 / '+' or 1 / '-'")
        strand.append(st)
        for b, e in segs:
            sb.append(int(b))
            se.append(int(e))
        first.append(len(sb))
    if any(x < 0 for x in sb) or any(x < 0 for x in se):
        raise ValueError("a negative segment coordinate")
    return (np.array(sb, np.uint64), np.array(se, np.uint64), np.array(first, np.uint64),
            np.array(strand, np.uint8))


class _SpecCalls:
    """The kp_spec_* session calls on ``self._h``: a :class:`Device`'s context, or None for the
    calling thread's host session (:class:`HostSpec`)."""

    _h = None
    _spec_P = 0

    def spec_begin(self, k, patterns, ptype, fold=True):
        """Open a spectrum session (kp_spec_begin): ``patterns`` are the pattern words of every
        mutation type in one list, ``ptype`` their type ids (0..11, 0..5 with ``fold``); the
        patterns of one type must be pairwise disjoint."""
        pats = np.ascontiguousarray(patterns, dtype=np.uint64).reshape(-1)
        ty = np.asarray(ptype, dtype=np.int64).reshape(-1)
        if ty.shape[0] != pats.shape[0]:
            raise ValueError("one type per pattern")
        if np.any(ty < 0) or np.any(ty >= 1 << 32):
            raise ValueError("a type id that is no uint32")
        ty = np.ascontiguousarray(ty, dtype=np.uint32)
        _check(load().kp_spec_begin(self._h, int(k), int(bool(fold)), _ptr(pats), _ptr(ty), ctypes.c_uint32(pats.shape[0])))
        self._spec_P = pats.shape[0]

    def spec_regions(self, seq, regions, rates=None, want_hist=True):
        """Per region of the contig ``seq``: ``(hist, other, expected)`` -- ``hist`` uint64 ``[m,
        P]`` (None without ``want_hist``), ``other`` uint64 ``[m, 4]`` positions without a
        pattern in slot 0, 1, 2 and positions without a valid window, ``expected`` float64 ``[m,
        12]`` per type id (None without ``rates``) (kp_spec_regions)."""
        seq, n = _seq_bytes(seq)
        rb, re, m = _regions_arrays(regions)
        P = self._spec_P
        r = exp = None
        if rates is not None:
            r = np.ascontiguousarray(rates, dtype=np.float64).reshape(-1)
            if r.shape[0] != P:
                raise ValueError("one rate per pattern")
            exp = np.zeros((m, 12), np.float64)
        hist = np.zeros((m, P), np.uint64) if want_hist else None
        other = np.zeros((m, 4), np.uint64)
        _check(load().kp_spec_regions(self._h, _ptr(seq), n, _ptr(rb), _ptr(re), ctypes.c_uint64(m), _ptr(r), _ptr(hist),
                                      _ptr(other), _ptr(exp)))
        return hist, other, exp

    def spec_track(self, seq, begin=0, end=None):
        """int32 ``[3, end - begin]``: per ALT slot the pattern of the window centred at each
        position, -1 if none, -2 without a valid window (kp_spec_track)."""
        seq, n = _seq_bytes(seq)
        end = seq.shape[0] if end is None else int(end)
        pid = np.zeros((3, max(end - int(begin), 0)), np.int32)
        _check(load().kp_spec_track(self._h, _ptr(seq), n, ctypes.c_uint64(int(begin)), ctypes.c_uint64(end), _ptr(pid)))
        return pid

    def spec_sites(self, seq, pos, alt):
        """int32 ``[len(pos)]``: the pattern in the slot of each site's (folded) ALT, -1 if none,
        -2 without a valid window, -3 where ALT equals the centre base (kp_spec_sites)."""
        seq, n = _seq_bytes(seq)
        pos = np.ascontiguousarray(pos, dtype=np.uint64).reshape(-1)
        alt = _alt_bytes(alt, pos.shape[0])
        pid = np.zeros(pos.shape[0], np.int32)
        _check(load().kp_spec_sites(self._h, _ptr(seq), n, _ptr(pos), _ptr(alt), ctypes.c_uint64(pos.shape[0]), _ptr(pid)))
        return pid

    def spec_simulate(self, seq, regions, rates, seed, contig_id=0, replicate=0, scale=1.0, cap=None):
        """A random mutation set of the contig ``seq`` drawn from the session's model with the
        pattern ``rates`` times ``scale`` (kp_spec_simulate): ``(pos uint64, alt uint8, pid
        int32)`` in ascending position order, ``alt`` the forward-strand ALT as upper-case ASCII,
        ``pid`` the pattern whose rate produced the hit.  ``regions`` must be ascending and
        disjoint.  The draw depends on ``(seed, contig_id, position, replicate)`` and the model
        only.  ``cap``: room for the first try (default: the largest expectation the rates allow
        plus six standard deviations); a set that does not fit is drawn again with its own size."""
        seq, n = _seq_bytes(seq)
        rb, re, m = _regions_arrays(regions)
        r = np.ascontiguousarray(rates, dtype=np.float64).reshape(-1)
        if r.shape[0] != self._spec_P:
            raise ValueError("one rate per pattern")
        for name, v in (("seed", seed), ("contig_id", contig_id), ("replicate", replicate)):
            if not 0 <= int(v) < (1 << 64 if name == "seed" else 1 << 32):
                raise ValueError(f"{name} must be an unsigned {64 if name == 'seed' else 32}-bit integer")
        if cap is None:
            span = float((re - rb).sum()) if m and np.all(re >= rb) else 0.0
            top = float(r.max()) * float(scale) if r.shape[0] else 0.0
            mean = span * min(max(3.0 * top, 0.0), 1.0) if np.isfinite(top) else 0.0
            cap = int(min(span, mean + 6.0 * mean ** 0.5 + 64.0))
        cap = int(cap)
        n_hits = ctypes.c_uint64(0)
        for _ in range(2):
            pos, alt, pid = np.zeros(cap, np.uint64), np.zeros(cap, np.uint8), np.zeros(cap, np.int32)
            _check(load().kp_spec_simulate(self._h, _ptr(seq), n, ctypes.c_uint32(int(contig_id)), _ptr(rb), _ptr(re),
                                           ctypes.c_uint64(m), _ptr(r), ctypes.c_double(float(scale)),
                                           ctypes.c_uint64(int(seed)), ctypes.c_uint32(int(replicate)), ctypes.c_uint64(cap),
                                           _ptr(pos), _ptr(alt), _ptr(pid), ctypes.byref(n_hits)))
            if n_hits.value <= cap:
                break
            cap = n_hits.value
        h = n_hits.value
        return pos[:h].copy(), alt[:h].copy(), pid[:h].copy()

    def spec_sim_stats(self):
        """Figures of the session's last :meth:`spec_simulate` call (kp_spec_last_sim) as a dict."""
        st = KPSpecSimStats()
        _check(load().kp_spec_last_sim(self._h, ctypes.byref(st)))
        return {name: getattr(st, name) for name, _ in KPSpecSimStats._fields_}

    def spec_null(self, seq, regions, rates, seed, contig_id=0, rep_first=0, n_reps=1, scale=1.0, by_type=False):
        """The mutation count of every region in each of ``n_reps`` replicates of
        :meth:`spec_simulate`'s draw (kp_spec_null): uint32 ``[m, n_reps]``, or with ``by_type``
        ``[m, n_reps, 12]`` by type id.  Column ``j`` counts the hits of replicate ``rep_first +
        j``; ``regions`` as :meth:`spec_regions`' (any order, overlapping or not)."""
        seq, n = _seq_bytes(seq)
        rb, re, m = _regions_arrays(regions)
        r = np.ascontiguousarray(rates, dtype=np.float64).reshape(-1)
        if r.shape[0] != self._spec_P:
            raise ValueError("one rate per pattern")
        for name, v in (("seed", seed), ("contig_id", contig_id), ("rep_first", rep_first), ("n_reps", n_reps)):
            if not 0 <= int(v) < (1 << 64 if name == "seed" else 1 << 32):
                raise ValueError(f"{name} must be an unsigned {64 if name == 'seed' else 32}-bit integer")
        shape = (m, int(n_reps), 12) if by_type else (m, int(n_reps))
        size = int(np.prod(shape, dtype=np.int64))
        counts = np.zeros(max(size, 1), np.uint32)  # (never a null pointer)
        _check(load().kp_spec_null(self._h, _ptr(seq), n, ctypes.c_uint32(int(contig_id)), _ptr(rb), _ptr(re),
                                   ctypes.c_uint64(m), _ptr(r), ctypes.c_double(float(scale)), ctypes.c_uint64(int(seed)),
                                   ctypes.c_uint32(int(rep_first)), ctypes.c_uint32(int(n_reps)), int(bool(by_type)),
                                   _ptr(counts)))
        return counts[:size].reshape(shape)

    def spec_null_stats(self):
        """Figures of the session's last :meth:`spec_null` call (kp_spec_last_null) as a dict."""
        st = KPSpecNullStats()
        _check(load().kp_spec_last_null(self._h, ctypes.byref(st)))
        return {name: getattr(st, name) for name, _ in KPSpecNullStats._fields_}

    def spec_coding(self, seq, transcripts, splice=2, rates=None, want_hist=True):
        """Per transcript of the contig ``seq`` the (position, ALT) pairs by coding consequence
        (kp_spec_coding): ``(hist, other, expected)`` -- ``hist`` uint64 ``[m, 5, P]`` per class
        (synonymous, missense, nonsense, stop-lost, essential splice) and pattern (None without
        ``want_hist``), ``other`` uint64 ``[m, 8]`` = all pairs per class, pairs with an invalid
        window, pairs without a pattern, positions without a class, ``expected`` float64 ``[m, 5,
        12]`` per class and type id (None without ``rates``).  ``transcripts``: ``(strand, segments)``
        each, ``strand`` 0 or 1 (or ``+`` / ``-``), ``segments`` ascending 0-based half-open
        ``(begin, end)`` pairs whose lengths sum to a multiple of 3."""
        seq, n = _seq_bytes(seq)
        sb, se, first, strand = _transcript_arrays(transcripts)
        m, P = strand.shape[0], self._spec_P
        r = exp = None
        if rates is not None:
            r = np.ascontiguousarray(rates, dtype=np.float64).reshape(-1)
            if r.shape[0] != P:
                raise ValueError("one rate per pattern")
            exp = np.zeros((m, 5, 12), np.float64)
        hist = np.zeros((m, 5, P), np.uint64) if want_hist else None
        other = np.zeros((m, 8), np.uint64)
        _check(load().kp_spec_coding(self._h, _ptr(seq), n, _ptr(sb), _ptr(se), ctypes.c_uint64(sb.shape[0]), _ptr(first),
                                     _ptr(strand), ctypes.c_uint64(m), ctypes.c_uint32(int(splice)), _ptr(r), _ptr(hist),
                                     _ptr(other), _ptr(exp)))
        return hist, other, exp

    def spec_coding_sites(self, seq, transcripts, pos, alt, tx, splice=2):
        """One result per (site, transcript) pair (kp_spec_coding_sites): ``(cls, pid, codons)`` --
        ``cls`` int32 the class 0..4, -1 where the position is neither coding nor an essential
        splice position of transcript ``tx[i]``, -2 without a class, -3 where ALT equals REF;
        ``pid`` as :meth:`spec_sites`; ``codons`` uint32 = the transcript-strand REF codon | ALT
        codon << 6 (6 bits each, ``16 b0 + 4 b1 + b2``) for classes 0..3."""
        seq, n = _seq_bytes(seq)
        sb, se, first, strand = _transcript_arrays(transcripts)
        pos = np.ascontiguousarray(pos, dtype=np.uint64).reshape(-1)
        alt = _alt_bytes(alt, pos.shape[0])
        tx = np.asarray(tx, dtype=np.int64).reshape(-1)
        if tx.shape[0] != pos.shape[0]:
            raise ValueError("one transcript per site")
        if np.any(tx < 0) or np.any(tx >= 1 << 32):
            raise ValueError("a transcript index that is no uint32")
        tx = np.ascontiguousarray(tx, dtype=np.uint32)
        m = pos.shape[0]
        cls, pid, codons = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.uint32)
        _check(load().kp_spec_coding_sites(self._h, _ptr(seq), n, _ptr(sb), _ptr(se), ctypes.c_uint64(sb.shape[0]),
                                           _ptr(first), _ptr(strand), ctypes.c_uint64(strand.shape[0]),
                                           ctypes.c_uint32(int(splice)), _ptr(pos), _ptr(alt), _ptr(tx), ctypes.c_uint64(m),
                                           _ptr(cls), _ptr(pid), _ptr(codons)))
        return cls, pid, codons

    def spec_coding_stats(self):
        """Figures of the session's last :meth:`spec_coding` call (kp_spec_last_coding) as a dict."""
        st = KPSpecCodingStats()
        _check(load().kp_spec_last_coding(self._h, ctypes.byref(st)))
        return {name: getattr(st, name) for name, _ in KPSpecCodingStats._fields_}

    def spec_coding_null(self, seq, transcripts, rates, seed, contig_id=0, rep_first=0, n_reps=1, scale=1.0, splice=2):
        """The mutation count of every transcript by coding consequence in each of ``n_reps``
        replicates of :meth:`spec_simulate`'s draw (kp_spec_coding_null): uint32 ``[m, n_reps, 5]``
        (synonymous, missense, nonsense, stop-lost, essential splice).  Column ``j`` counts the
        hits of replicate ``rep_first + j`` as :meth:`spec_coding_sites` classes them;
        ``transcripts`` as :meth:`spec_coding`'s."""
        seq, n = _seq_bytes(seq)
        sb, se, first, strand = _transcript_arrays(transcripts)
        m = strand.shape[0]
        r = np.ascontiguousarray(rates, dtype=np.float64).reshape(-1)
        if r.shape[0] != self._spec_P:
            raise ValueError("one rate per pattern")
        for name, v in (("seed", seed), ("contig_id", contig_id), ("rep_first", rep_first), ("n_reps", n_reps)):
            if not 0 <= int(v) < (1 << 64 if name == "seed" else 1 << 32):
                raise ValueError(f"{name} must be an unsigned {64 if name == 'seed' else 32}-bit integer")
        shape = (m, int(n_reps), 5)
        size = int(np.prod(shape, dtype=np.int64))
        counts = np.zeros(max(size, 1), np.uint32)  # (never a null pointer)
        _check(load().kp_spec_coding_null(self._h, _ptr(seq), n, ctypes.c_uint32(int(contig_id)), _ptr(sb), _ptr(se),
                                          ctypes.c_uint64(sb.shape[0]), _ptr(first), _ptr(strand), ctypes.c_uint64(m),
                                          ctypes.c_uint32(int(splice)), _ptr(r), ctypes.c_double(float(scale)),
                                          ctypes.c_uint64(int(seed)), ctypes.c_uint32(int(rep_first)),
                                          ctypes.c_uint32(int(n_reps)), _ptr(counts)))
        return counts[:size].reshape(shape)

    def spec_coding_null_stats(self):
        """Figures of the session's last :meth:`spec_coding_null` call (kp_spec_last_coding_null) as a dict."""
        st = KPSpecCodingNullStats()
        _check(load().kp_spec_last_coding_null(self._h, ctypes.byref(st)))
        return {name: getattr(st, name) for name, _ in KPSpecCodingNullStats._fields_}

    def spec_end(self):
        """Close the session (kp_spec_end)."""
        _check(load().kp_spec_end(self._h))

    def spec_stats(self):
        """Figures of the current or last session (kp_spec_last_stats) as a dict."""
        st = KPSpecStats()
        _check(load().kp_spec_last_stats(self._h, ctypes.byref(st)))
        return {name: getattr(st, name) for name, _ in KPSpecStats._fields_}


class HostSpec(_SpecCalls, _SeqCalls):
    """The kp_spec_* (and typed kp_seq_*) calls of the calling thread's host session (ctx = NULL):
    the kernels' per-base and per-code functions run serially on the host (parity and CPU tests,
    not a product path)."""


def spec_host(k, patterns, ptype, fold, seq, regions=None, rates=None, track=None, sites=None):
    """One host session of one contig in one call (kp_spec_host): the ``regions`` (with
    ``rates``), the ``track`` range ``(begin, end)`` and the ``sites`` ``(pos, alt)``, each
    optional.  Returns ``(hist, other, expected, track_pid, site_pid, stats)``."""
    seq, n = _seq_bytes(seq)
    pats = np.ascontiguousarray(patterns, dtype=np.uint64).reshape(-1)
    ty = np.ascontiguousarray(ptype, dtype=np.uint32).reshape(-1)
    P = pats.shape[0]
    rb, re, m = _regions_arrays(regions if regions is not None else np.zeros((0, 2)))
    r = exp = None
    if rates is not None:
        r = np.ascontiguousarray(rates, dtype=np.float64).reshape(-1)
        if r.shape[0] != P:
            raise ValueError("one rate per pattern")
        exp = np.zeros((m, 12), np.float64)
    hist, other = np.zeros((m, P), np.uint64), np.zeros((m, 4), np.uint64)
    tb, te = (0, 0) if track is None else (int(track[0]), int(track[1]))
    tlen = max(te - tb, 0)
    tpid = None if track is None else np.zeros(3 * tlen + 1, np.int32)  # (never a null pointer)
    p = np.ascontiguousarray(sites[0] if sites is not None else [], dtype=np.uint64).reshape(-1)
    a = _alt_bytes(sites[1] if sites is not None else b"", p.shape[0])
    spid = np.zeros(p.shape[0], np.int32)
    st = KPSpecStats()
    u64 = ctypes.c_uint64
    _check(load().kp_spec_host(int(k), int(bool(fold)), _ptr(pats), _ptr(ty), ctypes.c_uint32(P), _ptr(seq), n, _ptr(rb),
                               _ptr(re), u64(m), _ptr(r), _ptr(hist), _ptr(other), _ptr(exp), u64(tb), u64(te), _ptr(tpid),
                               _ptr(p), _ptr(a), u64(p.shape[0]), _ptr(spid), ctypes.byref(st)))
    return (hist, other, exp, None if tpid is None else tpid[:3 * tlen].reshape(3, tlen), spid,
            {name: getattr(st, name) for name, _ in KPSpecStats._fields_})


def _stats_dict(st):
    return {name: getattr(st, name) for name, _ in type(st)._fields_}


class _ISpecCalls:
    """The kp_ispec_* session calls on ``self._h``: a :class:`Device`'s context, or None for the
    calling thread's host session (:class:`HostISpec`)."""

    _h = None
    _ispec_P = 0

    def ispec_begin(self, k, patterns, pkind):
        """Open an indel-model session of even ``k`` (kp_ispec_begin): ``patterns`` are the pattern
        words of both kinds in one list, ``pkind`` their kinds (0 ins, 1 del); the patterns of one
        kind must be pairwise disjoint."""
        pats = np.ascontiguousarray(patterns, dtype=np.uint64).reshape(-1)
        kind = np.asarray(pkind, dtype=np.int64).reshape(-1)
        if kind.shape[0] != pats.shape[0]:
            raise ValueError("one kind per pattern")
        if np.any(kind < 0) or np.any(kind >= 1 << 32):
            raise ValueError("a kind that is no uint32")
        kind = np.ascontiguousarray(kind, dtype=np.uint32)
        _check(load().kp_ispec_begin(self._h, int(k), _ptr(pats), _ptr(kind), ctypes.c_uint32(pats.shape[0])))
        self._ispec_P = pats.shape[0]

    def ispec_regions(self, seq, regions, rates=None, want_hist=True, budget=None):
        """Per region of the contig ``seq`` (breakpoints ``begin <= b < end``): ``(hist, other,
        expected)`` -- ``hist`` uint64 ``[m, 2, P]`` by strand (None without ``want_hist``), ``other``
        uint64 ``[m, 5]`` = breakpoints without an ins pattern forward / rc, without a del pattern
        forward / rc, and without a valid window, ``expected`` float64 ``[m, 4]`` = ins forward, ins
        rc, del start, del end (None without ``rates``) (kp_ispec_regions).  With ``budget`` the
        regions go in batches of at most that many counters a call, which changes no result."""
        seq, n = _seq_bytes(seq)
        rb, re, m = _regions_arrays(regions)
        P = self._ispec_P
        r = exp = None
        if rates is not None:
            r = np.ascontiguousarray(rates, dtype=np.float64).reshape(-1)
            if r.shape[0] != P:
                raise ValueError("one rate per pattern")
            exp = np.zeros((m, 4), np.float64)
        hist = np.zeros((m, 2, P), np.uint64) if want_hist else None
        other = np.zeros((m, 5), np.uint64)
        step = m if budget is None else max(1, int(budget) // max(2 * P, 1))
        for b in range(0, m, max(step, 1)):
            e = min(m, b + step)
            _check(load().kp_ispec_regions(self._h, _ptr(seq), n, _ptr(rb[b:e]), _ptr(re[b:e]), ctypes.c_uint64(e - b),
                                           _ptr(r), _ptr(hist[b:e]) if want_hist else None, _ptr(other[b:e]),
                                           _ptr(exp[b:e]) if exp is not None else None))
        return hist, other, exp

    def ispec_track(self, seq, begin=0, end=None):
        """int32 ``[4, end - begin]``: per breakpoint the ins pattern of its window and of the
        window's reverse complement, then the del patterns; -1 if none, -2 without a valid window
        (kp_ispec_track)."""
        seq, n = _seq_bytes(seq)
        end = seq.shape[0] if end is None else int(end)
        pid = np.zeros((4, max(end - int(begin), 0)), np.int32)
        _check(load().kp_ispec_track(self._h, _ptr(seq), n, ctypes.c_uint64(int(begin)), ctypes.c_uint64(end), _ptr(pid)))
        return pid

    def ispec_sites(self, seq, contig, sites, place="left", seed=0, want_resolved=True):
        """The two patterns of every indel of ``sites`` (:func:`indel_sites`) on the contig ``seq``
        with index ``contig``, placed as :meth:`seq_indels` places it (kp_ispec_sites).  Returns
        ``(pid int32 [m, 2], resolved uint64 [m, 3] or None)``: an insertion's ins pattern on the
        forward and the other strand, a deletion's del pattern of its start and of its end; -1 none,
        both -2 for a site the counting skips."""
        seq, n = _seq_bytes(seq)
        pos, del_len, ins, ins_off, key = sites
        m = pos.shape[0]
        res = np.zeros((m, 3), np.uint64) if want_resolved else None
        pid = np.zeros((m, 2), np.int32)
        _check(load().kp_ispec_sites(self._h, _ptr(seq), n, int(contig), _ptr(pos), _ptr(del_len), _ptr(key), _ptr(ins_off),
                                     _ptr(ins), ctypes.c_uint64(m), INDEL_PLACE[place], ctypes.c_uint64(int(seed)),
                                     _ptr(res), _ptr(pid)))
        return pid, res

    def ispec_end(self):
        """Close the session (kp_ispec_end)."""
        _check(load().kp_ispec_end(self._h))

    def ispec_stats(self):
        """Figures of the current or last session (kp_ispec_last_stats) as a dict."""
        st = KPISpecStats()
        _check(load().kp_ispec_last_stats(self._h, ctypes.byref(st)))
        return _stats_dict(st)


class HostISpec(_ISpecCalls, _SeqCalls):
    """The kp_ispec_* (and kp_seq_*) calls of the calling thread's host session (ctx = NULL): the
    kernels' per-base and per-code functions run serially on the host (parity and CPU tests, ``--host``)."""


def ispec_host(k, patterns, pkind, seq, contig=0, regions=None, rates=None, track=None, sites=None, place="left", seed=0):
    """One host session of one contig in one call (kp_ispec_host): the ``regions`` (with ``rates``),
    the ``track`` range ``(begin, end)`` and the ``sites`` (:func:`indel_sites`), each optional.
    Returns ``(hist, other, expected, track_pid, site_pid, resolved, stats)``."""
    seq, n = _seq_bytes(seq)
    pats = np.ascontiguousarray(patterns, dtype=np.uint64).reshape(-1)
    kind = np.ascontiguousarray(pkind, dtype=np.uint32).reshape(-1)
    P = pats.shape[0]
    rb, re, m = _regions_arrays(regions if regions is not None else np.zeros((0, 2)))
    r = exp = None
    if rates is not None:
        r = np.ascontiguousarray(rates, dtype=np.float64).reshape(-1)
        if r.shape[0] != P:
            raise ValueError("one rate per pattern")
        exp = np.zeros((m, 4), np.float64)
    hist, other = np.zeros((m, 2, P), np.uint64), np.zeros((m, 5), np.uint64)
    tb, te = (0, 0) if track is None else (int(track[0]), int(track[1]))
    tlen = max(te - tb, 0)
    tpid = None if track is None else np.zeros(4 * tlen + 1, np.int32)  # (never a null pointer)
    pos, del_len, ins, ins_off, key = sites if sites is not None else indel_sites([], [], [])
    ns = pos.shape[0]
    spid, res = np.zeros((ns, 2), np.int32), np.zeros((ns, 3), np.uint64)
    st = KPISpecStats()
    u64 = ctypes.c_uint64
    _check(load().kp_ispec_host(int(k), _ptr(pats), _ptr(kind), ctypes.c_uint32(P), _ptr(seq), n, int(contig), _ptr(rb),
                                _ptr(re), u64(m), _ptr(r), _ptr(hist), _ptr(other), _ptr(exp), u64(tb), u64(te), _ptr(tpid),
                                _ptr(pos), _ptr(del_len), _ptr(key), _ptr(ins_off), _ptr(ins), u64(ns), INDEL_PLACE[place],
                                u64(int(seed)), _ptr(res), _ptr(spid), ctypes.byref(st)))
    return (hist, other, exp, None if tpid is None else tpid[:4 * tlen].reshape(4, tlen), spid, res, _stats_dict(st))


class Device(_SeqCalls, _PredCalls, _SpecCalls, _ISpecCalls):
    """One HIP device context (stream + events) of the library."""

    def __init__(self, device=0):
        L = load()
        self.device = device
        self._h = ctypes.c_void_p()
        _check(L.kp_create(int(device), ctypes.byref(self._h)))

    def mem(self):
        fr, tot = ctypes.c_uint64(), ctypes.c_uint64()
        _check(load().kp_device_mem(self._h, ctypes.byref(fr), ctypes.byref(tot)))
        return fr.value, tot.value

    def log(self, x):
        """float64 log of every element on this GPU (kp_math_log: the DP's device log)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty_like(x)
        _check(load().kp_math_log(self._h, _ptr(x), _ptr(y), ctypes.c_uint64(x.size)))
        return y

    def libm(self, x, fn):
        """The C library's log (fn 1) or log1p (fn 2) as the GPU computes it (kp_math_libm)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty_like(x)
        _check(load().kp_math_libm(self._h, _ptr(x), _ptr(y), ctypes.c_uint64(x.size), int(fn)))
        return y

    def allkmers_cv(self, M, U, alphas, betas):
        """--score all_kmers on this GPU (kp_allkmers_cv; all_kmers_CV.py :8-46): ``M``/``U``
        ``[n, nf]`` fold counts (rows in matches(gen_pat) order), ``betas`` ``[na, nf]``.
        Returns ``(sum_train, sum_test)`` ``[na, nf]`` float64, each summed k-mer by k-mer
        as the reference does."""
        M = np.ascontiguousarray(M, dtype=np.uint64)
        U = np.ascontiguousarray(U, dtype=np.uint64)
        if M.ndim != 2 or U.shape != M.shape:
            raise ValueError("counts must be [n_kmers, nfolds]")
        al = np.ascontiguousarray(alphas, dtype=np.float64).reshape(-1)
        be = np.ascontiguousarray(betas, dtype=np.float64).reshape(al.size, M.shape[1])
        tr = np.zeros(be.shape, np.float64)
        te = np.zeros(be.shape, np.float64)
        _check(load().kp_allkmers_cv(self._h, _ptr(M), _ptr(U), ctypes.c_uint64(M.shape[0]), int(M.shape[1]),
                                     _ptr(al), _ptr(be), int(al.size), _ptr(tr), _ptr(te)))
        return tr, te

    def greedy(self, gen_pat, M, U, lanes, nf=0):
        """The greedy top-down partition of every lane on this GPU (kp_greedy;
        greedy_penalty_plus_pseudo.py :159-196, :324-334).  ``M``/``U``: ``[n_kmers]`` or
        ``[n_kmers, nf]`` counts, rows in matches(gen_pat) order; ``lanes``: tuples ``(fold,
        chain, alpha, beta, penalty)`` (fold -1 = all data, chain -1 = none).  Returns
        ``(loss, chain_test, n_leaves)``."""
        return _greedy_call(self._h, gen_pat, M, U, lanes, nf)

    def greedy_batches(self):
        """Lane batches the last :meth:`greedy` call ran (it cuts the lanes to fit device memory)."""
        return self.greedy_stats()["batches"]

    def greedy_stats(self):
        """Figures of the last :meth:`greedy` call (kp_greedy_last_stats) as a dict."""
        st = KPGreedyStats()
        _check(load().kp_greedy_last_stats(self._h, ctypes.byref(st)))
        return {name: getattr(st, name) for name, _ in KPGreedyStats._fields_}

    def greedy_leaves(self, lane):
        """Patterns of lane ``lane`` of the last :meth:`greedy` call, in the reference's order."""
        return _greedy_leaves(self._h, lane)

    def apply(self, k, patterns, super_word, codes, M, U, rates=None, want_pid=True):
        """A partition applied to a count table on this GPU (kp_apply).  ``patterns``: pattern
        words (:func:`pattern_word`), ``super_word`` the super pattern's; ``codes`` ``[n]``
        KmerCounts codes, ``M``/``U`` ``[n]`` or ``[n, ncol]`` counts; ``rates`` ``[P]`` or None.
        Returns ``(pid, pat_M, pat_U, ll, stats)``: ``pid`` int32 ``[n]`` (-1 no pattern, -2
        several; None without ``want_pid``), ``pat_M``/``pat_U`` uint64 shaped ``[P]`` or ``[P,
        ncol]`` as the counts, ``ll`` float64 ``[ncol]`` (None without rates), ``stats`` a dict."""
        return _apply_call(self._h, k, patterns, super_word, codes, M, U, rates, want_pid)

    def close(self):
        if self._h:
            load().kp_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_MASK_LETTER = "?ACMGRSVTWYHKDBN"  # nucleotide bits A = 1, C = 2, G = 4, T = 8 -> IUPAC code


def pattern_word(pattern):
    """A pattern as kp_greedy's word: 4 bits per position, position 0 lowest."""
    return sum(_MASK_LETTER.index(x) << (4 * i) for i, x in enumerate(pattern))


def word_pattern(word, k):
    """The IUPAC pattern of a kp_greedy pattern word of ``k`` positions."""
    word = int(word)
    return "".join(_MASK_LETTER[(word >> (4 * i)) & 15] for i in range(k))


def _greedy_call(handle, gen_pat, M, U, lanes, nf):
    L = load()
    M = np.ascontiguousarray(M, dtype=np.uint64)
    U = np.ascontiguousarray(U, dtype=np.uint64)
    nf = int(nf)
    cols = max(nf, 1)
    if U.shape != M.shape or M.size % cols or (M.ndim == 2 and M.shape[1] != cols) or M.ndim > 2:
        raise ValueError("counts must be [n_kmers] or [n_kmers, nf]")
    n = M.size // cols
    arr = (KPGreedyLane * max(len(lanes), 1))()
    for i, (fold, chain, alpha, beta, penalty) in enumerate(lanes):
        arr[i] = KPGreedyLane(int(fold), int(chain), float(alpha), float(beta), float(penalty))
    n_chains = max([int(x[1]) + 1 for x in lanes] + [0])
    loss = np.zeros(len(lanes), np.float64)
    chain = np.zeros(n_chains, np.float64)
    nl = np.zeros(len(lanes), np.uint64)
    gp = gen_pat.encode("ascii")
    if handle is None:
        rc = L.kp_greedy_host(gp, _ptr(M), _ptr(U), ctypes.c_uint64(n), nf, arr, len(lanes), _ptr(loss), _ptr(chain),
                              _ptr(nl))
    else:
        rc = L.kp_greedy(handle, gp, _ptr(M), _ptr(U), ctypes.c_uint64(n), nf, arr, len(lanes), _ptr(loss),
                         _ptr(chain), _ptr(nl))
    _check(rc)
    return loss, chain, nl


def _greedy_leaves(handle, lane):
    L = load()
    n = ctypes.c_uint64(0)
    _check(L.kp_greedy_leaves(handle, int(lane), None, ctypes.c_uint64(0), ctypes.byref(n)))
    out = np.zeros(n.value, np.uint64)
    _check(L.kp_greedy_leaves(handle, int(lane), _ptr(out), ctypes.c_uint64(n.value), ctypes.byref(n)))
    return out


def greedy_host(gen_pat, M, U, lanes, nf=0):
    """:meth:`Device.greedy` computed serially on the host (kp_greedy_host: the kernels'
    per-node code; parity and CPU tests, not a product path).  Returns ``(loss, chain_test,
    n_leaves, leaves)`` with ``leaves[lane]`` the lane's pattern words."""
    loss, chain, nl = _greedy_call(None, gen_pat, M, U, lanes, nf)
    return loss, chain, nl, [_greedy_leaves(None, i) for i in range(len(lanes))]


def _apply_call(handle, k, patterns, super_word, codes, M, U, rates, want_pid):
    L = load()
    pats = np.ascontiguousarray(patterns, dtype=np.uint64).reshape(-1)
    codes = np.ascontiguousarray(codes, dtype=np.uint64).reshape(-1)
    M = np.ascontiguousarray(M, dtype=np.int64)
    U = np.ascontiguousarray(U, dtype=np.int64)
    n = codes.shape[0]
    if M.shape != U.shape or M.ndim not in (1, 2) or M.shape[0] != n:
        raise ValueError("counts must be [n_rows] or [n_rows, ncol], as many rows as codes")
    ncol = 1 if M.ndim == 1 else M.shape[1]
    P = pats.shape[0]
    r = ll = None
    if rates is not None:
        r = np.ascontiguousarray(rates, dtype=np.float64).reshape(-1)
        if r.shape[0] != P:
            raise ValueError("one rate per pattern")
        ll = np.zeros(ncol, np.float64)
    pid = np.zeros(n, np.int32) if want_pid else None
    shape = (P,) if M.ndim == 1 else (P, ncol)
    pat_M = np.zeros(shape, np.uint64)
    pat_U = np.zeros(shape, np.uint64)
    st = KPApplyStats()
    args = (int(k), _ptr(pats), ctypes.c_uint32(P), ctypes.c_uint64(int(super_word)), _ptr(codes), _ptr(M), _ptr(U),
            ctypes.c_uint64(n), int(ncol), _ptr(r), _ptr(pid), _ptr(pat_M), _ptr(pat_U), _ptr(ll), ctypes.byref(st))
    _check(L.kp_apply_host(*args) if handle is None else L.kp_apply(handle, *args))
    return pid, pat_M, pat_U, ll, {name: getattr(st, name) for name, _ in KPApplyStats._fields_}


def apply_host(k, patterns, super_word, codes, M, U, rates=None, want_pid=True):
    """:meth:`Device.apply` computed serially on the host (kp_apply_host: the kernels' per-row,
    per-pair and per-term code; parity and CPU tests, not a product path)."""
    return _apply_call(None, k, patterns, super_word, codes, M, U, rates, want_pid)


class Plan:
    """The lattice of one general pattern on one device, with its resident buffers."""

    def __init__(self, device, gen_pat, max_block=0):
        self.device = device
        self.gen_pat = gen_pat
        self._h = ctypes.c_void_p()
        _check(load().kp_plan_create(device._h, gen_pat.encode(), ctypes.c_uint32(max_block), ctypes.byref(self._h)))
        info = KPPlanInfo()
        _check(load().kp_plan_get_info(self._h, ctypes.byref(info)))
        self.info = {name: getattr(info, name) for name, _ in KPPlanInfo._fields_}
        self.nf = None
        self.itype = None
        self.last_lanes = 0
        self.lanes_held = 0  # lanes the device buffers hold (they only grow)

    def set_counts(self, M, U):
        """Fold counts ``[n_kmers, nf]`` (uint32/uint64) in KmerEnumeration order."""
        M = np.ascontiguousarray(M)
        if M.dtype not in (np.uint32, np.uint64):
            raise TypeError("counts must be uint32 or uint64")
        U = np.ascontiguousarray(U, dtype=M.dtype)
        if M.ndim == 1:
            M = M.reshape(-1, 1)
            U = U.reshape(-1, 1)
        _check(load().kp_set_counts(self._h, _ptr(M), _ptr(U), ctypes.c_uint64(M.shape[0]), int(M.shape[1]),
                                    int(M.dtype.itemsize)))
        self.nf = M.shape[1]
        self.itype = M.dtype
        self._refresh_info()

    def _refresh_info(self):
        """Re-read the plan's info: lanes_per_workgroup depends on the count width, fixed
        once counts are set (64-bit counts above 2^32 - 1 take more LDS)."""
        info = KPPlanInfo()
        _check(load().kp_plan_get_info(self._h, ctypes.byref(info)))
        self.info = {name: getattr(info, name) for name, _ in KPPlanInfo._fields_}

    def counts_begin(self, M_all, U_all, nf):
        """Start a fold-by-fold count upload: ``M_all``/``U_all`` ``[n_kmers]`` = counts of
        all data in k-mer order (uint32/uint64), ``nf`` folds to come (kp_counts_begin)."""
        M_all = np.ascontiguousarray(M_all).reshape(-1)
        if M_all.dtype not in (np.uint32, np.uint64):
            raise TypeError("counts must be uint32 or uint64")
        U_all = np.ascontiguousarray(U_all, dtype=M_all.dtype).reshape(-1)
        _check(load().kp_counts_begin(self._h, _ptr(M_all), _ptr(U_all), ctypes.c_uint64(M_all.shape[0]), int(nf),
                                      int(M_all.dtype.itemsize)))
        self.nf = int(nf)
        self.itype = M_all.dtype
        self._refresh_info()

    def counts_fold(self, fold, M_fold, U_fold):
        """Counts of one fold ``[n_kmers]`` (same itype as counts_begin; kp_counts_fold)."""
        M_fold = np.ascontiguousarray(M_fold, dtype=self.itype).reshape(-1)
        U_fold = np.ascontiguousarray(U_fold, dtype=self.itype).reshape(-1)
        _check(load().kp_counts_fold(self._h, int(fold), _ptr(M_fold), _ptr(U_fold), ctypes.c_uint64(M_fold.shape[0])))

    def run(self, groups):
        """One DP sweep.  ``groups``: list of ``(fold, alpha, beta, penalties)``; ``beta`` may
        be a callable returning it (the CV driver's betas of folds still being drawn).

        Returns ``(root_train f32[L], root_test f32[L], n_leaves u64[L])`` with lanes
        numbered group-major.
        """
        arr, nl = _group_array(groups)
        rt = np.zeros(nl, np.float32)
        re = np.zeros(nl, np.float32)
        nlv = np.zeros(nl, np.uint64)
        _check(load().kp_pass(self._h, arr, len(groups), _ptr(rt), _ptr(re), _ptr(nlv)))
        self.last_lanes = nl
        self.lanes_held = max(self.lanes_held, nl)
        return rt, re, nlv

    def reserve(self, lanes):
        """Allocate the per-lane buffers for ``lanes`` lanes now (kp_reserve_lanes)."""
        _check(load().kp_reserve_lanes(self._h, int(lanes)))
        self.lanes_held = max(self.lanes_held, int(lanes))

    def stats(self):
        s = KPPassStats()
        _check(load().kp_last_pass_stats(self._h, ctypes.byref(s)))
        return {name: getattr(s, name) for name, _ in KPPassStats._fields_}

    def block_check(self):
        """Entries of the device block list (built by kp_blocks_kernel) that differ from the
        host's block walk (kp_plan_block_check): 0 when they agree."""
        n = ctypes.c_uint64()
        _check(load().kp_plan_block_check(self._h, ctypes.byref(n)))
        return n.value

    def launch_ms(self):
        """Per-launch device times (ms) of the last pass (needs KP_LAUNCH_TIMES=1)."""
        n = ctypes.c_int()
        _check(load().kp_last_launch_ms(self._h, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, np.float32)
        _check(load().kp_last_launch_ms(self._h, _ptr(out), n.value, ctypes.byref(n)))
        return out

    def leaves(self, lane):
        """Cell indices of the optimal partition of ``lane``, in backtrack order."""
        n = ctypes.c_uint64()
        _check(load().kp_fit_leaves(self._h, int(lane), None, ctypes.c_uint64(0), ctypes.byref(n)))
        out = np.zeros(max(1, n.value), np.uint64)
        _check(load().kp_fit_leaves(self._h, int(lane), _ptr(out), ctypes.c_uint64(out.size), ctypes.byref(n)))
        return out[:n.value]

    def dump_lane(self, lane):
        score = np.zeros(self.info["npat"], np.float32)
        code = np.zeros(self.info["npat"], np.uint8)
        _check(load().kp_dump_lane(self._h, int(lane), _ptr(score), _ptr(code)))
        return score, code

    def gather_cells(self, lane, cells):
        """Train scores (f32) of the cells ``cells`` (uint64 indices) of ``lane`` of the last
        pass (kp_gather_cells)."""
        cells = np.ascontiguousarray(cells, dtype=np.uint64).reshape(-1)
        out = np.zeros(cells.size, np.float32)
        _check(load().kp_gather_cells(self._h, int(lane), _ptr(cells), ctypes.c_uint64(cells.size), _ptr(out)))
        return out

    def lanes_that_fit(self, reserve=2 << 30):
        fr, _ = self.device.mem()
        per = self.info["bytes_per_lane"]
        # the lane buffers already held are reused: count them as available
        held = self.lanes_held * per
        return max(0, int((fr + held - reserve) // per))

    def require_lanes(self, n=1, reserve=2 << 30):
        """Lanes that fit device memory now (``lanes_that_fit``); raises :class:`KPError`
        (KP_E_NOMEM) naming the lattice, its bytes per lane and the GPU's free memory if
        not even ``n`` do -- the reference would allocate its ``[npat, nf]`` arrays anyway
        (CV :93-102) and fail in numpy; a pass of zero lanes is never planned."""
        fit = self.lanes_that_fit(reserve)
        if fit < n:
            fr, tot = self.device.mem()
            per = self.info["bytes_per_lane"]
            raise KPError(-2, f"the lattice of {self.gen_pat} ({self.info['npat']:,} cells) needs "
                              f"{per / 1e9:.4g} GB of device memory per lane (float32 score per cell), "
                              f"{n} lane(s) at least; GPU {self.device.device} has {(fr + self.lanes_held * per) / 1e9:.4g} "
                              f"of {tot / 1e9:.4g} GB free after the plan's tables, of which {reserve / 2**30:.3g} GiB "
                              f"stay free for the library's working buffers. Restrict the general pattern "
                              f"with --super_pattern.")
        return fit

    def close(self):
        if self._h:
            load().kp_plan_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ----------------------------------------------------------------------------
# host helpers
# ----------------------------------------------------------------------------

def kmer_order(gen_pat, contexts):
    """KmerEnumeration index of every k-mer in ``contexts`` (vectorised): a list of k-mer
    strings, or a table with ``letters()`` (io_utils.KmerCounts, native parser output)."""
    k = len(gen_pat)
    if hasattr(contexts, "letters"):
        raw, name = contexts.letters(), contexts.kmer_at
    elif not contexts:
        return np.zeros(0, np.int64)
    else:
        raw = np.frombuffer("".join(contexts).encode("ascii"), dtype=np.uint8).reshape(len(contexts), k)
        name = contexts.__getitem__
    if raw.shape[0] == 0:
        return np.zeros(0, np.int64)
    idx = np.zeros(len(contexts), np.int64)
    w = 1
    for i, g in enumerate(gen_pat):
        lut = np.full(256, -1, np.int64)
        for nuc, d in code_no[g].items():
            lut[ord(nuc)] = d
        dig = lut[raw[:, i]]
        if (dig < 0).any():
            bad = name(int(np.argmax(dig < 0)))
            raise ValueError(f"k-mer {bad} does not match general pattern {gen_pat}")
        idx += dig * w
        w *= len(code_no[g])
    return idx


def counts_in_kmer_order(gen_pat, contexts, M, U, n_kmers, itype):
    """Scatter per-context rows ``[n, nf]`` into dense KmerEnumeration order (missing k-mers = 0)."""
    M = np.asarray(M)
    nf = 1 if M.ndim == 1 else M.shape[1]
    outM = np.zeros((n_kmers, nf), dtype=itype)
    outU = np.zeros((n_kmers, nf), dtype=itype)
    idx = kmer_order(gen_pat, contexts if hasattr(contexts, "letters") else list(contexts))
    outM[idx] = np.asarray(M, dtype=itype).reshape(len(idx), nf)
    outU[idx] = np.asarray(U, dtype=itype).reshape(len(idx), nf)
    return outM, outU


class FoldFeed:
    """Fold counts that arrive one fold at a time, in k-mer order: the CV driver draws the
    fold split on a host thread (CV_tools.fold_stream) while the GPUs already run the
    passes of the folds drawn so far.  ``M_all``/``U_all`` ``[n_kmers]`` = counts of all
    data (the sum of the folds to come), ``nf`` folds."""

    def __init__(self, M_all, U_all, nf):
        self.M_all = np.ascontiguousarray(M_all).reshape(-1)
        self.U_all = np.ascontiguousarray(U_all, dtype=self.M_all.dtype).reshape(-1)
        self.nf = int(nf)
        self._cols = [None] * self.nf
        self.t_put = [None] * self.nf  # perf_counter() at each fold's arrival
        self._err = None
        self._cv = threading.Condition()

    def put(self, fold, M_fold, U_fold):
        with self._cv:
            self._cols[fold] = (np.ascontiguousarray(M_fold, dtype=self.M_all.dtype),
                                np.ascontiguousarray(U_fold, dtype=self.M_all.dtype))
            self.t_put[fold] = time.perf_counter()
            self._cv.notify_all()

    def fail(self, exc):
        """The producer failed: every waiting and later ``get`` raises."""
        with self._cv:
            self._err = exc
            self._cv.notify_all()

    def get(self, fold):
        """``(M_fold, U_fold)``, waiting until the fold has been drawn."""
        with self._cv:
            while self._cols[fold] is None and self._err is None:
                self._cv.wait()
            if self._cols[fold] is None:
                raise RuntimeError(f"fold split failed before fold {fold}") from self._err
            return self._cols[fold]

    def arrays(self):
        """``(M, U)`` ``[n_kmers, nf]`` once every fold has arrived."""
        cols = [self.get(f) for f in range(self.nf)]
        return np.stack([c[0] for c in cols], axis=1), np.stack([c[1] for c in cols], axis=1)


def materialize(M, U, groups):
    """For runners without fold-by-fold upload: wait for a FoldFeed's folds and resolve
    callable betas.  Returns ``(M, U, groups)`` with arrays and float betas."""
    if isinstance(M, FoldFeed):
        M, U = M.arrays()
    groups = [(f, a, float(b() if callable(b) else b), pens) for f, a, b, pens in groups]
    return M, U, groups


# lanes a pass may hold when it packs groups of different widths (KMERPAPA_PASS_LANES; 0 =
# one sweep workgroup's width + 1, Plan.info["lanes_per_workgroup"] + 1)
PASS_LANES = int(os.environ.get("KMERPAPA_PASS_LANES", "0"))


def pass_cap(groups, fit, width=0):
    """Lanes per pass: PASS_LANES, by default one workgroup's ``width`` + 1 (6 at 9-mers),
    or the largest group if wider, if that fits.  A pass of two device groups runs their
    workgroups side by side in the same launches, so packing a small piece beside a full
    one saves the small pass's fixed work: 9-mer 5 + 1 lanes 468 ms against 371 + 108, 4 + 2
    482 against 310 + 182, 3 + 3 473 against 2 x 242 (profiles/r05/experiments/
    pack_lanes.txt) -- the pieces a lane-granular multi-GPU share is left with.  Wider packs
    gain less (5 + 2: 549 against 553) and every lane of the widest pass is allocated for the
    whole job (30.8 GB per lane at 9-mers), so one extra lane is the default.  The
    allocation's cost is the driver's wipe of HBM that earlier processes freed:
    about as long for 154 as for 185 GB when HBM is still being wiped, ~1 ms for either when
    it is clean.  Two 5-lane groups never share a pass: they are not faster per lane."""
    widest = max([len(g[3]) for g in groups] or [1])
    cap = PASS_LANES or ((width + 1) if width else 7)
    return min(fit, max(cap, widest))


def pack_passes(groups, max_lanes):
    """Split a group list into passes of at most ``max_lanes`` lanes (order kept)."""
    if max_lanes < 1:
        raise KPError(-2, "the lattice does not fit device memory even for one lane")
    passes, cur, n = [], [], 0
    for grp in groups:
        lanes = len(grp[3])
        if cur and n + lanes > max_lanes:
            passes.append(cur)
            cur, n = [], 0
        cur.append(grp)
        n += lanes
    if cur:
        passes.append(cur)
    return passes


def fold_pieces(groups, width):
    """The lanes of ``groups`` cut into pieces of at most ``width`` lanes, fold by fold: each
    fold's lanes (its groups in order, group-major) are cut together, so one piece may hold
    the last penalties of one alpha and the first of the next.  The library runs such a
    piece as ONE device group (a mixed group: the fold's count tables are shared, only the
    logs differ per alpha), so a 7-penalty grid runs as 5-lane workgroups instead of 5 + 2
    per alpha.  Returns pieces in order of first appearance of their fold; a piece is a list
    of ``(fold, alpha, beta, penalties, lane_ids)``, lane ids = group-major lane numbers in
    ``groups``."""
    start = np.cumsum([0] + [len(g[3]) for g in groups])
    folds = {}
    for gi, g in enumerate(groups):
        folds.setdefault(g[0], []).extend((gi, j) for j in range(len(g[3])))
    pieces = []
    for lanes in folds.values():
        for q in range(0, len(lanes), width):
            piece = []
            for gi, j in lanes[q:q + width]:
                f, a, b, pens = groups[gi][:4]
                if piece and piece[-1][5] == gi:
                    piece[-1][3].append(pens[j])
                    piece[-1][4].append(int(start[gi] + j))
                else:
                    piece.append([f, a, b, [pens[j]], [int(start[gi] + j)], gi])
            pieces.append([tuple(x[:5]) for x in piece])
    return pieces


def plan_passes(groups, max_lanes, width=None):
    """The passes one GPU runs for ``groups``, in run order: lowest fold first (folds are
    drawn in order, CV_tools.fold_stream, so the first pass starts as soon as the share's
    lowest fold is drawn), at most ``max_lanes`` lanes per pass.  With ``width`` (the lanes
    of one sweep workgroup, ``Plan.info["lanes_per_workgroup"]``) the lanes are first cut
    into fold pieces of that width (fold_pieces); without it every group is one piece.
    Pieces are packed in descending fold order and the passes then reversed, so a small
    piece (e.g. a 1-lane piece of a split group) joins the pass of a piece with the same or
    a HIGHER fold and never delays an earlier one.  Returns ``(passes, lane_order)``: a
    pass is a list of groups ``(fold, alpha, beta, penalties)``; ``lane_order[k]`` = the
    group-major lane number in ``groups`` of the k-th lane of the passes' concatenated
    results (unpermute_lanes)."""
    if max_lanes < 1:
        raise KPError(-2, "the lattice does not fit device memory even for one lane")
    if width:
        pieces = fold_pieces(groups, max(1, min(width, max_lanes)))
    else:
        start = np.cumsum([0] + [len(g[3]) for g in groups])
        pieces = [[(g[0], g[1], g[2], list(g[3]), list(range(start[i], start[i + 1])))] for i, g in enumerate(groups)]
    desc = sorted(range(len(pieces)), key=lambda i: -pieces[i][0][0])  # stable
    passes, cur, n = [], [], 0
    for i in desc:
        lanes = sum(len(x[3]) for x in pieces[i])
        if cur and n + lanes > max_lanes:
            passes.append(cur)
            cur, n = [], 0
        cur.extend(pieces[i])
        n += lanes
    if cur:
        passes.append(cur)
    passes.reverse()
    # the first pass starts when its highest fold is drawn: if it packs the share's lowest
    # fold with a higher one (e.g. a 1-lane fold-0 piece beside a 4-lane fold-2 piece), the
    # lowest fold's pieces run first on their own (fold 2 is drawn ~65 ms after fold 0 at
    # 9-mers, while packing saves ~10 ms of pass time)
    if passes and len({x[0] for x in passes[0]}) > 1:
        lo = min(x[0] for x in passes[0])
        passes[:1] = [[x for x in passes[0] if x[0] == lo], [x for x in passes[0] if x[0] != lo]]
    # within a pass the fold with the most lanes comes first (lanes 0..): a 1-lane piece laid
    # out before a 5-lane one costs the pass 486 vs 468 ms at 9-mers
    # (profiles/r05/experiments/pack_order.txt); the pieces of one fold stay adjacent, so
    # the library can still cut them into mixed device groups
    for i, pas in enumerate(passes):
        per_fold = {}
        for x in pas:
            per_fold[x[0]] = per_fold.get(x[0], 0) + len(x[3])
        passes[i] = sorted(pas, key=lambda x: (-per_fold[x[0]], x[0]))  # stable within a fold
    lane_order = np.array([lid for pas in passes for x in pas for lid in x[4]], dtype=np.int64)
    return [[tuple(x[:4]) for x in pas] for pas in passes], lane_order


def unpermute_lanes(lane_order, arr):
    """Lane results in the passes' order (plan_passes) back to the groups' own group-major
    lane order."""
    out = np.empty_like(arr)
    out[lane_order] = arr
    return out


_devices = {}
_plans = {}
_cache_lock = threading.Lock()


def get_device(dev, replica=0):
    """The library context of GPU ``dev``; ``replica`` > 0 = another context (its own HIP
    stream) on the same GPU, for a device list that names one GPU more than once."""
    with _cache_lock:
        if (dev, replica) not in _devices:
            _devices[(dev, replica)] = Device(dev)
        return _devices[(dev, replica)]


def get_plan(dev, gen_pat, max_block=0, replica=0):
    key = (dev, gen_pat, max_block, replica)
    with _cache_lock:
        plan = _plans.get(key)
    if plan is None:
        plan = Plan(get_device(dev, replica), gen_pat, max_block)
        with _cache_lock:
            # one resident lattice per device: drop other patterns' buffers first (replicas
            # of the same lattice stay)
            for other in [k for k in _plans if k[0] == dev and k[1:3] != key[1:3]]:
                _plans.pop(other).close()
            _plans[key] = plan
    return plan


def release_all():
    """Free every cached plan's device buffers (the devices stay open)."""
    with _cache_lock:
        for p in _plans.values():
            p.close()
        _plans.clear()


def _shutdown():
    """At interpreter exit, while the library and the HIP runtime are still loaded: plans
    first (a plan's pooled score buffer is freed on its device's stream), then devices.
    Left to garbage collection, module teardown may destroy a device before its plan."""
    try:
        release_all()
        with _cache_lock:
            for d in _devices.values():
                d.close()
            _devices.clear()
    except Exception:
        pass


atexit.register(_shutdown)


def _device_shares(groups, devices, width):
    from .shard import rank_groups
    return [rank_groups(groups, slot, len(devices), width) for slot in range(len(devices))]


def _replicas(devices):
    """Replica index of every slot: how often its GPU was named before (0 for a list of
    distinct GPUs).  A GPU named twice gets two contexts and two host threads: that runs
    the multi-GPU path on one GPU (a rehearsal; the slots share its HBM and bandwidth)."""
    seen = {}
    out = []
    for d in devices:
        out.append(seen.get(d, 0))
        seen[d] = out[-1] + 1
    return out


def prepare_groups(gen_pat, groups, devices=None, max_block=0, itype=np.uint32):
    """Everything ``run_groups`` needs before the counts exist: each GPU's plan (lattice
    tables uploaded) and one allocation for its largest pass.  Only the lane counts of
    ``groups`` matter (folds, alphas and betas may be placeholders), so a caller can run
    this while the host draws the fold split (CV_tools.fold_tables drops the GIL).  ``itype``
    = the counts' width to come (the shares depend on it, shard_width)."""
    devices = list(devices if devices is not None else visible_devices()[:1])
    wg = shard_width(gen_pat, itype, max_block)  # the sweep workgroup's lanes at the counts' width

    errors = []

    def prep(dev, rep, chunk):
        try:
            if chunk:
                plan = get_plan(dev, gen_pat, max_block, replica=rep)
                passes, _ = plan_passes(chunk, pass_cap(chunk, plan.require_lanes(), wg), wg)
                plan.reserve(max(sum(len(g[3]) for g in pas) for pas in passes))
        except Exception as e:  # re-raised in the caller's thread
            errors.append(e)
    threads = [threading.Thread(target=prep, args=(dev, rep, chunk))
               for dev, rep, chunk in zip(devices, _replicas(devices),
                                          _device_shares(groups, devices, wg if len(devices) > 1 else 0))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    if errors:
        raise errors[0]


PASS_LOG = None  # a list to receive one timing record per pass of run_groups (bench.py)


def run_groups(gen_pat, M, U, groups, devices=None, max_block=0):
    """Run every lane group over the lattice of ``gen_pat`` on the given GPUs.

    ``M``/``U`` are ``[n_kmers, nf]`` counts in k-mer order, or ``M`` is a
    :class:`FoldFeed` (``U`` unused): then every GPU uploads the all-data counts first and
    each fold as it arrives, and runs its passes in fold order, so the first passes start
    before the last folds are drawn.  The lanes (one penalty of one group, group-major)
    are split over the GPUs in equal shares and regrouped by (fold, alpha)
    (``shard.assign_lanes``: whole groups where each fits a workgroup, else contiguous lane
    runs -- the same split the ranks of a torchrun job use),
    each GPU's share packed into memory-sized passes, one host thread per GPU.  Returns
    ``(root_train, root_test, n_leaves)`` arrays over all lanes, group-major.
    """
    devices = list(devices) if devices is not None else visible_devices()[:1]
    reps = _replicas(devices)  # one host thread and one context per slot: a plan is never shared
    if not devices:
        raise KPError(-3, "no GPU visible")
    nd = len(devices)
    # (whole groups of one workgroup's width per device; results go back by shard.unshard)
    width = shard_width(gen_pat, counts_itype(M), max_block) if nd > 1 else 0
    shares = _device_shares(groups, devices, width)
    results = [None] * nd
    errors = []

    feed = M if isinstance(M, FoldFeed) else None

    def work(slot, dev, chunk):
        try:
            outs = []
            if chunk:
                plan = get_plan(dev, gen_pat, max_block, replica=reps[slot])
                if feed is not None:
                    plan.counts_begin(feed.M_all, feed.U_all, feed.nf)
                else:
                    plan.set_counts(M, U)
                # passes in fold order (folds arrive in order), small groups beside a full one
                width = plan.info["lanes_per_workgroup"]
                passes, order = plan_passes(chunk, pass_cap(chunk, plan.require_lanes(), width), width)
                plan.reserve(max(sum(len(g[3]) for g in pas) for pas in passes))  # one allocation
                outs = []
                queued = {}
                if feed is not None:
                    # a feeder thread queues each fold's count table (kp_counts_fold: the
                    # device's count stream) as soon as the fold is drawn, so it fills while
                    # the previous fold's passes run; a pass waits until its folds are queued
                    need = []
                    for pas in passes:
                        need += sorted({g[0] for g in pas if g[0] >= 0} - set(need))
                    queued = {f: threading.Event() for f in need}
                    fed_err = []

                    def feeder():
                        try:
                            for f in need:
                                plan.counts_fold(f, *feed.get(f))
                                queued[f].set()
                        except BaseException as e:  # raised by the pass loop below
                            fed_err.append(e)
                        finally:
                            for ev in queued.values():
                                ev.set()
                    fth = threading.Thread(target=feeder)
                    fth.start()
                try:
                    for pas in passes:
                        t_wait = time.perf_counter()
                        for f in sorted({g[0] for g in pas if g[0] in queued}):
                            queued[f].wait()
                            if fed_err:
                                raise fed_err[0]
                        t_run = time.perf_counter()
                        outs.append(plan.run(pas))
                        if PASS_LOG is not None:  # (slot, lanes, counts wait s, pass start, pass end, stats)
                            PASS_LOG.append((slot, sum(len(g[3]) for g in pas), t_run - t_wait, t_run,
                                             time.perf_counter(), plan.stats() if hasattr(plan, "stats") else {}))
                finally:
                    if feed is not None:
                        fth.join()
            if outs:
                results[slot] = tuple(unpermute_lanes(order, np.concatenate([o[i] for o in outs]))
                                      for i in range(3))
            else:
                results[slot] = (np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.uint64))
        except Exception as e:  # re-raised in the caller's thread
            errors.append(e)

    threads = []
    for slot, dev in enumerate(devices):
        chunk = shares[slot]
        if nd == 1:
            work(slot, dev, chunk)
        else:
            th = threading.Thread(target=work, args=(slot, dev, chunk))
            th.start()
            threads.append(th)
    for th in threads:
        th.join()
    if errors:
        raise errors[0]
    from .shard import unshard
    return tuple(unshard(groups, nd, [r[i] for r in results], width) for i in range(3))


run_groups.prepare = prepare_groups
run_groups.fold_feed = True  # accepts a FoldFeed for M
