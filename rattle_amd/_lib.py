"""ctypes binding of librattle_hip.so (include/rattle_hip.h).

The library is built in-tree by `__graft_entry__.build()` / `make -C rattle_amd/csrc`.
There is no fallback: if the shared object is missing, or no HIP device is present when a
context is created, the call fails loudly.
"""
from __future__ import annotations

import os as _os
_os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")      # before the HIP runtime starts: one hardware queue per POA column class (csrc/poa.hip)
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RATTLE_HIP_LIB", os.path.join(_HERE, "csrc", "librattle_hip.so"))


class ClusterParams(C.Structure):
    _fields_ = [("t_s", C.c_double), ("t_v", C.c_double), ("bv_threshold", C.c_double),
                ("min_bv_threshold", C.c_double), ("bv_falloff", C.c_double), ("min_reads_cluster", C.c_int),
                ("use_hc", C.c_int), ("repr_percentile", C.c_double), ("is_rna", C.c_int)]


class ClusterSet(C.Structure):
    _fields_ = [("n_clusters", C.c_uint32), ("main_id", C.POINTER(C.c_int32)), ("main_rev", C.POINTER(C.c_uint8)),
                ("offsets", C.POINTER(C.c_uint32)), ("member_id", C.POINTER(C.c_int32)),
                ("member_rev", C.POINTER(C.c_uint8)), ("counters", C.c_uint64 * 8), ("gene_id", C.POINTER(C.c_int32))]


class CorrectParams(C.Structure):
    _fields_ = [("min_occ", C.c_double), ("gap_occ", C.c_double), ("err_ratio", C.c_double), ("split", C.c_int),
                ("min_reads", C.c_int), ("n_threads", C.c_int), ("vote_order", C.c_char * 8),
                ("n_pack_orders", C.c_uint32), ("pack_order_cluster", C.POINTER(C.c_uint32)),
                ("pack_order_offsets", C.POINTER(C.c_uint32)), ("pack_order_perm", C.POINTER(C.c_uint32)),
                ("max_pack_cells", C.c_uint64), ("corrected_ready", C.c_void_p), ("corrected_ready_user", C.c_void_p)]


class ReadSet(C.Structure):
    _fields_ = [("n", C.c_uint32), ("read_id", C.POINTER(C.c_int32)), ("cluster_id", C.POINTER(C.c_int32)),
                ("n_reads", C.POINTER(C.c_int32)), ("off", C.POINTER(C.c_uint64)), ("seq", C.POINTER(C.c_char)),
                ("qual", C.POINTER(C.c_char))]


class SkipList(C.Structure):
    _fields_ = [("n", C.c_uint32), ("cluster_id", C.POINTER(C.c_int32)), ("pack", C.POINTER(C.c_uint32)),
                ("stage", C.POINTER(C.c_uint32)), ("read_off", C.POINTER(C.c_uint64)), ("read_id", C.POINTER(C.c_int32))]


class Correction(C.Structure):
    _fields_ = [("corrected", ReadSet), ("uncorrected", ReadSet), ("consensi", ReadSet), ("counters", C.c_uint64 * 8),
                ("skipped", SkipList), ("corrected_pack", C.POINTER(C.c_uint32)), ("uncorrected_pack", C.POINTER(C.c_uint32))]


class PackPlan(C.Structure):
    _fields_ = [("n_packs", C.c_uint32), ("pack_first", C.POINTER(C.c_uint32)), ("member_id", C.POINTER(C.c_int32)),
                ("member_rev", C.POINTER(C.c_uint8)), ("pack_cluster", C.POINTER(C.c_int32)),
                ("pack_local", C.POINTER(C.c_uint32)), ("pack_cost", C.POINTER(C.c_uint64)),
                ("pack_owner", C.POINTER(C.c_uint32)), ("n_unqueued", C.c_uint32), ("unqueued_id", C.POINTER(C.c_int32)),
                ("unqueued_cluster", C.POINTER(C.c_int32))]


class DebugRect(C.Structure):
    _fields_ = [("seed_ids", C.POINTER(C.c_uint32)), ("n_seeds", C.c_uint32), ("cand_ids", C.POINTER(C.c_uint32)),
                ("n_cands", C.c_uint32), ("triangular", C.c_int), ("thr", C.c_double)]


class DebugPairs(C.Structure):
    _fields_ = [("n", C.c_uint32), ("rect", C.POINTER(C.c_uint32)), ("seed", C.POINTER(C.c_uint32)),
                ("cand", C.POINTER(C.c_uint32)), ("strand", C.POINTER(C.c_uint8)), ("count", C.POINTER(C.c_int32))]


class DebugEval(C.Structure):
    _fields_ = [("survivors", DebugPairs), ("kept", DebugPairs), ("hits", DebugPairs), ("counters", C.POINTER(C.c_uint64)),
                ("count_pass", C.c_int), ("filter_launches", C.c_uint64), ("oversize_pairs", C.c_uint64),
                ("hit_bases", C.POINTER(C.c_int32)), ("hit_hc_bases", C.POINTER(C.c_int32)), ("hit_variance", C.POINTER(C.c_double))]


class DebugMsa(C.Structure):
    _fields_ = [("n_packs", C.c_uint32), ("pack_first", C.POINTER(C.c_uint32)), ("width", C.POINTER(C.c_uint32)),
                ("off", C.POINTER(C.c_uint64)), ("seq", C.POINTER(C.c_uint8)), ("qual", C.POINTER(C.c_uint8)),
                ("col", C.POINTER(C.c_uint32))]


# the correction report (rattle_correction_report): lengths and trim counts, then kernel D's six counters
REPORT_COUNTERS = ("match", "substituted", "mismatch_kept", "inserted", "deleted", "gap_kept")
REPORT_FIELDS = ("in_len", "out_len", "trim_front", "trim_back") + REPORT_COUNTERS


class DebugPost(C.Structure):
    _fields_ = [("n_packs", C.c_uint32), ("n_rows", C.c_uint32), ("mode", C.c_int), ("n_cols", C.c_uint64),
                ("moff", C.POINTER(C.c_uint64)), ("coff", C.POINTER(C.c_uint64)), ("rfirst", C.POINTER(C.c_int32)),
                ("rlast", C.POINTER(C.c_int32)), ("tfront", C.POINTER(C.c_uint32)), ("tback", C.POINTER(C.c_uint32)),
                ("olen", C.POINTER(C.c_uint32)), ("out_off", C.POINTER(C.c_uint64)), ("out_seq", C.POINTER(C.c_uint8)),
                ("out_qual", C.POINTER(C.c_uint8)), ("cons", C.POINTER(C.c_uint8)), ("flag", C.POINTER(C.c_uint8)),
                ("sym", C.POINTER(C.c_uint8)), ("err", C.POINTER(C.c_double)), ("cons_len", C.POINTER(C.c_uint32)),
                ("consensus", C.POINTER(C.c_uint8))] + [(f, C.POINTER(C.c_uint32)) for f in REPORT_COUNTERS]


class CorrectionReport(C.Structure):
    _fields_ = [("n", C.c_uint32)] + [(f, C.POINTER(C.c_uint32)) for f in REPORT_FIELDS]


# the consensus support (rattle_consensus_support): four values per base of the consensi
SUPPORT_FIELDS = ("support", "depth", "pack_support", "pack_depth")


class ConsensusSupport(C.Structure):
    _fields_ = [("n", C.c_uint32), ("level", C.POINTER(C.c_uint8)), ("off", C.POINTER(C.c_uint64))] + \
               [(f, C.POINTER(C.c_uint32)) for f in SUPPORT_FIELDS]


class DebugSupportMsa(C.Structure):
    _fields_ = [("n_packs", C.c_uint32), ("pack_first", C.POINTER(C.c_uint32)), ("width", C.POINTER(C.c_uint32)),
                ("off", C.POINTER(C.c_uint64)), ("seq", C.POINTER(C.c_uint8)), ("col", C.POINTER(C.c_uint32)),
                ("sup", C.POINTER(C.c_uint32)), ("dep", C.POINTER(C.c_uint32))]


class DebugSupport(C.Structure):
    _fields_ = [("n_packs", C.c_uint32), ("level", C.c_int), ("n_cols", C.c_uint64), ("coff", C.POINTER(C.c_uint64)),
                ("cons_len", C.POINTER(C.c_uint32)), ("consensus", C.POINTER(C.c_uint8))] + \
               [(f, C.POINTER(C.c_uint32)) for f in SUPPORT_FIELDS]


# the cluster report (rattle_cluster_report): one entry per join
CLUSTER_REPORT_FIELDS = (("level", C.c_uint8), ("pass", C.c_uint32), ("bv_threshold", C.c_double), ("into", C.c_int32),
                         ("absorbed", C.c_int32), ("rev", C.c_uint8), ("bases", C.c_int32), ("hc_bases", C.c_int32),
                         ("min_len", C.c_uint32), ("score", C.c_double), ("variance", C.c_double))


class ClusterReport(C.Structure):
    _fields_ = [("n", C.c_uint64)] + [(f, C.POINTER(t)) for f, t in CLUSTER_REPORT_FIELDS]


class AssignParams(C.Structure):
    _fields_ = [("t_s", C.c_double), ("t_v", C.c_double), ("bv_threshold", C.c_double), ("use_hc", C.c_int), ("is_rna", C.c_int),
                ("target_batch", C.c_uint32), ("read_chunk", C.c_uint32), ("count_pass", C.c_int)]


# the per-read record of assign (rattle_assignment): one entry per read
ASSIGN_FIELDS = (("target", C.c_int32), ("rev", C.c_uint8), ("bases", C.c_int32), ("hc_bases", C.c_int32), ("min_len", C.c_uint32),
                 ("score", C.c_double), ("variance", C.c_double), ("second_score", C.c_double), ("n_accepted", C.c_uint32))


class Assignment(C.Structure):
    _fields_ = [("n", C.c_uint32)] + [(f, C.POINTER(t)) for f, t in ASSIGN_FIELDS]


# a slot of the candidate list of assign_*_top (rattle_candidates): k entries per read, slot r * k + j
CANDIDATE_FIELDS = (("target", C.c_int32), ("rev", C.c_uint8), ("bases", C.c_int32), ("hc_bases", C.c_int32), ("min_len", C.c_uint32),
                    ("score", C.c_double), ("variance", C.c_double))


class Candidates(C.Structure):
    _fields_ = [("n", C.c_uint32), ("k", C.c_uint32), ("count", C.POINTER(C.c_uint32))] + [(f, C.POINTER(t)) for f, t in CANDIDATE_FIELDS]


# the EM of rattle_hip_abundance: its parameters and its result (per target, per iteration, per slot)
class AbundanceParams(C.Structure):
    _fields_ = [("ratio", C.c_double), ("tol", C.c_double), ("max_iters", C.c_uint32), ("iter_block", C.c_uint32)]


class Abundance(C.Structure):
    _fields_ = [("n_targets", C.c_uint32), ("n_reads", C.c_uint32), ("k", C.c_uint32), ("iterations", C.c_uint32), ("converged", C.c_int),
                ("n_placed", C.c_uint64), ("units", C.POINTER(C.c_uint64)), ("est_reads", C.POINTER(C.c_double)),
                ("cpm", C.POINTER(C.c_double)), ("compatible_reads", C.POINTER(C.c_uint32)), ("delta", C.POINTER(C.c_uint64)),
                ("posterior", C.POINTER(C.c_double))]


class AlignParams(C.Structure):
    _fields_ = [("max_cells", C.c_uint64), ("pair_chunk", C.c_uint32)]


# the scoring of align_pairs_scored / align_cigars_scored (rattle_align_scoring): four positive magnitudes
class AlignScoring(C.Structure):
    _fields_ = [("match", C.c_uint32), ("mismatch", C.c_uint32), ("gap_open", C.c_uint32), ("gap_extend", C.c_uint32)]


# the per-read record of align_pairs (rattle_alignment): one entry per read
ALIGN_FIELDS = (("status", C.c_uint8), ("score", C.c_int32), ("q_start", C.c_uint32), ("q_end", C.c_uint32), ("t_start", C.c_uint32),
                ("t_end", C.c_uint32), ("matches", C.c_uint32), ("mismatches", C.c_uint32), ("q_gap", C.c_uint32), ("t_gap", C.c_uint32))


class Alignment(C.Structure):
    _fields_ = [("n", C.c_uint32)] + [(f, C.POINTER(t)) for f, t in ALIGN_FIELDS]


# the CIGARs of align_cigars (rattle_cigars): ops[offset[r] .. offset[r + 1]) of read r, each len << 4 | op
class Cigars(C.Structure):
    _fields_ = [("n", C.c_uint32), ("offset", C.POINTER(C.c_uint64)), ("ops", C.POINTER(C.c_uint32))]


# the table of align_pileup (rattle_pileup): eight arrays of n counts, position p = byte p of the concatenated targets
PILEUP_FIELDS = ("a", "c", "g", "t", "del", "ins", "starts", "ends")


class Pileup(C.Structure):
    _fields_ = [("n", C.c_uint64)] + [(f, C.POINTER(C.c_uint32)) for f in PILEUP_FIELDS]


# int fn(void *user, const void *send, uint64 send_bytes, void *recv, const uint64 *recv_bytes)
ALLGATHERV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64))


class MsaSet(C.Structure):
    _fields_ = [("n_packs", C.c_uint32), ("width", C.POINTER(C.c_uint32)), ("row_offset", C.POINTER(C.c_uint64)),
                ("rows", C.POINTER(C.c_char)), ("counters", C.c_uint64 * 8)]


_P = C.POINTER
_u8p, _u16p, _u32p, _u64p = _P(C.c_uint8), _P(C.c_uint16), _P(C.c_uint32), _P(C.c_uint64)
_i32p, _f64p = _P(C.c_int32), _P(C.c_double)

# name -> (restype, argtypes); kept in step with include/rattle_hip.h (tests/test_abi.py checks it)
SIGNATURES = {
    "rattle_hip_last_error": (C.c_char_p, []),
    "rattle_hip_abi_version": (C.c_int, []),
    "rattle_hip_ctx_create": (C.c_int, [C.c_int, _P(C.c_void_p)]),
    "rattle_hip_ctx_create_host": (C.c_int, [_P(C.c_void_p)]),
    "rattle_hip_ctx_destroy": (None, [C.c_void_p]),
    "rattle_hip_load_reads": (C.c_int, [C.c_void_p, _u8p, _u64p, C.c_uint32, C.c_int, C.c_int]),
    "rattle_hip_get_read_index": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, _u32p, _i32p, _u64p, _u32p]),
    "rattle_hip_bv_filter": (C.c_int, [C.c_void_p, _u32p, C.c_uint32, _u32p, C.c_uint32, _u32p, _u16p, C.c_int, _u8p]),
    "rattle_hip_pair_score": (C.c_int, [C.c_void_p, _u32p, _u32p, _u8p, C.c_uint32, _i32p, _i32p, _i32p, _f64p, _i32p]),
    "rattle_hip_cluster_reads": (C.c_int, [C.c_void_p, _P(ClusterParams), _P(_P(ClusterSet))]),
    "rattle_hip_cluster_subset": (C.c_int, [C.c_void_p, _P(ClusterParams), _u32p, C.c_uint32, _P(_P(ClusterSet))]),
    "rattle_hip_cluster_subsets": (C.c_int, [C.c_void_p, _P(ClusterParams), _u32p, _u64p, C.c_uint32, _P(_P(ClusterSet)), C.c_int]),
    "rattle_hip_debug_phred_symbol": (C.c_int, [C.c_double, _P(C.c_int), _P(C.c_int)]),
    "rattle_hip_debug_evaluate": (C.c_int, [C.c_void_p, _P(ClusterParams), C.c_int, _P(DebugRect), C.c_uint32, _P(_P(DebugEval))]),
    "rattle_hip_debug_evaluate_free": (None, [_P(DebugEval)]),
    "rattle_hip_debug_post_msa": (C.c_int, [C.c_void_p, _P(CorrectParams), C.c_int, _P(DebugMsa), _P(_P(DebugPost))]),
    "rattle_hip_debug_post_msa_free": (None, [_P(DebugPost)]),
    "rattle_hip_stage_reads": (C.c_int, [C.c_void_p, _u8p, _u8p, _u64p, C.c_uint32]),
    "rattle_hip_unstage_reads": (C.c_int, [C.c_void_p]),
    "rattle_hip_cluster_unsorted": (C.c_int, [C.c_void_p, _u8p, _u64p, C.c_uint32, C.c_int, _P(ClusterParams),
                                              _P(_P(ClusterSet))]),
    "rattle_hip_cluster_iso_unsorted": (C.c_int, [C.c_void_p, _u8p, _u64p, C.c_uint32, C.c_int, C.c_int, _P(ClusterParams),
                                                  _P(ClusterParams), _P(_P(ClusterSet)), _u32p]),
    "rattle_hip_cluster_set_free": (None, [_P(ClusterSet)]),
    "rattle_hip_set_cluster_report": (C.c_int, [C.c_void_p, C.c_int]),
    "rattle_hip_cluster_report": (C.c_int, [_P(ClusterSet), _P(_P(ClusterReport))]),
    "rattle_hip_cluster_report_free": (None, [_P(ClusterReport)]),
    "rattle_hip_assign_loaded": (C.c_int, [C.c_void_p, _P(AssignParams), _u32p, C.c_uint32, _u32p, C.c_uint32, _P(_P(Assignment))]),
    "rattle_hip_assign_reads": (C.c_int, [C.c_void_p, _u8p, _u64p, C.c_uint32, _u8p, _u64p, C.c_uint32, C.c_int, _P(AssignParams),
                                          _P(_P(Assignment))]),
    "rattle_hip_assignment_free": (None, [_P(Assignment)]),
    "rattle_hip_assign_loaded_top": (C.c_int, [C.c_void_p, _P(AssignParams), _u32p, C.c_uint32, _u32p, C.c_uint32, C.c_uint32,
                                               _P(_P(Assignment)), _P(_P(Candidates))]),
    "rattle_hip_assign_reads_top": (C.c_int, [C.c_void_p, _u8p, _u64p, C.c_uint32, _u8p, _u64p, C.c_uint32, C.c_int, _P(AssignParams),
                                              C.c_uint32, _P(_P(Assignment)), _P(_P(Candidates))]),
    "rattle_hip_candidates_free": (None, [_P(Candidates)]),
    "rattle_hip_abundance": (C.c_int, [C.c_void_p, _P(Candidates), C.c_uint32, _P(AbundanceParams), _P(_P(Abundance))]),
    "rattle_hip_abundance_free": (None, [_P(Abundance)]),
    "rattle_hip_align_pairs": (C.c_int, [C.c_void_p, _u8p, _u64p, C.c_uint32, _u8p, _u64p, C.c_uint32, _i32p, _u8p, _P(AlignParams),
                                         _P(_P(Alignment))]),
    "rattle_hip_alignment_free": (None, [_P(Alignment)]),
    "rattle_hip_align_cigars": (C.c_int, [C.c_void_p, _u8p, _u64p, C.c_uint32, _u8p, _u64p, C.c_uint32, _i32p, _u8p, _P(AlignParams),
                                          _P(_P(Alignment)), _P(_P(Cigars))]),
    "rattle_hip_cigars_free": (None, [_P(Cigars)]),
    "rattle_hip_align_pairs_scored": (C.c_int, [C.c_void_p, _u8p, _u64p, C.c_uint32, _u8p, _u64p, C.c_uint32, _i32p, _u8p, _P(AlignParams),
                                                _P(AlignScoring), _P(_P(Alignment))]),
    "rattle_hip_align_cigars_scored": (C.c_int, [C.c_void_p, _u8p, _u64p, C.c_uint32, _u8p, _u64p, C.c_uint32, _i32p, _u8p, _P(AlignParams),
                                                 _P(AlignScoring), _P(_P(Alignment)), _P(_P(Cigars))]),
    "rattle_hip_align_pairs_mode": (C.c_int, [C.c_void_p, _u8p, _u64p, C.c_uint32, _u8p, _u64p, C.c_uint32, _i32p, _u8p, _P(AlignParams),
                                              _P(AlignScoring), C.c_int, _P(_P(Alignment))]),
    "rattle_hip_align_cigars_mode": (C.c_int, [C.c_void_p, _u8p, _u64p, C.c_uint32, _u8p, _u64p, C.c_uint32, _i32p, _u8p, _P(AlignParams),
                                               _P(AlignScoring), C.c_int, _P(_P(Alignment)), _P(_P(Cigars))]),
    "rattle_hip_align_pileup": (C.c_int, [C.c_void_p, _u8p, _u64p, C.c_uint32, _u8p, _u64p, C.c_uint32, _i32p, _u8p, _P(AlignParams),
                                          _P(AlignScoring), C.c_int, _P(_P(Alignment)), _P(_P(Cigars)), _P(_P(Pileup))]),
    "rattle_hip_pileup_free": (None, [_P(Pileup)]),
    "rattle_hip_poa_msa": (C.c_int, [C.c_void_p, _u8p, _u64p, C.c_uint32, _u32p, C.c_uint32, _P(_P(MsaSet))]),
    "rattle_hip_msa_set_free": (None, [_P(MsaSet)]),
    "rattle_hip_correct_reads": (C.c_int, [C.c_void_p, _u8p, _u8p, _u64p, C.c_uint32, C.c_uint32, _u32p, _i32p, _u8p,
                                           _P(CorrectParams), _P(_P(Correction))]),
    "rattle_hip_correction_free": (None, [_P(Correction)]),
    "rattle_hip_set_correction_report": (C.c_int, [C.c_void_p, C.c_int]),
    "rattle_hip_correction_report": (C.c_int, [_P(Correction), _P(_P(CorrectionReport))]),
    "rattle_hip_correction_report_free": (None, [_P(CorrectionReport)]),
    "rattle_hip_set_consensus_support": (C.c_int, [C.c_void_p, C.c_int]),
    "rattle_hip_consensus_support": (C.c_int, [_P(Correction), _P(_P(ConsensusSupport))]),
    "rattle_hip_consensus_support_free": (None, [_P(ConsensusSupport)]),
    "rattle_hip_debug_consensus_support": (C.c_int, [C.c_void_p, _P(CorrectParams), _P(DebugSupportMsa), _P(_P(DebugSupport))]),
    "rattle_hip_debug_consensus_support_free": (None, [_P(DebugSupport)]),
    "rattle_hip_reserve_arena": (C.c_int, [C.c_void_p, C.c_uint64]),
    "rattle_hip_set_exchange": (C.c_int, [C.c_void_p, C.c_int, C.c_int, ALLGATHERV_FN, C.c_void_p]),
    "rattle_hip_comm_unique_id": (C.c_int, [_u8p]),
    "rattle_hip_comm_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _u8p]),
    "rattle_hip_comm_destroy": (C.c_int, [C.c_void_p]),
    "rattle_hip_comm_stats": (C.c_int, [C.c_void_p, _u64p, _u64p]),
    "rattle_hip_comm_probe": (C.c_int, [C.c_void_p]),
    "rattle_hip_correction_gather": (C.c_int, [C.c_void_p, _P(Correction), C.c_int, _P(_P(Correction))]),
    "rattle_hip_plan_packs": (C.c_int, [_u64p, C.c_uint32, C.c_uint32, _u32p, _i32p, _u8p, _P(CorrectParams), C.c_int,
                                        _P(_P(PackPlan))]),
    "rattle_hip_pack_plan_free": (None, [_P(PackPlan)]),
    "rattle_hip_lpt_assign": (C.c_int, [_u64p, C.c_uint32, C.c_int, _u32p]),
    "rattle_hip_kernel_stats": (C.c_int, [C.c_void_p, C.c_int, _f64p, _u64p, _u64p]),
    "rattle_hip_kernel_stats_reset": (C.c_int, [C.c_void_p]),
    "rattle_hip_stage_ms": (C.c_int, [C.c_void_p, _f64p, C.c_int]),
}

_lib = None


def load():
    """Load librattle_hip.so; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


# return codes of include/rattle_hip.h
RATTLE_OK, RATTLE_ERR_HIP, RATTLE_ERR_ARG, RATTLE_ERR_STATE = 0, -1, -2, -3


class RattleError(RuntimeError):
    pass


def check(rc: int):
    if rc != 0:
        raise RattleError(f"librattle_hip error {rc}: {load().rattle_hip_last_error().decode()}")
