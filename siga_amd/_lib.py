"""ctypes bindings of include/sigax.h.  Fails loudly when the native library is missing."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SIGAX_LIB", os.path.join(HERE, "lib", "libsigax.so"))

SIGAX_IRREDUCIBLE = 1
SIGAX_RC = 2
SIGAX_EDGES = 4
SIGAX_DUPLICATE = 8
SIGAX_E_ARG = -1
SIGAX_E_STATE = -6

BLOCK_DTYPE = np.dtype([
    ("capped0_lo", "<u8"), ("capped0_hi", "<u8"), ("capped1_lo", "<u8"), ("capped1_hi", "<u8"),
    ("raw0_lo", "<u8"), ("raw0_hi", "<u8"), ("raw1_lo", "<u8"), ("raw1_hi", "<u8"),
    ("length", "<u4"), ("af", "<u4"), ("reserved", "<u8")])
EDGE_DTYPE = np.dtype([("query", "<u4"), ("target", "<u4"), ("length", "<u4"), ("af", "<u4")])
HIT_DTYPE = np.dtype([("query", "<u4"), ("read", "<u4"), ("offset", "<u4"), ("flags", "<u4")])  # sigax_hit
PLACEMENT_DTYPE = np.dtype([("read", "<u4"), ("flags", "<u4"), ("offset", "<u8")])  # sigax_placement
MM_EDGE_DTYPE = np.dtype([("query", "<u4"), ("target", "<u4"), ("length", "<u4"), ("af", "<u4"), ("num_diff", "<u4"), ("reserved", "<u4")])  # sigax_mm_edge
assert MM_EDGE_DTYPE.itemsize == 24
assert BLOCK_DTYPE.itemsize == 80 and EDGE_DTYPE.itemsize == 16 and HIT_DTYPE.itemsize == 16 and PLACEMENT_DTYPE.itemsize == 16
SIGAX_HIT_REV = 1
SIGAX_HIT_CUT = 2
SIGAX_LOCATE_SKIPPED = 1
SIGAX_LOCATE_OVER = 2
SIGAX_PLACED_REV = 1
SIGAX_UNITIG_CIRCULAR = 1
SIGAX_TRIM_NO_COVERAGE = 0xFFFFFFFF
SIGAX_REMOVED_CHIMERIC = 0x80000000
SIGAX_REMOVED_BUBBLE = 0x40000000
SIGAX_BUBBLE_NO_BASES = 0xFFFFFFFF
SIGAX_REMOVED_INDEL = 0x20000000
SIGAX_INDEL_MAX_EDITS = 31
SIGAX_INDEL_MAX_SPAN = 4096
# the entries 24-31 of sigax_unitigs_indel_*'s status32, by name
INDEL_STATUS = ("indel_popped", "indel_reads", "indel_rounds", "indel_kept", "indel_not_compared", "_29", "_30", "_31")
# bit 31 of cut[]: transitive in the latest reduction pass (sigax_unitigs_reduce_*); the low bits stay the round of a -d cut
SIGAX_CUT_TRANSITIVE = 0x80000000
# the entries 32-39 of sigax_unitigs_reduce_*'s status40, by name
REDUCE_STATUS = ("reduce_first", "reduce_final", "reduce_passes", "reduce_participants", "_36", "_37", "_38", "_39")
TRIM_MAX_ROUNDS = 64
SIGAX_NO_MATE = 0xFFFFFFFF
SIGAX_PAIRS_OUTWARD = 1
SIGAX_PAIRS_MAX_BINS = 8192
PAIR_LINK_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("count", "<u4"), ("min_span", "<u4"), ("sum_span", "<u8")])  # sigax_pair_link
assert PAIR_LINK_DTYPE.itemsize == 24
# the entries of sigax_consensus_*'s status8, by name
CONSENSUS_STATUS = ("unitigs", "columns", "changed", "shallow", "ties", "held_back", "max_depth", "invalid_placements")
# the entries of sigax_unitigs_pairs_*'s status24, by name
PAIRS_STATUS = ("mate_entries", "malformed", "pairs", "unplaced", "same", "inward", "outward", "tandem", "ring", "far", "d_n", "d_sum",
                "d_sq_low", "d_sq_high", "span_n", "span_sum", "span_sq_low", "span_sq_high", "across", "ring_links_dropped", "over_max_span",
                "linked_pairs", "link_records", "reserved")
SIGAX_SCAFFOLD_INSERT_FROM_STATUS = 1
# the entries of sigax_scaffold_*'s status16, by name
SCAFFOLD_STATUS = ("scaffolds", "bases", "links", "malformed", "self", "circular", "short", "thin", "weak", "ambiguous", "joins", "cycles",
                   "gap_bases", "below_min_gap", "clamped_at_max_gap", "bases_not_written")
# sigax_gapfill_*: the classes of a gap (sigax_gap.cls, .fwd, .rev), the record and the entries of status24, by name
GAP_CLASSES = ("FILLED", "SHORT", "NON_ACGT", "FAR", "NO_ROOM", "DEAD_END", "BRANCH", "TOO_LONG", "OVERLAP", "OFF_ESTIMATE", "MALFORMED")
SIGAX_GAP_NOT_RUN = 255
SIGAX_GAPFILL_AUTO = 0xFFFFFFFFFFFFFFFF
GAP_DTYPE = np.dtype([("scaffold", "<u4"), ("left", "<u4"), ("right", "<u4"), ("laid", "<u4"), ("fill", "<u4"), ("cls", "u1"), ("fwd", "u1"),
                      ("rev", "u1"), ("dir", "u1"), ("offset", "<u8")])  # sigax_gap
assert GAP_DTYPE.itemsize == 32
GAPFILL_STATUS = ("gaps",) + tuple(c.lower() for c in GAP_CLASSES) + (
    "filled_forward", "filled_reverse", "fill_bases", "n_bases_left", "bases", "steps", "lookups", "sectors", "bases_not_written",
    "walk_scratch_too_small", "scaffolds", "reserved")
assert len(GAPFILL_STATUS) == 24
# sigax_join_*: the classes of a gap (sigax_join.cls), the record and the entries of status16, by name
JOIN_CLASSES = ("JOINED", "CLOSED", "FAR", "SHORT", "NONE", "AMBIGUOUS", "UNSUPPORTED", "MALFORMED")
JOIN_DTYPE = np.dtype([("scaffold", "<u4"), ("left", "<u4"), ("right", "<u4"), ("laid", "<u4"), ("overlap", "<u4"), ("cls", "u1"), ("matches", "u1"),
                       ("windows", "<u2"), ("offset", "<u8")])  # sigax_join
assert JOIN_DTYPE.itemsize == 32
JOIN_STATUS = ("gaps",) + tuple(c.lower() for c in JOIN_CLASSES) + (
    "overlap_bases_removed", "n_bases_removed", "bases", "candidates", "windows", "bases_not_written", "scaffolds")
assert len(JOIN_STATUS) == 16
# sigax_join_approx_*: status24, and the fields of an mm entry
JOIN_APPROX_STATUS = JOIN_STATUS + ("approx_joined", "mismatch_columns", "columns_from_right", "approx_candidates", "choice_windows", "_21", "_22", "_23")
assert len(JOIN_APPROX_STATUS) == 24
JOIN_MM_APPROX = 1 << 16  # mm = mismatches | taken_right << 8 | JOIN_MM_APPROX


class TrimOpts(C.Structure):  # sigax_trim_opts
    _fields_ = [(n, C.c_uint32) for n in ("max_rounds", "min_branch_length", "min_branch_coverage", "reserved")]


class PruneOpts(C.Structure):  # sigax_prune_opts
    _fields_ = ([(n, C.c_uint32) for n in ("max_rounds", "min_branch_length", "min_branch_coverage", "delta", "careful", "reserved")] +
                [("num_reads", C.c_uint64), ("genome_size", C.c_uint64), ("uniq_threshold", C.c_double)])


class ChimericOpts(C.Structure):  # sigax_chimeric_opts
    _fields_ = ([("prune", PruneOpts)] +
                [(n, C.c_uint32) for n in ("min_chimeric_length", "min_chimeric_coverage", "chimeric_delta", "reserved2")] +
                [("chimeric_threshold", C.c_double)])


class BubbleOpts(C.Structure):  # sigax_bubble_opts
    _fields_ = [("chimeric", ChimericOpts), ("max_bubble_span", C.c_uint32), ("max_divergence_permille", C.c_uint32),
                ("reserved3", C.c_uint32 * 2)]


class IndelOpts(C.Structure):  # sigax_indel_opts
    _fields_ = [("bubble", BubbleOpts), ("max_edits", C.c_uint32), ("max_edit_permille", C.c_uint32), ("reserved4", C.c_uint32 * 2)]


class ReduceOpts(C.Structure):  # sigax_reduce_opts
    _fields_ = [("indel", IndelOpts), ("reduce", C.c_uint32), ("reserved5", C.c_uint32 * 3)]


class ContainedOpts(C.Structure):  # sigax_contained_opts
    _fields_ = [("reserved", C.c_uint32 * 4)]


# sigax_contained_place_*: place_class values and the entries of status8, by name
CP_CLASSES = ("not_contained", "placed", "no_record", "no_root", "root_removed", "invalid")
CONTAINED_STATUS = ("contained", "records", "records_invalid", "placed", "no_chain", "root_removed", "longest_chain", "placements")
PLACED_CONTAINED = 2  # SIGAX_PLACED_CONTAINED


class ConsensusOpts(C.Structure):  # sigax_consensus_opts
    _fields_ = [("min_votes", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class PairsOpts(C.Structure):  # sigax_pairs_opts
    _fields_ = [(n, C.c_uint32) for n in ("flags", "hist_bins", "hist_shift", "reserved")] + [("max_span", C.c_uint64)]


class ScaffoldOpts(C.Structure):  # sigax_scaffold_opts
    _fields_ = ([(n, C.c_uint32) for n in ("flags", "min_pairs", "link_ratio", "min_unitig_bases")] + [("insert_size", C.c_uint64)] +
                [(n, C.c_uint32) for n in ("min_gap", "max_gap")])


class GapfillOpts(C.Structure):  # sigax_gapfill_opts
    _fields_ = [(n, C.c_uint32) for n in ("flags", "k", "min_count", "slack", "max_fill", "reserved")]


class JoinOpts(C.Structure):  # sigax_join_opts
    _fields_ = [(n, C.c_uint32) for n in ("flags", "min_overlap", "max_overlap", "slack", "k", "min_count", "reserved")]


class JoinApproxOpts(C.Structure):  # sigax_join_approx_opts
    _fields_ = [(n, C.c_uint32) for n in ("flags", "min_overlap", "max_overlap", "slack", "k", "min_count", "max_mismatches", "mismatch_permille",
                                          "reserved")]


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "n_reads", "n_candidate_blocks", "n_blocks", "n_edges", "n_occ_find", "n_occ_extract", "n_substring",
        "n_slow_reads", "n_extract_errors", "n_sectors_find", "n_sectors_extract")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class Result(C.Structure):
    _fields_ = [("n_reads", C.c_uint32), ("block_offs", C.POINTER(C.c_uint64)), ("blocks", C.c_void_p),
                ("substring", C.POINTER(C.c_uint8)), ("n_edges", C.c_uint64), ("edges", C.c_void_p), ("stats", Stats)]


class IndexInfo(C.Structure):
    _fields_ = [("n_symbols", C.c_uint64), ("n_strings", C.c_uint64), ("device_bytes", C.c_uint64),
                ("pred", C.c_uint64 * 5), ("device", C.c_int), ("wide", C.c_int)]


class PileParams(C.Structure):
    """sigax_pile_params (`siga correct -a overlap`); the defaults are the CLI's"""
    _fields_ = [(n, C.c_uint32) for n in ("seed_length", "seed_stride", "max_seed_hits", "min_overlap", "error_permille", "conflict",
                                          "min_depth", "max_candidates", "max_read_len", "reserved")]

    def __init__(self, seed_length=24, seed_stride=12, max_seed_hits=256, min_overlap=45, error_permille=40, conflict=5, min_depth=2,
                 max_candidates=512, max_read_len=0):
        super().__init__(seed_length, seed_stride, max_seed_hits, min_overlap, error_permille, conflict, min_depth, max_candidates,
                         max_read_len, 0)


MMO_CONTAINMENTS = 1  # SIGAX_MMO_CONTAINMENTS
MM_CONTAINMENT = 8    # SIGAX_MM_CONTAINMENT


class MmoParams(C.Structure):
    """sigax_mmo_params (`siga overlap -e`); the defaults are the CLI's, error_permille has none"""
    _fields_ = [(n, C.c_uint32) for n in ("seed_length", "seed_stride", "max_seed_hits", "min_overlap", "error_permille", "max_candidates",
                                          "max_read_len", "flags")]

    def __init__(self, error_permille, seed_length=24, seed_stride=12, max_seed_hits=256, min_overlap=45, max_candidates=512, max_read_len=0,
                 flags=0):
        super().__init__(seed_length, seed_stride, max_seed_hits, min_overlap, error_permille, max_candidates, max_read_len, flags)


class RunInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("n_sub", "find_per_sub", "two_step", "coop", "read_order", "cap", "worst_cap", "row_bits",
                                          "row_syms", "row_text", "row_direct", "deep_k")] + \
               [("arena_bytes", C.c_uint64), ("workspace_bytes", C.c_uint64), ("reruns", C.c_uint64), ("order_ms", C.c_float)]

    def as_dict(self):
        return {n: (float(getattr(self, n)) if n == "order_ms" else int(getattr(self, n))) for n, _ in self._fields_}


# every symbol include/sigax.h declares (tests check that the library exports all of them)
SYMBOLS = [
    "sigax_last_error", "sigax_device_count", "sigax_stream_create", "sigax_stream_destroy", "sigax_index_open", "sigax_index_open_mem", "sigax_index_prepare", "sigax_index_prepare_overlap", "sigax_index_clone", "sigax_index_close",
    "sigax_index_info_get", "sigax_index_set_reads", "sigax_index_check_order", "sigax_occ_batch", "sigax_kmer_count_batch",
    "sigax_correct_batch", "sigax_correct_device", "sigax_overlap_batch", "sigax_result_free", "sigax_batch_create", "sigax_batch_destroy", "sigax_batch_upload",
    "sigax_batch_set_device_reads", "sigax_batch_upload_read_ids", "sigax_batch_set_device_read_ids", "sigax_batch_set_subbatches", "sigax_batch_run", "sigax_batch_finish", "sigax_batch_device_outputs",
    "sigax_batch_download", "sigax_batch_download_edges", "sigax_batch_size_hint", "sigax_batch_kernel_ms", "sigax_batch_run_info", "sigax_build_strand", "sigax_build_session", "sigax_free",
    "sigax_comm_unique_id", "sigax_comm_create", "sigax_comm_destroy", "sigax_gather_counts", "sigax_gather_edges",
    "sigax_locality_keys",
    "sigax_match_batch", "sigax_match_device", "sigax_matcher_create", "sigax_matcher_destroy", "sigax_matcher_capacity",
    "sigax_matcher_submit", "sigax_matcher_wait",
    "sigax_string_lengths_device", "sigax_get_strings_device", "sigax_get_strings", "sigax_kmer_spectrum_workspace",
    "sigax_kmer_spectrum_device", "sigax_kmer_spectrum_batch", "sigax_kmer_spectrum_rows", "sigax_kmer_spectrum_rows_hint",
    "sigax_locate_workspace", "sigax_locate_device", "sigax_locate_batch",
    "sigax_reference_text_workspace", "sigax_reference_text_device", "sigax_pileup_workspace", "sigax_pileup_device",
    "sigax_pile_ref_create", "sigax_pile_ref_destroy", "sigax_pile_ref_buffers", "sigax_pileup_batch",
    "sigax_mmoverlap_workspace", "sigax_mmoverlap_device", "sigax_mmoverlap_finish_workspace", "sigax_mmoverlap_finish_device",
    "sigax_mmoverlap_batch",
    "sigax_unitigs_workspace", "sigax_unitigs_device", "sigax_unitigs_host", "sigax_unitigs_last_status",
    "sigax_unitigs_trim_workspace", "sigax_unitigs_trim_device", "sigax_unitigs_trim_host",
    "sigax_unitigs_prune_workspace", "sigax_unitigs_prune_device", "sigax_unitigs_prune_host",
    "sigax_unitigs_chimeric_workspace", "sigax_unitigs_chimeric_device", "sigax_unitigs_chimeric_host",
    "sigax_unitigs_bubble_workspace", "sigax_unitigs_bubble_device", "sigax_unitigs_bubble_host",
    "sigax_unitigs_indel_workspace", "sigax_unitigs_indel_device", "sigax_unitigs_indel_host",
    "sigax_unitigs_reduce_workspace", "sigax_unitigs_reduce_device", "sigax_unitigs_reduce_host",
    "sigax_consensus_workspace", "sigax_consensus_device", "sigax_consensus_host",
    "sigax_contained_place_workspace", "sigax_contained_place_device", "sigax_contained_place_host",
    "sigax_unitigs_pairs_workspace", "sigax_unitigs_pairs_device", "sigax_unitigs_pairs_host", "sigax_pairs_estimate",
    "sigax_scaffold_workspace", "sigax_scaffold_device", "sigax_scaffold_host",
    "sigax_gapfill_workspace", "sigax_gapfill_device", "sigax_gapfill_host",
    "sigax_join_workspace", "sigax_join_device", "sigax_join_host",
    "sigax_join_approx_workspace", "sigax_join_approx_device", "sigax_join_approx_host",
    "sigax_edges_order_workspace", "sigax_edges_restore_order", "sigax_edges_restore_order_host", "sigax_flags_by_read_id",
]

_lib = None


def lib():
    """Load libsigax.so.  No fallback: a missing library is an error, not a slow path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "siga_amd native library missing: %s (build it with `python -m siga_amd.build` or "
            "__graft_entry__.build()); there is no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, u32, u64, cp, ci = C.c_void_p, C.c_uint32, C.c_uint64, C.c_char_p, C.c_int
    pvp = C.POINTER(C.c_void_p)
    L.sigax_last_error.restype = cp
    L.sigax_device_count.argtypes = [C.POINTER(ci)]
    L.sigax_stream_create.argtypes = [ci, C.POINTER(C.c_void_p)]
    L.sigax_stream_destroy.argtypes = [ci, C.c_void_p]
    L.sigax_stream_destroy.restype = None
    L.sigax_index_open.argtypes = [cp, cp, cp, cp, ci, pvp]
    L.sigax_index_open_mem.argtypes = [vp, u64, vp, u64, u64, u64, vp, vp, ci, pvp]
    L.sigax_index_prepare.argtypes = [vp]
    L.sigax_index_prepare_overlap.argtypes = [vp, u32]
    L.sigax_index_clone.argtypes = [vp, ci, pvp]
    L.sigax_index_close.argtypes = [vp]
    L.sigax_index_close.restype = None
    L.sigax_index_info_get.argtypes = [vp, C.POINTER(IndexInfo)]
    L.sigax_index_set_reads.argtypes = [vp, vp, vp, u64]
    L.sigax_index_check_order.argtypes = [vp, ci, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.sigax_occ_batch.argtypes = [vp, ci, vp, u64, vp]
    L.sigax_kmer_count_batch.argtypes = [vp, cp, u32, u64, vp]
    L.sigax_correct_batch.argtypes = [vp, cp, cp, vp, u32, u32, C.c_int32, u32, u32, vp, vp]
    L.sigax_correct_device.argtypes = [vp, vp, vp, vp, u64, u32, C.c_int32, u32, u32, vp, vp, vp, vp]
    L.sigax_overlap_batch.argtypes = [vp, cp, vp, u32, u32, u32, u32, C.POINTER(Result)]
    L.sigax_result_free.argtypes = [C.POINTER(Result)]
    L.sigax_result_free.restype = None
    L.sigax_batch_create.argtypes = [vp, u32, u64, u32, pvp]
    L.sigax_batch_destroy.argtypes = [vp]
    L.sigax_batch_destroy.restype = None
    L.sigax_batch_upload.argtypes = [vp, cp, vp, u32, vp]
    L.sigax_batch_set_device_reads.argtypes = [vp, vp, vp, u32, u64, u32]
    L.sigax_batch_upload_read_ids.argtypes = [vp, vp, u32, vp]
    L.sigax_locality_keys.argtypes = [C.c_int, vp, vp, u32, vp, vp]
    L.sigax_batch_set_device_read_ids.argtypes = [vp, vp, u32]
    L.sigax_batch_run.argtypes = [vp, u32, u32, u32, vp]
    L.sigax_batch_finish.argtypes = [vp, vp, C.POINTER(Stats)]
    L.sigax_batch_device_outputs.argtypes = [vp, pvp, pvp, pvp, pvp]
    L.sigax_batch_download.argtypes = [vp, C.POINTER(Result)]
    L.sigax_batch_download_edges.argtypes = [vp, vp, pvp, C.POINTER(u64)]
    L.sigax_batch_size_hint.argtypes = [vp, u32, u32, u32, u32, C.POINTER(u32)]
    L.sigax_batch_kernel_ms.argtypes = [vp, C.POINTER(C.c_float * 5), C.POINTER(C.c_uint32)]
    L.sigax_batch_set_subbatches.argtypes = [vp, u32]
    L.sigax_batch_run_info.argtypes = [vp, C.POINTER(RunInfo)]
    L.sigax_build_strand.argtypes = [vp, vp, u64, ci, ci, pvp, C.POINTER(u64), pvp, C.POINTER(u64)]
    L.sigax_free.argtypes = [vp]
    L.sigax_free.restype = None
    L.sigax_build_session.argtypes = [ci]
    L.sigax_build_session.restype = None
    L.sigax_comm_unique_id.argtypes = [vp]
    L.sigax_comm_create.argtypes = [ci, ci, ci, vp, pvp]
    L.sigax_comm_destroy.argtypes = [vp]
    L.sigax_comm_destroy.restype = None
    L.sigax_gather_counts.argtypes = [vp, u64, vp, vp]
    L.sigax_gather_edges.argtypes = [vp, vp, vp, ci, vp, vp]
    L.sigax_match_batch.argtypes = [vp, cp, vp, u64, u64, u32, vp]
    L.sigax_match_device.argtypes = [vp, vp, vp, u64, u64, u32, vp, vp, vp]
    L.sigax_matcher_create.argtypes = [vp, u32, u64, u64, pvp]
    L.sigax_matcher_destroy.argtypes = [vp]
    L.sigax_matcher_destroy.restype = None
    L.sigax_matcher_capacity.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.sigax_matcher_submit.argtypes = [vp, u32, cp, vp, u64, u64, u32]
    L.sigax_matcher_wait.argtypes = [vp, u32, pvp, C.POINTER(u64 * 4)]
    L.sigax_string_lengths_device.argtypes = [vp, ci, vp, u64, u32, vp, vp, vp, vp]
    L.sigax_get_strings_device.argtypes = [vp, ci, vp, u64, u32, vp, vp, vp, vp]
    L.sigax_get_strings.argtypes = [vp, ci, vp, u64, u32, pvp, pvp, vp]
    L.sigax_kmer_spectrum_workspace.argtypes = [u64, C.POINTER(u64)]
    L.sigax_kmer_spectrum_device.argtypes = [vp, vp, vp, u64, u32, u64, vp, vp, vp, u64, vp]
    L.sigax_kmer_spectrum_batch.argtypes = [vp, cp, vp, u64, u32, u64, vp, vp]
    L.sigax_kmer_spectrum_rows.argtypes = [vp, vp, u64, u32, u32, u64, vp, vp]
    L.sigax_kmer_spectrum_rows_hint.argtypes = [vp, u32, u64, C.POINTER(u64)]
    L.sigax_locate_workspace.argtypes = [u64, C.POINTER(u64)]
    L.sigax_locate_device.argtypes = [vp, vp, vp, u64, u32, u32, u32, vp, vp, vp, vp, vp, u64, vp, vp, u64, vp]
    L.sigax_locate_batch.argtypes = [vp, cp, vp, u64, u32, u32, u32, pvp, pvp, pvp, pvp]
    pp = C.POINTER(PileParams)
    L.sigax_reference_text_workspace.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.sigax_reference_text_device.argtypes = [vp, vp, u64, vp, vp, vp, u64, vp]
    L.sigax_pileup_workspace.argtypes = [u64, u64, pp, u64, C.POINTER(u64)]
    L.sigax_pileup_device.argtypes = [vp, vp, vp, u64, u64, pp, vp, vp, vp, vp, vp, vp, vp, u64, u64, vp]
    # (not in include/sigax.h: the measurement aid of tools/pileup_bench.py, sigax_pileup.h)
    L.sigax_pileup_pile_device.argtypes = L.sigax_pileup_device.argtypes
    L.sigax_pile_ref_create.argtypes = [vp, pvp]
    L.sigax_pile_ref_destroy.argtypes = [vp]
    L.sigax_pile_ref_destroy.restype = None
    L.sigax_pile_ref_buffers.argtypes = [vp, pvp, pvp, C.POINTER(u64)]
    L.sigax_pileup_batch.argtypes = [vp, vp, cp, vp, u64, pp, u32, vp, vp, vp, vp, C.POINTER(u32)]
    mp = C.POINTER(MmoParams)
    L.sigax_mmoverlap_workspace.argtypes = [u64, u64, mp, u64, C.POINTER(u64)]
    L.sigax_mmoverlap_device.argtypes = [vp, vp, vp, u64, u64, u64, mp, vp, u64, vp, vp, vp, vp, u64, u64, vp]
    # (not in include/sigax.h: the measurement aid of tools/mmoverlap_bench.py, sigax_mmoverlap.h)
    L.sigax_mmoverlap_stages_device.argtypes = L.sigax_mmoverlap_device.argtypes + [ci]
    L.sigax_mmoverlap_finish_workspace.argtypes = [u64, C.POINTER(u64)]
    L.sigax_mmoverlap_finish_device.argtypes = [vp, u64, vp, vp, u64, vp]
    L.sigax_mmoverlap_batch.argtypes = [vp, vp, mp, pvp, C.POINTER(u64), vp, vp]
    L.sigax_unitigs_workspace.argtypes = [u64, u64, C.POINTER(u64)]
    L.sigax_unitigs_device.argtypes = [ci, vp, u64, vp, vp, vp, u64, u32, vp, vp, vp, vp, vp, vp, vp, u64, vp]
    L.sigax_unitigs_host.argtypes = [ci, vp, u64, vp, cp, vp, u64, u32, C.POINTER(u64), pvp, pvp, pvp, pvp, pvp]
    L.sigax_unitigs_last_status.argtypes = [vp]
    L.sigax_unitigs_trim_workspace.argtypes = [u64, u64, ci, C.POINTER(u64)]
    L.sigax_unitigs_trim_device.argtypes = [ci, vp, u64, vp, vp, vp, u64, u32, C.POINTER(TrimOpts), vp, vp, vp, vp, vp, vp, vp, vp, vp, u64, vp]
    L.sigax_unitigs_trim_host.argtypes = [ci, vp, u64, vp, cp, vp, u64, u32, C.POINTER(TrimOpts), C.POINTER(u64), pvp, pvp, pvp, pvp, pvp, pvp,
                                          pvp, vp]
    L.sigax_unitigs_prune_workspace.argtypes = [u64, u64, ci, ci, C.POINTER(u64)]
    L.sigax_unitigs_prune_device.argtypes = [ci, vp, u64, vp, vp, vp, u64, u32, C.POINTER(PruneOpts), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                             u64, vp]
    L.sigax_unitigs_prune_host.argtypes = [ci, vp, u64, vp, cp, vp, u64, u32, C.POINTER(PruneOpts), C.POINTER(u64), pvp, pvp, pvp, pvp, pvp,
                                           pvp, pvp, pvp, vp]
    L.sigax_unitigs_chimeric_workspace.argtypes = [u64, u64, ci, ci, C.POINTER(u64)]
    L.sigax_unitigs_chimeric_device.argtypes = [ci, vp, u64, vp, vp, vp, u64, u32, C.POINTER(ChimericOpts), vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                                vp, u64, vp]
    L.sigax_unitigs_chimeric_host.argtypes = [ci, vp, u64, vp, cp, vp, u64, u32, C.POINTER(ChimericOpts), C.POINTER(u64), pvp, pvp, pvp, pvp,
                                              pvp, pvp, pvp, pvp, vp]
    L.sigax_unitigs_bubble_workspace.argtypes = [u64, u64, ci, ci, C.POINTER(u64)]
    L.sigax_unitigs_bubble_device.argtypes = [ci, vp, u64, vp, vp, vp, u64, u32, C.POINTER(BubbleOpts), vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                              vp, u64, vp]
    L.sigax_unitigs_bubble_host.argtypes = [ci, vp, u64, vp, cp, vp, u64, u32, C.POINTER(BubbleOpts), C.POINTER(u64), pvp, pvp, pvp, pvp,
                                            pvp, pvp, pvp, pvp, vp]
    L.sigax_unitigs_indel_workspace.argtypes = [u64, u64, ci, ci, C.POINTER(u64)]
    L.sigax_unitigs_indel_device.argtypes = [ci, vp, u64, vp, vp, vp, u64, u32, C.POINTER(IndelOpts), vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                             vp, u64, vp]
    L.sigax_unitigs_indel_host.argtypes = [ci, vp, u64, vp, cp, vp, u64, u32, C.POINTER(IndelOpts), C.POINTER(u64), pvp, pvp, pvp, pvp,
                                           pvp, pvp, pvp, pvp, vp]
    L.sigax_unitigs_reduce_workspace.argtypes = [u64, u64, ci, ci, C.POINTER(u64)]
    L.sigax_unitigs_reduce_device.argtypes = [ci, vp, u64, vp, vp, vp, u64, u32, C.POINTER(ReduceOpts), vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                              vp, u64, vp]
    L.sigax_unitigs_reduce_host.argtypes = [ci, vp, u64, vp, cp, vp, u64, u32, C.POINTER(ReduceOpts), C.POINTER(u64), pvp, pvp, pvp, pvp,
                                            pvp, pvp, pvp, pvp, vp]
    L.sigax_consensus_workspace.argtypes = [u64, u64, C.POINTER(u64)]
    L.sigax_consensus_device.argtypes = [ci, vp, u64, vp, vp, vp, vp, vp, vp, u64, C.POINTER(ConsensusOpts), vp, vp, vp, vp, vp, u64, vp]
    L.sigax_consensus_host.argtypes = [ci, u64, vp, vp, vp, vp, cp, vp, u64, C.POINTER(ConsensusOpts), vp, pvp, pvp, vp]
    L.sigax_contained_place_workspace.argtypes = [u64, u64, u64, C.POINTER(u64)]
    L.sigax_contained_place_device.argtypes = [ci, vp, u64, vp, vp, vp, vp, u64, vp, vp, u64, C.POINTER(ContainedOpts), vp, vp, vp, vp, vp, u64, vp]
    L.sigax_contained_place_host.argtypes = [ci, u64, vp, vp, vp, vp, u64, vp, vp, u64, C.POINTER(ContainedOpts), pvp, pvp, pvp, vp]
    L.sigax_unitigs_pairs_workspace.argtypes = [ci, u64, C.POINTER(u64)]
    L.sigax_unitigs_pairs_device.argtypes = [ci, vp, vp, u64, vp, vp, vp, vp, vp, C.POINTER(PairsOpts), vp, vp, vp, vp, u64, vp]
    L.sigax_unitigs_pairs_host.argtypes = [ci, vp, vp, u64, u64, vp, vp, vp, vp, C.POINTER(PairsOpts), pvp, pvp, vp]
    L.sigax_pairs_estimate.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.sigax_scaffold_workspace.argtypes = [u64, u64, C.POINTER(u64)]
    L.sigax_scaffold_device.argtypes = [ci, vp, u64, vp, vp, vp, u64, vp, vp, u64, vp, C.POINTER(ScaffoldOpts), vp, vp, vp, vp, vp, u64, vp, vp, u64, vp]
    L.sigax_scaffold_host.argtypes = [ci, u64, vp, vp, vp, vp, u64, vp, C.POINTER(ScaffoldOpts), C.POINTER(u64), pvp, pvp, pvp, pvp, pvp, vp]
    L.sigax_gapfill_workspace.argtypes = [u64, u64, C.POINTER(u64)]
    L.sigax_gapfill_device.argtypes = [vp, vp, u64, vp, vp, u64, vp, vp, vp, C.POINTER(GapfillOpts), vp, vp, vp, u64, vp, vp, vp, u64, u64, vp]
    L.sigax_gapfill_host.argtypes = [vp, u64, vp, vp, u64, vp, vp, C.POINTER(GapfillOpts), u64, pvp, pvp, pvp, pvp, C.POINTER(u64), vp]
    L.sigax_join_workspace.argtypes = [u64, C.POINTER(u64)]
    L.sigax_join_device.argtypes = [vp, vp, u64, vp, vp, vp, vp, vp, vp, u64, C.POINTER(JoinOpts), vp, vp, vp, u64, vp, vp, vp, u64, vp]
    L.sigax_join_host.argtypes = [vp, u64, vp, u64, vp, vp, vp, vp, C.POINTER(JoinOpts), pvp, pvp, pvp, pvp, C.POINTER(u64), vp]
    L.sigax_join_approx_workspace.argtypes = [u64, C.POINTER(u64)]
    L.sigax_join_approx_device.argtypes = [vp, vp, u64, vp, vp, vp, vp, vp, vp, u64, C.POINTER(JoinApproxOpts), vp, vp, vp, u64, vp, vp, vp, vp, u64, vp]
    L.sigax_join_approx_host.argtypes = [vp, u64, vp, u64, vp, vp, vp, vp, C.POINTER(JoinApproxOpts), pvp, pvp, pvp, pvp, C.POINTER(u64), pvp, vp]
    # (not in include/sigax.h: the measurement aid of tools/scaffold_bench.py, sigax_internal.h)
    L.sigax_scaffold_bases_device.argtypes = L.sigax_scaffold_device.argtypes
    # (not in include/sigax.h: the measurement aid of tools/unitig_bench.py, sigax_internal.h)
    L.sigax_unitigs_bases_device.argtypes = [ci, vp, vp, u64, u64, vp, vp, u64, vp]
    L.sigax_edges_order_workspace.argtypes = [u64, u64, C.POINTER(u64)]
    L.sigax_edges_restore_order.argtypes = [ci, vp, u64, u64, vp, vp, vp, u64, vp, vp]
    L.sigax_edges_restore_order_host.argtypes = [ci, vp, u64, u64, vp, vp]
    L.sigax_flags_by_read_id.argtypes = [ci, vp, vp, u64, u64, vp, vp, vp]
    _lib = L
    return L


def last_error():
    return lib().sigax_last_error().decode(errors="replace")
