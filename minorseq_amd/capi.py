"""ctypes binding of libjuliet_hip.so (include/juliet_hip.h) — the reference-side FFI stub, in Python.

The reference has no API for this path beyond the `juliet` command line (doc/JULIET.md:62-66), so the
class below mirrors the documented stages instead: pileup -> call (-> all-gather) -> phase, with the
documented knobs (`--min-perc`, `--max-perc`, `--drm-only`, phasing on/off) as arguments.
Fails loudly when the library or a gfx950 device is missing: there is no CPU fallback.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libjuliet_hip.so")

MAX_HAPLOTYPES = 702
HAP_INSUFFICIENT = 0xFFFE
HAP_DAMAGED = 0xFFFF
RESCUE_UNINFORMATIVE, RESCUE_NONE, RESCUE_AMBIGUOUS = 0xFFFB, 0xFFFC, 0xFFFD   # jl_phase_rescue_async (docs/SPEC.md §14)
RECOMB_WHOLE = 0xFFFA   # jl_phase_recombinants_async (docs/SPEC.md §23): some haplotype agrees with the whole read
NEAREST_MAX_DISTANCE = 7   # jl_phase_nearest_async (docs/SPEC.md §22): the largest mismatch budget
LINK_MAX = 1024   # jl_variant_linkage_async (docs/SPEC.md §15): positions, and variants, of one call
VARIANT_CAP = 4096
PACK_PATTERN_BYTES, PACK_HIT_BYTES = 8192, 16384   # jl_internal.h: what the pinned result block holds of hap_pattern / hit

GENE = np.dtype([("begin", "<u4"), ("end", "<u4")])
VARIANT = np.dtype([("gene", "<u4"), ("codon_pos", "<u4"), ("col", "<u4"), ("ref_codon", "u1"), ("codon", "u1"),
                    ("flags", "<u2"), ("count", "<u4"), ("coverage", "<u4"), ("expected", "<u4"), ("pad_", "<u4"),
                    ("p_value", "<f8"), ("log_p", "<f8")])
SUMMARY_FIELDS = ("reported_reads", "insufficient_reads", "damaged_reads", "marginal_gap", "marginal_heteroduplex",
                  "marginal_partial", "n_positions", "n_haplotypes")
SUMMARY = np.dtype([(n, "<u4") for n in SUMMARY_FIELDS])
SITE = np.dtype([("col", "<u4"), ("kind", "u1"), ("fill", "u1"), ("pad_", "<u2")])   # jl_site
SITE_CODON, SITE_DELETION = 0, 1
SITE_NO_FILL, SITE_PRESENT, SITE_DELETED, SITES_MAX = 0xFF, 0, 1, 4096
INSERTION_ALLELE = np.dtype([("col", "<u4"), ("len", "<u4"), ("seq", "<u8"), ("count", "<u4"), ("pad_", "<u4")])   # jl_insertion_allele
INSERTION_EVENT = np.dtype([("read", "<u4"), ("col", "<u4"), ("len", "<u4"), ("kind", "<u4"), ("seq", "<u8")])       # jl_insertion_event
SITE_INSERTION = 2
DELETION_ALLELE = np.dtype([("col", "<u4"), ("len", "<u4"), ("count", "<u4"), ("flank", "<u4")])   # jl_deletion_allele
SITE_INS_NONE, SITE_INS_OTHER, SITE_INS_MAX_ALLELES = 0, 63, 62

# every symbol include/juliet_hip.h declares (checked by tests/test_capi_exports.py)
EXPORTS = ("jl_abi_version", "jl_strerror", "jl_device_count", "jl_ctx_create", "jl_ctx_destroy", "jl_last_error",
           "jl_sync", "jl_col_stride", "jl_plane_stride", "jl_msa_upload", "jl_msa_alloc", "jl_msa_adopt", "jl_msa_pack_rows",
           "jl_msa_ingest_records", "jl_records_begin", "jl_records_append", "jl_records_finish", "jl_records_window", "jl_records_window_async", "jl_records_drop", "jl_records_append_masked", "jl_msa_ingest_records_masked", "jl_qmask_bytes", "jl_qmask_from_quals", "jl_msa_track_insertions", "jl_insertions_fetch", "jl_msa_take", "jl_msa_take_async", "jl_sample_reads", "jl_mix_counts", "jl_msa_download", "jl_msa_download_planes", "jl_synth_fill", "jl_synth_fill_window", "jl_pileup_async", "jl_n_positions", "jl_pileup_fetch",
           "jl_consensus_fetch", "jl_class_pileup_async", "jl_class_pileup_fetch", "jl_class_codons_async", "jl_class_codons_fetch", "jl_consensus_of_counts", "jl_phase_rescue_async", "jl_phase_rescue_fetch", "jl_phase_nearest_async", "jl_phase_nearest_fetch", "jl_phase_recombinants_async", "jl_phase_recombinants_fetch", "jl_haplotype_recombinants", "jl_variant_linkage_async", "jl_variant_linkage_fetch", "jl_linkage_stats", "jl_codon_deletions_async", "jl_codon_deletions_fetch", "jl_deletion_test", "jl_deletion_alleles_async", "jl_deletion_alleles_fetch", "jl_deletion_allele_test", "jl_read_stats_async", "jl_read_stats_fetch", "jl_read_filter", "jl_read_hypermut_async", "jl_read_hypermut_fetch", "jl_hypermut_eval", "jl_hypermut_test", "jl_hypermut_filter", "jl_read_orf_async", "jl_read_orf_fetch", "jl_orf_classify", "jl_orf_filter", "jl_sites_assemble", "jl_msa_track_insertion_alleles", "jl_insertion_alleles_fetch", "jl_insertion_test", "jl_msa_track_insertion_reads", "jl_insertion_reads_fetch", "jl_sites_assemble_alleles", "jl_call_async", "jl_call_fetch", "jl_variant_table_device", "jl_control_call_async", "jl_control_call_fetch", "jl_control_test", "jl_phase_async", "jl_phase_fetch",
           "jl_ctx_stream", "jl_run_async", "jl_run_wait", "jl_run_done", "jl_run_view_get", "jl_group_create", "jl_group_destroy",
           "jl_group_last_error", "jl_group_run_async", "jl_group_run_masked_async", "jl_group_views", "jl_group_time_pileup", "jl_msa_index_info", "jl_fisher_eval", "jl_fisher_eval_tail", "jl_control_eval", "jl_expand_read_hap", "jl_time_run", "jl_time_pileup", "jl_time_pileup_set", "jl_run_pileup_clock", "jl_run_pileup_ms", "jl_pileup_kernel_name", "jl_comm_unique_id", "jl_comm_create", "jl_comm_create_inproc", "jl_comm_destroy", "jl_comm_info",
           "jl_allgather_variants", "jl_allgather_variants_async", "jl_allgather_variants_async_many", "jl_allgather_variants_many", "jl_group_exchange_bind", "jl_group_exchange_collect", "jl_xwin_plan", "jl_xwin_assemble_local",
           "jl_xwin_assemble_rccl", "jl_xwin_assemble_slice_local", "jl_xwin_assemble_slice_rccl", "jl_phase_groups_async",
           "jl_phase_groups_fetch", "jl_phase_regroup", "jl_merge_tables", "jl_merge_groups", "jl_select_haplotypes",
           "jl_xwin_slice_plan", "jl_xwin_create", "jl_xwin_destroy", "jl_xwin_last_error", "jl_xwin_phase_sharded",
           "jl_xwin_read_hap_fetch", "jl_xwin_stage_us", "jl_allgather_groups")


READ_BASES, READ_GAPS, READ_MASKED, READ_COMPARED, READ_MISMATCHES, READ_STATS = range(6)   # jl_read_stats_async (docs/SPEC.md §20)
READ_RULES = ("min_bases", "mismatches", "mismatch_perc", "gap_perc", "n_perc")   # the order of jl_read_filter's failed[5]
HM_TARGET_SITES, HM_TARGET_MUT, HM_CONTROL_SITES, HM_CONTROL_MUT, HM_COUNTERS = range(5)   # jl_read_hypermut_async (docs/SPEC.md §26)
ORF_COVERED, ORF_GAP_CELLS, ORF_CODONS_READ, ORF_STOPS, ORF_COUNTERS = range(5)            # jl_read_orf_async (docs/SPEC.md §27)
ORF_MAX_SPANS, ORF_NO_STOP = 64, 0xFFFFFFFF
ORF_PARTIAL, ORF_STOP, ORF_FRAMESHIFT, ORF_DELETION = 1, 2, 4, 8                            # the flags of jl_orf_classify
ORF_SPAN = np.dtype([("col", np.uint32), ("n_codons", np.uint32)])                          # jl_orf_span


class OrfRule(C.Structure):   # jl_orf_rule
    _fields_ = [("max_gap_cells", C.c_uint32), ("tail_codons", C.c_uint32)]


class ReadRule(C.Structure):   # jl_read_rule
    _fields_ = [("min_bases", C.c_uint32), ("max_mismatches", C.c_uint32), ("max_mismatch_perc", C.c_double),
                ("max_gap_perc", C.c_double), ("max_masked_perc", C.c_double)]


class ErrorModel(C.Structure):
    _fields_ = [("match", C.c_double), ("substitution", C.c_double), ("deletion", C.c_double)]


class Params(C.Structure):
    _fields_ = [("alpha", C.c_double), ("n_tests", C.c_double), ("err", ErrorModel), ("expected_round", C.c_int32),
                ("tail", C.c_int32), ("min_perc", C.c_double), ("max_perc", C.c_double)]


class SynthParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("sub_rate", C.c_double), ("del_rate", C.c_double), ("mask_rate", C.c_double),
                ("partial_rate", C.c_double), ("minor_permille", C.c_uint32 * 4), ("reserved", C.c_uint32)]


class PhaseSummary(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in SUMMARY_FIELDS]


class TakePart(C.Structure):
    """jl_take_part: `n` reads `idx` of the resident matrix of `src` (include/juliet_hip.h)."""
    _fields_ = [("src", C.c_void_p), ("idx", C.c_void_p), ("n", C.c_uint64)]


TAKE_MAX_PARTS = 16


class XwinOp(C.Structure):
    """jl_xwin_op: one step of a rank's column-slice exchange (include/juliet_hip.h)."""
    _fields_ = [("op", C.c_int32), ("peer", C.c_int32), ("k_begin", C.c_uint32), ("k_count", C.c_uint32),
                ("read_begin", C.c_uint64), ("n_reads", C.c_uint64), ("dst_stride", C.c_uint64), ("bytes", C.c_uint64),
                ("dst_offset", C.c_uint64)]


XWIN_OP_LOCAL, XWIN_OP_SEND, XWIN_OP_RECV = 0, 1, 2


class XwinResult(C.Structure):
    """jl_xwin_result: what jl_xwin_phase_sharded returns (pointers into the session)."""
    _fields_ = [("n_variants", C.c_uint32), ("n_positions", C.c_uint32), ("n_haplotypes", C.c_uint32), ("n_groups", C.c_uint32),
                ("summary", PhaseSummary), ("merged", C.c_void_p), ("pos_global", C.c_void_p), ("hap_count", C.c_void_p),
                ("hap_pattern", C.c_void_p), ("hit", C.c_void_p), ("cooc", C.c_void_p), ("slice_begin", C.c_uint64),
                ("slice_reads", C.c_uint64), ("read_hap_bits", C.c_uint32), ("reserved", C.c_uint32)]


class RunView(C.Structure):
    """jl_run_view: pointers into the context's pinned result block (include/juliet_hip.h)."""
    _fields_ = [("complete", C.c_uint32), ("n_variants", C.c_uint32), ("phased", C.c_uint32),
                ("n_positions", C.c_uint32), ("n_haplotypes", C.c_uint32), ("n_var_phase", C.c_uint32),
                ("n_reads", C.c_uint64), ("summary", PhaseSummary), ("variants", C.c_void_p),
                ("pos_cols", C.c_void_p), ("hap_count", C.c_void_p), ("hap_pattern", C.c_void_p),
                ("hit", C.c_void_p), ("cooc", C.c_void_p), ("read_hap", C.c_void_p), ("read_hap_packed", C.c_void_p),
                ("read_hap_bits", C.c_uint32), ("reserved", C.c_uint32)]


def _view(addr, dtype, count):
    """numpy array over `count` items of host memory at `addr` (no copy; the owner must outlive the array)."""
    buf = (C.c_char * (int(count) * np.dtype(dtype).itemsize)).from_address(addr)
    return np.frombuffer(buf, dtype=dtype, count=int(count))


ERROR_MODELS = {  # docs/SPEC.md §5 (values UNPINNED)
    "sequel": (0.998826, 5.8e-5, 1.0e-3),
    "permissive": (0.99764, 1.2e-4, 2.0e-3),
}


def default_params(n_tests=0.0, alpha=0.01, chemistry="sequel", min_perc=-1.0, max_perc=-1.0, expected_round=0, tail=0):
    m, s, d = ERROR_MODELS[chemistry]
    return Params(alpha, n_tests, ErrorModel(m, s, d), expected_round, tail, min_perc, max_perc)


def expand_ids(packed, bits, n_reads):
    """Per-read haplotype ids as the kernels store them (4 / 8 / 16 bits per read, include/juliet_hip.h jl_run_view) ->
    uint16 ids (HAP_INSUFFICIENT / HAP_DAMAGED for the two unreported categories)."""
    if bits == 16:
        return packed.view(np.uint16)[:n_reads]
    p = packed.view(np.uint8)
    if bits == 4:
        b = p[: (n_reads + 1) // 2]
        c = np.empty(2 * len(b), dtype=np.uint16)
        c[0::2] = b & 15
        c[1::2] = b >> 4
        c = c[:n_reads]
        out = c.copy()
        out[c == 14] = HAP_INSUFFICIENT
        out[c == 15] = HAP_DAMAGED
        return out
    if bits == 8:
        c = p[:n_reads].astype(np.uint16)
        out = c.copy()
        out[c == 254] = HAP_INSUFFICIENT
        out[c == 255] = HAP_DAMAGED
        return out
    raise ValueError(f"per-read ids of width {bits}")


class IndexInfo(C.Structure):
    """jl_index_info (include/juliet_hip.h): the deviation index of a context's resident matrix."""
    _fields_ = [("state", C.c_uint32), ("runs", C.c_uint32), ("builds", C.c_uint32), ("last_form", C.c_uint32),
                ("plain_chunks", C.c_uint32), ("indexed_chunks", C.c_uint32),
                ("generation", C.c_uint64), ("entries", C.c_uint64), ("bytes", C.c_uint64)]


INDEX_NONE, INDEX_PENDING, INDEX_BUILT, INDEX_REFUSED = 0, 1, 2, 3


class JulietError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"libjuliet_hip: status {status}: {msg}")
        self.status = status


_lib = None


def load_library(path=LIB_PATH):
    """Load the C-ABI library; raises if it was not built (run `python -c 'import __graft_entry__ as g; g.build()'`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: build it with minorseq_amd/csrc/Makefile (hipcc, gfx950). "
                          "There is no CPU fallback for the juliet hot path.")
    lib = C.CDLL(path)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib.jl_strerror.restype = C.c_char_p
    lib.jl_last_error.restype = C.c_char_p
    lib.jl_last_error.argtypes = [vp]
    lib.jl_pileup_kernel_name.restype = C.c_char_p
    lib.jl_col_stride.restype = u64
    lib.jl_col_stride.argtypes = [u64]
    lib.jl_plane_stride.restype = u64
    lib.jl_plane_stride.argtypes = [u64]
    lib.jl_ctx_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
    lib.jl_ctx_stream.argtypes = [vp]
    lib.jl_ctx_stream.restype = vp
    lib.jl_ctx_destroy.argtypes = [vp]
    lib.jl_ctx_destroy.restype = None
    lib.jl_sync.argtypes = [vp]
    lib.jl_msa_upload.argtypes = [vp, vp, u64, u32, u64, u32]
    lib.jl_msa_alloc.argtypes = [vp, u64, u32, u32]
    lib.jl_msa_adopt.argtypes = [vp, vp, u64, u32, u64, u32]
    if hasattr(lib, "jl_msa_index_info"):   # (JL_LIB may name an older build of the library: A/B runs in one checkout)
        lib.jl_msa_index_info.argtypes = [vp, C.POINTER(IndexInfo), C.c_int, vp, u32]
    lib.jl_msa_pack_rows.argtypes = [vp, vp, u64, u32, u32]
    lib.jl_msa_ingest_records.argtypes = [vp, u64, u32, u32] + [vp] * 7 + [u32]
    lib.jl_records_begin.argtypes = [vp, u64, u64, u64, u64]
    lib.jl_records_append.argtypes = [vp, u64] + [vp] * 7
    lib.jl_records_finish.argtypes = [vp, u32, u32, u32]
    lib.jl_records_window.argtypes = [vp, vp, u32, u32, u32]
    lib.jl_records_window_async.argtypes = [vp, vp, u32, u32, u32]
    lib.jl_records_drop.argtypes = [vp]
    lib.jl_records_append_masked.argtypes = [vp, u64] + [vp] * 6
    lib.jl_msa_ingest_records_masked.argtypes = [vp, u64, u32, u32] + [vp] * 6 + [u32]
    lib.jl_qmask_bytes.restype = u64
    lib.jl_qmask_bytes.argtypes = [u64]
    lib.jl_qmask_from_quals.argtypes = [u64, vp, vp, vp, u32, vp, u64]
    lib.jl_msa_track_insertions.argtypes = [vp, C.c_int]
    lib.jl_insertions_fetch.argtypes = [vp, vp, vp]
    lib.jl_msa_download.argtypes = [vp, vp, u64]
    lib.jl_msa_download_planes.argtypes = [vp, vp, u64]
    lib.jl_msa_take.argtypes = [vp, vp, u32]
    lib.jl_msa_take_async.argtypes = [vp, vp, u32]
    lib.jl_sample_reads.argtypes = [u64, u64, u64, vp, C.POINTER(u64)]
    lib.jl_mix_counts.argtypes = [u32, u64, C.c_double, vp]
    lib.jl_synth_fill.argtypes = [vp, C.POINTER(SynthParams), vp]
    lib.jl_synth_fill_window.argtypes = [vp, C.POINTER(SynthParams), vp, u32]
    lib.jl_pileup_async.argtypes = [vp, vp, u32, vp, u32]
    lib.jl_n_positions.argtypes = [vp]
    lib.jl_n_positions.restype = u32
    lib.jl_pileup_fetch.argtypes = [vp] * 7
    lib.jl_consensus_fetch.argtypes = [vp, vp]
    lib.jl_class_pileup_async.argtypes = [vp, vp, u32]
    lib.jl_class_pileup_fetch.argtypes = [vp, vp, vp]
    lib.jl_class_codons_async.argtypes = [vp, vp, u32, vp, u32]
    lib.jl_class_codons_fetch.argtypes = [vp, vp, vp]
    lib.jl_phase_rescue_async.argtypes = [vp, vp, u32, vp, u32, u32, u32]
    lib.jl_phase_rescue_fetch.argtypes = [vp, vp, vp, vp]
    lib.jl_phase_nearest_async.argtypes = [vp, vp, u32, vp, u32, u32, u32, u32]
    lib.jl_phase_nearest_fetch.argtypes = [vp, vp, vp, vp, vp]
    lib.jl_phase_recombinants_async.argtypes = [vp, vp, u32, vp, u32, u32, u32]
    lib.jl_phase_recombinants_fetch.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    lib.jl_haplotype_recombinants.argtypes = [vp, u32, u32, u32, vp, C.c_double, vp]
    lib.jl_consensus_of_counts.argtypes = [vp, u32, vp]
    lib.jl_variant_linkage_async.argtypes = [vp, vp, u32, vp, vp, u32]
    lib.jl_variant_linkage_fetch.argtypes = [vp, vp, vp, vp]
    lib.jl_linkage_stats.argtypes = [vp, vp, vp, vp, u32, u32, u32, u32, vp]
    lib.jl_codon_deletions_async.argtypes = [vp]
    lib.jl_codon_deletions_fetch.argtypes = [vp, vp]
    lib.jl_deletion_test.argtypes = [vp, vp, C.c_double, vp]
    lib.jl_deletion_alleles_async.argtypes = [vp]
    lib.jl_deletion_alleles_fetch.argtypes = [vp, vp, vp, vp, C.c_uint32, vp]
    lib.jl_deletion_allele_test.argtypes = [C.c_uint32, C.c_uint32, vp, C.c_double, C.c_double, vp]
    lib.jl_read_stats_async.argtypes = [vp, vp]
    lib.jl_read_stats_fetch.argtypes = [vp, vp]
    lib.jl_read_filter.argtypes = [vp, u64, C.POINTER(ReadRule), vp, C.POINTER(u64), vp]
    lib.jl_read_hypermut_async.argtypes = [vp, vp]
    lib.jl_read_hypermut_fetch.argtypes = [vp, vp, vp, vp]
    lib.jl_hypermut_eval.argtypes = [vp, vp, u64, vp, vp]
    lib.jl_hypermut_test.argtypes = [u32, u32, u32, u32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.jl_hypermut_filter.argtypes = [vp, u64, C.c_double, vp, C.POINTER(u64), C.POINTER(u64)]
    lib.jl_read_orf_async.argtypes = [vp, vp, u32, vp]
    lib.jl_read_orf_fetch.argtypes = [vp, vp, vp]
    lib.jl_orf_classify.argtypes = [vp, vp, vp, u32, u64, C.POINTER(OrfRule), vp]
    lib.jl_orf_filter.argtypes = [vp, u32, u64, u32, vp, C.POINTER(u64), C.POINTER(u64)]
    lib.jl_sites_assemble.argtypes = [vp, vp, vp, u32]
    lib.jl_msa_track_insertion_alleles.argtypes = [vp, C.c_int]
    lib.jl_insertion_alleles_fetch.argtypes = [vp, vp, vp, u32, vp]
    lib.jl_msa_track_insertion_reads.argtypes = [vp, C.c_int]
    lib.jl_insertion_reads_fetch.argtypes = [vp, vp, u32, vp]
    lib.jl_sites_assemble_alleles.argtypes = [vp, vp, vp, u32, vp, u32]
    lib.jl_insertion_test.argtypes = [u32, vp, vp, C.c_double, C.c_double, vp]
    lib.jl_call_async.argtypes = [vp, C.POINTER(Params), vp]
    lib.jl_call_fetch.argtypes = [vp, vp, u32, C.POINTER(u32)]
    lib.jl_variant_table_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(u32)]
    lib.jl_control_call_async.argtypes = [vp, vp, C.POINTER(Params), vp]
    lib.jl_control_call_fetch.argtypes = [vp, vp, vp, u32, C.POINTER(u32)]
    lib.jl_control_test.argtypes = [u32, u32, u32, u32, C.POINTER(Params), C.c_double, vp]
    lib.jl_phase_async.argtypes = [vp, vp, u32, u32]
    lib.jl_phase_fetch.argtypes = [vp] * 8 + [u32]
    lib.jl_run_async.argtypes = [vp, vp, u32, vp, u32, C.POINTER(Params), vp, C.c_int, u32, C.c_int]
    lib.jl_time_run.argtypes = [vp, vp, u32, vp, u32, C.POINTER(Params), vp, C.c_int, u32, C.c_int, u32, C.POINTER(C.c_float)]
    lib.jl_group_create.argtypes = [vp, u32, C.POINTER(vp)]
    lib.jl_group_destroy.argtypes = [vp]
    lib.jl_group_destroy.restype = None
    lib.jl_group_last_error.argtypes = [vp]
    lib.jl_group_last_error.restype = C.c_char_p
    lib.jl_group_run_async.argtypes = [vp, vp, u32, vp, u32, C.POINTER(Params), C.c_int, u32, C.c_int]
    lib.jl_group_run_masked_async.argtypes = [vp, vp, u32, vp, u32, C.POINTER(Params), vp, C.c_int, u32, C.c_int]
    lib.jl_group_views.argtypes = [vp, C.c_void_p, u32, C.POINTER(u32)]
    lib.jl_group_time_pileup.argtypes = [vp, u32, u32, C.POINTER(C.c_float), C.POINTER(u64)]
    lib.jl_run_wait.argtypes = [vp]
    lib.jl_run_done.argtypes = [vp]
    lib.jl_run_view_get.argtypes = [vp, C.POINTER(RunView)]
    lib.jl_fisher_eval.argtypes = [vp, vp, vp, vp, u32, vp, vp]
    lib.jl_fisher_eval_tail.argtypes = [vp, vp, vp, vp, u32, C.c_int, vp, vp]
    lib.jl_control_eval.argtypes = [vp, vp, vp, vp, vp, u32, C.c_double, C.c_double, vp, vp, vp]
    lib.jl_expand_read_hap.argtypes = [vp, u32, u64, vp]
    lib.jl_time_pileup.argtypes = [vp, u32, C.POINTER(C.c_float)]
    lib.jl_time_pileup_set.argtypes = [vp, u32, u32, C.POINTER(C.c_float)]
    lib.jl_run_pileup_clock.argtypes = [vp, C.c_int]
    lib.jl_run_pileup_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(u64)]
    lib.jl_comm_unique_id.argtypes = [vp]
    lib.jl_comm_create.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(vp)]
    lib.jl_comm_create_inproc.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(vp)]
    lib.jl_comm_destroy.argtypes = [vp]
    lib.jl_comm_destroy.restype = None
    lib.jl_comm_info.argtypes = [vp] + [C.POINTER(C.c_int)] * 4
    lib.jl_allgather_variants.argtypes = [vp, vp, vp, vp, u32]
    lib.jl_allgather_variants_async.argtypes = [vp, vp]
    lib.jl_allgather_variants_async_many.argtypes = [vp, u32, vp]
    lib.jl_allgather_variants_many.argtypes = [vp, u32, vp, vp, vp, u32]
    lib.jl_group_exchange_bind.argtypes = [vp, vp]
    lib.jl_group_exchange_collect.argtypes = [vp, vp, vp, u32]
    lib.jl_xwin_plan.argtypes = [vp, vp, u32, vp, u32, vp, vp, vp, C.POINTER(u32)]
    lib.jl_xwin_assemble_local.argtypes = [vp, vp, u32, vp, u32, vp, vp, C.POINTER(u32)]
    lib.jl_xwin_assemble_rccl.argtypes = [vp, vp, vp, vp, vp, vp, u32, vp, vp, C.POINTER(u32)]
    lib.jl_xwin_assemble_slice_local.argtypes = [vp, vp, u32, vp, u32, u64, u64, vp, vp, C.POINTER(u32)]
    lib.jl_xwin_assemble_slice_rccl.argtypes = [vp, vp, vp, vp, vp, vp, u32, vp, vp, vp, C.POINTER(u32)]
    lib.jl_phase_groups_async.argtypes = [vp, vp, u32]
    lib.jl_phase_groups_fetch.argtypes = [vp, vp, u32, vp, u32, C.POINTER(u32), C.POINTER(u32), vp, u32, vp]
    lib.jl_phase_regroup.argtypes = [vp, vp, u32, u32, vp]
    lib.jl_merge_tables.argtypes = [vp, vp, vp, u32, vp, u32, C.POINTER(u32)]
    lib.jl_merge_groups.argtypes = [vp, vp, vp, vp, u32, u32, vp, vp, u32, C.POINTER(u32), vp]
    lib.jl_select_haplotypes.argtypes = [vp, vp, u32, u32, vp, u32, vp, u32, vp, u32, vp, vp, vp, vp, u32, vp, vp]
    lib.jl_xwin_slice_plan.argtypes = [vp, vp, vp, u32, vp, u32, vp, C.c_int32, C.c_int32, vp, u32, C.POINTER(u32)]
    lib.jl_xwin_create.argtypes = [vp, u32, vp, vp, vp, vp, u32, vp, C.POINTER(vp)]
    lib.jl_xwin_destroy.argtypes = [vp]
    lib.jl_xwin_destroy.restype = None
    lib.jl_xwin_last_error.argtypes = [vp]
    lib.jl_xwin_last_error.restype = C.c_char_p
    lib.jl_xwin_phase_sharded.argtypes = [vp, u32, C.POINTER(XwinResult)]
    lib.jl_xwin_read_hap_fetch.argtypes = [vp, vp]
    lib.jl_xwin_stage_us.argtypes = [vp, vp]
    lib.jl_allgather_groups.argtypes = [vp, vp, u32, u32, vp, vp, vp, vp, C.POINTER(u32)]
    if lib.jl_abi_version() != 5:
        raise ImportError("libjuliet_hip.so ABI version mismatch")
    _lib = lib
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _record_arrays(pos, cigar, cig_off, seq4, seq_off, qual, qual_off, qmask):
    """The arrays of aligned records as the library takes them (qual, qual_off: None without qualities); qualities or a mask, not both."""
    if qmask is not None and qual is not None:
        raise ValueError("records carry qualities or a mask, not both")
    if qual is not None:
        qual, qual_off = np.ascontiguousarray(qual, dtype=np.uint8), np.ascontiguousarray(qual_off, dtype=np.uint64)
    return (np.ascontiguousarray(pos, dtype=np.int32), np.ascontiguousarray(cigar, dtype=np.uint32), np.ascontiguousarray(cig_off, dtype=np.uint64),
            np.ascontiguousarray(seq4, dtype=np.uint8), np.ascontiguousarray(seq_off, dtype=np.uint64), qual, qual_off)


class _LazyIds:
    """The per-read ids of a run view: packed bytes in pinned memory + their width; expands to uint16 on first use
    (a step loop that only reads the small results never touches them)."""

    def __init__(self, packed, bits, n_reads):
        self.packed, self.bits, self.n_reads = packed, int(bits), int(n_reads)
        self._ids = None

    def ids(self):
        if self._ids is None:
            self._ids = expand_ids(self.packed, self.bits, self.n_reads)
        return self._ids

    def __array__(self, dtype=None, copy=None):
        a = self.ids()
        return a if dtype is None else a.astype(dtype)

    def __eq__(self, other):
        return self.ids() == other

    def __getitem__(self, k):
        return self.ids()[k]

    def __len__(self):
        return self.n_reads

    def copy(self):
        return self.ids().copy()


class Juliet:
    """One context = one GPU = one reference window of aligned CCS reads resident in HBM."""

    def __init__(self, device=0, stream=None):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.jl_ctx_create(device, C.c_void_p(stream) if stream else None, C.byref(h))
        if rc != 0:
            raise JulietError(rc, self.lib.jl_last_error(None).decode())
        self.h = h
        self.n_reads = 0
        self.n_cols = 0
        self.col_stride = 0
        self._keep = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.jl_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, allow=()):
        if rc != 0 and rc not in allow:
            raise JulietError(rc, self.lib.jl_last_error(self.h).decode())
        return rc

    # ------------------------------------------------------------------ residency
    def _shape(self, n_reads, n_cols, stride=None):
        """col_stride: the column stride of the INTERCHANGE format (what download_columns returns); the resident planes have
        plane_stride bytes per plane (the library's, or the caller's for an adopted matrix)."""
        self.n_reads, self.n_cols = int(n_reads), int(n_cols)
        self.col_stride = int(self.lib.jl_col_stride(int(n_reads)))
        self.plane_stride = int(stride) if stride is not None else int(self.lib.jl_plane_stride(int(n_reads)))

    def upload_columns(self, packed, n_reads, win_begin=0):
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        n_cols, stride = packed.shape
        self._chk(self.lib.jl_msa_upload(self.h, _p(packed), n_reads, n_cols, stride, win_begin))
        self._shape(n_reads, n_cols)

    def upload_rows(self, rows, win_begin=0):
        """By-row uint8 codes; transposed into the resident planes on the device."""
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        n, l = rows.shape
        self._chk(self.lib.jl_msa_pack_rows(self.h, _p(rows), n, l, win_begin))
        self._shape(n, l)

    def ingest_records(self, n_cols, win_begin, pos, cigar, cig_off, seq4, seq_off, qual=None, qual_off=None, min_qv=0, qmask=None):
        """Aligned records (BAM-decoded arrays) -> resident matrix, cigar expansion on the device.  `qmask`: the filter as one
        bit per base (jl_msa_ingest_records_masked, layout in include/juliet_hip.h) instead of qualities."""
        pos, cigar, cig_off, seq4, seq_off, qual, qual_off = _record_arrays(pos, cigar, cig_off, seq4, seq_off, qual, qual_off, qmask)
        n = len(pos)
        if qmask is not None:
            qmask = np.ascontiguousarray(qmask, dtype=np.uint8)
            self._chk(self.lib.jl_msa_ingest_records_masked(self.h, n, n_cols, win_begin, _p(pos), _p(cigar), _p(cig_off), _p(seq4),
                                                            _p(seq_off), _p(qmask), min_qv))
            self._shape(n, n_cols)
            return
        self._chk(self.lib.jl_msa_ingest_records(self.h, n, n_cols, win_begin, _p(pos), _p(cigar), _p(cig_off), _p(seq4),
                                                 _p(seq_off), _p(qual), _p(qual_off), min_qv))
        self._shape(n, n_cols)

    def ingest_records_chunked(self, n_cols, win_begin, pos, cigar, cig_off, seq4, seq_off, qual=None, qual_off=None,
                               min_qv=0, chunk_reads=1000, hints=(0, 0, 0, 0), qmask=None):
        """The same through jl_records_begin / _append / _finish, `chunk_reads` records per append; every chunk passes
        slices of the caller's arrays with offsets that do not start at 0 (the library rebases them).  `qmask` (for the whole
        arrays, relative to seq_off[0]): every chunk's mask is cut out of it, re-based to the chunk's first base."""
        pos, cigar, cig_off, seq4, seq_off, qual, qual_off = _record_arrays(pos, cigar, cig_off, seq4, seq_off, qual, qual_off, qmask)
        n = len(pos)
        hq = hints[3] if qual is not None else 0
        self._chk(self.lib.jl_records_begin(self.h, hints[0], hints[1], hints[2], hq))
        for a in range(0, n, chunk_reads):
            b = min(n, a + chunk_reads)
            co, so = np.ascontiguousarray(cig_off[a:b + 1]), np.ascontiguousarray(seq_off[a:b + 1])
            qo = np.ascontiguousarray(qual_off[a:b + 1]) if qual is not None else None
            if qmask is not None:
                qm = qmask_slice(qmask, int(so[0]) - int(seq_off[0]), int(so[-1]) - int(so[0]))
                self._chk(self.lib.jl_records_append_masked(self.h, b - a, _p(np.ascontiguousarray(pos[a:b])), _p(cigar), _p(co),
                                                            _p(seq4), _p(so), _p(qm)))
                continue
            self._chk(self.lib.jl_records_append(self.h, b - a, _p(np.ascontiguousarray(pos[a:b])), _p(cigar), _p(co), _p(seq4),
                                                 _p(so), _p(qual), _p(qo)))
        self._chk(self.lib.jl_records_finish(self.h, n_cols, win_begin, min_qv))
        self._shape(n, n_cols)

    def records_upload(self, pos, cigar, cig_off, seq4, seq_off, qual=None, qual_off=None, qmask=None):
        """jl_records_begin + one jl_records_append: the records stay resident on this context (for records_window /
        records_window_async on other contexts of the device) until records_drop.  `qmask`: jl_records_append_masked."""
        pos, cigar, cig_off, seq4, seq_off, qual, qual_off = _record_arrays(pos, cigar, cig_off, seq4, seq_off, qual, qual_off, qmask)
        n = len(pos)
        self._chk(self.lib.jl_records_begin(self.h, n, len(cigar), len(seq4), len(qual) if qual is not None else 0))
        if qmask is not None:
            qmask = np.ascontiguousarray(qmask, dtype=np.uint8)
            self._chk(self.lib.jl_records_append_masked(self.h, n, _p(pos), _p(cigar), _p(cig_off), _p(seq4), _p(seq_off), _p(qmask)))
        else:
            self._chk(self.lib.jl_records_append(self.h, n, _p(pos), _p(cigar), _p(cig_off), _p(seq4), _p(seq_off), _p(qual), _p(qual_off)))
        self._n_records = n

    def records_window(self, records, n_cols, win_begin=0, min_qv=0, wait=True):
        """This context's resident matrix from the records uploaded to `records` (another context of the device);
        wait=False only enqueues the build on this context's stream (jl_records_window_async)."""
        fn = self.lib.jl_records_window if wait else self.lib.jl_records_window_async
        self._chk(fn(records.h, self.h, n_cols, win_begin, min_qv))
        self._shape(records._n_records, n_cols)

    def records_drop(self):
        self._chk(self.lib.jl_records_drop(self.h))

    def track_insertions(self, on=True):
        self._chk(self.lib.jl_msa_track_insertions(self.h, 1 if on else 0))

    def insertions_fetch(self):
        """(len_hist[n_cols][32], base_counts[n_cols][30][4]) of the last ingest_records with tracking on."""
        lh = np.zeros((self.n_cols, 32), dtype=np.uint32)
        bc = np.zeros((self.n_cols, 30, 4), dtype=np.uint32)
        self._chk(self.lib.jl_insertions_fetch(self.h, _p(lh), _p(bc)))
        return lh, bc

    def track_insertion_alleles(self, on=True):
        """jl_msa_track_insertion_alleles (docs/SPEC.md §17): the next record build into this context also forms the junction
        counters and the table of in-frame insertion alleles."""
        self._chk(self.lib.jl_msa_track_insertion_alleles(self.h, 1 if on else 0))

    def insertion_alleles(self):
        """(jcnt uint32[n_cols][4] = span, inframe, frameshift, unread per junction; rows INSERTION_ALLELE[n], ascending by
        (col, len, seq)) of the last record build with track_insertion_alleles on."""
        jcnt = np.zeros((self.n_cols, 4), dtype=np.uint32)
        n = C.c_uint32(0)
        self._chk(self.lib.jl_insertion_alleles_fetch(self.h, _p(jcnt), None, 0, C.byref(n)))
        rows = np.zeros(n.value, dtype=INSERTION_ALLELE)
        if n.value:
            self._chk(self.lib.jl_insertion_alleles_fetch(self.h, None, _p(rows), n.value, C.byref(n)))
        return jcnt, rows

    def track_insertion_reads(self, on=True):
        """jl_msa_track_insertion_reads (docs/SPEC.md §19): the next record build into this context forms what
        track_insertion_alleles gives and one event per (read, junction) with an insertion."""
        self._chk(self.lib.jl_msa_track_insertion_reads(self.h, 1 if on else 0))

    def insertion_reads(self):
        """INSERTION_EVENT[n], ascending by (read, col), of the last record build with track_insertion_reads on: kind 1 in frame
        (len, seq the allele's key), 2 frameshift, 3 unread (len, seq zero)."""
        n = C.c_uint32(0)
        self._chk(self.lib.jl_insertion_reads_fetch(self.h, None, 0, C.byref(n)))
        rows = np.zeros(n.value, dtype=INSERTION_EVENT)
        if n.value:
            self._chk(self.lib.jl_insertion_reads_fetch(self.h, _p(rows), n.value, C.byref(n)))
        return rows

    def alloc(self, n_reads, n_cols, win_begin=0):
        self._chk(self.lib.jl_msa_alloc(self.h, n_reads, n_cols, win_begin))
        self._shape(n_reads, n_cols)

    def adopt(self, device_ptr, n_reads, n_cols, plane_stride, win_begin=0, keep_alive=None):
        """Caller-owned device memory in the resident format: [n_cols][3][plane_stride] bytes (msa.pack_planes)."""
        self._chk(self.lib.jl_msa_adopt(self.h, C.c_void_p(device_ptr), n_reads, n_cols, plane_stride, win_begin))
        self._shape(n_reads, n_cols, plane_stride)
        self._keep = keep_alive

    def take(self, parts, wait=True):
        """jl_msa_take: this context's resident matrix from chosen reads of other contexts' — parts = [(source, idx), ...],
        destination reads = the parts one after the other, read j of a part = read idx[j] of its source (any order, repeats
        allowed).  wait=False only enqueues on this context's stream (jl_msa_take_async)."""
        keep = [np.ascontiguousarray(idx, dtype=np.uint32) for _, idx in parts]
        arr = (TakePart * max(1, len(parts)))()
        for k, ((src, _), idx) in enumerate(zip(parts, keep)):
            arr[k] = TakePart(src.h, idx.ctypes.data if len(idx) else None, len(idx))
        fn = self.lib.jl_msa_take if wait else self.lib.jl_msa_take_async
        self._chk(fn(self.h, arr, len(parts)))
        self._shape(sum(len(idx) for idx in keep), parts[0][0].n_cols)
        self._keep = None

    def synth_fill(self, sp, ref):
        """sp: minorseq_amd.synth.SynthParams; fills the resident matrix on the device."""
        csp = SynthParams(sp.seed, sp.sub_rate, sp.del_rate, sp.mask_rate, sp.partial_rate,
                          (C.c_uint32 * 4)(*sp.minor_permille), 0)
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        assert len(ref) == self.n_cols
        self._chk(self.lib.jl_synth_fill(self.h, C.byref(csp), _p(ref)))

    def synth_fill_window(self, sp, ref_full):
        """The window [win_begin, win_begin + n_cols) of the reads synth.rows(sp, len(ref_full), ...) describes."""
        csp = SynthParams(sp.seed, sp.sub_rate, sp.del_rate, sp.mask_rate, sp.partial_rate,
                          (C.c_uint32 * 4)(*sp.minor_permille), 0)
        ref_full = np.ascontiguousarray(ref_full, dtype=np.uint8)
        self._chk(self.lib.jl_synth_fill_window(self.h, C.byref(csp), _p(ref_full), len(ref_full)))

    def download_columns(self):
        out = np.empty((self.n_cols, self.col_stride), dtype=np.uint8)
        self._chk(self.lib.jl_msa_download(self.h, _p(out), out.nbytes))
        return out

    def download_planes(self):
        """The resident planes as the device holds them, uint8[n_cols][3][plane_stride] (msa.pack_planes), padding included."""
        out = np.empty((self.n_cols, 3, self.plane_stride), dtype=np.uint8)
        self._chk(self.lib.jl_msa_download_planes(self.h, _p(out), out.nbytes))
        return out

    # ------------------------------------------------------------------ stages
    def pileup_async(self, genes, refseq=None):
        genes = np.ascontiguousarray(genes, dtype=GENE)
        if refseq is not None:
            refseq = np.ascontiguousarray(refseq, dtype=np.uint8)
        self._chk(self.lib.jl_pileup_async(self.h, _p(genes), len(genes), _p(refseq),
                                           0 if refseq is None else len(refseq)))

    def index_info(self, wait=False, chunk_flags=False, max_chunks=None):
        """jl_msa_index_info: the deviation index as a dict (state, runs, builds, last_form, plain_chunks, indexed_chunks,
        generation, entries, bytes); wait: a build that is enqueued is waited for; chunk_flags: with `chunk_flags`, one byte per
        chunk of the pileup's chunk table (0 planes, 1 indexed, 2 a plain chunk over the density bound)."""
        info = IndexInfo()
        flags = np.zeros(max_chunks or self.n_cols, dtype=np.uint8) if chunk_flags else None
        self._chk(self.lib.jl_msa_index_info(self.h, C.byref(info), 1 if wait else 0, _p(flags), 0 if flags is None else len(flags)))
        out = {k: int(getattr(info, k)) for k, _ in IndexInfo._fields_}
        if flags is not None:
            out["chunk_flags"] = flags
        return out

    def pileup_fetch(self):
        p = self.lib.jl_n_positions(self.h)
        col = np.zeros((self.n_cols, 6), dtype=np.uint32)
        pg, pk, pc = (np.zeros(p, dtype=np.uint32) for _ in range(3))
        hist = np.zeros((p, 64), dtype=np.uint32)
        cov = np.zeros(p, dtype=np.uint32)
        self._chk(self.lib.jl_pileup_fetch(self.h, _p(col), _p(pg), _p(pk), _p(pc), _p(hist), _p(cov)))
        return dict(col_counts=col, pos_gene=pg, pos_codon=pk, pos_col=pc, hist=hist, coverage=cov)

    def consensus(self):
        """Majority symbol per column of the last pileup: 0..3 base, 4 majority deletion, 5 uncovered."""
        out = np.zeros(self.n_cols, dtype=np.uint8)
        self._chk(self.lib.jl_consensus_fetch(self.h, _p(out)))
        return out

    def class_pileup(self, labels, n_classes, wait=True):
        """jl_class_pileup_async (docs/SPEC.md §13): the column pileup of the resident matrix by class of reads — read i counts
        for class labels[i] when labels[i] < n_classes, for none otherwise (the ids of a phasing run can be passed as they are).
        Returns (counts[n_classes, n_cols, 6], class_reads[n_classes]); wait=False only enqueues on this context's stream and
        returns None (class_pileup_fetch brings the arrays)."""
        labels = np.ascontiguousarray(labels, dtype=np.uint16)
        assert len(labels) == self.n_reads
        self._chk(self.lib.jl_class_pileup_async(self.h, _p(labels), int(n_classes)))
        self._class_shape = (int(n_classes), self.n_cols)
        return self.class_pileup_fetch() if wait else None

    def class_pileup_fetch(self):
        k, l = getattr(self, "_class_shape", (0, 0))
        counts = np.zeros((k, l, 6), dtype=np.uint32)
        reads = np.zeros(k, dtype=np.uint32)
        self._chk(self.lib.jl_class_pileup_fetch(self.h, _p(counts), _p(reads)))
        return counts, reads

    def class_codons(self, labels, n_classes, cols, wait=True):
        """jl_class_codons_async (docs/SPEC.md §24): the codon histograms of the resident matrix by class of reads at the codon
        starts cols[n_pos] (window columns, strictly ascending) — the labels are class_pileup's.  Returns
        (hist[n_classes, n_pos, 64], class_reads[n_classes]); wait=False only enqueues on this context's stream and returns
        None (class_codons_fetch brings the arrays)."""
        labels = np.ascontiguousarray(labels, dtype=np.uint16)
        cols = np.ascontiguousarray(cols, dtype=np.uint32)
        assert len(labels) == self.n_reads and cols.ndim == 1
        self._chk(self.lib.jl_class_codons_async(self.h, _p(labels), int(n_classes), _p(cols), len(cols)))
        self._class_codons_shape = (int(n_classes), len(cols))
        return self.class_codons_fetch() if wait else None

    def class_codons_fetch(self):
        k, p = getattr(self, "_class_codons_shape", (0, 0))
        hist = np.zeros((k, p, 64), dtype=np.uint32)
        reads = np.zeros(k, dtype=np.uint32)
        self._chk(self.lib.jl_class_codons_fetch(self.h, _p(hist), _p(reads)))
        return hist, reads

    def phase_rescue(self, pos_cols, hap_pattern, min_positions=1, wait=True):
        """jl_phase_rescue_async (docs/SPEC.md §14): which haplotype of hap_pattern[H, Vp] (codon indices at the codon starts
        pos_cols[Vp]) every read of the resident matrix agrees with at the positions where it can be read.  Returns
        dict(rescue[n_reads] uint16: h, RESCUE_UNINFORMATIVE, RESCUE_NONE or RESCUE_AMBIGUOUS; hap_reads[H]; tally[4] =
        assigned, ambiguous, none, uninformative); wait=False only enqueues on this context's stream and returns None
        (phase_rescue_fetch brings the arrays)."""
        pos_cols = np.ascontiguousarray(pos_cols, dtype=np.uint32)
        hap_pattern = np.ascontiguousarray(hap_pattern, dtype=np.uint8)
        assert hap_pattern.ndim == 2 and hap_pattern.shape[1] == len(pos_cols)
        self._chk(self.lib.jl_phase_rescue_async(self.h, _p(pos_cols), len(pos_cols), _p(hap_pattern), hap_pattern.shape[1],
                                                 hap_pattern.shape[0], int(min_positions)))
        self._rescue_shape = (self.n_reads, hap_pattern.shape[0])
        return self.phase_rescue_fetch() if wait else None

    def phase_rescue_fetch(self):
        n, h = getattr(self, "_rescue_shape", (0, 0))
        rescue = np.zeros(n, dtype=np.uint16)
        hap_reads = np.zeros(h, dtype=np.uint32)
        tally = np.zeros(4, dtype=np.uint64)
        self._chk(self.lib.jl_phase_rescue_fetch(self.h, _p(rescue), _p(hap_reads), _p(tally)))
        return dict(rescue=rescue, hap_reads=hap_reads, tally=tally)

    def phase_nearest(self, pos_cols, hap_pattern, min_positions=1, max_distance=1, wait=True):
        """jl_phase_nearest_async (docs/SPEC.md §22): which haplotype of hap_pattern[H, Vp] every read of the resident matrix is
        nearest to, counting the informative positions at which its codon differs, when that haplotype is the only one at the
        smallest distance and the distance is at most max_distance (0 .. NEAREST_MAX_DISTANCE).  Returns dict(nearest[n_reads]
        uint16: h, RESCUE_UNINFORMATIVE, RESCUE_NONE or RESCUE_AMBIGUOUS; dist[n_reads] uint8; hap_reads[H, D + 1]; tally[4] =
        assigned, ambiguous, none, uninformative); wait=False only enqueues on this context's stream and returns None
        (phase_nearest_fetch brings the arrays)."""
        pos_cols = np.ascontiguousarray(pos_cols, dtype=np.uint32)
        hap_pattern = np.ascontiguousarray(hap_pattern, dtype=np.uint8)
        assert hap_pattern.ndim == 2 and hap_pattern.shape[1] == len(pos_cols)
        self._chk(self.lib.jl_phase_nearest_async(self.h, _p(pos_cols), len(pos_cols), _p(hap_pattern), hap_pattern.shape[1],
                                                  hap_pattern.shape[0], int(min_positions), int(max_distance)))
        self._nearest_shape = (self.n_reads, hap_pattern.shape[0], int(max_distance))
        return self.phase_nearest_fetch() if wait else None

    def phase_nearest_fetch(self):
        n, h, d = getattr(self, "_nearest_shape", (0, 0, 0))
        nearest = np.zeros(n, dtype=np.uint16)
        dist = np.zeros(n, dtype=np.uint8)
        hap_reads = np.zeros((h, d + 1), dtype=np.uint32)
        tally = np.zeros(4, dtype=np.uint64)
        self._chk(self.lib.jl_phase_nearest_fetch(self.h, _p(nearest), _p(dist), _p(hap_reads), _p(tally)))
        return dict(nearest=nearest, dist=dist, hap_reads=hap_reads, tally=tally)

    def phase_recombinants(self, pos_cols, hap_pattern, min_positions=1, wait=True):
        """jl_phase_recombinants_async (docs/SPEC.md §23): which reads of the resident matrix are recombinants of two haplotypes of
        hap_pattern[H, Vp] — one agrees with the read from the first position up to a breakpoint, another from there to the last.
        Returns dict(left[n_reads], right[n_reads] uint16: h, RESCUE_UNINFORMATIVE, RECOMB_WHOLE, RESCUE_NONE or RESCUE_AMBIGUOUS;
        prefix[n_reads], suffix[n_reads] uint16; parent_reads[H, 2]; tally[5] = recombinant, ambiguous_parent, whole, none,
        uninformative); wait=False only enqueues on this context's stream and returns None (phase_recombinants_fetch brings the
        arrays)."""
        pos_cols = np.ascontiguousarray(pos_cols, dtype=np.uint32)
        hap_pattern = np.ascontiguousarray(hap_pattern, dtype=np.uint8)
        assert hap_pattern.ndim == 2 and hap_pattern.shape[1] == len(pos_cols)
        self._chk(self.lib.jl_phase_recombinants_async(self.h, _p(pos_cols), len(pos_cols), _p(hap_pattern), hap_pattern.shape[1],
                                                       hap_pattern.shape[0], int(min_positions)))
        self._recomb_shape = (self.n_reads, hap_pattern.shape[0])
        return self.phase_recombinants_fetch() if wait else None

    def phase_recombinants_fetch(self):
        n, h = getattr(self, "_recomb_shape", (0, 0))
        per_read = {key: np.zeros(n, dtype=np.uint16) for key in ("left", "right", "prefix", "suffix")}
        parent_reads = np.zeros((h, 2), dtype=np.uint32)
        tally = np.zeros(5, dtype=np.uint64)
        self._chk(self.lib.jl_phase_recombinants_fetch(self.h, *(_p(per_read[key]) for key in ("left", "right", "prefix", "suffix")),
                                                       _p(parent_reads), _p(tally)))
        return dict(per_read, parent_reads=parent_reads, tally=tally)

    def variant_linkage(self, pos_cols, var_pos, var_codon, wait=True):
        """jl_variant_linkage_async (docs/SPEC.md §15): pairwise linkage of variants over every read covering both.  pos_cols[P]
        codon starts, strictly ascending; var_pos[V] indices into pos_cols, non-decreasing; var_codon[V] codons 0..63; P and V from
        1 to LINK_MAX.  Read i is informative at p iff its three codes at pos_cols[p] .. + 2 are all < 4; it carries v iff it is
        informative at var_pos[v] and its codon there equals var_codon[v].  Returns dict(both[P, P]: reads informative at p and q;
        carry[V, P]: reads that carry v and are informative at q; joint[V, V]: reads that carry v and w), 32 bits, exact;
        wait=False only enqueues on this context's stream and returns None (variant_linkage_fetch brings the arrays)."""
        pos_cols = np.ascontiguousarray(pos_cols, dtype=np.uint32)
        var_pos = np.ascontiguousarray(var_pos, dtype=np.uint32)
        var_codon = np.ascontiguousarray(var_codon, dtype=np.uint8)
        assert len(var_pos) == len(var_codon)
        self._chk(self.lib.jl_variant_linkage_async(self.h, _p(pos_cols), len(pos_cols), _p(var_pos), _p(var_codon), len(var_pos)))
        self._link_shape = (len(pos_cols), len(var_pos))
        return self.variant_linkage_fetch() if wait else None

    def variant_linkage_fetch(self):
        p, v = getattr(self, "_link_shape", (0, 0))
        both = np.zeros((p, p), dtype=np.uint32)
        carry = np.zeros((v, p), dtype=np.uint32)
        joint = np.zeros((v, v), dtype=np.uint32)
        self._chk(self.lib.jl_variant_linkage_fetch(self.h, _p(both), _p(carry), _p(joint)))
        return dict(both=both, carry=carry, joint=joint)

    def codon_deletions(self, wait=True):
        """jl_codon_deletions_async (docs/SPEC.md §16): at every codon start c (c + 2 < n_cols) of the resident matrix the reads
        with a whole codon there, with all three bases deleted, with a deletion that breaks the codon, and the reads spanning it.
        Returns cnt[n_cols - 2, 4] = (codon, del3, partial, span), uint32, exact; wait=False only enqueues on this context's
        stream and returns None (codon_deletions_fetch brings the array)."""
        self._chk(self.lib.jl_codon_deletions_async(self.h))
        self._del_cols = self.n_cols
        return self.codon_deletions_fetch() if wait else None

    def codon_deletions_fetch(self):
        cnt = np.zeros((max(0, getattr(self, "_del_cols", 0) - 2), 4), dtype=np.uint32)
        self._chk(self.lib.jl_codon_deletions_fetch(self.h, _p(cnt) if cnt.size else None))
        return cnt

    def deletion_alleles(self, wait=True):
        """jl_deletion_alleles_async (docs/SPEC.md §25): every read's maximal runs of '-' in the resident matrix.  Returns
        dict(runs = uint64[2] (bounded, open), open = uint32[n_cols] reads in an open run at each column, alleles =
        DELETION_ALLELE rows (col, len, count, flank), one per distinct bounded (start, length), ascending by (col, len)), all
        exact.  The call waits once, for the number of runs (the table is sized from it); wait=False then only enqueues the rest on
        this context's stream and returns None (deletion_alleles_fetch brings the arrays, in this call's own n_cols)."""
        self._chk(self.lib.jl_deletion_alleles_async(self.h))
        self._dal_cols = self.n_cols
        return self.deletion_alleles_fetch() if wait else None

    def deletion_alleles_fetch(self):
        runs = np.zeros(2, dtype=np.uint64)
        open_ = np.zeros(max(1, getattr(self, "_dal_cols", 0)), dtype=np.uint32)
        n = C.c_uint32(0)
        self._chk(self.lib.jl_deletion_alleles_fetch(self.h, _p(runs), _p(open_), None, 0, C.byref(n)))
        rows = np.zeros(n.value, dtype=DELETION_ALLELE)
        if n.value:
            self._chk(self.lib.jl_deletion_alleles_fetch(self.h, None, None, _p(rows), n.value, C.byref(n)))
        return dict(runs=runs, open=open_[: getattr(self, "_dal_cols", 0)], alleles=rows)

    def read_stats(self, compare=None, wait=True):
        """jl_read_stats_async (docs/SPEC.md §20): per read of the resident matrix, over all columns, its bases, gaps, masked cells,
        bases in compared columns and mismatches among those.  compare[n_cols]: a code per column, 4 or above = not compared (the
        output of consensus() can be passed as it is); None: no column is compared.  Returns stats[5, n_reads] (READ_BASES ..
        READ_MISMATCHES), uint32, exact; wait=False only enqueues on this context's stream and returns None (read_stats_fetch
        brings the array)."""
        if compare is not None:
            compare = np.ascontiguousarray(compare, dtype=np.uint8)
            assert compare.shape == (self.n_cols,)
        self._chk(self.lib.jl_read_stats_async(self.h, _p(compare)))
        self._rs_reads = self.n_reads
        return self.read_stats_fetch() if wait else None

    def read_stats_fetch(self):
        stats = np.zeros((READ_STATS, getattr(self, "_rs_reads", 0)), dtype=np.uint32)
        self._chk(self.lib.jl_read_stats_fetch(self.h, _p(stats) if stats.size else None))
        return stats

    def read_hypermut(self, ref, wait=True):
        """jl_read_hypermut_async (docs/SPEC.md §26): per read of the resident matrix its G->A sites in APOBEC's target context GRD
        and in the control contexts, the mutated ones of each, and the one-sided exact test of the two.  ref[n_cols]: a code per
        column, only G (2) makes a site.  Returns (counts[4, n_reads] uint32 (HM_TARGET_SITES .. HM_CONTROL_MUT), p[n_reads],
        log_p[n_reads]); wait=False only enqueues on this context's stream and returns None (read_hypermut_fetch brings them)."""
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        assert ref.shape == (self.n_cols,)
        self._chk(self.lib.jl_read_hypermut_async(self.h, _p(ref)))
        self._hm_reads = self.n_reads
        return self.read_hypermut_fetch() if wait else None

    def read_hypermut_fetch(self):
        n = getattr(self, "_hm_reads", 0)
        counts = np.zeros((HM_COUNTERS, n), dtype=np.uint32)
        p, lp = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64)
        self._chk(self.lib.jl_read_hypermut_fetch(self.h, *((_p(counts), _p(p), _p(lp)) if n else (None, None, None))))
        return counts, p, lp

    def read_orf(self, spans, ref, wait=True):
        """jl_read_orf_async (docs/SPEC.md §27): per (span, read) of the resident matrix the covered cells, the gap cells, the codons
        read in full, the stops the reference does not have, and the first of them.  spans: ORF_SPAN rows or (col, n_codons) pairs;
        ref[n_cols]: a code per column.  Returns (counts[4, n_spans, n_reads] uint32 (ORF_COVERED .. ORF_STOPS), first_stop[n_spans,
        n_reads] uint32, ORF_NO_STOP for none); wait=False only enqueues on this context's stream and returns None (read_orf_fetch
        brings them)."""
        spans = orf_spans(spans)
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        assert ref.shape == (self.n_cols,)
        self._chk(self.lib.jl_read_orf_async(self.h, _p(spans), len(spans), _p(ref)))
        self._orf_shape = (len(spans), self.n_reads)
        return self.read_orf_fetch() if wait else None

    def read_orf_fetch(self):
        s, n = getattr(self, "_orf_shape", (0, 0))
        counts = np.zeros((ORF_COUNTERS, s, n), dtype=np.uint32)
        first = np.zeros((s, n), dtype=np.uint32)
        self._chk(self.lib.jl_read_orf_fetch(self.h, *((_p(counts), _p(first)) if s * n else (None, None))))
        return counts, first

    def hypermut_eval(self, counts):
        """jl_hypermut_eval: the test kernel of jl_read_hypermut_async over counts[4, n] of the caller; (p, log_p)."""
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        assert counts.ndim == 2 and counts.shape[0] == HM_COUNTERS
        n = counts.shape[1]
        p, lp = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64)
        if n:
            self._chk(self.lib.jl_hypermut_eval(self.h, _p(counts), n, _p(p), _p(lp)))
        return p, lp

    def sites_assemble(self, src, sites):
        """jl_sites_assemble (docs/SPEC.md §18): this context becomes the site matrix of `src` — its reads x 3 len(sites) columns,
        site k = (col, kind, fill) at columns 3k..3k+2: the three columns at `col` of `src`, the del3 reads of a SITE_DELETION site
        recoded to codon SITE_DELETED and its codon reads to SITE_PRESENT, the del3 reads of a SITE_CODON site with a fill (0..63)
        recoded to that codon; everything else copied.  Sites ascend by (col, kind).  Waits on the host for `src`'s stream, enqueues
        on this context's and returns; phase_async / phase_fetch of this context then group over codon and deletion sites alike."""
        arr = np.zeros(len(sites), dtype=SITE)
        for k, (col, kind, fill) in enumerate(sites):
            arr[k] = (col, kind, fill, 0)
        self._chk(self.lib.jl_sites_assemble(self.h, src.h, _p(arr) if len(arr) else _p(np.zeros(1, dtype=SITE)), len(arr)))
        self._shape(src.n_reads, 3 * len(arr))
        self._keep = None

    def sites_assemble_alleles(self, src, sites, alleles):
        """jl_sites_assemble_alleles (docs/SPEC.md §19): sites_assemble, with sites of kind SITE_INSERTION (col = the junction,
        fill SITE_NO_FILL) whose letters are the listed alleles [(col, len, seq)] of that junction, ascending: a read of `src` with
        the allele of rank r at the junction becomes codon 1 + r there, a read without an insertion SITE_INS_NONE, one with an
        in-frame allele that is not listed SITE_INS_OTHER, a frame-shifting or unreadable insertion 4 4 4 or 5 5 5.  `src`: a record
        build with track_insertion_reads on."""
        arr = np.zeros(len(sites), dtype=SITE)
        for k, (col, kind, fill) in enumerate(sites):
            arr[k] = (col, kind, fill, 0)
        al = np.zeros(len(alleles), dtype=INSERTION_ALLELE)
        for k, a in enumerate(alleles):
            al[k] = (a[0], a[1], a[2], 0, 0)
        self._chk(self.lib.jl_sites_assemble_alleles(self.h, src.h, _p(arr) if len(arr) else _p(np.zeros(1, dtype=SITE)), len(arr),
                                                     _p(al) if len(al) else None, len(al)))
        self._shape(src.n_reads, 3 * len(arr))
        self._keep = None

    def call_async(self, params=None, drm_masks=None):
        prm = params or default_params()
        if drm_masks is not None:
            drm_masks = np.ascontiguousarray(drm_masks, dtype=np.uint64)
            assert len(drm_masks) == self.lib.jl_n_positions(self.h)
        self._chk(self.lib.jl_call_async(self.h, C.byref(prm), _p(drm_masks)))

    def call_fetch(self, cap=VARIANT_CAP):
        out = np.zeros(cap, dtype=VARIANT)
        n = C.c_uint32()
        self._chk(self.lib.jl_call_fetch(self.h, _p(out), cap, C.byref(n)))
        return out[: n.value].copy()

    def control_call_async(self, control, params=None, drm_masks=None):
        """jl_control_call_async (docs/SPEC.md §21) with this context as the sample: its pileup's codons against the counts of
        `control`'s pileup of the same window.  Enqueues only; `control` must not start another pileup before control_call_fetch
        or sync of this context."""
        prm = params or default_params()
        if drm_masks is not None:
            drm_masks = np.ascontiguousarray(drm_masks, dtype=np.uint64)
            assert len(drm_masks) == self.lib.jl_n_positions(self.h)
        self._chk(self.lib.jl_control_call_async(self.h, control.h, C.byref(prm), _p(drm_masks)))

    def control_call_fetch(self, cap=VARIANT_CAP):
        """(rows, control_coverage) of the last control_call_async: VARIANT rows with expected = the control's count of the codon,
        and the control's coverage at each row's position.  Beyond `cap` rows: JulietError (overflow), as call_fetch."""
        out = np.zeros(cap, dtype=VARIANT)
        cov = np.zeros(cap, dtype=np.uint32)
        n = C.c_uint32()
        self._chk(self.lib.jl_control_call_fetch(self.h, _p(out) if cap else None, _p(cov) if cap else None, cap, C.byref(n)))
        return out[: n.value].copy(), cov[: n.value].copy()

    def variant_table_device(self):
        rows, cnt, cap = C.c_void_p(), C.c_void_p(), C.c_uint32()
        self._chk(self.lib.jl_variant_table_device(self.h, C.byref(rows), C.byref(cnt), C.byref(cap)))
        return rows.value, cnt.value, cap.value

    def phase_async(self, variants=None, min_reads=10):
        if variants is None:
            self._chk(self.lib.jl_phase_async(self.h, None, 0, min_reads))
        else:
            variants = np.ascontiguousarray(variants, dtype=VARIANT)
            # a zero-length table still needs a non-NULL pointer to mean "this table", not "the resident one"
            buf = variants if len(variants) else np.zeros(1, dtype=VARIANT)
            self._chk(self.lib.jl_phase_async(self.h, _p(buf), len(variants), min_reads))

    def phase_fetch(self, want_reads=True, cap_var=VARIANT_CAP):
        summ = np.zeros(1, dtype=SUMMARY)
        pos_cols = np.zeros(cap_var, dtype=np.uint32)
        hap_count = np.zeros(MAX_HAPLOTYPES, dtype=np.uint32)
        hap_pattern = np.zeros((MAX_HAPLOTYPES, cap_var), dtype=np.uint8)
        hit = np.zeros((cap_var, MAX_HAPLOTYPES), dtype=np.uint8)
        read_hap = np.zeros(self.n_reads, dtype=np.uint16) if want_reads else None
        cooc = np.zeros((cap_var, cap_var), dtype=np.uint32) if cap_var <= 1024 else None
        self._chk(self.lib.jl_phase_fetch(self.h, _p(summ), _p(pos_cols), _p(hap_count), _p(hap_pattern), _p(hit),
                                          _p(read_hap), _p(cooc), cap_var))
        s = {k: int(summ[0][k]) for k in SUMMARY_FIELDS}
        h, vp = s["n_haplotypes"], s["n_positions"]
        return dict(summary=s, pos_cols=pos_cols[:vp].copy(), hap_count=hap_count[:h].copy(),
                    hap_pattern=hap_pattern[:h, :vp].copy(), hit=hit, read_hap=read_hap, cooc=cooc)

    # ------------------------------------------------------------------ phasing sharded by reads (SURVEY §8e option A)
    def phase_groups_async(self, variants):
        """Keys + grouping of the resident matrix (a slice of the reads); the groups are exported, not ranked."""
        variants = np.ascontiguousarray(variants, dtype=VARIANT)
        buf = variants if len(variants) else np.zeros(1, dtype=VARIANT)
        self._chk(self.lib.jl_phase_groups_async(self.h, _p(buf), len(variants)))

    def phase_groups_fetch(self, cap_var=64):
        """dict(patterns uint8[G][Vp], counts uint32[G], pos_cols, summary): the groups of the last phase_groups_async."""
        ng, vp = C.c_uint32(), C.c_uint32()
        summ = np.zeros(1, dtype=SUMMARY)
        self._chk(self.lib.jl_phase_groups_fetch(self.h, None, 0, None, 0, C.byref(ng), C.byref(vp), None, 0, _p(summ)))
        g, v = ng.value, vp.value
        patterns = np.zeros((max(g, 1), max(v, 1)), dtype=np.uint8)
        counts = np.zeros(max(g, 1), dtype=np.uint32)
        pos_cols = np.zeros(max(v, 1), dtype=np.uint32)
        self._chk(self.lib.jl_phase_groups_fetch(self.h, _p(patterns), patterns.shape[1], _p(counts), len(counts), C.byref(ng),
                                                 C.byref(vp), _p(pos_cols), len(pos_cols), _p(summ)))
        return dict(patterns=patterns[:g, :v].copy(), counts=counts[:g].copy(), pos_cols=pos_cols[:v].copy(),
                    summary={k: int(summ[0][k]) for k in SUMMARY_FIELDS})

    def phase_regroup(self, hap_of_group, n_haplotypes, want_reads=True):
        """hap_of_group[q] = haplotype of exported group q after the merge (HAP_INSUFFICIENT: not reported) -> per-read ids."""
        hap = np.ascontiguousarray(hap_of_group, dtype=np.uint16)
        read_hap = np.zeros(self.n_reads, dtype=np.uint16) if want_reads else None
        self._chk(self.lib.jl_phase_regroup(self.h, _p(hap if len(hap) else np.zeros(1, dtype=np.uint16)), len(hap), n_haplotypes,
                                            _p(read_hap)))
        return read_hap

    def xwin_assemble_slice_local(self, windows, merged, read_begin, n_slice):
        """This context becomes the compact matrix of reads [read_begin, read_begin + n_slice) of the windows' variant
        columns.  Returns (remapped table, pos_global)."""
        merged = np.ascontiguousarray(merged, dtype=VARIANT)
        arr = (C.c_void_p * len(windows))(*[w.h for w in windows])
        remapped = np.zeros(max(len(merged), 1), dtype=VARIANT)
        pos_global = np.zeros(max(len(merged), 1), dtype=np.uint32)
        vp = C.c_uint32()
        self._chk(self.lib.jl_xwin_assemble_slice_local(self.h, arr, len(windows), _p(merged if len(merged) else remapped), len(merged),
                                                        read_begin, n_slice, _p(remapped), _p(pos_global), C.byref(vp)))
        if vp.value and n_slice:
            self._shape(n_slice, 3 * vp.value)
        return remapped[: len(merged)], pos_global[: vp.value]

    def xwin_assemble_slice_rccl(self, window, comm, win_begins, win_ncols, merged, slice_begin):
        """One window per rank: this context becomes the compact matrix of THIS rank's slice of the reads
        (slice_begin: world + 1 starts, sharding.read_slices).  Returns (remapped table, pos_global, reads of the slice)."""
        merged = np.ascontiguousarray(merged, dtype=VARIANT)
        wb = np.ascontiguousarray(win_begins, dtype=np.uint32)
        wn = np.ascontiguousarray(win_ncols, dtype=np.uint32)
        sb = np.ascontiguousarray(slice_begin, dtype=np.uint64)
        remapped = np.zeros(max(len(merged), 1), dtype=VARIANT)
        pos_global = np.zeros(max(len(merged), 1), dtype=np.uint32)
        vp = C.c_uint32()
        self._chk(self.lib.jl_xwin_assemble_slice_rccl(self.h, window.h, comm, _p(wb), _p(wn), _p(merged if len(merged) else remapped),
                                                       len(merged), _p(sb), _p(remapped), _p(pos_global), C.byref(vp)))
        return remapped[: len(merged)], pos_global[: vp.value], vp.value

    def fisher_eval(self, a, c, cov, tail=0):
        a, c, cov = (np.ascontiguousarray(x, dtype=np.uint32) for x in (a, c, cov))
        p = np.zeros(len(a), dtype=np.float64)
        lp = np.zeros(len(a), dtype=np.float64)
        self._chk(self.lib.jl_fisher_eval_tail(self.h, _p(a), _p(c), _p(cov), len(a), tail, _p(p), _p(lp)))
        return p, lp

    def control_eval(self, a, cov_s, c, cov_c, n_tests=None, alpha=None):
        """jl_control_eval: the general-margin routine of the control call on the device, one table [[a, cov_s - a],
        [c, cov_c - c]] per element.  (p, log_p) of the plain form; with n_tests and alpha (p, log_p, skipped) of the gated one."""
        a, cov_s, c, cov_c = (np.ascontiguousarray(x, dtype=np.uint32) for x in (a, cov_s, c, cov_c))
        assert len(a) == len(cov_s) == len(c) == len(cov_c)
        p = np.zeros(len(a), dtype=np.float64)
        lp = np.zeros(len(a), dtype=np.float64)
        if n_tests is None:
            self._chk(self.lib.jl_control_eval(self.h, _p(a), _p(cov_s), _p(c), _p(cov_c), len(a), 0.0, 0.0, _p(p), _p(lp), None))
            return p, lp
        sk = np.zeros(len(a), dtype=np.uint32)
        self._chk(self.lib.jl_control_eval(self.h, _p(a), _p(cov_s), _p(c), _p(cov_c), len(a), n_tests, alpha, _p(p), _p(lp), _p(sk)))
        return p, lp, sk.astype(bool)

    def sync(self):
        self._chk(self.lib.jl_sync(self.h))

    def run_pileup_clock(self, on=True):
        """Clock nodes around the pileup launch of this context's runs (jl_run_pileup_clock)."""
        self._chk(self.lib.jl_run_pileup_clock(self.h, 1 if on else 0))

    def run_pileup_ms(self):
        """ms the pileup of the last run took where it ran (jl_run_pileup_ms; waits for the run)."""
        ms = C.c_float()
        self._chk(self.lib.jl_run_pileup_ms(self.h, C.byref(ms), None))
        return float(ms.value)

    def run_pileup_interval(self):
        """(begin, end) of the last run's pileup in ms of the device's 100 MHz clock (one clock for all contexts of a device)."""
        ms, t0 = C.c_float(), C.c_uint64()
        self._chk(self.lib.jl_run_pileup_ms(self.h, C.byref(ms), C.byref(t0)))
        return 1e-5 * t0.value, 1e-5 * t0.value + float(ms.value)

    def time_run(self, genes, refseq=None, params=None, drm_masks=None, phasing=True, min_reads=10, want_read_hap=True, reps=20):
        """jl_time_run: average ms per run of `reps` runs one after the other, launched and waited for inside the library
        (the latency of the path at the C ABI, without this interpreter between the runs)."""
        g = np.ascontiguousarray(genes, dtype=GENE)
        r = None if refseq is None else np.ascontiguousarray(refseq, dtype=np.uint8)
        d = None if drm_masks is None else np.ascontiguousarray(drm_masks, dtype=np.uint64)
        prm = params or default_params()
        ms = C.c_float()
        self._chk(self.lib.jl_time_run(self.h, _p(g), len(g), _p(r), 0 if r is None else len(r), C.byref(prm), _p(d),
                                       1 if phasing else 0, min_reads, 1 if want_read_hap else 0, reps, C.byref(ms)))
        return float(ms.value)

    def time_pileup(self, reps=20):
        ms = C.c_float()
        self._chk(self.lib.jl_time_pileup(self.h, reps, C.byref(ms)))
        return ms.value

    # ------------------------------------------------------------------ the whole path in one enqueue
    def run_async(self, genes, refseq=None, params=None, drm_masks=None, phasing=True, min_reads=10,
                  want_read_hap=True):
        """pileup -> call (-> phase) as one captured HIP graph + one pinned result copy (jl_run_async)."""
        key = (id(genes), id(refseq), id(params), id(drm_masks))
        c = getattr(self, "_run_args", None)
        if c is None or c[0] != key:   # argument marshalling is cached: repeated steps pass the same objects
            g = np.ascontiguousarray(genes, dtype=GENE)
            r = None if refseq is None else np.ascontiguousarray(refseq, dtype=np.uint8)
            d = None if drm_masks is None else np.ascontiguousarray(drm_masks, dtype=np.uint64)
            prm = params or default_params()
            c = (key, (genes, refseq, params, drm_masks), (g, r, d, prm),
                 (_p(g), len(g), _p(r), 0 if r is None else len(r), C.byref(prm), _p(d)))
            self._run_args = c
        a = c[3]
        rc = self.lib.jl_run_async(self.h, a[0], a[1], a[2], a[3], a[4], a[5], 1 if phasing else 0, min_reads,
                                   1 if want_read_hap else 0)
        if rc:
            self._chk(rc)

    def _bufs(self, cap_var):
        b = getattr(self, "_fetch_bufs", None)
        if b is None or b["cap_var"] != cap_var or len(b["read_hap"]) != self.n_reads:
            b = dict(cap_var=cap_var, variants=np.zeros(VARIANT_CAP, dtype=VARIANT), n=C.c_uint32(),
                     summ=np.zeros(1, dtype=SUMMARY), pos_cols=np.zeros(cap_var, dtype=np.uint32),
                     hap_count=np.zeros(MAX_HAPLOTYPES, dtype=np.uint32),
                     hap_pattern=np.zeros((MAX_HAPLOTYPES, cap_var), dtype=np.uint8),
                     hit=np.zeros((cap_var, MAX_HAPLOTYPES), dtype=np.uint8),
                     read_hap=np.zeros(self.n_reads, dtype=np.uint16),
                     cooc=np.zeros((cap_var, cap_var), dtype=np.uint32))
            b["ptr"] = {k: _p(v) for k, v in b.items() if isinstance(v, np.ndarray)}
            b["n_ref"] = C.byref(b["n"])
            self._fetch_bufs = b
        return b

    def run_fetch(self, phasing=True, want_read_hap=True, cap_var=64):
        """Results of the last run_async.  Returned arrays are views of buffers reused by the next call."""
        b = self._bufs(cap_var)
        q = b["ptr"]
        rc = self.lib.jl_call_fetch(self.h, q["variants"], VARIANT_CAP, b["n_ref"])
        if rc:
            self._chk(rc)
        nv = b["n"].value
        out = dict(variants=b["variants"][:nv])
        if phasing:
            rc = self.lib.jl_phase_fetch(self.h, q["summ"], q["pos_cols"], q["hap_count"], q["hap_pattern"], q["hit"],
                                         q["read_hap"] if want_read_hap else None, q["cooc"], cap_var)
            if rc:
                self._chk(rc)
            s = dict(zip(SUMMARY_FIELDS, b["summ"][0].tolist()))
            h, vp = s["n_haplotypes"], s["n_positions"]
            out["phase"] = dict(summary=s, pos_cols=b["pos_cols"][:vp], hap_count=b["hap_count"][:h],
                                hap_pattern=b["hap_pattern"][:h, :vp], hit=b["hit"][:nv, :h],
                                read_hap=b["read_hap"] if want_read_hap else None, cooc=b["cooc"][:nv, :nv])
        return out

    def run_wait(self):
        """Block until the last run_async's results are on the host (pinned sequence word, no HIP sync)."""
        rc = self.lib.jl_run_wait(self.h)
        if rc:
            self._chk(rc)

    def run_done(self):
        return bool(self.lib.jl_run_done(self.h))

    def run_view_raw(self):
        """The jl_run_view struct itself (counts, read categories, pointers into the pinned result block): waits for the
        run like run_view, without building numpy views.  `complete` = 0: use run_fetch."""
        v = getattr(self, "_rv", None)
        if v is None:
            v = self._rv = RunView()
            self._rv_ref = C.byref(v)
            self._rv_cache = {}
        rc = self.lib.jl_run_view_get(self.h, self._rv_ref)
        if rc:
            self._chk(rc)
        return v

    def run_view(self):
        """Zero-copy results of the last run_async: numpy views of the pinned block the kernels stored into
        (valid until the next run on this context).  Returns None when the results do not fit that block
        (more than 128 variants / positions / haplotypes) — use run_fetch then."""
        v = getattr(self, "_rv", None)
        if v is None:
            v = self._rv = RunView()
            self._rv_ref = C.byref(v)
            self._rv_cache = {}
        rc = self.lib.jl_run_view_get(self.h, self._rv_ref)
        if rc:
            self._chk(rc)
        if not v.complete:
            return None
        key = (v.variants, v.read_hap_packed, v.n_reads, v.phased)
        c = self._rv_cache.get(key)
        if c is None:   # base arrays over the whole block, built once per allocation
            c = dict(variants=_view(v.variants, VARIANT, 128))
            if v.phased:
                c.update(pos_cols=_view(v.pos_cols, np.uint32, 128), hap_count=_view(v.hap_count, np.uint32, 128),
                         hap_pattern=_view(v.hap_pattern, np.uint8, PACK_PATTERN_BYTES), hit=_view(v.hit, np.uint8, PACK_HIT_BYTES),
                         cooc=_view(v.cooc, np.uint32, 4096) if v.cooc else None,
                         ids=_view(v.read_hap_packed, np.uint8, 2 * v.n_reads) if v.read_hap_packed else None)
            self._rv_cache = {key: c}
        nv = v.n_variants
        if not v.phased:
            return dict(variants=c["variants"][:nv])
        # the sliced and reshaped views are kept while the results keep their shape (a step loop's runs do): they look at
        # the same pinned block, whose contents the run has replaced; the summary and the ids' holder are made per run
        h, vp, nvp = v.n_haplotypes, v.n_positions, v.n_var_phase
        shape = (nv, h, vp, nvp, bool(v.cooc))
        sh = c.get("shaped")
        if sh is None or sh[0] != shape:
            sh = c["shaped"] = (shape, c["variants"][:nv],
                                dict(pos_cols=c["pos_cols"][:vp], hap_count=c["hap_count"][:h],
                                     hap_pattern=c["hap_pattern"][:h * vp].reshape(h, vp), hit=c["hit"][:nvp * h].reshape(nvp, h),
                                     cooc=None if c["cooc"] is None or not v.cooc else c["cooc"][:nvp * nvp].reshape(nvp, nvp)))
        ph = dict(sh[2])
        ph["summary"] = {n: getattr(v.summary, n) for n in SUMMARY_FIELDS}
        ph["read_hap"] = _LazyIds(c["ids"], v.read_hap_bits, v.n_reads) if c["ids"] is not None else None
        return dict(variants=sh[1], phase=ph)

    def run(self, genes, refseq=None, params=None, drm_masks=None, phasing=True, min_reads=10):
        """The whole hot path, blocking; arrays are copies."""
        self.run_async(genes, refseq, params, drm_masks, phasing, min_reads, want_read_hap=True)
        cap = 64
        while True:
            try:
                out = self.run_fetch(phasing, True, cap_var=cap)
                break
            except JulietError as e:
                if e.status != -5 or cap >= VARIANT_CAP:
                    raise
                cap = min(VARIANT_CAP, cap * 8)
        res = dict(variants=out["variants"].copy())
        if phasing:
            res["phase"] = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in out["phase"].items()}
        return res


def xwin_plan(win_begins, win_ncols, merged):
    """Host-only plan of the cross-window column exchange (jl_xwin_plan): (remapped table, global positions, owner window
    of each position).  Needs no GPU."""
    lib = load_library()
    merged = np.ascontiguousarray(merged, dtype=VARIANT)
    wb = np.ascontiguousarray(win_begins, dtype=np.uint32)
    wn = np.ascontiguousarray(win_ncols, dtype=np.uint32)
    remapped = np.zeros(max(1, len(merged)), dtype=VARIANT)
    pos = np.zeros(max(1, len(merged)), dtype=np.uint32)
    owner = np.zeros(max(1, len(merged)), dtype=np.int32)
    vp = C.c_uint32()
    rc = lib.jl_xwin_plan(_p(wb), _p(wn), len(wb), _p(merged), len(merged), _p(remapped), _p(pos), _p(owner), C.byref(vp))
    if rc:
        raise JulietError(rc, "jl_xwin_plan")
    return remapped[: len(merged)].copy(), pos[: vp.value].copy(), owner[: vp.value].copy()


def sample_reads(n_reads, k, seed=0):
    """jl_sample_reads (host only, docs/SPEC.md §12): the min(k, n_reads) reads a downsample keeps — the smallest
    (splitmix64(seed + i), i) — as ascending uint32 indices.  Samples of one seed are nested."""
    lib = load_library()
    out = np.zeros(max(1, min(int(k), int(n_reads))), dtype=np.uint32)
    n = C.c_uint64()
    rc = lib.jl_sample_reads(int(n_reads), int(k), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(out), C.byref(n))
    if rc:
        raise JulietError(rc, "jl_sample_reads")
    return out[: n.value].copy()


def consensus_of_counts(counts2d):
    """jl_consensus_of_counts (host only, docs/SPEC.md §13): the per-column consensus of one [n_cols, 6] count table — majority
    of A C G T -, lowest code on ties; 4 = majority deletion, 5 = nobody covers the column."""
    lib = load_library()
    counts2d = np.ascontiguousarray(counts2d, dtype=np.uint32)
    assert counts2d.ndim == 2 and counts2d.shape[1] == 6
    out = np.zeros(max(1, len(counts2d)), dtype=np.uint8)
    rc = lib.jl_consensus_of_counts(_p(counts2d), len(counts2d), _p(out))
    if rc:
        raise JulietError(rc, "jl_consensus_of_counts")
    return out[: len(counts2d)].copy()


class LinkPair(C.Structure):
    _fields_ = [("n", C.c_uint32), ("n11", C.c_uint32), ("n10", C.c_uint32), ("n01", C.c_uint32), ("n00", C.c_uint32),
                ("pad_", C.c_uint32), ("r2", C.c_double), ("d_prime", C.c_double), ("p_positive", C.c_double),
                ("p_negative", C.c_double)]


def linkage_stats(both, carry, joint, var_pos, v, w):
    """jl_linkage_stats (host only, docs/SPEC.md §15): the 2 x 2 table of the pair (v, w) — variants at different positions —
    from the tables of Juliet.variant_linkage, and its statistics: dict(n, n11, n10, n01, n00, r2, d_prime, p_positive,
    p_negative); the p-values are the two one-sided Fisher tests, not Bonferroni-corrected."""
    lib = load_library()
    both = np.ascontiguousarray(both, dtype=np.uint32)
    carry = np.ascontiguousarray(carry, dtype=np.uint32)
    joint = np.ascontiguousarray(joint, dtype=np.uint32)
    var_pos = np.ascontiguousarray(var_pos, dtype=np.uint32)
    n_pos, n_var = both.shape[0], joint.shape[0]
    assert both.shape == (n_pos, n_pos) and carry.shape == (n_var, n_pos) and joint.shape == (n_var, n_var) and len(var_pos) == n_var
    out = LinkPair()
    rc = lib.jl_linkage_stats(_p(both), _p(carry), _p(joint), _p(var_pos), n_pos, n_var, int(v), int(w), C.byref(out))
    if rc:
        raise JulietError(rc, "jl_linkage_stats: " + lib.jl_last_error(None).decode())
    return {name: getattr(out, name) for name, _ in LinkPair._fields_ if name != "pad_"}


class HapRecombinant(C.Structure):
    _fields_ = [("flagged", C.c_uint32), ("left", C.c_uint32), ("right", C.c_uint32), ("prefix", C.c_uint32), ("suffix", C.c_uint32)]


def haplotype_recombinants(hap_pattern, hap_count, min_parent_ratio=2.0):
    """jl_haplotype_recombinants (host only, docs/SPEC.md §23): for every row h of hap_pattern[H, Vp], whether it is a common prefix
    of one row and a common suffix of another that together cover it, both among the rows with hap_count >= min_parent_ratio *
    hap_count[h]: a list of dict(flagged, left, right, prefix, suffix)."""
    lib = load_library()
    hap_pattern = np.ascontiguousarray(hap_pattern, dtype=np.uint8)
    hap_count = np.ascontiguousarray(hap_count, dtype=np.uint32)
    assert hap_pattern.ndim == 2 and len(hap_count) == hap_pattern.shape[0]
    out = (HapRecombinant * max(1, hap_pattern.shape[0]))()
    rc = lib.jl_haplotype_recombinants(_p(hap_pattern), hap_pattern.shape[1], hap_pattern.shape[0], hap_pattern.shape[1], _p(hap_count),
                                       float(min_parent_ratio), C.byref(out))
    if rc:
        raise JulietError(rc, "jl_haplotype_recombinants: " + lib.jl_last_error(None).decode())
    return [dict(flagged=bool(o.flagged), left=o.left, right=o.right, prefix=o.prefix, suffix=o.suffix) for o in out[: hap_pattern.shape[0]]]


class DeletionCall(C.Structure):
    _fields_ = [("count", C.c_uint32), ("coverage", C.c_uint32), ("expected", C.c_uint32), ("partial", C.c_uint32),
                ("called", C.c_uint32), ("pad_", C.c_uint32), ("p_value", C.c_double), ("log_p", C.c_double)]


def deletion_test(cnt, params, n_tests):
    """jl_deletion_test (host only, docs/SPEC.md §16): one row (codon, del3, partial, span) of Juliet.codon_deletions against the
    error model's deletion rate, with the codon test's resolved Bonferroni factor n_tests: dict(count, coverage, expected,
    partial, called, p_value = min(1, p * n_tests), log_p = ln p)."""
    lib = load_library()
    cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
    assert cnt.shape == (4,)
    out = DeletionCall()
    rc = lib.jl_deletion_test(_p(cnt), C.byref(params), float(n_tests), C.byref(out))
    if rc:
        raise JulietError(rc, "jl_deletion_test: " + lib.jl_last_error(None).decode())
    d = {name: getattr(out, name) for name, _ in DeletionCall._fields_ if name != "pad_"}
    d["called"] = bool(d["called"])
    return d


class DeletionAlleleCall(C.Structure):
    _fields_ = [("count", C.c_uint32), ("coverage", C.c_uint32), ("expected", C.c_uint32), ("called", C.c_uint32),
                ("p_value", C.c_double), ("log_p", C.c_double)]


def deletion_allele_test(count, flank, params, rate, n_tests):
    """jl_deletion_allele_test (host only, docs/SPEC.md §25): one row of Juliet.deletion_alleles against a rate of such deletions by
    error, coverage = flank, with the codon test's resolved Bonferroni factor n_tests: dict(count, coverage, expected, called,
    p_value = min(1, p * n_tests), log_p = ln p)."""
    lib = load_library()
    out = DeletionAlleleCall()
    rc = lib.jl_deletion_allele_test(int(count), int(flank), C.byref(params), float(rate), float(n_tests), C.byref(out))
    if rc:
        raise JulietError(rc, "jl_deletion_allele_test: " + lib.jl_last_error(None).decode())
    d = {name: getattr(out, name) for name, _ in DeletionAlleleCall._fields_}
    d["called"] = bool(d["called"])
    return d


class ControlCall(C.Structure):
    _fields_ = [("count", C.c_uint32), ("coverage", C.c_uint32), ("control_count", C.c_uint32), ("control_coverage", C.c_uint32),
                ("called", C.c_uint32), ("pad_", C.c_uint32), ("p_value", C.c_double), ("log_p", C.c_double)]


def control_test(a, cov_s, c, cov_c, params, n_tests):
    """jl_control_test (host only, docs/SPEC.md §21): the table [[a, cov_s - a], [c, cov_c - c]] of a sample against a control
    through the routine the kernel compiles: dict(count, coverage, control_count, control_coverage, called, p_value = min(1, p *
    n_tests), log_p = ln p)."""
    lib = load_library()
    out = ControlCall()
    rc = lib.jl_control_test(int(a), int(cov_s), int(c), int(cov_c), C.byref(params), float(n_tests), C.byref(out))
    if rc:
        raise JulietError(rc, "jl_control_test: " + lib.jl_last_error(None).decode())
    d = {name: getattr(out, name) for name, _ in ControlCall._fields_ if name != "pad_"}
    d["called"] = bool(d["called"])
    return d


def read_rule(min_bases=0, max_mismatches=0xFFFFFFFF, max_mismatch_perc=-1.0, max_gap_perc=-1.0, max_masked_perc=-1.0):
    """A jl_read_rule; the defaults switch every rule off."""
    return ReadRule(int(min_bases), int(max_mismatches), float(max_mismatch_perc), float(max_gap_perc), float(max_masked_perc))


def read_filter(stats, **rule):
    """jl_read_filter (host only, docs/SPEC.md §20): the reads of Juliet.read_stats' table that pass every rule that is switched
    on (read_rule's keywords) — (idx, failed): ascending uint32 indices, what Juliet.take takes, and failed[5] = reads failing
    each of READ_RULES (a read that fails several counts in each)."""
    lib = load_library()
    stats = np.ascontiguousarray(stats, dtype=np.uint32)
    assert stats.ndim == 2 and stats.shape[0] == READ_STATS
    n = stats.shape[1]
    idx = np.zeros(max(1, n), dtype=np.uint32)
    failed = np.zeros(5, dtype=np.uint64)
    kept = C.c_uint64()
    r = read_rule(**rule)
    rc = lib.jl_read_filter(_p(stats), n, C.byref(r), _p(idx), C.byref(kept), _p(failed))
    if rc:
        raise JulietError(rc, "jl_read_filter: " + lib.jl_last_error(None).decode())
    return idx[: kept.value].copy(), failed


def hypermut_test(target_mut, target_sites, control_mut, control_sites):
    """jl_hypermut_test (host only, docs/SPEC.md §26): (p, log_p) of one read's table, P(X >= target_mut) one-sided."""
    lib = load_library()
    p, lp = C.c_double(), C.c_double()
    rc = lib.jl_hypermut_test(int(target_mut), int(target_sites), int(control_mut), int(control_sites), C.byref(p), C.byref(lp))
    if rc:
        raise JulietError(rc, "jl_hypermut_test: " + lib.jl_last_error(None).decode())
    return p.value, lp.value


def hypermut_filter(p, alpha=0.05):
    """jl_hypermut_filter (host only, docs/SPEC.md §26): (idx, n_flagged) — the reads with p >= alpha, ascending uint32 indices, what
    Juliet.take takes, and how many reads were flagged as hypermutated (p < alpha)."""
    lib = load_library()
    p = np.ascontiguousarray(p, dtype=np.float64)
    assert p.ndim == 1
    idx = np.zeros(max(1, len(p)), dtype=np.uint32)
    kept, flagged = C.c_uint64(), C.c_uint64()
    rc = lib.jl_hypermut_filter(_p(p), len(p), float(alpha), _p(idx), C.byref(kept), C.byref(flagged))
    if rc:
        raise JulietError(rc, "jl_hypermut_filter: " + lib.jl_last_error(None).decode())
    return idx[: kept.value].copy(), flagged.value


def orf_spans(spans):
    """ORF_SPAN rows of (col, n_codons) pairs, or of an ORF_SPAN array as it stands."""
    if isinstance(spans, np.ndarray) and spans.dtype == ORF_SPAN:
        return np.ascontiguousarray(spans)
    return np.array([tuple(int(x) for x in s) for s in spans], dtype=ORF_SPAN)


def orf_classify(counts, first_stop, spans, max_gap_cells=0, tail_codons=0):
    """jl_orf_classify (host only, docs/SPEC.md §27): flags[n_spans, n_reads] uint8 of ORF_PARTIAL | ORF_STOP | ORF_FRAMESHIFT |
    ORF_DELETION from counts[4, n_spans, n_reads] and first_stop[n_spans, n_reads]."""
    lib = load_library()
    spans = orf_spans(spans)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    first_stop = np.ascontiguousarray(first_stop, dtype=np.uint32)
    assert counts.ndim == 3 and counts.shape[:2] == (ORF_COUNTERS, len(spans)) and first_stop.shape == counts.shape[1:]
    flags = np.zeros(first_stop.shape, dtype=np.uint8)
    rule = OrfRule(int(max_gap_cells), int(tail_codons))
    rc = lib.jl_orf_classify(_p(counts), _p(first_stop), _p(spans), len(spans), first_stop.shape[1], C.byref(rule), _p(flags))
    if rc:
        raise JulietError(rc, "jl_orf_classify: " + lib.jl_last_error(None).decode())
    return flags


def orf_filter(flags, mask=ORF_STOP | ORF_FRAMESHIFT):
    """jl_orf_filter (host only, docs/SPEC.md §27): (idx, n_flagged) — the reads none of whose spans' flags meets `mask`, ascending
    uint32 indices, what Juliet.take takes, and how many reads were defective."""
    lib = load_library()
    flags = np.ascontiguousarray(flags, dtype=np.uint8)
    assert flags.ndim == 2
    idx = np.zeros(max(1, flags.shape[1]), dtype=np.uint32)
    kept, flagged = C.c_uint64(), C.c_uint64()
    rc = lib.jl_orf_filter(_p(flags), flags.shape[0], flags.shape[1], int(mask), _p(idx), C.byref(kept), C.byref(flagged))
    if rc:
        raise JulietError(rc, "jl_orf_filter: " + lib.jl_last_error(None).decode())
    return idx[: kept.value].copy(), flagged.value


class InsertionCall(C.Structure):
    _fields_ = [("count", C.c_uint32), ("coverage", C.c_uint32), ("expected", C.c_uint32), ("frameshift", C.c_uint32),
                ("unread", C.c_uint32), ("called", C.c_uint32), ("p_value", C.c_double), ("log_p", C.c_double)]


def insertion_test(count, jcnt, params, rate, n_tests):
    """jl_insertion_test (host only, docs/SPEC.md §17): `count` reads of one allele at a junction whose row of
    Juliet.insertion_alleles()[0] is jcnt = (span, inframe, frameshift, unread), against `rate`, with the codon test's resolved
    Bonferroni factor n_tests: dict(count, coverage, expected, frameshift, unread, called, p_value = min(1, p * n_tests), log_p)."""
    lib = load_library()
    jcnt = np.ascontiguousarray(jcnt, dtype=np.uint32)
    assert jcnt.shape == (4,)
    out = InsertionCall()
    rc = lib.jl_insertion_test(int(count), _p(jcnt), C.byref(params), float(rate), float(n_tests), C.byref(out))
    if rc:
        raise JulietError(rc, "jl_insertion_test: " + lib.jl_last_error(None).decode())
    d = {name: getattr(out, name) for name, _ in InsertionCall._fields_}
    d["called"] = bool(d["called"])
    return d


def mix_counts(n_sources, coverage, percentage):
    """jl_mix_counts (host only, doc/MIXDATA.md:10-22): reads per source of a mixture — every minor
    floor(coverage * percentage / 100), the first source the rest."""
    lib = load_library()
    out = np.zeros(max(1, int(n_sources)), dtype=np.uint64)
    rc = lib.jl_mix_counts(int(n_sources), int(coverage), float(percentage), _p(out))
    if rc:
        raise JulietError(rc, "jl_mix_counts")
    return out[: int(n_sources)].copy()


def qmask_from_quals(seq_off, qual, qual_off, min_qv):
    """jl_qmask_from_quals (host only): the byte form's filter — qual < min(min_qv, 127) and not 0xFF — as one bit per base,
    bit 2 * (seq_off[r] - seq_off[0]) + q for base q of read r (include/juliet_hip.h)."""
    lib = load_library()
    seq_off = np.ascontiguousarray(seq_off, dtype=np.uint64)
    qual_off = np.ascontiguousarray(qual_off, dtype=np.uint64)
    qual = np.ascontiguousarray(qual, dtype=np.uint8)
    n = len(seq_off) - 1
    out = np.zeros(int(lib.jl_qmask_bytes(int(seq_off[-1] - seq_off[0]))), dtype=np.uint8)
    rc = lib.jl_qmask_from_quals(n, _p(seq_off), _p(qual), _p(qual_off), min_qv, _p(out), len(out))
    if rc != 0:
        raise JulietError(rc, "jl_qmask_from_quals")
    return out


def qmask_slice(qmask, seq_byte, seq_bytes):
    """The mask of the `seq_bytes` bytes of packed bases from byte `seq_byte` on, out of a mask of the whole array: two bits per
    byte, moved down to bit 0."""
    bits = np.unpackbits(np.ascontiguousarray(qmask, dtype=np.uint8), bitorder="little")[2 * seq_byte:2 * (seq_byte + seq_bytes)]
    return np.packbits(bits, bitorder="little") if len(bits) else np.zeros(1, dtype=np.uint8)


def merge_tables(tables, win_begins):
    """jl_merge_tables: per-window tables (window-relative `col`) -> one table, global columns, (gene, codon_pos, codon) order."""
    lib = load_library()
    tabs = [np.ascontiguousarray(t, dtype=VARIANT) for t in tables]
    n = len(tabs)
    ptrs = (C.c_void_p * max(1, n))(*[t.ctypes.data if len(t) else None for t in tabs])
    counts = np.array([len(t) for t in tabs], dtype=np.uint32)
    wb = np.ascontiguousarray(win_begins, dtype=np.uint32)
    total = int(counts.sum())
    out = np.zeros(max(1, total), dtype=VARIANT)
    got = C.c_uint32()
    rc = lib.jl_merge_tables(ptrs, _p(counts), _p(wb), n, _p(out), len(out), C.byref(got))
    if rc:
        raise JulietError(rc, "jl_merge_tables")
    return out[: got.value].copy()


def merge_groups(tables):
    """jl_merge_groups: per-slice group tables dict(patterns uint8[G][Vp], counts uint32[G]) -> (distinct patterns ascending,
    summed counts int64, per table the merged row of each of its groups)."""
    lib = load_library()
    vp = max((np.asarray(t["patterns"]).reshape(len(t["counts"]), -1).shape[1] for t in tables if len(t["counts"])), default=0)
    pats = [np.ascontiguousarray(np.asarray(t["patterns"], dtype=np.uint8).reshape(len(t["counts"]), -1)[:, :vp]) if len(t["counts"])
            else np.zeros((0, vp), dtype=np.uint8) for t in tables]
    cnts = [np.ascontiguousarray(t["counts"], dtype=np.uint32) for t in tables]
    n = len(tables)
    total = sum(len(c) for c in cnts)
    index = [np.zeros(max(1, len(c)), dtype=np.uint32) for c in cnts]
    pp = (C.c_void_p * max(1, n))(*[p.ctypes.data if p.size else None for p in pats])
    cp = (C.c_void_p * max(1, n))(*[c.ctypes.data if len(c) else None for c in cnts])
    ip = (C.c_void_p * max(1, n))(*[i.ctypes.data for i in index])
    strides = np.full(max(1, n), max(vp, 1), dtype=np.uint32)
    strides[:n] = [p.shape[1] if p.size else max(vp, 1) for p in pats]
    ng = np.array([len(c) for c in cnts] or [0], dtype=np.uint32)
    mp = np.zeros((max(1, total), max(1, vp)), dtype=np.uint8)
    mc = np.zeros(max(1, total), dtype=np.uint64)
    got = C.c_uint32()
    # merged_patterns is [cap][vp]: contiguous rows of exactly vp bytes
    flat = np.zeros(max(1, total) * max(1, vp), dtype=np.uint8)
    rc = lib.jl_merge_groups(pp, _p(strides), cp, _p(ng), n, vp, _p(flat), _p(mc), max(1, total), C.byref(got), ip)
    if rc:
        raise JulietError(rc, "jl_merge_groups")
    m = got.value
    mp = flat[: m * vp].reshape(m, vp).copy() if vp else np.zeros((m, 0), dtype=np.uint8)
    return mp, mc[:m].astype(np.int64), [i[: len(c)].astype(np.int64) for i, c in zip(index, cnts)]


def select_haplotypes(patterns, counts, variants, pos_cols, min_reads=10, partials=()):
    """jl_select_haplotypes (docs/SPEC.md §8 on merged groups) -> dict like Juliet.phase_fetch (no read_hap) +
    hap_of_merged int64[M] (HAP_INSUFFICIENT where not reported)."""
    lib = load_library()
    patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    m = len(counts)
    vp = len(pos_cols)
    patterns = patterns.reshape(m, vp) if m else np.zeros((0, vp), dtype=np.uint8)
    variants = np.ascontiguousarray(variants, dtype=VARIANT)
    nv = len(variants)
    pc = np.ascontiguousarray(pos_cols, dtype=np.uint32)
    parts = np.zeros(max(1, len(partials)), dtype=SUMMARY)
    for k, p in enumerate(partials):
        for f in ("damaged_reads", "marginal_gap", "marginal_heteroduplex", "marginal_partial"):
            parts[k][f] = int(p[f])
    summ = np.zeros(1, dtype=SUMMARY)
    hap_count = np.zeros(MAX_HAPLOTYPES, dtype=np.uint32)
    hap_pattern = np.zeros((MAX_HAPLOTYPES, max(1, vp)), dtype=np.uint8)
    hcap = max(1, min(MAX_HAPLOTYPES, m))
    hit = np.zeros((max(1, nv), hcap), dtype=np.uint8)
    cooc = np.zeros((max(1, nv), max(1, nv)), dtype=np.uint32)
    hom = np.zeros(max(1, m), dtype=np.uint16)
    flatp = np.ascontiguousarray(patterns).reshape(-1) if patterns.size else np.zeros(1, dtype=np.uint8)
    hp_flat = np.zeros(MAX_HAPLOTYPES * max(1, vp), dtype=np.uint8)
    rc = lib.jl_select_haplotypes(_p(flatp), _p(counts if m else np.zeros(1, dtype=np.uint64)), m, vp,
                                  _p(variants if nv else np.zeros(1, dtype=VARIANT)), nv, _p(pc if vp else np.zeros(1, dtype=np.uint32)),
                                  min_reads, _p(parts), len(partials), _p(summ), _p(hap_count), _p(hp_flat), _p(hit), hcap, _p(cooc), _p(hom))
    if rc:
        raise JulietError(rc, "jl_select_haplotypes")
    s = {k: int(summ[0][k]) for k in SUMMARY_FIELDS}
    h = s["n_haplotypes"]
    hap_of_merged = hom[:m].astype(np.int64)
    return dict(summary=s, hap_count=hap_count[:h].copy(), hap_pattern=hp_flat[: h * vp].reshape(h, vp).copy() if vp else np.zeros((h, 0), dtype=np.uint8),
                hit=hit[:nv, :h].copy(), cooc=cooc[:nv, :nv].copy(), hap_of_merged=hap_of_merged)


def xwin_slice_plan(win_begins, win_ncols, win_rank, merged, slice_begin, world, rank):
    """jl_xwin_slice_plan: the ops of `rank` in issue order, as dicts (op, peer, k_begin, k_count, read_begin, n_reads,
    dst_stride, bytes, dst_offset).  Needs no GPU."""
    lib = load_library()
    merged = np.ascontiguousarray(merged, dtype=VARIANT)
    wb = np.ascontiguousarray(win_begins, dtype=np.uint32)
    wn = np.ascontiguousarray(win_ncols, dtype=np.uint32)
    wr = np.ascontiguousarray(win_rank, dtype=np.int32)
    sb = np.ascontiguousarray(slice_begin, dtype=np.uint64)
    cap = 2 * world + 1
    ops = (XwinOp * cap)()
    n = C.c_uint32()
    rc = lib.jl_xwin_slice_plan(_p(wb), _p(wn), _p(wr), len(wb), _p(merged if len(merged) else np.zeros(1, dtype=VARIANT)), len(merged),
                                _p(sb), world, rank, ops, cap, C.byref(n))
    if rc:
        raise JulietError(rc, "jl_xwin_slice_plan")
    return [{f: getattr(ops[k], f) for f, _ in XwinOp._fields_} for k in range(n.value)]


class Xwin:
    """A cross-window phasing session (jl_xwin_*): this rank's windows of ONE reference whose reads span every window.
    `windows`: this rank's Juliet contexts in ascending column order; `comm`: the RCCL communicator handle (None when every
    window is on this device); `win_begins/win_ncols/win_rank`: the layout of ALL windows; `slice_begin`: world + 1 starts."""

    def __init__(self, windows, win_begins, win_ncols, win_rank, slice_begin, comm=None):
        self.lib = load_library()
        self.windows = list(windows)
        arr = (C.c_void_p * len(self.windows))(*[w.h for w in self.windows])
        wb = np.ascontiguousarray(win_begins, dtype=np.uint32)
        wn = np.ascontiguousarray(win_ncols, dtype=np.uint32)
        wr = np.ascontiguousarray(win_rank, dtype=np.int32)
        sb = np.ascontiguousarray(slice_begin, dtype=np.uint64)
        h = C.c_void_p()
        rc = self.lib.jl_xwin_create(arr, len(self.windows), comm, _p(wb), _p(wn), _p(wr), len(wb), _p(sb), C.byref(h))
        if rc:
            raise JulietError(rc, "jl_xwin_create: bad layout (windows / ranks / slices)")
        self.h = h
        self._res = XwinResult()
        self._res_ref = C.byref(self._res)

    def close(self):
        if getattr(self, "h", None):
            self.lib.jl_xwin_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def phase_raw(self, min_reads=10):
        """One jl_xwin_phase_sharded call; returns the result struct (pointers into the session, no copies)."""
        rc = self.lib.jl_xwin_phase_sharded(self.h, min_reads, self._res_ref)
        if rc:
            raise JulietError(rc, self.lib.jl_xwin_last_error(self.h).decode())
        return self._res

    def phase(self, min_reads=10, want_reads=True):
        """dict like phase_across_windows' (copies): merged table, summary, haplotypes, hit, cooc, pos_cols (global
        columns), read_hap of THIS rank's slice."""
        r = self.phase_raw(min_reads)
        nv, vp, h = r.n_variants, r.n_positions, r.n_haplotypes
        merged = _view(r.merged, VARIANT, nv).copy() if nv else np.zeros(0, dtype=VARIANT)
        out = dict(merged=merged, pos_cols=_view(r.pos_global, np.uint32, vp).copy() if vp else np.zeros(0, dtype=np.uint32),
                   summary={n: getattr(r.summary, n) for n in SUMMARY_FIELDS}, n_groups=r.n_groups,
                   slice=(int(r.slice_begin), int(r.slice_reads)), read_hap_bits=int(r.read_hap_bits))
        if vp:
            out.update(hap_count=_view(r.hap_count, np.uint32, h).copy() if h else np.zeros(0, dtype=np.uint32),
                       hap_pattern=_view(r.hap_pattern, np.uint8, h * vp).reshape(h, vp).copy() if h else np.zeros((0, vp), dtype=np.uint8),
                       hit=_view(r.hit, np.uint8, nv * h).reshape(nv, h).copy() if nv * h else np.zeros((nv, h), dtype=np.uint8),
                       cooc=_view(r.cooc, np.uint32, nv * nv).reshape(nv, nv).copy() if nv else np.zeros((0, 0), dtype=np.uint32))
        if want_reads:
            out["read_hap"] = self.read_hap()
        return out

    STAGES = ("tables on the host", "gather + merge of the tables", "plan", "pack + exchange + grouping enqueued", "wait for the groups",
              "merge + selection", "per-read ids")

    def stage_us(self):
        """Host microseconds of the last phase call by stage (jl_xwin_stage_us)."""
        out = np.zeros(8, dtype=np.float32)
        self.lib.jl_xwin_stage_us(self.h, _p(out))
        return dict(zip(self.STAGES, out.tolist()))

    def read_hap(self):
        n = int(self._res.slice_reads)
        ids = np.zeros(max(1, n), dtype=np.uint16)
        rc = self.lib.jl_xwin_read_hap_fetch(self.h, _p(ids))
        if rc:
            raise JulietError(rc, self.lib.jl_xwin_last_error(self.h).decode())
        return ids[:n]


def phase_across_windows(windows, merged, min_reads=10, comm=None, win_begins=None, win_ncols=None, device=0):
    """Cross-window phasing: `windows` = contexts holding the SAME reads over different column
    windows (all on this device), or a single context plus an RCCL `comm` when every rank owns one window.
    `merged`: all windows' variant rows with GLOBAL columns.  Returns (phase result, global columns of the positions)."""
    merged = np.ascontiguousarray(merged, dtype=VARIANT)
    pc = Juliet(device)
    remapped = np.zeros(max(1, len(merged)), dtype=VARIANT)
    pos_global = np.zeros(max(1, len(merged)), dtype=np.uint32)
    vp = C.c_uint32()
    if comm is None:
        arr = (C.c_void_p * len(windows))(*[w.h for w in windows])
        pc._chk(pc.lib.jl_xwin_assemble_local(pc.h, arr, len(windows), _p(merged), len(merged), _p(remapped), _p(pos_global),
                                              C.byref(vp)))
    else:
        wb = np.ascontiguousarray(win_begins, dtype=np.uint32)
        wn = np.ascontiguousarray(win_ncols, dtype=np.uint32)
        pc._chk(pc.lib.jl_xwin_assemble_rccl(pc.h, windows[0].h, comm, _p(wb), _p(wn), _p(merged), len(merged), _p(remapped),
                                             _p(pos_global), C.byref(vp)))
    if vp.value == 0:
        pc.close()
        return None, pos_global[:0]
    pc._shape(windows[0].n_reads, 3 * vp.value, windows[0].plane_stride)
    pc.phase_async(remapped[: len(merged)], min_reads)
    ph = pc.phase_fetch(want_reads=True, cap_var=max(1, len(merged)))
    ph["hit"] = ph["hit"][: len(merged), : ph["summary"]["n_haplotypes"]].copy()
    if ph["cooc"] is not None:
        ph["cooc"] = ph["cooc"][: len(merged), : len(merged)].copy()
    pc.close()
    return ph, pos_global[: vp.value].copy()


def phase_sharded_by_reads(windows, merged, n_shards, min_reads=10, device=0, want_reads=True):
    """Cross-window phasing with the reads sharded (SURVEY §8e option A), every shard on THIS device — what the ranks of a
    multi-GPU run do, one after the other: slice assembly, grouping + export per shard, merge and selection on the host
    (sharding.merge_groups / select_haplotypes), the ids of every shard from jl_phase_regroup.
    Returns (phase result as phase_across_windows gives it, global columns of the positions)."""
    from . import sharding

    merged = np.ascontiguousarray(merged, dtype=VARIANT)
    n = windows[0].n_reads
    bounds = sharding.read_slices(n, n_shards)
    shards, tables, remapped, pos_global = [], [], None, None
    for s in range(n_shards):
        pc = Juliet(device)
        remapped, pos_global = pc.xwin_assemble_slice_local(windows, merged, bounds[s], bounds[s + 1] - bounds[s])
        if len(pos_global) == 0:
            pc.close()
            for q in shards:
                q.close()
            return None, pos_global
        if bounds[s + 1] > bounds[s]:
            pc.phase_groups_async(remapped)
            tables.append(pc.phase_groups_fetch(cap_var=max(1, len(pos_global))))
        else:   # a rank without reads contributes nothing
            tables.append(dict(patterns=np.zeros((0, len(pos_global)), dtype=np.uint8), counts=np.zeros(0, dtype=np.uint32),
                               pos_cols=3 * np.arange(len(pos_global), dtype=np.uint32),
                               summary={k: 0 for k in SUMMARY_FIELDS}))
        shards.append(pc)
    patterns, counts, index = merge_groups(tables)
    pos_cols = next(t["pos_cols"] for t in tables if len(t["pos_cols"]))
    ph = select_haplotypes(patterns, counts, remapped, pos_cols, min_reads, [t["summary"] for t in tables])
    ids = []
    for s, pc in enumerate(shards):
        if bounds[s + 1] > bounds[s]:
            hap = ph["hap_of_merged"][index[s]].astype(np.uint16)
            r = pc.phase_regroup(hap, ph["summary"]["n_haplotypes"], want_reads)
            if want_reads:
                ids.append(r)
        pc.close()
    ph["read_hap"] = np.concatenate(ids) if want_reads and ids else None
    ph["pos_cols"] = pos_global.copy()
    return ph, pos_global.copy()


class Group:
    """Several resident windows (Juliet contexts of one device) run through the path in three launches
    (jl_group_run_async); results are read from each context as after run_async (run_view / run_fetch)."""

    def __init__(self, ctxs):
        self.lib = load_library()
        self.ctxs = list(ctxs)
        arr = (C.c_void_p * len(self.ctxs))(*[c.h for c in self.ctxs])
        h = C.c_void_p()
        rc = self.lib.jl_group_create(arr, len(self.ctxs), C.byref(h))
        if rc != 0:
            raise JulietError(rc, "jl_group_create failed")
        self.h = h
        self._args = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.jl_group_destroy(self.h)
            self.h = None

    def bind_exchange(self, comm):
        """jl_group_exchange_bind: every run of the group from now on carries the all-gather of its windows' table heads
        (comm: the jl_comm handle, None unbinds).  A collective the first time a communicator is bound."""
        rc = self.lib.jl_group_exchange_bind(self.h, comm)
        if rc:
            raise JulietError(rc, self.lib.jl_group_last_error(self.h).decode())

    def exchange_collect(self, world, cap_rows=128, rows=None, counts=None):
        """jl_group_exchange_collect: the group's oldest pending exchange -> (rows [windows][world][cap_rows] of VARIANT,
        counts [windows][world])."""
        n = len(self.ctxs)
        if rows is None:
            rows = np.zeros(n * world * cap_rows, dtype=VARIANT)
            counts = np.zeros(n * world, dtype=np.uint32)
        rc = self.lib.jl_group_exchange_collect(self.h, rows.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p), cap_rows)
        if rc:
            raise JulietError(rc, self.lib.jl_group_last_error(self.h).decode())
        return rows.reshape(n, world, cap_rows), counts.reshape(n, world)

    def views(self):
        """jl_group_views: the jl_run_view of every window after a group run, ONE call (it waits for each window in turn).
        Returns a numpy record array over the structs (fields complete, n_variants, n_haplotypes, ...), reused between
        calls."""
        if getattr(self, "_views", None) is None:
            self._views = (RunView * len(self.ctxs))()
            self._views_n = C.c_uint32()
            dt = np.dtype(dict(names=["complete", "n_variants", "phased", "n_positions", "n_haplotypes", "n_var_phase"],
                               formats=[np.uint32] * 6, offsets=[0, 4, 8, 12, 16, 20], itemsize=C.sizeof(RunView)))
            self._views_np = np.frombuffer(self._views, dtype=dt)
        rc = self.lib.jl_group_views(self.h, self._views, len(self.ctxs), C.byref(self._views_n))
        if rc:
            raise JulietError(rc, self.lib.jl_group_last_error(self.h).decode())
        return self._views_np

    def run_masked_async(self, genes, refseq, params, drm_masks, phasing=True, min_reads=10, want_read_hap=True):
        """drm_masks: one uint64[P] array (or None) per window (--drm-only, doc/JULIET.md:370)."""
        g = np.ascontiguousarray(genes, dtype=GENE)
        r = None if refseq is None else np.ascontiguousarray(refseq, dtype=np.uint8)
        prm = params or default_params()
        keep = [None if m is None else np.ascontiguousarray(m, dtype=np.uint64) for m in drm_masks]
        arr = (C.c_void_p * len(keep))(*[None if m is None else m.ctypes.data for m in keep])
        rc = self.lib.jl_group_run_masked_async(self.h, _p(g), len(g), _p(r), 0 if r is None else len(r), C.byref(prm), arr,
                                                1 if phasing else 0, min_reads, 1 if want_read_hap else 0)
        if rc:
            raise JulietError(rc, self.lib.jl_group_last_error(self.h).decode())

    def run_async(self, genes, refseq=None, params=None, phasing=True, min_reads=10, want_read_hap=True):
        key = (id(genes), id(refseq), id(params))
        c = self._args
        if c is None or c[0] != key:   # marshalling cached: repeated steps pass the same objects
            g = np.ascontiguousarray(genes, dtype=GENE)
            r = None if refseq is None else np.ascontiguousarray(refseq, dtype=np.uint8)
            prm = params or default_params()
            c = self._args = (key, (genes, refseq, params), (g, r, prm),
                              (_p(g), len(g), _p(r), 0 if r is None else len(r), C.byref(prm)))
        a = c[3]
        rc = self.lib.jl_group_run_async(self.h, a[0], a[1], a[2], a[3], a[4], 1 if phasing else 0, min_reads,
                                         1 if want_read_hap else 0)
        if rc:
            raise JulietError(rc, self.lib.jl_group_last_error(self.h).decode())


def time_pileup_groups(groups, reps=20):
    """(average ms per grouped pileup launch, algorithmic bytes per launch), rotating over the groups
    (jl_group_time_pileup)."""
    arr = (C.c_void_p * len(groups))(*[g.h for g in groups])
    ms, nbytes = C.c_float(), C.c_uint64()
    rc = groups[0].lib.jl_group_time_pileup(arr, len(groups), reps, C.byref(ms), C.byref(nbytes))
    if rc:
        raise JulietError(rc, groups[0].lib.jl_group_last_error(groups[0].h).decode())
    return float(ms.value), int(nbytes.value)


def time_pileup_set(ctxs, reps=20):
    """Average ms per pileup launch over the contexts' windows in rotation (jl_time_pileup_set)."""
    arr = (C.c_void_p * len(ctxs))(*[c.h for c in ctxs])
    ms = C.c_float()
    ctxs[0]._chk(ctxs[0].lib.jl_time_pileup_set(arr, len(ctxs), reps, C.byref(ms)))
    return float(ms.value)


def haplotype_name(h: int) -> str:
    """Haplotype ids `[A-Z]{1}[a-z]?` (doc/JULIET.md:198): A..Z, then Aa..Az, Ba.. (docs/SPEC.md §8)."""
    if h < 26:
        return chr(65 + h)
    h -= 26
    return chr(65 + h // 26) + chr(97 + h % 26)
