"""CPU-side checks of the C-ABI library: it loads, exports every symbol include/juliet_hip.h declares,
its PODs have the documented sizes, and without a GPU it refuses loudly (no CPU fallback).  No compute."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from minorseq_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "juliet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(jl_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    lib = capi.load_library()
    declared = _declared()
    assert len(declared) >= 28
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/juliet_hip.h but not exported"
    assert sorted(capi.EXPORTS) == declared


def test_header_is_the_export_list():
    """-fvisibility=hidden + the header's visibility pragma + csrc/exports.map: the dynamic symbol table of the library
    holds exactly the functions include/juliet_hip.h declares — no internal jl_* helper, no mangled C++ symbol, no kernel
    handle."""
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(line.split()[-1] for line in out.splitlines() if line.strip())
    kinds = {line.split()[-2] for line in out.splitlines() if line.strip()}
    assert exported == _declared()
    assert kinds == {"T"}


def test_pod_layouts():
    assert capi.VARIANT.itemsize == 48          # the all-gather row
    assert capi.GENE.itemsize == 8
    assert capi.SUMMARY.itemsize == 32
    assert C.sizeof(capi.Params) == 64
    lib = capi.load_library()
    assert lib.jl_col_stride(1) == 128 and lib.jl_col_stride(256) == 128 and lib.jl_col_stride(257) == 256
    assert lib.jl_col_stride(100000) == 50048
    # the resident planes: whole 128-byte lines, 1024 reads each; 3 bits per cell
    assert lib.jl_plane_stride(1) == 128 and lib.jl_plane_stride(1024) == 128 and lib.jl_plane_stride(1025) == 256
    assert lib.jl_plane_stride(100000) == 12544 and 3 * 3000 * lib.jl_plane_stride(100000) < 113e6
    assert lib.jl_strerror(0) == b"ok" and b"gfx950" in lib.jl_strerror(-2)


def test_no_cpu_fallback():
    lib = capi.load_library()
    if lib.jl_device_count() > 0:
        pytest.skip("a gfx950 device is present")
    with pytest.raises(capi.JulietError) as e:
        capi.Juliet(0)
    assert e.value.status == -2 and "no CPU fallback" in str(e.value)


def test_haplotype_names():
    # doc/JULIET.md:198  [A-Z]{1}[a-z]?
    names = [capi.haplotype_name(h) for h in range(capi.MAX_HAPLOTYPES)]
    assert names[0] == "A" and names[25] == "Z" and names[26] == "Aa" and names[51] == "Az" and names[52] == "Ba"
    assert names[-1] == "Zz" and len(set(names)) == 702
    assert all(re.fullmatch(r"[A-Z][a-z]?", n) for n in names)


def test_header_is_plain_c_and_links(tmp_path):
    """include/juliet_hip.h is a C header (no C++/torch types): a C99 program compiles against it, links the
    library and runs without a GPU (it only asks for the ABI version and the device count)."""
    import subprocess
    src = tmp_path / "use.c"
    src.write_text('#include <stdio.h>\n#include "juliet_hip.h"\n'
                   'int main(void) {\n'
                   '    jl_params p = {0.01, 0.0, {0.998826, 5.8e-5, 1.0e-3}, 0, 0, -1.0, -1.0};\n'
                   '    jl_ctx *ctx = 0;\n'
                   '    int n = jl_device_count();\n'
                   '    int rc = n ? 0 : jl_ctx_create(0, 0, &ctx);\n'
                   '    printf("%d %d %d %s|%s\\n", jl_abi_version(), n, rc, jl_strerror(rc), jl_last_error(0));\n'
                   '    return (int)(p.alpha > 1.0);\n}\n')
    exe = tmp_path / "use"
    lib_dir = os.path.join(ROOT, "minorseq_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src), "-L" + lib_dir, "-ljuliet_hip", "-Wl,-rpath," + lib_dir,
                           "-Wl,-rpath-link,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    ver, n, rc, msg = out.stdout.strip().split(" ", 3)
    assert ver == "5"
    if n == "0":
        assert rc == "-2" and "no CPU fallback" in msg      # loud failure without a device


C_MERGE = r"""
#include <stdio.h>
#include <string.h>
#include "juliet_hip.h"
/* The host side of phasing sharded by reads, from plain C: two windows' tables -> one; two slices' groups -> the merged
 * groups; the haplotypes of the MERGED counts (doc/JULIET.md:253-254); the schedule of the column-slice exchange. */
int main(void) {
    jl_variant a[2], b[1], merged[3];
    const jl_variant *tabs[2];
    uint32_t cnt[2] = {2, 1}, wb[2] = {0, 300}, n = 0, m = 0, k;
    uint8_t p0[4] = {3, 1, 0, 2}, p1[6] = {0, 2, 3, 1, 3, 0}, mp[10];
    const uint8_t *pats[2];
    uint32_t c0[2] = {4, 6}, c1[3] = {5, 6, 9}, ng[2] = {2, 3}, ps[2] = {2, 2}, i0[2], i1[3];
    const uint32_t *cnts[2];
    uint32_t *idx[2];
    uint64_t mc[5];
    uint32_t pos_cols[2] = {0, 3}, hap_count[702], cooc[4];
    uint8_t hap_pattern[702 * 2], hit[2 * 3];
    uint16_t hom[3];
    jl_phase_summary part[2], sum;
    jl_variant v[2];
    jl_xwin_op ops[5];
    uint32_t wn[2] = {302, 300}, n_ops = 0;
    int32_t wr[2] = {0, 1};
    uint64_t sb[3] = {0, 512, 1000};
    memset(a, 0, sizeof a); memset(b, 0, sizeof b); memset(part, 0, sizeof part); memset(v, 0, sizeof v);
    a[0].gene = 0; a[0].codon_pos = 9; a[0].codon = 7; a[0].col = 24;
    a[1].gene = 0; a[1].codon_pos = 3; a[1].codon = 1; a[1].col = 6;
    b[0].gene = 0; b[0].codon_pos = 104; b[0].codon = 2; b[0].col = 9;
    tabs[0] = a; tabs[1] = b;
    if (jl_merge_tables(tabs, cnt, wb, 2, merged, 3, &n) != JL_OK || n != 3) return 1;
    if (merged[0].col != 6 || merged[1].col != 24 || merged[2].col != 309) return 2;
    if (jl_merge_tables(tabs, cnt, wb, 2, merged, 2, &n) != JL_ERR_OVERFLOW || n != 3) return 3;
    pats[0] = p0; pats[1] = p1; cnts[0] = c0; cnts[1] = c1; idx[0] = i0; idx[1] = i1;
    if (jl_merge_groups(pats, ps, cnts, ng, 2, 2, mp, mc, 5, &m, idx) != JL_OK || m != 3) return 4;
    if (mp[0] != 0 || mp[1] != 2 || mc[0] != 11 || mc[1] != 9 || mc[2] != 10 || i0[0] != 2 || i1[2] != 1) return 5;
    v[0].col = 0; v[0].codon = 3; v[1].col = 3; v[1].codon = 2;
    part[0].damaged_reads = 7; part[1].damaged_reads = 5; part[1].marginal_gap = 2;
    if (jl_select_haplotypes(mp, mc, m, 2, v, 2, pos_cols, 10, part, 2, &sum, hap_count, hap_pattern, hit, 3, cooc, hom) != JL_OK) return 6;
    if (sum.n_haplotypes != 2 || sum.reported_reads != 21 || sum.insufficient_reads != 9 || sum.damaged_reads != 12 || sum.marginal_gap != 2) return 7;
    if (hap_count[0] != 11 || hap_count[1] != 10 || hom[0] != 0 || hom[1] != JL_HAP_INSUFFICIENT || hom[2] != 1) return 8;
    if (hit[0] != 0 || hit[1] != 1 || hit[3] != 1 || hit[4] != 0 || cooc[0] != 10 || cooc[3] != 11 || cooc[1] != 0) return 9;
    /* two ranks, one window each; both positions belong to rank 1's window except column 6 */
    if (jl_xwin_slice_plan(wb, wn, wr, 2, merged, 3, sb, 2, 0, ops, 5, &n_ops) != JL_OK || n_ops != 3) return 10;
    if (ops[0].op != JL_XWIN_OP_LOCAL || ops[1].op != JL_XWIN_OP_SEND || ops[2].op != JL_XWIN_OP_RECV) return 11;
    if (ops[0].k_count != 2 || ops[1].peer != 1 || ops[1].n_reads != 488 || ops[1].dst_stride != 128 || ops[1].bytes != 9 * 2 * 128) return 12;
    if (ops[2].k_begin != 2 || ops[2].k_count != 1 || ops[2].dst_stride != 128 || ops[2].dst_offset != 9 * 2 * 128) return 13;
    for (k = 0; k < n_ops; ++k) printf("%d:%d:%llu ", ops[k].op, ops[k].peer, (unsigned long long)ops[k].bytes);
    printf("\n");
    return 0;
}
"""


def test_merge_and_schedule_from_c99(tmp_path):
    """jl_merge_tables / jl_merge_groups / jl_select_haplotypes / jl_xwin_slice_plan are host-only: a C99 program
    drives them without a GPU and checks the answers."""
    import subprocess
    src = tmp_path / "merge.c"
    src.write_text(C_MERGE)
    exe = tmp_path / "merge"
    lib_dir = os.path.join(ROOT, "minorseq_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src), "-L" + lib_dir, "-ljuliet_hip", "-Wl,-rpath," + lib_dir,
                           "-Wl,-rpath-link,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert out.stdout.strip() == "0:0:2304 1:1:2304 2:1:1152"


# ---------------------------------------------------------------------------------------------- who reads the resident matrix
# Every exported function is in exactly one of three lists.  A stage added later has to be classified here before the suite passes;
# one that reads the resident matrix gets a test in tests/test_gpu_high_rows.py, where the matrix has plane rows on both sides of
# 4 GiB, or a reason why it cannot take that matrix.
READS_MATRIX = {                      # function -> the test of tests/test_gpu_high_rows.py that runs it on the tensor
    "jl_run_async": "test_run_with_phasing", "jl_run_wait": "test_run_with_phasing", "jl_run_done": "test_run_with_phasing",
    "jl_run_view_get": "test_run_with_phasing",
    "jl_pileup_async": "test_stage_api_pileup_call_phase", "jl_pileup_fetch": "test_stage_api_pileup_call_phase",
    "jl_consensus_fetch": "test_stage_api_pileup_call_phase", "jl_call_async": "test_stage_api_pileup_call_phase",
    "jl_call_fetch": "test_stage_api_pileup_call_phase", "jl_phase_async": "test_stage_api_pileup_call_phase",
    "jl_phase_fetch": "test_stage_api_pileup_call_phase", "jl_n_positions": "test_stage_api_pileup_call_phase",
    "jl_pileup_kernel_name": "test_run_with_phasing",
    "jl_control_call_async": "test_control_call", "jl_control_call_fetch": "test_control_call",
    "jl_class_pileup_async": "test_class_pileup_and_consensus", "jl_class_pileup_fetch": "test_class_pileup_and_consensus",
    "jl_class_codons_async": "test_class_codons", "jl_class_codons_fetch": "test_class_codons",
    "jl_codon_deletions_async": "test_codon_deletions", "jl_codon_deletions_fetch": "test_codon_deletions",
    "jl_deletion_alleles_async": "test_deletion_alleles", "jl_deletion_alleles_fetch": "test_deletion_alleles",
    "jl_sites_assemble": "test_sites_assemble",
    "jl_variant_linkage_async": "test_variant_linkage", "jl_variant_linkage_fetch": "test_variant_linkage",
    "jl_phase_rescue_async": "test_rescue", "jl_phase_rescue_fetch": "test_rescue",
    "jl_phase_nearest_async": "test_nearest", "jl_phase_nearest_fetch": "test_nearest",
    "jl_phase_recombinants_async": "test_recombinant", "jl_phase_recombinants_fetch": "test_recombinant",
    "jl_read_stats_async": "test_read_stats", "jl_read_stats_fetch": "test_read_stats",
    "jl_read_hypermut_async": "test_read_hypermut", "jl_read_hypermut_fetch": "test_read_hypermut",
    "jl_read_orf_async": "test_read_orf", "jl_read_orf_fetch": "test_read_orf",
    "jl_msa_take": "test_take", "jl_msa_take_async": "test_take",
    "jl_msa_download": "test_download",
    "jl_msa_adopt": "test_a_plane_stride_of_4_gib_is_refused",
    "jl_xwin_assemble_slice_local": "test_cross_window_pack_and_session",
    "jl_xwin_create": "test_cross_window_pack_and_session", "jl_xwin_phase_sharded": "test_cross_window_pack_and_session",
    "jl_xwin_read_hap_fetch": "test_cross_window_pack_and_session", "jl_xwin_destroy": "test_cross_window_pack_and_session",
}
READS_MATRIX_NOT_ON_THE_TENSOR = {    # function -> why tests/test_gpu_high_rows.py does not run it
    "jl_msa_index_info": "an adopted matrix is never indexed (test_gpu_deviation_index.test_adopted_matrix_is_never_indexed)",
    "jl_msa_download_planes": "one hipMemcpy of the whole allocation, no kernel and no row offset",
    "jl_group_run_async": "the kernels of jl_run_async, launched for several contexts",
    "jl_group_run_masked_async": "the kernels of jl_run_async, launched for several contexts",
    "jl_group_time_pileup": "the pileup of jl_run_async in a timing loop", "jl_time_pileup": "the pileup of jl_run_async in a timing loop",
    "jl_time_pileup_set": "the pileup of jl_run_async in a timing loop", "jl_time_run": "jl_run_async in a timing loop",
    "jl_sites_assemble_alleles": "its source is a record build (the insertion events), which is never adopted",
    "jl_xwin_assemble_local": "the pack kernel of jl_xwin_assemble_slice_local with whole columns at the windows' stride",
    "jl_xwin_assemble_rccl": "the pack kernel of the local assembly; needs a communicator",
    "jl_xwin_assemble_slice_rccl": "the pack kernel of the local assembly; needs a communicator",
    "jl_phase_groups_async": "the key and grouping kernels of jl_phase_async over a slice", "jl_phase_groups_fetch": "fetch of the former",
    "jl_phase_regroup": "reads the keys of jl_phase_groups_async, not the matrix rows by offset of its own",
    "jl_insertions_fetch": "counters of a record build", "jl_insertion_alleles_fetch": "counters of a record build",
    "jl_insertion_reads_fetch": "events of a record build",
}
READS_NO_MATRIX = [
    "jl_abi_version", "jl_allgather_groups", "jl_allgather_variants", "jl_allgather_variants_async", "jl_allgather_variants_async_many",
    "jl_allgather_variants_many", "jl_col_stride", "jl_comm_create", "jl_comm_create_inproc", "jl_comm_destroy", "jl_comm_info",
    "jl_comm_unique_id", "jl_consensus_of_counts", "jl_control_eval", "jl_control_test", "jl_ctx_create", "jl_ctx_destroy", "jl_ctx_stream",
    "jl_deletion_allele_test", "jl_deletion_test", "jl_device_count", "jl_expand_read_hap", "jl_fisher_eval", "jl_fisher_eval_tail",
    "jl_group_create", "jl_group_destroy", "jl_group_exchange_bind", "jl_group_exchange_collect", "jl_group_last_error", "jl_group_views",
    "jl_haplotype_recombinants", "jl_hypermut_eval", "jl_hypermut_filter", "jl_hypermut_test", "jl_insertion_test", "jl_last_error",
    "jl_linkage_stats", "jl_merge_groups", "jl_merge_tables", "jl_mix_counts", "jl_orf_classify", "jl_orf_filter", "jl_plane_stride",
    "jl_qmask_bytes", "jl_qmask_from_quals", "jl_read_filter", "jl_run_pileup_clock", "jl_run_pileup_ms", "jl_sample_reads",
    "jl_select_haplotypes", "jl_strerror", "jl_sync", "jl_variant_table_device", "jl_xwin_last_error", "jl_xwin_plan", "jl_xwin_slice_plan",
    "jl_xwin_stage_us",
    # producers: they write the resident matrix and read none
    "jl_msa_alloc", "jl_msa_upload", "jl_msa_pack_rows", "jl_msa_ingest_records", "jl_msa_ingest_records_masked", "jl_msa_track_insertions",
    "jl_msa_track_insertion_alleles", "jl_msa_track_insertion_reads", "jl_records_begin", "jl_records_append", "jl_records_append_masked",
    "jl_records_finish", "jl_records_drop", "jl_records_window", "jl_records_window_async", "jl_synth_fill", "jl_synth_fill_window",
]


def test_every_export_is_classified_as_a_reader_of_the_matrix_or_not():
    lists = [list(READS_MATRIX), list(READS_MATRIX_NOT_ON_THE_TENSOR), READS_NO_MATRIX]
    everything = [name for lst in lists for name in lst]
    assert len(everything) == len(set(everything)), sorted(n for n in set(everything) if everything.count(n) > 1)
    declared = _declared()
    assert sorted(everything) == declared, (sorted(set(declared) - set(everything)), sorted(set(everything) - set(declared)))
    text = open(os.path.join(ROOT, "tests", "test_gpu_high_rows.py")).read()
    defined = set(re.findall(r"^def (test_[a-z0-9_]+)\(", text, flags=re.M))
    assert set(READS_MATRIX.values()) <= defined, sorted(set(READS_MATRIX.values()) - defined)
    assert all(reason for reason in READS_MATRIX_NOT_ON_THE_TENSOR.values())
