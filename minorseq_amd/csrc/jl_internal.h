// jl_internal.h — private to libjuliet_hip.so: context layout, launch helpers, kernel entry points.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/juliet_hip.h"
#include "deviation_index.h"
#include "jl_synth.h"

// The environment: the library reads these four switches and no other, each once (jl_env, kernels_util.hip).
//   JL_NO_GRAPH                eager launches, no captured graphs: a debugging aid
//   JL_EXCHANGE_STAGED=1       the all-gather's staged form (tests/test_gpu_parity.py)
// The fold = the Fisher stage in the pileup launch's epilogue ("fold", "folded", "unfolded" mean nothing else in the library):
//   JL_NO_FOLD_CALL            the separate call launch always, never the folded Fisher stage: A/B of the fold
//                              (group runs choose between the two per launch otherwise: capi_group.hip)
// Inline ids = the phasing launch writing the per-read ids itself (JL_INLINE_IDS_MAX_BLOCKS below):
//   JL_FORCE_IDS_WAIT_TIMEOUT  test hook of the -DJL_TUNING build (tools_tuning/build_tuning_lib.sh): such a launch gives up waiting at
//                              once (test_fold_timeout_is_rerun_unfolded).  JL_TUNING adds five read-outs besides (capi_group.hip, kernels_pileup.hip) and
//                              the shape override of the per-read counters (jl_tuning_read_stats_shape, capi_readstats.hip), nothing else.
struct jl_env_switches {
    bool no_fold_call, no_graph, exchange_staged, force_ids_wait_timeout;
};
const jl_env_switches &jl_env();

#define JL_VARIANT_CAP 4096u      // rows of the resident variant table (all-gather stride)
#define JL_CAND_CAP 4096u         // haplotype candidates (groups with >= min_reads) the selector can rank
#define JL_POS_PER_WORD 10u       // variant positions per 64-bit key word (6 bits each)
// Largest phase launch whose workgroups may wait for each other inside the launch (the per-read ids are then written by
// the same launch, "inline ids"): all of them must be resident at once, next to as many more such launches as queues run at a time.
// 1536 places on the chip (75 VGPRs, 20.5 KB LDS per block); 128 leaves room for eight concurrent launches and more.
#ifndef JL_INLINE_IDS_MAX_BLOCKS
#define JL_INLINE_IDS_MAX_BLOCKS 128u
#endif
#define JL_INS_LEN_BINS 32u        // insertion lengths 0..30 by value, 31 = longer
#define JL_INS_MAX_BASES 30u       // inserted bases tracked per insertion
#define JL_GUESS_PAD 32u           // zero bytes after the last column's seed base


// resolved reference codon per position
#define JL_REF_MAJORITY 0xFFu
#define JL_REF_SKIP 0xFEu

constexpr uint32_t JL_PHASE_OVF_CANDIDATES = 1u;     // more than JL_CAND_CAP haplotype candidates
constexpr uint32_t JL_PHASE_OVF_HAPLOTYPES = 2u;     // more than JL_MAX_HAPLOTYPES qualified
constexpr uint32_t JL_PHASE_OVF_KEY_WORDS = 4u;      // the key buffer was too small for vp_true positions
constexpr uint32_t JL_PHASE_OVF_FORM = 8u;           // more positions, or a larger result, than the fused launch in use covers
constexpr uint32_t JL_PHASE_OVF_EXPORT = 16u;        // an exporting run found more groups than its block holds
constexpr uint32_t JL_PHASE_OVF_IDS_WAIT_TIMEOUT = 32u;  // a workgroup of a launch with inline ids gave up waiting: some reads have no id
struct jl_phase_meta {  // device-resident scalars of one phasing run
    uint32_t n_var;     // rows used
    uint32_t vp;        // distinct variant columns
    uint32_t kwords;    // 64-bit words per read key
    uint32_t n_occupied;
    uint32_t overflow;  // JL_PHASE_OVF_* (KEY_WORDS, FORM: phasing was skipped, the fetch calls re-run it with what it needs)
    uint32_t vp_true;   // distinct variant columns before the capacity check
    uint32_t id_bits;   // width of the per-read ids the run wrote: 4, 8 or 16 (see JL_ID_* below)
    uint32_t pad_;
    jl_phase_summary summary;
};

// Per-read haplotype ids travel in the narrowest code that holds the run's haplotype count H (they cross PCIe into
// pinned host memory: 2 bytes per read were the largest transfer of a step):
//   4 bits (H <= 14): 0..13 haplotype, 14 insufficient coverage, 15 damaged; read i in nibble i & 7 of dword i >> 3
//   8 bits (H <= 254): 0..253, 254 insufficient, 255 damaged
//   16 bits: the id itself (JL_HAP_INSUFFICIENT / JL_HAP_DAMAGED)
// jl_phase_fetch expands to 16 bits; jl_run_view hands out the packed form with its width.
#define JL_ID4_MAX_H 14u
#define JL_ID8_MAX_H 254u

// Small fixed-size result block: everything a typical run returns except the per-read ids, gathered by one
// tiny kernel so that ONE device-to-host copy into pinned memory ends the step (results that do not fit set
// fits_* = 0 and the fetch calls fall back to their piecewise copies).
#define JL_PACK_MAX_VAR 128u
#define JL_PACK_MAX_VP 128u
#define JL_PACK_MAX_HAP 128u
#define JL_PACK_PATTERN_BYTES 8192u   // e.g. 128 haplotypes x 64 positions
#define JL_PACK_HIT_BYTES 16384u      // e.g. 128 variants x 128 haplotypes
#define JL_SEL_HIT_BYTES 8192u        // what the selection out of LDS holds of it (larger results take the general path)
#define JL_PACK_COOC_N 64u
#define JL_PACK_MAGIC 0x4A4C504Bu
struct jl_pack {
    uint32_t magic, nvar_total, fits_call, fits_phase;
    uint32_t phase_ran, overflow, vp, H;
    jl_phase_summary summary;
    uint32_t nv_phase, cooc_fits, id_bits, pad_[5];
    jl_variant variants[JL_PACK_MAX_VAR];
    uint32_t pos_cols[JL_PACK_MAX_VP];
    uint32_t hap_count[JL_PACK_MAX_HAP];
    uint8_t hap_pattern[JL_PACK_PATTERN_BYTES];  // [H][vp]
    uint8_t hit[JL_PACK_HIT_BYTES];              // [nv][H]
    uint32_t cooc[JL_PACK_COOC_N * JL_PACK_COOC_N];  // [nv][nv]
};

// bytes of jl_pack up to and including variants[]: what one rank contributes to the compact all-gather
#define JL_PACK_HEAD_BYTES (offsetof(jl_pack, pos_cols))

// ---- per-window argument blocks of the three stage kernels.  A single run passes one by value; a group run
// (jl_group_run_async) keeps an array of them in device memory and launches each stage ONCE for all windows
// (blockIdx.z = window).  `n_blocks` = workgroups of the window's own grid (the arrival counters count to it).
// Pointers that a kernel loads from an argument block in memory are "generic" to the compiler, which then emits flat
// loads (they count on two wait counters at once, so no wait on them can be an exact count and a register prefetch
// overlaps nothing).  The streaming code therefore takes pointers typed as global memory (address space 1).
#if defined(__HIP_DEVICE_COMPILE__)
#define JL_AS1 __attribute__((address_space(1)))
#else
#define JL_AS1
#endif

struct jl_call_args {
    double alpha, n_tests, match, substitution, min_perc, max_perc;
    int32_t expected_round;
    uint32_t P;
    int32_t tail;   // 0 one-sided greater, 1 two-sided
    uint32_t pad_;
};

struct jl_win_pileup {
    const uint8_t *msa;          // the window's bit planes
    uint64_t plane_stride;       // bytes per plane
    uint32_t n_cols, n_tiles, n_chunks, pad_;
    const uint2 *chunks;
    const uint32_t *guess32;
    uint32_t *counts, *hist;
};

struct jl_win_call {   // call_kernel: the Fisher stage from histograms in HBM (stage API, windows too deep for one block per chunk)
    jl_call_args A;
    const uint32_t *pos_gene, *pos_codon, *pos_col;
    const uint8_t *pos_refcfg;
    const uint32_t *hist;
    const uint64_t *drm;
    uint64_t *called;
    jl_variant *staged;
    jl_phase_meta *meta;   // run counters to zero (null: none)
    uint32_t n_blocks, pad_;
};

// compact_kernel: ordered compaction of the staged rows into the variant table, then optionally the phasing plan
// (multi-word pipeline, stage API) and / or the result block of a run without phasing
struct jl_win_compact {
    uint32_t P, cap, n_cols, kwords_cap;
    const uint64_t *called;
    const jl_variant *staged;
    jl_variant *rows;
    uint32_t *n_rows;
    uint8_t *varcol;
    uint32_t *vpcols, *col2pos;
    jl_phase_meta *meta;
    uint32_t plan, fast_only;        // plan != 0: distinct variant columns (phase_plan.h)
    uint32_t pack, pad_;             // pack != 0: write the result block (run without phasing)
    jl_pack *pk, *mirror;
    uint32_t *seq_dev;
    volatile uint32_t *seq_host;     // non-null: this launch ends a run
    uint8_t *xhead;                  // bound exchange: see jl_select_args
};

constexpr uint32_t JL_IDS_SEPARATE = 0u;   // jl_select_args::ids_mode: a launch of their own (phase_assign(_group)_kernel) writes the ids
constexpr uint32_t JL_IDS_INLINE = 1u;     // this launch does
#ifdef JL_TUNING
constexpr uint32_t JL_IDS_INLINE_GIVE_UP = 2u;   // ... and its waiting workgroups give up at once (JL_FORCE_IDS_WAIT_TIMEOUT)
#endif
// what the last block of the fused phase launch needs to run the selection (and to end the run)
struct jl_select_args {
    uint32_t run;  // 0: the generic (multi-word) pipeline follows with its own select launch
    uint32_t min_reads, n_cols, cooc_cap;
    uint32_t *slot_hap;
    const jl_variant *variants;
    const uint32_t *col2pos;
    uint32_t *hap_count;
    uint8_t *hap_pattern;
    uint8_t *hit;
    const uint32_t *n_rows;
    uint32_t *cooc;
    jl_pack *pk, *mirror;
    uint32_t *arrive;
    uint32_t *seq_dev;
    volatile uint32_t *seq_host;
    // not JL_IDS_SEPARATE: the per-read ids are written by this launch too (all its workgroups are resident together): the
    // other workgroups wait for the selection on `flag`, then map their own reads
    uint32_t ids_mode, pad_;
    uint32_t *flag, *arrive2;
    uint16_t *read_hap;
    // plan from the call masks (whole-path runs): every workgroup derives the variant columns itself, one extra
    // workgroup compacts the rows into the table meanwhile
    const uint64_t *called;          // null: the plan is in meta / vpcols already (stage API, multi-word pipeline)
    const jl_variant *staged;
    const uint32_t *pos_col;
    jl_variant *rows;
    uint32_t *n_rows_out, *vpcols_out, *col2pos_out;
    uint32_t P, cap, kwords_cap, pad2_;
    // export (phasing sharded by reads, SURVEY §8e option A): instead of ranking the groups of THIS matrix the
    // selection writes them out — count and pattern of every occupied slot, in the order of the occupied list — for the
    // host to merge with the other ranks' (jl_phase_groups_fetch); the per-read ids follow in jl_phase_regroup
    uint32_t *exp_count;             // null: normal selection
    uint8_t *exp_pattern;            // [exp_cap][exp_stride]
    uint32_t exp_cap, exp_stride;
    uint32_t *exp_head;              // optional: [JL_EXP_HEAD_WORDS] what a merge needs of the run's scalars (jl_exp_head)
    // bound exchange (jl_group_exchange_bind): where the head of the result block goes a third time — this rank's part of the
    // region the all-gather of the launch works in (pinned host memory, or its device stage).  Null: none.
    uint8_t *xhead;
};

// head of an exported group table: the block's first words when it travels (pinned host memory, or the all-gather)
struct jl_exp_head {
    uint32_t n_groups, vp, overflow;   // overflow != 0: more groups than the block holds (n_groups = the number needed)
    uint32_t damaged, gap, heteroduplex, partial, clean;   // the slice's read categories (clean = in some group)
};
#define JL_EXP_HEAD_WORDS 8u

// The fused phase launch reading its variant columns where they lie (a session whose positions are all in windows of this
// device: no compact matrix, no pack launch, no plan kernel in front).  Position p = nine plane rows (three columns x three
// planes) of `stride` bytes starting at col[p] (already offset to the byte of the slice's first read); vp travels by value.
struct jl_direct_cols {
    const uint8_t *col[JL_POS_PER_WORD];
    uint64_t stride;
    uint32_t on, vp;
};

// The fused phase launch for 11..20 variant positions (two key words): every read's pattern is grouped in three rounds of
// the one-word machinery — its first word numbered in table A, its second word in table B, the PAIR of those numbers
// (one 64-bit word again) in the main table.  Exact by construction: equal pairs <=> equal words <=> equal patterns.
// The half-key tables only number their keys: no counts, no representatives.
struct jl_two_word {
    unsigned long long *key_a, *key_b;   // [table slots] each, emptied after every run
    uint32_t *occ_a, *occ_b;             // the slots a run touched
    uint32_t *n_occ;                     // [2] how many
};

struct jl_done_ent {   // completion word of one window (see done_kernel)
    uint32_t *seq_dev;
    volatile uint32_t *seq_host;
};

struct jl_win_phase {
    const uint8_t *msa;
    uint64_t col_stride, n_reads, reads_pad;
    const uint32_t *vpcols;
    jl_phase_meta *meta;
    uint64_t *keys;
    uint32_t *flagw;
    uint64_t slots_mask;
    unsigned long long *slot_key;
    uint32_t *slot_rep, *slot_count, *occupied, *read_slot;
    uint32_t *blockcat;
    jl_select_args S;
    uint32_t n_blocks, pad_;
};

// Group launches take the argument blocks of their (at most JL_GROUP_MAX) windows BY VALUE, i.e. in the kernel-argument
// segment: pointers loaded from there are known to be global ones, while pointers loaded from a table in device memory
// are generic to the compiler and every access through them becomes a flat access (slower, and never waited for with
// an exact count).
#define JL_GROUP_MAX 8           // windows per call / phase / id launch (their argument blocks are 250-350 bytes each)
#define JL_GROUP_WINDOWS_MAX 32  // windows per group = per pileup launch (56-byte argument blocks)
struct jl_call_group_args { jl_win_call w[JL_GROUP_MAX]; };
struct jl_compact_group_args { jl_win_compact w[JL_GROUP_MAX]; };
struct jl_phase_group_args { jl_win_phase w[JL_GROUP_MAX]; };
struct jl_pileup_group_args { jl_win_pileup w[JL_GROUP_WINDOWS_MAX]; };
// a window counted from its deviation index (deviation_index.h; kernels_pileup.hip pileup_index_body): one workgroup per plain chunk
struct jl_win_index {
    const uint8_t *msa;          // the planes: a plain chunk over the density bound is still counted from them
    uint64_t plane_stride;
    uint32_t n_reads, n_plain;   // n_plain = workgroups of the window's own grid
    const uint4 *tab;            // [n_plain] {first column, first entry, entries (all ones: not indexed), -}
    const jl_ix_stored_t *entries;   // 16-bit stored entries; tab[].y counts in entries
    const uint8_t *seed;         // [n_cols] the index seed
    uint32_t *counts, *hist;
};
struct jl_index_group_args { jl_win_index w[JL_GROUP_MAX]; };
// the Fisher stage of a window, evaluated by the pileup workgroup that counted the codon (one workgroup per chunk): the call
// stage's own argument block + the positions by column
struct jl_win_fold {
    jl_win_call c;
    const uint32_t *col_head, *pos_next;
};
struct jl_pileup_fold_group_args { jl_win_pileup w[JL_GROUP_MAX]; jl_win_fold f[JL_GROUP_MAX]; };
struct jl_index_fold_group_args { jl_win_index w[JL_GROUP_MAX]; jl_win_fold f[JL_GROUP_MAX]; };

// exchange: the heads of the result blocks of up to JL_GATHER_MAX windows copied next to each other (one send buffer,
// one all-gather for the launch)
#define JL_GATHER_MAX 32
struct jl_gather_args { const uint8_t *src[JL_GATHER_MAX]; };
void jl_launch_gather_heads(const uint8_t *const *srcs, uint32_t n, uint8_t *dst, hipStream_t st);
void jl_launch_heads_to_host(const uint8_t *d_region, uint8_t *h_region, uint32_t n_heads, hipStream_t st);

struct jl_comm;

// ---- cross-window phasing with the reads sharded (kernels_xwin.hip)
#define JL_XW_POS_MAX 48u    // owned variant positions per pack launch
#define JL_XW_DST_MAX 8u     // destination ranks per pack launch
#define JL_XW_TAB_MAX 1024u  // exported groups whose haplotypes travel in the kernel arguments
struct jl_xw_pack_args {
    const uint8_t *src[JL_XW_POS_MAX];   // plane 0 of the first column of each owned position in its window, at read 0
    uint64_t src_stride;                 // plane stride of the windows
    uint32_t n_pos, n_dst;
    // dst: where the first plane row of this launch goes; byte_begin / bytes: the slice within a plane row (8 reads a byte);
    // tail_mask: the bits of the slice's last byte that are its reads (0xFF: all eight)
    struct { uint8_t *dst; uint64_t dst_stride, byte_begin, bytes; uint32_t tail_mask, pad_; } d[JL_XW_DST_MAX];
    // the compact matrix's phasing plan, written by the first launch of a step (meta == null: not by this one)
    jl_phase_meta *meta;
    uint32_t *vpcols, *col2pos;
    uint32_t vp_total, kwords, n_var, pad_;
};
struct jl_xw_assign_args {
    uint64_t n_dwords;
    const uint32_t *flagw, *read_slot, *slot_hap;
    uint16_t *read_hap;
    uint32_t n_groups, bits, phased, pad_;
    uint32_t *arrive, *seq_dev;
    volatile uint32_t *seq_host;     // null: no completion word
};
struct jl_xw_hap_table { uint16_t h[JL_XW_TAB_MAX]; };
void jl_launch_xw_pack(const jl_xw_pack_args *a, hipStream_t st);
void jl_launch_xw_assign(const jl_xw_assign_args *a, const uint16_t *host_tab, const uint16_t *d_tab, hipStream_t st);
void jl_launch_xw_fetch(const void *d_src, void *h_dst, uint64_t bytes, uint32_t *arrive, uint32_t *seq_dev, volatile uint32_t *seq_host,
                        hipStream_t st);

// ---- a matrix of chosen reads of other matrices (kernels_take.hip, capi_take.hip)
struct jl_take_src {
    const uint8_t *base;   // the source's planes
    uint32_t stride;       // ... and its plane stride (its own: an adopted matrix may have any)
    uint32_t pad_;
    uint64_t begin;        // the part's first destination read
};
struct jl_take_args {
    jl_take_src part[JL_TAKE_MAX_PARTS];
    uint32_t n_parts, n_cols;
    uint64_t n_total;      // destination reads: the parts' sum
    const uint32_t *idx;   // [n_total] the parts' indices one after the other, each into its own source
    uint8_t *dst;
    uint64_t dst_stride;   // whole 128-byte lines: jl_plane_stride(n_total)
};
void jl_launch_take(const jl_take_args *a, hipStream_t st);

// ---- column pileup by class of reads (kernels_class.hip, capi_class.hip)
struct jl_class_args {
    const uint8_t *msa;        // the window's bit planes
    uint64_t plane_stride;     // ... and their stride (an adopted matrix brings its own)
    uint64_t n_reads;
    uint32_t n_cols, n_classes;
    const uint16_t *label;     // [n_reads]
    uint8_t *mask;             // [n_classes][mask_stride] one row per class in the plane-row layout
    uint64_t mask_stride;      // jl_plane_stride(n_reads): whole 128-byte lines, whatever plane_stride is
    uint32_t *counts;          // [n_classes][n_cols][6], zeroed
    uint32_t *class_reads;     // [n_classes], zeroed
    uint32_t seg_tiles;        // tiles of 512 reads a workgroup of the counting walks (set by the launcher, as is:)
    uint32_t k_first;          // first class of the counting launch's pass 0
};
void jl_launch_class_pileup(const jl_class_args *a, hipStream_t st);
void jl_launch_class_masks(const jl_class_args *a, hipStream_t st);   // its first step alone: mask rows and class_reads

// ---- codon histograms by class of reads at chosen codon starts (kernels_class_codons.hip, capi_class_codons.hip; docs/SPEC.md §24)
struct jl_class_codons_args {
    const uint8_t *msa;        // the window's bit planes
    uint64_t plane_stride;     // ... and their stride (an adopted matrix brings its own)
    uint64_t n_reads;
    uint32_t n_pos, n_classes;
    const uint32_t *col;       // [n_pos] codon starts, strictly ascending, each + 2 < n_cols
    const uint16_t *label;     // [n_reads]
    const uint8_t *mask;       // [n_classes][mask_stride]: the rows of jl_launch_class_masks
    uint64_t mask_stride;      // jl_plane_stride(n_reads)
    uint32_t *hist;            // [n_classes][n_pos][64], zeroed
    uint32_t seg_tiles;        // tiles of 512 reads a workgroup walks (set by the launcher, as is:)
    uint32_t k_first;          // first class of the launch's pass 0
};
void jl_launch_class_codons(const jl_class_codons_args *a, hipStream_t st);

// ---- which reported haplotype a read agrees with (kernels_rescue.hip, capi_rescue.hip; docs/SPEC.md §14)
#define JL_RESCUE_POS_MAX JL_VARIANT_CAP   // variant positions of one call: the variant table's capacity
#define JL_RESCUE_HAP_PAD 704u             // JL_MAX_HAPLOTYPES in whole chunks of 64 (a lane owns a haplotype)
struct jl_rescue_args {
    const uint8_t *msa;        // the window's bit planes
    uint64_t plane_stride;     // ... and their stride (an adopted matrix brings its own)
    uint64_t n_reads;
    uint32_t n_runs;           // runs of 64 reads: ceil(n_reads / 64); 8 (n_runs) <= plane_stride
    uint32_t n_pos, n_hap, min_positions;
    uint32_t hap_pad, pad_;    // n_hap in whole chunks of 64
    const uint32_t *pos_cols;  // [n_pos], each + 2 < n_cols
    const uint32_t *pat4;      // [ceil(n_pos / 4)][hap_pad]: the packed pattern (jl_pack_pat4, hap_stage.h)
    uint16_t *rescue;          // [n_reads]
    uint32_t *hap_reads;       // [n_hap], zeroed
    unsigned long long *tally; // [4] assigned, ambiguous, none, uninformative; zeroed
};
void jl_launch_phase_rescue(const jl_rescue_args *a, hipStream_t st);

// ---- which reported haplotype a read is nearest to, within a mismatch budget (kernels_nearest.hip, capi_nearest.hip; docs/SPEC.md §22)
// positions and haplotypes are bounded as the rescue's (JL_RESCUE_POS_MAX, JL_RESCUE_HAP_PAD); the walk is shared: hap_walk.h
#define JL_NEAREST_HIST_WORDS (JL_RESCUE_HAP_PAD * (JL_NEAREST_MAX_DISTANCE + 1u))   // hap_reads at its largest: [704][8]
struct jl_nearest_args {
    const uint8_t *msa;        // the window's bit planes
    uint64_t plane_stride;     // ... and their stride (an adopted matrix brings its own)
    uint64_t n_reads;
    uint32_t n_runs;           // runs of 64 reads: ceil(n_reads / 64); 8 (n_runs) <= plane_stride
    uint32_t n_pos, n_hap, min_positions;
    uint32_t hap_pad;          // n_hap in whole chunks of 64
    uint32_t max_distance;     // D <= JL_NEAREST_MAX_DISTANCE
    const uint32_t *pos_cols;  // [n_pos], each + 2 < n_cols
    const uint32_t *pat4;      // [ceil(n_pos / 4)][hap_pad]: the packed pattern (jl_pack_pat4, hap_stage.h)
    uint16_t *nearest;         // [n_reads]
    uint8_t *dist;             // [n_reads]
    uint32_t *hap_reads;       // [n_hap][D + 1], zeroed
    unsigned long long *tally; // [4] assigned, ambiguous, none, uninformative; zeroed
};
void jl_launch_phase_nearest(const jl_nearest_args *a, hipStream_t st);

// ---- which reads are recombinants of two reported haplotypes (kernels_recomb.hip, capi_recomb.hip; docs/SPEC.md §23)
// positions and haplotypes are bounded as the rescue's (JL_RESCUE_POS_MAX, JL_RESCUE_HAP_PAD); the walk is shared: hap_walk.h.  The second
// direction walks the positions from the last to the first, and gets its own copy of both in that order
#define JL_RECOMB_HIST_WORDS (JL_RESCUE_HAP_PAD * 2u)   // parent_reads at its largest: [704][2]
struct jl_recomb_args {
    const uint8_t *msa;        // the window's bit planes
    uint64_t plane_stride;     // ... and their stride (an adopted matrix brings its own)
    uint64_t n_reads;
    uint32_t n_runs;           // runs of 64 reads: ceil(n_reads / 64); 8 (n_runs) <= plane_stride
    uint32_t n_pos, n_hap, min_positions;
    uint32_t hap_pad, pad_;    // n_hap in whole chunks of 64
    const uint32_t *pos_cols[2];  // [n_pos], each + 2 < n_cols: [0] ascending, [1] the same descending
    const uint32_t *pat4[2];      // [ceil(n_pos / 4)][hap_pad] (jl_pack_pat4, hap_stage.h): [0] of pattern, [1] of pattern with every row reversed
    uint16_t *left, *right;    // [n_reads] each
    uint16_t *prefix, *suffix; // [n_reads] each
    uint32_t *parent_reads;    // [n_hap][2], zeroed
    unsigned long long *tally; // [5] recombinant, ambiguous_parent, whole, none, uninformative; zeroed
};
void jl_launch_phase_recombinants(const jl_recomb_args *a, hipStream_t st);

// ---- pairwise linkage of variants over every read covering both (kernels_link.hip, capi_link.hip; docs/SPEC.md §15)
#define JL_LINK_TILE 8u                    // rows of a wave's tile side: 8 x 8 pairs in the registers of every lane
#define JL_LINK_BLOCK_TILE 16u             // ... and of a workgroup's: four waves, 2 x 2 wave tiles
#define JL_LINK_SPLIT_WORDS 256u           // smallest run of words (32 reads each) a workgroup takes of a row: four rounds a lane
struct jl_link_args {
    const uint8_t *msa;        // the window's bit planes
    uint64_t plane_stride;     // ... and their stride (an adopted matrix brings its own)
    uint64_t n_reads;
    uint32_t n_pos, n_var;
    uint32_t n_words;          // words of a row that hold reads: ceil(n_reads / 32)
    uint32_t row_words;        // words of a row: jl_plane_stride(n_reads) / 4, whole 128-byte lines, >= n_words
    uint32_t split_words;      // words of a row a workgroup of the product takes: a multiple of 64
    uint32_t n_splits;         // ceil(n_words / split_words)
    const uint32_t *pos_cols;  // [n_pos], each + 2 < n_cols
    const uint32_t *var_first; // [n_pos + 1]: the variants of position p are var_first[p] .. var_first[p + 1] - 1
    const uint32_t *var_codon; // [n_var], 0..63
    uint32_t *rows;            // [n_pos + n_var][row_words]: the informative rows, then the carry rows; a bit per read
    uint32_t *both, *carry, *joint;   // [n_pos][n_pos], [n_var][n_pos], [n_var][n_var]; zeroed
};
void jl_launch_variant_linkage(const jl_link_args *a, hipStream_t st);

// ---- whole-codon deletions at every codon start (kernels_del.hip, capi_del.hip; docs/SPEC.md §16)
struct jl_del_args {
    const uint8_t *msa;        // the window's bit planes
    uint64_t plane_stride;     // ... and their stride (an adopted matrix brings its own)
    uint64_t n_reads;
    uint32_t n_cols;           // >= 3
    uint32_t seg_tiles;        // tiles of 512 reads a workgroup walks (set by the launcher)
    uint32_t *cnt;             // [n_cols - 2][4] codon, del3, partial, span; zeroed
};
void jl_launch_codon_deletions(const jl_del_args *a, hipStream_t st);

// ---- deletions by extent: (start, length) alleles (kernels_del_alleles.hip, capi_del_alleles.hip; docs/SPEC.md §25)
struct jl_dal_args {
    const uint8_t *msa;        // the window's bit planes
    uint64_t plane_stride;     // ... and their stride (an adopted matrix brings its own)
    uint64_t n_reads;
    uint32_t n_cols;           // >= 1
    uint32_t n_words;          // words of a row that hold reads: ceil(n_reads / 32); 4 n_words <= plane_stride
    uint32_t seg_cols;         // columns a workgroup walks (set by the launcher)
    uint32_t occ_cap;          // room in occ[] (and in the rows): no more distinct alleles can exist
    unsigned long long *n_starts;   // [1] the runs of the matrix (the counting launch); zeroed
    unsigned long long *runs;  // [2] bounded, open; zeroed
    uint32_t *diff;            // [n_cols + 1]: + k where k open runs begin, - k where they end, modulo 2^32; zeroed
    // the allele table: `slots` (a power of two, at least twice occ_cap) key words col << 32 | len, all ones = empty, and their
    // read counts, zeroed; occ[] lists the slots in use, *n_occ (zeroed) how many
    unsigned long long *keys;
    uint32_t *count, *occ, *n_occ;
    uint64_t slots_mask;
};
void jl_launch_deletion_starts(const jl_dal_args *a, hipStream_t st);
void jl_launch_deletion_runs(const jl_dal_args *a, hipStream_t st);
void jl_launch_deletion_rows(const jl_dal_args *a, jl_deletion_allele *rows, hipStream_t st);

// ---- codon calls against a control's histograms (kernels_control.hip, capi_control.hip; docs/SPEC.md §21)
struct jl_control_args {
    jl_call_args A;            // alpha, n_tests, min_perc, max_perc, P (the error model's fields are not read)
    const uint32_t *pos_gene, *pos_codon, *pos_col;   // [P], the sample's (the control's are equal)
    const uint8_t *pos_refcfg; // [P]
    const uint32_t *hist_s;    // [n_cols][64] the sample's histograms
    const uint32_t *hist_c;    // ... and the control's
    const uint64_t *drm;       // [P] or null
    uint64_t *called;          // [P] scratch: the masks of the called codons
    jl_variant *staged;        // [P][64] scratch: their rows before the ordered compaction
    uint32_t *ctl_cov;         // [P] the control's coverage
    jl_variant *rows;          // [cap]
    uint32_t *n_rows;          // [1] rows needed
    uint32_t cap, pad_;
};
void jl_launch_control_call(const jl_control_args *a, hipStream_t st);
// jl_control_eval: n tables [[a, cov_s - a], [c, cov_c - c]], one thread each; skipped == nullptr: the plain form
void jl_launch_control_eval(uint32_t n, const uint32_t *a, const uint32_t *cov_s, const uint32_t *c, const uint32_t *cov_c,
                            double n_tests, double alpha, double *p, double *lp, uint32_t *skipped, hipStream_t st);

// ---- per-read counters over the whole window (kernels_readstats.hip, capi_readstats.hip; docs/SPEC.md §20)
struct jl_readstats_shape;     // readstats_shape.h
struct jl_readstats_args {
    const uint8_t *msa;        // the window's bit planes
    uint64_t plane_stride;     // ... and their stride (an adopted matrix brings its own)
    uint64_t n_reads;
    uint32_t n_cols;
    uint32_t n_words;          // words of a row that hold reads: ceil(n_reads / 32); 4 n_words <= plane_stride
    uint32_t n_chunks, seg_cols;   // of the launch shape (set by the launcher)
    const uint8_t *compare;    // [n_cols], or null: no column is compared
    uint32_t *part;            // the segments' byte counters (jl_readstats_part_words), or null when the shape combines by atomics
    uint32_t *stats;           // [JL_READ_STATS][n_reads]
};
void jl_launch_read_stats(const jl_readstats_args *a, const jl_readstats_shape *shape, hipStream_t st);
size_t jl_readstats_part_words(const jl_readstats_shape *shape);

// ---- per-read hypermutation counters and their exact test (kernels_hypermut.hip, capi_hypermut.hip; docs/SPEC.md §26)
struct jl_hypermut_args {
    const uint8_t *msa;        // the window's bit planes
    uint64_t plane_stride;     // ... and their stride (an adopted matrix brings its own)
    uint64_t n_reads;
    uint32_t n_cols;
    uint32_t n_words;          // words of a row that hold reads: ceil(n_reads / 32); 4 n_words <= plane_stride
    uint32_t n_chunks, seg_cols;   // of the launch shape (set by the launcher)
    const uint8_t *ref;        // [n_cols]
    uint32_t *part;            // the segments' byte counters (jl_hypermut_part_words), or null when the shape combines by atomics
    uint32_t *counts;          // [JL_HM_COUNTERS][n_reads]
};
void jl_launch_hypermut_counts(const jl_hypermut_args *a, const jl_readstats_shape *shape, hipStream_t st);
size_t jl_hypermut_part_words(const jl_readstats_shape *shape);
// one thread a read: p[i], lp[i] of the table counts[.][i] (n > 0; ceil(n / 256) workgroups fit a launch)
void jl_launch_hypermut_test(const uint32_t *counts, uint64_t n, double *p, double *lp, hipStream_t st);

// ---- per-read reading-frame counters per span (kernels_orf.hip, capi_orf.hip; docs/SPEC.md §27)
struct jl_orf_shape;           // orf_shape.h
struct jl_orf_seg {            // one workgroup's walk: whole codons of one span (the table capi_orf.hip builds from the shape)
    uint32_t col;              // window column of its first codon
    uint32_t n_codons;         // 1 .. 85
    uint32_t span;
    uint32_t first_codon;      // ... of the span that is codon 0 here
};
struct jl_orf_args {
    const uint8_t *msa;        // the window's bit planes
    uint64_t plane_stride;     // ... and their stride (an adopted matrix brings its own)
    uint64_t n_reads;
    uint32_t n_cols;
    uint32_t n_words;          // words of a row that hold reads: ceil(n_reads / 32); 4 n_words <= plane_stride
    uint32_t n_chunks;         // of the launch shape (set by the launcher)
    uint32_t n_spans, n_segs;
    const uint8_t *ref;        // [n_cols]
    const jl_orf_seg *segs;    // [n_segs], the segments of span 0 first, each span's in codon order
    const uint32_t *span_seg0; // [n_spans + 1]: the first segment of every span, and n_segs
    uint32_t *part;            // the segments' byte counters (jl_orf_part_words)
    uint32_t *counts;          // [JL_ORF_COUNTERS][n_spans][n_reads]
    uint32_t *first_stop;      // [n_spans][n_reads]
};
void jl_launch_orf_counts(const jl_orf_args *a, const jl_orf_shape *shape, hipStream_t st);
size_t jl_orf_part_words(const jl_orf_shape *shape);

// ---- the site matrix: chosen codon starts of a matrix, deletion sites recoded (kernels_sites.hip, capi_sites.hip; docs/SPEC.md §18)
struct jl_sites_args {
    const uint8_t *src;        // the source's bit planes
    uint64_t src_stride;       // ... and their stride (an adopted matrix brings its own)
    uint64_t n_reads;
    uint8_t *dst;              // [9 n_sites][dst_stride]
    uint64_t dst_stride;       // jl_plane_stride(n_reads): whole 128-byte lines, whatever src_stride is
    const jl_site *sites;      // [n_sites], each of kind 0 or 1 with col + 2 < the source's n_cols (an insertion site is skipped)
    uint32_t n_sites, pad_;    // 1 .. JL_SITES_MAX
};
void jl_launch_sites_assemble(const jl_sites_args *a, hipStream_t st);
// ... its insertion sites (docs/SPEC.md §19): an init pass over the planes, then one thread per event of the source's record build
struct jl_ins_site {
    uint32_t col;              // the junction: 1 .. the source's n_cols - 1
    uint32_t k;                // its site: destination rows 9 k .. 9 k + 8
    uint32_t a_begin, a_end;   // its alleles: [a_begin, a_end) of `alleles`, 1 .. JL_SITE_INS_MAX_ALLELES of them
};
struct jl_sites_ins_args {
    const uint8_t *src;
    uint64_t src_stride;
    uint64_t n_reads;
    uint8_t *dst;
    uint64_t dst_stride;
    const jl_ins_site *isites;            // [n_isites] ascending by col, no column twice
    const jl_insertion_allele *alleles;   // ascending by (col, len, seq)
    const jl_insertion_event *events;     // the source's, [min(*n_events, events_cap)]
    const uint32_t *n_events;
    uint32_t events_cap;
    uint32_t n_isites;                    // 1 .. JL_SITES_MAX
};
void jl_launch_sites_insertions(const jl_sites_ins_args *a, hipStream_t st);

// ---- in-frame insertion alleles of a record build (kernels_ins.hip, capi_ins.hip; docs/SPEC.md §17)
#define JL_INSAL_MAX_BASES 30u             // longest insertion that is an allele: 60 bits of sequence
struct jl_insal_args {
    // the records (jl_records: one run of device arrays) and the window
    uint64_t n_reads;
    uint32_t n_cols, win_begin;
    uint32_t min_qv, pad_;     // min_qv at most 127, as the planes kernel takes it
    const int32_t *pos;
    const uint32_t *cigar;
    const uint64_t *cig_off;
    const uint8_t *seq4;
    const uint64_t *seq_off;
    const uint8_t *qual;       // the filter in force, as jl_launch_ingest resolves it: quality bytes, or
    const uint64_t *qual_off;
    const uint8_t *qmask;      // a bit per base, or neither
    uint32_t *jcnt;            // [n_cols][4] span, inframe, frameshift, unread; zeroed
    // the allele table: `slots` (a power of two, at least twice the I ops of the records) of key words (col << 32 | len) and
    // (seq), all ones = empty, and their read counts, zeroed; occ[] lists the slots in use, *n_occ (zeroed) how many
    unsigned long long *key0, *key1;
    uint32_t *count, *occ, *n_occ;
    uint64_t slots_mask;
    // the per-read events (jl_msa_track_insertion_reads; docs/SPEC.md §19), null when not tracked: room for events_cap rows,
    // *n_events (zeroed) counts every event, written or not
    jl_insertion_event *events;
    uint32_t *n_events;
    uint32_t events_cap, pad2_;
};
void jl_launch_insertion_alleles(const jl_insal_args *a, hipStream_t st);
struct jl_insal_span_args {
    const uint8_t *msa;        // the window's bit planes
    uint64_t plane_stride;
    uint64_t n_reads;
    uint32_t n_cols;           // >= 2
    uint32_t seg_tiles;        // tiles of 512 reads a workgroup walks (set by the launcher)
    uint32_t *jcnt;            // [n_cols][4]: [c][0] += reads whose cells at c - 1 and c are both covered
};
void jl_launch_junction_span(const jl_insal_span_args *a, hipStream_t st);
// the occupied slots of the table as rows, in the order of occ[] (capi_ins.hip sorts them on the host)
void jl_launch_insertion_rows(const unsigned long long *key0, const unsigned long long *key1, const uint32_t *count, const uint32_t *occ,
                              uint32_t n, jl_insertion_allele *rows, hipStream_t st);

inline int jl_hip_status(hipError_t e) { return e == hipErrorOutOfMemory ? JL_ERR_MEMORY : JL_ERR_DEVICE; }

// ---- owning arrays.  Every buffer a context owns is one of these: it frees itself when the context is deleted (jl_ctx_destroy, the
// device still current), so there is no list of pointers to keep.  None may have static or thread-local storage duration: its
// destructor would call into a HIP runtime that is gone at process exit.
// `cap` elements at `d`, device memory or (Pinned) pinned host memory.  The object stands where the pointer stood: it converts to T *.
template <typename T, bool Pinned>
struct jl_owned_array {
    T *d = nullptr;
    size_t cap = 0;
    jl_owned_array() = default;
    jl_owned_array(const jl_owned_array &) = delete;
    jl_owned_array &operator=(const jl_owned_array &) = delete;
    ~jl_owned_array() { release(); }
    operator T *() const { return d; }
    T *operator->() const { return d; }
    template <typename U> U *as() const { return reinterpret_cast<U *>(d); }   // the same memory in another element type
    // Room for exactly `n` elements, grow-only, contents not kept; *moved: `d` is another pointer now (or none: the error returned).
    // The old array is freed BEFORE the new one is made: the peak stays low, and hipFree waits for the device, so nothing enqueued
    // still reads what goes.
    hipError_t reserve_exact(size_t n, bool *moved)
    {
        *moved = !(d && cap >= n);
        if (!*moved) return hipSuccess;
        release();
        const hipError_t e = Pinned ? hipHostMalloc((void **)&d, n * sizeof(T), hipHostMallocDefault) : hipMalloc((void **)&d, n * sizeof(T));
        if (e == hipSuccess) cap = n;
        return e;
    }
    void release()
    {
        if (d) Pinned ? hipHostFree((void *)d) : hipFree((void *)d);
        d = nullptr, cap = 0;
    }
};
template <typename T> using jl_pinned_array = jl_owned_array<T, true>;

// A device array that grows with slack.  Making room returns HIP's error (jl_hip_status: the status it becomes).
template <typename T>
struct jl_dev_array : jl_owned_array<T, false> {
    using jl_owned_array<T, false>::d;
    using jl_owned_array<T, false>::cap;
    // room for `need` elements (+ pad_bytes behind them); the first `used` move along, on `st`
    hipError_t grow_keep(hipStream_t st, size_t used, size_t need, size_t pad_bytes)
    {
        if (d && need <= cap) return hipSuccess;
        const size_t ncap = std::max<size_t>({need, cap + cap / 2, (size_t)1024});
        T *nd = nullptr;
        hipError_t e = hipMalloc(&nd, ncap * sizeof(T) + pad_bytes);
        if (e != hipSuccess) return e;
        if (d && used) e = hipMemcpyAsync(nd, d, used * sizeof(T), hipMemcpyDeviceToDevice, st);
        if (d) {
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            hipFree(d);
        }
        d = nd;
        cap = ncap;
        return e;
    }
    // room for `n` elements, grow-only; the old contents are not kept
    hipError_t grow_discard(hipStream_t st, size_t n)
    {
        if (d && cap >= n) return hipSuccess;
        hipError_t e = d ? hipStreamSynchronize(st) : hipSuccess;   // what is enqueued on `st` may still read it
        bool moved;
        return e != hipSuccess ? e : this->reserve_exact(n + n / 8 + 64, &moved);
    }
};

// What a call uploads on every invocation: the host fills pinned staging, one copy takes it to the device array.
template <typename T>
struct jl_upload_staging {
    jl_pinned_array<T> h;
    jl_dev_array<T> dev;
    hipEvent_t ev = nullptr;   // behind the last upload out of the staging: it may be refilled then
    jl_upload_staging() = default;
    jl_upload_staging(const jl_upload_staging &) = delete;
    jl_upload_staging &operator=(const jl_upload_staging &) = delete;
    ~jl_upload_staging() { if (ev) hipEventDestroy(ev); }
    // *out = the staging with room for `n` elements, once the last upload has read it
    hipError_t host(size_t n, T **out)
    {
        hipError_t e = ev ? hipSuccess : hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventSynchronize(ev);
        bool moved;
        if (e == hipSuccess && h.cap < n) e = h.reserve_exact(n + n / 8 + 1024, &moved);
        *out = h;
        return e;
    }
    // its first `n` elements to `dev` (grown, the old contents not kept) on `st`
    hipError_t upload(hipStream_t st, size_t n)
    {
        hipError_t e = dev.grow_discard(st, n);
        if (e == hipSuccess) e = hipMemcpyAsync(dev, h, n * sizeof(T), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipEventRecord(ev, st);
        return e;
    }
};

// Records uploaded so far by jl_records_append: one run of device arrays, offsets rebased to it (capi_records.hip).
struct jl_records {
    bool open = false, have_qual = false;
    bool masked = false;     // a masked stream (jl_records_append_masked): `mask` holds a bit per nibble of `seq`, every chunk begins on 16 bytes of `seq`
    jl_dev_array<uint8_t> seq, qual, mask;
    jl_dev_array<uint32_t> cig;
    jl_dev_array<uint64_t> co, so, qo;   // the reads' offsets into cig, seq, qual
    jl_dev_array<int32_t> pos;
    uint64_t n_reads = 0, n_cig = 0, n_seq = 0, n_qual = 0;
    uint64_t n_ins_ops = 0;  // 'I' ops among the cigar words so far: what the allele table of a tracking build is sized from (docs/SPEC.md §17)
    // does any read need the ingest's launch for long reads (kernels_ingest.hip jl_ingest_read_is_long)?  Found out at the upload for
    // the few reads a CCS sample has with more ops than entries fit; `true` as soon as looking would cost more than the launch
    bool maybe_long = false;
    // frees them and is a stream not begun again
    void release()
    {
        seq.release(), qual.release(), mask.release(), cig.release(), co.release(), so.release(), qo.release(), pos.release();
        open = have_qual = masked = maybe_long = false;
        n_reads = n_cig = n_seq = n_qual = n_ins_ops = 0;
    }
};

// How a build takes the QV filter: the planes kernel's template argument (kernels_ingest.hip kQvNone, kQvBytes, kQvMask).
enum jl_qv_mode : uint32_t {
    JL_QV_NONE = 0,    // no filter: min_qv 0, or a stream with neither qualities nor a mask
    JL_QV_BYTES = 1,   // a quality byte per base against min_qv
    JL_QV_MASK = 2,    // a bit per base (a masked stream; min_qv only switches the filter on)
};
inline jl_qv_mode jl_qv_mode_of(bool have_qual, bool masked, uint32_t min_qv)
{
    return min_qv == 0u ? JL_QV_NONE : have_qual ? JL_QV_BYTES : masked ? JL_QV_MASK : JL_QV_NONE;
}

// Scratch of the record ingest INTO a context (kernels_ingest.hip), kept between builds.
struct jl_ingest_scratch {
    jl_dev_array<uint2> runs;       // the reads' runs
    jl_dev_array<uint32_t> nruns;
    jl_dev_array<uint4> desc;       // one descriptor per (sweep, read): the run at every sweep's first column
    jl_dev_array<uint2> slow;       // the units handed on to the planes kernel's second size
    jl_dev_array<uint32_t> d_count; // 64 bytes: the counters of a build and the verdict word (jl_launch_ingest)
    bool check_pending = false;     // an ingest ran (or is enqueued) whose verdict on the records has not been read yet
};

enum class jl_phase_form : uint32_t {   // the pipeline that phases a context; the value is the plan's fast_only (phase_plan.h)
    multi_word = 0,   // more than 20 positions, or a result beyond the fused selection: keys, group, select, assign launches
    one_word = 1,     // up to 10 positions: phase_fused1_kernel (phase_group_run_kernel in a group run)
    two_word = 2,     // 11..20 positions: phase_fused2_kernel (jl_two_word)
};
enum class jl_phase_plan {   // where jl_launch_phase finds the plan (meta, vpcols)
    plan_kernel,   // the stand-alone plan kernel runs first, from the resident variant table (stage API, re-runs)
    resident,      // a compact launch or the cross-window session wrote it already
    call_masks,    // the fused launch derives it from the Fisher stage's call masks (whole-path runs)
};

struct jl_ctx {
    int device = -1;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;

    // ---- resident MSA: THE format, written directly by every producer (upload, by-row pack, record ingest, synthetic
    // fill) and read by every consumer (pileup, phasing, cross-window exchange, an adopted matrix): per column three BIT
    // PLANES — plane k holds bit k of every read's 3-bit symbol code (A C G T - N ' ' = 0..6), read i in bit i & 7 of byte
    // i >> 3 — i.e. 3 bits per cell.  Plane k of column c at d_msa + (3 c + k) * plane_stride; plane_stride =
    // jl_plane_stride(n_reads) (reads padded to a multiple of 1024 with code 6: whole 128-byte lines per plane), or the
    // caller's for an adopted matrix.  `col_stride` = 4 * plane_stride is the same stride counted in "8 reads per dword"
    // units: the phasing kernels give a lane 8 reads (dword t of a column <=> byte t of each plane), reads_pad = 2 col_stride.
    uint8_t *d_msa = nullptr;         // raw: owned (own_msa) or the caller's (jl_msa_adopt)
    bool own_msa = false;
    size_t msa_capacity = 0;          // bytes, of an owned one
    uint64_t plane_stride = 0;
    uint64_t n_reads = 0;
    uint32_t n_cols = 0;
    uint64_t col_stride = 0;
    uint32_t win_begin = 0;

    // ---- insertions per column (fuse-style consensus; off unless jl_msa_track_insertions)
    bool track_insertions = false;
    bool ins_valid = false;
    jl_dev_array<uint32_t> d_ins_len;    // [n_cols][JL_INS_LEN_BINS]
    jl_dev_array<uint32_t> d_ins_base;   // [n_cols][JL_INS_MAX_BASES][4]

    // ---- in-frame insertion alleles of the last record build (docs/SPEC.md §17; off unless jl_msa_track_insertion_alleles)
    bool track_ins_alleles = false;
    bool insal_valid = false;                      // gone with the matrix they belong to: set_shape
    jl_dev_array<uint32_t> insal_jcnt;             // [n_cols][4]
    jl_dev_array<unsigned long long> insal_keys;   // key0 [insal_slots], then key1 [insal_slots]
    jl_dev_array<uint32_t> insal_count;            // count [insal_slots], occ [insal_slots], n_occ [1]
    jl_dev_array<jl_insertion_allele> insal_rows;  // the fetch's gather
    uint64_t insal_slots = 0;                      // of the last tracking build
    // ... and its per-read events (docs/SPEC.md §19; off unless jl_msa_track_insertion_reads, which implies the alleles)
    bool track_ins_reads = false;
    bool insev_valid = false;                      // gone where insal_valid goes
    jl_dev_array<jl_insertion_event> insev_rows;   // [insev_cap], in the order of the walk's atomics
    jl_dev_array<uint32_t> insev_count;            // [1]: events counted
    uint32_t insev_cap = 0;                        // the 'I' ops of the last tracking build's records

    // ---- aligned records on their way in (jl_records_begin / _append / _finish)
    jl_records rec;
    jl_ingest_scratch ing;            // ... and of the builds into this context's matrix

    // ---- jl_msa_take INTO this context: the parts' indices on their way to the device (capi_take.hip)
    jl_upload_staging<uint32_t> take_idx;

    // ---- jl_class_pileup_async: buffers of its own, grown on demand (capi_class.hip); no stage and no run touches them
    jl_upload_staging<uint16_t> class_label;
    jl_dev_array<uint8_t> class_mask;
    jl_dev_array<uint32_t> class_out;   // counts [class_k][class_cols][6], then class_reads [class_k]
    uint32_t class_k = 0, class_cols = 0;   // shape of the last class pileup enqueued (class_k = 0: none)

    // ---- jl_class_codons_async: buffers of its own, grown on demand (capi_class_codons.hip); no stage, no run and no class pileup touches them
    jl_upload_staging<uint16_t> cc_label;
    jl_upload_staging<uint32_t> cc_col;
    jl_dev_array<uint8_t> cc_mask;
    jl_dev_array<uint32_t> cc_out;      // hist [cc_k][cc_pos][64], then class_reads [cc_k]
    uint32_t cc_k = 0, cc_pos = 0;      // shape of the last call enqueued (cc_k = 0: none)

    // ---- jl_phase_rescue_async: buffers of its own, grown on demand (capi_rescue.hip); no stage and no run touches them
    jl_upload_staging<uint32_t> rescue_in;   // pos_cols [n_pos], then pat4 (jl_stage_hap_direction, hap_stage.h)
    jl_dev_array<uint32_t> rescue_out;   // tally [4] as 8 words, hap_reads [JL_RESCUE_HAP_PAD], then rescue [rescue_n] 16 bits each
    uint64_t rescue_n = 0;               // reads of the last rescue enqueued (0: none)
    uint32_t rescue_h = 0;               // ... and its haplotypes

    // ---- jl_phase_nearest_async: buffers of its own, grown on demand (capi_nearest.hip); no stage, no run and no rescue touches them
    jl_upload_staging<uint32_t> nearest_in;   // pos_cols [n_pos], then pat4 (jl_stage_hap_direction, hap_stage.h)
    jl_dev_array<uint32_t> nearest_out;  // tally [4] as 8 words, hap_reads [JL_NEAREST_HIST_WORDS], nearest [nearest_n] 16 bits each, dist [nearest_n] bytes
    uint64_t nearest_n = 0;              // reads of the last call enqueued (0: none)
    uint32_t nearest_h = 0, nearest_d = 0;   // ... its haplotypes and its budget D

    // ---- jl_phase_recombinants_async: buffers of its own, grown on demand (capi_recomb.hip); no stage, no run, no rescue and no nearest call touches them
    jl_upload_staging<uint32_t> recomb_in;   // pos_cols [n_pos] and pat4, then both again in descending order (jl_recomb_args)
    jl_dev_array<uint32_t> recomb_out;   // tally [5] as 12 words, parent_reads [JL_RECOMB_HIST_WORDS], left, right, prefix, suffix [recomb_n] 16 bits each
    uint64_t recomb_n = 0;               // reads of the last call enqueued (0: none)
    uint32_t recomb_h = 0;               // ... and its haplotypes

    // ---- jl_variant_linkage_async: buffers of its own, grown on demand (capi_link.hip); no stage and no run touches them
    jl_upload_staging<uint32_t> link_in;   // pos_cols [n_pos], var_first [n_pos + 1], var_codon [n_var] (jl_link_args)
    jl_dev_array<uint32_t> link_rows;      // the bit rows
    jl_dev_array<uint32_t> link_out;       // both [link_p][link_p], carry [link_v][link_p], joint [link_v][link_v]
    uint32_t link_p = 0, link_v = 0;       // shape of the last linkage enqueued (link_p = 0: none)

    // ---- jl_codon_deletions_async: a buffer of its own, grown on demand (capi_del.hip); no stage and no run touches it
    jl_dev_array<uint32_t> del_out;        // cnt [del_cols - 2][4]
    uint32_t del_cols = 0;                 // columns of the last call enqueued (0: none)

    // ---- jl_deletion_alleles_async: buffers of its own, grown on demand (capi_del_alleles.hip); no stage and no run touches them
    jl_dev_array<unsigned long long> dal_u64;   // n_starts [1], runs [2], a spare word, then the keys [dal_slots]
    jl_dev_array<uint32_t> dal_u32;             // n_occ [1] and three spare words, diff [dal_cols + 1], count [dal_slots], occ [dal_cap]
    jl_dev_array<jl_deletion_allele> dal_rows;  // [dal_cap], in the order in which the slots were claimed
    uint64_t dal_slots = 0;                     // of the last call enqueued
    uint32_t dal_cap = 0;                       // ... its bound on the distinct alleles
    uint32_t dal_cols = 0;                      // ... and its columns (0: none)

    // ---- jl_control_call_async with this context as the SAMPLE: result buffers of its own, grown on demand (capi_control.hip); the
    // masks and the staged rows of the call stage (d_called, d_staged) are its scratch, no stage result and no run sees the rest
    jl_dev_array<jl_variant> ctl_rows;     // [JL_VARIANT_CAP]
    jl_dev_array<uint32_t> ctl_out;        // rows needed [2], then the control's coverage [ctl_p]
    std::vector<uint32_t> ctl_pos_gene, ctl_pos_codon;   // the positions of the last call enqueued: the fetch finds a row's by them
    uint32_t ctl_p = 0;                    // ... and how many
    bool ctl_done = false;
    struct event_slot {                    // the control's pileup before the sample's launch, when their streams differ
        hipEvent_t ev = nullptr;
        ~event_slot() { if (ev) hipEventDestroy(ev); }
    } ctl_ev;

    // ---- jl_read_stats_async: buffers of its own, grown on demand (capi_readstats.hip); no stage and no run touches them
    jl_upload_staging<uint8_t> rs_compare; // the compare row on its way to the device
    jl_dev_array<uint32_t> rs_part;        // the column segments' byte counters, when a second kernel combines them
    jl_dev_array<uint32_t> rs_out;         // stats [JL_READ_STATS][rs_reads]
    uint64_t rs_reads = 0;                 // reads of the last call enqueued (0: none)

    // ---- jl_read_hypermut_async: buffers of its own, grown on demand (capi_hypermut.hip); no stage and no run touches them
    jl_upload_staging<uint8_t> hm_ref;     // the reference row on its way to the device
    jl_dev_array<uint32_t> hm_part;        // the column segments' byte counters, when a second kernel combines them
    jl_dev_array<uint32_t> hm_out;         // counts [JL_HM_COUNTERS][hm_reads]
    jl_dev_array<double> hm_p;             // p [hm_reads], then log_p [hm_reads]
    uint64_t hm_reads = 0;                 // reads of the last call enqueued (0: none)

    // ---- jl_read_orf_async: buffers of its own, grown on demand (capi_orf.hip); no stage and no run touches them
    jl_upload_staging<uint8_t> orf_ref;    // the reference row on its way to the device
    jl_upload_staging<uint32_t> orf_tab;   // the segment table (jl_orf_seg [n_segs]), then the spans' first segments [n_spans + 1]
    jl_dev_array<uint32_t> orf_part;       // the segments' byte counters
    jl_dev_array<uint32_t> orf_out;        // counts [JL_ORF_COUNTERS][orf_spans][orf_reads], then first_stop [orf_spans][orf_reads]
    uint64_t orf_reads = 0;                // reads of the last call enqueued (0: none)
    uint32_t orf_spans = 0;                // ... and its spans

    // ---- jl_sites_assemble INTO this context: the site table on its way to the device (capi_sites.hip)
    jl_upload_staging<jl_site> sites_in;
    jl_upload_staging<jl_ins_site> ins_sites_in;             // jl_sites_assemble_alleles: the insertion sites and
    jl_upload_staging<jl_insertion_allele> site_alleles_in;  // their alleles

    // ---- phasing sharded by reads: the groups of this matrix exported for the merge (jl_phase_groups_async / _fetch)
    bool phase_export = false;        // the phase launch in flight / last run exported instead of selecting
    jl_dev_array<uint32_t> d_exp_count;  // [exp_cap]
    jl_dev_array<uint8_t> d_exp_pattern; // [exp_cap][exp_stride]
    jl_dev_array<uint16_t> d_exp_hap;    // [exp_cap] the merge's answer on its way to the slots
    uint32_t exp_cap = 0, exp_stride = 0;   // the shape the three were made for (more than a capacity: kernels index with them)
    uint32_t exp_n_groups = 0;        // groups the last export produced, once the host has read the count (regroup checks it)
    uint32_t exp_vp = 0;              // ... and its variant positions (0: nothing was phased, no read has flags or a slot)
    bool exp_known = false;
    // a session (capi_xwin.hip) has the groups written into its own block instead (pinned host memory, or the send
    // buffer of the all-gather); null: the context's arrays above
    uint32_t *exp_ext_count = nullptr;
    uint8_t *exp_ext_pattern = nullptr;
    uint32_t *exp_ext_head = nullptr;
    uint32_t exp_ext_cap = 0, exp_ext_stride = 0;
    jl_direct_cols direct = {};       // direct.on: the next fused phase launch reads these columns (see jl_direct_cols)

    // ---- pileup plan (host copies + device arrays)
    std::vector<jl_gene> genes;
    std::vector<uint8_t> refseq;
    bool have_ref = false;
    bool plan_valid = false;
    uint32_t P = 0;
    double default_n_tests = 0.0;
    std::vector<uint32_t> h_pos_gene, h_pos_codon, h_pos_col;
    jl_dev_array<uint32_t> d_pos_gene, d_pos_codon, d_pos_col;   // [P] each, as are d_pos_next, d_called, d_drm; d_staged [P][64]
    jl_dev_array<uint8_t> d_pos_refcfg;
    // the positions by column, for the Fisher stage folded into the pileup launch (kernels_pileup.hip): col_head[c] = the first
    // position whose codon begins at column c (all ones: none), pos_next[p] = the next one at the same column (genes that overlap
    // in one frame)
    jl_dev_array<uint32_t> d_col_head, d_pos_next;
    jl_dev_array<uint8_t> d_guess; // [n_cols + JL_GUESS_PAD] base the codon compare is seeded with (never affects
                                   // results); the zeroed pad lets the kernel fetch it as aligned dwords

    // ---- pileup outputs: one zeroed region = col counts [n_cols][6] then hist [n_cols][64]
    jl_dev_array<uint32_t> d_counts;
    uint32_t *d_hist = nullptr;    // a view into d_counts
    size_t counts_words = 0;
    bool pileup_done = false;
    // pileup chunk table (host-built, see build_chunks): chunk k owns columns [c0, c0 + n), n <= pileup_w
    uint32_t pileup_w = 3;
    uint32_t n_chunks = 0;
    jl_dev_array<uint64_t> d_chunks;  // [n_chunks] records {first column, JL_CHUNK_META}: see kernels_pileup.hip

    // ---- call
    jl_dev_array<uint64_t> d_called;   // [P] mask of called codons
    jl_dev_array<jl_variant> d_staged; // [P][64] finished rows of the called codons, before the ordered compaction
    jl_dev_array<uint64_t> d_drm;      // [P] optional
    jl_dev_array<jl_variant> d_variants;  // [JL_VARIANT_CAP]
    jl_dev_array<uint32_t> d_nvar;        // [0] rows needed, [1] spare
    bool call_done = false;

    // ---- phase
    jl_dev_array<jl_phase_meta> d_meta;
    jl_dev_array<uint32_t> d_vpcols;   // [JL_VARIANT_CAP]
    jl_dev_array<uint32_t> d_col2pos;  // [n_cols]
    jl_dev_array<uint8_t> d_varcol;    // [n_cols] scratch flags
    jl_dev_array<uint64_t> d_keys;     // [kwords_cap][reads_pad]
    uint32_t keys_words = 0;        // 64-bit words per read the key buffer holds
    uint32_t last_min_reads = 10;
    jl_dev_array<uint32_t> d_flagw;    // [reads_pad/8] nibble flags
    jl_dev_array<uint32_t> d_blockcat; // [phase workgroups][4] read categories of each workgroup's reads (summed by the selection)
    jl_dev_array<uint32_t> d_read_slot;  // [reads_pad]
    jl_dev_array<uint16_t> d_read_hap;   // [reads_pad]
    jl_dev_array<uint32_t> d_slot_rep, d_slot_count;  // [M]
    jl_dev_array<uint64_t> d_slot_key;                // [M] single-word keys (fused path)
    jl_dev_array<uint32_t> d_slot_hap;                // [M] haplotype id of a table slot (32-bit: write-through stores)
    jl_dev_array<uint32_t> d_occupied;                // [reads_pad]
    uint64_t table_slots = 0;
    size_t reads_capacity = 0;      // reads_pad the per-read arrays and the grouping table were made AND INITIALISED for (more than a
                                    // capacity: the whole group is made anew, its table emptied, when this grows)
    jl_dev_array<uint32_t> d_hap_count;   // [JL_MAX_HAPLOTYPES]
    jl_dev_array<uint8_t> d_hap_pattern;  // [JL_MAX_HAPLOTYPES][JL_VARIANT_CAP]
    jl_dev_array<uint8_t> d_hit;          // [JL_VARIANT_CAP][JL_MAX_HAPLOTYPES]
    jl_dev_array<uint32_t> d_cooc;        // [cooc_cap][cooc_cap]
    uint32_t cooc_cap = 256;
    bool phase_done = false;
    bool ids_separate = false;   // a phase launch of this context with inline ids timed out once: the ids take a launch of their own
    jl_phase_form phase_form = jl_phase_form::one_word;   // only grows, except where a session sets it (jl_phase_groups_prepare)
    jl_dev_array<uint64_t> d_slot_key_a, d_slot_key_b;   // half-key tables of the two-word launch [table slots]
    jl_dev_array<uint32_t> d_occ_a, d_occ_b;             // [reads_pad]
    uint64_t two_slots = 0;   // table size the half-key tables were made and emptied for (more than a capacity: 0 = to be made anew)

    // ---- whole-path run: result pack, pinned mirrors, captured graph
    jl_dev_array<jl_pack> d_pack;     // [2]: run n writes block n & 1 (an exchange may still read the other one)
    jl_pinned_array<jl_pack> h_pack;
    jl_pinned_array<uint16_t> h_read_hap;   // [reads_pad]
    jl_pack *pack_mirror = nullptr;     // where kernels mirror the result block (h_pack during jl_run_async)
    uint16_t *read_hap_out = nullptr;   // where phase_assign_kernel writes (h_read_hap when the host wants the ids)
    bool pack_valid = false;          // the last stage calls were one jl_run_async
    bool run_read_hap = false;
    // completion without a HIP sync: the last kernel of a run bumps d_sync[0] and stores it to *h_seq (pinned)
    jl_dev_array<uint32_t> d_sync;    // [16] zeroed once: [0] runs completed, [1..] arrival counters of fused kernels
    jl_pinned_array<volatile uint32_t> h_seq;  // [16]: [0] the run word; [4] the word of jl_fetch_to_host
    jl_pinned_array<uint8_t> h_scratch;   // small device arrays on their way to the host (a first pageable copy of a
                                          // process costs the runtime milliseconds: staging buffers, pinning the target)
    uint32_t fetches = 0;             // completed jl_fetch_to_host calls (device word d_sync[8], host word h_seq[4])
    uint32_t runs_launched = 0;
    uint32_t exch_pending = 0;        // exchanges requested and not yet collected: each still reads one of the two result blocks
    std::vector<uint32_t> exch_runs;  // ... and the runs (values of runs_launched) whose blocks they read
    hipStream_t run_stream = nullptr;  // where the last run was enqueued (the ctx stream, or a group's)
    bool pileup_clock = false;        // jl_run_pileup_clock: clock nodes around the pileup of a run -> h_seq[8..11] (two 64-bit stamps)
    uint32_t clock_run = 0;           // value of runs_launched of the run those stamps belong to (0: none)
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    std::vector<uint8_t> graph_sig;
    std::vector<uint8_t> graph_seen;   // signature of the last eager run (a configuration is captured on its second run)
    // What a captured graph bakes in went stale.  Bumped by jl_ctx_reserve (capi.hip) when an array moved, the one place that
    // reserves what a run or a stage touches, and by hand where no allocation is behind it.  These four are the complete list:
    // set_shape (the matrix's shape), free_msa (an adopted or owned matrix goes), phase_ids_go_separate (the ids get a launch
    // of their own), jl_run_pileup_clock (the clock nodes come or go).
    uint64_t alloc_version = 0;
    uint64_t plan_version = 0;

    // ---- the deviation index (deviation_index.h, capi_index.hip): a structure DERIVED from the planes, owned here, dropped in
    // one place (jl_msa_touched) and by a new chunk table (build_plan).  Never built for a matrix that is analysed once.
    uint64_t msa_gen = 1;              // the matrix generation: bumped by jl_msa_touched
    uint32_t ix_runs = 0;              // runs enqueued on this generation and chunk table
    bool ix_reserved = false;          // the buffers below are made for this generation and chunk table
    bool ix_build_due = false;         // the run being enqueued is the second: the build goes behind its last node
    bool ix_enqueued = false;          // ... and is on a stream (or done): the pinned record says which
    uint32_t ix_last_form = 0;         // 1: the last enqueued run counted from the index
    uint32_t ix_builds = 0;            // builds enqueued over the context's life
    hipStream_t ix_stream = nullptr;   // where the build was enqueued
    uint32_t ix_n_plain = 0, ix_n_rest = 0;
    std::vector<uint64_t> h_chunks;    // host copy of the chunk table (build_plan)
    jl_dev_array<uint4> d_ix_tab;      // [ix_n_plain] jl_win_index::tab
    jl_dev_array<uint64_t> d_ix_rest;  // [ix_n_rest] chunk records of the chunks that are not plain: the plane kernel's table of an index-form run
    jl_dev_array<jl_ix_stored_t> d_ix_entries;   // jl_ix_alloc_entries(...) stored entries, JL_IX_ENTRY_BYTES each
    jl_dev_array<uint8_t> d_ix_seed;   // [n_cols]
    jl_dev_array<uint32_t> d_ix_rec;   // [8] the build's record on the device; [4..] cursors of the build
    event_slot ix_ev;                  // behind the build's last kernel: whoever drops the index waits for it
    jl_pinned_array<volatile uint32_t> h_ix;   // [8] {state, entries, indexed chunks, generation (low word)}: stored by the build's last kernel
    int pileup_blocks_per_cu[16] = {0};  // occupancy per kernel variant, queried once

    // ---- timing
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

// status helpers -----------------------------------------------------------------------------
int jl_fail(jl_ctx *ctx, int status, const char *fmt, ...);
#define JL_HIP(ctx, expr)                                                                            \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess)                                                                        \
            return jl_fail(ctx, jl_hip_status(e_), "%s: %s", #expr, hipGetErrorString(e_));          \
    } while (0)

// What `enqueue` (a callable returning a status) puts on `st`, captured and instantiated.  False: both stay null, the caller launches eagerly.
template <class F>
static inline bool jl_capture_graph(hipStream_t st, hipGraph_t *graph, hipGraphExec_t *exec, F &&enqueue)
{
    if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) return false;
    const int rc = enqueue();
    hipGraph_t g = nullptr;
    const bool ok = hipStreamEndCapture(st, &g) == hipSuccess && g && rc == JL_OK && hipGraphInstantiate(exec, g, nullptr, nullptr, 0) == hipSuccess;
    if (ok) *graph = g;
    else { if (g) hipGraphDestroy(g); *exec = nullptr; }
    (void)hipGetLastError();
    return ok;
}

// kernel launchers (defined in the .hip files) -------------------------------------------------
void jl_launch_guess(jl_ctx *ctx, hipStream_t st);
void jl_launch_pileup(jl_ctx *ctx, hipStream_t st);
// The pileup launch with the Fisher stage in its epilogue (runs only; every chunk counted by ONE workgroup): false = not
// possible for this shape (the reads of a column are split over several workgroups), nothing was launched.
bool jl_pileup_can_fold(jl_ctx *ctx);
bool jl_fold_enabled(void);
void jl_launch_pileup_fold(jl_ctx *ctx, hipStream_t st, const jl_win_call *call);
void jl_fill_win_fold(jl_ctx *ctx, const jl_win_call *call, jl_win_fold *f);
int jl_launch_pileup_fold_group(jl_ctx *const *ctxs, uint32_t n_win, const jl_win_pileup *h_wins, const jl_win_fold *h_fold, uint32_t max_chunks, hipStream_t st);
uint32_t jl_pileup_rsplit(jl_ctx *ctx);
bool jl_pileup_needs_zero(jl_ctx *ctx);
void jl_prepare_pileup(jl_ctx *ctx);
void jl_launch_call(jl_ctx *ctx, hipStream_t st, const jl_params *prm, double n_tests, bool use_drm, bool with_meta);
void jl_launch_compact(jl_ctx *ctx, hipStream_t st, bool plan, bool pack, bool signal);
bool jl_launch_phase(jl_ctx *ctx, hipStream_t st, uint32_t min_reads, jl_phase_plan plan, bool signal);
void jl_fill_call_args(jl_ctx *ctx, const jl_params *prm, double n_tests, jl_call_args *A);
// the deviation index (capi_index.hip, kernels_index.hip, kernels_pileup.hip)
void jl_msa_touched(jl_ctx *ctx);                    // the one invalidation point: every writer of d_msa reaches it
void jl_index_drop(jl_ctx *ctx);                     // a new chunk table: the index and its run counter go, the generation stays
int jl_index_count_run(jl_ctx *ctx);                 // a run is about to be enqueued: counts it; the second reserves the buffers (may wait)
void jl_index_after_run(jl_ctx *ctx, hipStream_t st);    // ... it is enqueued: the build behind its last node, if due
bool jl_index_usable(const jl_ctx *ctx);             // the pinned record says "built" for the current generation: no HIP call
void jl_launch_index_build(jl_ctx *ctx, hipStream_t st);   // kernels_index.hip: the five launches of a build
void jl_fill_win_index(jl_ctx *ctx, jl_win_index *w);
void jl_fill_win_pileup_rest(jl_ctx *ctx, bool grouped, jl_win_pileup *w);   // the plane kernel's block over the chunks that are not plain
void jl_launch_pileup_index(jl_ctx *ctx, hipStream_t st, const jl_win_call *call);   // one window: index kernel (+ plane kernel over the rest); call != null: folded
int jl_launch_pileup_index_group(jl_ctx *const *ctxs, uint32_t n_win, const jl_win_index *h_wins, const jl_win_fold *h_fold, uint32_t max_plain, hipStream_t st);
// group runs: fill one window's argument block / launch a stage once for `n_win` <= JL_GROUP_MAX windows (the blocks
// travel by value in the kernel arguments)
void jl_fill_win_pileup(jl_ctx *ctx, jl_win_pileup *w);
void jl_fill_win_call(jl_ctx *ctx, const jl_params *prm, double n_tests, bool use_drm, bool with_meta, jl_win_call *w);
void jl_fill_win_compact(jl_ctx *ctx, bool plan, bool pack, bool signal, jl_win_compact *w);
// jl_phase_ids_inline decides who writes a launch's per-read ids: true goes into every window's block (`ids_inline`), false adds the ids launch
uint32_t jl_phase_grid_blocks(const jl_ctx *ctx);
bool jl_phase_ids_inline(jl_ctx *const *ctxs, uint32_t n_win);
void jl_fill_win_phase(jl_ctx *ctx, uint32_t min_reads, bool signal, bool ids_inline, jl_phase_plan plan, jl_win_phase *w);
int jl_launch_pileup_group(jl_ctx *const *ctxs, uint32_t n_win, const jl_win_pileup *h_wins, uint32_t max_chunks, hipStream_t st);
void jl_launch_call_group(const jl_win_call *h_wins, uint32_t n_win, uint32_t max_blocks, hipStream_t st);
void jl_launch_compact_group(const jl_win_compact *h_wins, uint32_t n_win, hipStream_t st);
void jl_launch_phase_group(const jl_win_phase *h_wins, uint32_t n_win, uint32_t max_blocks, hipStream_t st);
void jl_launch_assign_group(const jl_win_phase *h_wins, uint32_t n_win, uint32_t max_read_blocks, bool to_host, hipStream_t st);
void jl_launch_synth(jl_ctx *ctx, const jl_synth_plan *plan, const uint8_t *d_ref, uint32_t col0);
void jl_launch_pack_rows(jl_ctx *ctx, const uint8_t *d_rows, uint32_t *d_bad);
// interchange format (column-packed nibbles, include/juliet_hip.h) <-> the resident planes, `n` columns from column c0 on
void jl_launch_nibbles_to_planes(jl_ctx *ctx, const uint8_t *d_nib, uint64_t nib_stride, uint32_t c0, uint32_t n, uint32_t *d_bad);
void jl_launch_planes_to_nibbles(jl_ctx *ctx, uint8_t *d_nib, uint64_t nib_stride, uint32_t c0, uint32_t n);
void jl_launch_done(jl_ctx *ctx);
void jl_launch_done_on(jl_ctx *ctx, hipStream_t st);
// a run whose phase launch gave up waiting to write its ids (JL_PHASE_OVF_IDS_WAIT_TIMEOUT): the phasing stage again, the ids separate,
// behind everything on the run's stream; blocks until it is done.  The call stage's results are still resident.
extern "C" int jl_phase_rerun_ids_separate(jl_ctx *ctx);
void jl_launch_done_group(const jl_done_ent *d_ents, uint32_t n, hipStream_t st);
// capi_group.hip: `ctx` is about to be destroyed — the groups it is a window of stop being counted as launches in flight
void jl_group_forget_ctx(const jl_ctx *ctx);
extern "C" int jl_run_prepare(jl_ctx *ctx, const jl_gene *genes, uint32_t n_genes, const uint8_t *refseq, uint32_t ref_len,
                              const jl_params *prm, const uint64_t *drm_masks, int phasing, uint32_t min_reads,
                              int want_read_hap, double *n_tests_out);
extern "C" void jl_run_finish(jl_ctx *ctx, int phasing, int want_read_hap);
extern "C" int jl_run_wait_impl(jl_ctx *ctx);
extern "C" int jl_run_wait_seq(jl_ctx *ctx, uint32_t want);
void jl_launch_consensus(jl_ctx *ctx, uint8_t *d_out);
void jl_launch_clock(jl_ctx *ctx, hipStream_t st, uint32_t which);   // h_seq[8 + 2 which ..] = the device's 100 MHz clock
uint32_t jl_ingest_short_ops();
bool jl_ingest_read_is_long(const uint32_t *cigar, uint64_t n_ops);
// the matrix of `dst` (allocated, at least one read) from the records R, with the scratch of `dst` (made by the caller: capi_records.hip records_build)
void jl_launch_ingest(jl_ctx *dst, const jl_records &R, uint32_t min_qv);
uint32_t jl_ingest_sweeps(uint32_t n_cols);
size_t jl_ingest_slow_room(const jl_ctx *ctx);
extern "C" int jl_ingest_verdict(jl_ctx *ctx);
void jl_launch_regroup(jl_ctx *ctx, const uint16_t *d_hap_of_group, uint32_t n_groups, uint32_t n_haplotypes, bool phased);
void jl_launch_insertions(jl_ctx *dst, const jl_records &R);
void jl_launch_fisher_eval(jl_ctx *ctx, uint32_t n, const uint32_t *a, const uint32_t *c, const uint32_t *cov, int tail,
                           double *p, double *lp);
// per-read ids in their packed form (4 / 8 / 16 bits, see JL_ID4_MAX_H) expanded to 16-bit ids on the host
extern "C" void jl_expand_ids(const void *packed, uint32_t bits, uint64_t n_reads, uint16_t *out);
int jl_msa_alloc_strided(jl_ctx *ctx, uint64_t n_reads, uint32_t n_cols, uint64_t plane_stride, uint32_t win_begin);
// capi_xwin.hip: buffers of an exporting phase run whose plan (vp positions at columns 3k) a kernel of the caller writes
int jl_phase_groups_prepare(jl_ctx *ctx, uint32_t vp);
// the variant table of a context's last call stage on the host: a pointer into the pinned result block when the run left
// it there, else copied into `scratch`
int jl_ctx_table_host(jl_ctx *ctx, std::vector<jl_variant> *scratch, const jl_variant **rows, uint32_t *n);
// jl_run_wait_seq without touching ctx->err (threads other than the context's owner)
int jl_run_wait_seq_quiet(jl_ctx *ctx, uint32_t want, hipStream_t stream);
// `bytes` of device memory to `dst` (pageable is fine) behind everything enqueued on the context's run stream: a copy kernel into
// the context's pinned scratch + a completion word, no runtime copy path
int jl_fetch_to_host(jl_ctx *ctx, const void *d_src, size_t bytes, void *dst, size_t readable);
