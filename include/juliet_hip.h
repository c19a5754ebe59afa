/*
 * juliet_hip.h — C ABI of libjuliet_hip.so: juliet's call+phase hot path on MI355X (gfx950).
 *
 * What this replaces.  The reference exposes NO library, plugin or FFI surface for this path — only the
 * `juliet` process boundary (doc/JULIET.md:62-66) — and ships no source, so there is no
 * reference interface file:line for an entry point to mirror.  Each entry point below therefore cites the
 * reference TEXT whose behaviour it implements (doc/JULIET.md as J:line) and the docs/SPEC.md section that
 * fixes the details the text leaves open.  A host (the C++ `juliet` front end in minorseq_amd/host/, or any
 * FFI: ctypes in minorseq_amd/capi.py, cgo/JNI stubs in INTEGRATION.md) drives the path through these calls.
 *
 * Conventions.  Plain C, fixed-width PODs, no exceptions cross the boundary.  Every function returns
 * JL_OK (0) or a negative jl_status; jl_last_error(ctx) has the detail.  The caller owns every host
 * buffer; the ctx owns device memory unless a buffer is adopted.  One ctx per (thread, device); all work
 * of a ctx is ordered on one HIP stream (its own, or the caller's — e.g. torch's current stream).
 * `*_async` calls only enqueue; results are valid after jl_sync() or a `*_fetch`/blocking call.
 * There is no CPU fallback: without a usable gfx950 device every call fails with JL_ERR_DEVICE.
 */
#ifndef JULIET_HIP_H
#define JULIET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the functions declared between this push and the pop at the end of
 * the file ARE its export list (tests/test_capi_exports.py checks the equality both ways). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define JL_ABI_VERSION 5

/* symbol codes of the MSA (SPEC §1; J:99-100, 256-259, 372-381) */
enum { JL_SYM_A = 0, JL_SYM_C = 1, JL_SYM_G = 2, JL_SYM_T = 3, JL_SYM_GAP = 4, JL_SYM_MASK = 5, JL_SYM_NONE = 6 };

typedef enum {
    JL_OK = 0,
    JL_ERR_ARG = -1,      /* bad argument / shape */
    JL_ERR_DEVICE = -2,   /* no gfx950 device, HIP error */
    JL_ERR_MEMORY = -3,   /* allocation failed */
    JL_ERR_STATE = -4,    /* call order: e.g. jl_call before jl_pileup */
    JL_ERR_OVERFLOW = -5, /* an output capacity was exceeded (n_out holds the needed size) */
    JL_ERR_COMM = -6      /* RCCL failure */
} jl_status;

enum { JL_MAX_HAPLOTYPES = 702 /* [A-Z][a-z]?  J:198 */, JL_HAP_INSUFFICIENT = 0xFFFE, JL_HAP_DAMAGED = 0xFFFF };

typedef struct jl_ctx jl_ctx;
typedef struct jl_comm jl_comm;

/* gene / ORF: 1-based [begin, end) in alignment space (J:134-136) */
typedef struct {
    uint32_t begin;
    uint32_t end;
} jl_gene;

/* ErrorEstimates (SPEC §5; J:40-41, 221-225).  Values are UNPINNED, hence parameters. */
typedef struct {
    double match;
    double substitution; /* per target base */
    double deletion;     /* a read shows a whole-codon deletion by error (jl_deletion_test, docs/SPEC.md section 16); the
                            codon calls ignore indels (J:26-27) and this field */
} jl_error_model;

typedef struct {
    double alpha;           /* significance level after Bonferroni; default 0.01 */
    double n_tests;         /* Bonferroni factor; <= 0 selects sum of codons over all genes passed to jl_pileup */
    jl_error_model err;
    int32_t expected_round; /* 0 ceil (default), 1 floor, 2 nearest */
    int32_t tail;           /* 0 one-sided greater (default), 1 two-sided */
    double min_perc;        /* --min-perc: keep 100*count/coverage >  min_perc; < 0 disables (J:342-344) */
    double max_perc;        /* --max-perc: keep 100*count/coverage <  max_perc; < 0 disables (J:352-354) */
} jl_params;

/* one called variant codon (SPEC §6; J:94-98).  48 bytes, the all-gather payload row. */
typedef struct {
    uint32_t gene;      /* index into the genes passed to jl_pileup */
    uint32_t codon_pos; /* 1-based amino-acid position in the gene */
    uint32_t col;       /* window column of the codon's first base */
    uint8_t ref_codon;  /* 0..63 = 16*b0+4*b1+b2 */
    uint8_t codon;
    uint16_t flags;
    uint32_t count;
    uint32_t coverage;
    uint32_t expected;
    uint32_t pad_;
    double p_value; /* Bonferroni-adjusted, <= 1 */
    double log_p;   /* ln of the unadjusted p */
} jl_variant;

/* read categories (J:372-381) and sizes of the phasing result */
typedef struct {
    uint32_t reported_reads;
    uint32_t insufficient_reads;
    uint32_t damaged_reads;
    uint32_t marginal_gap;
    uint32_t marginal_heteroduplex;
    uint32_t marginal_partial;
    uint32_t n_positions;  /* Vp: distinct variant columns */
    uint32_t n_haplotypes; /* H */
} jl_phase_summary;

/* synthetic aligned-CCS generator (bench + tests) */
typedef struct {
    uint64_t seed;
    double sub_rate;      /* per base, uniform over the other three bases */
    double del_rate;      /* '-' */
    double mask_rate;     /* 'N' */
    double partial_rate;  /* fraction of reads that start late / end early */
    uint32_t minor_permille[4]; /* frequency of the four minor haplotypes, in 1/1000 of the reads */
    uint32_t reserved;
} jl_synth_params;

/* ---------------------------------------------------------------- context */

int jl_abi_version(void);
const char *jl_strerror(int status);
/* Number of usable gfx950 devices (0 if none). Does not create a context. */
int jl_device_count(void);
/* `stream` = NULL: the ctx creates its own non-blocking stream; else a hipStream_t owned by the caller. */
int jl_ctx_create(int device, void *stream, jl_ctx **out);
/* The hipStream_t this context orders its work on (its own or the caller's).  Contexts of one device that a thread drives
 * one after the other may share one: a stream of its own costs the runtime about 8 ms to create. */
void *jl_ctx_stream(const jl_ctx *ctx);
void jl_ctx_destroy(jl_ctx *ctx);
const char *jl_last_error(const jl_ctx *ctx);
/* Waits for everything enqueued for this context: its own stream and, after a group run, the group's. */
int jl_sync(jl_ctx *ctx);

/* ---------------------------------------------------------------- MSA residency */

/* THE resident format (ABI 5): per column three BIT PLANES — plane k holds bit k of every read's 3-bit symbol code, read i
 * in bit i & 7 of byte i >> 3; plane k of column c at base + (3 c + k) * plane_stride; reads past n_reads are padding with
 * code 6 (plane 0 clear, planes 1 and 2 set).  3 bits per cell: 112.5 MB for 100k reads x 3 kb.  Every producer (upload,
 * pack_rows, record ingest, synthetic fill) writes the planes directly and every stage (pileup, phasing, the exchange of
 * cross-window phasing) reads them; there is no second copy.  The column-packed NIBBLE layout of earlier ABI versions
 * (read i in byte i / 2, low nibble even; column stride jl_col_stride) remains the host-side INTERCHANGE format of
 * jl_msa_upload and jl_msa_download only: it is converted on the device, a bounded run of columns at a time. */

/* Bytes per column of the interchange (nibble) format for n_reads reads (ceil(n/2) rounded up to 128). */
uint64_t jl_col_stride(uint64_t n_reads);
/* Bytes per plane of the resident format the library allocates: ceil(n/1024) * 128 (whole 128-byte lines). */
uint64_t jl_plane_stride(uint64_t n_reads);
/* A host matrix in the interchange format, [n_cols][col_stride] nibbles, into resident planes owned by the ctx; symbol
 * codes outside 0..6 are rejected (JL_ERR_ARG); whatever the buffer holds past read n_reads - 1 of a column is ignored. */
int jl_msa_upload(jl_ctx *ctx, const uint8_t *colpacked, uint64_t n_reads, uint32_t n_cols, uint64_t col_stride,
                  uint32_t win_begin);
/* Allocate an uninitialised resident matrix (for jl_synth_fill / jl_msa_pack_rows). */
int jl_msa_alloc(jl_ctx *ctx, uint64_t n_reads, uint32_t n_cols, uint32_t win_begin);
/* Use caller-owned device memory (e.g. a torch tensor) holding the resident format — [n_cols][3][plane_stride] bytes,
 * 16-byte aligned, plane_stride a multiple of 16, >= ceil(n_reads / 8) and below 4 GiB, padding reads = code 6 — as the resident
 * matrix; never copied, not freed by the ctx, and the caller may rewrite it between runs. */
int jl_msa_adopt(jl_ctx *ctx, void *d_planes, uint64_t n_reads, uint32_t n_cols, uint64_t plane_stride,
                 uint32_t win_begin);
/* Device-side transpose of a host by-row matrix uint8[n_reads][n_cols] (codes 0..6) into the resident layout; a code
 * outside 0..6 is rejected as jl_msa_upload rejects it (JL_ERR_ARG, the same message, and no resident matrix is left). */
int jl_msa_pack_rows(jl_ctx *ctx, const uint8_t *rows, uint64_t n_reads, uint32_t n_cols, uint32_t win_begin);
/*
 * Aligned records -> resident matrix entirely on the device: cigar expansion (= X I D S H N; M is rejected,
 * J:53), insertions dropped and deletions '-' (J:26-27), optional QV masking to N (J:256-259), transpose.
 * pos[r]: 0-based leftmost reference position; cigar words are BAM's (len << 4 | op), read r owns
 * cigar[cig_off[r] .. cig_off[r+1]); seq4 holds BAM's 4-bit bases, read r starting at byte seq_off[r];
 * qual (optional, with qual_off) one byte per base, 0xFF = absent; bases with qual < min_qv become N (min_qv is
 * taken as at most 127: BAM qualities end at 93).
 */
int jl_msa_ingest_records(jl_ctx *ctx, uint64_t n_reads, uint32_t n_cols, uint32_t win_begin, const int32_t *pos,
                          const uint32_t *cigar, const uint64_t *cig_off, const uint8_t *seq4, const uint64_t *seq_off,
                          const uint8_t *qual, const uint64_t *qual_off, uint32_t min_qv);
/*
 * The same in pieces, so a decoder can hand over each batch of records while it inflates the next one (the upload
 * then hides under the decode; the kernels run in jl_records_finish, once the window is known).  The hints size the
 * device arrays up front (they grow when exceeded; qual_bytes_hint 0 = no qualities expected).  A chunk's offsets
 * index ITS arrays (read r of the chunk owns cigar[cig_off[r] .. cig_off[r+1]) etc., cig_off[0] need not be 0); the
 * host arrays may be reused as soon as jl_records_append returns.  Either every chunk carries qualities or none.
 * Validation and errors are those of jl_msa_ingest_records, which is begin + one append + finish.  One thread at
 * a time per context.
 */
int jl_records_begin(jl_ctx *ctx, uint64_t reads_hint, uint64_t cigar_words_hint, uint64_t seq_bytes_hint,
                     uint64_t qual_bytes_hint);
int jl_records_append(jl_ctx *ctx, uint64_t n_reads, const int32_t *pos, const uint32_t *cigar, const uint64_t *cig_off,
                      const uint8_t *seq4, const uint64_t *seq_off, const uint8_t *qual, const uint64_t *qual_off);
int jl_records_finish(jl_ctx *ctx, uint32_t n_cols, uint32_t win_begin, uint32_t min_qv);
/* One upload, several column windows (`juliet --windows K`: the BAM is decoded and uploaded once): the resident matrix
 * of `window` — another context of the same device — from the records appended to `records`, which stay until
 * jl_records_drop (or jl_records_finish on `records` itself). */
int jl_records_window(jl_ctx *records, jl_ctx *window, uint32_t n_cols, uint32_t win_begin, uint32_t min_qv);
/* The same, enqueued only (three launches on the window's stream, no allocation once a window of this shape was built on
 * `window`): the matrix is complete when the window's stream gets there, so a run enqueued behind it (jl_run_async on
 * `window`) reads it — records -> planes -> call + phase without a host round trip in between. */
int jl_records_window_async(jl_ctx *records, jl_ctx *window, uint32_t n_cols, uint32_t win_begin, uint32_t min_qv);
int jl_records_drop(jl_ctx *records);
/*
 * The QV filter decided by the caller: one bit per base in place of one quality byte and a threshold.  A set bit makes the
 * base N, exactly as qual < min_qv && qual != 0xFF does in the byte form; a caller with its own policy (per-track
 * thresholds, a precomputed mask) sets whatever bits it likes.
 * LAYOUT of `qmask`: parallel to the chunk's seq4, one bit per 4-bit base in the bases' own (query) order.  Base q of read
 * r of the chunk is bit i = 2 * (seq_off[r] - seq_off[0]) + q, stored in bit (i & 7) of byte (i >> 3): the first base of a
 * seq4 byte (its high nibble) has the even bit, and the bit of the spare low nibble of an odd-length read is ignored.  The
 * mask has no offsets of its own and begins at the chunk's first base whatever seq_off[0] is; it holds
 * jl_qmask_bytes(seq_off[n_reads] - seq_off[0]) bytes.
 * A stream is masked (every chunk through jl_records_append_masked), or carries qualities, or neither: a chunk of another
 * form, or a NULL mask, fails with JL_ERR_ARG and drops the stream.  The chunks need no alignment of their own (the
 * library starts each on a 16-byte boundary of its resident arrays).  A masked stream has no quality count to check a
 * cigar against; every other rule is jl_records_append's.  jl_records_finish / _window / _window_async: min_qv == 0 builds
 * without the filter, any other value applies the mask — one upload feeds filtered and unfiltered windows.
 */
int jl_records_append_masked(jl_ctx *ctx, uint64_t n_reads, const int32_t *pos, const uint32_t *cigar,
                             const uint64_t *cig_off, const uint8_t *seq4, const uint64_t *seq_off, const uint8_t *qmask);
/* jl_records_begin + one jl_records_append_masked + jl_records_finish. */
int jl_msa_ingest_records_masked(jl_ctx *ctx, uint64_t n_reads, uint32_t n_cols, uint32_t win_begin, const int32_t *pos,
                                 const uint32_t *cigar, const uint64_t *cig_off, const uint8_t *seq4,
                                 const uint64_t *seq_off, const uint8_t *qmask, uint32_t min_qv);
/* Host only (no device, no context).  Bytes of the mask of seq_bytes bytes of packed bases: ceil(seq_bytes / 4). */
uint64_t jl_qmask_bytes(uint64_t seq_bytes);
/* The byte form's rule as a mask in the layout above: read r has qual_off[r+1] - qual_off[r] bases (at most two per byte
 * of its seq4), min_qv is taken as at most 127, 0xFF never masks; every other bit of the first
 * jl_qmask_bytes(seq_off[n_reads] - seq_off[0]) bytes is cleared (all qmask_bytes are written).  JL_ERR_ARG when
 * qmask_bytes is less than that, or the offsets decrease. */
int jl_qmask_from_quals(uint64_t n_reads, const uint64_t *seq_off, const uint8_t *qual, const uint64_t *qual_off,
                        uint32_t min_qv, uint8_t *qmask, uint64_t qmask_bytes);
/*
 * Insertions are not part of the matrix (J:26-27) but `fuse` "includes in-frame insertions with a certain distance to
 * each other" (doc/FUSE.md:19): with tracking on, jl_msa_ingest_records also counts them per window column — an
 * insertion sits BEFORE the column of the next reference base.  len_hist[n_cols][32]: insertions by length (31 = longer
 * than 30); base_counts[n_cols][30][4]: inserted bases A C G T by offset.  Either pointer may be NULL.
 */
int jl_msa_track_insertions(jl_ctx *ctx, int on);
int jl_insertions_fetch(jl_ctx *ctx, uint32_t *len_hist, uint32_t *base_counts);
/*
 * Take reads: the resident matrix of `dst` made of chosen reads of other resident matrices of the same device — a downsample
 * ("downsample it to 6000x", doc/JULIETFLOW.md:23-25; doc/JULIET.md:244-251), a mixture of clones at a given ratio and coverage
 * (doc/MIXDATA.md), a bootstrap resample — without another decode, upload or ingest: a read is one bit position in the three
 * planes of a column, so this is a bit gather over planes that are in HBM already (docs/SPEC.md §12).
 * Destination reads are the parts one after the other, in argument order; within a part read j is read idx[j] of the part's
 * source.  idx may be in any order and may repeat.  `dst` becomes a resident window of sum(n) reads with the sources' n_cols and
 * win_begin, owned by `dst` (plane stride jl_plane_stride(sum n)), padded with code 6; whatever `dst` held, and its stage
 * results and insertion counters, are gone.  Every stage accepts it as any other window.  The index arrays may be reused on return.
 * JL_ERR_ARG (jl_last_error(dst) says which): no parts, more than JL_TAKE_MAX_PARTS, sum(n) = 0 or above 2^31 - 1; an index at or
 * beyond its source's reads; sources of different n_cols or win_begin, or on another device than `dst`; `dst` among the sources.
 * JL_ERR_STATE: a source without a resident matrix.  A call refused with either leaves `dst` as it was.
 * jl_msa_take waits for the sources' streams, enqueues on dst's and waits for it; jl_msa_take_async only enqueues on dst's
 * stream, as jl_records_window_async does (one upload of the indices and one launch; the sources must be complete when dst's
 * stream gets there — e.g. they share the stream — and stay unchanged until it has).
 */
enum { JL_TAKE_MAX_PARTS = 16 };
typedef struct {
    jl_ctx *src;          /* a context with a resident matrix */
    const uint32_t *idx;  /* [n] reads of src */
    uint64_t n;
} jl_take_part;
int jl_msa_take(jl_ctx *dst, const jl_take_part *parts, uint32_t n_parts);
int jl_msa_take_async(jl_ctx *dst, const jl_take_part *parts, uint32_t n_parts);
/* Host only (no device, no context), docs/SPEC.md §12.  Which k of n_reads reads a downsample keeps: read i has the key
 * splitmix64(seed + i) (the generator of the synthetic reads), kept are the k reads with the smallest (key, i), written to
 * idx in ascending i; *n_out = min(k, n_reads) of them (idx has room for that many; k >= n_reads keeps every read).  Samples
 * of one seed are nested — the sample of k reads contains the sample of every smaller k — and no device has a say in them.
 * JL_ERR_ARG: n_reads above 2^32 - 1 (an index is 32 bits). */
int jl_sample_reads(uint64_t n_reads, uint64_t k, uint64_t seed, uint32_t *idx, uint64_t *n_out);
/* Host only.  Reads per source of a mixture of `coverage` reads in which every minor clone has `percentage` percent
 * (doc/MIXDATA.md:10-22): counts[1 .. n_sources) = floor(coverage * percentage / 100), counts[0] — the major clone — the rest,
 * so that the counts sum to `coverage` exactly.  JL_ERR_ARG: no source, a percentage outside (0, 100), or minors that
 * alone exceed the coverage. */
int jl_mix_counts(uint32_t n_sources, uint64_t coverage, double percentage, uint64_t *counts);
/* The resident matrix back on the host in the interchange format, [n_cols][jl_col_stride(n_reads)] nibbles (tests). */
int jl_msa_download(jl_ctx *ctx, uint8_t *colpacked, uint64_t bytes);
/* The first `bytes` bytes of the resident planes as they are, [n_cols][3][plane_stride] (owned or adopted): one copy behind
 * what the context's stream holds and a wait, no conversion — padding reads and whatever an adopted matrix holds past them
 * included (tests).  JL_ERR_ARG: bytes > 3 * n_cols * plane_stride, or no resident matrix. */
int jl_msa_download_planes(jl_ctx *ctx, uint8_t *planes, uint64_t bytes);
/* Fill the resident matrix with synthetic reads, on the device. `ref` = n_cols base codes (host). */
int jl_synth_fill(jl_ctx *ctx, const jl_synth_params *sp, const uint8_t *ref);
/* The same reads seen through a WINDOW of a longer reference (BASELINE.json configs[3]/[4]: one reference whose
 * reads span every window): `ref` = ref_len base codes of the whole reference, the resident matrix is its columns
 * [win_begin, win_begin + n_cols).  Windows filled with the same parameters hold the same reads. */
int jl_synth_fill_window(jl_ctx *ctx, const jl_synth_params *sp, const uint8_t *ref, uint32_t ref_len);

/* ---------------------------------------------------------------- call */

/*
 * Column pileup + per-codon histograms for every evaluated position of `genes` (SPEC §2-3; J:94-100).
 * `refseq`: base codes of the whole reference (0..3, other = non-ACGT), 0-based, or NULL for
 * majority-codon mode (J:133-134).  Enqueues; returns without waiting.
 */
int jl_pileup_async(jl_ctx *ctx, const jl_gene *genes, uint32_t n_genes, const uint8_t *refseq, uint32_t ref_len);
/* Number of evaluated positions P of the last jl_pileup_async. */
uint32_t jl_n_positions(const jl_ctx *ctx);
/*
 * Wait, then copy out: col_counts[n_cols][6] (A C G T - N), pos_gene/pos_codon/pos_col[P] (codon_pos 1-based),
 * hist[P][64], coverage[P].  Any pointer may be NULL.
 */
int jl_pileup_fetch(jl_ctx *ctx, uint32_t *col_counts, uint32_t *pos_gene, uint32_t *pos_codon, uint32_t *pos_col,
                    uint32_t *hist, uint32_t *coverage);
/*
 * By-product of the pileup: per-column consensus (majority of A C G T -), the part of `fuse`
 * (doc/FUSE.md:17-20) that needs no insertion tracking.  out[n_cols]: 0..3 base, 4 = majority deletion
 * ("major deletions are being removed"), 5 = column without coverage.  Blocking.
 */
int jl_consensus_fetch(jl_ctx *ctx, uint8_t *out);
/*
 * Column pileup of the resident matrix BY CLASS OF READS (docs/SPEC.md §13): what a haplotype — or the damaged reads, or any
 * other set of reads — looks like along the whole window, not only at the called codons.  A read is one bit position in every
 * plane row, so a class is a bit mask in the plane-row layout and a per-class count is popcount(symbol word & class mask) over
 * the words the plain pileup streams: one pass over the matrix for up to 16 classes, ceil(n_classes / 16) passes in all.
 * label[n_reads]: read i belongs to class label[i] when label[i] < n_classes and to no class otherwise, so the ids of
 * jl_phase_fetch can be passed as they are (JL_HAP_INSUFFICIENT / JL_HAP_DAMAGED fall out).  The labels are copied before the
 * call returns; it uploads and enqueues on the context's stream, into buffers of its own (grown on demand, released with the
 * context), and touches nothing else: the matrix, the insertion counters, the results of an earlier jl_pileup_async /
 * jl_call_async / jl_phase_async / jl_run_async and what their fetch calls return afterwards, and the context's captured
 * graph stay as they are.  Every kind of resident matrix is accepted, an adopted one with its own plane stride included.
 * JL_ERR_STATE: no resident matrix.  JL_ERR_ARG (jl_last_error says which): label == NULL, n_classes == 0 or above
 * JL_CLASS_MAX.  A refused call changes nothing.
 */
enum { JL_CLASS_MAX = 704 };   /* JL_MAX_HAPLOTYPES + the two read categories */
int jl_class_pileup_async(jl_ctx *ctx, const uint16_t *label, uint32_t n_classes);
/* Wait and copy out: counts[n_classes][n_cols][6] (A C G T - N, as col_counts of jl_pileup_fetch), class_reads[n_classes]
 * (reads per class), both of the last jl_class_pileup_async.  Either pointer may be NULL.  JL_ERR_STATE: none was enqueued. */
int jl_class_pileup_fetch(jl_ctx *ctx, uint32_t *counts, uint32_t *class_reads);
/* Host only (no device, no context).  Per-column consensus of ONE [n_cols][6] count table by the rule of jl_consensus_fetch:
 * majority of A C G T -, lowest code on ties (N does not vote); out[n_cols]: 0..3 base, 4 = majority deletion, 5 = nobody
 * covers the column. */
int jl_consensus_of_counts(const uint32_t *col_counts, uint32_t n_cols, uint8_t *out);
/*
 * Codon histograms of the resident matrix BY CLASS OF READS at chosen codon starts (docs/SPEC.md §24): the codon counterpart of
 * jl_class_pileup_async — a column majority is not a codon majority — in one pass over the planes for up to 16 classes.
 * label[n_reads] and n_classes are jl_class_pileup_async's, word for word: read i belongs to class label[i] when label[i] <
 * n_classes and to no class otherwise (the ids of jl_phase_fetch can be passed as they are); n_classes is 1 .. JL_CLASS_MAX.
 * col[n_pos]: window columns of codon starts, strictly ascending, each + 2 < n_cols; positions of different frames may overlap
 * (c, c + 1, c + 2 can all be starts).  A read of class k whose three codes at col[p], col[p] + 1, col[p] + 2 are all < 4 adds
 * one to hist[k][p][codon], codon = 16 * first + 4 * second + third as in hist of jl_pileup_fetch; a read with a '-', an N or
 * an uncovered cell there counts nowhere, so the sum over codons of hist[k][p] is class k's coverage at p, and with every read
 * in one class hist[0] is jl_pileup_fetch's hist at the same columns.  32 bits, exact, independent of launch shape and order
 * and of the seed codon the kernel counts by popcount.  Reads past n_reads count nowhere: the padding, and whatever an adopted
 * matrix holds behind the last read of a plane row.
 * The contract is jl_class_pileup_async's: the inputs are copied before the call returns; it enqueues on the context's stream
 * into buffers of its own (grown on demand, released with the context) and touches nothing else — the matrix, the insertion
 * counters, earlier stage results, the class pileup's buffers and the captured graph stay as they are.  Every kind of resident
 * matrix is accepted, an adopted one with its own plane stride included.
 * JL_ERR_STATE: no resident matrix.  JL_ERR_ARG (jl_last_error says which): label == NULL; col == NULL; n_classes 0 or above
 * JL_CLASS_MAX; n_pos 0; n_classes * n_pos above JL_CLASS_CODONS_CELLS (256 MiB of counters); a column with c + 2 >= n_cols;
 * columns not strictly ascending.  A refused call changes nothing: what an earlier call enqueued can still be fetched.
 * A call that fails later, in the runtime (JL_ERR_MEMORY, JL_ERR_DEVICE: its buffers could not grow, an upload or a launch
 * failed), leaves NOTHING fetchable: the table of the call before it lives in the buffer this one was about to overwrite.
 */
enum { JL_CLASS_CODONS_CELLS = 1 << 20 };
int jl_class_codons_async(jl_ctx *ctx, const uint16_t *label, uint32_t n_classes, const uint32_t *col, uint32_t n_pos);
/* Wait and copy out: hist[n_classes][n_pos][64] and class_reads[n_classes] (reads per class), both of the last
 * jl_class_codons_async.  Either pointer may be NULL.  JL_ERR_STATE: none was enqueued. */
int jl_class_codons_fetch(jl_ctx *ctx, uint32_t *hist /* [n_classes][n_pos][64] */, uint32_t *class_reads /* [n_classes] */);
/*
 * Which reported haplotype a read agrees with WHERE IT CAN BE READ (docs/SPEC.md §14): phasing drops a read with a deletion, a
 * filtered N or an uncovered cell at any variant position (JL_HAP_DAMAGED); most such reads are clean at the other positions and
 * match exactly one reported haplotype there.  pos_cols[n_pos]: window columns of codon starts, strictly ascending, each + 2 <
 * n_cols (overlapping codons allowed); pattern[n_hap] rows of n_pos codon indices 0..63, pattern_stride bytes apart — pos_cols
 * and hap_pattern of jl_phase_fetch can be passed as they are.  Per read i: position p is INFORMATIVE iff the three codes at
 * pos_cols[p] .. + 2 are all < 4 (a gap, an N and an uncovered cell alike make it open); k_i = informative positions; haplotype
 * h AGREES iff its codon equals the read's at every informative position; m_i = agreeing haplotypes.  rescue[i] =
 * JL_RESCUE_UNINFORMATIVE if k_i < min_positions, else JL_RESCUE_NONE if m_i == 0, else that h if m_i == 1, else
 * JL_RESCUE_AMBIGUOUS.  Every read is evaluated, not only the damaged ones: a clean read of haplotype h gets h.
 * The contract is jl_class_pileup_async's: the inputs are copied before the call returns; it enqueues on the context's stream
 * into buffers of its own (grown on demand, released with the context) and touches nothing else — the matrix, the insertion
 * counters, earlier stage results and the captured graph stay as they are.  Every kind of resident matrix is accepted.
 * JL_ERR_STATE: no resident matrix.  JL_ERR_ARG (jl_last_error says which): a NULL array; n_pos 0 or above 4096; n_hap 0 or
 * above JL_MAX_HAPLOTYPES; pattern_stride < n_pos; min_positions 0 or above n_pos; a column with c + 2 >= n_cols; columns not
 * strictly ascending; a pattern byte above 63.  A refused call changes nothing: what an earlier call enqueued can still be fetched.
 */
enum { JL_RESCUE_UNINFORMATIVE = 0xFFFB, JL_RESCUE_NONE = 0xFFFC, JL_RESCUE_AMBIGUOUS = 0xFFFD };
int jl_phase_rescue_async(jl_ctx *ctx, const uint32_t *pos_cols, uint32_t n_pos, const uint8_t *pattern,
                          uint32_t pattern_stride, uint32_t n_hap, uint32_t min_positions);
/* Wait and copy out, all of the last jl_phase_rescue_async: rescue[n_reads]; hap_reads[n_hap] = reads with rescue == h;
 * tally[4] = reads {assigned, ambiguous, none, uninformative}, summing to n_reads.  Any pointer may be NULL.
 * JL_ERR_STATE: none was enqueued. */
int jl_phase_rescue_fetch(jl_ctx *ctx, uint16_t *rescue, uint32_t *hap_reads, uint64_t *tally /* [4] */);
/*
 * Which reported haplotype a read is NEAREST to, within a mismatch budget (docs/SPEC.md §22): one sequencing or PCR error at one
 * variant position gives a read a pattern of its own, which never reaches min_reads (JL_HAP_INSUFFICIENT); such a read is one
 * codon away from the haplotype it came from.  pos_cols, pattern, pattern_stride, n_hap and min_positions are
 * jl_phase_rescue_async's, as are INFORMATIVE and k_i.  Per read i: d(i, h) = informative positions at which the read's codon
 * differs from pattern[h][p] (a codon position counts once, however many of its bases differ); dmin_i = min over h of d(i, h);
 * n_i = haplotypes at dmin_i.  The first line that holds decides nearest[i] and dist[i]:
 *   k_i < min_positions      JL_RESCUE_UNINFORMATIVE   0xFF
 *   dmin_i > max_distance    JL_RESCUE_NONE            max_distance + 1
 *   n_i == 1                 that h                    dmin_i
 *   otherwise                JL_RESCUE_AMBIGUOUS       dmin_i
 * Two equal pattern rows tie.  With max_distance 0, nearest is jl_phase_rescue_async's rescue.  Every read is evaluated.
 * The contract is jl_phase_rescue_async's: the inputs are copied before the call returns; it enqueues on the context's stream
 * into buffers of its own and touches nothing else — the matrix, earlier stage results, the captured graph and the last
 * rescue's results stay as they are.  JL_ERR_STATE: no resident matrix.  JL_ERR_ARG (jl_last_error says which): what
 * jl_phase_rescue_async refuses, and max_distance above JL_NEAREST_MAX_DISTANCE.  A refused call changes nothing: what an
 * earlier call enqueued can still be fetched.
 */
enum { JL_NEAREST_MAX_DISTANCE = 7 };
int jl_phase_nearest_async(jl_ctx *ctx, const uint32_t *pos_cols, uint32_t n_pos, const uint8_t *pattern,
                           uint32_t pattern_stride, uint32_t n_hap, uint32_t min_positions, uint32_t max_distance);
/* Wait and copy out, all of the last jl_phase_nearest_async (D = its max_distance): nearest[n_reads]; dist[n_reads];
 * hap_reads[n_hap][D + 1], rows D + 1 apart = reads with nearest == h and dist == d; tally[4] = reads {assigned, ambiguous,
 * none, uninformative}, summing to n_reads.  Any pointer may be NULL.  JL_ERR_STATE: none was enqueued. */
int jl_phase_nearest_fetch(jl_ctx *ctx, uint16_t *nearest, uint8_t *dist, uint32_t *hap_reads /* [n_hap][D+1] */,
                           uint64_t *tally /* [4] */);
/*
 * Which reads are RECOMBINANTS of two reported haplotypes (docs/SPEC.md §23): PCR-mediated recombination (template switching) gives
 * a molecule the codons of one clone at the left variant positions and of another at the right.  The rescue asks whether one
 * haplotype agrees with the read everywhere and the nearest call counts differences wherever they lie; this call is sensitive to
 * ORDER.  pos_cols, pattern, pattern_stride, n_hap and min_positions are jl_phase_rescue_async's, as are INFORMATIVE and k_i.
 * Per read i and haplotype h: agree(i, h, p) iff p is open for the read or its codon there equals pattern[h][p];
 * pre(i, h) = the smallest p with !agree, n_pos when there is none; suf(i, h) = n_pos - 1 - the largest p with !agree, n_pos when
 * there is none; P_i = max over h of pre, S_i = max over h of suf, nP_i and nS_i = the haplotypes attaining each maximum.
 * prefix[i] = P_i and suffix[i] = S_i, always.  The first line that holds decides left[i] and right[i]:
 *   k_i < min_positions      JL_RESCUE_UNINFORMATIVE, both
 *   P_i == n_pos             JL_RECOMB_WHOLE, both (some haplotype agrees with the whole read; then S_i == n_pos too)
 *   P_i + S_i < n_pos        JL_RESCUE_NONE, both (no single breakpoint explains the read)
 *   otherwise                left = the h at P_i if nP_i == 1, else JL_RESCUE_AMBIGUOUS; right likewise by S_i and nS_i
 * The last line is a recombinant: every b in [n_pos - S_i, P_i] is a possible breakpoint, in front of position b.
 * The contract is jl_phase_nearest_async's: the inputs are copied before the call returns; it enqueues on the context's stream
 * into buffers of its own and touches nothing else — the matrix, earlier stage results, the captured graph, the last rescue's and
 * the last nearest call's results stay as they are.  JL_ERR_STATE: no resident matrix.  JL_ERR_ARG (jl_last_error says which):
 * what jl_phase_rescue_async refuses.  A refused call changes nothing: what an earlier call enqueued can still be fetched.
 */
enum { JL_RECOMB_WHOLE = 0xFFFA };
int jl_phase_recombinants_async(jl_ctx *ctx, const uint32_t *pos_cols, uint32_t n_pos, const uint8_t *pattern,
                                uint32_t pattern_stride, uint32_t n_hap, uint32_t min_positions);
/* Wait and copy out, all of the last jl_phase_recombinants_async: left, right, prefix, suffix [n_reads] each;
 * parent_reads[n_hap][2] = the reads with left == h (column 0) and right == h (column 1) among the recombinants with BOTH parents
 * unique; tally[5] = reads {recombinant (both parents unique), ambiguous_parent, whole, none, uninformative}, summing to n_reads.
 * Any pointer may be NULL.  JL_ERR_STATE: none was enqueued. */
int jl_phase_recombinants_fetch(jl_ctx *ctx, uint16_t *left, uint16_t *right, uint16_t *prefix, uint16_t *suffix,
                                uint32_t *parent_reads /* [n_hap][2] */, uint64_t *tally /* [5] */);
/* Is a reported haplotype itself a recombinant of two more frequent ones (docs/SPEC.md §23)?  prefix / suffix are the largest
 * common prefix / suffix length of row h with a candidate parent's row, left / right the lowest candidate attaining each. */
typedef struct {
    uint32_t flagged;        /* 1: candidates exist and prefix + suffix >= n_pos */
    uint32_t left, right;    /* candidate parents (0 when there is no candidate) */
    uint32_t prefix, suffix; /* (0 when there is no candidate) */
} jl_hap_recombinant;
/* Host only (no device, no context): out[n_hap] from pattern[n_hap] rows of n_pos codons, pattern_stride bytes apart, and
 * hap_count[n_hap].  The candidate parents of h are the a != h with hap_count[a] >= min_parent_ratio * hap_count[h] (the product
 * in IEEE double).  JL_ERR_ARG (jl_last_error(NULL) says which): a NULL array; min_parent_ratio < 1 (or NaN); n_pos 0 or above
 * 4096; n_hap 0 or above JL_MAX_HAPLOTYPES; pattern_stride < n_pos. */
int jl_haplotype_recombinants(const uint8_t *pattern, uint32_t pattern_stride, uint32_t n_hap, uint32_t n_pos,
                              const uint32_t *hap_count, double min_parent_ratio, jl_hap_recombinant *out);
/*
 * Pairwise linkage of called variants over EVERY READ COVERING BOTH (docs/SPEC.md §15): do variant v and variant w occur on the
 * same molecules?  The co-occurrence of jl_phase_fetch counts the reads of the reported haplotypes only — reads that can be read
 * at all Vp positions, in groups of min_reads; a pair needs only the reads that can be read at its TWO positions.
 * pos_cols[n_pos]: window columns of codon starts, strictly ascending, each + 2 < n_cols (overlapping codons allowed);
 * var_pos[n_var]: for each variant an index into pos_cols, non-decreasing (the variant table's order, several variants per
 * position); var_codon[n_var]: codons 0..63.  1 <= n_pos <= JL_LINK_MAX, 1 <= n_var <= JL_LINK_MAX.  Per read i: it is
 * INFORMATIVE at p iff its three codes at pos_cols[p] .. + 2 are all < 4 (jl_phase_rescue_async's definition); it CARRIES v iff
 * it is informative at var_pos[v] and its codon there equals var_codon[v].  Outputs, 32 bits, exact, independent of launch shape
 * and order:
 *   both[n_pos][n_pos]   reads informative at p and q; symmetric; both[p][p] = the codon coverage
 *   carry[n_var][n_pos]  reads that carry v and are informative at q; carry[v][var_pos[v]] = the variant's count
 *   joint[n_var][n_var]  reads that carry v and w; symmetric; joint[v][v] = the count; 0 for two different codons at one position
 * Reads past n_reads count nowhere: the padding, and whatever an adopted matrix holds past byte ceil(n_reads / 8) of a plane row.
 * Only the upper triangle of the symmetric outputs is computed; it is mirrored on store, on the device: the fetch copies whole tables.
 * The contract is jl_class_pileup_async's: the inputs are copied before the call returns; it enqueues on the context's stream
 * into buffers of its own (grown on demand, released with the context) and touches nothing else — the matrix, the insertion
 * counters, earlier stage results and the captured graph stay as they are.  Every kind of resident matrix is accepted.
 * JL_ERR_STATE: no resident matrix.  JL_ERR_ARG (jl_last_error says which): a NULL array; n_pos or n_var 0 or above
 * JL_LINK_MAX; a column with c + 2 >= n_cols; columns not strictly ascending; var_pos[v] >= n_pos, or var_pos decreasing; a
 * codon above 63.  A refused call changes nothing: what an earlier call enqueued can still be fetched.
 */
enum { JL_LINK_MAX = 1024 };
int jl_variant_linkage_async(jl_ctx *ctx, const uint32_t *pos_cols, uint32_t n_pos, const uint32_t *var_pos,
                             const uint8_t *var_codon, uint32_t n_var);
/* Wait and copy out, all of the last jl_variant_linkage_async: both[n_pos][n_pos], carry[n_var][n_pos], joint[n_var][n_var].
 * Any pointer may be NULL.  JL_ERR_STATE: none was enqueued. */
int jl_variant_linkage_fetch(jl_ctx *ctx, uint32_t *both, uint32_t *carry, uint32_t *joint);
/* The 2 x 2 table of a pair (v, w) at different positions p != q and its statistics: n = both[p][q], n11 = joint[v][w],
 * n10 = carry[v][q] - n11, n01 = carry[w][p] - n11, n00 = n - n11 - n10 - n01.  D_num = n11 n - (n11 + n10)(n11 + n01), in exact
 * integers; r2 = D_num^2 / ((n11 + n10)(n01 + n00)(n11 + n01)(n10 + n00)), 0 when a margin is 0; d_prime = D_num / D_max with
 * D_max = min((n11 + n10)(n10 + n00), (n01 + n00)(n11 + n01)) when D_num >= 0, min((n11 + n10)(n11 + n01), (n01 + n00)(n10 + n00))
 * when D_num < 0, and 0 when D_max is 0; p_positive = P(X >= n11) and p_negative = P(X <= n11), X hypergeometric with the
 * table's margins: the two one-sided Fisher tests, NOT Bonferroni-corrected. */
typedef struct {
    uint32_t n, n11, n10, n01, n00, pad_;
    double r2, d_prime, p_positive, p_negative;
} jl_link_pair;
/* Host only (no device, no context): *out = the pair (v, w) of the tables of jl_variant_linkage_fetch.  JL_ERR_ARG
 * (jl_last_error(NULL) says which): a NULL array; v or w >= n_var; var_pos[v] == var_pos[w]. */
int jl_linkage_stats(const uint32_t *both, const uint32_t *carry, const uint32_t *joint, const uint32_t *var_pos,
                     uint32_t n_pos, uint32_t n_var, uint32_t v, uint32_t w, jl_link_pair *out);
/*
 * Whole-codon deletions at EVERY CODON START of the resident matrix (docs/SPEC.md §16): the codon calls skip a read with a '-' in
 * the codon (J:26-27), so a clean three-base deletion — a real allele — shows only as a dip in coverage, lumped together with the
 * frame-shifting damage around it.  For every column c with c + 2 < n_cols and every read, by the three codes at c, c + 1, c + 2
 * the read counts in at most one of
 *   codon    all three < 4 (the codon coverage of jl_pileup_fetch, both[p][p] of jl_variant_linkage_fetch)
 *   del3     all three == 4
 *   partial  none is 5, none is 6, at least one is 4 and at least one is < 4: a deletion that breaks this codon
 * and in span when none of the three is 6.  A read with an N in the codon counts in span only, a code-6 cell counts nowhere.
 * cnt[n_cols - 2][4] = {codon, del3, partial, span}, 32 bits, exact, independent of launch shape and order.  There is no position
 * list: every column is a codon start of some frame, the host picks the ones it wants.  Reads past n_reads count nowhere: the
 * padding, and whatever an adopted matrix holds past byte ceil(n_reads / 8) of a plane row or past the last read in its last byte.
 * The contract is jl_class_pileup_async's: it enqueues on the context's stream into a buffer of its own (grown on demand, released
 * with the context) and touches nothing else — the matrix, the insertion counters, earlier stage results and the captured graph stay
 * as they are.  Every kind of resident matrix is accepted, an adopted one with its own plane stride included.
 * JL_ERR_STATE: no resident matrix.  JL_ERR_ARG: fewer than 3 columns.  A refused call changes nothing.
 */
int jl_codon_deletions_async(jl_ctx *ctx);
/* Wait and copy out cnt[n_cols - 2][4] of the last jl_codon_deletions_async (NULL: only wait).  JL_ERR_STATE: none was enqueued. */
int jl_codon_deletions_fetch(jl_ctx *ctx, uint32_t *cnt /* [n_cols-2][4] */);
/* One position of that table tested against the error model: coverage = codon + del3, expected = round_mode(coverage *
 * prm->err.deletion) clamped to [0, coverage] (prm->expected_round, the product in IEEE double), the table [[del3, coverage -
 * del3], [expected, coverage - expected]], p by prm->tail from the routines of the codon test, p_value = min(1, p * n_tests),
 * called = del3 > 0 and p_value < prm->alpha and the prm->min_perc / max_perc filters on 100 del3 / coverage (strict, as the
 * codon calls).  coverage == 0: not called, p_value 1, log_p 0. */
typedef struct {
    uint32_t count;     /* del3 */
    uint32_t coverage;  /* codon + del3 */
    uint32_t expected;
    uint32_t partial;   /* reads whose deletion breaks this codon: not part of the test */
    uint32_t called;    /* 0 or 1 */
    uint32_t pad_;
    double p_value;     /* Bonferroni-adjusted, <= 1 */
    double log_p;       /* ln of the unadjusted p */
} jl_deletion_call;
/* Host only (no device, no context).  n_tests: the Bonferroni factor, RESOLVED (the codon test's own: prm->n_tests is not read).
 * JL_ERR_ARG (jl_last_error(NULL) says which): a NULL argument; n_tests <= 0; prm->err.deletion outside [0, 1]; codon + del3
 * above 2^32 - 1. */
int jl_deletion_test(const uint32_t cnt[4], const jl_params *prm, double n_tests, jl_deletion_call *out);
/*
 * Deletions BY EXTENT (docs/SPEC.md §25): the table above sees a deletion codon by codon; this call names it by where it starts
 * and how long it is.  Per read i < n_reads a RUN is a maximal stretch [s, s + len) of columns whose cells are all code 4.  A run
 * is BOUNDED iff s >= 1, s + len <= n_cols - 1 and the cells at s - 1 and at s + len are not code 6 (they are a base or an N
 * then); any other run is OPEN: it touches the window's edge or an uncovered cell, its true extent is unknown, and it is never
 * an allele.  Results, exact integers independent of launch shape and order:
 *   runs[2]        {bounded, open}: the runs of each kind over all reads
 *   open[n_cols]   reads whose cell at c is code 4 and lies in an open run
 *   rows           one {col = s, len, count, flank} per distinct (s, len) among the bounded runs, ascending by (col, len):
 *                  count = the reads with exactly that run, flank = the reads whose cells at s - 1 and s + len are both != 6
 * Grouping is on the full key, never on a hash; the caller gives no capacity and no allele is ever dropped.  Reads past n_reads
 * count nowhere: the padding, and whatever an adopted matrix holds past byte ceil(n_reads / 8) of a plane row or past the last
 * read in its last byte.  Any n_cols >= 1 is accepted (below 3 columns no run is bounded and the table is empty).
 * The contract is jl_codon_deletions_async's: buffers of its own on the context's stream, nothing else of the context is touched,
 * every kind of resident matrix is accepted.  ONE WAIT: the table is sized from the number of runs of the matrix, so the call
 * enqueues a kernel that counts them and waits for that single count on the context's stream; the walk over the runs, the flank
 * counts and the rows are then enqueued, not waited for, and the matrix is not needed again at fetch time.
 * JL_ERR_STATE: no resident matrix.  JL_ERR_MEMORY: no room for the table.  A refused call changes nothing.
 */
typedef struct {
    uint32_t col;     /* s: the first deleted column */
    uint32_t len;
    uint32_t count;   /* reads with exactly this run */
    uint32_t flank;   /* reads covered (code != 6) at s - 1 and at s + len */
} jl_deletion_allele;
int jl_deletion_alleles_async(jl_ctx *ctx);
/* Wait and copy out the results of the last jl_deletion_alleles_async, in THAT call's n_cols, whatever was enqueued behind it and
 * whatever matrix is resident now.  runs, open: NULL = not wanted.  *n_rows = the rows of the table; rows == NULL: the count
 * only.  JL_ERR_STATE: none was enqueued.  JL_ERR_ARG: cap below the rows (nothing is lost: fetch again with room). */
int jl_deletion_alleles_fetch(jl_ctx *ctx, uint64_t runs[2], uint32_t *open /* [n_cols] */, jl_deletion_allele *rows, uint32_t cap,
                              uint32_t *n_rows);
/* One allele tested against a rate of such deletions by error: coverage = flank, expected = round_mode(coverage * rate) clamped
 * to [0, coverage] (prm->expected_round, the product in IEEE double), the table [[count, coverage - count], [expected, coverage -
 * expected]], p by prm->tail from the routines of the codon test, p_value = min(1, p * n_tests), called = count > 0 and p_value <
 * prm->alpha and the prm->min_perc / max_perc filters on 100 count / coverage (strict).  coverage == 0: not called, p_value 1. */
typedef struct {
    uint32_t count;
    uint32_t coverage;  /* flank */
    uint32_t expected;
    uint32_t called;    /* 0 or 1 */
    double p_value;     /* Bonferroni-adjusted, <= 1 */
    double log_p;       /* ln of the unadjusted p */
} jl_deletion_allele_call;
/* Host only (no device, no context).  n_tests: the Bonferroni factor, RESOLVED.  JL_ERR_ARG (jl_last_error(NULL) says which): a
 * NULL argument; n_tests <= 0; rate outside [0, 1]; count > flank. */
int jl_deletion_allele_test(uint32_t count, uint32_t flank, const jl_params *prm, double rate, double n_tests,
                            jl_deletion_allele_call *out);
/*
 * PER-READ counters over the whole resident window (docs/SPEC.md §20): every other stage looks at the matrix by column; a read that
 * disagrees with the window at dozens of columns (off-target, chimeric, hypermutated, badly aligned at its ends) raises several
 * minor codons at once, and this is the call that shows it.  For read i, summed over all n_cols columns, with `code` its cell
 * (0..3 base, 4 '-', 5 N, 6 uncovered) and compare[c] the column's compare code:
 *   JL_READ_BASES       code < 4
 *   JL_READ_GAPS        code == 4
 *   JL_READ_MASKED      code == 5
 *   JL_READ_COMPARED    code < 4 and compare[c] < 4
 *   JL_READ_MISMATCHES  code < 4 and compare[c] < 4 and code != compare[c]
 * A compare[c] of 4 or above means "this column is not compared": the output of jl_consensus_fetch / jl_consensus_of_counts (4 =
 * majority deletion, 5 = uncovered) and a reference slice with non-ACGT codes can be passed as they are.  compare == NULL: no column
 * is compared, `compared` and `mismatches` are zero.  The covered cells of a read are bases + gaps + masked; a code-6 cell counts
 * nowhere.  Reads past n_reads count nowhere: the padding, and whatever an adopted matrix holds past the last read of a plane row.
 * stats[JL_READ_STATS][n_reads], struct of arrays: counter k of read i at stats[k * n_reads + i], 32 bits, exact, independent of
 * launch shape and order.
 * The contract is jl_class_pileup_async's: compare[n_cols] is copied before the call returns; it enqueues on the context's stream
 * into buffers of its own (grown on demand, released with the context) and touches nothing else — the matrix, the insertion
 * counters, earlier stage results and the captured graph stay as they are.  Every kind of resident matrix is accepted, an adopted
 * one with its own plane stride included.
 * JL_ERR_STATE: no resident matrix.  A refused call changes nothing.
 */
enum { JL_READ_BASES = 0, JL_READ_GAPS = 1, JL_READ_MASKED = 2, JL_READ_COMPARED = 3, JL_READ_MISMATCHES = 4, JL_READ_STATS = 5 };
int jl_read_stats_async(jl_ctx *ctx, const uint8_t *compare /* [n_cols] or NULL */);
/* Wait and copy out stats[JL_READ_STATS][n_reads] of the last jl_read_stats_async (NULL: only wait).  JL_ERR_STATE: none was enqueued. */
int jl_read_stats_fetch(jl_ctx *ctx, uint32_t *stats /* [JL_READ_STATS][n_reads] */);
/* Which reads a rule keeps, from that table.  A read is kept when it passes every rule that is switched on; the products are
 * evaluated in IEEE double, left to right, as written (a read with compared == 0 passes a percentage rule: 0 <= 0). */
typedef struct {
    uint32_t min_bases;          /* keep bases >= min_bases; 0 disables */
    uint32_t max_mismatches;     /* keep mismatches <= max_mismatches; UINT32_MAX disables */
    double max_mismatch_perc;    /* keep 100.0 * mismatches <= x * compared; < 0 disables */
    double max_gap_perc;         /* keep 100.0 * gaps <= x * (bases + gaps); < 0 disables */
    double max_masked_perc;      /* keep 100.0 * masked <= x * (bases + gaps + masked); < 0 disables */
} jl_read_rule;
/* Host only (no device, no context).  idx[0 .. *n_kept): the kept reads, ascending — what jl_msa_take takes; room for n_reads.
 * failed[5], may be NULL: reads that fail {min_bases, max_mismatches, max_mismatch_perc, max_gap_perc, max_masked_perc}; a read
 * that fails several rules counts in each.  JL_ERR_ARG (jl_last_error(NULL) says which): a NULL argument; a percentage above
 * 100; n_reads above 2^32 - 1. */
int jl_read_filter(const uint32_t *stats, uint64_t n_reads, const jl_read_rule *rule, uint32_t *idx, uint64_t *n_kept,
                   uint64_t failed[5]);
/*
 * PER-READ APOBEC hypermutation counters and their exact test (docs/SPEC.md §26).  APOBEC3G/F turns G into A where the two bases
 * downstream are R and D; a read edited that way passes any mismatch bound a clean minority haplotype must also pass, and is found
 * as Hypermut 2.0 finds it: G->A in the target context GRD against G->A in the control contexts GYN / GRC, one-sided Fisher test.
 * For read i and column c with c + 2 < n_cols, x, y, z its cells at c, c + 1, c + 2 (alignment columns; codes as above): the
 * column is a SITE of the read when ref[c] == 2 (G), x is A or G, y < 4 and z < 4.  The context is the READ's own y and z:
 *   target   y in {A, G} and z != C          control   every other site (y in {C, T}; or y in {A, G} and z == C)
 * A gap, N or uncovered cell in y or z: no site; the last two columns of the window are never sites.  Summed over the window:
 *   JL_HM_TARGET_SITES    target-context sites          JL_HM_TARGET_MUT     of those, x == A
 *   JL_HM_CONTROL_SITES   control-context sites         JL_HM_CONTROL_MUT    of those, x == A
 * counts[JL_HM_COUNTERS][n_reads], struct of arrays as jl_read_stats_async's, 32 bits, exact, independent of launch shape and
 * order; reads past n_reads count nowhere.  A ref[c] of 4 or above (and any other than 2) makes column c no site.
 * p[i] = P(X >= a) of the table [[a, n - a], [c, m - c]] with a = target mutations, n = target sites, c = control mutations, m =
 * control sites (the routine of jl_control_test), log_p[i] = ln p; n == 0 or m == 0: p = 1, log_p = 0.  No multiple-test
 * correction.
 * The contract is jl_read_stats_async's: ref[n_cols] is copied before the call returns; both kernels are enqueued on the
 * context's stream into buffers of its own and nothing else of the context is touched; every kind of resident matrix is accepted.
 * JL_ERR_ARG: ref == NULL.  JL_ERR_STATE: no resident matrix.  A refused call changes nothing.
 */
enum { JL_HM_TARGET_SITES = 0, JL_HM_TARGET_MUT = 1, JL_HM_CONTROL_SITES = 2, JL_HM_CONTROL_MUT = 3, JL_HM_COUNTERS = 4 };
int jl_read_hypermut_async(jl_ctx *ctx, const uint8_t *ref /* [n_cols] */);
/* Wait and copy out what the last jl_read_hypermut_async computed; any pointer may be NULL (all NULL: only wait).
 * JL_ERR_STATE: none was enqueued. */
int jl_read_hypermut_fetch(jl_ctx *ctx, uint32_t *counts /* [JL_HM_COUNTERS][n_reads] */, double *p /* [n_reads] */,
                           double *log_p /* [n_reads] */);
/* The test kernel alone over `n` tables the caller supplies (host arrays in and out), as jl_control_eval is for the control call.
 * JL_ERR_ARG: a NULL array, or a mutation count above its site count. */
int jl_hypermut_eval(jl_ctx *ctx, const uint32_t *counts /* [JL_HM_COUNTERS][n] */, uint64_t n, double *p, double *log_p);
/* Host only (no device, no context): the same expressions for one read.  JL_ERR_ARG: a NULL pointer, a mutation count above its
 * site count. */
int jl_hypermut_test(uint32_t target_mut, uint32_t target_sites, uint32_t control_mut, uint32_t control_sites, double *p,
                     double *log_p);
/* Host only.  A read is hypermutated when p < alpha (strict) and is dropped; idx[0 .. *n_kept): the kept reads, ascending — what
 * jl_msa_take takes; room for n_reads.  *n_flagged = n_reads - *n_kept.  JL_ERR_ARG (jl_last_error(NULL) says which): a NULL
 * argument; alpha outside (0, 1]; n_reads above 2^32 - 1. */
int jl_hypermut_filter(const double *p, uint64_t n_reads, double alpha, uint32_t *idx, uint64_t *n_kept, uint64_t *n_flagged);
/*
 * PER-READ reading-frame integrity per open reading frame (docs/SPEC.md §27): which reads carry a premature stop, are out of frame
 * or lack a large piece, in which gene — the second half of the proviral intactness screen after hypermutation.  A SPAN is an open
 * reading frame in window columns: codon k of span g is the columns col + 3 k .. col + 3 k + 2.  1 <= n_spans <= JL_ORF_MAX_SPANS,
 * n_codons >= 1 and col + 3 n_codons <= n_cols (summed in 64 bits); spans may overlap in any frame and need no order.  Per (span
 * g, read i), over the span's 3 n_codons columns only (codes as above):
 *   JL_ORF_COVERED      cells != 6                     JL_ORF_GAP_CELLS   cells == 4
 *   JL_ORF_CODONS_READ  codons whose three cells are all < 4
 *   JL_ORF_STOPS        of those, the read's codon is TAA, TAG or TGA and the codon of ref at the same three columns is none of
 *                       the three (a ref codon with any code >= 4 is no stop)
 * An N cell (5) is covered, no gap, and makes its codon unread.  first_stop[g][i]: the lowest codon index k counted in
 * JL_ORF_STOPS, or JL_ORF_NO_STOP.  counts[JL_ORF_COUNTERS][n_spans][n_reads] and first_stop[n_spans][n_reads], 32 bits, exact,
 * independent of launch shape and order; reads past n_reads count nowhere.  ref[n_cols] follows jl_read_stats_async's compare
 * convention.
 * The contract is jl_read_hypermut_async's: spans and ref are copied before the call returns; the kernels are enqueued on the
 * context's stream into buffers of its own and nothing else of the context is touched; every kind of resident matrix is accepted.
 * JL_ERR_ARG: spans or ref NULL, n_spans outside 1 .. 64, a span outside the window.  JL_ERR_STATE: no resident matrix.  A refused
 * call changes nothing.
 */
typedef struct {
    uint32_t col;
    uint32_t n_codons;
} jl_orf_span;
enum { JL_ORF_MAX_SPANS = 64 };
enum { JL_ORF_COVERED = 0, JL_ORF_GAP_CELLS = 1, JL_ORF_CODONS_READ = 2, JL_ORF_STOPS = 3, JL_ORF_COUNTERS = 4 };
#define JL_ORF_NO_STOP 0xFFFFFFFFu
int jl_read_orf_async(jl_ctx *ctx, const jl_orf_span *spans, uint32_t n_spans, const uint8_t *ref /* [n_cols] */);
/* Wait and copy out what the last jl_read_orf_async computed, for its n_spans and the n_reads it saw; any pointer may be NULL (both
 * NULL: only wait).  JL_ERR_STATE: none was enqueued. */
int jl_read_orf_fetch(jl_ctx *ctx, uint32_t *counts /* [JL_ORF_COUNTERS][n_spans][n_reads] */,
                      uint32_t *first_stop /* [n_spans][n_reads] */);
/* Host only (no device, no context): the flags of every (span, read) from the counters.  With n = n_codons of the span:
 *   JL_ORF_PARTIAL      covered < 3 n
 *   JL_ORF_STOP         first_stop < n - min(tail_codons, n): a stop before the last tail_codons codons (the first stop in the
 *                       tail: all are)
 *   JL_ORF_FRAMESHIFT   gap_cells % 3 != 0: the NET frame of the read's deletions inside the span (a -1 and a -2 deletion cancel;
 *                       insertions never enter the matrix)
 *   JL_ORF_DELETION     max_gap_cells > 0 and gap_cells >= max_gap_cells
 * A partial read keeps every other flag it earns.  rule {0, 0}: DELETION off, no tail.  JL_ERR_ARG (jl_last_error(NULL) says
 * which): a NULL argument; n_spans outside 1 .. 64; n_reads above 2^32 - 1; a counter that contradicts its span — covered > 3 n,
 * gap_cells > covered, stops > codons_read, a first_stop that is neither JL_ORF_NO_STOP nor < n.  A refused call writes nothing. */
typedef struct {
    uint32_t max_gap_cells;
    uint32_t tail_codons;
} jl_orf_rule;
enum { JL_ORF_PARTIAL = 1, JL_ORF_STOP = 2, JL_ORF_FRAMESHIFT = 4, JL_ORF_DELETION = 8 };
int jl_orf_classify(const uint32_t *counts, const uint32_t *first_stop, const jl_orf_span *spans, uint32_t n_spans,
                    uint64_t n_reads, const jl_orf_rule *rule, uint8_t *flags /* [n_spans][n_reads] */);
/* Host only.  A read is defective when the flags of any span meet `mask`, a non-empty subset of JL_ORF_STOP | JL_ORF_FRAMESHIFT |
 * JL_ORF_DELETION, and is dropped; idx[0 .. *n_kept): the kept reads, ascending — what jl_msa_take takes; room for n_reads.
 * *n_flagged = n_reads - *n_kept.  JL_ERR_ARG: a NULL argument; n_spans outside 1 .. 64; such a mask; n_reads above 2^32 - 1. */
int jl_orf_filter(const uint8_t *flags, uint32_t n_spans, uint64_t n_reads, uint32_t mask, uint32_t *idx, uint64_t *n_kept,
                  uint64_t *n_flagged);
/*
 * The SITE MATRIX (docs/SPEC.md §18): called codon deletions as sites of a haplotype.  Phasing groups reads by their codons at the
 * variant positions, and a deleted codon is no codon: its carriers are GAP-damaged where the position is a variant position and
 * invisible where it is not.  This call builds, as jl_xwin_assemble_local does, a compact matrix of chosen codon starts of `src`
 * — n_reads of `src` x 3 n_sites columns, win_begin 0, plane stride jl_plane_stride(n_reads), site k at columns 3k..3k+2 — with
 * the deletion sites recoded to a two-letter alphabet, so that jl_phase_async on `pc` groups over codons and deletions alike and
 * no phasing kernel changes.  Per read and site, by the three codes at col, col + 1, col + 2 of `src` and the classes of
 * jl_codon_deletions_async:
 *                                  JL_SITE_CODON, fill 0xFF   JL_SITE_CODON, fill f (0..63)    JL_SITE_DELETION
 *   codon (all three < 4)          copied                     copied                           A A A (codon JL_SITE_PRESENT)
 *   del3 (all three == 4)          copied                     the three bases of codon f       A A C (codon JL_SITE_DELETED)
 *   anything else                  copied                     copied                           copied
 * "Copied" keeps the three cells, so the damage flags of such a read are those of a plain codon position; only the del3 reads stop
 * being GAP at a recoded site.  A variant position that is also a called deletion is a codon site filled with a codon that is no
 * variant row there (its reference codon) FOLLOWED by a deletion site at the same column.  Every bit at or beyond n_reads, out to
 * the end of every plane row of `pc`, is code 6 — whatever an adopted `src` holds in those bits and whatever its own plane stride
 * is; bytes of `src` that do not exist read as uncovered.
 * Whatever `pc` held is replaced, as with jl_msa_alloc.  The call waits on the host for `src`'s stream, stages the table through a
 * pinned buffer of `pc`'s own, enqueues on `pc`'s stream and returns: later calls on `pc` are stream-ordered behind it.  Nothing
 * of `src` changes: matrix, insertion counters, stage results and captured graph stay as they are.  A site of a third kind
 * (JL_SITE_INSERTION: the called insertion alleles of a junction) is jl_sites_assemble_alleles's, below; this call refuses it.
 * JL_ERR_STATE: `src` has no resident matrix.  JL_ERR_ARG (jl_last_error(pc) says which): a NULL argument; pc == src; different
 * devices; n_sites 0 or above JL_SITES_MAX; col + 2 >= src's n_cols; kind above 1; fill neither 0xFF nor <= 63; a fill on a
 * deletion site; sites not non-decreasing by (col, kind); the same (col, kind) twice.  A refused call changes nothing of `pc`.
 */
enum { JL_SITE_CODON = 0, JL_SITE_DELETION = 1 };
enum { JL_SITE_NO_FILL = 0xFF, JL_SITE_PRESENT = 0 /* AAA */, JL_SITE_DELETED = 1 /* AAC */, JL_SITES_MAX = 4096 };
typedef struct {
    uint32_t col;   /* codon start in `src` */
    uint8_t kind;   /* JL_SITE_CODON, JL_SITE_DELETION; JL_SITE_INSERTION (col = the junction): jl_sites_assemble_alleles only */
    uint8_t fill;   /* JL_SITE_NO_FILL, or the codon a del3 read of a codon site becomes */
    uint16_t pad_;
} jl_site;
int jl_sites_assemble(jl_ctx *pc, jl_ctx *src, const jl_site *sites, uint32_t n_sites);
/*
 * In-frame insertion ALLELES of a record build (docs/SPEC.md §17).  An insertion never enters the matrix (J:26-27) and the
 * counters of jl_msa_track_insertions lose the joint sequence, have no denominator and apply no QV filter.  With this switch on,
 * the next record build INTO `ctx` (jl_records_finish, jl_records_window[_async], jl_msa_ingest_records[_masked]) also forms, on
 * the window's stream, per junction c (between window columns c - 1 and c, 1 <= c < n_cols; row 0 exists and stays zero)
 *   jcnt[c] = {span, inframe, frameshift, unread}, 32 bits each, exact, independent of launch shape and order:
 *     span        reads whose matrix cells at c - 1 and c are both covered (code != 6), counted from the resident planes
 *   and of the reads spanning c whose 'I' ops between the two reference-consuming ops around the junction — all of them, 'S',
 *   'H', 'P' and empty ops do not separate them — add up to L > 0 bases, each in exactly one of
 *     inframe     L % 3 == 0, 3 <= L <= 30, every inserted base exactly A, C, G or T and past the build's QV filter
 *     frameshift  L % 3 != 0
 *     unread      L % 3 == 0 and (L > 30 or some base is not readable)
 * and the table of the distinct (col = c, len = L, seq) among the inframe reads with their read counts: base j of the
 * insertion (A C G T = 0..3) in bits 2 j, 2 j + 1 of seq, the bits above 2 L zero; len is part of the key (AAA and AAAAAA have one
 * seq).  An insertion of a read that does not span its junction — at the read's first or last aligned base, next to an 'N' op,
 * outside 1 .. n_cols - 1 — counts nowhere.  The counters of jl_msa_track_insertions, the matrix and every stage are untouched.
 */
typedef struct {
    uint32_t col, len;
    uint64_t seq;
    uint32_t count, pad_;
} jl_insertion_allele;
int jl_msa_track_insertion_alleles(jl_ctx *ctx, int on);
/* Wait, and copy out jcnt[n_cols][4] (NULL: not wanted) and the table, sorted ascending by (col, len, seq): *n_rows (NULL: not
 * wanted) = its rows; rows == NULL returns only that count, else `cap` rows of room are needed.  JL_ERR_STATE: the last build into
 * `ctx` did not track, or a later call replaced the matrix (jl_msa_take, jl_msa_upload, ...).  JL_ERR_ARG: cap is too small. */
int jl_insertion_alleles_fetch(jl_ctx *ctx, uint32_t *jcnt /* [n_cols][4] */, jl_insertion_allele *rows, uint32_t cap, uint32_t *n_rows);
/* One allele of that table tested against `rate`, the probability that a read shows ANY in-frame insertion at a junction by
 * error (used for one specific sequence: conservative): coverage = span - frameshift - unread (the reads with no insertion there
 * and the reads with a readable in-frame one), expected = round_mode(coverage * rate) clamped to [0, coverage]
 * (prm->expected_round, the product in IEEE double), the table [[count, coverage - count], [expected, coverage - expected]], p by
 * prm->tail from the routines of the codon test, p_value = min(1, p * n_tests), called = count > 0 and p_value < prm->alpha and
 * the prm->min_perc / max_perc filters on 100 count / coverage (strict).  coverage == 0: not called, p_value 1, log_p 0. */
typedef struct {
    uint32_t count;
    uint32_t coverage;    /* span - frameshift - unread */
    uint32_t expected;
    uint32_t frameshift;  /* jcnt[2], jcnt[3]: not part of the test */
    uint32_t unread;
    uint32_t called;      /* 0 or 1 */
    double p_value;       /* Bonferroni-adjusted, <= 1 */
    double log_p;         /* ln of the unadjusted p */
} jl_insertion_call;
/* Host only (no device, no context).  jcnt: one junction's row of jl_insertion_alleles_fetch; n_tests: the Bonferroni factor,
 * RESOLVED.  JL_ERR_ARG (jl_last_error(NULL) says which): a NULL argument; n_tests <= 0; rate outside [0, 1]; frameshift + unread
 * above span; count above the coverage. */
int jl_insertion_test(uint32_t count, const uint32_t jcnt[4], const jl_params *prm, double rate, double n_tests, jl_insertion_call *out);
/*
 * The per-read insertion EVENTS of a record build (docs/SPEC.md §19; this build's own rule: UNPINNED).  The switch implies
 * jl_msa_track_insertion_alleles for the builds it is on — jcnt and the allele table are exactly that build's — and the build also
 * leaves one event per (read, junction) that §17 counts in inframe, frameshift or unread: `kind` 1, 2 or 3, the event's column of
 * jcnt; for kind 1 `len` and `seq` are the allele's key, exactly the table's, for kinds 2 and 3 both are 0.  A read has at most
 * one event per junction (all 'I' ops of a junction are one insertion) and none where it does not span.  Off: nothing changes.
 */
typedef struct {
    uint32_t read, col, len, kind;
    uint64_t seq;
} jl_insertion_event;   /* 24 bytes */
int jl_msa_track_insertion_reads(jl_ctx *ctx, int on);
/* Wait, and copy out the events ascending by (read, col): *n_rows (NULL: not wanted) = how many; rows == NULL returns only that
 * count, else `cap` rows of room are needed.  JL_ERR_STATE: the last build into `ctx` did not track reads, or a later call replaced
 * the matrix (the invalidation points of jl_insertion_alleles_fetch).  JL_ERR_ARG: cap is too small. */
int jl_insertion_reads_fetch(jl_ctx *ctx, jl_insertion_event *rows, uint32_t cap, uint32_t *n_rows);
/*
 * The site matrix with INSERTION sites (docs/SPEC.md §19): jl_sites_assemble, and a third kind of site whose letters are the called
 * insertion alleles of one junction.  Sites of kind 0 and 1 follow every rule above.  A site of kind JL_SITE_INSERTION has col =
 * the junction c (1 <= c < src's n_cols; no col + 2 rule) and fill JL_SITE_NO_FILL; sites ascend by (col, kind), so it follows the
 * codon and the deletion site of its column.  `alleles`: rows of jl_insertion_alleles_fetch (count is not read), strictly ascending
 * by (col, len, seq), len in 3, 6 .. 30, seq zero above bit 2 len, every col the column of an insertion site, every insertion site
 * with 1 to JL_SITE_INS_MAX_ALLELES of them, n_alleles <= JL_SITES_MAX.  The CODE of an allele is 1 + its rank among the alleles of
 * its site.  Per read at an insertion site k (columns 3k..3k+2, the three cells one codon), by the events `src`'s record build left:
 *   does not span c (cell c - 1 or c of `src` is 6), and every bit at or beyond n_reads     6 6 6
 *   spans, no event                                                                          A A A  (codon JL_SITE_INS_NONE)
 *   in-frame event, allele listed with code r                                                the three bases of codon r (1 .. 62)
 *   in-frame event, allele not listed                                                        T T T  (codon JL_SITE_INS_OTHER)
 *   frameshift event                                                                         4 4 4
 *   unread event                                                                             5 5 5
 * With no insertion site and n_alleles == 0 the result is jl_sites_assemble's, byte for byte.  JL_ERR_STATE: `src` has no resident
 * matrix, or an insertion site is asked for and `src` holds no valid events (jl_msa_track_insertion_reads before its record build).
 * JL_ERR_ARG (jl_last_error(pc) says which): every rule above.  A refused call changes nothing of `pc`.
 */
enum { JL_SITE_INSERTION = 2 };
enum { JL_SITE_INS_NONE = 0 /* AAA */, JL_SITE_INS_OTHER = 63 /* TTT */, JL_SITE_INS_MAX_ALLELES = 62 };
int jl_sites_assemble_alleles(jl_ctx *pc, jl_ctx *src, const jl_site *sites, uint32_t n_sites, const jl_insertion_allele *alleles,
                              uint32_t n_alleles);
/*
 * Reference/majority codon, error model, Fisher's exact x Bonferroni, filters, variant table
 * (SPEC §4-7; J:38-42).  `drm_masks`: optional [P] 64-bit codon masks; with --drm-only a codon is kept
 * only if its bit is set (J:370); NULL disables.  Table stays on the device; enqueues only.
 */
int jl_call_async(jl_ctx *ctx, const jl_params *prm, const uint64_t *drm_masks);
/* Wait and copy the table out.  *n_out = rows produced; JL_ERR_OVERFLOW if > cap (first cap rows are valid). */
int jl_call_fetch(jl_ctx *ctx, jl_variant *out, uint32_t cap, uint32_t *n_out);
/* Device address and capacity (rows) of the resident variant table and of its row counter (uint32). */
int jl_variant_table_device(jl_ctx *ctx, void **d_rows, void **d_count, uint32_t *cap_rows);
/*
 * The codon calls of a SAMPLE against a CONTROL instead of the error model (docs/SPEC.md section 21).  Both contexts hold a
 * pileup (jl_pileup_async) of the same window with the same genes and reference sequence.  At every position with coverage in
 * both, the reference codon is resolved as jl_call_async resolves it (the majority from the SAMPLE's histogram), and every other
 * codon j the sample shows is tested by the table [[hs[j], cov_s - hs[j]], [hc[j], cov_c - hc[j]]]: p = P(X >= hs[j]), X ~
 * Hypergeometric(cov_s + cov_c, hs[j] + hc[j], cov_s), one-sided greater; p_value = min(1, p * n_tests), called iff p_value <
 * prm->alpha, then prm->min_perc / max_perc and `drm_masks` on the sample's frequency as in jl_call_async.  prm->err and
 * prm->expected_round are not read.  Rows are jl_variant in the order of jl_call_fetch with expected := hc[j], the control's count.
 * Stream order and lifetime: the launch runs on the sample's stream behind an event recorded on the control's stream, so the
 * control's pileup need not be waited for; the control must not start another pileup (or anything else that rewrites its
 * histograms) until jl_control_call_fetch or jl_sync of the SAMPLE has returned.  The result lives in buffers of the sample's
 * context that no other call reads: jl_call_fetch, jl_phase_async(NULL) and the runs see nothing of it.  The masks and staged
 * rows of the sample's call stage are its scratch, so it is ordered with jl_call_async as stages of one stream are.
 * sample == control is allowed (and calls nothing: no count exceeds itself).
 * JL_ERR_STATE: no pileup in either context; windows, position lists or reference codons that differ.  JL_ERR_ARG: a NULL
 * argument (drm_masks may be NULL), contexts on different devices, prm->tail != 0 (the two-sided test is not defined for
 * unequal rows here), alpha <= 0.  A refused call changes nothing; jl_last_error(sample) says why (jl_last_error(NULL) when
 * sample is NULL).
 */
int jl_control_call_async(jl_ctx *sample, jl_ctx *control, const jl_params *prm, const uint64_t *drm_masks);
/* Wait and copy the table out: rows[i] and control_coverage[i] = cov_c at that row's position.  *n_out = rows produced;
 * JL_ERR_OVERFLOW if > cap (the first cap rows and coverages are valid), as jl_call_fetch.  cap == 0: both arrays may be NULL.
 * JL_ERR_STATE: none was enqueued. */
int jl_control_call_fetch(jl_ctx *sample, jl_variant *rows, uint32_t *control_coverage, uint32_t cap, uint32_t *n_out);
typedef struct {
    uint32_t count;             /* a: the sample's reads with the codon */
    uint32_t coverage;          /* cov_s */
    uint32_t control_count;     /* c */
    uint32_t control_coverage;  /* cov_c */
    uint32_t called;            /* 0 or 1 */
    uint32_t pad_;
    double p_value;             /* Bonferroni-adjusted, <= 1 */
    double log_p;               /* ln of the unadjusted p */
} jl_control_call;
/* Host only (no device, no context): one table of jl_control_call_async through the very routine its kernel compiles, with
 * prm->alpha, min_perc and max_perc.  n_tests: the Bonferroni factor, RESOLVED.  a == 0, cov_s == 0 or cov_c == 0: not called,
 * p_value 1, log_p 0.  JL_ERR_ARG (jl_last_error(NULL) says which): a NULL argument; n_tests <= 0; prm->tail != 0; a > cov_s or
 * c > cov_c. */
int jl_control_test(uint32_t a, uint32_t cov_s, uint32_t c, uint32_t cov_c, const jl_params *prm, double n_tests, jl_control_call *out);

/* ---------------------------------------------------------------- phase */

/*
 * Read x variant phasing (SPEC §8; J:192-211, 253-254, 372-381).  `variants` = host table to phase
 * against (e.g. all-gathered and filtered), or NULL to use the table jl_call_async left on the device.
 * Enqueues only.
 */
int jl_phase_async(jl_ctx *ctx, const jl_variant *variants, uint32_t n_var, uint32_t min_reads);
/*
 * Wait and copy out.  pos_cols[Vp]; hap_count[H]; hap_pattern[H][Vp] (codon indices);
 * hit[V][H] (J:207-209); read_hap[n_reads]; cooc[V][V].  Any pointer may be NULL; capacities are the
 * caller's: pos_cols/hap_pattern rows are sized with cap_var, hap_* with JL_MAX_HAPLOTYPES.
 */
int jl_phase_fetch(jl_ctx *ctx, jl_phase_summary *summary, uint32_t *pos_cols, uint32_t *hap_count,
                   uint8_t *hap_pattern, uint8_t *hit, uint16_t *read_hap, uint32_t *cooc, uint32_t cap_var);

/* ---------------------------------------------------------------- the whole path in one enqueue */

/*
 * pileup -> call (-> phase) -> one small result copy, enqueued as a captured HIP graph that is replayed
 * while genes / reference / parameters / buffers are unchanged (what `juliet in.bam out.json` does per
 * window, J:62-66, 195).  Results are then read with jl_call_fetch / jl_phase_fetch, which decode the
 * pinned result block without further device traffic.  `want_read_hap` also copies the per-read haplotype
 * ids (the haplotype block's read lists, J:209-211).  Set the environment variable JL_NO_GRAPH to run eagerly.
 */
int jl_run_async(jl_ctx *ctx, const jl_gene *genes, uint32_t n_genes, const uint8_t *refseq, uint32_t ref_len,
                 const jl_params *prm, const uint64_t *drm_masks, int phasing, uint32_t min_reads, int want_read_hap);

/*
 * Completion of the last jl_run_async without a HIP synchronisation call: the run's last kernel stores a
 * sequence word into pinned host memory behind a system-scope fence and these calls read it (a
 * hipStreamSynchronize after a graph launch costs 10-18 us of host time on ROCm 7.2 even when the work has
 * long finished).  jl_run_wait spins until the results are on the host; jl_run_done never blocks (1 done, 0 not).
 * jl_call_fetch / jl_phase_fetch wait the same way, so calling these first is optional.
 */
int jl_run_wait(jl_ctx *ctx);
int jl_run_done(jl_ctx *ctx);

/*
 * Zero-copy view of the results of the last jl_run_async: pointers into the context's pinned result block
 * (host memory the kernels stored into directly), valid until the next jl_run_async / stage call on this
 * context.  `complete` = 0 means some part did not fit the fixed-size block (more than 128 variants /
 * positions / haplotypes): use jl_call_fetch / jl_phase_fetch then.  Waits like jl_run_wait.
 */
typedef struct {
    uint32_t complete;      /* 1: every field below is valid */
    uint32_t n_variants;    /* rows of `variants` (total called; J:94-98) */
    uint32_t phased;        /* 1 if the run included phasing */
    uint32_t n_positions;   /* Vp */
    uint32_t n_haplotypes;  /* H */
    uint32_t n_var_phase;   /* rows the hit / co-occurrence matrices cover */
    uint64_t n_reads;
    jl_phase_summary summary;
    const jl_variant *variants;
    const uint32_t *pos_cols;     /* [Vp] */
    const uint32_t *hap_count;    /* [H] */
    const uint8_t *hap_pattern;   /* [H][Vp] */
    const uint8_t *hit;           /* [n_var_phase][H] (haplotype_hit, J:207-209) */
    const uint32_t *cooc;         /* [n_var_phase][n_var_phase], NULL if it did not fit */
    /* Per-read haplotype ids (the haplotype block's read lists, J:209-211), NULL / 0 unless the run asked for them.
     * They cross PCIe in the narrowest code that holds H: read_hap_bits = 4 (H <= 14: haplotype 0..13, 14 = insufficient
     * coverage, 15 = damaged; read i in bits 4*(i&1).. of byte i/2), 8 (H <= 254: 254 insufficient, 255 damaged) or
     * 16 (the ids themselves, JL_HAP_INSUFFICIENT / JL_HAP_DAMAGED).  `read_hap` is set only for 16-bit ids;
     * jl_phase_fetch and jl_expand_read_hap give 16-bit ids for every width. */
    const uint16_t *read_hap;
    const void *read_hap_packed;
    uint32_t read_hap_bits;
    uint32_t reserved;
} jl_run_view;
int jl_run_view_get(jl_ctx *ctx, jl_run_view *out);
/* Packed per-read ids of a view (read_hap_packed, read_hap_bits) -> out[n_reads] 16-bit ids.  Host only. */
int jl_expand_read_hap(const void *packed, uint32_t bits, uint64_t n_reads, uint16_t *out);

/*
 * Group runs: the whole path for SEVERAL (at most 32) resident windows (one context each, same device) in a few launches —
 * per stage ONE launch for up to eight windows (blockIdx.z = window): counting, the Fisher stage (in the counting launch's epilogue
 * or as a launch of its own, chosen per run from what else the device has in flight: same results), phasing, per-read ids.  A 150 MB window is too short a stream to hide a launch's ramp and drain, and its phasing stage
 * is a latency chain that occupies a hardware queue while doing little; grouped, the pileup runs at the rate of one long
 * stream and the latency chains of all windows overlap.  Groups of more than eight windows are pipelined inside the
 * launch: the counting of the next eight runs beside the phasing of the previous eight.
 * Results are per window and identical to jl_run_async on each context: every context keeps its own result block,
 * per-read ids and completion word, so jl_run_wait, jl_run_done, jl_run_view_get, jl_call_fetch, jl_phase_fetch and
 * jl_allgather_variants_async apply unchanged.  All windows get the same genes / reference / parameters (they are windows
 * of one reference, or samples of one amplicon); phasing may be off (call only).  A window with more than 10 variant
 * positions is flagged as in jl_run_async (its fetch calls then re-run the multi-word pipeline).  Every window is counted
 * by one block per column chunk, so windows of millions of reads are better run one by one.
 * The contexts' own streams must be idle (uploads finished).
 */
typedef struct jl_group jl_group;
int jl_group_create(jl_ctx *const *ctxs, uint32_t n_ctx, jl_group **out);
void jl_group_destroy(jl_group *group);
const char *jl_group_last_error(const jl_group *group);
int jl_group_run_async(jl_group *group, const jl_gene *genes, uint32_t n_genes, const uint8_t *refseq, uint32_t ref_len,
                       const jl_params *prm, int phasing, uint32_t min_reads, int want_read_hap);
/* The same with --drm-only masks per window (J:370): drm_masks[k] = [P] 64-bit codon masks of window k as in
 * jl_call_async, or NULL for a window without; drm_masks itself may be NULL. */
int jl_group_run_masked_async(jl_group *group, const jl_gene *genes, uint32_t n_genes, const uint8_t *refseq,
                              uint32_t ref_len, const jl_params *prm, const uint64_t *const *drm_masks, int phasing,
                              uint32_t min_reads, int want_read_hap);
/* The results of the last group run, one view per window (the group's context order): jl_run_view_get on every context in
 * ONE call — waits for each window's completion word in turn.  out[cap]; *n = the group's windows.  A window whose view
 * fails ends the call with its status (jl_group_last_error names it). */
int jl_group_views(jl_group *group, jl_run_view *out, uint32_t cap, uint32_t *n);
/* Timing hook (bench): average device time in ms of the grouped pileup launch alone — the plain counting kernel, without the
 * Fisher stage a run may carry in its epilogue — `reps` back-to-back launches rotating over `groups` (each must have run once);
 * `bytes_per_launch` = algorithmic bytes of one launch of groups[0]: 3 bits per cell, every cell read once.  No side effect on
 * the groups' last runs: their results stay complete and fetchable. */
int jl_group_time_pileup(jl_group *const *groups, uint32_t n_groups, uint32_t reps, float *ms_avg, uint64_t *bytes_per_launch);

/* The deviation index of a context's resident matrix: a structure the library derives from the planes of a window that is run
 * again and again — per plain codon chunk, the reads that differ from the column majority — and counts from instead of the planes
 * from the third run on.  Results never depend on it (docs/SPEC.md); this call only observes it.
 *   state           0 none, 1 a build is enqueued, 2 built, 3 refused (no chunk's list would have at most 9 plane_stride / 8
 *                   entries, one per eight of the chunk's plane bytes: every chunk is counted from the planes)
 *   generation      of the matrix: every producer that rewrites the matrix starts a new one, with no index and run counter 0
 *   runs            runs enqueued on this generation and chunk table (jl_run_async, jl_group_run(_masked)_async, jl_pileup_async)
 *   builds          index builds this context has enqueued over its life
 *   last_form       1: the last enqueued run counted from the index, 0: from the planes
 *   plain_chunks    chunks the index covers at most; indexed_chunks: those that have a list; entries: reads in all lists
 *   bytes           device memory of the entry buffer (allocated at its bound before the build; an entry is 2 bytes: a deviating
 *                   read's three codes, not its number)
 * Cost: a window's SECOND run on a matrix and chunk table allocates the entry buffer at its bound (9 plane_stride / 8 entries per
 * plain chunk: 28 MB for 100 000 reads x 3 000 columns) and uploads two small tables with one stream synchronisation before it is
 * enqueued — once per matrix generation; a caller whose second run is latency-critical sees that run some hundred microseconds late.
 * wait != 0: a build that is enqueued is waited for first.  chunk_flags (optional, room for cap_chunks >= the chunk table's length;
 * implies wait): per chunk of the pileup's chunk table 0 = counted from the planes (not a plain chunk, or no index), 1 = has a
 * list, 2 = a plain chunk over the density bound (counted from the planes). */
typedef struct jl_index_info {
    uint32_t state, runs, builds, last_form;
    uint32_t plain_chunks, indexed_chunks;
    uint64_t generation, entries, bytes;
} jl_index_info;
int jl_msa_index_info(jl_ctx *ctx, jl_index_info *info, int wait, uint8_t *chunk_flags, uint32_t cap_chunks);

/* ---------------------------------------------------------------- numerics self-check */

/*
 * Evaluate the device's Fisher routine on `n` tables [[a, cov-a], [c, cov-c]] (host arrays in and out):
 * p[i] = P(X >= a[i]) unadjusted, log_p[i] = ln p.  Lets a host pin the device numerics against its own
 * golden vectors (tests/golden/fisher_golden.json).
 */
int jl_fisher_eval(jl_ctx *ctx, const uint32_t *a, const uint32_t *c, const uint32_t *cov, uint32_t n, double *p,
                   double *log_p);
/* The same with the tail of jl_params: 0 = P(X >= a), 1 = two-sided. */
int jl_fisher_eval_tail(jl_ctx *ctx, const uint32_t *a, const uint32_t *c, const uint32_t *cov, uint32_t n, int tail,
                        double *p, double *log_p);
/*
 * The same for the general-margin routine of the control call (SPEC §21): `n` tables [[a, cov_s-a], [c, cov_c-c]] with both
 * coverages above 0.  skipped == NULL: p[i] = P(X >= a[i]), log_p[i] = ln p, and n_tests, alpha are not read.  Otherwise the
 * form the control call's kernel evaluates: skipped[i] = 1 and p[i] = 1 where the point mass alone, times n_tests, reaches
 * alpha (n_tests > 0, alpha > 0), the plain value everywhere else.
 */
int jl_control_eval(jl_ctx *ctx, const uint32_t *a, const uint32_t *cov_s, const uint32_t *c, const uint32_t *cov_c, uint32_t n,
                    double n_tests, double alpha, double *p, double *log_p, uint32_t *skipped);

/* ---------------------------------------------------------------- timing hooks (bench) */

/* Latency of the whole path at this boundary, host clock: `reps` runs one after the other, each jl_run_async ->
 * jl_run_view_get (which waits for the completion word) before the next is launched; average ms per run. */
int jl_time_run(jl_ctx *ctx, const jl_gene *genes, uint32_t n_genes, const uint8_t *refseq, uint32_t ref_len,
                const jl_params *prm, const uint64_t *drm_masks, int phasing, uint32_t min_reads, int want_read_hap,
                uint32_t reps, float *ms_avg);
/* Average device time in ms of `reps` back-to-back launches of the pileup kernel alone, by HIP events on the ctx stream. */
int jl_time_pileup(jl_ctx *ctx, uint32_t reps, float *ms_avg);
/* The same over several contexts' resident windows in rotation, all on the first context's stream: no launch finds
 * its input in the Infinity Cache (4 x 150 MB > 256 MiB), as in a pipelined loop over several batches. */
int jl_time_pileup_set(jl_ctx *const *ctxs, uint32_t n_ctx, uint32_t reps, float *ms_avg);
/* The pileup of a RUN, timed where it runs: `on` puts two one-thread nodes around the pileup launch of this context's runs
 * (jl_run_async), each storing the device's constant-rate clock into pinned host memory; jl_run_pileup_ms (after jl_run_wait or
 * a fetch of the run) gives the distance between the two of the LAST run in ms — the pileup as it ran beside whatever else the
 * device was doing (another sample's latency-bound stages, another window's pileup), not alone (jl_time_pileup).  Off by
 * default: two more nodes are 2-3 us of a run. */
int jl_run_pileup_clock(jl_ctx *ctx, int on);
/* begin_ticks (may be null): the first of the two stamps, in ticks of that 100 MHz clock — one clock for all contexts of a
 * device, so the pileups of several contexts can be laid on one time line (do they overlap?  how long is the device without one?). */
int jl_run_pileup_ms(jl_ctx *ctx, float *ms, uint64_t *begin_ticks);
/* Name of the dominant kernel as rocprofv3 reports it. */
const char *jl_pileup_kernel_name(void);

/* ---------------------------------------------------------------- multi-GPU */

/* Rank 0 makes a 128-byte RCCL unique id and hands it to the other ranks out of band. */
int jl_comm_unique_id(uint8_t id[128]);
/* One communicator per (rank, device); any context on that device may use it.  Collectives run on the
 * communicator's own stream, ordered behind the producing context by an event. */
int jl_comm_create(jl_ctx *ctx, const uint8_t id[128], int rank, int world, jl_comm **out);
/* The same communicator for ranks that are THREADS OF ONE PROCESS (a host that drives several devices from one process,
 * or — RCCL refuses that — several ranks on one device): every exchange is a set of device copies between the ranks'
 * buffers (same device, or peer devices over xGMI) between two barriers of the rank threads; no RCCL communicator is
 * made.  `id`: 128 bytes that name the world (jl_comm_unique_id, or any bytes unique in the process); every rank of the
 * world calls this once.  Everything that takes a jl_comm works on it unchanged. */
int jl_comm_create_inproc(jl_ctx *ctx, const uint8_t id[128], int rank, int world, jl_comm **out);
void jl_comm_destroy(jl_comm *comm);
/* What the communicator is, for a caller's records: rccl_ranks = what ncclCommCount reports (0: the in-process form, which has
 * no RCCL communicator), rank / world as given at creation, exchange_form = how a group's bound exchange travels on it
 * (-1 not decided yet: nothing was bound; 1 the all-gather works in place in pinned host memory; 0 staged: device region +
 * heads_to_host kernel).  Any pointer may be null.  Match: SURVEY 8e (one all-gather of the variant table). */
int jl_comm_info(jl_comm *comm, int *rccl_ranks, int *rank, int *world, int *exchange_form);
/*
 * The one collective of the path: all-gather of the fixed-stride variant table over RCCL/xGMI.
 * all_rows[world*cap_rows], all_counts[world] are HOST outputs; rows of rank r start at r*cap_rows.
 */
int jl_allgather_variants(jl_ctx *ctx, jl_comm *comm, jl_variant *all_rows, uint32_t *all_counts, uint32_t cap_rows);
/*
 * Enqueue-only half for hosts that keep several batches in flight: call right after jl_run_async; the
 * exchange (6.2 KB per rank: result header + up to 128 rows) then overlaps other work and the following
 * jl_allgather_variants on the same ctx/comm only waits and unpacks.  The call itself makes no HIP call: a worker
 * thread of the communicator waits for the run's completion word and then issues the collective on the
 * communicator's stream.  The device result block is double-buffered by run parity, so a context may launch its
 * next run — and request that run's exchange — before collecting this one: at most TWO exchanges pending per
 * context (a third, and a run started while two are pending, are refused with JL_ERR_STATE);
 * jl_allgather_variants returns the OLDEST pending one.  A run that called more than 128 variants on some rank falls back
 * to the full fixed-stride table, which is not double-buffered: such an exchange must be collected before the
 * context's next run (JL_ERR_STATE otherwise, on every rank alike).
 * At most 128 exchanges in flight per communicator; every collective of a communicator is issued by its worker thread.
 */
int jl_allgather_variants_async(jl_ctx *ctx, jl_comm *comm);
/* The same for several contexts at once (the windows of a group run): their all-gathers are issued as ONE RCCL group,
 * i.e. one collective launch.  Every rank must pass the same number of contexts in the same call order.  Collect
 * each context's exchange with jl_allgather_variants as usual. */
int jl_allgather_variants_async_many(jl_ctx *const *ctxs, uint32_t n, jl_comm *comm);
/* The collecting half for several contexts in one call (e.g. the windows of one launch, one cycle later):
 * all_rows [n_ctx][world][cap_rows], all_counts [n_ctx][world]; jl_last_error of the failing context tells why. */
int jl_allgather_variants_many(jl_ctx *const *ctxs, uint32_t n_ctx, jl_comm *comm, jl_variant *all_rows,
                               uint32_t *all_counts, uint32_t cap_rows);
/*
 * The exchange of a group run as ONE device operation, carried by the run itself.  After jl_group_exchange_bind(group, comm)
 * every jl_group_run(_masked)_async of the group (at most 32 windows) also exchanges the heads of its windows' tables: the
 * run's last kernels write them — besides the result blocks — into this rank's part of a pinned host region
 * [rank][window][head], and the same call issues ONE all-gather IN PLACE in that region on the group's stream, behind
 * the run, and one event.  No gather kernel, no copy back, no worker thread, no second stream; with one rank the
 * all-gather is nothing at all.  The launching thread makes the RCCL call itself, behind whatever the communicator's
 * worker still had to issue, so every rank keeps one order of collectives as long as every rank runs the same program.
 * jl_group_exchange_collect returns the OLDEST pending exchange of the group — all_rows [n_windows][world][cap_rows],
 * all_counts [n_windows][world], as jl_allgather_variants_many — spinning on its event (JL_ERR_COMM after 60 s, and when a
 * rank's run did not reach its result block: every rank sees that rank's empty head).  Two regions by run parity: a
 * group may launch its next run before collecting this one; a third pending exchange is refused (JL_ERR_STATE).  A run
 * that fails on a rank before or at its launch still issues that rank's collective, with empty heads: the launching call
 * returns the run's own error, the collecting calls of ALL ranks report that rank (JL_ERR_COMM), nobody waits for ever.  A run
 * in which some rank called more than 128 variants falls back — on every rank alike — to the full fixed-stride table of
 * every window, which must then be collected before the group's next run.
 * Binding is a collective the first time a communicator is bound: the ranks try a 64-byte all-gather in pinned host memory
 * and agree on the outcome; where that does not work (or with JL_EXCHANGE_STAGED=1) the all-gather works in device memory
 * and a copy to the pinned region follows it (two operations).  comm = NULL unbinds; a group must be unbound or destroyed
 * before its communicator is.  In-process communicators block
 * in the launching call, as all their exchanges do.  Match: SURVEY 8e "exchange the variant table", doc/JULIET.md:94-100.
 */
int jl_group_exchange_bind(jl_group *group, jl_comm *comm);
int jl_group_exchange_collect(jl_group *group, jl_variant *all_rows, uint32_t *all_counts, uint32_t cap_rows);

/* ---------------------------------------------------------------- cross-window phasing */

/*
 * Reads that span several windows are phased on a compact matrix made of only the variant columns of ALL
 * windows: position k (ascending global column) occupies columns 3k..3k+2 of `pc`'s resident matrix.
 * `merged`: every window's called rows with GLOBAL (reference) columns, e.g. the all-gathered table.
 * Outputs: `remapped` (same rows, col = 3k) to pass to jl_phase_async(pc, remapped, ...), `pos_global[vp]`.
 * All windows must hold the same reads in the same order.  Phasing itself then runs replicated on the
 * compact matrix (3*Vp columns: a few MB even at 1e7 reads).
 */
/* The plan alone, on the host (no device, no communicator — what both functions below compute first, exposed for hosts that
 * move the columns themselves): vp_total distinct positions, pos_global[k] ascending, remapped rows (col = 3k), and
 * owner[k] = index of the window [win_begin[w], win_begin[w] + win_ncols[w]) that holds columns pos..pos+2 (-1: none). */
int jl_xwin_plan(const uint32_t *win_begin, const uint32_t *win_ncols, uint32_t n_windows, const jl_variant *merged,
                 uint32_t n_var, jl_variant *remapped, uint32_t *pos_global, int32_t *owner, uint32_t *vp_total);
/* every window resident on this device: device-to-device copies */
int jl_xwin_assemble_local(jl_ctx *pc, jl_ctx *const *windows, uint32_t n_windows, const jl_variant *merged,
                           uint32_t n_var, jl_variant *remapped, uint32_t *pos_global, uint32_t *vp_total);
/* one window per rank: each position's owner broadcasts its 3 columns over RCCL (second exchange of the run) */
int jl_xwin_assemble_rccl(jl_ctx *pc, jl_ctx *window, jl_comm *comm, const uint32_t *win_begin,
                          const uint32_t *win_ncols, const jl_variant *merged, uint32_t n_var, jl_variant *remapped,
                          uint32_t *pos_global, uint32_t *vp_total);

/*
 * Cross-window phasing with the READS sharded (SURVEY §8e option A; docs/SPEC.md §8).  Rank s phases reads
 * [slice_begin[s], slice_begin[s+1]) only: its compact matrix holds that slice of every variant position's three columns,
 * so the second exchange moves 1/world of the bytes and every rank groups 1/world of the reads.  Sequence per rank:
 *   jl_xwin_assemble_slice_*  ->  jl_phase_groups_async  ->  jl_phase_groups_fetch  (this slice's groups: pattern + count)
 *   all-gather of the group tables (KB) and merge on the host: counts of equal patterns add up; the merged groups with
 *     >= min_reads reads are the haplotypes, ordered as SPEC §8 says; hit and co-occurrence follow from patterns and counts
 *   jl_phase_regroup          (each exported group's haplotype id back to the device: per-read ids of the slice)
 * Slices start on multiples of 256 reads.  The host side of the merge is minorseq_amd/sharding.py (merge_groups,
 * select_haplotypes); tests/test_gpu_sharded_phase.py checks the whole sequence against the unsharded run.
 */
int jl_xwin_assemble_slice_local(jl_ctx *pc, jl_ctx *const *windows, uint32_t n_windows, const jl_variant *merged,
                                 uint32_t n_var, uint64_t read_begin, uint64_t n_slice, jl_variant *remapped,
                                 uint32_t *pos_global, uint32_t *vp_total);
/* one window per rank: the owner of a position sends rank s its slice (ncclSend / ncclRecv in one group);
 * slice_begin has world + 1 entries, the same on every rank */
int jl_xwin_assemble_slice_rccl(jl_ctx *pc, jl_ctx *window, jl_comm *comm, const uint32_t *win_begin,
                                const uint32_t *win_ncols, const jl_variant *merged, uint32_t n_var,
                                const uint64_t *slice_begin, jl_variant *remapped, uint32_t *pos_global, uint32_t *vp_total);
/* keys + grouping of the resident matrix, the groups written out instead of ranked (variants as in jl_phase_async) */
int jl_phase_groups_async(jl_ctx *ctx, const jl_variant *variants, uint32_t n_var);
/* group q: counts[q] reads with codon code patterns[q * pattern_stride + p] at variant position p (pos_cols[p]);
 * *partial: this matrix's damaged reads and marginals, its clean reads under insufficient_reads.  Pointers except
 * n_groups / n_positions may be NULL. */
int jl_phase_groups_fetch(jl_ctx *ctx, uint8_t *patterns, uint32_t pattern_stride, uint32_t *counts, uint32_t cap_groups,
                          uint32_t *n_groups, uint32_t *n_positions, uint32_t *pos_cols, uint32_t cap_var,
                          jl_phase_summary *partial);
/* hap_of_group[q] = haplotype id of exported group q after the merge (JL_HAP_INSUFFICIENT: not reported);
 * read_hap (optional, [n_reads of this matrix]) receives the per-read ids */
int jl_phase_regroup(jl_ctx *ctx, const uint16_t *hap_of_group, uint32_t n_groups, uint32_t n_haplotypes, uint16_t *read_hap);

/* ---------------------------------------------------------------- the merge of the sharded path: host only
 *
 * No device and no communicator: these run anywhere the library loads (the gloo tests call them on CPU ranks).
 * Behaviour: the >= 10-read rule applies to the MERGED count of a pattern (J:253-254); order, ids, haplotype_hit and the
 * read categories as docs/SPEC.md §8 (J:192-211, 372-381). */

/* Per-window tables (window-relative `col`) -> one table with GLOBAL columns in (gene, codon_pos, codon) order.
 * tables[t] has counts[t] rows and belongs to the window starting at reference column win_begin[t].
 * JL_ERR_OVERFLOW if the rows do not fit `cap` (*n_merged then holds the number needed). */
int jl_merge_tables(const jl_variant *const *tables, const uint32_t *counts, const uint32_t *win_begin, uint32_t n_tables,
                    jl_variant *merged, uint32_t cap, uint32_t *n_merged);
/* Exported group tables (jl_phase_groups_fetch: patterns[t][q * pattern_stride[t] + p], counts[t][q], n_groups[t] groups
 * of vp positions) -> the distinct patterns in ascending order (codon codes compared position by position), the summed
 * counts, and index[t][q] = merged row of group q of table t (index or index[t] may be NULL). */
int jl_merge_groups(const uint8_t *const *patterns, const uint32_t *pattern_stride, const uint32_t *const *counts,
                    const uint32_t *n_groups, uint32_t n_tables, uint32_t vp, uint8_t *merged_patterns /* [cap][vp] */,
                    uint64_t *merged_counts, uint32_t cap, uint32_t *n_merged, uint32_t *const *index);
/* docs/SPEC.md §8 on merged groups: reported = count >= min_reads, ordered by (count desc, pattern asc), at most
 * JL_MAX_HAPLOTYPES.  `variants`: the table with col = 3 * position index (jl_xwin_plan's `remapped`) or any table whose
 * `col` values appear in pos_cols[vp].  partials[n_partials]: each slice's damaged reads and marginals.
 * Outputs (any may be NULL): summary; hap_count[H]; hap_pattern[H][vp]; hit[n_var][hit_stride] (J:207-209);
 * cooc[n_var][n_var]; hap_of_group[n_groups] (JL_HAP_INSUFFICIENT where not reported). */
int jl_select_haplotypes(const uint8_t *patterns, const uint64_t *counts, uint32_t n_groups, uint32_t vp,
                         const jl_variant *variants, uint32_t n_var, const uint32_t *pos_cols, uint32_t min_reads,
                         const jl_phase_summary *partials, uint32_t n_partials, jl_phase_summary *summary,
                         uint32_t *hap_count, uint8_t *hap_pattern, uint8_t *hit, uint32_t hit_stride, uint32_t *cooc,
                         uint16_t *hap_of_group);

/* The schedule of the column-slice exchange as data (what jl_xwin_phase_sharded / jl_xwin_assemble_slice_rccl issue):
 * positions are ascending global columns and windows ascending column ranges, so the positions a rank owns are ONE run
 * k_begin .. k_begin + k_count, and a rank sends every peer ONE packed message: slice s of the 9 * k_count plane
 * rows of the owned columns (three columns x three planes per position), each row padded with 'not covered' (code 6: 0x00
 * in plane 0, 0xFF in planes 1 and 2) to dst_stride = jl_plane_stride(reads of slice s) — exactly the bytes of columns
 * 3 * k_begin .. of the receiver's compact matrix, where the matching receive lands them.
 * win_rank[w] = rank that holds window w (non-decreasing).  ops of rank `rank`, in issue order: its own slice (a device
 * copy), then per peer in ascending order the send and the receive.  Every send has exactly one matching receive
 * (same byte count) in the peer's list.  JL_ERR_ARG if a variant column lies in no window. */
enum { JL_XWIN_OP_LOCAL = 0, JL_XWIN_OP_SEND = 1, JL_XWIN_OP_RECV = 2 };
typedef struct {
    int32_t op, peer;            /* peer: the other rank (own rank for JL_XWIN_OP_LOCAL) */
    uint32_t k_begin, k_count;   /* positions whose columns travel */
    uint64_t read_begin, n_reads;/* the slice of the reads (the RECEIVER's slice) */
    uint64_t dst_stride;         /* bytes per plane row in the message = the receiver's plane stride */
    uint64_t bytes;              /* 9 * k_count * dst_stride */
    uint64_t dst_offset;         /* where the message lands in the receiver's compact matrix: 9 * k_begin * dst_stride */
} jl_xwin_op;
int jl_xwin_slice_plan(const uint32_t *win_begin, const uint32_t *win_ncols, const int32_t *win_rank, uint32_t n_windows,
                       const jl_variant *merged, uint32_t n_var, const uint64_t *slice_begin, int32_t world, int32_t rank,
                       jl_xwin_op *ops, uint32_t cap_ops, uint32_t *n_ops);

/* ---------------------------------------------------------------- cross-window phasing, the whole sequence
 *
 * A session = this rank's windows of ONE reference whose reads span every window (BASELINE.json configs[3]/[4]), the
 * communicator (NULL when world = 1: every window is on this device), the column layout of ALL windows and the read
 * slices.  windows[0 .. n_local) are this rank's windows in ascending column order, i.e. the windows w with
 * win_rank[w] == rank.  Slices start on multiples of 256 reads; slice_begin has world + 1 entries.
 *
 * jl_xwin_phase_sharded, called by every rank after its windows' call stage (jl_run_async / jl_group_run_async with
 * phasing off, or jl_call_async), runs the rest of the path with the reads sharded (option A):
 *   all-gather of the variant tables (RCCL, one collective; none at world = 1)  ->  merge + plan on the host  ->
 *   one packed send per peer of the variant columns' slices (RCCL; a device copy for the own slice)  ->
 *   keys + grouping of the slice on the device, the groups exported  ->  all-gather of the group tables (RCCL) ->
 *   merge + selection on the host (jl_merge_groups, jl_select_haplotypes)  ->  per-read ids of the slice on the device.
 * The result's pointers are into the session and stay valid until the next call; the per-read ids stay in HBM — their
 * launch is enqueued when the call returns, not awaited — until jl_xwin_read_hap_fetch (which waits for it).  While the call runs the communicator must have no asynchronous exchange pending
 * (JL_ERR_STATE otherwise): the session issues its collectives from the calling thread. */
typedef struct jl_xwin jl_xwin;
typedef struct {
    uint32_t n_variants;          /* rows of `merged` */
    uint32_t n_positions;         /* Vp */
    uint32_t n_haplotypes;        /* H */
    uint32_t n_groups;            /* distinct patterns over all slices */
    jl_phase_summary summary;     /* read categories over ALL reads (J:372-381) */
    const jl_variant *merged;     /* every window's rows, global columns, (gene, codon_pos, codon) order */
    const uint32_t *pos_global;   /* [Vp] ascending global columns */
    const uint32_t *hap_count;    /* [H] */
    const uint8_t *hap_pattern;   /* [H][Vp] */
    const uint8_t *hit;           /* [n_variants][H] (haplotype_hit, J:207-209) */
    const uint32_t *cooc;         /* [n_variants][n_variants] */
    uint64_t slice_begin, slice_reads;  /* this rank's reads */
    uint32_t read_hap_bits;       /* width of the per-read ids in HBM: 4, 8 or 16 */
    uint32_t reserved;
} jl_xwin_result;
int jl_xwin_create(jl_ctx *const *windows, uint32_t n_local, jl_comm *comm, const uint32_t *win_begin,
                   const uint32_t *win_ncols, const int32_t *win_rank, uint32_t n_windows, const uint64_t *slice_begin,
                   jl_xwin **out);
void jl_xwin_destroy(jl_xwin *x);
const char *jl_xwin_last_error(const jl_xwin *x);
int jl_xwin_phase_sharded(jl_xwin *x, uint32_t min_reads, jl_xwin_result *out);
/* Host time of the last jl_xwin_phase_sharded by stage, in microseconds (out[JL_XWIN_STAGES]): 0 the windows' tables on
 * the host (waits for their call stage), 1 all-gather + merge of the tables, 2 plan, 3 pack + exchange + grouping
 * enqueued, 4 waiting for the groups (and their all-gather), 5 merge + selection, 6 per-read ids. */
enum { JL_XWIN_STAGES = 8 };
int jl_xwin_stage_us(const jl_xwin *x, float *out);
/* 16-bit ids of this rank's slice (read_hap[slice_reads]) of the last jl_xwin_phase_sharded. */
int jl_xwin_read_hap_fetch(jl_xwin *x, uint16_t *read_hap);
/* The collective on its own, for hosts that drive the stages themselves: fixed-stride all-gather over RCCL of the
 * groups jl_phase_groups_async exported on `ctx` (cap_groups rows of pattern_stride bytes per rank, plus counts, the
 * partial summary and the number of positions).  Host outputs: patterns[world][cap_groups][pattern_stride],
 * counts[world][cap_groups], n_groups[world], partials[world].  JL_ERR_OVERFLOW, on every rank alike, when a rank
 * exported more than cap_groups groups. */
int jl_allgather_groups(jl_ctx *ctx, jl_comm *comm, uint32_t cap_groups, uint32_t pattern_stride, uint8_t *patterns,
                        uint32_t *counts, uint32_t *n_groups, jl_phase_summary *partials, uint32_t *n_positions);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif /* JULIET_HIP_H */
