// capi_records.hip — the record stream of include/juliet_hip.h: upload of aligned records, the builds from them, insertion counters.
// Aligned records straight to the resident layout: cigar expansion, QV masking and the transpose all run
// on the device.  Arrays are what a BAM decoder holds: per read its leftmost position, its
// cigar words (len << 4 | op), its 4-bit packed bases exactly as stored in BAM, optionally its qualities.
// Streamed form: jl_records_begin / jl_records_append (any number of chunks, e.g. one per inflated BGZF batch,
// so the upload hides under the decode of the next chunk) / jl_records_finish (alloc + kernels).
#include <string.h>

#include <algorithm>

#include "jl_internal.h"

static void records_drop(jl_ctx *ctx) { ctx->rec.release(); }

// a HIP call of the upload ("records") or of a build ("ingest") failed
static int hip_fail(jl_ctx *ctx, const char *what, hipError_t e) { return jl_fail(ctx, jl_hip_status(e), "%s: %s", what, hipGetErrorString(e)); }

extern "C" {

int jl_records_begin(jl_ctx *ctx, uint64_t reads_hint, uint64_t cigar_words_hint, uint64_t seq_bytes_hint, uint64_t qual_bytes_hint)
{
    if (!ctx) return JL_ERR_ARG;
    JL_HIP(ctx, hipSetDevice(ctx->device));
    records_drop(ctx);
    jl_records &r = ctx->rec;
    hipStream_t st = ctx->stream;
    r.open = true;
    hipError_t e = r.pos.grow_keep(st, 0, (size_t)reads_hint, 0);
    if (e == hipSuccess) e = r.co.grow_keep(st, 0, (size_t)reads_hint + 1, 0);
    if (e == hipSuccess) e = r.so.grow_keep(st, 0, (size_t)reads_hint + 1, 0);
    if (e == hipSuccess) e = r.cig.grow_keep(st, 0, (size_t)cigar_words_hint, 64);
    if (e == hipSuccess) e = r.seq.grow_keep(st, 0, (size_t)seq_bytes_hint, 64);
    // (the qualities begin 16 bytes into their array: the ingest reads a piece's 32 qualities from up to six bytes before a read's first)
    r.n_qual = 16;
    if (e == hipSuccess && qual_bytes_hint) e = r.qual.grow_keep(st, 0, (size_t)qual_bytes_hint + 16, 64);
    if (e == hipSuccess && qual_bytes_hint) e = r.qo.grow_keep(st, 0, (size_t)reads_hint + 1, 0);
    if (e != hipSuccess) {
        records_drop(ctx);
        return hip_fail(ctx, "records", e);
    }
    return JL_OK;
}

// bytes of a mask of `seq_bytes` bytes of packed bases: a bit per nibble
uint64_t jl_qmask_bytes(uint64_t seq_bytes) { return (seq_bytes + 3u) / 4u; }

// The byte form's rule (kernels_ingest.hip mask_low_quals, slow_pair) on the host: bit 2 (seq_off[r] - seq_off[0]) + q is set when
// base q of read r has a quality below min_qv (at most 127) that is not 0xFF.
int jl_qmask_from_quals(uint64_t n_reads, const uint64_t *seq_off, const uint8_t *qual, const uint64_t *qual_off, uint32_t min_qv,
                        uint8_t *qmask, uint64_t qmask_bytes)
{
    if (!seq_off || !qual_off || (!qmask && qmask_bytes)) return JL_ERR_ARG;
    for (uint64_t r = 0; r < n_reads; ++r)
        if (seq_off[r + 1] < seq_off[r] || qual_off[r + 1] < qual_off[r]) return JL_ERR_ARG;
    if (qmask_bytes < jl_qmask_bytes(seq_off[n_reads] - seq_off[0])) return JL_ERR_ARG;
    for (uint64_t r = 0; r < n_reads; ++r)      // (a read's bits lie inside its own bytes of the bases: two a byte)
        if (qual_off[r + 1] - qual_off[r] > 2u * (seq_off[r + 1] - seq_off[r])) return JL_ERR_ARG;
    if (qmask_bytes) memset(qmask, 0, (size_t)qmask_bytes);
    if (n_reads && !qual && qual_off[n_reads] != qual_off[0]) return JL_ERR_ARG;
    const uint32_t t = std::min<uint32_t>(min_qv, 127u);
    for (uint64_t r = 0; r < n_reads; ++r) {
        const uint8_t *q = qual + qual_off[r];
        const uint64_t n = qual_off[r + 1] - qual_off[r], i0 = 2u * (seq_off[r] - seq_off[0]);
        for (uint64_t b = 0; b < n; ++b)
            if (q[b] < t && q[b] != 0xFFu) qmask[(i0 + b) >> 3] |= (uint8_t)(1u << ((i0 + b) & 7u));
    }
    return JL_OK;
}

// jl_records_append (qmask null, masked false) and jl_records_append_masked (no qualities, masked true)
static int records_append(jl_ctx *ctx, uint64_t n_reads, const int32_t *pos, const uint32_t *cigar, const uint64_t *cig_off,
                          const uint8_t *seq4, const uint64_t *seq_off, const uint8_t *qual, const uint64_t *qual_off,
                          const uint8_t *qmask, bool masked)
{
    jl_records &R = ctx->rec;
    if (!R.open) return jl_fail(ctx, JL_ERR_STATE, "jl_records_append before jl_records_begin");
    if (masked && !qmask) {
        records_drop(ctx);
        return jl_fail(ctx, JL_ERR_ARG, "jl_records_append_masked: no mask (a stream without a filter takes jl_records_append without qualities)");
    }
    if (R.n_reads && masked != R.masked) {
        records_drop(ctx);
        return jl_fail(ctx, JL_ERR_ARG, "records: either every chunk carries a mask (jl_records_append_masked) or none does");
    }
    if (R.n_reads && (qual != nullptr) != R.have_qual) {
        records_drop(ctx);
        return jl_fail(ctx, JL_ERR_ARG, "records: either every chunk carries qualities or none does");
    }
    if (!n_reads) return JL_OK;
    // a chunk that fails validation ends the stream (jl_records_begin starts over).  Here: the offsets, which the uploads
    // below follow; what the cigars say — an 'M', more bases than the record holds — is checked where they are walked, on
    // the device (cigar_walk_kernel, cigar_runs_kernel for long reads), and reported by the build (jl_records_finish /
    // jl_records_window): the loop over twelve million cigar words was most of an append on the host.
    for (uint64_t r = 0; r < n_reads; ++r)
        if (cig_off[r + 1] < cig_off[r] || seq_off[r + 1] < seq_off[r] || (qual && qual_off[r + 1] < qual_off[r])) {
            const unsigned long long at = R.n_reads + r;
            records_drop(ctx);
            return jl_fail(ctx, JL_ERR_ARG, "record %llu: offsets must not decrease", at);
        }
    // ... and whether a read needs the ingest's launch for long reads: only a read with more ops than entries fit can, and a CCS
    // sample has few of those — their cigars are looked at here, a word per read of the chunk at most (then: "maybe").  Only
    // behind the check of EVERY offset: then each read's cigar lies within [cig_off[0], cig_off[n_reads]), the caller's array.
    const uint64_t short_ops = jl_ingest_short_ops();
    uint64_t looked = 0;
    for (uint64_t r = 0; r < n_reads; ++r) {
        const uint64_t n_ops = cig_off[r + 1] - cig_off[r];
        if (n_ops > short_ops && !R.maybe_long) {
            looked += n_ops;
            R.maybe_long = looked > n_reads + 4096u || jl_ingest_read_is_long(cigar + cig_off[r], n_ops);
        }
    }
    // ... and the chunk's 'I' ops, which size the allele table of a build that tracks insertion alleles (docs/SPEC.md §17; whether
    // one will is not known here: the switch belongs to the window).  A compare and an add a word, no branch.
    uint64_t n_ins = 0;
    for (uint64_t k = cig_off[0]; k < cig_off[n_reads]; ++k) n_ins += (cigar[k] & 15u) == 1u;
    JL_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // the chunk's arrays start wherever its offsets say; on the device everything is one run of arrays
    const uint64_t c0 = cig_off[0], s0 = seq_off[0], q0 = qual ? qual_off[0] : 0;
    const size_t n_cig = (size_t)(cig_off[n_reads] - c0), n_seq = (size_t)(seq_off[n_reads] - s0),
                 n_q = qual ? (size_t)(qual_off[n_reads] - q0) : 0;
    const size_t nr = (size_t)R.n_reads;
    // A masked stream's chunks begin on 16 bytes of the resident bases (offsets may leave gaps: nobody's bases), so that the chunk's
    // mask — a bit per nibble, relative to the chunk's first base — begins on a dword of the resident mask, at a quarter of the
    // bases' offset: bit 2 x byte + nibble, for every read of the stream, which is where the kernels look.
    const uint64_t seq_at = masked ? (R.n_seq + 15u) & ~(uint64_t)15u : R.n_seq;
    const size_t n_mask = masked ? (size_t)jl_qmask_bytes(n_seq) : 0;
    hipError_t e = R.pos.grow_keep(st, nr, nr + n_reads, 0);
    if (e == hipSuccess) e = R.co.grow_keep(st, nr + 1, nr + n_reads + 1, 0);
    if (e == hipSuccess) e = R.so.grow_keep(st, nr + 1, nr + n_reads + 1, 0);
    if (e == hipSuccess) e = R.cig.grow_keep(st, (size_t)R.n_cig, (size_t)R.n_cig + n_cig, 64);
    // the kernel reads the bases in aligned 32-byte pieces: padding behind them
    if (e == hipSuccess) e = R.seq.grow_keep(st, (size_t)R.n_seq, (size_t)seq_at + n_seq, 64);
    // (the mask's share of those 64 bytes: a piece's dword of flags lies inside the allocation wherever the piece does)
    // (its first allocation follows the bases' — the hint of jl_records_begin — so that it grows when they do, not chunk after chunk)
    if (e == hipSuccess && masked)
        e = R.mask.grow_keep(st, (size_t)jl_qmask_bytes(R.n_seq), std::max((size_t)(seq_at / 4u) + n_mask, R.mask ? (size_t)0 : R.seq.cap / 4u), 16);
    if (e == hipSuccess && qual) e = R.qual.grow_keep(st, (size_t)R.n_qual, (size_t)R.n_qual + n_q, 64);
    if (e == hipSuccess && qual) e = R.qo.grow_keep(st, nr + 1, nr + n_reads + 1, 0);
    std::vector<uint64_t> off((size_t)(n_reads + 1) * (qual ? 3 : 2));
    uint64_t *co = off.data(), *so = co + n_reads + 1, *qo = so + n_reads + 1;
    for (uint64_t r = 0; r <= n_reads; ++r) {
        co[r] = cig_off[r] - c0 + R.n_cig;
        so[r] = seq_off[r] - s0 + seq_at;
        if (qual) qo[r] = qual_off[r] - q0 + R.n_qual;
    }
    const size_t off_bytes = (size_t)(n_reads + 1) * 8;
    if (e == hipSuccess && n_seq) e = hipMemcpyAsync(R.seq + seq_at, seq4 + s0, n_seq, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && n_mask) e = hipMemcpyAsync(R.mask + seq_at / 4u, qmask, n_mask, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && n_cig) e = hipMemcpyAsync(R.cig + R.n_cig, cigar + c0, n_cig * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(R.co + nr, co, off_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(R.so + nr, so, off_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(R.pos + nr, pos, (size_t)n_reads * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && qual && n_q) e = hipMemcpyAsync(R.qual + R.n_qual, qual + q0, n_q, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && qual) e = hipMemcpyAsync(R.qo + nr, qo, off_bytes, hipMemcpyHostToDevice, st);
    // the caller may reuse its chunk buffers (and `off` goes away) as soon as this returns
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        records_drop(ctx);
        return hip_fail(ctx, "records", e);
    }
    R.have_qual = qual != nullptr;
    R.masked = masked;
    R.n_reads += n_reads;
    R.n_cig += n_cig;
    R.n_ins_ops += n_ins;
    R.n_seq = seq_at + n_seq;
    R.n_qual += n_q;
    return JL_OK;
}

int jl_records_append(jl_ctx *ctx, uint64_t n_reads, const int32_t *pos, const uint32_t *cigar, const uint64_t *cig_off,
                      const uint8_t *seq4, const uint64_t *seq_off, const uint8_t *qual, const uint64_t *qual_off)
{
    if (!ctx || !pos || !cigar || !cig_off || !seq4 || !seq_off || (qual && !qual_off)) return JL_ERR_ARG;
    return records_append(ctx, n_reads, pos, cigar, cig_off, seq4, seq_off, qual, qual_off, nullptr, false);
}

int jl_records_append_masked(jl_ctx *ctx, uint64_t n_reads, const int32_t *pos, const uint32_t *cigar, const uint64_t *cig_off,
                             const uint8_t *seq4, const uint64_t *seq_off, const uint8_t *qmask)
{
    if (!ctx || !pos || !cigar || !cig_off || !seq4 || !seq_off) return JL_ERR_ARG;
    return records_append(ctx, n_reads, pos, cigar, cig_off, seq4, seq_off, nullptr, nullptr, qmask, true);
}

// What the last record ingest into `ctx` found wrong with the records (its kernels have run): the first malformed read.
// Called by the blocking builds, and by the first blocking call behind an enqueued one (jl_sync, jl_run_wait, the fetches).
int jl_ingest_verdict(jl_ctx *ctx)
{
    if (!ctx->ing.check_pending) return JL_OK;
    ctx->ing.check_pending = false;
    // (through the context's pinned block: a process's first pageable device-to-host copy costs the runtime milliseconds)
    unsigned long long both[2] = {0, ~0ull};     // (the counters, the verdict: kernels_ingest.hip jl_launch_ingest)
    if (int rc = jl_fetch_to_host(ctx, ctx->ing.d_count, 16, both, 64)) return rc;
    const unsigned long long w = both[1];
    if (w == ~0ull) return JL_OK;
    // (read: the word is all ones again for the builds to come — behind whatever this context has enqueued)
    JL_HIP(ctx, hipMemsetAsync(ctx->ing.d_count + 2, 0xFF, 8, ctx->stream));
    const unsigned long long r = w >> 8;
    const unsigned code = (unsigned)(w & 0xFFu);
    ctx->pileup_done = ctx->call_done = ctx->phase_done = false;
    if (code == 1u) return jl_fail(ctx, JL_ERR_ARG, "record %llu: cigar M is forbidden in PacBio-compliant BAM (doc/JULIET.md:53)", r);
    if (code == 4u) return jl_fail(ctx, JL_ERR_ARG, "record %llu: its cigar spans 2^30 reference bases or more", r);
    if (code == 5u) return jl_fail(ctx, JL_ERR_STATE, "record %llu: a long cigar the upload had not seen (jl_ingest_read_is_long and cigar_walk_kernel disagree)", r);
    return jl_fail(ctx, JL_ERR_ARG, "record %llu: its cigar consumes more %s than the record holds", r, code == 2u ? "bases" : "qualities");
}
}  // extern "C"

// the insertion counters of `dst` for n_cols columns, zeroed on its stream
static hipError_t reserve_insertions(jl_ctx *dst, uint32_t n_cols)
{
    bool moved;   // (no run and no stage touches the counters: no captured graph to tell)
    hipError_t e = dst->d_ins_len.reserve_exact((size_t)n_cols * JL_INS_LEN_BINS, &moved);
    if (e == hipSuccess) e = dst->d_ins_base.reserve_exact((size_t)n_cols * JL_INS_MAX_BASES * 4, &moved);
    if (e == hipSuccess) e = hipMemsetAsync(dst->d_ins_len, 0, (size_t)n_cols * JL_INS_LEN_BINS * 4, dst->stream);
    if (e == hipSuccess) e = hipMemsetAsync(dst->d_ins_base, 0, (size_t)n_cols * JL_INS_MAX_BASES * 16, dst->stream);
    return e;
}

// the junction counters and the allele table of `dst` for a build from R, emptied on its stream (docs/SPEC.md §17)
static hipError_t reserve_insertion_alleles(jl_ctx *dst, const jl_records &R, uint32_t n_cols)
{
    hipStream_t st = dst->stream;
    uint64_t slots = 64;   // a power of two, at least twice the 'I' ops: an allele needs one
    while (slots < 2u * R.n_ins_ops) slots *= 2u;
    dst->insal_slots = slots;
    hipError_t e = dst->insal_jcnt.grow_discard(st, (size_t)n_cols * 4u);
    if (e == hipSuccess) e = dst->insal_keys.grow_discard(st, (size_t)slots * 2u);
    if (e == hipSuccess) e = dst->insal_count.grow_discard(st, (size_t)slots * 2u + 1u);
    if (e == hipSuccess) e = hipMemsetAsync(dst->insal_jcnt, 0, (size_t)n_cols * 16u, st);
    if (e == hipSuccess) e = hipMemsetAsync(dst->insal_keys, 0xFF, (size_t)slots * 16u, st);
    // (the counts and n_occ; occ[] between them is written before it is read)
    if (e == hipSuccess) e = hipMemsetAsync(dst->insal_count, 0, ((size_t)slots * 2u + 1u) * 4u, st);
    return e;
}

// the event rows of `dst` for a build from R that tracks reads, their counter zeroed on its stream (docs/SPEC.md §19): a row an
// 'I' op, since an event needs one (R.n_ins_ops fits 32 bits: records_build)
static hipError_t reserve_insertion_events(jl_ctx *dst, const jl_records &R)
{
    hipStream_t st = dst->stream;
    dst->insev_cap = (uint32_t)R.n_ins_ops;
    hipError_t e = dst->insev_rows.grow_discard(st, (size_t)R.n_ins_ops);
    if (e == hipSuccess) e = dst->insev_count.grow_discard(st, 1);
    if (e == hipSuccess) e = hipMemsetAsync(dst->insev_count, 0, 4u, st);
    return e;
}

// the record walk of a tracking build: the filter as jl_launch_ingest resolves it
static void launch_insertion_alleles(jl_ctx *dst, const jl_records &R, uint32_t min_qv)
{
    const jl_qv_mode mode = jl_qv_mode_of(R.have_qual, R.masked, min_qv);
    jl_insal_args a = {};
    a.n_reads = dst->n_reads, a.n_cols = dst->n_cols, a.win_begin = dst->win_begin;
    a.min_qv = std::min<uint32_t>(min_qv, 127u);
    a.pos = R.pos, a.cigar = R.cig, a.cig_off = R.co, a.seq4 = R.seq, a.seq_off = R.so;
    a.qual = mode == JL_QV_BYTES ? R.qual : nullptr;
    a.qual_off = mode == JL_QV_BYTES ? R.qo : nullptr;
    a.qmask = mode == JL_QV_MASK ? R.mask : nullptr;
    a.jcnt = dst->insal_jcnt;
    a.key0 = dst->insal_keys, a.key1 = dst->insal_keys + dst->insal_slots;
    a.count = dst->insal_count, a.occ = dst->insal_count + dst->insal_slots, a.n_occ = dst->insal_count + 2u * dst->insal_slots;
    a.slots_mask = dst->insal_slots - 1u;
    if (dst->track_ins_reads) a.events = dst->insev_rows, a.n_events = dst->insev_count, a.events_cap = dst->insev_cap;
    jl_launch_insertion_alleles(&a, dst->stream);
}

// The resident matrix of `dst` from the records uploaded to `src` (the same context for jl_records_finish; another one of
// the same device when one upload feeds several column windows).  The records stay.  Everything is ENQUEUED on dst's
// stream (three launches + the insertion counters and the insertion alleles when asked for); `wait`: return when it has run.
static int records_build(jl_ctx *src, jl_ctx *dst, uint32_t n_cols, uint32_t win_begin, uint32_t min_qv, bool wait)
{
    const jl_records &R = src->rec;
    const bool track_alleles = dst->track_ins_alleles || dst->track_ins_reads;   // (the events imply the alleles: docs/SPEC.md §19)
    if (dst->track_ins_reads && R.n_ins_ops > 0xFFFFFFFFull)
        return jl_fail(dst, JL_ERR_ARG, "records: %llu 'I' ops, the event list of jl_msa_track_insertion_reads holds 2^32 - 1", (unsigned long long)R.n_ins_ops);
    // (a stream nothing was appended to ends here, "empty matrix": what follows never sees zero reads)
    int rc = jl_msa_alloc(dst, R.n_reads, n_cols, win_begin);
    if (rc) return rc;
    hipStream_t st = dst->stream;
    jl_ingest_scratch &S = dst->ing;
    const uint32_t ns = jl_ingest_sweeps(n_cols);
    const size_t nr = (size_t)R.n_reads;
    hipError_t e = S.runs.grow_discard(st, (size_t)R.n_cig + 3 * nr + 8);   // (three entries around a read's runs; + 8: the planes kernel reads entries four and eight at a time)
    if (e == hipSuccess) e = S.nruns.grow_discard(st, nr + 1);
    if (e == hipSuccess) e = S.desc.grow_discard(st, (nr + 1) * ns);
    if (e == hipSuccess) e = S.slow.grow_discard(st, jl_ingest_slow_room(dst));
    if (e == hipSuccess && !S.d_count) {
        bool moved;
        e = S.d_count.reserve_exact(16, &moved);
        // (counters zero, the verdict word — [2..3] — all ones: no malformed record seen; kernels_ingest.hip jl_launch_ingest)
        if (e == hipSuccess) e = hipMemsetAsync(S.d_count, 0, 64, st);
        if (e == hipSuccess) e = hipMemsetAsync(S.d_count + 2, 0xFF, 8, st);
    }
    dst->ins_valid = false;
    if (e == hipSuccess && dst->track_insertions) {
        e = reserve_insertions(dst, n_cols);
        if (e == hipSuccess) {
            jl_launch_insertions(dst, R);
            e = hipGetLastError();
            dst->ins_valid = e == hipSuccess;
        }
    }
    dst->insal_valid = dst->insev_valid = false;
    if (e == hipSuccess && track_alleles) {
        e = reserve_insertion_alleles(dst, R, n_cols);
        if (e == hipSuccess && dst->track_ins_reads) e = reserve_insertion_events(dst, R);
        if (e == hipSuccess) {
            launch_insertion_alleles(dst, R, min_qv);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess) {
        jl_launch_ingest(dst, R, min_qv);
        e = hipGetLastError();
        S.check_pending = e == hipSuccess;
        if (e == hipSuccess && track_alleles) {   // the reads spanning every junction, from the planes just built
            if (n_cols >= 2u) {
                jl_insal_span_args sa = {};
                sa.msa = dst->d_msa, sa.plane_stride = dst->plane_stride;   // (a multiple of 16, >= ceil(n_reads / 8): set_shape)
                sa.n_reads = dst->n_reads, sa.n_cols = n_cols;
                sa.jcnt = dst->insal_jcnt;
                jl_launch_junction_span(&sa, st);
                e = hipGetLastError();
            }
            dst->insal_valid = e == hipSuccess;
            dst->insev_valid = dst->insal_valid && dst->track_ins_reads;
        }
        if (e == hipSuccess && wait) e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess) return hip_fail(dst, "ingest", e);
    return wait ? jl_ingest_verdict(dst) : JL_OK;
}

// jl_records_window (`wait`) and jl_records_window_async, `fn` the one that was called
static int records_window(const char *fn, jl_ctx *records, jl_ctx *window, uint32_t n_cols, uint32_t win_begin, uint32_t min_qv, bool wait)
{
    if (!records || !window) return JL_ERR_ARG;
    if (!records->rec.open) return jl_fail(window, JL_ERR_STATE, "%s: no records uploaded (jl_records_begin / _append)", fn);
    if (records->device != window->device) return jl_fail(window, JL_ERR_ARG, "records and window are on different devices");
    JL_HIP(window, hipSetDevice(window->device));
    if (wait) JL_HIP(window, hipStreamSynchronize(records->stream));   // the uploads are complete
    return records_build(records, window, n_cols, win_begin, min_qv, wait);
}

// jl_msa_ingest_records (qmask null, masked false) and jl_msa_ingest_records_masked (no qualities, masked true): one chunk, built at once
static int ingest_records(jl_ctx *ctx, uint64_t n_reads, uint32_t n_cols, uint32_t win_begin, const int32_t *pos, const uint32_t *cigar,
                          const uint64_t *cig_off, const uint8_t *seq4, const uint64_t *seq_off, const uint8_t *qual,
                          const uint64_t *qual_off, const uint8_t *qmask, bool masked, uint32_t min_qv)
{
    if (!ctx || !pos || !cigar || !cig_off || !seq4 || !seq_off || (qual && !qual_off)) return JL_ERR_ARG;
    int rc = jl_records_begin(ctx, n_reads, cig_off[n_reads] - cig_off[0], seq_off[n_reads] - seq_off[0],
                              qual ? std::max<uint64_t>(qual_off[n_reads] - qual_off[0], 1) : 0);
    if (rc == JL_OK) rc = records_append(ctx, n_reads, pos, cigar, cig_off, seq4, seq_off, qual, qual_off, qmask, masked);
    if (rc == JL_OK) rc = jl_records_finish(ctx, n_cols, win_begin, min_qv);
    else if (ctx->rec.open) records_drop(ctx);
    return rc;
}

extern "C" {

int jl_records_finish(jl_ctx *ctx, uint32_t n_cols, uint32_t win_begin, uint32_t min_qv)
{
    if (!ctx) return JL_ERR_ARG;
    if (!ctx->rec.open) return jl_fail(ctx, JL_ERR_STATE, "jl_records_finish before jl_records_begin");
    JL_HIP(ctx, hipSetDevice(ctx->device));
    const int rc = records_build(ctx, ctx, n_cols, win_begin, min_qv, true);
    records_drop(ctx);
    return rc;
}

int jl_records_window(jl_ctx *records, jl_ctx *window, uint32_t n_cols, uint32_t win_begin, uint32_t min_qv)
{
    return records_window("jl_records_window", records, window, n_cols, win_begin, min_qv, true);
}

// The same, enqueued only: the window's matrix is complete when the window's stream reaches this point — a run enqueued
// behind it on that stream (jl_run_async) reads it.  No allocation once a window of this shape has been built on `window`.
int jl_records_window_async(jl_ctx *records, jl_ctx *window, uint32_t n_cols, uint32_t win_begin, uint32_t min_qv)
{
    return records_window("jl_records_window_async", records, window, n_cols, win_begin, min_qv, false);
}

int jl_records_drop(jl_ctx *ctx)
{
    if (!ctx) return JL_ERR_ARG;
    JL_HIP(ctx, hipSetDevice(ctx->device));
    records_drop(ctx);
    return JL_OK;
}

int jl_msa_ingest_records(jl_ctx *ctx, uint64_t n_reads, uint32_t n_cols, uint32_t win_begin, const int32_t *pos,
                          const uint32_t *cigar, const uint64_t *cig_off, const uint8_t *seq4, const uint64_t *seq_off,
                          const uint8_t *qual, const uint64_t *qual_off, uint32_t min_qv)
{
    return ingest_records(ctx, n_reads, n_cols, win_begin, pos, cigar, cig_off, seq4, seq_off, qual, qual_off, nullptr, false, min_qv);
}

int jl_msa_ingest_records_masked(jl_ctx *ctx, uint64_t n_reads, uint32_t n_cols, uint32_t win_begin, const int32_t *pos,
                                 const uint32_t *cigar, const uint64_t *cig_off, const uint8_t *seq4, const uint64_t *seq_off,
                                 const uint8_t *qmask, uint32_t min_qv)
{
    return ingest_records(ctx, n_reads, n_cols, win_begin, pos, cigar, cig_off, seq4, seq_off, nullptr, nullptr, qmask, true, min_qv);
}

int jl_msa_track_insertions(jl_ctx *ctx, int on)
{
    if (!ctx) return JL_ERR_ARG;
    ctx->track_insertions = on != 0;
    return JL_OK;
}

int jl_insertions_fetch(jl_ctx *ctx, uint32_t *len_hist, uint32_t *base_counts)
{
    if (!ctx) return JL_ERR_ARG;
    if (!ctx->ins_valid) return jl_fail(ctx, JL_ERR_STATE, "no insertion counts: jl_msa_track_insertions(ctx, 1) before jl_msa_ingest_records");
    JL_HIP(ctx, hipSetDevice(ctx->device));
    if (len_hist) JL_HIP(ctx, hipMemcpyAsync(len_hist, ctx->d_ins_len, (size_t)ctx->n_cols * JL_INS_LEN_BINS * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (base_counts) JL_HIP(ctx, hipMemcpyAsync(base_counts, ctx->d_ins_base, (size_t)ctx->n_cols * JL_INS_MAX_BASES * 16, hipMemcpyDeviceToHost, ctx->stream));
    JL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JL_OK;
}

}  // extern "C"
