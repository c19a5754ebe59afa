// capi_orf.hip — jl_read_orf_async / _fetch of include/juliet_hip.h: per (span, read) of the resident matrix the covered cells, the
// gap cells, the codons read in full, the stop codons the reference does not have and the first of them (docs/SPEC.md §27); and the
// host-only rules on top of them: jl_orf_classify turns the counters into flags, jl_orf_filter the flags into the indices
// jl_msa_take takes.
// The stage call owns its buffers and touches nothing else of the context: no stage result, no plan, no captured graph sees it.
// Every size the kernels (kernels_orf.hip) form an address from is checked here.
#include <string.h>

#include <algorithm>

#include "jl_internal.h"
#include "orf_shape.h"

static_assert(JL_ORF_SHAPE_MAX_SPANS == JL_ORF_MAX_SPANS, "orf_shape.h and juliet_hip.h name one bound");
static_assert(sizeof(jl_orf_seg) == 4 * sizeof(uint32_t), "the segment table travels as words");

#ifdef JL_TUNING
// hook of the -DJL_TUNING build (tools_tuning/orf_time.py): the slices of a counter (4 .. 6, 0: the shape's own) of every later
// call of this process
static int g_tune_k = 0;
extern "C" __attribute__((visibility("default"))) int jl_tuning_orf_shape(int k)
{
    if (k != 0 && (k < 4 || k > 6)) return JL_ERR_ARG;
    g_tune_k = k;
    return JL_OK;
}
#endif

extern "C" {

int jl_read_orf_async(jl_ctx *ctx, const jl_orf_span *spans, uint32_t n_spans, const uint8_t *ref)
{
    static const char *fn = "jl_read_orf_async";
    if (!ctx) return JL_ERR_ARG;
    if (!ctx->d_msa) return jl_fail(ctx, JL_ERR_STATE, "%s: no resident matrix", fn);
    if (!spans) return jl_fail(ctx, JL_ERR_ARG, "%s: no spans", fn);
    if (!ref) return jl_fail(ctx, JL_ERR_ARG, "%s: no reference row", fn);
    if (n_spans < 1u || n_spans > JL_ORF_MAX_SPANS) return jl_fail(ctx, JL_ERR_ARG, "%s: %u spans, not 1 .. %d", fn, n_spans, (int)JL_ORF_MAX_SPANS);
    uint32_t n_codons[JL_ORF_MAX_SPANS];
    for (uint32_t g = 0; g < n_spans; ++g) {
        if (spans[g].n_codons < 1u || (uint64_t)spans[g].col + 3ull * spans[g].n_codons > ctx->n_cols)
            return jl_fail(ctx, JL_ERR_ARG, "%s: span %u (column %u, %u codons) is empty or outside the window of %u columns", fn, g, spans[g].col, spans[g].n_codons, ctx->n_cols);
        n_codons[g] = spans[g].n_codons;
    }
    const uint64_t n_words = (ctx->n_reads + 31u) / 32u;
    // (a multiple of 16, >= ceil(n_reads / 8): set_shape, jl_msa_adopt — so every word with a read lies within a plane row)
    if (4u * n_words > ctx->plane_stride) return jl_fail(ctx, JL_ERR_ARG, "%s: plane stride %llu holds no %llu reads", fn, (unsigned long long)ctx->plane_stride, (unsigned long long)ctx->n_reads);
    uint32_t k = JL_ORF_K;
#ifdef JL_TUNING
    if (g_tune_k) k = (uint32_t)g_tune_k;
#endif
    const jl_orf_shape shape = jl_orf_shape_for(n_codons, n_spans, ctx->n_reads, k);
    // the grids: segments x chunks of the counting kernel, 1024 reads a workgroup of the combining one
    if (shape.grid > 0x7FFFFFFFull || (ctx->n_reads + 1023u) / 1024u > 0x7FFFFFFFull)
        return jl_fail(ctx, JL_ERR_ARG, "%s: %llu reads x %u spans are more workgroups than a launch takes", fn, (unsigned long long)ctx->n_reads, n_spans);
    JL_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t per_kind = (size_t)n_spans * ctx->n_reads;
    const size_t tab_words = 4u * (size_t)shape.n_segs + n_spans + 1u;
    ctx->orf_reads = 0, ctx->orf_spans = 0;   // (what was fetchable is gone as soon as a buffer may move)
    uint8_t *h = nullptr;
    uint32_t *tab = nullptr;
    hipError_t e = ctx->orf_ref.host(ctx->n_cols, &h);
    if (e == hipSuccess) {
        memcpy(h, ref, ctx->n_cols);
        e = ctx->orf_ref.upload(st, ctx->n_cols);
    }
    if (e == hipSuccess) e = ctx->orf_tab.host(tab_words, &tab);
    if (e == hipSuccess) {
        // the segments of span 0 first, each span's in codon order (orf_shape.h: segment s begins at codon s * seg_codons)
        jl_orf_seg *segs = reinterpret_cast<jl_orf_seg *>(tab);
        uint32_t *span_seg0 = tab + 4u * (size_t)shape.n_segs;
        uint32_t at = 0;
        for (uint32_t g = 0; g < n_spans; ++g) {
            span_seg0[g] = at;
            for (uint32_t s = 0; s < shape.span_segs[g]; ++s, ++at) {
                const uint32_t first = s * shape.seg_codons;
                segs[at] = {spans[g].col + 3u * first, std::min(shape.seg_codons, n_codons[g] - first), g, first};
            }
        }
        span_seg0[n_spans] = at;   // (== shape.n_segs)
        e = ctx->orf_tab.upload(st, tab_words);
    }
    if (e == hipSuccess) e = ctx->orf_out.grow_discard(st, (JL_ORF_COUNTERS + 1u) * per_kind);
    if (e == hipSuccess) e = ctx->orf_part.grow_discard(st, jl_orf_part_words(&shape));
    if (e == hipSuccess) {
        jl_orf_args A = {};
        A.msa = ctx->d_msa, A.plane_stride = ctx->plane_stride;
        A.n_reads = ctx->n_reads, A.n_cols = ctx->n_cols, A.n_words = (uint32_t)n_words;
        A.n_spans = n_spans;
        A.ref = (const uint8_t *)ctx->orf_ref.dev;
        A.segs = reinterpret_cast<const jl_orf_seg *>((const uint32_t *)ctx->orf_tab.dev);
        A.span_seg0 = (const uint32_t *)ctx->orf_tab.dev + 4u * (size_t)shape.n_segs;
        A.part = ctx->orf_part;
        A.counts = ctx->orf_out;
        A.first_stop = ctx->orf_out + JL_ORF_COUNTERS * per_kind;
        jl_launch_orf_counts(&A, &shape, st);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return jl_fail(ctx, jl_hip_status(e), "%s: %s", fn, hipGetErrorString(e));
    ctx->orf_reads = ctx->n_reads, ctx->orf_spans = n_spans;
    return JL_OK;
}

int jl_read_orf_fetch(jl_ctx *ctx, uint32_t *counts, uint32_t *first_stop)
{
    if (!ctx) return JL_ERR_ARG;
    if (!ctx->orf_reads) return jl_fail(ctx, JL_ERR_STATE, "jl_read_orf_fetch before jl_read_orf_async");
    JL_HIP(ctx, hipSetDevice(ctx->device));
    const size_t per_kind = (size_t)ctx->orf_spans * ctx->orf_reads;
    if (counts) JL_HIP(ctx, hipMemcpyAsync(counts, ctx->orf_out, JL_ORF_COUNTERS * per_kind * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (first_stop) JL_HIP(ctx, hipMemcpyAsync(first_stop, ctx->orf_out + JL_ORF_COUNTERS * per_kind, per_kind * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    JL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JL_OK;
}

// the flags of every (span, read) (docs/SPEC.md §27); the counters are checked against their spans first: a refused call writes nothing
int jl_orf_classify(const uint32_t *counts, const uint32_t *first_stop, const jl_orf_span *spans, uint32_t n_spans, uint64_t n_reads,
                    const jl_orf_rule *rule, uint8_t *flags)
{
    static const char *fn = "jl_orf_classify";
    if (!counts || !first_stop || !spans || !rule || !flags) return jl_fail(nullptr, JL_ERR_ARG, "%s: a NULL argument", fn);
    if (n_spans < 1u || n_spans > JL_ORF_MAX_SPANS) return jl_fail(nullptr, JL_ERR_ARG, "%s: %u spans, not 1 .. %d", fn, n_spans, (int)JL_ORF_MAX_SPANS);
    if (n_reads > 0xFFFFFFFFull) return jl_fail(nullptr, JL_ERR_ARG, "%s: %llu reads, an index is 32 bits", fn, (unsigned long long)n_reads);
    const uint64_t per_kind = (uint64_t)n_spans * n_reads;
    const uint32_t *covered = counts + JL_ORF_COVERED * per_kind, *gaps = counts + JL_ORF_GAP_CELLS * per_kind;
    const uint32_t *read = counts + JL_ORF_CODONS_READ * per_kind, *stops = counts + JL_ORF_STOPS * per_kind;
    for (uint32_t g = 0; g < n_spans; ++g) {
        const uint64_t n = spans[g].n_codons;
        for (uint64_t i = 0; i < n_reads; ++i) {
            const uint64_t e = g * n_reads + i;
            const char *why = covered[e] > 3u * n ? "more covered cells than the span has" : gaps[e] > covered[e] ? "more gap cells than covered cells"
                              : stops[e] > read[e] ? "more stops than codons read" : first_stop[e] != JL_ORF_NO_STOP && first_stop[e] >= n ? "a first stop outside the span" : nullptr;
            if (why) return jl_fail(nullptr, JL_ERR_ARG, "%s: span %u, read %llu: %s", fn, g, (unsigned long long)i, why);
        }
    }
    for (uint32_t g = 0; g < n_spans; ++g) {
        const uint64_t n = spans[g].n_codons;
        const uint64_t body = n - std::min<uint64_t>(rule->tail_codons, n);   // codons before the tail
        for (uint64_t i = 0; i < n_reads; ++i) {
            const uint64_t e = g * n_reads + i;
            uint8_t f = 0;
            if (covered[e] < 3u * n) f |= JL_ORF_PARTIAL;
            if (first_stop[e] < body) f |= JL_ORF_STOP;   // (JL_ORF_NO_STOP is below no body)
            if (gaps[e] % 3u != 0u) f |= JL_ORF_FRAMESHIFT;
            if (rule->max_gap_cells > 0u && gaps[e] >= rule->max_gap_cells) f |= JL_ORF_DELETION;
            flags[e] = f;
        }
    }
    return JL_OK;
}

// the reads no span of which meets the mask (docs/SPEC.md §27)
int jl_orf_filter(const uint8_t *flags, uint32_t n_spans, uint64_t n_reads, uint32_t mask, uint32_t *idx, uint64_t *n_kept, uint64_t *n_flagged)
{
    static const char *fn = "jl_orf_filter";
    if (!flags || !idx || !n_kept || !n_flagged) return jl_fail(nullptr, JL_ERR_ARG, "%s: a NULL argument", fn);
    if (n_spans < 1u || n_spans > JL_ORF_MAX_SPANS) return jl_fail(nullptr, JL_ERR_ARG, "%s: %u spans, not 1 .. %d", fn, n_spans, (int)JL_ORF_MAX_SPANS);
    if (n_reads > 0xFFFFFFFFull) return jl_fail(nullptr, JL_ERR_ARG, "%s: %llu reads, an index is 32 bits", fn, (unsigned long long)n_reads);
    if (mask == 0u || (mask & ~(uint32_t)(JL_ORF_STOP | JL_ORF_FRAMESHIFT | JL_ORF_DELETION)))
        return jl_fail(nullptr, JL_ERR_ARG, "%s: mask %u is no non-empty subset of STOP | FRAMESHIFT | DELETION", fn, mask);
    uint64_t kept = 0;
    for (uint64_t i = 0; i < n_reads; ++i) {
        uint32_t any = 0;
        for (uint32_t g = 0; g < n_spans; ++g) any |= flags[g * n_reads + i];
        if (!(any & mask)) idx[kept++] = (uint32_t)i;
    }
    *n_kept = kept;
    *n_flagged = n_reads - kept;
    return JL_OK;
}

}  // extern "C"
