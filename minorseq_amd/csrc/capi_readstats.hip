// capi_readstats.hip — jl_read_stats_async / _fetch of include/juliet_hip.h: per read of the resident matrix its bases, gaps,
// masked cells, bases in compared columns and mismatches among those, over all columns of the window (docs/SPEC.md §20), and the
// host-only rule that turns the five counters into the indices jl_msa_take takes (jl_read_filter).  The call owns its buffers and
// touches nothing else of the context: no stage result, no plan, no captured graph sees it.  Every size the kernels
// (kernels_readstats.hip) form an address from is checked here.
#include <string.h>

#include "jl_internal.h"
#include "readstats_shape.h"

#ifdef JL_TUNING
// hook of the -DJL_TUNING build (tools_tuning/read_stats_time.py): the slices of a counter (4 .. 6, 0: the shape's own) and the
// combine form (JL_RS_COMBINE_*, negative: the shape's own) of every later call of this process
static int g_tune_k = 0, g_tune_combine = -1;
extern "C" __attribute__((visibility("default"))) int jl_tuning_read_stats_shape(int k, int combine)
{
    if ((k != 0 && (k < 4 || k > 6)) || combine > JL_RS_COMBINE_ATOMIC) return JL_ERR_ARG;
    g_tune_k = k, g_tune_combine = combine;
    return JL_OK;
}
#endif

extern "C" {

int jl_read_stats_async(jl_ctx *ctx, const uint8_t *compare)
{
    static const char *fn = "jl_read_stats_async";
    if (!ctx) return JL_ERR_ARG;
    if (!ctx->d_msa) return jl_fail(ctx, JL_ERR_STATE, "%s: no resident matrix", fn);
    const uint64_t n_words = (ctx->n_reads + 31u) / 32u;
    // (a multiple of 16, >= ceil(n_reads / 8): set_shape, jl_msa_adopt — so every word with a read lies within a plane row)
    if (4u * n_words > ctx->plane_stride) return jl_fail(ctx, JL_ERR_ARG, "%s: plane stride %llu holds no %llu reads", fn, (unsigned long long)ctx->plane_stride, (unsigned long long)ctx->n_reads);
    jl_readstats_shape shape = jl_readstats_shape_for(ctx->n_reads, ctx->n_cols);
#ifdef JL_TUNING
    if (g_tune_k) shape.k = (uint32_t)g_tune_k, shape.flush = (1u << shape.k) - 1u;
    if (g_tune_combine >= 0) shape.combine = (uint32_t)g_tune_combine;
#endif
    if ((uint64_t)shape.n_chunks * shape.n_segs > 0x7FFFFFFFull)
        return jl_fail(ctx, JL_ERR_ARG, "%s: %llu reads x %u columns are more workgroups than a launch takes", fn, (unsigned long long)ctx->n_reads, ctx->n_cols);
    JL_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t words = (size_t)JL_READ_STATS * ctx->n_reads;
    const bool atomic = shape.combine == JL_RS_COMBINE_ATOMIC;
    ctx->rs_reads = 0;   // (what was fetchable is gone as soon as a buffer may move)
    hipError_t e = hipSuccess;
    if (compare) {
        uint8_t *h = nullptr;
        e = ctx->rs_compare.host(ctx->n_cols, &h);
        if (e == hipSuccess) {
            memcpy(h, compare, ctx->n_cols);
            e = ctx->rs_compare.upload(st, ctx->n_cols);
        }
    }
    if (e == hipSuccess) e = ctx->rs_out.grow_discard(st, words);
    if (e == hipSuccess && !atomic) e = ctx->rs_part.grow_discard(st, jl_readstats_part_words(&shape));
    if (e == hipSuccess && atomic) e = hipMemsetAsync(ctx->rs_out, 0, words * sizeof(uint32_t), st);
    if (e == hipSuccess) {
        jl_readstats_args A = {};
        A.msa = ctx->d_msa, A.plane_stride = ctx->plane_stride;
        A.n_reads = ctx->n_reads, A.n_cols = ctx->n_cols, A.n_words = (uint32_t)n_words;
        A.compare = compare ? (const uint8_t *)ctx->rs_compare.dev : nullptr;
        A.part = atomic ? nullptr : (uint32_t *)ctx->rs_part;
        A.stats = ctx->rs_out;
        jl_launch_read_stats(&A, &shape, st);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return jl_fail(ctx, jl_hip_status(e), "%s: %s", fn, hipGetErrorString(e));
    ctx->rs_reads = ctx->n_reads;
    return JL_OK;
}

int jl_read_stats_fetch(jl_ctx *ctx, uint32_t *stats)
{
    if (!ctx) return JL_ERR_ARG;
    if (!ctx->rs_reads) return jl_fail(ctx, JL_ERR_STATE, "jl_read_stats_fetch before jl_read_stats_async");
    JL_HIP(ctx, hipSetDevice(ctx->device));
    if (stats)
        JL_HIP(ctx, hipMemcpyAsync(stats, ctx->rs_out, (size_t)JL_READ_STATS * ctx->rs_reads * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    JL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JL_OK;
}

// the reads a rule keeps (docs/SPEC.md §20): every product in IEEE double, left to right, as the header writes it
int jl_read_filter(const uint32_t *stats, uint64_t n_reads, const jl_read_rule *rule, uint32_t *idx, uint64_t *n_kept, uint64_t failed[5])
{
    static const char *fn = "jl_read_filter";
    if (!stats || !rule || !idx || !n_kept) return jl_fail(nullptr, JL_ERR_ARG, "%s: a NULL argument", fn);
    if (n_reads > 0xFFFFFFFFull) return jl_fail(nullptr, JL_ERR_ARG, "%s: %llu reads, an index is 32 bits", fn, (unsigned long long)n_reads);
    const double perc[3] = {rule->max_mismatch_perc, rule->max_gap_perc, rule->max_masked_perc};
    for (double x : perc)
        if (!(x < 0.0) && !(x <= 100.0)) return jl_fail(nullptr, JL_ERR_ARG, "%s: a percentage of %g, above 100", fn, x);
    uint64_t kept = 0, f[5] = {0, 0, 0, 0, 0};
    for (uint64_t i = 0; i < n_reads; ++i) {
        const uint32_t bases = stats[JL_READ_BASES * n_reads + i], gaps = stats[JL_READ_GAPS * n_reads + i];
        const uint32_t masked = stats[JL_READ_MASKED * n_reads + i], compared = stats[JL_READ_COMPARED * n_reads + i];
        const uint32_t mism = stats[JL_READ_MISMATCHES * n_reads + i];
        const uint64_t aligned = (uint64_t)bases + gaps, covered = aligned + masked;
        const bool fail[5] = {
            !(bases >= rule->min_bases),
            !(mism <= rule->max_mismatches),
            !(perc[0] < 0.0) && !(100.0 * (double)mism <= perc[0] * (double)compared),
            !(perc[1] < 0.0) && !(100.0 * (double)gaps <= perc[1] * (double)aligned),
            !(perc[2] < 0.0) && !(100.0 * (double)masked <= perc[2] * (double)covered),
        };
        bool keep = true;
        for (int r = 0; r < 5; ++r) f[r] += fail[r], keep = keep && !fail[r];
        if (keep) idx[kept++] = (uint32_t)i;
    }
    *n_kept = kept;
    if (failed) memcpy(failed, f, sizeof f);
    return JL_OK;
}

}  // extern "C"
