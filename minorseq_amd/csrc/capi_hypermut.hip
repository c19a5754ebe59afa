// capi_hypermut.hip — jl_read_hypermut_async / _fetch of include/juliet_hip.h: per read of the resident matrix its G->A sites in
// APOBEC's target context and in the control contexts, the mutated ones of each, and the one-sided exact test of the two
// (docs/SPEC.md §26); the test kernel alone over tables of the caller (jl_hypermut_eval), the same expressions on the host
// (jl_hypermut_test) and the host-only rule that turns the p-values into the indices jl_msa_take takes (jl_hypermut_filter).
// The stage call owns its buffers and touches nothing else of the context: no stage result, no plan, no captured graph sees it.
// Every size the kernels (kernels_hypermut.hip) form an address from is checked here.
#include <string.h>

#include "hypermut_test.h"
#include "jl_internal.h"
#include "readstats_shape.h"

#ifdef JL_TUNING
// hook of the -DJL_TUNING build (tools_tuning/hypermut_time.py): the slices of a counter (4 .. 6, 0: the shape's own) and the
// combine form (JL_RS_COMBINE_*, negative: the shape's own) of every later call of this process
static int g_tune_k = 0, g_tune_combine = -1;
extern "C" __attribute__((visibility("default"))) int jl_tuning_hypermut_shape(int k, int combine)
{
    if ((k != 0 && (k < 4 || k > 6)) || combine > JL_RS_COMBINE_ATOMIC) return JL_ERR_ARG;
    g_tune_k = k, g_tune_combine = combine;
    return JL_OK;
}
#endif

extern "C" {

int jl_read_hypermut_async(jl_ctx *ctx, const uint8_t *ref)
{
    static const char *fn = "jl_read_hypermut_async";
    if (!ctx) return JL_ERR_ARG;
    if (!ctx->d_msa) return jl_fail(ctx, JL_ERR_STATE, "%s: no resident matrix", fn);
    if (!ref) return jl_fail(ctx, JL_ERR_ARG, "%s: no reference row", fn);
    const uint64_t n_words = (ctx->n_reads + 31u) / 32u;
    // (a multiple of 16, >= ceil(n_reads / 8): set_shape, jl_msa_adopt — so every word with a read lies within a plane row)
    if (4u * n_words > ctx->plane_stride) return jl_fail(ctx, JL_ERR_ARG, "%s: plane stride %llu holds no %llu reads", fn, (unsigned long long)ctx->plane_stride, (unsigned long long)ctx->n_reads);
    jl_readstats_shape shape = jl_readstats_shape_for(ctx->n_reads, ctx->n_cols);
#ifdef JL_TUNING
    if (g_tune_k) shape.k = (uint32_t)g_tune_k, shape.flush = (1u << shape.k) - 1u;
    if (g_tune_combine >= 0) shape.combine = (uint32_t)g_tune_combine;
#endif
    // the grids: segments x chunks of the counting kernel, 256 reads a workgroup of the test kernel
    if ((uint64_t)shape.n_chunks * shape.n_segs > 0x7FFFFFFFull || (ctx->n_reads + 255u) / 256u > 0x7FFFFFFFull)
        return jl_fail(ctx, JL_ERR_ARG, "%s: %llu reads x %u columns are more workgroups than a launch takes", fn, (unsigned long long)ctx->n_reads, ctx->n_cols);
    JL_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t words = (size_t)JL_HM_COUNTERS * ctx->n_reads;
    const bool atomic = shape.combine == JL_RS_COMBINE_ATOMIC;
    ctx->hm_reads = 0;   // (what was fetchable is gone as soon as a buffer may move)
    uint8_t *h = nullptr;
    hipError_t e = ctx->hm_ref.host(ctx->n_cols, &h);
    if (e == hipSuccess) {
        memcpy(h, ref, ctx->n_cols);
        e = ctx->hm_ref.upload(st, ctx->n_cols);
    }
    if (e == hipSuccess) e = ctx->hm_out.grow_discard(st, words);
    if (e == hipSuccess) e = ctx->hm_p.grow_discard(st, 2u * (size_t)ctx->n_reads);
    if (e == hipSuccess && !atomic) e = ctx->hm_part.grow_discard(st, jl_hypermut_part_words(&shape));
    if (e == hipSuccess && atomic) e = hipMemsetAsync(ctx->hm_out, 0, words * sizeof(uint32_t), st);
    if (e == hipSuccess) {
        jl_hypermut_args A = {};
        A.msa = ctx->d_msa, A.plane_stride = ctx->plane_stride;
        A.n_reads = ctx->n_reads, A.n_cols = ctx->n_cols, A.n_words = (uint32_t)n_words;
        A.ref = (const uint8_t *)ctx->hm_ref.dev;
        A.part = atomic ? nullptr : (uint32_t *)ctx->hm_part;
        A.counts = ctx->hm_out;
        jl_launch_hypermut_counts(&A, &shape, st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        jl_launch_hypermut_test(ctx->hm_out, ctx->n_reads, ctx->hm_p, ctx->hm_p + ctx->n_reads, st);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return jl_fail(ctx, jl_hip_status(e), "%s: %s", fn, hipGetErrorString(e));
    ctx->hm_reads = ctx->n_reads;
    return JL_OK;
}

int jl_read_hypermut_fetch(jl_ctx *ctx, uint32_t *counts, double *p, double *log_p)
{
    if (!ctx) return JL_ERR_ARG;
    if (!ctx->hm_reads) return jl_fail(ctx, JL_ERR_STATE, "jl_read_hypermut_fetch before jl_read_hypermut_async");
    JL_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)ctx->hm_reads;
    if (counts) JL_HIP(ctx, hipMemcpyAsync(counts, ctx->hm_out, JL_HM_COUNTERS * n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (p) JL_HIP(ctx, hipMemcpyAsync(p, ctx->hm_p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (log_p) JL_HIP(ctx, hipMemcpyAsync(log_p, ctx->hm_p + n, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    JL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JL_OK;
}

// the test kernel alone, over tables of the caller (a diagnostic, as jl_control_eval is for the control call)
int jl_hypermut_eval(jl_ctx *ctx, const uint32_t *counts, uint64_t n, double *p, double *log_p)
{
    static const char *fn = "jl_hypermut_eval";
    if (!ctx) return JL_ERR_ARG;
    if (!counts || !p || !log_p) return jl_fail(ctx, JL_ERR_ARG, "%s: a NULL array", fn);
    if (n == 0) return JL_OK;
    if ((n + 255u) / 256u > 0x7FFFFFFFull) return jl_fail(ctx, JL_ERR_ARG, "%s: %llu tables are more workgroups than a launch takes", fn, (unsigned long long)n);
    for (uint64_t i = 0; i < n; ++i)
        if (counts[JL_HM_TARGET_MUT * n + i] > counts[JL_HM_TARGET_SITES * n + i] || counts[JL_HM_CONTROL_MUT * n + i] > counts[JL_HM_CONTROL_SITES * n + i])
            return jl_fail(ctx, JL_ERR_ARG, "%s: table %llu: more mutations than sites", fn, (unsigned long long)i);
    JL_HIP(ctx, hipSetDevice(ctx->device));
    uint32_t *d_in = nullptr;
    double *d_out = nullptr;    // p | log_p
    JL_HIP(ctx, hipMalloc(&d_in, (size_t)n * JL_HM_COUNTERS * sizeof(uint32_t)));
    if (hipMalloc(&d_out, (size_t)n * 2 * sizeof(double)) != hipSuccess) { hipFree(d_in); return jl_fail(ctx, JL_ERR_MEMORY, "%s buffers", fn); }
    hipStream_t st = ctx->stream;
    hipError_t e = hipMemcpyAsync(d_in, counts, (size_t)n * JL_HM_COUNTERS * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        jl_launch_hypermut_test(d_in, n, d_out, d_out + n, st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(p, d_out, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(log_p, d_out + n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    hipFree(d_in);
    hipFree(d_out);
    if (e != hipSuccess) return jl_fail(ctx, JL_ERR_DEVICE, "%s: %s", fn, hipGetErrorString(e));
    return JL_OK;
}

// one read's table: the expressions the kernel evaluates, compiled for the host
int jl_hypermut_test(uint32_t target_mut, uint32_t target_sites, uint32_t control_mut, uint32_t control_sites, double *p, double *log_p)
{
    static const char *fn = "jl_hypermut_test";
    if (!p || !log_p) return jl_fail(nullptr, JL_ERR_ARG, "%s: a NULL argument", fn);
    if (target_mut > target_sites || control_mut > control_sites)
        return jl_fail(nullptr, JL_ERR_ARG, "%s: more mutations than sites (%u of %u, %u of %u)", fn, target_mut, target_sites, control_mut, control_sites);
    *p = jl_hypermut_p(target_mut, target_sites, control_mut, control_sites, log_p);
    return JL_OK;
}

// the reads that are not hypermutated (docs/SPEC.md §26): p < alpha, strict, drops a read
int jl_hypermut_filter(const double *p, uint64_t n_reads, double alpha, uint32_t *idx, uint64_t *n_kept, uint64_t *n_flagged)
{
    static const char *fn = "jl_hypermut_filter";
    if (!p || !idx || !n_kept || !n_flagged) return jl_fail(nullptr, JL_ERR_ARG, "%s: a NULL argument", fn);
    if (n_reads > 0xFFFFFFFFull) return jl_fail(nullptr, JL_ERR_ARG, "%s: %llu reads, an index is 32 bits", fn, (unsigned long long)n_reads);
    if (!(alpha > 0.0 && alpha <= 1.0)) return jl_fail(nullptr, JL_ERR_ARG, "%s: alpha %g outside (0, 1]", fn, alpha);
    uint64_t kept = 0;
    for (uint64_t i = 0; i < n_reads; ++i)
        if (!(p[i] < alpha)) idx[kept++] = (uint32_t)i;
    *n_kept = kept;
    *n_flagged = n_reads - kept;
    return JL_OK;
}

}  // extern "C"
