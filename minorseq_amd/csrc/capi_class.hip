// capi_class.hip — jl_class_pileup_async / _fetch of include/juliet_hip.h: the column pileup of the resident matrix by class of
// reads (docs/SPEC.md §13), and the host-only consensus rule over one count table (jl_consensus_of_counts).  The call owns its
// buffers — labels, mask rows, counts — and touches nothing else of the context: no stage result, no plan, no captured graph
// sees it.  Every size the kernels (kernels_class.hip) form an address from is checked here.
#include <string.h>

#include "jl_internal.h"

extern "C" {

int jl_class_pileup_async(jl_ctx *ctx, const uint16_t *label, uint32_t n_classes)
{
    static const char *fn = "jl_class_pileup_async";
    if (!ctx) return JL_ERR_ARG;
    if (!ctx->d_msa) return jl_fail(ctx, JL_ERR_STATE, "%s: no resident matrix", fn);
    if (!label) return jl_fail(ctx, JL_ERR_ARG, "%s: no labels", fn);
    if (n_classes == 0) return jl_fail(ctx, JL_ERR_ARG, "%s: no classes", fn);
    if (n_classes > (uint32_t)JL_CLASS_MAX) return jl_fail(ctx, JL_ERR_ARG, "%s: %u classes, at most %d", fn, n_classes, (int)JL_CLASS_MAX);
    JL_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t n = ctx->n_reads;
    // the labels into pinned staging (an upload of the last call may still read it: wait for that)
    uint16_t *h_label = nullptr;
    JL_HIP(ctx, ctx->class_label.host((size_t)n, &h_label));
    memcpy(h_label, label, (size_t)n * sizeof(uint16_t));
    const uint64_t mask_stride = jl_plane_stride(n);
    const size_t count_words = (size_t)n_classes * ctx->n_cols * 6u;
    ctx->class_k = 0;   // (what was fetchable is gone as soon as a buffer may move)
    hipError_t e = ctx->class_mask.grow_discard(st, (size_t)(n_classes * mask_stride));
    if (e == hipSuccess) e = ctx->class_out.grow_discard(st, count_words + n_classes);
    if (e == hipSuccess) e = ctx->class_label.upload(st, (size_t)n);
    if (e == hipSuccess) e = hipMemsetAsync(ctx->class_out, 0, (count_words + n_classes) * sizeof(uint32_t), st);
    if (e == hipSuccess) {
        jl_class_args A = {};
        A.msa = ctx->d_msa, A.plane_stride = ctx->plane_stride;
        A.n_reads = n, A.n_cols = ctx->n_cols, A.n_classes = n_classes;
        A.label = ctx->class_label.dev;
        A.mask = ctx->class_mask, A.mask_stride = mask_stride;
        A.counts = ctx->class_out, A.class_reads = ctx->class_out + count_words;
        jl_launch_class_pileup(&A, st);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return jl_fail(ctx, jl_hip_status(e), "%s: %s", fn, hipGetErrorString(e));
    ctx->class_k = n_classes, ctx->class_cols = ctx->n_cols;
    return JL_OK;
}

int jl_class_pileup_fetch(jl_ctx *ctx, uint32_t *counts, uint32_t *class_reads)
{
    if (!ctx) return JL_ERR_ARG;
    if (!ctx->class_k) return jl_fail(ctx, JL_ERR_STATE, "jl_class_pileup_fetch before jl_class_pileup_async");
    JL_HIP(ctx, hipSetDevice(ctx->device));
    const size_t count_words = (size_t)ctx->class_k * ctx->class_cols * 6u;
    if (counts) JL_HIP(ctx, hipMemcpyAsync(counts, ctx->class_out, count_words * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (class_reads)
        JL_HIP(ctx, hipMemcpyAsync(class_reads, ctx->class_out + count_words, (size_t)ctx->class_k * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    JL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JL_OK;
}

// the rule of consensus_kernel (kernels_util.hip) over a table on the host: N does not vote
int jl_consensus_of_counts(const uint32_t *col_counts, uint32_t n_cols, uint8_t *out)
{
    if (!col_counts || !out) return JL_ERR_ARG;
    for (uint32_t c = 0; c < n_cols; ++c) {
        const uint32_t *k = col_counts + (size_t)c * 6u;
        uint32_t best = 0, bv = k[0];
        for (uint32_t s = 1; s < 5; ++s)
            if (k[s] > bv) { bv = k[s]; best = s; }
        out[c] = bv == 0 ? (uint8_t)5 : (uint8_t)best;
    }
    return JL_OK;
}

}  // extern "C"
