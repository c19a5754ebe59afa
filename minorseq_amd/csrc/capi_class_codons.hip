// capi_class_codons.hip — jl_class_codons_async / _fetch of include/juliet_hip.h: the codon histograms of the resident matrix by
// class of reads at chosen codon starts (docs/SPEC.md §24).  The call owns its buffers — labels, columns, mask rows, table — and
// touches nothing else of the context: no stage result, no plan, no captured graph and not the class pileup's buffers see it.
// Every size the kernels (class_masks_kernel of kernels_class.hip, kernels_class_codons.hip) form an address from is checked here.
#include <string.h>

#include "jl_internal.h"

#include "hap_stage.h"

extern "C" {

int jl_class_codons_async(jl_ctx *ctx, const uint16_t *label, uint32_t n_classes, const uint32_t *col, uint32_t n_pos)
{
    static const char *fn = "jl_class_codons_async";
    if (!ctx) return JL_ERR_ARG;
    if (!ctx->d_msa) return jl_fail(ctx, JL_ERR_STATE, "%s: no resident matrix", fn);
    if (!label) return jl_fail(ctx, JL_ERR_ARG, "%s: no labels", fn);
    if (!col) return jl_fail(ctx, JL_ERR_ARG, "%s: no positions array", fn);
    if (n_classes == 0) return jl_fail(ctx, JL_ERR_ARG, "%s: no classes", fn);
    if (n_classes > (uint32_t)JL_CLASS_MAX) return jl_fail(ctx, JL_ERR_ARG, "%s: %u classes, at most %d", fn, n_classes, (int)JL_CLASS_MAX);
    if (n_pos == 0) return jl_fail(ctx, JL_ERR_ARG, "%s: no positions", fn);
    if ((uint64_t)n_classes * n_pos > (uint64_t)JL_CLASS_CODONS_CELLS)
        return jl_fail(ctx, JL_ERR_ARG, "%s: %u classes x %u positions, at most %u cells", fn, n_classes, n_pos, (unsigned)JL_CLASS_CODONS_CELLS);
    if (int rc = jl_check_codon_columns(ctx, fn, col, n_pos)) return rc;
    JL_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t n = ctx->n_reads;
    // labels and columns into pinned staging (an upload of the last call may still read it: wait for that)
    uint16_t *h_label = nullptr;
    uint32_t *h_col = nullptr;
    JL_HIP(ctx, ctx->cc_label.host((size_t)n, &h_label));
    JL_HIP(ctx, ctx->cc_col.host((size_t)n_pos, &h_col));
    memcpy(h_label, label, (size_t)n * sizeof(uint16_t));
    memcpy(h_col, col, (size_t)n_pos * sizeof(uint32_t));
    const uint64_t mask_stride = jl_plane_stride(n);
    const size_t hist_words = (size_t)n_classes * n_pos * 64u;
    ctx->cc_k = 0;   // (what was fetchable is gone as soon as a buffer may move)
    hipError_t e = ctx->cc_mask.grow_discard(st, (size_t)(n_classes * mask_stride));
    if (e == hipSuccess) e = ctx->cc_out.grow_discard(st, hist_words + n_classes);
    if (e == hipSuccess) e = ctx->cc_label.upload(st, (size_t)n);
    if (e == hipSuccess) e = ctx->cc_col.upload(st, (size_t)n_pos);
    if (e == hipSuccess) e = hipMemsetAsync(ctx->cc_out, 0, (hist_words + n_classes) * sizeof(uint32_t), st);
    if (e == hipSuccess && n) {
        jl_class_args M = {};   // the mask rows: the class pileup's, in this call's own buffer
        M.n_reads = n, M.n_classes = n_classes;
        M.label = ctx->cc_label.dev;
        M.mask = ctx->cc_mask, M.mask_stride = mask_stride;
        M.class_reads = ctx->cc_out + hist_words;
        jl_launch_class_masks(&M, st);
        jl_class_codons_args A = {};
        A.msa = ctx->d_msa, A.plane_stride = ctx->plane_stride;
        A.n_reads = n, A.n_pos = n_pos, A.n_classes = n_classes;
        A.col = ctx->cc_col.dev, A.label = ctx->cc_label.dev;
        A.mask = ctx->cc_mask, A.mask_stride = mask_stride;
        A.hist = ctx->cc_out;
        jl_launch_class_codons(&A, st);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return jl_fail(ctx, jl_hip_status(e), "%s: %s", fn, hipGetErrorString(e));
    ctx->cc_k = n_classes, ctx->cc_pos = n_pos;
    return JL_OK;
}

int jl_class_codons_fetch(jl_ctx *ctx, uint32_t *hist, uint32_t *class_reads)
{
    if (!ctx) return JL_ERR_ARG;
    if (!ctx->cc_k) return jl_fail(ctx, JL_ERR_STATE, "jl_class_codons_fetch before jl_class_codons_async");
    JL_HIP(ctx, hipSetDevice(ctx->device));
    const size_t hist_words = (size_t)ctx->cc_k * ctx->cc_pos * 64u;
    if (hist) JL_HIP(ctx, hipMemcpyAsync(hist, ctx->cc_out, hist_words * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (class_reads)
        JL_HIP(ctx, hipMemcpyAsync(class_reads, ctx->cc_out + hist_words, (size_t)ctx->cc_k * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    JL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JL_OK;
}

}  // extern "C"
