// capi_rescue.hip — jl_phase_rescue_async / _fetch of include/juliet_hip.h: which reported haplotype a read agrees with where it
// can be read (docs/SPEC.md §14).  The call owns its buffers — positions and pattern in, ids, haplotype counts and tally out — and
// touches nothing else of the context: no stage result, no plan, no captured graph sees it.  Every size the kernel
// (kernels_rescue.hip) forms an address from is checked here, and the pattern is packed into the form it streams.
#include <string.h>

#include "jl_internal.h"

namespace {
constexpr size_t kTallyWords = 8;                                  // tally [4], 64 bits each
constexpr size_t kHeadWords = kTallyWords + JL_RESCUE_HAP_PAD;     // ... then hap_reads; the ids follow
}

extern "C" {

int jl_phase_rescue_async(jl_ctx *ctx, const uint32_t *pos_cols, uint32_t n_pos, const uint8_t *pattern, uint32_t pattern_stride,
                          uint32_t n_hap, uint32_t min_positions)
{
    static const char *fn = "jl_phase_rescue_async";
    if (!ctx) return JL_ERR_ARG;
    if (!ctx->d_msa) return jl_fail(ctx, JL_ERR_STATE, "%s: no resident matrix", fn);
    if (!pos_cols) return jl_fail(ctx, JL_ERR_ARG, "%s: no positions array", fn);
    if (!pattern) return jl_fail(ctx, JL_ERR_ARG, "%s: no pattern array", fn);
    if (n_pos == 0 || n_pos > JL_RESCUE_POS_MAX) return jl_fail(ctx, JL_ERR_ARG, "%s: %u positions, 1 to %u", fn, n_pos, JL_RESCUE_POS_MAX);
    if (n_hap == 0 || n_hap > (uint32_t)JL_MAX_HAPLOTYPES)
        return jl_fail(ctx, JL_ERR_ARG, "%s: %u haplotypes, 1 to %d", fn, n_hap, (int)JL_MAX_HAPLOTYPES);
    if (pattern_stride < n_pos) return jl_fail(ctx, JL_ERR_ARG, "%s: pattern_stride %u below the %u positions of a row", fn, pattern_stride, n_pos);
    if (min_positions == 0 || min_positions > n_pos)
        return jl_fail(ctx, JL_ERR_ARG, "%s: min_positions %u, 1 to the %u positions", fn, min_positions, n_pos);
    for (uint32_t p = 0; p < n_pos; ++p) {
        if ((uint64_t)pos_cols[p] + 2u >= ctx->n_cols)
            return jl_fail(ctx, JL_ERR_ARG, "%s: position %u: the codon at column %u ends beyond the window's %u columns", fn, p, pos_cols[p], ctx->n_cols);
        if (p && pos_cols[p] <= pos_cols[p - 1]) return jl_fail(ctx, JL_ERR_ARG, "%s: position %u: columns not strictly ascending", fn, p);
    }
    for (uint32_t h = 0; h < n_hap; ++h)
        for (uint32_t p = 0; p < n_pos; ++p)
            if (pattern[(size_t)h * pattern_stride + p] > 63u)
                return jl_fail(ctx, JL_ERR_ARG, "%s: pattern byte %u of haplotype %u at position %u is no codon (0..63)", fn,
                               (unsigned)pattern[(size_t)h * pattern_stride + p], h, p);
    JL_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t n = ctx->n_reads;
    const uint32_t hap_pad = (n_hap + 63u) / 64u * 64u, groups = (n_pos + 3u) / 4u;
    const size_t in_words = (size_t)n_pos + (size_t)groups * hap_pad;
    // positions and packed pattern into pinned staging (an upload of the last call may still read it: wait for that)
    uint32_t *h_in = nullptr;
    JL_HIP(ctx, ctx->rescue_in.host(in_words, &h_in));
    memcpy(h_in, pos_cols, (size_t)n_pos * sizeof(uint32_t));
    uint32_t *pat4 = h_in + n_pos;
    memset(pat4, 0, (size_t)groups * hap_pad * sizeof(uint32_t));
    for (uint32_t h = 0; h < n_hap; ++h)
        for (uint32_t p = 0; p < n_pos; ++p)
            pat4[(size_t)(p / 4u) * hap_pad + h] |= (uint32_t)pattern[(size_t)h * pattern_stride + p] << (8u * (p % 4u));
    const size_t out_words = kHeadWords + (size_t)((n + 1u) / 2u);
    ctx->rescue_n = 0;   // (what was fetchable is gone as soon as a buffer may move)
    hipError_t e = ctx->rescue_out.grow_discard(st, out_words);
    if (e == hipSuccess) e = ctx->rescue_in.upload(st, in_words);
    if (e == hipSuccess) e = hipMemsetAsync(ctx->rescue_out, 0, kHeadWords * sizeof(uint32_t), st);
    if (e == hipSuccess) {
        jl_rescue_args A = {};
        A.msa = ctx->d_msa, A.plane_stride = ctx->plane_stride;
        A.n_reads = n, A.n_runs = (uint32_t)((n + 63u) / 64u);   // (8 n_runs <= plane_stride: a multiple of 16 and >= ceil(n / 8))
        A.n_pos = n_pos, A.n_hap = n_hap, A.min_positions = min_positions, A.hap_pad = hap_pad;
        A.pos_cols = ctx->rescue_in.dev, A.pat4 = ctx->rescue_in.dev + n_pos;
        A.tally = ctx->rescue_out.as<unsigned long long>();
        A.hap_reads = ctx->rescue_out + kTallyWords;
        A.rescue = (uint16_t *)(ctx->rescue_out + kHeadWords);
        jl_launch_phase_rescue(&A, st);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return jl_fail(ctx, jl_hip_status(e), "%s: %s", fn, hipGetErrorString(e));
    ctx->rescue_n = n, ctx->rescue_h = n_hap;
    return JL_OK;
}

int jl_phase_rescue_fetch(jl_ctx *ctx, uint16_t *rescue, uint32_t *hap_reads, uint64_t *tally)
{
    if (!ctx) return JL_ERR_ARG;
    if (!ctx->rescue_n) return jl_fail(ctx, JL_ERR_STATE, "jl_phase_rescue_fetch before jl_phase_rescue_async");
    JL_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t *out = ctx->rescue_out;
    if (tally) JL_HIP(ctx, hipMemcpyAsync(tally, out, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (hap_reads) JL_HIP(ctx, hipMemcpyAsync(hap_reads, out + kTallyWords, (size_t)ctx->rescue_h * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (rescue) JL_HIP(ctx, hipMemcpyAsync(rescue, out + kHeadWords, (size_t)ctx->rescue_n * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx->stream));
    JL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JL_OK;
}

}  // extern "C"
