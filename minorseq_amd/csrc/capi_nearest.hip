// capi_nearest.hip — jl_phase_nearest_async / _fetch of include/juliet_hip.h: which reported haplotype a read is nearest to, within
// a mismatch budget (docs/SPEC.md §22).  As the rescue's (capi_rescue.hip), the call owns its buffers — positions and pattern in,
// ids, distances, haplotype counts and tally out — and touches nothing else of the context: no stage result, no plan, no captured
// graph and no rescue result sees it.  Every size the kernel (kernels_nearest.hip) forms an address from is checked here, and
// the pattern is packed into the form it streams.
#include <string.h>

#include "jl_internal.h"

namespace {
constexpr size_t kTallyWords = 8;                                   // tally [4], 64 bits each
constexpr size_t kHeadWords = kTallyWords + JL_NEAREST_HIST_WORDS;  // ... then hap_reads; nearest, then dist follow
}

extern "C" {

int jl_phase_nearest_async(jl_ctx *ctx, const uint32_t *pos_cols, uint32_t n_pos, const uint8_t *pattern, uint32_t pattern_stride,
                           uint32_t n_hap, uint32_t min_positions, uint32_t max_distance)
{
    static const char *fn = "jl_phase_nearest_async";
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
    if (max_distance > (uint32_t)JL_NEAREST_MAX_DISTANCE)
        return jl_fail(ctx, JL_ERR_ARG, "%s: max_distance %u, 0 to %d", fn, max_distance, (int)JL_NEAREST_MAX_DISTANCE);
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
    JL_HIP(ctx, ctx->nearest_in.host(in_words, &h_in));
    memcpy(h_in, pos_cols, (size_t)n_pos * sizeof(uint32_t));
    uint32_t *pat4 = h_in + n_pos;
    memset(pat4, 0, (size_t)groups * hap_pad * sizeof(uint32_t));
    for (uint32_t h = 0; h < n_hap; ++h)
        for (uint32_t p = 0; p < n_pos; ++p)
            pat4[(size_t)(p / 4u) * hap_pad + h] |= (uint32_t)pattern[(size_t)h * pattern_stride + p] << (8u * (p % 4u));
    const size_t id_words = (size_t)((n + 1u) / 2u), dist_words = (size_t)((n + 3u) / 4u);
    const size_t out_words = kHeadWords + id_words + dist_words;
    ctx->nearest_n = 0;   // (what was fetchable is gone as soon as a buffer may move)
    hipError_t e = ctx->nearest_out.grow_discard(st, out_words);
    if (e == hipSuccess) e = ctx->nearest_in.upload(st, in_words);
    if (e == hipSuccess) e = hipMemsetAsync(ctx->nearest_out, 0, kHeadWords * sizeof(uint32_t), st);
    if (e == hipSuccess) {
        jl_nearest_args A = {};
        A.msa = ctx->d_msa, A.plane_stride = ctx->plane_stride;
        A.n_reads = n, A.n_runs = (uint32_t)((n + 63u) / 64u);   // (8 n_runs <= plane_stride: a multiple of 16 and >= ceil(n / 8))
        A.n_pos = n_pos, A.n_hap = n_hap, A.min_positions = min_positions, A.hap_pad = hap_pad, A.max_distance = max_distance;
        A.pos_cols = ctx->nearest_in.dev, A.pat4 = ctx->nearest_in.dev + n_pos;
        A.tally = ctx->nearest_out.as<unsigned long long>();
        A.hap_reads = ctx->nearest_out + kTallyWords;
        A.nearest = (uint16_t *)(ctx->nearest_out + kHeadWords);
        A.dist = (uint8_t *)(ctx->nearest_out + kHeadWords + id_words);
        jl_launch_phase_nearest(&A, st);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return jl_fail(ctx, jl_hip_status(e), "%s: %s", fn, hipGetErrorString(e));
    ctx->nearest_n = n, ctx->nearest_h = n_hap, ctx->nearest_d = max_distance;
    return JL_OK;
}

int jl_phase_nearest_fetch(jl_ctx *ctx, uint16_t *nearest, uint8_t *dist, uint32_t *hap_reads, uint64_t *tally)
{
    if (!ctx) return JL_ERR_ARG;
    if (!ctx->nearest_n) return jl_fail(ctx, JL_ERR_STATE, "jl_phase_nearest_fetch before jl_phase_nearest_async");
    JL_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t *out = ctx->nearest_out;
    const size_t n = (size_t)ctx->nearest_n, id_words = (n + 1u) / 2u;
    if (tally) JL_HIP(ctx, hipMemcpyAsync(tally, out, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (hap_reads)
        JL_HIP(ctx, hipMemcpyAsync(hap_reads, out + kTallyWords, (size_t)ctx->nearest_h * (ctx->nearest_d + 1u) * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                   ctx->stream));
    if (nearest) JL_HIP(ctx, hipMemcpyAsync(nearest, out + kHeadWords, n * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx->stream));
    if (dist) JL_HIP(ctx, hipMemcpyAsync(dist, out + kHeadWords + id_words, n * sizeof(uint8_t), hipMemcpyDeviceToHost, ctx->stream));
    JL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JL_OK;
}

}  // extern "C"
