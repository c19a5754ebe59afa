// capi_nearest.hip — jl_phase_nearest_async / _fetch of include/juliet_hip.h: which reported haplotype a read is nearest to, within
// a mismatch budget (docs/SPEC.md §22).  As the rescue's (capi_rescue.hip), the call owns its buffers — positions and pattern in,
// ids, distances, haplotype counts and tally out — and touches nothing else of the context: no stage result, no plan, no captured
// graph and no rescue result sees it.  Every size the kernel (kernels_nearest.hip) forms an address from is checked here, and
// the pattern is packed into the form it streams.
#include "jl_internal.h"

#include "hap_stage.h"

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
    if (int rc = jl_check_hap_table(ctx, fn, pos_cols, n_pos, pattern, pattern_stride, n_hap, min_positions)) return rc;
    if (max_distance > (uint32_t)JL_NEAREST_MAX_DISTANCE)
        return jl_fail(ctx, JL_ERR_ARG, "%s: max_distance %u, 0 to %d", fn, max_distance, (int)JL_NEAREST_MAX_DISTANCE);
    if (int rc = jl_check_hap_contents(ctx, fn, pos_cols, n_pos, pattern, pattern_stride, n_hap)) return rc;
    JL_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t n = ctx->n_reads;
    const jl_pat4_shape shape = jl_pat4_shape_for(n_pos, n_hap);
    const size_t in_words = shape.dir_words;
    // positions and packed pattern into pinned staging (an upload of the last call may still read it: wait for that)
    uint32_t *h_in = nullptr;
    JL_HIP(ctx, ctx->nearest_in.host(in_words, &h_in));
    jl_stage_hap_direction(h_in, shape, pos_cols, n_pos, pattern, pattern_stride, n_hap, false);
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
        A.n_pos = n_pos, A.n_hap = n_hap, A.min_positions = min_positions, A.hap_pad = shape.hap_pad, A.max_distance = max_distance;
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
