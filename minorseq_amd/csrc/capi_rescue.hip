// capi_rescue.hip — jl_phase_rescue_async / _fetch of include/juliet_hip.h: which reported haplotype a read agrees with where it
// can be read (docs/SPEC.md §14).  The call owns its buffers — positions and pattern in, ids, haplotype counts and tally out — and
// touches nothing else of the context: no stage result, no plan, no captured graph sees it.  Every size the kernel
// (kernels_rescue.hip) forms an address from is checked here, and the pattern is packed into the form it streams.
#include "jl_internal.h"

#include "hap_stage.h"

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
    if (int rc = jl_check_hap_table(ctx, fn, pos_cols, n_pos, pattern, pattern_stride, n_hap, min_positions)) return rc;
    if (int rc = jl_check_hap_contents(ctx, fn, pos_cols, n_pos, pattern, pattern_stride, n_hap)) return rc;
    JL_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t n = ctx->n_reads;
    const jl_pat4_shape shape = jl_pat4_shape_for(n_pos, n_hap);
    const size_t in_words = shape.dir_words;
    // positions and packed pattern into pinned staging (an upload of the last call may still read it: wait for that)
    uint32_t *h_in = nullptr;
    JL_HIP(ctx, ctx->rescue_in.host(in_words, &h_in));
    jl_stage_hap_direction(h_in, shape, pos_cols, n_pos, pattern, pattern_stride, n_hap, false);
    const size_t out_words = kHeadWords + (size_t)((n + 1u) / 2u);
    ctx->rescue_n = 0;   // (what was fetchable is gone as soon as a buffer may move)
    hipError_t e = ctx->rescue_out.grow_discard(st, out_words);
    if (e == hipSuccess) e = ctx->rescue_in.upload(st, in_words);
    if (e == hipSuccess) e = hipMemsetAsync(ctx->rescue_out, 0, kHeadWords * sizeof(uint32_t), st);
    if (e == hipSuccess) {
        jl_rescue_args A = {};
        A.msa = ctx->d_msa, A.plane_stride = ctx->plane_stride;
        A.n_reads = n, A.n_runs = (uint32_t)((n + 63u) / 64u);   // (8 n_runs <= plane_stride: a multiple of 16 and >= ceil(n / 8))
        A.n_pos = n_pos, A.n_hap = n_hap, A.min_positions = min_positions, A.hap_pad = shape.hap_pad;
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
