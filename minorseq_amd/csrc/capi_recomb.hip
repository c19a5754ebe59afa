// capi_recomb.hip — jl_phase_recombinants_async / _fetch and jl_haplotype_recombinants of include/juliet_hip.h: which reads, and
// which reported haplotypes, are recombinants of two others (docs/SPEC.md §23).  As the nearest call's (capi_nearest.hip), the
// device call owns its buffers — positions and pattern in, parents, lengths, parent counts and tally out — and touches nothing
// else of the context: no stage result, no plan, no captured graph, no rescue and no nearest result sees it.  Every size the
// kernel (kernels_recomb.hip) forms an address from is checked here, and the pattern is packed into the form it streams, once in
// the order of the positions and once reversed.
#include "jl_internal.h"

#include "hap_stage.h"

namespace {
constexpr size_t kTallyWords = 12;                                  // tally [5], 64 bits each, and a pad to 16 bytes
constexpr size_t kHeadWords = kTallyWords + JL_RECOMB_HIST_WORDS;   // ... then parent_reads; left, right, prefix, suffix follow
}

extern "C" {

int jl_phase_recombinants_async(jl_ctx *ctx, const uint32_t *pos_cols, uint32_t n_pos, const uint8_t *pattern, uint32_t pattern_stride,
                                uint32_t n_hap, uint32_t min_positions)
{
    static const char *fn = "jl_phase_recombinants_async";
    if (!ctx) return JL_ERR_ARG;
    if (int rc = jl_check_hap_table(ctx, fn, pos_cols, n_pos, pattern, pattern_stride, n_hap, min_positions)) return rc;
    if (int rc = jl_check_hap_contents(ctx, fn, pos_cols, n_pos, pattern, pattern_stride, n_hap)) return rc;
    JL_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t n = ctx->n_reads;
    const jl_pat4_shape shape = jl_pat4_shape_for(n_pos, n_hap);
    const size_t dir_words = shape.dir_words, in_words = 2u * dir_words;
    // positions and packed pattern, ascending and then descending, into pinned staging (an upload of the last call may still read
    // it: wait for that)
    uint32_t *h_in = nullptr;
    JL_HIP(ctx, ctx->recomb_in.host(in_words, &h_in));
    for (uint32_t dir = 0; dir < 2u; ++dir) jl_stage_hap_direction(h_in + dir * dir_words, shape, pos_cols, n_pos, pattern, pattern_stride, n_hap, dir != 0u);
    const size_t id_words = (size_t)((n + 1u) / 2u);
    const size_t out_words = kHeadWords + 4u * id_words;
    ctx->recomb_n = 0;   // (what was fetchable is gone as soon as a buffer may move)
    hipError_t e = ctx->recomb_out.grow_discard(st, out_words);
    if (e == hipSuccess) e = ctx->recomb_in.upload(st, in_words);
    if (e == hipSuccess) e = hipMemsetAsync(ctx->recomb_out, 0, kHeadWords * sizeof(uint32_t), st);
    if (e == hipSuccess) {
        jl_recomb_args A = {};
        A.msa = ctx->d_msa, A.plane_stride = ctx->plane_stride;
        A.n_reads = n, A.n_runs = (uint32_t)((n + 63u) / 64u);   // (8 n_runs <= plane_stride: a multiple of 16 and >= ceil(n / 8))
        A.n_pos = n_pos, A.n_hap = n_hap, A.min_positions = min_positions, A.hap_pad = shape.hap_pad;
        for (uint32_t dir = 0; dir < 2u; ++dir) {
            A.pos_cols[dir] = ctx->recomb_in.dev + dir * dir_words;
            A.pat4[dir] = A.pos_cols[dir] + n_pos;
        }
        A.tally = ctx->recomb_out.as<unsigned long long>();
        A.parent_reads = ctx->recomb_out + kTallyWords;
        A.left = (uint16_t *)(ctx->recomb_out + kHeadWords);
        A.right = (uint16_t *)(ctx->recomb_out + kHeadWords + id_words);
        A.prefix = (uint16_t *)(ctx->recomb_out + kHeadWords + 2u * id_words);
        A.suffix = (uint16_t *)(ctx->recomb_out + kHeadWords + 3u * id_words);
        jl_launch_phase_recombinants(&A, st);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return jl_fail(ctx, jl_hip_status(e), "%s: %s", fn, hipGetErrorString(e));
    ctx->recomb_n = n, ctx->recomb_h = n_hap;
    return JL_OK;
}

int jl_phase_recombinants_fetch(jl_ctx *ctx, uint16_t *left, uint16_t *right, uint16_t *prefix, uint16_t *suffix, uint32_t *parent_reads,
                                uint64_t *tally)
{
    if (!ctx) return JL_ERR_ARG;
    if (!ctx->recomb_n) return jl_fail(ctx, JL_ERR_STATE, "jl_phase_recombinants_fetch before jl_phase_recombinants_async");
    JL_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t *out = ctx->recomb_out;
    const size_t n = (size_t)ctx->recomb_n, id_words = (n + 1u) / 2u;
    if (tally) JL_HIP(ctx, hipMemcpyAsync(tally, out, 5 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (parent_reads)
        JL_HIP(ctx, hipMemcpyAsync(parent_reads, out + kTallyWords, (size_t)ctx->recomb_h * 2u * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    uint16_t *const per_read[4] = {left, right, prefix, suffix};
    for (size_t k = 0; k < 4u; ++k)
        if (per_read[k])
            JL_HIP(ctx, hipMemcpyAsync(per_read[k], out + kHeadWords + k * id_words, n * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx->stream));
    JL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JL_OK;
}

// is a reported haplotype a recombinant of two more frequent ones (docs/SPEC.md §23, the haplotype level)
int jl_haplotype_recombinants(const uint8_t *pattern, uint32_t pattern_stride, uint32_t n_hap, uint32_t n_pos, const uint32_t *hap_count,
                              double min_parent_ratio, jl_hap_recombinant *out)
{
    static const char *fn = "jl_haplotype_recombinants";
    if (!pattern || !hap_count || !out) return jl_fail(nullptr, JL_ERR_ARG, "%s: a NULL array", fn);
    if (!(min_parent_ratio >= 1.0)) return jl_fail(nullptr, JL_ERR_ARG, "%s: min_parent_ratio %g, 1 at least", fn, min_parent_ratio);
    if (int rc = jl_check_hap_shape(nullptr, fn, n_pos, pattern_stride, n_hap)) return rc;
    for (uint32_t h = 0; h < n_hap; ++h) {
        const uint8_t *row = pattern + (size_t)h * pattern_stride;
        const double need = min_parent_ratio * (double)hap_count[h];
        jl_hap_recombinant r = {0u, 0u, 0u, 0u, 0u};
        bool any = false;
        for (uint32_t c = 0; c < n_hap; ++c) {
            if (c == h || !((double)hap_count[c] >= need)) continue;
            const uint8_t *other = pattern + (size_t)c * pattern_stride;
            uint32_t pre = 0, suf = 0;
            while (pre < n_pos && row[pre] == other[pre]) ++pre;
            while (suf < n_pos && row[n_pos - 1u - suf] == other[n_pos - 1u - suf]) ++suf;
            if (!any || pre > r.prefix) r.prefix = pre, r.left = c;     // (strictly greater: the lowest index keeps a tie)
            if (!any || suf > r.suffix) r.suffix = suf, r.right = c;
            any = true;
        }
        r.flagged = any && (uint64_t)r.prefix + r.suffix >= n_pos ? 1u : 0u;
        out[h] = r;
    }
    return JL_OK;
}

}  // extern "C"
