// capi_link.hip — jl_variant_linkage_async / _fetch of include/juliet_hip.h: for every pair of called variants, the reads that can
// be read at both positions and what they carry there (docs/SPEC.md §15), and the host-only statistics of one pair's 2 x 2 table
// (jl_linkage_stats).  The call owns its buffers — positions and variants in, bit rows, three count tables out — and touches nothing
// else of the context: no stage result, no plan, no captured graph sees it.  Every size the kernels (kernels_link.hip) form an
// address from is checked here.
#include <math.h>
#include <string.h>

#include "jl_fisher_general.h"
#include "jl_internal.h"

#include "hap_stage.h"

namespace {

// X ~ Hypergeometric(n, K marked, r drawn), max(0, r + K - n) < min(r, K): *ge = P(X >= x), *le = P(X <= x), each as the upper
// tail of a 2 x 2 table under the general-margin routine of jl_fisher_general.h (the lower tail of X is the upper tail of K - X,
// the marked among the n - r not drawn)
void hypergeometric_tails(uint32_t x, uint32_t K, uint32_t r, uint32_t n, double *ge, double *le)
{
    double lp;
    *ge = jl_fisher_greater_general(x, r, K - x, n - r, &lp);
    *le = jl_fisher_greater_general(K - x, n - r, x, r, &lp);
}

}  // namespace

extern "C" {

int jl_variant_linkage_async(jl_ctx *ctx, const uint32_t *pos_cols, uint32_t n_pos, const uint32_t *var_pos, const uint8_t *var_codon,
                             uint32_t n_var)
{
    static const char *fn = "jl_variant_linkage_async";
    if (!ctx) return JL_ERR_ARG;
    if (!ctx->d_msa) return jl_fail(ctx, JL_ERR_STATE, "%s: no resident matrix", fn);
    if (!pos_cols) return jl_fail(ctx, JL_ERR_ARG, "%s: no positions array", fn);
    if (!var_pos) return jl_fail(ctx, JL_ERR_ARG, "%s: no variant positions array", fn);
    if (!var_codon) return jl_fail(ctx, JL_ERR_ARG, "%s: no variant codons array", fn);
    if (n_pos == 0 || n_pos > (uint32_t)JL_LINK_MAX) return jl_fail(ctx, JL_ERR_ARG, "%s: %u positions, 1 to %d", fn, n_pos, (int)JL_LINK_MAX);
    if (n_var == 0 || n_var > (uint32_t)JL_LINK_MAX) return jl_fail(ctx, JL_ERR_ARG, "%s: %u variants, 1 to %d", fn, n_var, (int)JL_LINK_MAX);
    if (int rc = jl_check_codon_columns(ctx, fn, pos_cols, n_pos)) return rc;
    for (uint32_t v = 0; v < n_var; ++v) {
        if (var_pos[v] >= n_pos) return jl_fail(ctx, JL_ERR_ARG, "%s: variant %u: position index %u beyond the %u positions", fn, v, var_pos[v], n_pos);
        if (v && var_pos[v] < var_pos[v - 1]) return jl_fail(ctx, JL_ERR_ARG, "%s: variant %u: position indices decreasing", fn, v);
        if (var_codon[v] > 63u) return jl_fail(ctx, JL_ERR_ARG, "%s: codon byte %u of variant %u is no codon (0..63)", fn, (unsigned)var_codon[v], v);
    }
    const uint64_t n = ctx->n_reads;   // (1 to 2^31 - 1, set_shape: every count fits its 32 bits)
    JL_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // positions, the variants of each position and the codons into pinned staging (an upload of the last call may still read it)
    const size_t in_words = (size_t)n_pos + (n_pos + 1u) + n_var;
    uint32_t *h_in = nullptr;
    JL_HIP(ctx, ctx->link_in.host(in_words, &h_in));
    memcpy(h_in, pos_cols, (size_t)n_pos * sizeof(uint32_t));
    uint32_t *first = h_in + n_pos, *codon = first + n_pos + 1u;
    for (uint32_t p = 0, v = 0; p <= n_pos; ++p) {   // (var_pos is non-decreasing)
        while (v < n_var && var_pos[v] < p) ++v;
        first[p] = v;
    }
    for (uint32_t v = 0; v < n_var; ++v) codon[v] = var_codon[v];

    jl_link_args A = {};
    A.msa = ctx->d_msa, A.plane_stride = ctx->plane_stride, A.n_reads = n;
    A.n_pos = n_pos, A.n_var = n_var;
    A.n_words = (uint32_t)((n + 31u) / 32u), A.row_words = (uint32_t)(jl_plane_stride(n) / 4u);
    // the product's workgroups: the blocks of the upper triangle, and runs of a row until there are about four per compute unit
    const uint32_t blocks = (n_pos + n_var + JL_LINK_BLOCK_TILE - 1u) / JL_LINK_BLOCK_TILE, upper = blocks * (blocks + 1u) / 2u;
    const uint32_t max_splits = std::max(1u, A.n_words / JL_LINK_SPLIT_WORDS);
    const uint32_t want = std::min(max_splits, std::max(1u, (1024u + upper - 1u) / upper));
    A.split_words = ((A.n_words + want - 1u) / want + 63u) / 64u * 64u;
    A.n_splits = (A.n_words + A.split_words - 1u) / A.split_words;
    const size_t pp = (size_t)n_pos * n_pos, vp = (size_t)n_var * n_pos, vv = (size_t)n_var * n_var;
    ctx->link_p = 0;   // (what was fetchable is gone as soon as a buffer may move)
    hipError_t e = ctx->link_rows.grow_discard(st, (size_t)(n_pos + n_var) * A.row_words);
    if (e == hipSuccess) e = ctx->link_out.grow_discard(st, pp + vp + vv);
    if (e == hipSuccess) e = ctx->link_in.upload(st, in_words);
    if (e == hipSuccess) e = hipMemsetAsync(ctx->link_out, 0, (pp + vp + vv) * sizeof(uint32_t), st);
    if (e == hipSuccess) {
        A.pos_cols = ctx->link_in.dev, A.var_first = ctx->link_in.dev + n_pos, A.var_codon = ctx->link_in.dev + 2u * n_pos + 1u;
        A.rows = ctx->link_rows;
        A.both = ctx->link_out, A.carry = ctx->link_out + pp, A.joint = ctx->link_out + pp + vp;
        jl_launch_variant_linkage(&A, st);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return jl_fail(ctx, jl_hip_status(e), "%s: %s", fn, hipGetErrorString(e));
    ctx->link_p = n_pos, ctx->link_v = n_var;
    return JL_OK;
}

int jl_variant_linkage_fetch(jl_ctx *ctx, uint32_t *both, uint32_t *carry, uint32_t *joint)
{
    if (!ctx) return JL_ERR_ARG;
    if (!ctx->link_p) return jl_fail(ctx, JL_ERR_STATE, "jl_variant_linkage_fetch before jl_variant_linkage_async");
    JL_HIP(ctx, hipSetDevice(ctx->device));
    const size_t pp = (size_t)ctx->link_p * ctx->link_p, vp = (size_t)ctx->link_v * ctx->link_p, vv = (size_t)ctx->link_v * ctx->link_v;
    const uint32_t *out = ctx->link_out;
    if (both) JL_HIP(ctx, hipMemcpyAsync(both, out, pp * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (carry) JL_HIP(ctx, hipMemcpyAsync(carry, out + pp, vp * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (joint) JL_HIP(ctx, hipMemcpyAsync(joint, out + pp + vp, vv * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    JL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JL_OK;
}

// the 2 x 2 table of one pair from the three count tables, and its statistics (docs/SPEC.md §15)
int jl_linkage_stats(const uint32_t *both, const uint32_t *carry, const uint32_t *joint, const uint32_t *var_pos, uint32_t n_pos,
                     uint32_t n_var, uint32_t v, uint32_t w, jl_link_pair *out)
{
    static const char *fn = "jl_linkage_stats";
    if (!both || !carry || !joint || !var_pos || !out) return jl_fail(nullptr, JL_ERR_ARG, "%s: a NULL array", fn);
    if (v >= n_var || w >= n_var) return jl_fail(nullptr, JL_ERR_ARG, "%s: variants %u and %u, the table has %u", fn, v, w, n_var);
    const uint32_t p = var_pos[v], q = var_pos[w];
    if (p >= n_pos || q >= n_pos) return jl_fail(nullptr, JL_ERR_ARG, "%s: position index %u beyond the %u positions", fn, p >= n_pos ? p : q, n_pos);
    if (p == q) return jl_fail(nullptr, JL_ERR_ARG, "%s: variants %u and %u lie at one position", fn, v, w);
    const uint64_t n = both[(size_t)p * n_pos + q], n11 = joint[(size_t)v * n_var + w];
    const uint64_t row1 = carry[(size_t)v * n_pos + q], col1 = carry[(size_t)w * n_pos + p];   // reads that carry v / w among the n
    if (row1 > n || col1 > n || n11 > row1 || n11 > col1 || row1 + col1 - n11 > n)
        return jl_fail(nullptr, JL_ERR_ARG, "%s: the tables are not those of one call (a cell of the pair's table would be negative)", fn);
    const uint64_t row0 = n - row1, col0 = n - col1;
    memset(out, 0, sizeof *out);
    out->n = (uint32_t)n, out->n11 = (uint32_t)n11, out->n10 = (uint32_t)(row1 - n11), out->n01 = (uint32_t)(col1 - n11);
    out->n00 = (uint32_t)(n - row1 - col1 + n11);
    out->p_positive = out->p_negative = 1.0;
    if (row1 == 0 || row0 == 0 || col1 == 0 || col0 == 0) return JL_OK;   // a margin of 0: one table only
    // D_num = n11 n - row1 col1 in exact integers: both products are below 2^64, every product of two of them below 2^128
    typedef unsigned __int128 u128;
    const u128 left = (u128)n11 * n, right = (u128)row1 * col1;
    const bool negative = left < right;
    const u128 d = negative ? right - left : left - right;   // < 2^62
    out->r2 = (double)(d * d) / (double)((u128)(row1 * row0) * (u128)(col1 * col0));
    const uint64_t d_max = negative ? std::min(row1 * col1, row0 * col0) : std::min(row1 * col0, row0 * col1);
    out->d_prime = d_max ? (negative ? -1.0 : 1.0) * ((double)d / (double)d_max) : 0.0;
    hypergeometric_tails((uint32_t)n11, (uint32_t)col1, (uint32_t)row1, (uint32_t)n, &out->p_positive, &out->p_negative);
    return JL_OK;
}

}  // extern "C"
