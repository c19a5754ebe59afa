// capi_del.hip — jl_codon_deletions_async / _fetch of include/juliet_hip.h: at every codon start of the resident matrix the reads
// with a whole codon, a whole-codon deletion, a partly deleted codon, and the reads that span it (docs/SPEC.md §16), and the
// host-only test of one position's counts against the error model (jl_deletion_test).  The call owns its buffer and touches
// nothing else of the context: no stage result, no plan, no captured graph sees it.  Every size the kernel (kernels_del.hip)
// forms an address from is checked here.
#include <math.h>
#include <string.h>

#include "jl_fisher.h"
#include "jl_internal.h"

extern "C" {

int jl_codon_deletions_async(jl_ctx *ctx)
{
    static const char *fn = "jl_codon_deletions_async";
    if (!ctx) return JL_ERR_ARG;
    if (!ctx->d_msa) return jl_fail(ctx, JL_ERR_STATE, "%s: no resident matrix", fn);
    if (ctx->n_cols < 3u) return jl_fail(ctx, JL_ERR_ARG, "%s: %u columns hold no codon (at least 3)", fn, ctx->n_cols);
    JL_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t words = (size_t)(ctx->n_cols - 2u) * 4u;
    ctx->del_cols = 0;   // (what was fetchable is gone as soon as the buffer may move)
    hipError_t e = ctx->del_out.grow_discard(st, words);
    if (e == hipSuccess) e = hipMemsetAsync(ctx->del_out, 0, words * sizeof(uint32_t), st);
    if (e == hipSuccess) {
        jl_del_args A = {};
        A.msa = ctx->d_msa, A.plane_stride = ctx->plane_stride;   // (a multiple of 16, >= ceil(n_reads / 8): set_shape, jl_msa_adopt)
        A.n_reads = ctx->n_reads, A.n_cols = ctx->n_cols;
        A.cnt = ctx->del_out;
        jl_launch_codon_deletions(&A, st);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return jl_fail(ctx, jl_hip_status(e), "%s: %s", fn, hipGetErrorString(e));
    ctx->del_cols = ctx->n_cols;
    return JL_OK;
}

int jl_codon_deletions_fetch(jl_ctx *ctx, uint32_t *cnt)
{
    if (!ctx) return JL_ERR_ARG;
    if (!ctx->del_cols) return jl_fail(ctx, JL_ERR_STATE, "jl_codon_deletions_fetch before jl_codon_deletions_async");
    JL_HIP(ctx, hipSetDevice(ctx->device));
    if (cnt)
        JL_HIP(ctx, hipMemcpyAsync(cnt, ctx->del_out, (size_t)(ctx->del_cols - 2u) * 4u * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    JL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JL_OK;
}

// one position's counts against the rate of whole-codon deletions by error (docs/SPEC.md §16): the codon test of §5 with
// coverage = codon + del3 and P_err = prm->err.deletion
int jl_deletion_test(const uint32_t cnt[4], const jl_params *prm, double n_tests, jl_deletion_call *out)
{
    static const char *fn = "jl_deletion_test";
    if (!cnt || !prm || !out) return jl_fail(nullptr, JL_ERR_ARG, "%s: a NULL argument", fn);
    if (!(n_tests > 0.0)) return jl_fail(nullptr, JL_ERR_ARG, "%s: n_tests %g, the resolved Bonferroni factor is above 0", fn, n_tests);
    const double rate = prm->err.deletion;
    if (!(rate >= 0.0 && rate <= 1.0)) return jl_fail(nullptr, JL_ERR_ARG, "%s: deletion rate %g outside [0, 1]", fn, rate);
    const uint64_t cov64 = (uint64_t)cnt[0] + cnt[1];
    if (cov64 > 0xFFFFFFFFull) return jl_fail(nullptr, JL_ERR_ARG, "%s: codon + del3 = %llu reads do not fit 32 bits", fn, (unsigned long long)cov64);
    const uint32_t cov = (uint32_t)cov64, del3 = cnt[1];
    memset(out, 0, sizeof *out);
    out->count = del3, out->coverage = cov, out->partial = cnt[2];
    out->p_value = 1.0, out->log_p = 0.0;
    if (cov == 0u) return JL_OK;
    const double x = (double)cov * rate;
    double r = prm->expected_round == 1 ? floor(x) : (prm->expected_round == 2 ? floor(x + 0.5) : ceil(x));
    if (r < 0.0) r = 0.0;
    if (r > (double)cov) r = (double)cov;
    const uint32_t e = (uint32_t)r;
    out->expected = e;
    double lp = 0.0;
    const double p = prm->tail == 0 ? jl_fisher_greater_equal_rows(del3, e, cov, &lp) : jl_fisher_two_sided_equal_rows(del3, e, cov, &lp);
    double p_adj = p * n_tests;
    if (p_adj > 1.0) p_adj = 1.0;
    bool called = del3 > 0u && p_adj < prm->alpha;   // (nothing observed is never called: §5 tests the codons with hist > 0 only)
    const double perc = 100.0 * (double)del3 / (double)cov;
    if (prm->min_perc >= 0.0 && !(perc > prm->min_perc)) called = false;
    if (prm->max_perc >= 0.0 && !(perc < prm->max_perc)) called = false;
    out->called = called ? 1u : 0u;
    out->p_value = p_adj, out->log_p = lp;
    return JL_OK;
}

}  // extern "C"
