// capi_ins.hip — the in-frame insertion alleles of include/juliet_hip.h (docs/SPEC.md §17): the switch, the fetch of what a tracking
// record build left (capi_records.hip records_build enqueues the kernels of kernels_ins.hip), and the host-only test of one allele
// against a rate of in-frame insertions by error (jl_insertion_test); the per-read events of such a build (§19): switch and fetch.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "jl_fisher.h"
#include "jl_internal.h"

extern "C" {

int jl_msa_track_insertion_alleles(jl_ctx *ctx, int on)
{
    if (!ctx) return JL_ERR_ARG;
    ctx->track_ins_alleles = on != 0;
    return JL_OK;
}

int jl_insertion_alleles_fetch(jl_ctx *ctx, uint32_t *jcnt, jl_insertion_allele *rows, uint32_t cap, uint32_t *n_rows)
{
    static const char *fn = "jl_insertion_alleles_fetch";
    if (!ctx) return JL_ERR_ARG;
    if (!ctx->insal_valid)
        return jl_fail(ctx, JL_ERR_STATE, "%s: no insertion alleles: jl_msa_track_insertion_alleles(ctx, 1) before the record build of this matrix", fn);
    JL_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t slots = ctx->insal_slots;
    uint32_t n = 0;
    JL_HIP(ctx, hipMemcpyAsync(&n, ctx->insal_count + 2u * slots, sizeof n, hipMemcpyDeviceToHost, st));
    if (jcnt) JL_HIP(ctx, hipMemcpyAsync(jcnt, ctx->insal_jcnt, (size_t)ctx->n_cols * 16u, hipMemcpyDeviceToHost, st));
    JL_HIP(ctx, hipStreamSynchronize(st));
    if (n > slots) return jl_fail(ctx, JL_ERR_DEVICE, "%s: %u alleles in a table of %llu", fn, n, (unsigned long long)slots);
    if (n_rows) *n_rows = n;
    if (!rows || !n) return JL_OK;
    if (cap < n) return jl_fail(ctx, JL_ERR_ARG, "%s: room for %u rows, the table has %u", fn, cap, n);
    hipError_t e = ctx->insal_rows.grow_discard(st, n);
    if (e != hipSuccess) return jl_fail(ctx, jl_hip_status(e), "%s: %s", fn, hipGetErrorString(e));
    jl_launch_insertion_rows(ctx->insal_keys, ctx->insal_keys + slots, ctx->insal_count, ctx->insal_count + slots, n, ctx->insal_rows, st);
    JL_HIP(ctx, hipGetLastError());
    JL_HIP(ctx, hipMemcpyAsync(rows, ctx->insal_rows, (size_t)n * sizeof *rows, hipMemcpyDeviceToHost, st));
    JL_HIP(ctx, hipStreamSynchronize(st));
    // the table's order is the order in which its slots were claimed: the delivered one is the keys'
    std::sort(rows, rows + n, [](const jl_insertion_allele &x, const jl_insertion_allele &y) {
        return x.col != y.col ? x.col < y.col : x.len != y.len ? x.len < y.len : x.seq < y.seq;
    });
    return JL_OK;
}

int jl_msa_track_insertion_reads(jl_ctx *ctx, int on)
{
    if (!ctx) return JL_ERR_ARG;
    ctx->track_ins_reads = on != 0;
    return JL_OK;
}

int jl_insertion_reads_fetch(jl_ctx *ctx, jl_insertion_event *rows, uint32_t cap, uint32_t *n_rows)
{
    static const char *fn = "jl_insertion_reads_fetch";
    if (!ctx) return JL_ERR_ARG;
    if (!ctx->insev_valid)
        return jl_fail(ctx, JL_ERR_STATE, "%s: no insertion events: jl_msa_track_insertion_reads(ctx, 1) before the record build of this matrix", fn);
    JL_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    uint32_t n = 0;
    JL_HIP(ctx, hipMemcpyAsync(&n, ctx->insev_count, sizeof n, hipMemcpyDeviceToHost, st));
    JL_HIP(ctx, hipStreamSynchronize(st));
    if (n > ctx->insev_cap) return jl_fail(ctx, JL_ERR_DEVICE, "%s: %u events in a list of %u", fn, n, ctx->insev_cap);
    if (n_rows) *n_rows = n;
    if (!rows || !n) return JL_OK;
    if (cap < n) return jl_fail(ctx, JL_ERR_ARG, "%s: room for %u rows, the list has %u", fn, cap, n);
    JL_HIP(ctx, hipMemcpyAsync(rows, ctx->insev_rows, (size_t)n * sizeof *rows, hipMemcpyDeviceToHost, st));
    JL_HIP(ctx, hipStreamSynchronize(st));
    // the list's order is the order of the walk's atomics: the delivered one is (read, col)
    std::sort(rows, rows + n, [](const jl_insertion_event &x, const jl_insertion_event &y) { return x.read != y.read ? x.read < y.read : x.col < y.col; });
    return JL_OK;
}

// one allele's reads against the rate of in-frame insertions by error (docs/SPEC.md §17): the codon test of §5 with
// coverage = span - frameshift - unread and P_err = rate
int jl_insertion_test(uint32_t count, const uint32_t jcnt[4], const jl_params *prm, double rate, double n_tests, jl_insertion_call *out)
{
    static const char *fn = "jl_insertion_test";
    if (!jcnt || !prm || !out) return jl_fail(nullptr, JL_ERR_ARG, "%s: a NULL argument", fn);
    if (!(n_tests > 0.0)) return jl_fail(nullptr, JL_ERR_ARG, "%s: n_tests %g, the resolved Bonferroni factor is above 0", fn, n_tests);
    if (!(rate >= 0.0 && rate <= 1.0)) return jl_fail(nullptr, JL_ERR_ARG, "%s: insertion rate %g outside [0, 1]", fn, rate);
    const uint64_t out_of = (uint64_t)jcnt[2] + jcnt[3];
    if (out_of > jcnt[0])
        return jl_fail(nullptr, JL_ERR_ARG, "%s: frameshift + unread = %llu reads of %u spanning", fn, (unsigned long long)out_of, jcnt[0]);
    const uint32_t cov = jcnt[0] - (uint32_t)out_of;
    if (count > cov) return jl_fail(nullptr, JL_ERR_ARG, "%s: count %u above the coverage %u", fn, count, cov);
    memset(out, 0, sizeof *out);
    out->count = count, out->coverage = cov, out->frameshift = jcnt[2], out->unread = jcnt[3];
    out->p_value = 1.0, out->log_p = 0.0;
    if (cov == 0u) return JL_OK;
    const double x = (double)cov * rate;
    double r = prm->expected_round == 1 ? floor(x) : (prm->expected_round == 2 ? floor(x + 0.5) : ceil(x));
    if (r < 0.0) r = 0.0;
    if (r > (double)cov) r = (double)cov;
    const uint32_t e = (uint32_t)r;
    out->expected = e;
    double lp = 0.0;
    const double p = prm->tail == 0 ? jl_fisher_greater_equal_rows(count, e, cov, &lp) : jl_fisher_two_sided_equal_rows(count, e, cov, &lp);
    double p_adj = p * n_tests;
    if (p_adj > 1.0) p_adj = 1.0;
    bool called = count > 0u && p_adj < prm->alpha;
    const double perc = 100.0 * (double)count / (double)cov;
    if (prm->min_perc >= 0.0 && !(perc > prm->min_perc)) called = false;
    if (prm->max_perc >= 0.0 && !(perc < prm->max_perc)) called = false;
    out->called = called ? 1u : 0u;
    out->p_value = p_adj, out->log_p = lp;
    return JL_OK;
}

}  // extern "C"
