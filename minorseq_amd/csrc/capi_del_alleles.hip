// capi_del_alleles.hip — jl_deletion_alleles_async / _fetch of include/juliet_hip.h: every read's maximal runs of '-' in the
// resident matrix, the bounded ones as a table of (start, length) alleles with their reads and their flank coverage, the open
// ones per column (docs/SPEC.md §25), and the host-only test of one allele against a rate of deletions by error
// (jl_deletion_allele_test).  The call owns its buffers and touches nothing else of the context: no stage result, no plan, no
// captured graph sees it.  Every size the kernels (kernels_del_alleles.hip) form an address from is checked here.
// ONE WAIT.  The table must hold every distinct allele, and the caller gives no capacity: the enqueue counts the runs of the matrix
// with one launch and waits for that single number.  distinct alleles <= min(runs, (n_cols - 1)(n_cols - 2) / 2) — the second being
// the (s, len) with 1 <= s and s + len <= n_cols - 1 — and the table has twice as many slots or more.  Everything after that is
// enqueued on the context's stream: the walk, the flank counts and the rows, so the fetch needs the matrix no more.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "jl_fisher.h"
#include "jl_internal.h"

namespace {

constexpr size_t kMeta64 = 4;      // dal_u64: n_starts, runs[2], a spare word; then the keys
constexpr size_t kMeta32 = 4;      // dal_u32: n_occ and three spare words; then diff, count, occ

}  // namespace

extern "C" {

int jl_deletion_alleles_async(jl_ctx *ctx)
{
    static const char *fn = "jl_deletion_alleles_async";
    if (!ctx) return JL_ERR_ARG;
    if (!ctx->d_msa || !ctx->n_reads || !ctx->n_cols) return jl_fail(ctx, JL_ERR_STATE, "%s: no resident matrix", fn);
    const uint64_t n_words = (ctx->n_reads + 31u) / 32u;
    if (n_words > 0xFFFFFFFFull) return jl_fail(ctx, JL_ERR_ARG, "%s: %llu reads are beyond this call", fn, (unsigned long long)ctx->n_reads);
    if (4u * n_words > ctx->plane_stride)   // (a multiple of 16, >= ceil(n_reads / 8): set_shape, jl_msa_adopt)
        return jl_fail(ctx, JL_ERR_ARG, "%s: plane stride %llu holds no %llu reads", fn, (unsigned long long)ctx->plane_stride, (unsigned long long)ctx->n_reads);
    JL_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t n_cols = ctx->n_cols;
    ctx->dal_cols = 0;   // (what was fetchable is gone as soon as a buffer may move)

    jl_dal_args A = {};
    A.msa = ctx->d_msa, A.plane_stride = ctx->plane_stride;
    A.n_reads = ctx->n_reads, A.n_cols = n_cols, A.n_words = (uint32_t)n_words;

    // the runs of the matrix: the one number this call waits for
    unsigned long long n_runs = 0;
    hipError_t e = ctx->dal_u64.grow_discard(st, kMeta64);
    if (e == hipSuccess) e = hipMemsetAsync(ctx->dal_u64, 0, kMeta64 * sizeof(unsigned long long), st);
    if (e == hipSuccess) {
        A.n_starts = ctx->dal_u64;
        jl_launch_deletion_starts(&A, st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&n_runs, ctx->dal_u64, sizeof n_runs, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return jl_fail(ctx, jl_hip_status(e), "%s: %s", fn, hipGetErrorString(e));

    const uint64_t possible = n_cols >= 3u ? (uint64_t)(n_cols - 1u) * (n_cols - 2u) / 2u : 0u;
    const uint64_t bound = std::min<uint64_t>(n_runs, possible);
    if (bound > (1ull << 30))
        return jl_fail(ctx, JL_ERR_MEMORY, "%s: %llu runs in %u columns: a table of up to %llu alleles is beyond this call", fn, n_runs, n_cols,
                       (unsigned long long)bound);
    const uint32_t cap = (uint32_t)std::max<uint64_t>(bound, 1u);
    uint64_t slots = 64;
    while (slots < 2u * bound) slots <<= 1;

    const size_t words32 = kMeta32 + (size_t)n_cols + 1u + slots;   // what is zeroed; occ [cap] follows
    e = ctx->dal_u64.grow_discard(st, kMeta64 + slots);
    if (e == hipSuccess) e = ctx->dal_u32.grow_discard(st, words32 + cap);
    if (e == hipSuccess) e = ctx->dal_rows.grow_discard(st, cap);
    if (e == hipSuccess) e = hipMemsetAsync(ctx->dal_u64, 0, kMeta64 * sizeof(unsigned long long), st);
    if (e == hipSuccess) e = hipMemsetAsync(ctx->dal_u64 + kMeta64, 0xFF, slots * sizeof(unsigned long long), st);
    if (e == hipSuccess) e = hipMemsetAsync(ctx->dal_u32, 0, words32 * sizeof(uint32_t), st);
    if (e == hipSuccess && n_runs) {
        A.n_starts = nullptr;
        A.runs = ctx->dal_u64 + 1;
        A.keys = ctx->dal_u64 + kMeta64, A.slots_mask = slots - 1u;
        A.n_occ = ctx->dal_u32;
        A.diff = ctx->dal_u32 + kMeta32;
        A.count = A.diff + n_cols + 1u;
        A.occ = A.count + slots, A.occ_cap = cap;
        jl_launch_deletion_runs(&A, st);
        e = hipGetLastError();
        if (e == hipSuccess) {
            jl_launch_deletion_rows(&A, ctx->dal_rows, st);
            e = hipGetLastError();
        }
    }
    if (e != hipSuccess) return jl_fail(ctx, jl_hip_status(e), "%s: %s", fn, hipGetErrorString(e));
    ctx->dal_cols = n_cols, ctx->dal_slots = slots, ctx->dal_cap = cap;
    return JL_OK;
}

int jl_deletion_alleles_fetch(jl_ctx *ctx, uint64_t runs[2], uint32_t *open, jl_deletion_allele *rows, uint32_t cap, uint32_t *n_rows)
{
    static const char *fn = "jl_deletion_alleles_fetch";
    if (!ctx) return JL_ERR_ARG;
    if (!ctx->dal_cols) return jl_fail(ctx, JL_ERR_STATE, "%s before jl_deletion_alleles_async", fn);
    JL_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t n_cols = ctx->dal_cols;
    unsigned long long meta[kMeta64] = {};
    uint32_t n = 0;
    std::vector<uint32_t> diff(open ? (size_t)n_cols + 1u : 0u);
    JL_HIP(ctx, hipMemcpyAsync(meta, ctx->dal_u64, sizeof meta, hipMemcpyDeviceToHost, st));
    JL_HIP(ctx, hipMemcpyAsync(&n, ctx->dal_u32, sizeof n, hipMemcpyDeviceToHost, st));
    if (open) JL_HIP(ctx, hipMemcpyAsync(diff.data(), ctx->dal_u32 + kMeta32, diff.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    JL_HIP(ctx, hipStreamSynchronize(st));
    if (n > ctx->dal_cap) return jl_fail(ctx, JL_ERR_DEVICE, "%s: %u alleles where at most %u can exist", fn, n, ctx->dal_cap);
    if (runs) runs[0] = meta[1], runs[1] = meta[2];
    if (open) {   // the kernel left + k where k open runs begin and - k where they end: the reads inside one are the prefix sum
        uint32_t acc = 0;
        for (uint32_t c = 0; c < n_cols; ++c) open[c] = acc += diff[c];
    }
    if (n_rows) *n_rows = n;
    if (!rows || !n) return JL_OK;
    if (cap < n) return jl_fail(ctx, JL_ERR_ARG, "%s: room for %u rows, the table has %u", fn, cap, n);
    JL_HIP(ctx, hipMemcpyAsync(rows, ctx->dal_rows, (size_t)n * sizeof *rows, hipMemcpyDeviceToHost, st));
    JL_HIP(ctx, hipStreamSynchronize(st));
    // the table's order is the order in which its slots were claimed: the delivered one is the keys'
    std::sort(rows, rows + n, [](const jl_deletion_allele &x, const jl_deletion_allele &y) { return x.col != y.col ? x.col < y.col : x.len < y.len; });
    return JL_OK;
}

// one allele's reads against a rate of such deletions by error (docs/SPEC.md §25): the codon test of §5 with coverage = flank
int jl_deletion_allele_test(uint32_t count, uint32_t flank, const jl_params *prm, double rate, double n_tests, jl_deletion_allele_call *out)
{
    static const char *fn = "jl_deletion_allele_test";
    if (!prm || !out) return jl_fail(nullptr, JL_ERR_ARG, "%s: a NULL argument", fn);
    if (!(n_tests > 0.0)) return jl_fail(nullptr, JL_ERR_ARG, "%s: n_tests %g, the resolved Bonferroni factor is above 0", fn, n_tests);
    if (!(rate >= 0.0 && rate <= 1.0)) return jl_fail(nullptr, JL_ERR_ARG, "%s: deletion rate %g outside [0, 1]", fn, rate);
    if (count > flank) return jl_fail(nullptr, JL_ERR_ARG, "%s: count %u above the flank coverage %u", fn, count, flank);
    const uint32_t cov = flank;
    memset(out, 0, sizeof *out);
    out->count = count, out->coverage = cov;
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
