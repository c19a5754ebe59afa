// capi_control.hip — jl_control_call_async / _fetch of include/juliet_hip.h: the codons of a sample's pileup tested against the
// counts a control's pileup holds at the same positions (docs/SPEC.md §21), and the host-only test of one such table
// (jl_control_test).  The call owns its result buffers in the SAMPLE's context; the masks and staged rows of the call stage are
// its scratch.  No stage result, no plan and no captured graph of either context sees it.  Everything the kernels
// (kernels_control.hip) form an address from is checked here: both contexts hold the same window and the same position list.
#include <math.h>
#include <string.h>

#include "jl_fisher_general.h"
#include "jl_internal.h"

namespace {

// the reference codon of position p as build_plan (capi.hip) resolves it
uint8_t ref_config(const jl_ctx *ctx, uint32_t p)
{
    if (!ctx->have_ref) return JL_REF_MAJORITY;
    const uint64_t r = (uint64_t)ctx->win_begin + ctx->h_pos_col[p];
    const std::vector<uint8_t> &s = ctx->refseq;
    if (r + 2 >= s.size() || s[r] > 3 || s[r + 1] > 3 || s[r + 2] > 3) return JL_REF_SKIP;
    return (uint8_t)(16 * s[r] + 4 * s[r + 1] + s[r + 2]);
}

}  // namespace

extern "C" {

int jl_control_call_async(jl_ctx *sample, jl_ctx *control, const jl_params *prm, const uint64_t *drm_masks)
{
    static const char *fn = "jl_control_call_async";
    if (!sample) return jl_fail(nullptr, JL_ERR_ARG, "%s: no sample context", fn);
    if (!control) return jl_fail(sample, JL_ERR_ARG, "%s: no control context", fn);
    if (!prm) return jl_fail(sample, JL_ERR_ARG, "%s: no parameters", fn);
    if (prm->tail != 0) return jl_fail(sample, JL_ERR_ARG, "%s: tail %d: only the one-sided greater test (0) is defined against a control", fn, (int)prm->tail);
    if (!(prm->alpha > 0.0)) return jl_fail(sample, JL_ERR_ARG, "%s: alpha must be > 0", fn);
    if (sample->device != control->device)
        return jl_fail(sample, JL_ERR_ARG, "%s: the sample is on device %d, the control on device %d", fn, sample->device, control->device);
    if (!sample->pileup_done) return jl_fail(sample, JL_ERR_STATE, "%s: the sample has no pileup (jl_pileup_async first)", fn);
    if (!control->pileup_done) return jl_fail(sample, JL_ERR_STATE, "%s: the control has no pileup (jl_pileup_async first)", fn);
    if (sample->n_cols != control->n_cols || sample->win_begin != control->win_begin)
        return jl_fail(sample, JL_ERR_STATE, "%s: windows differ: the sample's %u columns from %u, the control's %u from %u", fn, sample->n_cols,
                       sample->win_begin, control->n_cols, control->win_begin);
    if (sample->P != control->P || sample->h_pos_gene != control->h_pos_gene || sample->h_pos_codon != control->h_pos_codon ||
        sample->h_pos_col != control->h_pos_col)
        return jl_fail(sample, JL_ERR_STATE, "%s: position lists differ (%u positions in the sample, %u in the control)", fn, sample->P, control->P);
    for (uint32_t p = 0; p < sample->P; ++p)
        if (ref_config(sample, p) != ref_config(control, p))
            return jl_fail(sample, JL_ERR_STATE, "%s: the reference codons of position %u differ", fn, p);
    const uint32_t P = sample->P;
    JL_HIP(sample, hipSetDevice(sample->device));
    hipStream_t st = sample->stream;
    if (drm_masks && P) {
        JL_HIP(sample, hipMemcpyAsync(sample->d_drm, drm_masks, (size_t)P * 8, hipMemcpyHostToDevice, st));
        JL_HIP(sample, hipStreamSynchronize(st));
    }
    sample->ctl_done = false;   // (what was fetchable is gone as soon as a buffer may move)
    hipError_t e = sample->ctl_rows.grow_discard(st, JL_VARIANT_CAP);
    if (e == hipSuccess) e = sample->ctl_out.grow_discard(st, 2u + (size_t)P);
    if (e == hipSuccess && control->stream != st) {   // the control's histograms are complete before the launch reads them
        if (!sample->ctl_ev.ev) e = hipEventCreateWithFlags(&sample->ctl_ev.ev, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(sample->ctl_ev.ev, control->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(st, sample->ctl_ev.ev, 0);
    }
    if (e == hipSuccess) {
        jl_control_args A;
        memset(&A, 0, sizeof A);
        const double n_tests = prm->n_tests > 0.0 ? prm->n_tests : sample->default_n_tests;
        jl_fill_call_args(sample, prm, n_tests, &A.A);
        A.pos_gene = sample->d_pos_gene, A.pos_codon = sample->d_pos_codon, A.pos_col = sample->d_pos_col;
        A.pos_refcfg = sample->d_pos_refcfg;
        A.hist_s = sample->d_hist, A.hist_c = control->d_hist;
        A.drm = drm_masks ? (const uint64_t *)sample->d_drm : nullptr;
        A.called = sample->d_called, A.staged = sample->d_staged;
        A.ctl_cov = sample->ctl_out + 2;
        A.rows = sample->ctl_rows, A.n_rows = sample->ctl_out, A.cap = JL_VARIANT_CAP;
        jl_launch_control_call(&A, st);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return jl_fail(sample, jl_hip_status(e), "%s: %s", fn, hipGetErrorString(e));
    sample->ctl_pos_gene = sample->h_pos_gene, sample->ctl_pos_codon = sample->h_pos_codon;
    sample->ctl_p = P;
    sample->ctl_done = true;
    return JL_OK;
}

int jl_control_call_fetch(jl_ctx *sample, jl_variant *rows, uint32_t *control_coverage, uint32_t cap, uint32_t *n_out)
{
    static const char *fn = "jl_control_call_fetch";
    if (!sample) return jl_fail(nullptr, JL_ERR_ARG, "%s: no sample context", fn);
    if (!n_out || (cap && (!rows || !control_coverage))) return jl_fail(sample, JL_ERR_ARG, "%s: a NULL argument", fn);
    if (!sample->ctl_done) return jl_fail(sample, JL_ERR_STATE, "%s before jl_control_call_async", fn);
    JL_HIP(sample, hipSetDevice(sample->device));
    hipStream_t st = sample->stream;
    const uint32_t P = sample->ctl_p;
    std::vector<uint32_t> out(2u + (size_t)P);
    JL_HIP(sample, hipMemcpyAsync(out.data(), sample->ctl_out, out.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    JL_HIP(sample, hipStreamSynchronize(st));
    const uint32_t n = out[0];
    *n_out = n;
    const uint32_t have = n < JL_VARIANT_CAP ? n : JL_VARIANT_CAP, take = have < cap ? have : cap;
    if (take) {
        JL_HIP(sample, hipMemcpyAsync(rows, sample->ctl_rows, (size_t)take * sizeof(jl_variant), hipMemcpyDeviceToHost, st));
        JL_HIP(sample, hipStreamSynchronize(st));
    }
    // rows and positions ascend together in (gene, codon): one walk finds every row's position
    uint32_t p = 0;
    for (uint32_t i = 0; i < take; ++i) {
        while (p < P && (sample->ctl_pos_gene[p] != rows[i].gene || sample->ctl_pos_codon[p] != rows[i].codon_pos)) ++p;
        if (p == P) return jl_fail(sample, JL_ERR_DEVICE, "%s: row %u lies at no position of the call", fn, i);
        control_coverage[i] = out[2u + p];
    }
    if (n > take) return jl_fail(sample, JL_ERR_OVERFLOW, "%u variant rows, capacity %u (device table holds %u)", n, cap, JL_VARIANT_CAP);
    return JL_OK;
}

// one codon of one position: a of the sample's cov_s reads carry it, c of the control's cov_c (docs/SPEC.md §21) — the
// expressions the kernel evaluates, compiled for the host
int jl_control_test(uint32_t a, uint32_t cov_s, uint32_t c, uint32_t cov_c, const jl_params *prm, double n_tests, jl_control_call *out)
{
    static const char *fn = "jl_control_test";
    if (!prm || !out) return jl_fail(nullptr, JL_ERR_ARG, "%s: a NULL argument", fn);
    if (!(n_tests > 0.0)) return jl_fail(nullptr, JL_ERR_ARG, "%s: n_tests %g, the resolved Bonferroni factor is above 0", fn, n_tests);
    if (prm->tail != 0) return jl_fail(nullptr, JL_ERR_ARG, "%s: tail %d: only the one-sided greater test (0) is defined against a control", fn, (int)prm->tail);
    if (a > cov_s || c > cov_c) return jl_fail(nullptr, JL_ERR_ARG, "%s: a count above its coverage (%u of %u, %u of %u)", fn, a, cov_s, c, cov_c);
    memset(out, 0, sizeof *out);
    out->count = a, out->coverage = cov_s, out->control_count = c, out->control_coverage = cov_c;
    out->p_value = 1.0, out->log_p = 0.0;
    if (cov_s == 0u || cov_c == 0u || a == 0u) return JL_OK;   // a skipped position; nothing observed is never called
    double lp = 0.0;
    const double p = jl_fisher_greater_general(a, cov_s, c, cov_c, &lp);
    double p_adj = p * n_tests;
    if (p_adj > 1.0) p_adj = 1.0;
    bool called = p_adj < prm->alpha;
    const double perc = 100.0 * (double)a / (double)cov_s;
    if (prm->min_perc >= 0.0 && !(perc > prm->min_perc)) called = false;
    if (prm->max_perc >= 0.0 && !(perc < prm->max_perc)) called = false;
    out->called = called ? 1u : 0u;
    out->p_value = p_adj, out->log_p = lp;
    return JL_OK;
}

// the same header as the DEVICE evaluates it, one thread a table (a diagnostic, as jl_fisher_eval_tail is for jl_fisher.h)
int jl_control_eval(jl_ctx *ctx, const uint32_t *a, const uint32_t *cov_s, const uint32_t *c, const uint32_t *cov_c, uint32_t n,
                    double n_tests, double alpha, double *p, double *log_p, uint32_t *skipped)
{
    static const char *fn = "jl_control_eval";
    if (!ctx) return JL_ERR_ARG;
    if (!a || !cov_s || !c || !cov_c || !p || !log_p) return jl_fail(ctx, JL_ERR_ARG, "%s: a NULL array", fn);
    if (skipped && !(n_tests > 0.0 && alpha > 0.0)) return jl_fail(ctx, JL_ERR_ARG, "%s: the gated form needs n_tests > 0 and alpha > 0", fn);
    if (n == 0) return JL_OK;
    for (uint32_t i = 0; i < n; ++i)
        if (cov_s[i] == 0u || cov_c[i] == 0u || a[i] > cov_s[i] || c[i] > cov_c[i])
            return jl_fail(ctx, JL_ERR_ARG, "%s: table %u: coverages above 0, a <= cov_s and c <= cov_c", fn, i);
    JL_HIP(ctx, hipSetDevice(ctx->device));
    uint32_t *d_in = nullptr;   // a | cov_s | c | cov_c | skipped
    double *d_out = nullptr;    // p | log_p
    JL_HIP(ctx, hipMalloc(&d_in, (size_t)n * 20));
    if (hipMalloc(&d_out, (size_t)n * 16) != hipSuccess) { hipFree(d_in); return jl_fail(ctx, JL_ERR_MEMORY, "%s buffers", fn); }
    hipStream_t st = ctx->stream;
    const uint32_t *src[4] = {a, cov_s, c, cov_c};
    hipError_t e = hipSuccess;
    for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipMemcpyAsync(d_in + k * (size_t)n, src[k], (size_t)n * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        uint32_t *d_skip = skipped ? d_in + 4 * (size_t)n : nullptr;
        jl_launch_control_eval(n, d_in, d_in + n, d_in + 2 * (size_t)n, d_in + 3 * (size_t)n, n_tests, alpha, d_out, d_out + n, d_skip, st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(p, d_out, (size_t)n * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(log_p, d_out + n, (size_t)n * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && skipped) e = hipMemcpyAsync(skipped, d_in + 4 * (size_t)n, (size_t)n * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    hipFree(d_in);
    hipFree(d_out);
    if (e != hipSuccess) return jl_fail(ctx, JL_ERR_DEVICE, "%s: %s", fn, hipGetErrorString(e));
    return JL_OK;
}

}  // extern "C"
