// kernels_control.hip — codon calls of a sample against a CONTROL's counts at the same position (jl_control_call_async;
// docs/SPEC.md §21): the table [[hs[j], cov_s - hs[j]], [hc[j], cov_c - hc[j]]] under the general-margin Fisher test of
// jl_fisher_general.h, Bonferroni, the filters of §7 on the sample's frequency, rows as §6 with expected := hc[j].
// Shape: call_kernel's (kernels_call.hip).  A wave evaluates a position, lane = codon, four positions a workgroup; each lane
// loads its bin of both histograms, coverages and the sample's majority come from the wave reductions of call_eval.h, the lanes
// with a codon to test sum their tails (of different lengths: up to min(a, c) terms before the early stop), called rows go to
// the staged [P][64] area; one workgroup then compacts them in (gene, codon, codon index) order (jl_compact_rows_block).
// Both launches follow each other on the sample's stream, so the stores are plain.
#include <string.h>

#include "call_eval.h"
#include "jl_fisher_general.h"
#include "jl_internal.h"

namespace {

__global__ __launch_bounds__(256) void control_call_kernel(jl_control_args w)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint32_t p = blockIdx.x * 4u + wid;
    if (p >= w.A.P) return;  // wave-uniform
    const uint32_t col = w.pos_col[p];
    const uint32_t hs = w.hist_s[(uint64_t)col * 64u + lane];
    const uint32_t hc = w.hist_c[(uint64_t)col * 64u + lane];
    const uint32_t cov_s = jl_wave_sum_all(hs), cov_c = jl_wave_sum_all(hc);
    if (lane == 0) w.ctl_cov[p] = cov_c;
    uint32_t ref = w.pos_refcfg[p];
    if (ref == JL_REF_MAJORITY) {
        // argmax of the SAMPLE's histogram, lowest codon index on ties (SPEC §4)
        const uint64_t key = ((uint64_t)hs << 8) | (uint64_t)(63u - lane);
        const uint64_t best = jl_wave_max_all(key);
        ref = cov_s ? 63u - (uint32_t)(best & 0xFFu) : JL_REF_SKIP;
    }
    bool is_called = false;
    double p_adj = 1.0, lp = 0.0;
    if (ref < 64u && cov_s > 0u && cov_c > 0u && hs > 0u && lane != ref) {
        bool skipped;
        const double pv = jl_fisher_greater_general_or_skip(hs, cov_s, hc, cov_c, w.A.n_tests, w.A.alpha, &lp, &skipped);
        p_adj = pv * w.A.n_tests;
        if (p_adj > 1.0) p_adj = 1.0;
        is_called = !skipped && p_adj < w.A.alpha;
        const double perc = 100.0 * (double)hs / (double)cov_s;
        if (w.A.min_perc >= 0.0 && !(perc > w.A.min_perc)) is_called = false;
        if (w.A.max_perc >= 0.0 && !(perc < w.A.max_perc)) is_called = false;
        if (w.drm && !((w.drm[p] >> lane) & 1ull)) is_called = false;
    }
    const uint64_t mask = __ballot(is_called);
    if (lane == 0) w.called[p] = mask;
    if (is_called) {
        jl_variant v;
        v.gene = w.pos_gene[p];
        v.codon_pos = w.pos_codon[p];
        v.col = col;
        v.ref_codon = (uint8_t)ref;
        v.codon = (uint8_t)lane;
        v.flags = 0;
        v.count = hs;
        v.coverage = cov_s;
        v.expected = hc;
        v.pad_ = 0;
        v.p_value = p_adj;
        v.log_p = lp;
        uint64_t q[6];
        memcpy(q, &v, sizeof v);
        uint64_t *dst = reinterpret_cast<uint64_t *>(w.staged + (uint64_t)p * 64u + lane);
#pragma unroll
        for (int k = 0; k < 6; ++k) dst[k] = q[k];
    }
}

__global__ __launch_bounds__(256) void control_compact_kernel(jl_control_args w)
{
    __shared__ uint32_t s_scan[4];
    __shared__ uint32_t s_running;
    const uint32_t n = jl_compact_rows_block<false>(w.A.P, w.called, w.staged, w.rows, w.cap, s_scan, &s_running, nullptr, 0u, false);
    if (threadIdx.x == 0) w.n_rows[0] = n;
}

// jl_control_eval: the header's value for table i, nothing of the call stage around it (a diagnostic; not on any hot path)
__global__ __launch_bounds__(256) void control_eval_kernel(uint32_t n, const uint32_t *__restrict__ a,
                                                            const uint32_t *__restrict__ cov_s, const uint32_t *__restrict__ c,
                                                            const uint32_t *__restrict__ cov_c, double n_tests, double alpha,
                                                            double *__restrict__ p, double *__restrict__ lp,
                                                            uint32_t *__restrict__ skipped)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    double l;
    if (skipped) {
        bool s;
        p[i] = jl_fisher_greater_general_or_skip(a[i], cov_s[i], c[i], cov_c[i], n_tests, alpha, &l, &s);
        skipped[i] = s ? 1u : 0u;
    } else {
        p[i] = jl_fisher_greater_general(a[i], cov_s[i], c[i], cov_c[i], &l);
    }
    lp[i] = l;
}

}  // namespace

void jl_launch_control_eval(uint32_t n, const uint32_t *a, const uint32_t *cov_s, const uint32_t *c, const uint32_t *cov_c,
                            double n_tests, double alpha, double *p, double *lp, uint32_t *skipped, hipStream_t st)
{
    hipLaunchKernelGGL(control_eval_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, n, a, cov_s, c, cov_c, n_tests, alpha, p, lp,
                       skipped);
}

// every array of `a` holds what its comment in jl_internal.h says; a->A.P may be 0 (the table is then empty)
void jl_launch_control_call(const jl_control_args *a, hipStream_t st)
{
    if (a->A.P) hipLaunchKernelGGL(control_call_kernel, dim3((a->A.P + 3u) / 4u), dim3(256), 0, st, *a);
    hipLaunchKernelGGL(control_compact_kernel, dim3(1), dim3(256), 0, st, *a);
}
