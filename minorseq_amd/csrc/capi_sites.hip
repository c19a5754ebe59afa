// capi_sites.hip — jl_sites_assemble of include/juliet_hip.h: a resident matrix of chosen codon starts of another resident matrix,
// the called deletions among them recoded to a two-letter alphabet, for the phasing that exists to group over (docs/SPEC.md §18).
// Everything is checked here, on the host, before `pc` is touched: sites_assemble_kernel (kernels_sites.hip) forms its addresses
// from the table and the two strides without looking at them.
#include "jl_internal.h"

extern "C" {

int jl_sites_assemble(jl_ctx *pc, jl_ctx *src, const jl_site *sites, uint32_t n_sites)
{
    static const char *fn = "jl_sites_assemble";
    if (!pc || !src || !sites) return jl_fail(pc, JL_ERR_ARG, "%s: a NULL argument", fn);
    if (pc == src) return jl_fail(pc, JL_ERR_ARG, "%s: the source is the destination itself", fn);
    if (src->device != pc->device) return jl_fail(pc, JL_ERR_ARG, "%s: the source is on device %d, the destination on %d", fn, src->device, pc->device);
    if (!src->d_msa) return jl_fail(pc, JL_ERR_STATE, "%s: the source has no resident matrix", fn);
    if (n_sites == 0 || n_sites > (uint32_t)JL_SITES_MAX) return jl_fail(pc, JL_ERR_ARG, "%s: %u sites, 1 to %d", fn, n_sites, (int)JL_SITES_MAX);
    for (uint32_t k = 0; k < n_sites; ++k) {
        const jl_site &s = sites[k];
        if ((uint64_t)s.col + 2u >= src->n_cols)
            return jl_fail(pc, JL_ERR_ARG, "%s: site %u at column %u, its codon ends beyond the source's %u columns", fn, k, s.col, src->n_cols);
        if (s.kind > (uint8_t)JL_SITE_DELETION) return jl_fail(pc, JL_ERR_ARG, "%s: site %u has kind %u (0 codon, 1 deletion)", fn, k, s.kind);
        if (s.fill != (uint8_t)JL_SITE_NO_FILL && s.fill > 63u)
            return jl_fail(pc, JL_ERR_ARG, "%s: site %u has fill %u, neither a codon (0..63) nor 0xFF", fn, k, s.fill);
        if (s.kind == (uint8_t)JL_SITE_DELETION && s.fill != (uint8_t)JL_SITE_NO_FILL)
            return jl_fail(pc, JL_ERR_ARG, "%s: site %u is a deletion site with a fill (%u)", fn, k, s.fill);
        if (k) {
            const jl_site &q = sites[k - 1u];
            if (q.col == s.col && q.kind == s.kind) return jl_fail(pc, JL_ERR_ARG, "%s: sites %u and %u are the same (column %u, kind %u)", fn, k - 1u, k, s.col, s.kind);
            if (q.col > s.col || (q.col == s.col && q.kind > s.kind))
                return jl_fail(pc, JL_ERR_ARG, "%s: site %u (column %u, kind %u) is not in ascending order of (column, kind)", fn, k, s.col, s.kind);
        }
    }
    JL_HIP(pc, hipSetDevice(pc->device));
    hipStream_t st = pc->stream;
    // the table into pinned staging (an upload of the last call may still read the staging: wait for it)
    jl_site *h_sites = nullptr;
    JL_HIP(pc, pc->sites_in.host(n_sites, &h_sites));
    for (uint32_t k = 0; k < n_sites; ++k) h_sites[k] = jl_site{sites[k].col, sites[k].kind, sites[k].fill, 0};
    if (src->stream != st) JL_HIP(pc, hipStreamSynchronize(src->stream));   // the source is complete
    // (read before the allocation: the sizes the kernel forms its addresses from)
    jl_sites_args A = {};
    A.src = src->d_msa, A.src_stride = src->plane_stride;   // (a multiple of 16, >= ceil(n_reads / 8): set_shape, jl_msa_adopt)
    A.n_reads = src->n_reads;
    A.n_sites = n_sites;
    if (int rc = jl_msa_alloc(pc, A.n_reads, 3u * n_sites, 0)) return rc;
    hipError_t e = pc->sites_in.upload(st, n_sites);
    if (e == hipSuccess) {
        A.dst = pc->d_msa, A.dst_stride = pc->plane_stride;
        A.sites = pc->sites_in.dev;
        jl_launch_sites_assemble(&A, st);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return jl_fail(pc, jl_hip_status(e), "%s: %s", fn, hipGetErrorString(e));
    return JL_OK;
}

}  // extern "C"
