// capi_sites.hip — jl_sites_assemble and jl_sites_assemble_alleles of include/juliet_hip.h: a resident matrix of chosen codon starts
// of another resident matrix, the called deletions among them recoded to a two-letter alphabet (docs/SPEC.md §18), and the called
// insertion alleles of chosen junctions as sites of their own (§19), for the phasing that exists to group over.
// Everything is checked here, on the host, before `pc` is touched: the kernels of kernels_sites.hip form their addresses from the
// tables and the two strides without looking at them.
#include <vector>

#include "jl_internal.h"

namespace {

// Both entry points: `with_alleles` false is jl_sites_assemble, which knows kinds 0 and 1 only and takes no alleles.
int sites_assemble(const char *fn, jl_ctx *pc, jl_ctx *src, const jl_site *sites, uint32_t n_sites, const jl_insertion_allele *alleles,
                   uint32_t n_alleles, bool with_alleles)
{
    if (!pc || !src || !sites || (n_alleles && !alleles)) return jl_fail(pc, JL_ERR_ARG, "%s: a NULL argument", fn);
    if (pc == src) return jl_fail(pc, JL_ERR_ARG, "%s: the source is the destination itself", fn);
    if (src->device != pc->device) return jl_fail(pc, JL_ERR_ARG, "%s: the source is on device %d, the destination on %d", fn, src->device, pc->device);
    if (!src->d_msa) return jl_fail(pc, JL_ERR_STATE, "%s: the source has no resident matrix", fn);
    if (n_sites == 0 || n_sites > (uint32_t)JL_SITES_MAX) return jl_fail(pc, JL_ERR_ARG, "%s: %u sites, 1 to %d", fn, n_sites, (int)JL_SITES_MAX);
    const uint8_t max_kind = with_alleles ? (uint8_t)JL_SITE_INSERTION : (uint8_t)JL_SITE_DELETION;
    uint32_t n_ins = 0, n_plain = 0;
    for (uint32_t k = 0; k < n_sites; ++k) {
        const jl_site &s = sites[k];
        if (s.kind > max_kind)
            return jl_fail(pc, JL_ERR_ARG, with_alleles ? "%s: site %u has kind %u (0 codon, 1 deletion, 2 insertion)" : "%s: site %u has kind %u (0 codon, 1 deletion)", fn, k, s.kind);
        if (s.kind == (uint8_t)JL_SITE_INSERTION) {
            if (s.col == 0u || s.col >= src->n_cols)
                return jl_fail(pc, JL_ERR_ARG, "%s: site %u is an insertion site at junction %u, the source has junctions 1 to %u", fn, k, s.col, src->n_cols - 1u);
            if (s.fill != (uint8_t)JL_SITE_NO_FILL) return jl_fail(pc, JL_ERR_ARG, "%s: site %u is an insertion site with a fill (%u)", fn, k, s.fill);
            ++n_ins;
        } else {
            if ((uint64_t)s.col + 2u >= src->n_cols)
                return jl_fail(pc, JL_ERR_ARG, "%s: site %u at column %u, its codon ends beyond the source's %u columns", fn, k, s.col, src->n_cols);
            if (s.fill != (uint8_t)JL_SITE_NO_FILL && s.fill > 63u)
                return jl_fail(pc, JL_ERR_ARG, "%s: site %u has fill %u, neither a codon (0..63) nor 0xFF", fn, k, s.fill);
            if (s.kind == (uint8_t)JL_SITE_DELETION && s.fill != (uint8_t)JL_SITE_NO_FILL)
                return jl_fail(pc, JL_ERR_ARG, "%s: site %u is a deletion site with a fill (%u)", fn, k, s.fill);
            ++n_plain;
        }
        if (k) {
            const jl_site &q = sites[k - 1u];
            if (q.col == s.col && q.kind == s.kind) return jl_fail(pc, JL_ERR_ARG, "%s: sites %u and %u are the same (column %u, kind %u)", fn, k - 1u, k, s.col, s.kind);
            if (q.col > s.col || (q.col == s.col && q.kind > s.kind))
                return jl_fail(pc, JL_ERR_ARG, "%s: site %u (column %u, kind %u) is not in ascending order of (column, kind)", fn, k, s.col, s.kind);
        }
    }
    // the alleles: ascending as the sites are, so one walk pairs every insertion site with its run of them
    if (n_alleles > (uint32_t)JL_SITES_MAX) return jl_fail(pc, JL_ERR_ARG, "%s: %u alleles, at most %d", fn, n_alleles, (int)JL_SITES_MAX);
    std::vector<jl_ins_site> isites;
    isites.reserve(n_ins);
    uint32_t at = 0;
    for (uint32_t k = 0; k < n_sites; ++k) {
        if (sites[k].kind != (uint8_t)JL_SITE_INSERTION) continue;
        const uint32_t col = sites[k].col;
        if (at < n_alleles && alleles[at].col < col)
            return jl_fail(pc, JL_ERR_ARG, "%s: allele %u is at junction %u, which is no insertion site (or the alleles do not ascend)", fn, at, alleles[at].col);
        const uint32_t begin = at;
        while (at < n_alleles && alleles[at].col == col) ++at;
        if (at == begin) return jl_fail(pc, JL_ERR_ARG, "%s: site %u, the insertion site at junction %u, has no allele", fn, k, col);
        if (at - begin > (uint32_t)JL_SITE_INS_MAX_ALLELES)
            return jl_fail(pc, JL_ERR_ARG, "%s: site %u, the insertion site at junction %u, has %u alleles, at most %d", fn, k, col, at - begin, (int)JL_SITE_INS_MAX_ALLELES);
        isites.push_back(jl_ins_site{col, k, begin, at});
    }
    if (at < n_alleles)
        return jl_fail(pc, JL_ERR_ARG, "%s: allele %u is at junction %u, which is no insertion site (or the alleles do not ascend)", fn, at, alleles[at].col);
    for (uint32_t i = 0; i < n_alleles; ++i) {
        const jl_insertion_allele &x = alleles[i];
        if (x.len < 3u || x.len > JL_INSAL_MAX_BASES || x.len % 3u != 0u)
            return jl_fail(pc, JL_ERR_ARG, "%s: allele %u has length %u, an allele has 3, 6 .. %u bases", fn, i, x.len, JL_INSAL_MAX_BASES);
        if (x.seq >> (2u * x.len)) return jl_fail(pc, JL_ERR_ARG, "%s: allele %u has bits of its sequence set above its %u bases", fn, i, x.len);
        if (i && alleles[i - 1u].col == x.col) {
            const jl_insertion_allele &q = alleles[i - 1u];
            if (q.len > x.len || (q.len == x.len && q.seq >= x.seq))
                return jl_fail(pc, JL_ERR_ARG, "%s: allele %u is not in strictly ascending order of (column, length, sequence)", fn, i);
        }
    }
    if (n_ins && !src->insev_valid)
        return jl_fail(pc, JL_ERR_STATE, "%s: an insertion site, and the source holds no insertion events: jl_msa_track_insertion_reads(src, 1) before the record build of its matrix", fn);

    JL_HIP(pc, hipSetDevice(pc->device));
    hipStream_t st = pc->stream;
    // the tables into pinned staging (an upload of the last call may still read the staging: wait for it)
    jl_site *h_sites = nullptr;
    JL_HIP(pc, pc->sites_in.host(n_sites, &h_sites));
    for (uint32_t k = 0; k < n_sites; ++k) h_sites[k] = jl_site{sites[k].col, sites[k].kind, sites[k].fill, 0};
    if (n_ins) {
        jl_ins_site *h_isites = nullptr;
        jl_insertion_allele *h_alleles = nullptr;
        JL_HIP(pc, pc->ins_sites_in.host(n_ins, &h_isites));
        JL_HIP(pc, pc->site_alleles_in.host(n_alleles, &h_alleles));
        for (uint32_t i = 0; i < n_ins; ++i) h_isites[i] = isites[i];
        for (uint32_t i = 0; i < n_alleles; ++i) h_alleles[i] = jl_insertion_allele{alleles[i].col, alleles[i].len, alleles[i].seq, 0, 0};
    }
    if (src->stream != st) JL_HIP(pc, hipStreamSynchronize(src->stream));   // the source is complete
    // (read before the allocation: the sizes the kernels form their addresses from)
    jl_sites_args A = {};
    A.src = src->d_msa, A.src_stride = src->plane_stride;   // (a multiple of 16, >= ceil(n_reads / 8): set_shape, jl_msa_adopt)
    A.n_reads = src->n_reads;
    A.n_sites = n_sites;
    if (int rc = jl_msa_alloc(pc, A.n_reads, 3u * n_sites, 0)) return rc;
    hipError_t e = pc->sites_in.upload(st, n_sites);
    if (e == hipSuccess) {
        A.dst = pc->d_msa, A.dst_stride = pc->plane_stride;
        A.sites = pc->sites_in.dev;
        if (n_plain || !with_alleles) {
            jl_launch_sites_assemble(&A, st);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess && n_ins) e = pc->ins_sites_in.upload(st, n_ins);
    if (e == hipSuccess && n_ins) e = pc->site_alleles_in.upload(st, n_alleles);
    if (e == hipSuccess && n_ins) {
        jl_sites_ins_args I = {};
        I.src = A.src, I.src_stride = A.src_stride, I.n_reads = A.n_reads;
        I.dst = A.dst, I.dst_stride = A.dst_stride;
        I.isites = pc->ins_sites_in.dev, I.n_isites = n_ins;
        I.alleles = pc->site_alleles_in.dev;
        I.events = src->insev_rows, I.n_events = src->insev_count, I.events_cap = src->insev_cap;
        jl_launch_sites_insertions(&I, st);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return jl_fail(pc, jl_hip_status(e), "%s: %s", fn, hipGetErrorString(e));
    return JL_OK;
}

}  // namespace

extern "C" {

int jl_sites_assemble(jl_ctx *pc, jl_ctx *src, const jl_site *sites, uint32_t n_sites)
{
    return sites_assemble("jl_sites_assemble", pc, src, sites, n_sites, nullptr, 0, false);
}

int jl_sites_assemble_alleles(jl_ctx *pc, jl_ctx *src, const jl_site *sites, uint32_t n_sites, const jl_insertion_allele *alleles,
                              uint32_t n_alleles)
{
    return sites_assemble("jl_sites_assemble_alleles", pc, src, sites, n_sites, alleles, n_alleles, true);
}

}  // extern "C"
