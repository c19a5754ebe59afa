// capi_take.hip — jl_msa_take of include/juliet_hip.h: a resident matrix from chosen reads of other resident matrices, and the two
// host-only rules that say WHICH reads (jl_sample_reads, jl_mix_counts; docs/SPEC.md §12).  Everything is checked here, on the
// host, before `dst` is touched: take_kernel (kernels_take.hip) forms its addresses from the indices without looking at them.
#include <math.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "jl_internal.h"

// jl_msa_take (`wait`) and jl_msa_take_async, `fn` the one that was called
static int msa_take(const char *fn, jl_ctx *dst, const jl_take_part *parts, uint32_t n_parts, bool wait)
{
    if (!dst) return JL_ERR_ARG;
    if (!parts || n_parts == 0) return jl_fail(dst, JL_ERR_ARG, "%s: no parts", fn);
    if (n_parts > (uint32_t)JL_TAKE_MAX_PARTS) return jl_fail(dst, JL_ERR_ARG, "%s: %u parts, at most %d", fn, n_parts, (int)JL_TAKE_MAX_PARTS);
    uint64_t total = 0;
    for (uint32_t p = 0; p < n_parts; ++p) {
        const jl_ctx *s = parts[p].src;
        if (!s || (parts[p].n && !parts[p].idx)) return jl_fail(dst, JL_ERR_ARG, "%s: part %u has no source or no indices", fn, p);
        if (s == dst) return jl_fail(dst, JL_ERR_ARG, "%s: part %u takes from the destination itself", fn, p);
        if (s->device != dst->device) return jl_fail(dst, JL_ERR_ARG, "%s: part %u is on device %d, the destination on %d", fn, p, s->device, dst->device);
        if (!s->d_msa) return jl_fail(dst, JL_ERR_STATE, "%s: part %u has no resident matrix", fn, p);
        if (s->n_cols != parts[0].src->n_cols || s->win_begin != parts[0].src->win_begin)
            return jl_fail(dst, JL_ERR_ARG, "%s: part %u is the window %u+%u, part 0 the window %u+%u", fn, p, s->win_begin, s->n_cols,
                           parts[0].src->win_begin, parts[0].src->n_cols);
        if (s->plane_stride > 0xFFFFFFFFull) return jl_fail(dst, JL_ERR_ARG, "%s: part %u has a plane stride of 4 GiB or more", fn, p);
        if (parts[p].n > 0x7FFFFFFFull - total) return jl_fail(dst, JL_ERR_ARG, "%s: more than 2^31-1 reads", fn);
        total += parts[p].n;
    }
    if (total == 0) return jl_fail(dst, JL_ERR_ARG, "%s: no reads chosen", fn);
    JL_HIP(dst, hipSetDevice(dst->device));
    hipStream_t st = dst->stream;
    // the indices into pinned staging, checked on the way (an upload of the last take may still read the staging: wait for it)
    uint32_t *h_idx = nullptr;
    JL_HIP(dst, dst->take_idx.host((size_t)total, &h_idx));
    jl_take_args A = {};
    uint64_t at = 0;
    for (uint32_t p = 0; p < n_parts; ++p) {
        const jl_ctx *s = parts[p].src;
        const uint32_t *idx = parts[p].idx;
        uint32_t *out = h_idx + at;
        const uint64_t n = parts[p].n, lim = s->n_reads;
        uint32_t worst = 0;
        for (uint64_t i = 0; i < n; ++i) {
            const uint32_t v = idx[i];
            out[i] = v;
            worst = std::max(worst, v);
        }
        if (n && worst >= lim) {
            uint64_t i = 0;
            while (idx[i] < lim) ++i;
            return jl_fail(dst, JL_ERR_ARG, "%s: part %u index %llu is read %u, its source has %llu reads", fn, p, (unsigned long long)i, idx[i],
                           (unsigned long long)lim);
        }
        A.part[p].base = s->d_msa;
        A.part[p].stride = (uint32_t)s->plane_stride;
        A.part[p].begin = at;
        at += n;
    }
    if (wait)   // the sources are complete
        for (uint32_t p = 0; p < n_parts; ++p)
            if (parts[p].src->stream != st) JL_HIP(dst, hipStreamSynchronize(parts[p].src->stream));
    const uint32_t n_cols = parts[0].src->n_cols;
    if (int rc = jl_msa_alloc(dst, total, n_cols, parts[0].src->win_begin)) return rc;
    hipError_t e = dst->take_idx.upload(st, (size_t)total);
    if (e == hipSuccess) {
        A.n_parts = n_parts, A.n_cols = n_cols;
        A.n_total = total;
        A.idx = dst->take_idx.dev;
        A.dst = dst->d_msa, A.dst_stride = dst->plane_stride;
        jl_launch_take(&A, st);
        e = hipGetLastError();
    }
    if (e == hipSuccess && wait) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return jl_fail(dst, jl_hip_status(e), "%s: %s", fn, hipGetErrorString(e));
    return JL_OK;
}

extern "C" {

int jl_msa_take(jl_ctx *dst, const jl_take_part *parts, uint32_t n_parts) { return msa_take("jl_msa_take", dst, parts, n_parts, true); }

int jl_msa_take_async(jl_ctx *dst, const jl_take_part *parts, uint32_t n_parts) { return msa_take("jl_msa_take_async", dst, parts, n_parts, false); }

// docs/SPEC.md §12: the k reads with the smallest (splitmix64(seed + i), i), in ascending i
int jl_sample_reads(uint64_t n_reads, uint64_t k, uint64_t seed, uint32_t *idx, uint64_t *n_out)
{
    if (!n_out || n_reads > 0xFFFFFFFFull) return JL_ERR_ARG;
    const uint64_t keep = std::min(k, n_reads);
    *n_out = keep;
    if (keep == 0) return JL_OK;
    if (!idx) return JL_ERR_ARG;
    if (keep == n_reads) {
        for (uint64_t i = 0; i < n_reads; ++i) idx[i] = (uint32_t)i;
        return JL_OK;
    }
    std::vector<std::pair<uint64_t, uint32_t>> key((size_t)n_reads);
    for (uint64_t i = 0; i < n_reads; ++i) key[(size_t)i] = {jl_splitmix64(seed + i), (uint32_t)i};
    std::nth_element(key.begin(), key.begin() + (ptrdiff_t)keep, key.end());
    for (uint64_t i = 0; i < keep; ++i) idx[i] = key[(size_t)i].second;
    std::sort(idx, idx + keep);
    return JL_OK;
}

// doc/MIXDATA.md:10-22: every minor floor(coverage * percentage / 100) reads, the major clone the rest
int jl_mix_counts(uint32_t n_sources, uint64_t coverage, double percentage, uint64_t *counts)
{
    if (!counts || n_sources == 0 || !(percentage > 0.0 && percentage < 100.0)) return JL_ERR_ARG;
    const uint64_t minor = (uint64_t)floor((double)coverage * percentage / 100.0);
    if (n_sources > 1 && minor > coverage / (n_sources - 1u)) return JL_ERR_ARG;   // (the minors alone exceed the coverage)
    counts[0] = coverage - minor * (n_sources - 1u);
    for (uint32_t m = 1; m < n_sources; ++m) counts[m] = minor;
    return JL_OK;
}

}  // extern "C"
