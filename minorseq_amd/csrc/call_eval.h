// call_eval.h — one codon position evaluated by one wavefront (lane = codon): coverage, reference / majority codon,
// error model, Fisher's exact x Bonferroni, filters, and the hand-over of the called codons.
// Shared by call_kernel (histograms read back from HBM) and by the epilogue of the pileup kernel (histogram still in
// LDS: jl_run_async / jl_group_run_async evaluate a position in the workgroup that just counted it).
// Behaviour: doc/JULIET.md:38-42, :133-134, :342-357, :370; docs/SPEC.md §4-7.
#pragma once
#include <string.h>

#include "jl_fisher.h"
#include "jl_internal.h"

__device__ __forceinline__ uint32_t jl_wave_sum_all(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ uint64_t jl_wave_max_all(uint64_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}

// One position in three stages, so that what the FP64 Fisher stage holds in registers is a handful of words and a kernel that runs
// it as an epilogue (pileup_tail) is not allocated the sum of the three:
//   screen   coverage, reference / majority codon, expected count, and every filter that needs no p-value;
//   fisher   the p-value of a lane that passed the screen;
//   store    the call mask and the finished 48-byte rows; gene and codon come from the caller here, not before.
// Every expression is evaluated as before and in the same order: p-values, log_p and the call bits are bit for bit the same.
struct jl_call_screened {
    uint32_t cov;     // coverage (wave-uniform)
    uint32_t ref;     // reference codon, or JL_REF_SKIP and above: no calls at this position (wave-uniform)
    uint32_t e;       // this lane's expected count
    bool candidate;   // this lane's codon can still be called: only such a lane needs its p-value
};

// h = this lane's bin of the position's histogram.
__device__ __forceinline__ jl_call_screened jl_call_screen(const jl_call_args &A, uint32_t p, uint32_t h, uint32_t refcfg,
                                                           const uint64_t *drm)
{
    const uint32_t lane = threadIdx.x & 63u;
    jl_call_screened s;
    // (both are the same in every lane after the butterflies: kept in scalar registers across the Fisher stage)
    s.cov = (uint32_t)__builtin_amdgcn_readfirstlane((int)jl_wave_sum_all(h));
    uint32_t ref = refcfg;
    if (ref == JL_REF_MAJORITY) {
        // argmax, lowest codon index on ties (SPEC §4)
        const uint64_t key = ((uint64_t)h << 8) | (uint64_t)(63u - lane);
        const uint64_t best = jl_wave_max_all(key);
        ref = s.cov ? 63u - (uint32_t)(best & 0xFFu) : JL_REF_SKIP;
    }
    s.ref = (uint32_t)__builtin_amdgcn_readfirstlane((int)ref);
    s.e = 0;
    s.candidate = false;
    if (s.ref < 64u && h > 0 && lane != s.ref) {
        double perr = 1.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int sh = 4 - 2 * i;
            perr = perr * ((((s.ref >> sh) & 3u) == ((lane >> sh) & 3u)) ? A.match : A.substitution);
        }
        const double x = (double)s.cov * perr;
        double r = A.expected_round == 1 ? floor(x) : (A.expected_round == 2 ? floor(x + 0.5) : ceil(x));
        if (r < 0.0) r = 0.0;
        if (r > (double)s.cov) r = (double)s.cov;
        s.e = (uint32_t)r;
        s.candidate = true;
        if (A.tail == 0) {
            // An observed count at or below the expected one has p >= 1/2 (the null is symmetric about K/2
            // because both rows sum to the coverage), so it cannot be called once min(1, n_tests/2) >= alpha;
            // uncalled codons are never reported, so their p-value is not needed.
            const double floor_adj = 0.5 * A.n_tests < 1.0 ? 0.5 * A.n_tests : 1.0;
            s.candidate = h > s.e || !(floor_adj >= A.alpha);
        }
        // the filters that only ever take a call away: a lane they stop needs no p-value either
        const double perc = 100.0 * (double)h / (double)s.cov;
        if (A.min_perc >= 0.0 && !(perc > A.min_perc)) s.candidate = false;
        if (A.max_perc >= 0.0 && !(perc < A.max_perc)) s.candidate = false;
        if (drm && !((drm[p] >> lane) & 1ull)) s.candidate = false;
    }
    return s;
}

// a candidate lane's adjusted p-value and ln p; returns whether its codon is called
__device__ __forceinline__ bool jl_call_fisher(const jl_call_args &A, const jl_call_screened &s, uint32_t h, double *p_adj, double *lp)
{
    if (A.tail == 0) {
        bool skipped;
        const double pv = jl_fisher_greater_equal_rows_or_skip(h, s.e, s.cov, A.n_tests, A.alpha, lp, &skipped);
        double pa = pv * A.n_tests;
        if (pa > 1.0) pa = 1.0;
        *p_adj = pa;
        return !skipped && pa < A.alpha;
    }
    const double pv = jl_fisher_two_sided_equal_rows(h, s.e, s.cov, lp);
    double pa = pv * A.n_tests;
    if (pa > 1.0) pa = 1.0;
    *p_adj = pa;
    return pa < A.alpha;
}

// the position's call mask (lane 0)
template <bool COHERENT>
__device__ __forceinline__ void jl_call_store_mask(uint32_t p, uint64_t mask, uint64_t *called)
{
    if ((threadIdx.x & 63u) == 0) {
        if (COHERENT) __hip_atomic_store(&called[p], mask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else called[p] = mask;
    }
}

// a called lane's finished 48-byte row to the staging area [p][codon]
template <bool COHERENT>
__device__ __forceinline__ void jl_call_store_row(uint32_t p, uint32_t col, uint32_t h, const jl_call_screened &s, double p_adj, double lp,
                                                  uint32_t gene, uint32_t codon_pos, jl_variant *staged)
{
    const uint32_t lane = threadIdx.x & 63u;
    jl_variant v;
    v.gene = gene;
    v.codon_pos = codon_pos;
    v.col = col;
    v.ref_codon = (uint8_t)s.ref;
    v.codon = (uint8_t)lane;
    v.flags = 0;
    v.count = h;
    v.coverage = s.cov;
    v.expected = s.e;
    v.pad_ = 0;
    v.p_value = p_adj;
    v.log_p = lp;
    uint64_t w[6];
    memcpy(w, &v, sizeof v);
    uint64_t *dst = reinterpret_cast<uint64_t *>(staged + (uint64_t)p * 64u + lane);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        if (COHERENT) __hip_atomic_store(dst + k, w[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else dst[k] = w[k];
    }
}

// The three stages for one position.  Writes the position's call mask and the rows of its called codons.  `row_source()` gives the
// position's {gene, codon}: it is asked behind the Fisher stage and by the called lanes only.  A wave none of whose lanes passed
// the screen writes an empty mask and leaves (a wave-uniform branch).  COHERENT: the consumer is another workgroup of the SAME
// launch (call_kernel's last block), so the stores are write-through (agent scope); otherwise plain stores (the consumer is the
// next kernel on the stream).
template <bool COHERENT, class RowSource>
__device__ __forceinline__ void jl_call_position_staged(const jl_call_args &A, uint32_t p, uint32_t col, uint32_t h, uint32_t refcfg,
                                                        RowSource row_source, const uint64_t *drm, uint64_t *called, jl_variant *staged)
{
    const jl_call_screened s = jl_call_screen(A, p, h, refcfg, drm);
    if (__ballot(s.candidate) == 0ull) {
        jl_call_store_mask<COHERENT>(p, 0ull, called);
        return;
    }
    bool is_called = false;
    double p_adj = 1.0, lp = 0.0;
    if (s.candidate) is_called = jl_call_fisher(A, s, h, &p_adj, &lp);
    jl_call_store_mask<COHERENT>(p, __ballot(is_called), called);
    if (is_called) {
        const uint2 gc = row_source();
        jl_call_store_row<COHERENT>(p, col, h, s, p_adj, lp, gc.x, gc.y, staged);
    }
}

// ... with the position's gene and codon already in registers (call_kernel)
template <bool COHERENT>
__device__ __forceinline__ void jl_call_position(const jl_call_args &A, uint32_t p, uint32_t col, uint32_t h, uint32_t refcfg,
                                                 uint32_t gene, uint32_t codon_pos, const uint64_t *drm, uint64_t *called,
                                                 jl_variant *staged)
{
    jl_call_position_staged<COHERENT>(A, p, col, h, refcfg, [=]() { return make_uint2(gene, codon_pos); }, drm, called, staged);
}

// ... and with the two read from the position tables when a row needs them (the folded epilogue: nothing of a row is live across
// the Fisher stage)
template <bool COHERENT>
__device__ __forceinline__ void jl_call_position_at(const jl_call_args &A, uint32_t p, uint32_t col, uint32_t h, uint32_t refcfg,
                                                    const uint32_t *pos_gene, const uint32_t *pos_codon, const uint64_t *drm,
                                                    uint64_t *called, jl_variant *staged)
{
    jl_call_position_staged<COHERENT>(A, p, col, h, refcfg, [=]() { return make_uint2(pos_gene[p], pos_codon[p]); }, drm, called, staged);
}

// Ordered compaction of the staged rows into the fixed-stride table: positions are laid out in (gene, codon) order
// (SPEC §6), so rows in (position, codon index) order are the table.  Call with all 256 threads of a block; `s_scan`
// [4] and `s_running` [1] are LDS words of the caller.  COHERENT as above (masks and rows written by other
// workgroups of this launch are read past the L1).  `lds_cols` (optional, [n_lds]) receives the columns of the first
// rows.  Returns the number of rows needed (may exceed cap; only the first cap are written).
template <bool COHERENT>
__device__ __forceinline__ uint32_t jl_compact_rows_block(uint32_t P, const uint64_t *called, const jl_variant *staged,
                                                          jl_variant *rows, uint32_t cap, uint32_t *s_scan,
                                                          uint32_t *s_running, uint32_t *lds_cols, uint32_t n_lds,
                                                          bool rows_coherent)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    if (tid == 0) *s_running = 0;
    __syncthreads();
    constexpr uint32_t kPer = 8;  // consecutive positions per thread and pass
    for (uint32_t base = 0; base < P; base += 256u * kPer) {
        uint64_t m[kPer];
        uint32_t c = 0;
#pragma unroll
        for (uint32_t k = 0; k < kPer; ++k) {
            const uint32_t q = base + tid * kPer + k;
            m[k] = 0ull;
            if (q < P) m[k] = COHERENT ? __hip_atomic_load(&called[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : called[q];
        }
#pragma unroll
        for (uint32_t k = 0; k < kPer; ++k) c += (uint32_t)__popcll(m[k]);
        uint32_t inc = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(inc, o, 64);
            if ((int)lane >= o) inc += u;
        }
        if (lane == 63) s_scan[wid] = inc;
        __syncthreads();
        uint32_t wave_off = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t v = s_scan[w];
            if (w < (int)wid) wave_off += v;
            total += v;
        }
        uint32_t o = *s_running + wave_off + inc - c;
#pragma unroll
        for (uint32_t k = 0; k < kPer; ++k) {
            uint64_t mk = m[k];
            const uint32_t q = base + tid * kPer + k;
            while (mk) {
                const uint32_t j = (uint32_t)__ffsll((unsigned long long)mk) - 1u;
                mk &= mk - 1ull;
                if (o < cap) {
                    const uint64_t *src = reinterpret_cast<const uint64_t *>(staged + (uint64_t)q * 64u + j);
                    uint64_t w[6];
#pragma unroll
                    for (int i = 0; i < 6; ++i)
                        w[i] = COHERENT ? __hip_atomic_load(src + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : src[i];
                    uint64_t *dst = reinterpret_cast<uint64_t *>(rows + o);
#pragma unroll
                    for (int i = 0; i < 6; ++i) {
                        if (rows_coherent) __hip_atomic_store(dst + i, w[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        else dst[i] = w[i];
                    }
                    if (lds_cols && o < n_lds) lds_cols[o] = (uint32_t)(w[1] & 0xFFFFFFFFull);  // jl_variant.col
                }
                ++o;
            }
        }
        __syncthreads();
        if (tid == 0) *s_running += total;
        __syncthreads();
    }
    return *s_running;
}
