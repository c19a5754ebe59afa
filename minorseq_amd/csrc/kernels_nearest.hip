// kernels_nearest.hip — which reported haplotype is a read nearest to, within a mismatch budget (jl_phase_nearest_async;
// docs/SPEC.md §22).  The walk is hap_walk.h's: one wave a workgroup, runs of 64 reads, a lane a haplotype, the mismatch word
// per position.  What is this kernel's own is the distance.  Where the rescue clears a bit of `agree`, this adds `mismatch` to a
// BIT-SLICED COUNTER, four words s[0..3] a read word: bit i of s[k] is bit k of read i's count.  The add is a ripple of half
// adders into the three low slices; the carry out of them is ORed into s[3], never XORed: the top slice is sticky, a read that
// differs at 8, 16 or 130 positions keeps it set and never wraps back into the budget.  After a chunk's positions the low slices
// take s[3] in: a count of 8 or more reads 15, the SATURATED distance, which no budget (D <= 7) admits.  19 VALU operations per
// position, word and lane (the mismatch word's 11, the AND with known, 7 for the add) where the rescue has 13.
// Per read the answer is hap_walk.h's sliced_verdict over the SMALLEST distance, four slices.  A haplotype slot h >= n_hap enters
// saturated; the empty set is {15, no tie}.  A tie flagged among saturated distances is no error: the comparison with D comes once
// per read, after the expansion, and any best above D is JL_RESCUE_NONE whatever tie and id say.
// hap_reads [n_hap][D + 1] goes through an LDS histogram of the same shape (at most 704 x 8 words, sized by the launch); nearest
// and dist leave by ordinary vector stores.  Addresses are formed from sizes the host checked only (capi_nearest.hip); pattern
// bytes are data.
#include "hap_walk.h"

namespace {

using namespace jl_hap;

typedef sliced_verdict<4, false> verdict;   // best: the smallest distance in the set (15: saturated, or nobody)

// the distance of the lane's haplotype to the reads of the two words, sliced
struct distance : no_hooks {
    uint32_t s[2][4];
    // count += mismatch, saturating: the carry out of the low three slices sticks in the top one
    template <class Q>
    __device__ __forceinline__ void operator()(uint32_t, Q, uint32_t j, uint32_t mismatch)
    {
        uint32_t carry = mismatch;
#pragma unroll
        for (uint32_t k = 0; k < 3u; ++k) {
            const uint32_t up = s[j][k] & carry;
            s[j][k] ^= carry;
            carry = up;
        }
        s[j][3] |= carry;
    }
};

// grid: x = one-wave workgroups, each walking the runs x, x + gridDim.x, ...; dynamic LDS: n_hap (D + 1) words of histogram
__global__ __launch_bounds__(64) void phase_nearest_kernel(jl_nearest_args a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_pos[kTilePos * kPosWords];
    extern __shared__ uint32_t s_hist[];   // [n_hap][D + 1]
    const uint32_t lane = threadIdx.x;
    const uint32_t n_chunks = a.hap_pad / 64u;
    const uint32_t row = a.max_distance + 1u, n_hist = a.n_hap * row;
    const table t = {(const uint8_t JL_AS1 *)a.msa, a.plane_stride, (const uint32_t JL_AS1 *)a.pos_cols, (const uint32_t JL_AS1 *)a.pat4, a.n_pos, a.hap_pad};
    clear(s_hist, n_hist, lane);
    uint32_t n_assigned = 0, n_ambiguous = 0, n_none = 0, n_uninformative = 0;   // wave-uniform

    for (uint32_t run = blockIdx.x; run < a.n_runs; run += gridDim.x) {
        verdict v[2];
        v[0].empty_set();
        v[1].empty_set();
        uint32_t informative = 0;   // k_i of read 64 run + lane
        for (uint32_t c = 0; c < n_chunks; ++c) {
            distance f;
#pragma unroll
            for (uint32_t j = 0; j < 2u; ++j)
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k) f.s[j][k] = 0u;
            f = walk_chunk<true>(t, s_pos, run, c, lane, informative, f);
            // the chunk's set: one haplotype a lane, at its distance (8 and more: 15; a slot beyond the last haplotype: 15)
            const uint32_t absent = 64u * c + lane < a.n_hap ? 0u : 0xFFFFFFFFu;
#pragma unroll
            for (uint32_t j = 0; j < 2u; ++j) {
                verdict one;
                one.empty_set();
                one.best[3] = f.s[j][3] | absent;
#pragma unroll
                for (uint32_t k = 0; k < 3u; ++k) one.best[k] = f.s[j][k] | one.best[3];
#pragma unroll
                for (uint32_t b = 6; b < 10u; ++b) one.id[b] = id_slice(64u * c, b);
                v[j].join(one);
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < 2u; ++j) {
#pragma unroll
            for (uint32_t b = 0; b < 6u; ++b) v[j].id[b] = id_slice(lane, b);
            ladder(v[j]);
        }
        // expand (hap_walk.h): lane l answers for read 64 run + l = bit l & 31 of word l >> 5
        const uint32_t bit = lane & 31u, hi = lane >> 5;
        uint32_t dmin = 0, id = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) dmin |= (((hi ? v[1].best[k] : v[0].best[k]) >> bit) & 1u) << k;
#pragma unroll
        for (uint32_t b = 0; b < 10u; ++b) id |= (((hi ? v[1].id[b] : v[0].id[b]) >> bit) & 1u) << b;
        const uint32_t tie = ((hi ? v[1].tie : v[0].tie) >> bit) & 1u;
        const uint64_t i = 64ull * run + lane;
        const bool exists = i < a.n_reads;
        const uint32_t value = informative < a.min_positions ? (uint32_t)JL_RESCUE_UNINFORMATIVE
                               : dmin > a.max_distance       ? (uint32_t)JL_RESCUE_NONE
                               : tie                         ? (uint32_t)JL_RESCUE_AMBIGUOUS
                                                             : id;
        const uint32_t d = informative < a.min_positions ? 0xFFu : min(dmin, row);
        const bool assigned = exists && value < a.n_hap;   // (then d <= D: the histogram's cell exists)
        if (exists) {
            ((uint16_t JL_AS1 *)a.nearest)[i] = (uint16_t)value;
            ((uint8_t JL_AS1 *)a.dist)[i] = (uint8_t)d;
        }
        if (assigned) atomicAdd(&s_hist[value * row + d], 1u);
        n_assigned += votes(assigned);
        n_ambiguous += votes(exists && value == (uint32_t)JL_RESCUE_AMBIGUOUS);
        n_none += votes(exists && value == (uint32_t)JL_RESCUE_NONE);
        n_uninformative += votes(exists && value == (uint32_t)JL_RESCUE_UNINFORMATIVE);
    }
    const uint32_t n[4] = {n_assigned, n_ambiguous, n_none, n_uninformative};
    flush(s_hist, n_hist, a.hap_reads, n, a.tally, lane);
}

}  // namespace

// a->hap_reads [n_hap][D + 1] and a->tally [4] zeroed
void jl_launch_phase_nearest(const jl_nearest_args *a, hipStream_t st)
{
    const size_t hist_bytes = (size_t)a->n_hap * (a->max_distance + 1u) * sizeof(uint32_t);   // <= JL_NEAREST_HIST_WORDS words: 22 KiB
    hipLaunchKernelGGL(phase_nearest_kernel, dim3(jl_hap_walk_blocks(a->n_runs)), dim3(64), hist_bytes, st, *a);
}
