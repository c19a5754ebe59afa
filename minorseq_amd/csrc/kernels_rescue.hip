// kernels_rescue.hip — which reported haplotype does a read agree with where it can be read (jl_phase_rescue_async; docs/SPEC.md §14).
// The walk is hap_walk.h's: one wave a workgroup, runs of 64 reads, a lane a haplotype, the mismatch word per position.  Here
//   agree_h &= ~mismatch                                              13 VALU operations per position, word and lane
// Per read the answer is bit-sliced over the agree words (the chunks of a lane one after the other, then the lanes by the ladder):
//   two |= one & agree, one |= agree; id_b |= agree & broadcast(bit b of h), ten id words, valid where one & ~two
// Combining two DISJOINT sets of haplotypes is the same rule — two = two_a | two_b | (one_a & one_b), the rest ORs.
// The 64 ids are expanded and stored, 128 bytes a run, with ordinary vector stores; hap_reads [n_hap] and tally [4] as hap_walk.h
// says.  Addresses are formed from sizes the host checked only (capi_rescue.hip); pattern bytes are data.
#include "hap_walk.h"

namespace {

using namespace jl_hap;

// what a set of haplotypes says about the 32 reads of a word
struct verdict {
    uint32_t one, two;   // some haplotype agrees / two or more do
    uint32_t id[10];     // bit b of the agreeing haplotype's number (valid where one & ~two)

    // (a lane the row mask leaves out joins nothing: every word is an OR)
    template <int CTRL, int ROW_MASK, bool BOUND>
    __device__ __forceinline__ void join_lane()
    {
        const uint32_t o = dpp<CTRL, ROW_MASK, BOUND>(one), t = dpp<CTRL, ROW_MASK, BOUND>(two);
        two |= t | (one & o);
        one |= o;
#pragma unroll
        for (uint32_t b = 0; b < 10u; ++b) id[b] |= dpp<CTRL, ROW_MASK, BOUND>(id[b]);
    }
    template <class F>
    __device__ __forceinline__ void each_word(F f)
    {
        f(one), f(two);
#pragma unroll
        for (uint32_t b = 0; b < 10u; ++b) f(id[b]);
    }
};

// the reads of the two words that agree with the lane's haplotype wherever they can be read
struct agreement : no_hooks {
    uint32_t agree[2];
    template <class Q>
    __device__ __forceinline__ void operator()(uint32_t, Q, uint32_t j, uint32_t mismatch) { agree[j] &= ~mismatch; }
};

// grid: x = one-wave workgroups, each walking the runs x, x + gridDim.x, ...
__global__ __launch_bounds__(64) void phase_rescue_kernel(jl_rescue_args a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_pos[kTilePos * kPosWords];
    __shared__ uint32_t s_hist[JL_RESCUE_HAP_PAD];
    const uint32_t lane = threadIdx.x;
    const uint32_t n_chunks = a.hap_pad / 64u;
    const table t = {(const uint8_t JL_AS1 *)a.msa, a.plane_stride, (const uint32_t JL_AS1 *)a.pos_cols, (const uint32_t JL_AS1 *)a.pat4, a.n_pos, a.hap_pad};
    clear(s_hist, JL_RESCUE_HAP_PAD, lane);
    uint32_t n_assigned = 0, n_ambiguous = 0, n_none = 0, n_uninformative = 0;   // wave-uniform

    for (uint32_t run = blockIdx.x; run < a.n_runs; run += gridDim.x) {
        verdict v[2];
#pragma unroll
        for (uint32_t j = 0; j < 2u; ++j) {
            v[j].one = v[j].two = 0u;
#pragma unroll
            for (uint32_t b = 0; b < 10u; ++b) v[j].id[b] = 0u;
        }
        uint32_t informative = 0;   // k_i of read 64 run + lane
        for (uint32_t c = 0; c < n_chunks; ++c) {
            agreement f;
            f.agree[0] = f.agree[1] = 64u * c + lane < a.n_hap ? 0xFFFFFFFFu : 0u;
            f = walk_chunk<true>(t, s_pos, run, c, lane, informative, f);
#pragma unroll
            for (uint32_t j = 0; j < 2u; ++j) {
                v[j].two |= v[j].one & f.agree[j];
                v[j].one |= f.agree[j];
#pragma unroll
                for (uint32_t b = 6; b < 10u; ++b) v[j].id[b] |= f.agree[j] & id_slice(64u * c, b);
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < 2u; ++j) {
#pragma unroll
            for (uint32_t b = 0; b < 6u; ++b) v[j].id[b] = v[j].one & id_slice(lane, b);
            ladder(v[j]);
        }
        // expand (hap_walk.h): lane l answers for read 64 run + l = bit l & 31 of word l >> 5
        const uint32_t bit = lane & 31u, hi = lane >> 5;
        const uint32_t one = ((hi ? v[1].one : v[0].one) >> bit) & 1u, two = ((hi ? v[1].two : v[0].two) >> bit) & 1u;
        uint32_t id = 0;
#pragma unroll
        for (uint32_t b = 0; b < 10u; ++b) id |= (((hi ? v[1].id[b] : v[0].id[b]) >> bit) & 1u) << b;
        const uint64_t i = 64ull * run + lane;
        const bool exists = i < a.n_reads;
        const uint32_t value = informative < a.min_positions ? (uint32_t)JL_RESCUE_UNINFORMATIVE
                               : !one                        ? (uint32_t)JL_RESCUE_NONE
                               : two                         ? (uint32_t)JL_RESCUE_AMBIGUOUS
                                                             : id;
        if (exists) {
            ((uint16_t JL_AS1 *)a.rescue)[i] = (uint16_t)value;
            if (value < a.n_hap) atomicAdd(&s_hist[value], 1u);
        }
        n_assigned += votes(exists && value < a.n_hap);
        n_ambiguous += votes(exists && value == (uint32_t)JL_RESCUE_AMBIGUOUS);
        n_none += votes(exists && value == (uint32_t)JL_RESCUE_NONE);
        n_uninformative += votes(exists && value == (uint32_t)JL_RESCUE_UNINFORMATIVE);
    }
    const uint32_t n[4] = {n_assigned, n_ambiguous, n_none, n_uninformative};
    flush(s_hist, a.n_hap, a.hap_reads, n, a.tally, lane);
}

}  // namespace

// a->hap_reads [n_hap] and a->tally [4] zeroed
void jl_launch_phase_rescue(const jl_rescue_args *a, hipStream_t st)
{
    hipLaunchKernelGGL(phase_rescue_kernel, dim3(jl_hap_walk_blocks(a->n_runs)), dim3(64), 0, st, *a);
}
