// kernels_nearest.hip — which reported haplotype is a read nearest to, within a mismatch budget (jl_phase_nearest_async;
// docs/SPEC.md §22).  The shape is kernels_rescue.hip's: a workgroup is ONE wave, it owns runs of 64 reads (two words, 8 bytes of
// every plane row), a lane owns a HAPLOTYPE, 64 of them a chunk; the positions stream in tiles of 64 through LDS, the pattern
// travels packed, four positions a dword (pat4 of jl_rescue_args).  Per word of 32 reads and position p
//   mismatch = OR_b (w[b] ^ broadcast(bit b of pattern[h][p])) & known          the reads that can be read there and differ
// What is new is the distance.  Where the rescue clears a bit of `agree`, this adds `mismatch` to a BIT-SLICED COUNTER, four
// words s[0..3] a read word: bit i of s[k] is bit k of read i's count.  The add is a ripple of half adders into the three low
// slices; the carry out of them is ORed into s[3], never XORed: the top slice is sticky, a read that differs at 8, 16 or 130
// positions keeps it set and never wraps back into the budget.  After a chunk's positions the low slices take s[3] in: a count
// of 8 or more reads 15, the SATURATED distance, which no budget (D <= 7) admits.  19 VALU operations per position, word and lane
// (the mismatch word's 11, the AND with known, 7 for the add) where the rescue has 13.
// Per read the answer is bit-sliced too: what a SET of haplotypes says of the 32 reads of a word is
//   best[4] the smallest distance in the set, tie: two or more of the set are at it, id[10]: the number of the one at it
// and two DISJOINT sets are joined by comparing best slice by slice from the top:
//   lt = best_a < best_b, eq = best_a == best_b;  best = lt ? a : b;  tie = lt ? tie_a : eq ? all : tie_b;  id = lt ? id_a : id_b
// (where eq, id is the id of neither: tie says so).  The join is associative and commutative in best and tie, and in id
// wherever tie is clear; the same function joins a lane's chunks one after the other and the lanes by the DPP ladder of
// kernels_rescue.hip, whose total lands in lane 63.  A haplotype slot h >= n_hap enters saturated; the empty set is
// {15, no tie}.  A tie flagged among saturated distances is no error: the comparison with D comes once per read, after the
// expansion, and any best above D is JL_RESCUE_NONE whatever tie and id say.
// hap_reads [n_hap][D + 1] goes through an LDS histogram of the same shape (at most 704 x 8 words, sized by the launch), tally
// through ballots; both reach the zeroed outputs as integer atomics: exact, independent of launch shape and order.  nearest and
// dist leave by ordinary vector stores.  Garbage past the last read of a plane row touches bits no lane reports.  Addresses
// are formed from sizes the host checked only (capi_nearest.hip); pattern bytes are data.
#include "jl_internal.h"

namespace {

constexpr uint32_t kTilePos = 64;     // positions a tile stages: one per lane
constexpr uint32_t kPosWords = 16;    // a staged position in LDS: known[2], w[6][2], 2 of padding

template <int CTRL, int ROW_MASK, bool BOUND>
__device__ __forceinline__ uint32_t dpp(uint32_t old, uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, ROW_MASK, 0xF, BOUND);
}

// what a set of haplotypes says about the 32 reads of a word
struct verdict {
    uint32_t best[4];    // slice k: bit k of the smallest distance in the set (15: saturated, or nobody)
    uint32_t tie;        // two or more of the set are at it
    uint32_t id[10];     // bit b of the number of the haplotype at it (valid where ~tie)
};

__device__ __forceinline__ void empty_set(verdict &v)
{
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) v.best[k] = 0xFFFFFFFFu;
    v.tie = 0u;
#pragma unroll
    for (uint32_t b = 0; b < 10u; ++b) v.id[b] = 0u;
}

// a joined with the (disjoint) set b
__device__ __forceinline__ void join(verdict &a, const verdict &b)
{
    uint32_t lt = 0u, eq = 0xFFFFFFFFu;
#pragma unroll
    for (int k = 3; k >= 0; --k) {
        lt |= eq & ~a.best[k] & b.best[k];
        eq &= ~(a.best[k] ^ b.best[k]);
    }
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) a.best[k] = (a.best[k] & lt) | (b.best[k] & ~lt);
    a.tie = (a.tie & lt) | eq | (b.tie & ~lt);
#pragma unroll
    for (uint32_t k = 0; k < 10u; ++k) a.id[k] = (a.id[k] & lt) | (b.id[k] & ~lt);
}

// this lane's set joined with the set of the lane the DPP control names; a lane the row mask leaves out joins the empty set
template <int CTRL, int ROW_MASK, bool BOUND>
__device__ __forceinline__ void join_lane(verdict &v)
{
    verdict o;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) o.best[k] = dpp<CTRL, ROW_MASK, BOUND>(0xFFFFFFFFu, v.best[k]);
    o.tie = dpp<CTRL, ROW_MASK, BOUND>(0u, v.tie);
#pragma unroll
    for (uint32_t b = 0; b < 10u; ++b) o.id[b] = dpp<CTRL, ROW_MASK, BOUND>(0u, v.id[b]);
    join(v, o);
}

// all 64 lanes' sets joined: the result is lane 63's, handed to every lane
__device__ __forceinline__ void join_wave(verdict &v)
{
    join_lane<0xB1, 0xF, true>(v);     // quad_perm [1,0,3,2]
    join_lane<0x4E, 0xF, true>(v);     // quad_perm [2,3,0,1]
    join_lane<0x141, 0xF, true>(v);    // row_half_mirror
    join_lane<0x140, 0xF, true>(v);    // row_mirror
    join_lane<0x142, 0xA, false>(v);   // row_bcast:15 -> rows 1, 3
    join_lane<0x143, 0xC, false>(v);   // row_bcast:31 -> rows 2, 3
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) v.best[k] = (uint32_t)__builtin_amdgcn_readlane((int)v.best[k], 63);
    v.tie = (uint32_t)__builtin_amdgcn_readlane((int)v.tie, 63);
#pragma unroll
    for (uint32_t b = 0; b < 10u; ++b) v.id[b] = (uint32_t)__builtin_amdgcn_readlane((int)v.id[b], 63);
}

// grid: x = one-wave workgroups, each walking the runs x, x + gridDim.x, ...; dynamic LDS: n_hap (D + 1) words of histogram
__global__ __launch_bounds__(64) void phase_nearest_kernel(jl_nearest_args a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_pos[kTilePos * kPosWords];
    extern __shared__ uint32_t s_hist[];   // [n_hap][D + 1]
    const uint32_t lane = threadIdx.x;
    const uint32_t n_chunks = a.hap_pad / 64u;
    const uint32_t row = a.max_distance + 1u, n_hist = a.n_hap * row;
    const uint8_t JL_AS1 *msa = (const uint8_t JL_AS1 *)a.msa;
    const uint32_t JL_AS1 *pos_cols = (const uint32_t JL_AS1 *)a.pos_cols;
    const uint32_t JL_AS1 *pat4 = (const uint32_t JL_AS1 *)a.pat4;
    for (uint32_t k = lane; k < n_hist; k += 64u) s_hist[k] = 0u;
    uint32_t n_assigned = 0, n_ambiguous = 0, n_none = 0, n_uninformative = 0;   // wave-uniform

    for (uint32_t run = blockIdx.x; run < a.n_runs; run += gridDim.x) {
        verdict v[2];
        empty_set(v[0]);
        empty_set(v[1]);
        uint32_t informative = 0;   // k_i of read 64 run + lane
        for (uint32_t c = 0; c < n_chunks; ++c) {
            const uint32_t h = 64u * c + lane;
            uint32_t s[2][4];       // the distance of the lane's haplotype to the reads of the two words, sliced
#pragma unroll
            for (uint32_t j = 0; j < 2u; ++j)
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k) s[j][k] = 0u;
            for (uint32_t p0 = 0; p0 < a.n_pos; p0 += kTilePos) {
                // stage: lane l brings position p0 + l; a position beyond the last is open to every read
                uint32_t st[14];
#pragma unroll
                for (uint32_t q = 0; q < 14u; ++q) st[q] = 0u;
                if (p0 + lane < a.n_pos) {
                    const uint8_t JL_AS1 *rows = msa + 3ull * pos_cols[p0 + lane] * a.plane_stride + 8ull * run;
                    uint2 r[9];
#pragma unroll
                    for (uint32_t q = 0; q < 9u; ++q) r[q] = *(const uint2 JL_AS1 *)(rows + (uint64_t)q * a.plane_stride);
                    st[0] = ~(r[2].x | r[5].x | r[8].x), st[1] = ~(r[2].y | r[5].y | r[8].y);
                    // row 3 k + b = plane b of column k; codon bits 0, 1 = planes 0, 1 of column 2; 2, 3 of column 1; 4, 5 of column 0
                    st[2] = r[6].x, st[3] = r[6].y, st[4] = r[7].x, st[5] = r[7].y;
                    st[6] = r[3].x, st[7] = r[3].y, st[8] = r[4].x, st[9] = r[4].y;
                    st[10] = r[0].x, st[11] = r[0].y, st[12] = r[1].x, st[13] = r[1].y;
                }
                __syncthreads();   // the last tile has been read
#pragma unroll
                for (uint32_t q = 0; q < 14u; ++q) s_pos[lane * kPosWords + q] = st[q];
                __syncthreads();
                const uint32_t tile_n = min(kTilePos, a.n_pos - p0);
                if (c == 0u) {     // a lane owns a read here: its bit of `known` at every position of the tile
                    for (uint32_t q = 0; q < tile_n; ++q) informative += (s_pos[q * kPosWords + (lane >> 5)] >> (lane & 31u)) & 1u;
                }
                const uint32_t JL_AS1 *pat = pat4 + (uint64_t)(p0 / 4u) * a.hap_pad + h;
                for (uint32_t g = 0; 4u * g < tile_n; ++g) {
                    const uint32_t four = pat[(uint64_t)g * a.hap_pad];
#pragma unroll
                    for (uint32_t q = 0; q < 4u; ++q) {   // (a position beyond the tile's last: known = 0, nothing is added)
                        const uint32_t *sp = s_pos + (4u * g + q) * kPosWords;
                        uint32_t m[6];
#pragma unroll
                        for (uint32_t b = 0; b < 6u; ++b) m[b] = 0u - ((four >> (8u * q + b)) & 1u);
#pragma unroll
                        for (uint32_t j = 0; j < 2u; ++j) {
                            uint32_t mismatch = 0u;
#pragma unroll
                            for (uint32_t b = 0; b < 6u; ++b) mismatch |= sp[2u + 2u * b + j] ^ m[b];
                            // count += mismatch & known, saturating: the carry out of the low three slices sticks in the top one
                            uint32_t carry = mismatch & sp[j];
#pragma unroll
                            for (uint32_t k = 0; k < 3u; ++k) {
                                const uint32_t up = s[j][k] & carry;
                                s[j][k] ^= carry;
                                carry = up;
                            }
                            s[j][3] |= carry;
                        }
                    }
                }
            }
            // the chunk's set: one haplotype a lane, at its distance (8 and more: 15; a slot beyond the last haplotype: 15), the high
            // bits of its number the chunk's (wave-uniform), the low bits the lane's (set below, once)
            const uint32_t absent = h < a.n_hap ? 0u : 0xFFFFFFFFu;
#pragma unroll
            for (uint32_t j = 0; j < 2u; ++j) {
                verdict one;
                one.best[3] = s[j][3] | absent;
#pragma unroll
                for (uint32_t k = 0; k < 3u; ++k) one.best[k] = s[j][k] | one.best[3];
                one.tie = 0u;
#pragma unroll
                for (uint32_t b = 0; b < 6u; ++b) one.id[b] = 0u;
#pragma unroll
                for (uint32_t b = 6; b < 10u; ++b) one.id[b] = 0u - ((c >> (b - 6u)) & 1u);
                join(v[j], one);
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < 2u; ++j) {
#pragma unroll
            for (uint32_t b = 0; b < 6u; ++b) v[j].id[b] = 0u - ((lane >> b) & 1u);   // the low bits of h are the lane's
            join_wave(v[j]);
        }
        // expand: lane l answers for read 64 run + l = bit l & 31 of word l >> 5
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
        n_assigned += (uint32_t)__popcll(__ballot(assigned));
        n_ambiguous += (uint32_t)__popcll(__ballot(exists && value == (uint32_t)JL_RESCUE_AMBIGUOUS));
        n_none += (uint32_t)__popcll(__ballot(exists && value == (uint32_t)JL_RESCUE_NONE));
        n_uninformative += (uint32_t)__popcll(__ballot(exists && value == (uint32_t)JL_RESCUE_UNINFORMATIVE));
    }

    __syncthreads();
    for (uint32_t k = lane; k < n_hist; k += 64u)
        if (s_hist[k]) atomicAdd(a.hap_reads + k, s_hist[k]);
    if (lane == 0u) {
        if (n_assigned) atomicAdd(a.tally + 0, (unsigned long long)n_assigned);
        if (n_ambiguous) atomicAdd(a.tally + 1, (unsigned long long)n_ambiguous);
        if (n_none) atomicAdd(a.tally + 2, (unsigned long long)n_none);
        if (n_uninformative) atomicAdd(a.tally + 3, (unsigned long long)n_uninformative);
    }
}

}  // namespace

// a->hap_reads [n_hap][D + 1] and a->tally [4] zeroed; the runs shared out over at most a few waves per SIMD
void jl_launch_phase_nearest(const jl_nearest_args *a, hipStream_t st)
{
    const uint32_t blocks = std::min(a->n_runs, 4096u);
    const size_t hist_bytes = (size_t)a->n_hap * (a->max_distance + 1u) * sizeof(uint32_t);   // <= JL_NEAREST_HIST_WORDS words: 22 KiB
    hipLaunchKernelGGL(phase_nearest_kernel, dim3(blocks), dim3(64), hist_bytes, st, *a);
}
