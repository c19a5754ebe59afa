// kernels_rescue.hip — which reported haplotype does a read agree with where it can be read (jl_phase_rescue_async; docs/SPEC.md §14).
// Bit-parallel on the planes: a read is one bit position in every plane row, A C G T <=> plane 2 clear, planes 1 and 0 the two
// bits of a base.  Per word of 32 reads and variant position p (a codon: three columns, nine plane rows)
//   known    = ~(plane 2 of the three columns)                       the reads whose codon is A C G T throughout
//   w[b]     = planes 1, 0 of the three columns                      the six bit-words of the codon, b = 5 .. 0
//   agree_h &= ~(OR_b (w[b] ^ broadcast(bit b of pattern[h][p])) & known)
// Shape.  A workgroup is ONE wave; it owns runs of 64 reads (two words, 8 bytes of every plane row) and a lane owns a
// HAPLOTYPE, 64 of them a chunk (ceil(H / 64) <= 11 chunks).  Per chunk the positions stream in tiles of 64: lane l fetches the
// nine 8-byte row pieces of position p0 + l — 64 positions in flight at once, no serial chain of dependent loads — and leaves
// `known` and the six codon words in LDS, where the inner loop reads them at a wave-uniform address (a broadcast).  The pattern
// travels transposed and packed by the host, four positions a dword, [ceil(Vp / 4)][64 chunks'] dwords: a coalesced load per lane
// and four positions.  13 VALU operations per position, word and lane + 6 per position for the broadcast masks.
// Per read the answer is bit-sliced over the agree words (the chunks of a lane one after the other, then the lanes by DPP):
//   two |= one & agree, one |= agree; id_b |= agree & broadcast(bit b of h), ten id words, valid where one & ~two
// Combining two DISJOINT sets of haplotypes is the same rule — two = two_a | two_b | (one_a & one_b), the rest ORs — which is what
// every step of the DPP ladder of kernels_pileup.hip's wave_sum does: the total lands in lane 63.  The informative positions
// of a read (k_i of §14) are counted while chunk 0 streams, a lane owning a READ there; so it does when the 64 ids are expanded
// and stored, 128 bytes a run, with ordinary vector stores.  hap_reads goes through an LDS histogram, tally through ballots;
// both reach the zeroed outputs as integer atomics: exact, independent of launch shape and order.
// Garbage past the last read of a plane row touches bits no lane reports: a read is its own bit position and nothing crosses
// between them.  Addresses are formed from sizes the host checked only (capi_rescue.hip); pattern bytes are data.
#include "jl_internal.h"

namespace {

constexpr uint32_t kTilePos = 64;     // positions a tile stages: one per lane
constexpr uint32_t kPosWords = 16;    // a staged position in LDS: known[2], w[6][2], 2 of padding

template <int CTRL, int ROW_MASK, bool BOUND>
__device__ __forceinline__ uint32_t dpp(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, BOUND);
}

// what a set of haplotypes says about the 32 reads of a word
struct verdict {
    uint32_t one, two;   // some haplotype agrees / two or more do
    uint32_t id[10];     // bit b of the agreeing haplotype's number (valid where one & ~two)
};

// this lane's set joined with the (disjoint) set of the lane the DPP control names; a lane the row mask leaves out joins nothing
template <int CTRL, int ROW_MASK, bool BOUND>
__device__ __forceinline__ void join(verdict &v)
{
    const uint32_t o = dpp<CTRL, ROW_MASK, BOUND>(v.one), t = dpp<CTRL, ROW_MASK, BOUND>(v.two);
    v.two |= t | (v.one & o);
    v.one |= o;
#pragma unroll
    for (uint32_t b = 0; b < 10u; ++b) v.id[b] |= dpp<CTRL, ROW_MASK, BOUND>(v.id[b]);
}

// all 64 lanes' sets joined: the result is lane 63's, handed to every lane
__device__ __forceinline__ void join_wave(verdict &v)
{
    join<0xB1, 0xF, true>(v);     // quad_perm [1,0,3,2]
    join<0x4E, 0xF, true>(v);     // quad_perm [2,3,0,1]
    join<0x141, 0xF, true>(v);    // row_half_mirror
    join<0x140, 0xF, true>(v);    // row_mirror
    join<0x142, 0xA, false>(v);   // row_bcast:15 -> rows 1, 3
    join<0x143, 0xC, false>(v);   // row_bcast:31 -> rows 2, 3
    v.one = (uint32_t)__builtin_amdgcn_readlane((int)v.one, 63);
    v.two = (uint32_t)__builtin_amdgcn_readlane((int)v.two, 63);
#pragma unroll
    for (uint32_t b = 0; b < 10u; ++b) v.id[b] = (uint32_t)__builtin_amdgcn_readlane((int)v.id[b], 63);
}

// grid: x = one-wave workgroups, each walking the runs x, x + gridDim.x, ...
__global__ __launch_bounds__(64) void phase_rescue_kernel(jl_rescue_args a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_pos[kTilePos * kPosWords];
    __shared__ uint32_t s_hist[JL_RESCUE_HAP_PAD];
    const uint32_t lane = threadIdx.x;
    const uint32_t n_chunks = a.hap_pad / 64u;
    const uint8_t JL_AS1 *msa = (const uint8_t JL_AS1 *)a.msa;
    const uint32_t JL_AS1 *pos_cols = (const uint32_t JL_AS1 *)a.pos_cols;
    const uint32_t JL_AS1 *pat4 = (const uint32_t JL_AS1 *)a.pat4;
    for (uint32_t k = lane; k < JL_RESCUE_HAP_PAD; k += 64u) s_hist[k] = 0u;
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
            const uint32_t h = 64u * c + lane;
            uint32_t agree[2];
            agree[0] = agree[1] = h < a.n_hap ? 0xFFFFFFFFu : 0u;
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
                    for (uint32_t q = 0; q < 4u; ++q) {   // (a position beyond the tile's last: known = 0, nothing happens)
                        const uint32_t *sp = s_pos + (4u * g + q) * kPosWords;
                        uint32_t m[6];
#pragma unroll
                        for (uint32_t b = 0; b < 6u; ++b) m[b] = 0u - ((four >> (8u * q + b)) & 1u);
#pragma unroll
                        for (uint32_t j = 0; j < 2u; ++j) {
                            uint32_t mismatch = 0u;
#pragma unroll
                            for (uint32_t b = 0; b < 6u; ++b) mismatch |= sp[2u + 2u * b + j] ^ m[b];
                            agree[j] &= ~(mismatch & sp[j]);
                        }
                    }
                }
            }
#pragma unroll
            for (uint32_t j = 0; j < 2u; ++j) {
                v[j].two |= v[j].one & agree[j];
                v[j].one |= agree[j];
#pragma unroll
                for (uint32_t b = 6; b < 10u; ++b)
                    if ((c >> (b - 6u)) & 1u) v[j].id[b] |= agree[j];   // (wave-uniform)
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < 2u; ++j) {
#pragma unroll
            for (uint32_t b = 0; b < 6u; ++b) v[j].id[b] = (lane >> b) & 1u ? v[j].one : 0u;   // the low bits of h are the lane's
            join_wave(v[j]);
        }
        // expand: lane l answers for read 64 run + l = bit l & 31 of word l >> 5
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
        n_assigned += (uint32_t)__popcll(__ballot(exists && value < a.n_hap));
        n_ambiguous += (uint32_t)__popcll(__ballot(exists && value == (uint32_t)JL_RESCUE_AMBIGUOUS));
        n_none += (uint32_t)__popcll(__ballot(exists && value == (uint32_t)JL_RESCUE_NONE));
        n_uninformative += (uint32_t)__popcll(__ballot(exists && value == (uint32_t)JL_RESCUE_UNINFORMATIVE));
    }

    __syncthreads();
    for (uint32_t k = lane; k < a.n_hap; k += 64u)
        if (s_hist[k]) atomicAdd(a.hap_reads + k, s_hist[k]);
    if (lane == 0u) {
        if (n_assigned) atomicAdd(a.tally + 0, (unsigned long long)n_assigned);
        if (n_ambiguous) atomicAdd(a.tally + 1, (unsigned long long)n_ambiguous);
        if (n_none) atomicAdd(a.tally + 2, (unsigned long long)n_none);
        if (n_uninformative) atomicAdd(a.tally + 3, (unsigned long long)n_uninformative);
    }
}

}  // namespace

// a->hap_reads [n_hap] and a->tally [4] zeroed; the runs shared out over at most a few waves per SIMD
void jl_launch_phase_rescue(const jl_rescue_args *a, hipStream_t st)
{
    const uint32_t blocks = std::min(a->n_runs, 4096u);
    hipLaunchKernelGGL(phase_rescue_kernel, dim3(blocks), dim3(64), 0, st, *a);
}
