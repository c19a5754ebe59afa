// kernels_recomb.hip — which reads are recombinants of two reported haplotypes (jl_phase_recombinants_async; docs/SPEC.md §23).
// The shape is kernels_rescue.hip's: a workgroup is ONE wave, it owns runs of 64 reads (two words, 8 bytes of every plane row), a
// lane owns a HAPLOTYPE, 64 of them a chunk; the positions stream in tiles of 64 through LDS, the pattern travels packed, four
// positions a dword (pat4 of jl_rescue_args).  Per word of 32 reads and position p
//   mismatch = OR_b (w[b] ^ broadcast(bit b of pattern[h][p])) & known          the reads that can be read there and differ
// What is new is ORDER.  Where the rescue keeps a bit and the nearest call a counter, this keeps `alive`, the reads that have not
// yet disagreed with the lane's haplotype, and where a bit of it dies at position p it records p BIT-SLICED: 13 words first[0..12]
// a read word, bit i of first[b] = bit b of the position at which read i first disagreed.  p is wave-uniform and the walk is
// hierarchical, so the slices are paid where they change: p = 64 t + 4 g + q with q unrolled, so
//   bits 0, 1   one OR of (alive & mismatch) per set bit of q, known at compile time (4 a group of four positions)
//   bits 2..5   once a group: the reads that died in it (alive before & ~alive after), ANDed with a scalar mask per bit of g
//   bits 6..12  once a tile, the same with the bits of t
// and once a chunk the reads still alive take n_pos itself, "never disagreed" — which is why there are 13 slices: 4096 must be
// representable.  About 16 VALU operations per position, word and lane where the rescue has 13.
// Per read the answer is bit-sliced too: what a SET of haplotypes says of the 32 reads of a word is
//   best[13] the LARGEST first-mismatch index in the set, tie: two or more of the set are at it, id[10]: the number of the one at it
// and two DISJOINT sets are joined by comparing best slice by slice from the top — the mirror image of kernels_nearest.hip's join:
//   gt = best_a > best_b, eq = best_a == best_b;  best = gt ? a : b;  tie = gt ? tie_a : eq ? all : tie_b;  id = gt ? id_a : id_b
// associative and commutative in best and tie, and in id wherever tie is clear; the same function joins a lane's chunks one after
// the other and the lanes by the DPP ladder of kernels_rescue.hip, whose total lands in lane 63.  A haplotype slot h >= n_hap
// enters at 0 and the empty set is {0, no tie}: a tie flagged at 0 never shows, because a recombinant has P >= 1 and S >= 1
// (P + S >= n_pos with P < n_pos gives S >= 1; S == n_pos would make P == n_pos, so S < n_pos and P >= 1) and only a recombinant
// reports its ties.
// TWO PASSES, one function: the suffix of a read is its prefix over the positions in descending order, so the host hands over the
// positions and the packed pattern a second time, reversed, and pass 1 runs the code of pass 0 on them.  A pass ends in three
// numbers a lane (P or S, its tie, its id for the lane's read); the 2 x (13 + 1) + 2 x (13 + 1 + 10) words of slices and verdicts
// are alive in one pass only.  Sharing one pass over the staged tiles would keep both directions' 152 words at once — and the
// descending direction needs the LAST mismatch of an ascending walk, an overwrite of all 13 slices where this is an OR.
// parent_reads [n_hap][2] goes through an LDS histogram of the same shape, tally through ballots; both reach the zeroed outputs as
// integer atomics: exact, independent of launch shape and order.  left, right, prefix and suffix leave by ordinary vector stores.
// Garbage past the last read of a plane row touches bits no lane reports.  Addresses are formed from sizes the host checked only
// (capi_recomb.hip); pattern bytes are data.
#include "jl_internal.h"

namespace {

constexpr uint32_t kTilePos = 64;     // positions a tile stages: one per lane
constexpr uint32_t kPosWords = 16;    // a staged position in LDS: known[2], w[6][2], 2 of padding
constexpr uint32_t kSlices = 13;      // bits of a first-mismatch index: 0 .. 4096

template <int CTRL, int ROW_MASK, bool BOUND>
__device__ __forceinline__ uint32_t dpp(uint32_t old, uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, ROW_MASK, 0xF, BOUND);
}

// what a set of haplotypes says about the 32 reads of a word
struct verdict {
    uint32_t best[kSlices];   // slice k: bit k of the largest first-mismatch index in the set (0: nobody)
    uint32_t tie;             // two or more of the set are at it
    uint32_t id[10];          // bit b of the number of the haplotype at it (valid where ~tie)
};

__device__ __forceinline__ void empty_set(verdict &v)
{
#pragma unroll
    for (uint32_t k = 0; k < kSlices; ++k) v.best[k] = 0u;
    v.tie = 0u;
#pragma unroll
    for (uint32_t b = 0; b < 10u; ++b) v.id[b] = 0u;
}

// a joined with the (disjoint) set b
__device__ __forceinline__ void join(verdict &a, const verdict &b)
{
    uint32_t gt = 0u, eq = 0xFFFFFFFFu;
#pragma unroll
    for (int k = (int)kSlices - 1; k >= 0; --k) {
        gt |= eq & a.best[k] & ~b.best[k];
        eq &= ~(a.best[k] ^ b.best[k]);
    }
#pragma unroll
    for (uint32_t k = 0; k < kSlices; ++k) a.best[k] = (a.best[k] & gt) | (b.best[k] & ~gt);
    a.tie = (a.tie & gt) | eq | (b.tie & ~gt);
#pragma unroll
    for (uint32_t k = 0; k < 10u; ++k) a.id[k] = (a.id[k] & gt) | (b.id[k] & ~gt);
}

// this lane's set joined with the set of the lane the DPP control names; a lane the row mask leaves out joins the empty set
template <int CTRL, int ROW_MASK, bool BOUND>
__device__ __forceinline__ void join_lane(verdict &v)
{
    verdict o;
#pragma unroll
    for (uint32_t k = 0; k < kSlices; ++k) o.best[k] = dpp<CTRL, ROW_MASK, BOUND>(0u, v.best[k]);
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
    for (uint32_t k = 0; k < kSlices; ++k) v.best[k] = (uint32_t)__builtin_amdgcn_readlane((int)v.best[k], 63);
    v.tie = (uint32_t)__builtin_amdgcn_readlane((int)v.tie, 63);
#pragma unroll
    for (uint32_t b = 0; b < 10u; ++b) v.id[b] = (uint32_t)__builtin_amdgcn_readlane((int)v.id[b], 63);
}

// what one direction says of the read of this lane
struct side {
    uint32_t len;   // P_i or S_i
    uint32_t tie;   // 1: two or more haplotypes attain it
    uint32_t id;    // the haplotype that attains it (valid where tie is 0)
};

// One direction over run `run`: the positions in the order of pos_cols, the pattern as pat4 packs it.  With COUNT, `informative`
// takes k_i of the lane's read in.
template <bool COUNT>
__device__ __forceinline__ side walk(const jl_recomb_args &a, const uint32_t JL_AS1 *pos_cols, const uint32_t JL_AS1 *pat4, uint32_t *s_pos,
                                     uint32_t run, uint32_t &informative)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t n_chunks = a.hap_pad / 64u;
    const uint8_t JL_AS1 *msa = (const uint8_t JL_AS1 *)a.msa;
    verdict v[2];
    empty_set(v[0]);
    empty_set(v[1]);
    for (uint32_t c = 0; c < n_chunks; ++c) {
        const uint32_t h = 64u * c + lane;
        uint32_t alive[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};   // the reads of the two words that have not yet disagreed with haplotype h
        uint32_t first[2][kSlices];                        // ... and where the others did first, sliced
#pragma unroll
        for (uint32_t j = 0; j < 2u; ++j)
#pragma unroll
            for (uint32_t k = 0; k < kSlices; ++k) first[j][k] = 0u;
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
            if (COUNT && c == 0u) {   // a lane owns a read here: its bit of `known` at every position of the tile
                for (uint32_t q = 0; q < tile_n; ++q) informative += (s_pos[q * kPosWords + (lane >> 5)] >> (lane & 31u)) & 1u;
            }
            const uint32_t JL_AS1 *pat = pat4 + (uint64_t)(p0 / 4u) * a.hap_pad + h;
            const uint32_t in_tile[2] = {alive[0], alive[1]};
            for (uint32_t g = 0; 4u * g < tile_n; ++g) {
                const uint32_t four = pat[(uint64_t)g * a.hap_pad];
                const uint32_t in_group[2] = {alive[0], alive[1]};
#pragma unroll
                for (uint32_t q = 0; q < 4u; ++q) {   // (a position beyond the tile's last: known = 0, nobody dies)
                    const uint32_t *sp = s_pos + (4u * g + q) * kPosWords;
                    uint32_t m[6];
#pragma unroll
                    for (uint32_t b = 0; b < 6u; ++b) m[b] = 0u - ((four >> (8u * q + b)) & 1u);
#pragma unroll
                    for (uint32_t j = 0; j < 2u; ++j) {
                        uint32_t mismatch = 0u;
#pragma unroll
                        for (uint32_t b = 0; b < 6u; ++b) mismatch |= sp[2u + 2u * b + j] ^ m[b];
                        mismatch &= sp[j];
                        if (q & 1u) first[j][0] |= alive[j] & mismatch;
                        if (q & 2u) first[j][1] |= alive[j] & mismatch;
                        alive[j] &= ~mismatch;
                    }
                }
#pragma unroll
                for (uint32_t j = 0; j < 2u; ++j) {
                    const uint32_t died = in_group[j] & ~alive[j];
#pragma unroll
                    for (uint32_t b = 0; b < 4u; ++b) first[j][2u + b] |= died & (0u - ((g >> b) & 1u));
                }
            }
            const uint32_t t = p0 / kTilePos;
#pragma unroll
            for (uint32_t j = 0; j < 2u; ++j) {
                const uint32_t died = in_tile[j] & ~alive[j];
#pragma unroll
                for (uint32_t b = 0; b < 7u; ++b) first[j][6u + b] |= died & (0u - ((t >> b) & 1u));
            }
        }
        // the chunk's set: one haplotype a lane, at its first mismatch (never: n_pos; a slot beyond the last haplotype: 0), the
        // high bits of its number the chunk's (wave-uniform), the low bits the lane's (set below, once)
        const uint32_t present = h < a.n_hap ? 0xFFFFFFFFu : 0u;
#pragma unroll
        for (uint32_t j = 0; j < 2u; ++j) {
            verdict one;
#pragma unroll
            for (uint32_t k = 0; k < kSlices; ++k) one.best[k] = (first[j][k] | (alive[j] & (0u - ((a.n_pos >> k) & 1u)))) & present;
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
    side s = {0u, 0u, 0u};
#pragma unroll
    for (uint32_t k = 0; k < kSlices; ++k) s.len |= (((hi ? v[1].best[k] : v[0].best[k]) >> bit) & 1u) << k;
#pragma unroll
    for (uint32_t b = 0; b < 10u; ++b) s.id |= (((hi ? v[1].id[b] : v[0].id[b]) >> bit) & 1u) << b;
    s.tie = ((hi ? v[1].tie : v[0].tie) >> bit) & 1u;
    return s;
}

// grid: x = one-wave workgroups, each walking the runs x, x + gridDim.x, ...; dynamic LDS: 2 n_hap words of histogram
__global__ __launch_bounds__(64) void phase_recombinants_kernel(jl_recomb_args a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_pos[kTilePos * kPosWords];
    extern __shared__ __attribute__((aligned(16))) uint32_t s_hist[];   // [n_hap][2]
    const uint32_t lane = threadIdx.x;
    const uint32_t n_hist = 2u * a.n_hap;
    for (uint32_t k = lane; k < n_hist; k += 64u) s_hist[k] = 0u;
    uint32_t n_recombinant = 0, n_ambiguous = 0, n_whole = 0, n_none = 0, n_uninformative = 0;   // wave-uniform

    for (uint32_t run = blockIdx.x; run < a.n_runs; run += gridDim.x) {
        uint32_t informative = 0;   // k_i of read 64 run + lane
        const side pre = walk<true>(a, (const uint32_t JL_AS1 *)a.pos_cols[0], (const uint32_t JL_AS1 *)a.pat4[0], s_pos, run, informative);
        const side suf = walk<false>(a, (const uint32_t JL_AS1 *)a.pos_cols[1], (const uint32_t JL_AS1 *)a.pat4[1], s_pos, run, informative);
        const uint64_t i = 64ull * run + lane;
        const bool exists = i < a.n_reads;
        uint32_t left, right;
        if (informative < a.min_positions) left = right = (uint32_t)JL_RESCUE_UNINFORMATIVE;
        else if (pre.len == a.n_pos) left = right = (uint32_t)JL_RECOMB_WHOLE;
        else if (pre.len + suf.len < a.n_pos) left = right = (uint32_t)JL_RESCUE_NONE;
        else {
            left = pre.tie ? (uint32_t)JL_RESCUE_AMBIGUOUS : pre.id;
            right = suf.tie ? (uint32_t)JL_RESCUE_AMBIGUOUS : suf.id;
        }
        const bool recombinant = exists && left < a.n_hap && right < a.n_hap;   // both parents unique: the histogram's cells exist
        const bool one_sided = exists && !recombinant && (left < a.n_hap || right < a.n_hap || left == (uint32_t)JL_RESCUE_AMBIGUOUS);
        if (exists) {
            ((uint16_t JL_AS1 *)a.left)[i] = (uint16_t)left;
            ((uint16_t JL_AS1 *)a.right)[i] = (uint16_t)right;
            ((uint16_t JL_AS1 *)a.prefix)[i] = (uint16_t)pre.len;
            ((uint16_t JL_AS1 *)a.suffix)[i] = (uint16_t)suf.len;
        }
        if (recombinant) {
            atomicAdd(&s_hist[2u * left], 1u);
            atomicAdd(&s_hist[2u * right + 1u], 1u);
        }
        n_recombinant += (uint32_t)__popcll(__ballot(recombinant));
        n_ambiguous += (uint32_t)__popcll(__ballot(one_sided));
        n_whole += (uint32_t)__popcll(__ballot(exists && left == (uint32_t)JL_RECOMB_WHOLE));
        n_none += (uint32_t)__popcll(__ballot(exists && left == (uint32_t)JL_RESCUE_NONE));
        n_uninformative += (uint32_t)__popcll(__ballot(exists && left == (uint32_t)JL_RESCUE_UNINFORMATIVE));
    }

    __syncthreads();
    for (uint32_t k = lane; k < n_hist; k += 64u)
        if (s_hist[k]) atomicAdd(a.parent_reads + k, s_hist[k]);
    if (lane == 0u) {
        if (n_recombinant) atomicAdd(a.tally + 0, (unsigned long long)n_recombinant);
        if (n_ambiguous) atomicAdd(a.tally + 1, (unsigned long long)n_ambiguous);
        if (n_whole) atomicAdd(a.tally + 2, (unsigned long long)n_whole);
        if (n_none) atomicAdd(a.tally + 3, (unsigned long long)n_none);
        if (n_uninformative) atomicAdd(a.tally + 4, (unsigned long long)n_uninformative);
    }
}

}  // namespace

// a->parent_reads [n_hap][2] and a->tally [5] zeroed; the runs shared out over at most a few waves per SIMD
void jl_launch_phase_recombinants(const jl_recomb_args *a, hipStream_t st)
{
    const uint32_t blocks = std::min(a->n_runs, 4096u);
    const size_t hist_bytes = (size_t)a->n_hap * 2u * sizeof(uint32_t);   // <= JL_RECOMB_HIST_WORDS words: 5.5 KiB
    hipLaunchKernelGGL(phase_recombinants_kernel, dim3(blocks), dim3(64), hist_bytes, st, *a);
}
