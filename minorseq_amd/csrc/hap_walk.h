// hap_walk.h — the walk of the kernels that compare every read of the resident matrix with a table of reported haplotypes: the
// rescue (kernels_rescue.hip), the nearest-haplotype call (kernels_nearest.hip) and the recombinant call (kernels_recomb.hip).
// Private to libjuliet_hip.so.
// Bit-parallel on the planes: a read is one bit position in every plane row, A C G T <=> plane 2 clear, planes 1 and 0 the two
// bits of a base.  Per word of 32 reads and variant position p (a codon: three columns, nine plane rows)
//   known    = ~(plane 2 of the three columns)                       the reads whose codon is A C G T throughout
//   w[b]     = planes 1, 0 of the three columns                      the six bit-words of the codon, b = 5 .. 0
//   mismatch = OR_b (w[b] ^ broadcast(bit b of pattern[h][p])) & known          the reads that can be read there and differ
// Shape.  A workgroup is ONE wave; it owns runs of 64 reads (two words, 8 bytes of every plane row) and a lane owns a
// HAPLOTYPE, 64 of them a chunk (ceil(H / 64) <= 11 chunks).  Per chunk the positions stream in tiles of 64: lane l fetches the
// nine 8-byte row pieces of position p0 + l — 64 positions in flight at once, no serial chain of dependent loads — and leaves
// `known` and the six codon words in LDS, where the inner loop reads them at a wave-uniform address (a broadcast).  The pattern
// travels transposed and packed by the host (jl_pack_pat4, hap_stage.h), four positions a dword, [ceil(n_pos / 4)][hap_pad]
// dwords: a coalesced load per lane and four positions.  11 VALU operations per position, word and lane for the mismatch word,
// the AND with known, + 6 per position for the broadcast masks; what a kernel does with the word is its FUNCTOR's.
// Per read the answer is bit-sliced: what a SET of haplotypes says of the 32 reads of a word is a `verdict` of the kernel's, and
// two DISJOINT sets are joined by a rule that is associative and commutative; the same rule joins a lane's chunks one after the
// other and the lanes by the DPP ladder of kernels_pileup.hip's wave_sum, whose total lands in lane 63 (`ladder`).  The number
// of a haplotype, h = 64 c + lane, travels in ten slices: the low six bits are the lane's, the high four the chunk's.
// Per-haplotype counts go through an LDS histogram, tallies through ballots; both reach the zeroed outputs as integer atomics:
// exact, independent of launch shape and order (`flush`).
// Garbage past the last read of a plane row touches bits no lane reports: a read is its own bit position and nothing crosses
// between them.  Addresses are formed from sizes the host checked only (jl_check_hap_table, hap_stage.h): pos_cols[p] + 2 <
// n_cols, 8 n_runs <= plane_stride; pattern bytes are data.
#pragma once
#include <stdint.h>

#include <algorithm>

// ---- host: the launch shape.  One-wave workgroups, each walking the runs x, x + gridDim.x, ...: at most a few waves per SIMD
static inline uint32_t jl_hap_walk_blocks(uint32_t n_runs) { return std::min(n_runs, 4096u); }

#if defined(__HIPCC__)
#include <type_traits>

#include "jl_internal.h"

namespace jl_hap {

constexpr uint32_t kTilePos = 64;     // positions a tile stages: one per lane
constexpr uint32_t kPosWords = 16;    // a staged position in LDS: known[2], w[6][2], 2 of padding
// a tile in LDS: `__shared__ __attribute__((aligned(16))) uint32_t s_pos[jl_hap::kTilePos * jl_hap::kPosWords]`

// the table a run is walked against, in one direction (all wave-uniform)
struct table {
    const uint8_t JL_AS1 *msa;          // the window's bit planes
    uint64_t plane_stride;
    const uint32_t JL_AS1 *pos_cols;    // [n_pos]
    const uint32_t JL_AS1 *pat4;        // [ceil(n_pos / 4)][hap_pad]
    uint32_t n_pos, hap_pad;
};

// Stage the tile of positions p0 .. p0 + 63 of run `run`: lane l brings position p0 + l; a position beyond the last is open to
// every read (known = 0).  Returns the positions the tile holds.  All lanes call it; s_pos is visible to all on return.
__device__ __forceinline__ uint32_t stage(const table &t, uint32_t p0, uint32_t run, uint32_t *s_pos, uint32_t lane)
{
    uint32_t st[14];
#pragma unroll
    for (uint32_t q = 0; q < 14u; ++q) st[q] = 0u;
    if (p0 + lane < t.n_pos) {
        const uint8_t JL_AS1 *rows = t.msa + 3ull * t.pos_cols[p0 + lane] * t.plane_stride + 8ull * run;
        uint2 r[9];
#pragma unroll
        for (uint32_t q = 0; q < 9u; ++q) r[q] = *(const uint2 JL_AS1 *)(rows + (uint64_t)q * t.plane_stride);
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
    return min(kTilePos, t.n_pos - p0);
}

// n += the positions of a staged tile at which the read of this lane can be read (k_i of SPEC §14): a lane owns a READ here,
// its bit of `known` at every position
__device__ __forceinline__ void informative(const uint32_t *s_pos, uint32_t tile_n, uint32_t lane, uint32_t &n)
{
    for (uint32_t q = 0; q < tile_n; ++q) n += (s_pos[q * kPosWords + (lane >> 5)] >> (lane & 31u)) & 1u;
}

// What a functor may leave out: the callbacks around a tile (t = p0 / 64) and around a group of four positions of it.
struct no_hooks {
    __device__ __forceinline__ void tile_begins() {}
    __device__ __forceinline__ void group_begins() {}
    __device__ __forceinline__ void group_ends(uint32_t) {}
    __device__ __forceinline__ void tile_ends(uint32_t) {}
};

template <uint32_t Q, class F>
__device__ __forceinline__ F position(const uint32_t *s_pos, uint32_t four, uint32_t g, F f)
{
    const uint32_t *sp = s_pos + (4u * g + Q) * kPosWords;
    uint32_t m[6];
#pragma unroll
    for (uint32_t b = 0; b < 6u; ++b) m[b] = 0u - ((four >> (8u * Q + b)) & 1u);
#pragma unroll
    for (uint32_t j = 0; j < 2u; ++j) {
        uint32_t mismatch = 0u;
#pragma unroll
        for (uint32_t b = 0; b < 6u; ++b) mismatch |= sp[2u + 2u * b + j] ^ m[b];
        f(g, std::integral_constant<uint32_t, Q>(), j, mismatch & sp[j]);
    }
    return f;
}

// Haplotype h against the staged tile: f(g, q, j, mismatch) for position 4 g + q of the tile (q an integral_constant) and read
// word j.  A position beyond the tile's last has known = 0: its mismatch is 0.
template <class F>
__device__ __forceinline__ F walk_tile(const table &t, const uint32_t *s_pos, uint32_t p0, uint32_t tile_n, uint32_t h, F f)
{
    const uint32_t JL_AS1 *pat = t.pat4 + (uint64_t)(p0 / 4u) * t.hap_pad + h;
    f.tile_begins();
    for (uint32_t g = 0; 4u * g < tile_n; ++g) {
        const uint32_t four = pat[(uint64_t)g * t.hap_pad];
        f.group_begins();
        f = position<0>(s_pos, four, g, f);
        f = position<1>(s_pos, four, g, f);
        f = position<2>(s_pos, four, g, f);
        f = position<3>(s_pos, four, g, f);
        f.group_ends(g);
    }
    f.tile_ends(p0 / kTilePos);
    return f;
}

// All positions of the table against haplotype h = 64 c + lane for run `run`.  With COUNT, chunk 0 adds k_i of the lane's READ
// to `informative_reads` on its way.
template <bool COUNT, class F>
__device__ __forceinline__ F walk_chunk(const table &t, uint32_t *s_pos, uint32_t run, uint32_t c, uint32_t lane, uint32_t &informative_reads, F f)
{
    const uint32_t h = 64u * c + lane;
    for (uint32_t p0 = 0; p0 < t.n_pos; p0 += kTilePos) {
        const uint32_t tile_n = stage(t, p0, run, s_pos, lane);
        if (COUNT && c == 0u) informative(s_pos, tile_n, lane, informative_reads);
        f = walk_tile(t, s_pos, p0, tile_n, h, f);
    }
    return f;
}

// ---- joining verdicts over the wave
template <int CTRL, int ROW_MASK, bool BOUND>
__device__ __forceinline__ uint32_t dpp(uint32_t old, uint32_t v)   // (old: what a lane the row mask leaves out gets)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, ROW_MASK, 0xF, BOUND);
}
template <int CTRL, int ROW_MASK, bool BOUND>
__device__ __forceinline__ uint32_t dpp(uint32_t v)
{
    return dpp<CTRL, ROW_MASK, BOUND>(0u, v);
}

// All 64 lanes' sets joined: the result is lane 63's, handed to every lane.  A verdict V brings join_lane<CTRL, ROW_MASK, BOUND>():
// this lane's set joined with the set of the lane the DPP control names, a lane the row mask leaves out joining the empty set;
// and each_word(f): f on every word of it.
template <class V>
__device__ __forceinline__ void ladder(V &v)
{
    v.template join_lane<0xB1, 0xF, true>();     // quad_perm [1,0,3,2]
    v.template join_lane<0x4E, 0xF, true>();     // quad_perm [2,3,0,1]
    v.template join_lane<0x141, 0xF, true>();    // row_half_mirror
    v.template join_lane<0x140, 0xF, true>();    // row_mirror
    v.template join_lane<0x142, 0xA, false>();   // row_bcast:15 -> rows 1, 3
    v.template join_lane<0x143, 0xC, false>();   // row_bcast:31 -> rows 2, 3
    v.each_word([](uint32_t &w) { w = (uint32_t)__builtin_amdgcn_readlane((int)w, 63); });
}

// The number of a haplotype, h = 64 c + lane, travels in ten slices.  The high four bits are the chunk's (wave-uniform): a chunk's
// set enters with slices 6..9 of 64 c.  The low six are the lane's: set once, before the ladder, from slices 0..5 of `lane`.
// Slice b of the number h, for every read of a word:
__device__ __forceinline__ uint32_t id_slice(uint32_t h, uint32_t b) { return 0u - ((h >> b) & 1u); }

// What a set of haplotypes says about the 32 reads of a word, by an extreme of a bit-sliced number:
//   best[SLICES] the LARGEST (or smallest) number in the set, tie: two or more of the set are at it, id[10]: the number of the
//   haplotype at it (valid where ~tie)
// Two DISJOINT sets are joined by comparing best slice by slice from the top:
//   win = best_a beats best_b, eq = best_a == best_b;  best = win ? a : b;  tie = win ? tie_a : eq ? all : tie_b;  id = win ? id_a : id_b
// (where eq, id is the id of neither: tie says so).  Associative and commutative in best and tie, and in id wherever tie is
// clear.  The empty set is the number nobody loses to (0, or all ones), no tie.
template <uint32_t SLICES, bool LARGEST>
struct sliced_verdict {
    static constexpr uint32_t kEmpty = LARGEST ? 0u : 0xFFFFFFFFu;
    uint32_t best[SLICES];
    uint32_t tie;
    uint32_t id[10];

    __device__ __forceinline__ void empty_set()
    {
#pragma unroll
        for (uint32_t k = 0; k < SLICES; ++k) best[k] = kEmpty;
        tie = 0u;
#pragma unroll
        for (uint32_t b = 0; b < 10u; ++b) id[b] = 0u;
    }

    // joined with the (disjoint) set b
    __device__ __forceinline__ void join(const sliced_verdict &b)
    {
        uint32_t win = 0u, eq = 0xFFFFFFFFu;
#pragma unroll
        for (int k = (int)SLICES - 1; k >= 0; --k) {
            win |= LARGEST ? eq & best[k] & ~b.best[k] : eq & ~best[k] & b.best[k];
            eq &= ~(best[k] ^ b.best[k]);
        }
#pragma unroll
        for (uint32_t k = 0; k < SLICES; ++k) best[k] = (best[k] & win) | (b.best[k] & ~win);
        tie = (tie & win) | eq | (b.tie & ~win);
#pragma unroll
        for (uint32_t k = 0; k < 10u; ++k) id[k] = (id[k] & win) | (b.id[k] & ~win);
    }

    template <int CTRL, int ROW_MASK, bool BOUND>
    __device__ __forceinline__ void join_lane()
    {
        sliced_verdict o;
#pragma unroll
        for (uint32_t k = 0; k < SLICES; ++k) o.best[k] = dpp<CTRL, ROW_MASK, BOUND>(kEmpty, best[k]);
        o.tie = dpp<CTRL, ROW_MASK, BOUND>(0u, tie);
#pragma unroll
        for (uint32_t b = 0; b < 10u; ++b) o.id[b] = dpp<CTRL, ROW_MASK, BOUND>(0u, id[b]);
        join(o);
    }

    template <class F>
    __device__ __forceinline__ void each_word(F f)
    {
#pragma unroll
        for (uint32_t k = 0; k < SLICES; ++k) f(best[k]);
        f(tie);
#pragma unroll
        for (uint32_t b = 0; b < 10u; ++b) f(id[b]);
    }
};

// ---- per read.  Lane l answers for read 64 run + l = bit l & 31 of word l >> 5.  The kernels write this expansion out (bit = lane
// & 31, hi = lane >> 5, a select and a shift per slice): behind a function of this header the compiler orders the per-read tail
// differently and the rescue and the nearest kernel go over their register counts (tests/test_hap_walk_resources.py).

// the lanes of the wave for which p holds
__device__ __forceinline__ uint32_t votes(bool p) { return (uint32_t)__popcll(__ballot(p)); }

// ---- the workgroup's counts.  clear() before the first run; flush() after the last: the n_hist words of LDS histogram and the
// K (wave-uniform) tallies into the zeroed outputs
__device__ __forceinline__ void clear(uint32_t *s_hist, uint32_t n_hist, uint32_t lane)
{
    for (uint32_t k = lane; k < n_hist; k += 64u) s_hist[k] = 0u;
}
template <uint32_t K>
__device__ __forceinline__ void flush(const uint32_t *s_hist, uint32_t n_hist, uint32_t *hist, const uint32_t (&n)[K], unsigned long long *tally, uint32_t lane)
{
    __syncthreads();
    for (uint32_t k = lane; k < n_hist; k += 64u)
        if (s_hist[k]) atomicAdd(hist + k, s_hist[k]);
    if (lane == 0u) {
#pragma unroll
        for (uint32_t k = 0; k < K; ++k)
            if (n[k]) atomicAdd(tally + k, (unsigned long long)n[k]);
    }
}

}  // namespace jl_hap
#endif
