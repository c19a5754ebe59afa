// kernels_pileup.hip — column pileup + per-codon histogram over the resident bit planes.
//
// Behaviour implemented: doc/JULIET.md:99-100 (per-column counts of A C G T - N), :21-27/:94-98
// (codon-wise counting, deletions ignored), :256-259 (N does not count towards the coverage);
// details in docs/SPEC.md §2-3.
//
// Shape of the work.  The matrix is n_cols columns of three BIT PLANES each (plane k = bit k of every read's 3-bit code,
// reads in bit order; jl_internal.h): every cell is read exactly once — algorithmic bytes = n_reads * n_cols * 3 / 8 — so
// the kernel is an HBM stream and one instruction handles 32 reads:
//   * a lane loads 16 (or 8) bytes of each plane of each of its chunk's columns (a wave = 1 KiB contiguous per load),
//   * column counts are six popcounts per 32 reads (b0, b1, b2, b0&b1, b0&b2, b1&b2; code 7 does not occur),
//   * codon histograms are counted against a per-column seed base: six xors with the seed's bits, or-ed with the three b2
//     words (a code >= 4 anywhere: no codon): reads equal to the seed codon are ONE popcount per 32 reads (the contended
//     "major codon" bin never sees an atomic), the rare valid mismatches take an LDS atomic each.
//     The seed only steers which bin is counted the fast way — any seed gives the same histogram.
// A block owns one chunk of <= W consecutive columns from a host-built table (capi.hip: build_chunks) and a strided set of
// read tiles.  Chunks start on codon boundaries, so stretches that are locally single-frame need no halo; only where a
// codon of the chunk reaches past its last column are the next two columns loaded as well.  Loads are non-temporal (every
// cell is read once) and the next tile is prefetched into a second register set while the current one is counted.
// Per-lane counters are packed two per register, wave-reduced by DPP and flushed to LDS before 16-bit fields can overflow.
// A block that counts its chunk alone (gridDim.y = 1) stores the totals; when the reads of a long column are split over
// several blocks they go to HBM with integer atomics, which commute, so results are bit-exact and order-independent either
// way.  There is no reuse between blocks (halo columns aside), so the block -> XCD mapping does not matter here.
// pileup_planes_group_kernel runs the same body for several windows in one launch (blockIdx.z = window).
// (Rounds 1-2 counted a 4-bit-per-cell matrix with v_dot8 measurements; the planes replaced it as THE resident format in
// round 4 — every producer writes them directly — and that kernel is gone.)
#include <stdlib.h>
#include <string.h>

#include "call_eval.h"
#include "deviation_index.h"
#include "jl_internal.h"

namespace {


__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    // full 64-lane sum by DPP; the total lands in lane 63
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true);  // row_half_mirror
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true);  // row_mirror
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false); // row_bcast:15 -> rows 1,3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false); // row_bcast:31 -> rows 2,3
    return v;
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// chunk record (host-built, capi.hip: build_chunks): x = first column, y = own columns (bits 0-3) | codon-start
// flags of the own columns (bits 4-15) | "a codon reaches into the next two columns" (bit 16)
#define JL_CHUNK_META(ncols, startf, halo) ((uint32_t)(ncols) | ((uint32_t)(startf) << 4) | ((uint32_t)(halo) << 16))

// ---------------------------------------------------------------------------------------- counting from the bit planes
// The resident matrix (jl_ctx::d_msa): per column three planes — bit k of every read's code, reads in bit order — so a cell
// costs 3 bits of HBM traffic and one instruction handles 32 reads:
//   * column counts: six popcounts per 32 reads (b0, b1, b2, b0&b1, b0&b2, b1&b2; code 7 does not occur), from which
//     T = n01, N = n02, uncovered = n12, C = n0 - n01 - n02, G = n1 - n01 - n12, '-' = n2 - n02 - n12, A = the rest;
//   * codons against the seed: six xors against the seed's bits (block-uniform all-ones / all-zero words), or-ed together
//     with the three b2 words (a code >= 4 anywhere: not a codon): reads equal to the seed codon are a popcount, the rare
//     valid mismatches are walked bit by bit into the LDS histogram as before.
// A lane takes 8 or 16 bytes = 64 / 128 reads of each plane per tile; the next tile's words are prefetched into a second
// register set while the current one is counted.
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
// NQ = dwords of a plane a lane reads per tile.  16 bytes (NQ = 4) stream best: 142 us per 0.9 GB launch of eight windows
// against 149 with 8-byte loads — at 154 registers, three waves per SIMD, which a single short window pays for (22.8 us
// against 20.5 for 100k reads x 3 kb): grouped launches and deep windows take NQ = 4, a short window alone NQ = 2; the
// six-column chunks always NQ = 2 (eight columns of tiles twice over: 249 registers at 16 bytes).
constexpr uint32_t plane_tile_bytes(int nq) { return 256u * 4u * (uint32_t)nq; }
constexpr uint32_t plane_flush_tiles(int nq) { return 1023u / (32u * (uint32_t)nq); }   // 64 lanes x 32 nq reads x tiles < 2^16

template <int W, int NQ>
struct ptile_regs {
    uint32_t d[W + 2][3][NQ];   // [column][plane][dword]
};

template <int W, int NQ, bool FAST>
__device__ __forceinline__ void load_ptile(ptile_regs<W, NQ> &r, const uint8_t JL_AS1 *planes, uint64_t plane_stride, uint32_t n_cols,
                                           uint32_t c0, uint32_t ncols, uint64_t off, bool need_halo)
{
#pragma unroll
    for (int j = 0; j < W + 2; ++j) {
        if (FAST && j >= 3) continue;
        const bool live = FAST ? true : (c0 + j < n_cols) && ((uint32_t)j < ncols || (need_halo && (uint32_t)j < ncols + 2u));
        if (live) {
            const uint8_t JL_AS1 *base = planes + (uint64_t)(c0 + j) * 3u * plane_stride + off;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (NQ == 2) {
                    const u32x2 v = __builtin_nontemporal_load((const u32x2 JL_AS1 *)(base + (uint64_t)k * plane_stride));
                    r.d[j][k][0] = v.x;
                    r.d[j][k][1] = v.y;
                } else {
                    const u32x4 v = __builtin_nontemporal_load((const u32x4 JL_AS1 *)(base + (uint64_t)k * plane_stride));
                    r.d[j][k][0] = v.x;
                    r.d[j][k][1] = v.y;
                    r.d[j][k][NQ - 2] = v.z;
                    r.d[j][k][NQ - 1] = v.w;
                }
            }
        } else {   // code 6 everywhere: b0 = 0, b1 = b2 = 1
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                r.d[j][0][q] = 0u;
                r.d[j][1][q] = r.d[j][2][q] = 0xFFFFFFFFu;
            }
        }
    }
}

template <int W, int NQ, bool FAST>
__device__ __forceinline__ void pileup_planes_stream(const uint8_t JL_AS1 *planes, uint64_t plane_stride, uint32_t n_cols,
                                                     uint32_t n_tiles, uint32_t c0, uint32_t ncols, uint32_t startf, bool need_halo,
                                                     const uint32_t (&g)[W + 2], uint32_t (*s_hist)[64], uint32_t (*s_col)[6],
                                                     uint32_t *s_match)
{
    constexpr uint32_t TILE = plane_tile_bytes(NQ);
    const uint32_t tid = threadIdx.x;
    const bool last_lane = (tid & 63u) == 63u;
    const uint64_t lane_off = (uint64_t)tid * 4u * NQ;
    // the seed codon's bits as words: sh / sl[j] = all ones when bit 1 / bit 0 of column j's seed base is set
    uint32_t sh[W + 2], sl[W + 2];
#pragma unroll
    for (int j = 0; j < W + 2; ++j) {
        sh[j] = (g[j] & 2u) ? 0xFFFFFFFFu : 0u;
        sl[j] = (g[j] & 1u) ? 0xFFFFFFFFu : 0u;
    }

    uint32_t tile = blockIdx.y;
    ptile_regs<W, NQ> nxt;
    bool nxt_live = false;
    if (tile < n_tiles) {
        const uint64_t off = (uint64_t)tile * TILE + lane_off;
        nxt_live = off < plane_stride;
        if (nxt_live) load_ptile<W, NQ, FAST>(nxt, planes, plane_stride, n_cols, c0, ncols, off, need_halo);
    }

    while (tile < n_tiles) {
        uint32_t acc[W][6];   // n0 n1 n2 n01 n02 n12
        uint32_t match[W];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            match[j] = 0;
#pragma unroll
            for (int k = 0; k < 6; ++k) acc[j][k] = 0;
        }
        uint32_t reads = 0;

        for (uint32_t it = 0; it < plane_flush_tiles(NQ) && tile < n_tiles; ++it, tile += gridDim.y) {
            const ptile_regs<W, NQ> cur = nxt;
            const bool live = nxt_live;
            const uint32_t tn = tile + gridDim.y;
            nxt_live = false;
            if (tn < n_tiles) {
                const uint64_t off = (uint64_t)tn * TILE + lane_off;
                nxt_live = off < plane_stride;
                if (nxt_live) load_ptile<W, NQ, FAST>(nxt, planes, plane_stride, n_cols, c0, ncols, off, need_halo);
            }
            if (!live) continue;
            reads += 32u * NQ;
#pragma unroll
            for (int j = 0; j < W; ++j) {
                if (FAST ? j < 3 : (uint32_t)j < ncols) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        const uint32_t b0 = cur.d[j][0][q], b1 = cur.d[j][1][q], b2 = cur.d[j][2][q];
                        acc[j][0] += __popc(b0);
                        acc[j][1] += __popc(b1);
                        acc[j][2] += __popc(b2);
                        acc[j][3] += __popc(b0 & b1);
                        acc[j][4] += __popc(b0 & b2);
                        acc[j][5] += __popc(b1 & b2);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < W; ++j) {
                if (FAST ? j == 0 : (startf & (1u << j)) != 0) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        const uint32_t inv = cur.d[j][2][q] | cur.d[j + 1][2][q] | cur.d[j + 2][2][q];   // some code >= 4: not in coverage
                        const uint32_t x = (cur.d[j][1][q] ^ sh[j]) | (cur.d[j][0][q] ^ sl[j]) | (cur.d[j + 1][1][q] ^ sh[j + 1]) |
                                           (cur.d[j + 1][0][q] ^ sl[j + 1]) | (cur.d[j + 2][1][q] ^ sh[j + 2]) | (cur.d[j + 2][0][q] ^ sl[j + 2]);
                        match[j] += __popc(~(x | inv));      // valid and equal to the seed codon
                        uint32_t rest = x & ~inv;            // valid codon, not the seed one
                        while (rest) {
                            const int b = __ffs((int)rest) - 1;
                            rest &= rest - 1;
                            const uint32_t idx = (((cur.d[j][1][q] >> b) & 1u) << 5) | (((cur.d[j][0][q] >> b) & 1u) << 4) |
                                                 (((cur.d[j + 1][1][q] >> b) & 1u) << 3) | (((cur.d[j + 1][0][q] >> b) & 1u) << 2) |
                                                 (((cur.d[j + 2][1][q] >> b) & 1u) << 1) | ((cur.d[j + 2][0][q] >> b) & 1u);
                            atomicAdd(&s_hist[j][idx], 1u);
                        }
                    }
                }
            }
        }

        // ---- flush this batch: the counts from the six popcount sums, 16-bit packing, DPP wave sums, LDS atomics
#pragma unroll
        for (int j = 0; j < W; ++j) {
            if (FAST && j >= 3) continue;
            const uint32_t nT = acc[j][3], nN = acc[j][4], nU = acc[j][5];
            const uint32_t nC = acc[j][0] - nT - nN, nG = acc[j][1] - nT - nU, nD = acc[j][2] - nN - nU;
            const uint32_t nA = reads - (nC + nG + nT + nD + nN + nU);
            const uint32_t p0 = wave_sum(nA | (nC << 16));
            const uint32_t p1 = wave_sum(nG | (nT << 16));
            const uint32_t p2 = wave_sum(nD | (nN << 16));
            const bool starts = FAST ? j == 0 : (startf & (1u << j)) != 0;
            uint32_t p3 = 0;
            if (starts) p3 = wave_sum(match[j]);   // (block-uniform branch)
            if (last_lane && (uint32_t)j < ncols) {
                if (p0 & 0xFFFFu) atomicAdd(&s_col[j][0], p0 & 0xFFFFu);
                if (p0 >> 16) atomicAdd(&s_col[j][1], p0 >> 16);
                if (p1 & 0xFFFFu) atomicAdd(&s_col[j][2], p1 & 0xFFFFu);
                if (p1 >> 16) atomicAdd(&s_col[j][3], p1 >> 16);
                if (p2 & 0xFFFFu) atomicAdd(&s_col[j][4], p2 & 0xFFFFu);
                if (p2 >> 16) atomicAdd(&s_col[j][5], p2 >> 16);
                if (starts && p3) atomicAdd(&s_match[j], p3);
            }
        }
    }
}

// The end of a chunk's workgroup, behind the barrier that closes its counting: store (or add) the column counts, put the seed codon's
// reads into their bin, store the histogram, and (FOLD) the Fisher stage from the histogram still in LDS.  Shared by the plane
// kernels and the index kernels (pileup_index_body): what is downstream of the counters is one piece of code.
template <int W, bool FOLD>
__device__ __forceinline__ void pileup_tail(uint32_t (*s_hist)[64], uint32_t (*s_col)[6], uint32_t *s_match, const uint32_t (&g)[W + 2],
                                            uint32_t c0, uint32_t ncols, uint32_t startf, uint32_t JL_AS1 *counts, uint32_t JL_AS1 *hist,
                                            const jl_win_fold *fold)
{
    const uint32_t tid = threadIdx.x;
    const bool excl = gridDim.y == 1;
    if (tid < W * 6) {
        const uint32_t j = tid / 6u, k = tid - j * 6u;
        const uint32_t v = s_col[j][k];
        if (j < ncols) {
            if (excl) counts[(uint64_t)(c0 + j) * 6u + k] = v;
            else if (v) atomicAdd((uint32_t *)(counts + (uint64_t)(c0 + j) * 6u + k), v);
        }
    }
    if (tid < W && (startf & (1u << tid))) {
        const uint32_t j = tid;
        const uint32_t seed = (g[j] << 4) | (g[j + 1] << 2) | g[j + 2];
        s_hist[j][seed] += s_match[j];   // reads equal to the seed codon were only counted, never binned
    }
    __syncthreads();
    for (uint32_t i = tid; i < W * 64; i += 256) {
        const uint32_t j = i >> 6;
        const uint32_t v = s_hist[j][i & 63u];
        if (startf & (1u << j)) {
            if (excl) hist[(uint64_t)(c0 + j) * 64u + (i & 63u)] = v;
            else if (v) atomicAdd((uint32_t *)(hist + (uint64_t)(c0 + j) * 64u + (i & 63u)), v);
        }
    }
    if (FOLD) {
        const jl_win_call &c = fold->c;
        if (blockIdx.x == 0 && tid == 0 && c.meta) {   // counters of the phasing launch that follows on the stream (call_kernel's first block did this)
            // (an index-form run of a window with a rest table does this twice, in the index launch and in the plane launch over the
            // rest: harmless, nothing between the two writes these counters — the phasing launch comes behind both)
            c.meta->n_occupied = 0;
            c.meta->overflow = 0;
            jl_phase_summary z = {0, 0, 0, 0, 0, 0, 0, 0};
            c.meta->summary = z;
        }
        const uint32_t wid = tid >> 6, lane = tid & 63u;
#pragma unroll
        for (int j = 0; j < W; ++j) {
            if (((uint32_t)j & 3u) != wid || !(startf & (1u << j))) continue;      // (wave-uniform)
            const uint32_t col = c0 + (uint32_t)j;
            const uint32_t h = s_hist[j][lane];
            for (uint32_t p = fold->col_head[col]; p != 0xFFFFFFFFu; p = fold->pos_next[p])
                jl_call_position_at<false>(c.A, p, col, h, c.pos_refcfg[p], c.pos_gene, c.pos_codon, c.drm, c.called, c.staged);
        }
    }
}

// FOLD (round 6): the Fisher stage of the chunk's codons in the workgroup that has just counted them — the histogram is still in
// LDS — instead of a call launch that reads it back from HBM (8 us of a 64 us window, 20 of the 72 us an eight-window launch's
// tail exposes).  Only where ONE workgroup counts a chunk (gridDim.y = 1).  Wave j & 3 takes the codon that begins at the chunk's
// column j — the positions at that column from the host's lists (jl_win_fold) — behind the kernel's last barrier: the other
// waves store the histogram and leave, so what the evaluation holds for its 2-3 us is one wave's registers, not the workgroup's.
// A single run (jl_run_async) always takes this form where it can.  A group run takes it per launch, only while its tail is
// likely to be exposed (capi_group.hip "Two forms"): in a steady stream of group launches the epilogue cost 2.7 % of a step.
template <int W, int NQ, bool FOLD>
__device__ __forceinline__ void pileup_planes_body(const uint8_t JL_AS1 *planes, uint64_t plane_stride, uint32_t n_cols, uint32_t n_tiles,
                                                   const uint2 JL_AS1 *chunks, const uint32_t JL_AS1 *guess32, uint32_t JL_AS1 *counts,
                                                   uint32_t JL_AS1 *hist, const jl_win_fold *fold)
{
    __shared__ uint32_t s_hist[W][64];
    __shared__ uint32_t s_col[W][6];   // A C G T - N
    __shared__ uint32_t s_match[W];
    const uint32_t tid = threadIdx.x;
    const uint2 rec = chunks[blockIdx.x];
    const uint32_t c0 = rec.x;
    const uint32_t ncols = rec.y & 15u;
    const uint32_t startf = (rec.y >> 4) & 0xFFFu;
    const bool need_halo = ((rec.y >> 16) & 1u) != 0;
    constexpr int NG = (W + 2 + 3 + 3) / 4;
    uint32_t gw[NG];
#pragma unroll
    for (int k = 0; k < NG; ++k) gw[k] = guess32[(c0 >> 2) + k];
    uint32_t g[W + 2];   // the seed base of column c0 + j (0..3)
#pragma unroll
    for (int j = 0; j < W + 2; ++j) {
        const uint32_t b = (c0 & 3u) + (uint32_t)j;
        uint32_t word = gw[0];
#pragma unroll
        for (int k = 1; k < NG; ++k)
            if ((b >> 2) == (uint32_t)k) word = gw[k];
        g[j] = (word >> (8u * (b & 3u))) & 3u;
    }
    for (uint32_t i = tid; i < W * 64; i += 256) (&s_hist[0][0])[i] = 0;
    if (tid < W * 6) (&s_col[0][0])[tid] = 0;
    if (tid < W) s_match[tid] = 0;
    __syncthreads();
    if (W == 3 && rec.y == JL_CHUNK_META(3, 1, 0))
        pileup_planes_stream<W, NQ, true>(planes, plane_stride, n_cols, n_tiles, c0, ncols, startf, need_halo, g, s_hist, s_col, s_match);
    else
        pileup_planes_stream<W, NQ, false>(planes, plane_stride, n_cols, n_tiles, c0, ncols, startf, need_halo, g, s_hist, s_col, s_match);
    __syncthreads();
    pileup_tail<W, FOLD>(s_hist, s_col, s_match, g, c0, ncols, startf, counts, hist, fold);
}

template <int W, int NQ>
__global__ __launch_bounds__(256) void pileup_planes_kernel(const uint8_t *__restrict__ planes, uint64_t plane_stride, uint32_t n_cols,
                                                            uint32_t n_tiles, const uint2 *__restrict__ chunks,
                                                            const uint32_t *__restrict__ guess32, uint32_t *__restrict__ counts,
                                                            uint32_t *__restrict__ hist)
{
    pileup_planes_body<W, NQ, false>((const uint8_t JL_AS1 *)planes, plane_stride, n_cols, n_tiles, (const uint2 JL_AS1 *)chunks,
                                     (const uint32_t JL_AS1 *)guess32, (uint32_t JL_AS1 *)counts, (uint32_t JL_AS1 *)hist, nullptr);
}

template <int W, int NQ>
__global__ __launch_bounds__(256) void pileup_planes_group_kernel(jl_pileup_group_args args)
{
    const jl_win_pileup &w = args.w[blockIdx.z];
    if (blockIdx.x >= w.n_chunks) return;
    pileup_planes_body<W, NQ, false>((const uint8_t JL_AS1 *)w.msa, w.plane_stride, w.n_cols, w.n_tiles, (const uint2 JL_AS1 *)w.chunks,
                                     (const uint32_t JL_AS1 *)w.guess32, (uint32_t JL_AS1 *)w.counts, (uint32_t JL_AS1 *)w.hist, nullptr);
}

// ... and with the Fisher stage folded in (runs whose chunks are counted by one workgroup each; gridDim.y = 1)
template <int W, int NQ>
__global__ __launch_bounds__(256) void pileup_fold_kernel(jl_win_pileup w, jl_win_fold f)
{
    pileup_planes_body<W, NQ, true>((const uint8_t JL_AS1 *)w.msa, w.plane_stride, w.n_cols, w.n_tiles, (const uint2 JL_AS1 *)w.chunks,
                                    (const uint32_t JL_AS1 *)w.guess32, (uint32_t JL_AS1 *)w.counts, (uint32_t JL_AS1 *)w.hist, &f);
}

template <int W, int NQ>
__global__ __launch_bounds__(256) void pileup_fold_group_kernel(jl_pileup_fold_group_args args)
{
    const jl_win_pileup &w = args.w[blockIdx.z];
    if (blockIdx.x >= w.n_chunks) return;
    pileup_planes_body<W, NQ, true>((const uint8_t JL_AS1 *)w.msa, w.plane_stride, w.n_cols, w.n_tiles, (const uint2 JL_AS1 *)w.chunks,
                                    (const uint32_t JL_AS1 *)w.guess32, (uint32_t JL_AS1 *)w.counts, (uint32_t JL_AS1 *)w.hist, &args.f[blockIdx.z]);
}

// ------------------------------------------------------------------------------- counting from the deviation index
// A resident window that is run again and again keeps, per plain codon chunk, the list of the reads that differ from the chunk's
// index seed anywhere in its three columns (deviation_index.h; built by kernels_index.hip behind the window's second run): about
// 6 % of the reads of a CCS sample, 2 bytes each (the three codes; the read number is not stored), against nine plane rows.  One
// workgroup per plain chunk:
//   * a lane streams four entries per round with one 8-byte non-temporal load, two entries to a dword, DEPTH rounds held in
//     registers: the loads of the first DEPTH rounds all go out before the first is consumed, and each register is loaded with
//     round r + DEPTH as round r leaves it.  DEPTH = JL_IX_DEPTH = 2 in the unfolded kernels, which hide the chain of round trips
//     behind eight workgroups per CU and must keep the registers for that: 4 KB per workgroup in flight, a benchmark chunk's list
//     (12.6 KB) in 3.1 dependent round trips; DEPTH = JL_IX_FOLD_DEPTH = 16 in the folded ones, whose Fisher epilogue leaves five
//     workgroups per CU (JL_IX_FOLD_WAVES) whatever the walk needs: 32 KB per workgroup in flight, a benchmark chunk's whole list
//     in one round trip;
//   * column counts: per lane one 64-bit accumulator per column with a 9-bit field per code 0..6 — at most JL_IX_FLUSH_ROUNDS
//     rounds x 4 entries = 508 <= 511 per field between flushes (whole batches of DEPTH rounds: 126 rounds at depth 2, 112 at
//     depth 16); a flush unpacks them two to a register (64 lanes x 508 < 2^16), sums over the wave by DPP and adds to LDS, as the
//     plane kernel does;
//   * an entry whose three codes are all bases is a valid codon other than the seed codon (it differs somewhere): one LDS atomic;
//     an entry with a code >= 4 is outside the coverage, as `inv` says in the plane kernel;
//   * the n_reads - E reads that are not in the list carry the seed base in every column: added to those bins and to the seed
//     codon's count (s_match), from where pileup_tail takes over unchanged.  Padding reads are never in a list.
// A plain chunk over the density bound has no list (tab[].z all ones): its workgroup counts it from the planes with a simple
// walk — few registers, no prefetch: the path is rare and must not cost the common one its occupancy.
// Registers (gfx950, the compiler's kernel-resource-usage remarks): pileup_index_kernel and pileup_index_group_kernel 58 VGPRs,
// eight waves per SIMD, no scratch; pileup_index_fold_kernel and pileup_index_fold_group_kernel 96 VGPRs, five waves per SIMD, 128
// bytes of scratch a lane, at depth 16 as at depth 8, and the unfolded ones' 58 at depth 1, 2 and 4 alike (without a bound the
// folded ones take 132, three waves — the epilogue sets the figure, the walk stays under 60).  tests/test_fold_budget_resources.py pins these.  The plane path's 154 are why index and plane counting are
// separate kernels.
// The folded index kernels' register budget, as waves per SIMD (__launch_bounds__): 5 = 96 VGPRs, five workgroups per CU.  What does
// not fit is the Fisher stage's (its FP64 constants, which the compiler hoists out of the loop over a column's positions): the
// spill's stores and loads all lie behind the barrier that closes the walk, in the one wave that evaluates.  The sweep of 3 / 4 / 5
// waves against depth 8 / 4 / 2 (of 16-byte rounds, the 4-byte entry of the day) is in profiles/fold_budget/: the deepest is ahead at
// every budget, so the depth does not follow the budget.  The depths of the 8-byte rounds: profiles/narrow_index/.
#ifndef JL_IX_FOLD_WAVES
#define JL_IX_FOLD_WAVES 5
#endif
template <int DEPTH>
__device__ __forceinline__ void index_stream(const jl_ix_stored_t JL_AS1 *list, uint32_t E, uint32_t (*s_hist)[64], uint32_t (*s_col)[6])
{
    static_assert(DEPTH >= 1 && DEPTH <= (int)JL_IX_MAX_DEPTH, "rounds held in registers");
    // rounds between two flushes: whole batches, at most JL_IX_FLUSH_ROUNDS (126 at depth 2, 112 at depth 16: 448 <= 511 per field)
    constexpr uint32_t FLUSH_BATCHES = jl_ix_flush_rounds_at((uint32_t)DEPTH) / (uint32_t)DEPTH;
    static_assert(FLUSH_BATCHES >= 1u && FLUSH_BATCHES * (uint32_t)DEPTH <= JL_IX_FLUSH_ROUNDS, "a 9-bit field never above 511");
    static_assert(sizeof(jl_ix_stored_t) * JL_IX_ROUND_ENTRIES == sizeof(u32x2), "a lane's round is one 8-byte load");
    const uint32_t tid = threadIdx.x;
    const bool last_lane = (tid & 63u) == 63u;
    const u32x2 JL_AS1 *src = (const u32x2 JL_AS1 *)list;   // (a list begins on four entries: jl_ix_padded)
    const uint32_t n_rounds = (E + 4u * 256u - 1u) / (4u * 256u);
    // buf[k]: this lane's four entries of round r + k, two to a dword — the first batch's loads all go out before the first is consumed
    u32x2 buf[DEPTH];
#pragma unroll
    for (int k = 0; k < DEPTH; ++k) {
        buf[k] = u32x2{0u, 0u};
        if (((uint32_t)k * 256u + tid) * 4u < E) buf[k] = __builtin_nontemporal_load(src + (size_t)k * 256u + tid);
    }
    uint32_t r = 0;
    while (r < n_rounds) {
        // (codes are 0..6: every producer of an OWNED matrix writes or validates them — jl_msa_upload and jl_msa_pack_rows refuse a
        // matrix with a code outside 0..6, ingest, synth fill, take and the assemblies write none — and an adopted matrix, the only
        // way caller-made planes get in, is never indexed: no field 7, which would sit at bit 63)
        unsigned long long acc[3] = {0ull, 0ull, 0ull};
        for (uint32_t it = 0; it < FLUSH_BATCHES && r < n_rounds; ++it, r += (uint32_t)DEPTH) {
#pragma unroll
            for (int k = 0; k < DEPTH; ++k) {
                if (r + (uint32_t)k >= n_rounds) break;                  // (uniform: the batch's later rounds are past the list too)
                const u32x2 cur = buf[k];
                const uint32_t first = ((r + (uint32_t)k) * 256u + tid) * 4u;   // this lane's first entry of the round
                // the register is free: round r + k + DEPTH goes out into it, DEPTH - 1 younger loads still in flight
                const uint32_t nfirst = first + (uint32_t)DEPTH * 4u * 256u;
                if (nfirst < E) buf[k] = __builtin_nontemporal_load(src + (size_t)(r + (uint32_t)k + (uint32_t)DEPTH) * 256u + tid);
                // (a stored entry's upper seven bits are zero: the high half of a dword needs no mask)
                const uint32_t e4[4] = {cur.x & 0xFFFFu, cur.x >> 16, cur.y & 0xFFFFu, cur.y >> 16};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (first + (uint32_t)i >= E) continue;
                    const uint32_t e = e4[i];
                    const uint32_t a = (e >> 6) & 7u, b = (e >> 3) & 7u, c = e & 7u;
                    acc[0] += 1ull << (JL_IX_FIELD_BITS * a);
                    acc[1] += 1ull << (JL_IX_FIELD_BITS * b);
                    acc[2] += 1ull << (JL_IX_FIELD_BITS * c);
                    if ((e & 0x124u) == 0u) atomicAdd(&s_hist[0][(a << 4) | (b << 2) | c], 1u);   // no code >= 4: a valid codon
                }
            }
        }
        // ---- flush: codes 0..5 of each column (code 6, uncovered, is not reported), two 9-bit fields to a DPP sum
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const uint32_t m = (1u << JL_IX_FIELD_BITS) - 1u;
            uint32_t p[3];
#pragma unroll
            for (int k = 0; k < 3; ++k)
                p[k] = wave_sum(((uint32_t)(acc[j] >> (JL_IX_FIELD_BITS * 2u * k)) & m) | (((uint32_t)(acc[j] >> (JL_IX_FIELD_BITS * (2u * k + 1u))) & m) << 16));
            if (last_lane) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    if (p[k] & 0xFFFFu) atomicAdd(&s_col[j][2 * k], p[k] & 0xFFFFu);
                    if (p[k] >> 16) atomicAdd(&s_col[j][2 * k + 1], p[k] >> 16);
                }
            }
        }
    }
}

// a plain chunk that has no list, from its nine plane rows: a lane takes 32 reads of every row per step
__device__ __forceinline__ void index_dense_stream(const uint8_t JL_AS1 *planes, uint64_t plane_stride, uint32_t c0, const uint32_t (&g)[5],
                                                   uint32_t (*s_hist)[64], uint32_t (*s_col)[6], uint32_t *s_match)
{
    const uint32_t tid = threadIdx.x;
    const bool last_lane = (tid & 63u) == 63u;
    const uint32_t n_words = (uint32_t)(plane_stride / 4u);
    const uint32_t JL_AS1 *base = (const uint32_t JL_AS1 *)(planes + (uint64_t)c0 * 3u * plane_stride);
    const uint64_t row = plane_stride / 4u;
    uint32_t acc[3][6], match = 0, reads = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 6; ++k) acc[j][k] = 0;
    for (uint32_t w = tid; w < n_words; w += 256u) {
        uint32_t d[3][3];
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int k = 0; k < 3; ++k) d[j][k] = base[(uint64_t)(3 * j + k) * row + w];
        reads += 32u;
        uint32_t inv = 0, x = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const uint32_t b0 = d[j][0], b1 = d[j][1], b2 = d[j][2];
            acc[j][0] += __popc(b0);
            acc[j][1] += __popc(b1);
            acc[j][2] += __popc(b2);
            acc[j][3] += __popc(b0 & b1);
            acc[j][4] += __popc(b0 & b2);
            acc[j][5] += __popc(b1 & b2);
            inv |= b2;
            x |= (b1 ^ ((g[j] & 2u) ? 0xFFFFFFFFu : 0u)) | (b0 ^ ((g[j] & 1u) ? 0xFFFFFFFFu : 0u));
        }
        match += __popc(~(x | inv));
        uint32_t rest = x & ~inv;
        while (rest) {
            const int b = __ffs((int)rest) - 1;
            rest &= rest - 1;
            const uint32_t idx = (((d[0][1] >> b) & 1u) << 5) | (((d[0][0] >> b) & 1u) << 4) | (((d[1][1] >> b) & 1u) << 3) |
                                 (((d[1][0] >> b) & 1u) << 2) | (((d[2][1] >> b) & 1u) << 1) | ((d[2][0] >> b) & 1u);
            atomicAdd(&s_hist[0][idx], 1u);
        }
    }
    // (a lane's sums reach 2^15 at 2^23 reads: whole registers through the wave sums here, no packing)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const uint32_t nT = acc[j][3], nN = acc[j][4], nU = acc[j][5];
        const uint32_t nC = acc[j][0] - nT - nN, nG = acc[j][1] - nT - nU, nD = acc[j][2] - nN - nU;
        const uint32_t nA = reads - (nC + nG + nT + nD + nN + nU);
        const uint32_t v[6] = {wave_sum(nA), wave_sum(nC), wave_sum(nG), wave_sum(nT), wave_sum(nD), wave_sum(nN)};
        if (last_lane) {
#pragma unroll
            for (int k = 0; k < 6; ++k)
                if (v[k]) atomicAdd(&s_col[j][k], v[k]);
        }
    }
    const uint32_t ms = wave_sum(match);
    if (last_lane && ms) atomicAdd(&s_match[0], ms);
}

template <bool FOLD>
__device__ __forceinline__ void pileup_index_body(const uint8_t JL_AS1 *planes, uint64_t plane_stride, uint32_t n_reads, const uint4 JL_AS1 *tab,
                                                  const jl_ix_stored_t JL_AS1 *entries, const uint8_t JL_AS1 *seed, uint32_t JL_AS1 *counts,
                                                  uint32_t JL_AS1 *hist, const jl_win_fold *fold)
{
    __shared__ uint32_t s_hist[3][64];
    __shared__ uint32_t s_col[3][6];   // A C G T - N
    __shared__ uint32_t s_match[3];
    const uint32_t tid = threadIdx.x;
    const uint4 rec = tab[blockIdx.x];   // {first column, first entry, entries or all ones, -}
    const uint32_t c0 = rec.x;
    const uint32_t g[5] = {seed[c0] & 3u, seed[c0 + 1u] & 3u, seed[c0 + 2u] & 3u, 0u, 0u};   // (a plain chunk: c0 + 2 < n_cols)
    for (uint32_t i = tid; i < 3 * 64; i += 256) (&s_hist[0][0])[i] = 0;
    if (tid < 3 * 6) (&s_col[0][0])[tid] = 0;
    if (tid < 3) s_match[tid] = 0;
    __syncthreads();
    if (rec.z != 0xFFFFFFFFu) {
        index_stream<FOLD ? JL_IX_FOLD_DEPTH : JL_IX_DEPTH>(entries + rec.y, rec.z, s_hist, s_col);
        if (tid < 3) atomicAdd(&s_col[tid][g[tid]], n_reads - rec.z);   // the reads not in the list: the seed base in every column
        if (tid == 3) s_match[0] = n_reads - rec.z;                     // ... and the seed codon
    } else {
        index_dense_stream(planes, plane_stride, c0, g, s_hist, s_col, s_match);
    }
    __syncthreads();
    pileup_tail<3, FOLD>(s_hist, s_col, s_match, g, c0, 3u, 1u, counts, hist, fold);
}

#define JL_INDEX_BODY(FOLD, w, f)                                                                                                     \
    pileup_index_body<FOLD>((const uint8_t JL_AS1 *)(w).msa, (w).plane_stride, (w).n_reads, (const uint4 JL_AS1 *)(w).tab,            \
                            (const jl_ix_stored_t JL_AS1 *)(w).entries, (const uint8_t JL_AS1 *)(w).seed, (uint32_t JL_AS1 *)(w).counts,     \
                            (uint32_t JL_AS1 *)(w).hist, f)

__global__ __launch_bounds__(256) void pileup_index_kernel(jl_win_index w) { JL_INDEX_BODY(false, w, nullptr); }
__global__ __launch_bounds__(256, JL_IX_FOLD_WAVES) void pileup_index_fold_kernel(jl_win_index w, jl_win_fold f) { JL_INDEX_BODY(true, w, &f); }
__global__ __launch_bounds__(256) void pileup_index_group_kernel(jl_index_group_args args)
{
    const jl_win_index &w = args.w[blockIdx.z];
    if (blockIdx.x >= w.n_plain) return;
    JL_INDEX_BODY(false, w, nullptr);
}
__global__ __launch_bounds__(256, JL_IX_FOLD_WAVES) void pileup_index_fold_group_kernel(jl_index_fold_group_args args)
{
    const jl_win_index &w = args.w[blockIdx.z];
    if (blockIdx.x >= w.n_plain) return;
    JL_INDEX_BODY(true, w, &args.f[blockIdx.z]);
}
#undef JL_INDEX_BODY

// Seed base per column for majority-codon mode: majority base among the first 2048 reads of the column.
// (Any value is correct; a good seed keeps the codon compare on its fast path.)
__global__ __launch_bounds__(64) void guess_kernel(const uint8_t *__restrict__ planes, uint64_t plane_stride,
                                                   uint32_t n_cols, uint8_t *__restrict__ guess)
{
    const uint32_t c = blockIdx.x;
    if (c >= n_cols) return;
    const uint32_t lane = threadIdx.x;
    uint32_t nA = 0, nC = 0, nG = 0, nT = 0;
    const uint64_t off = (uint64_t)lane * 4u;   // 64 lanes x 32 reads
    if (off < plane_stride) {
        const uint8_t *base = planes + (uint64_t)c * 3u * plane_stride + off;
        const uint32_t b0 = *reinterpret_cast<const uint32_t *>(base);
        const uint32_t b1 = *reinterpret_cast<const uint32_t *>(base + plane_stride);
        const uint32_t b2 = *reinterpret_cast<const uint32_t *>(base + 2u * plane_stride);
        nA = __popc(~b2 & ~b1 & ~b0);
        nC = __popc(~b2 & ~b1 & b0);
        nG = __popc(~b2 & b1 & ~b0);
        nT = __popc(~b2 & b1 & b0);
    }
    const uint32_t p0 = wave_sum(nA | (nC << 16));
    const uint32_t p1 = wave_sum(nG | (nT << 16));
    if (lane == 63) {
        uint32_t best = 0, bv = p0 & 0xFFFFu;
        if ((p0 >> 16) > bv) { bv = p0 >> 16; best = 1; }
        if ((p1 & 0xFFFFu) > bv) { bv = p1 & 0xFFFFu; best = 2; }
        if ((p1 >> 16) > bv) { bv = p1 >> 16; best = 3; }
        guess[c] = (uint8_t)best;
    }
}

}  // namespace

const char *jl_pileup_kernel_name(void) { return "pileup_planes_kernel"; }   // rocprofv3 prints the template arguments behind it

// the load width of a launch (see plane_tile_bytes above); chunk tables are 3 or 6 columns wide (build_chunks)
static int planes_nq(const jl_ctx *ctx, bool grouped) { return ctx->pileup_w == 3 && (grouped || ctx->plane_stride >= 32768u) ? 4 : 2; }
static uint32_t planes_tiles(const jl_ctx *ctx, bool grouped)
{
    const uint32_t tile = plane_tile_bytes(planes_nq(ctx, grouped));
    return (uint32_t)((ctx->plane_stride + tile - 1) / tile);
}
// slot of the single-window kernel in the context's occupancy table
static int planes_slot(const jl_ctx *ctx) { return ctx->pileup_w == 3 ? (planes_nq(ctx, false) == 4 ? 0 : 1) : 2; }

void jl_launch_guess(jl_ctx *ctx, hipStream_t st)
{
    hipLaunchKernelGGL(guess_kernel, dim3(ctx->n_cols), dim3(64), 0, st, ctx->d_msa, ctx->plane_stride, ctx->n_cols, ctx->d_guess);
}

// occupancy query, once per kernel and outside any stream capture
void jl_prepare_pileup(jl_ctx *ctx)
{
    const int idx = planes_slot(ctx);
    if (ctx->pileup_blocks_per_cu[idx] > 0) return;
    // (the single-window launch: a short window alone reads 8 bytes a lane, a deep one 16)
    const void *fn = idx == 0 ? (const void *)pileup_planes_kernel<3, 4> : idx == 1 ? (const void *)pileup_planes_kernel<3, 2>
                                                                                    : (const void *)pileup_planes_kernel<6, 2>;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 256, 0) != hipSuccess || per_cu < 1) per_cu = 2;
    if (per_cu > 8) per_cu = 8;
    ctx->pileup_blocks_per_cu[idx] = per_cu;
}

// Launch shape: chunks x read splits.  One resident wave of blocks (CUs x the blocks the kernel's registers admit
// per CU) for short columns, four per slot for long ones; reads are split no finer than a tile.
uint32_t jl_pileup_rsplit(jl_ctx *ctx)
{
    jl_prepare_pileup(ctx);
    const uint32_t n_chunks = ctx->n_chunks ? ctx->n_chunks : 1u;
    const uint32_t n_tiles = planes_tiles(ctx, false);
    const int per_cu = ctx->pileup_blocks_per_cu[planes_slot(ctx)];
    // long columns: several blocks per slot smooth the tail; short ones: exactly one resident wave of blocks
    const uint32_t target = 256u * (uint32_t)per_cu * (n_tiles >= 64 ? 4u : 1u);
    uint32_t rsplit = target / n_chunks;  // never more blocks than resident slots: a second wave costs more than it balances
    if (rsplit > n_tiles) rsplit = n_tiles;
    if (rsplit < 1) rsplit = 1;
    if (rsplit > 65535u) rsplit = 65535u;
    return rsplit;
}

// With one read split every chunk is counted by exactly one block, which stores its totals: no zeroing needed.
bool jl_pileup_needs_zero(jl_ctx *ctx) { return jl_pileup_rsplit(ctx) != 1u; }

void jl_launch_pileup(jl_ctx *ctx, hipStream_t st)
{
    const uint32_t rsplit = jl_pileup_rsplit(ctx);
    const uint32_t nt = planes_tiles(ctx, false);
#define JL_LAUNCH_PLANES(W, NQ)                                                                                                       \
    hipLaunchKernelGGL((pileup_planes_kernel<W, NQ>), dim3(ctx->n_chunks, rsplit), dim3(256), 0, st, ctx->d_msa, ctx->plane_stride,   \
                       ctx->n_cols, nt, ctx->d_chunks.as<const uint2>(), ctx->d_guess.as<const uint32_t>(), ctx->d_counts, ctx->d_hist)
    if (ctx->pileup_w == 6) JL_LAUNCH_PLANES(6, 2);
    else if (planes_nq(ctx, false) == 4) JL_LAUNCH_PLANES(3, 4);
    else JL_LAUNCH_PLANES(3, 2);
#undef JL_LAUNCH_PLANES
}

// (JL_NO_FOLD_CALL, one of the four environment switches of jl_internal.h: the separate call launch always, for A/B measurements)
bool jl_fold_enabled(void) { return !jl_env().no_fold_call; }
bool jl_pileup_can_fold(jl_ctx *ctx) { return jl_fold_enabled() && ctx->P != 0 && jl_pileup_rsplit(ctx) == 1u; }

void jl_fill_win_fold(jl_ctx *ctx, const jl_win_call *call, jl_win_fold *f)
{
    f->c = *call;
    f->col_head = ctx->d_col_head;
    f->pos_next = ctx->d_pos_next;
}

void jl_launch_pileup_fold(jl_ctx *ctx, hipStream_t st, const jl_win_call *call)
{
    jl_win_pileup w;
    jl_win_fold f;
    w.msa = ctx->d_msa;
    w.plane_stride = ctx->plane_stride;
    w.n_cols = ctx->n_cols;
    w.n_tiles = planes_tiles(ctx, false);
    w.n_chunks = ctx->n_chunks;
    w.pad_ = 0;
    w.chunks = ctx->d_chunks.as<const uint2>();
    w.guess32 = ctx->d_guess.as<const uint32_t>();
    w.counts = ctx->d_counts;
    w.hist = ctx->d_hist;
    jl_fill_win_fold(ctx, call, &f);
    if (ctx->pileup_w == 6) hipLaunchKernelGGL((pileup_fold_kernel<6, 2>), dim3(ctx->n_chunks, 1), dim3(256), 0, st, w, f);
    else if (planes_nq(ctx, false) == 4) hipLaunchKernelGGL((pileup_fold_kernel<3, 4>), dim3(ctx->n_chunks, 1), dim3(256), 0, st, w, f);
    else hipLaunchKernelGGL((pileup_fold_kernel<3, 2>), dim3(ctx->n_chunks, 1), dim3(256), 0, st, w, f);
}

int jl_launch_pileup_fold_group(jl_ctx *const *ctxs, uint32_t n_win, const jl_win_pileup *h_wins, const jl_win_fold *h_fold, uint32_t max_chunks, hipStream_t st)
{
    if (n_win == 0 || n_win > JL_GROUP_MAX) return JL_ERR_ARG;
    for (uint32_t k = 1; k < n_win; ++k)
        if (ctxs[k]->pileup_w != ctxs[0]->pileup_w) return JL_ERR_ARG;
    jl_pileup_fold_group_args args;
    memset(&args, 0, sizeof args);
    memcpy(args.w, h_wins, sizeof(jl_win_pileup) * n_win);
    memcpy(args.f, h_fold, sizeof(jl_win_fold) * n_win);
    if (ctxs[0]->pileup_w == 3) hipLaunchKernelGGL((pileup_fold_group_kernel<3, 4>), dim3(max_chunks, 1, n_win), dim3(256), 0, st, args);
    else hipLaunchKernelGGL((pileup_fold_group_kernel<6, 2>), dim3(max_chunks, 1, n_win), dim3(256), 0, st, args);
    return JL_OK;
}

void jl_fill_win_pileup(jl_ctx *ctx, jl_win_pileup *w)
{
    w->msa = ctx->d_msa;
    w->plane_stride = ctx->plane_stride;
    w->n_cols = ctx->n_cols;
    w->n_tiles = planes_tiles(ctx, true);
    w->n_chunks = ctx->n_chunks;
    w->pad_ = 0;
    w->chunks = ctx->d_chunks.as<const uint2>();
    w->guess32 = ctx->d_guess.as<const uint32_t>();
    w->counts = ctx->d_counts;
    w->hist = ctx->d_hist;
}

// Every window of a group must use the same chunk width; each is counted by ONE block per chunk whatever its
// depth (a single run would split very long columns over several blocks).
int jl_launch_pileup_group(jl_ctx *const *ctxs, uint32_t n_win, const jl_win_pileup *h_wins, uint32_t max_chunks, hipStream_t st)
{
    if (n_win == 0 || n_win > JL_GROUP_WINDOWS_MAX) return JL_ERR_ARG;
    for (uint32_t k = 1; k < n_win; ++k)
        if (ctxs[k]->pileup_w != ctxs[0]->pileup_w) return JL_ERR_ARG;
    jl_pileup_group_args args;
    memset(&args, 0, sizeof args);
    memcpy(args.w, h_wins, sizeof(jl_win_pileup) * n_win);
    if (ctxs[0]->pileup_w == 3) hipLaunchKernelGGL((pileup_planes_group_kernel<3, 4>), dim3(max_chunks, 1, n_win), dim3(256), 0, st, args);
    else hipLaunchKernelGGL((pileup_planes_group_kernel<6, 2>), dim3(max_chunks, 1, n_win), dim3(256), 0, st, args);
    return JL_OK;
}

// ---- runs that count from the deviation index: the index kernel over the plain chunks, the plane kernel over the rest (if any)
void jl_fill_win_index(jl_ctx *ctx, jl_win_index *w)
{
    w->msa = ctx->d_msa;
    w->plane_stride = ctx->plane_stride;
    w->n_reads = (uint32_t)ctx->n_reads;
    w->n_plain = ctx->ix_n_plain;
    w->tab = ctx->d_ix_tab;
    w->entries = ctx->d_ix_entries;
    w->seed = ctx->d_ix_seed;
    w->counts = ctx->d_counts;
    w->hist = ctx->d_hist;
}

void jl_fill_win_pileup_rest(jl_ctx *ctx, bool grouped, jl_win_pileup *w)
{
    jl_fill_win_pileup(ctx, w);
    w->n_tiles = planes_tiles(ctx, grouped);
    w->n_chunks = ctx->ix_n_rest;
    w->chunks = ctx->d_ix_rest.as<const uint2>();
}

// one window; `call` non-null: the Fisher stage in the epilogue (the caller has checked jl_pileup_can_fold).  The rest keeps the
// single run's launch shape (read splits, load width), so whoever zeroes the counters for it still does.
void jl_launch_pileup_index(jl_ctx *ctx, hipStream_t st, const jl_win_call *call)
{
    jl_win_index wi;
    jl_win_pileup w;
    jl_win_fold f;
    jl_fill_win_index(ctx, &wi);
    jl_fill_win_pileup_rest(ctx, false, &w);
    if (call) jl_fill_win_fold(ctx, call, &f);
    if (call) hipLaunchKernelGGL(pileup_index_fold_kernel, dim3(wi.n_plain), dim3(256), 0, st, wi, f);
    else hipLaunchKernelGGL(pileup_index_kernel, dim3(wi.n_plain), dim3(256), 0, st, wi);
    if (!w.n_chunks) return;
    const int nq = planes_nq(ctx, false);   // (an indexed window's chunk table is three columns wide)
    if (call) {
        if (nq == 4) hipLaunchKernelGGL((pileup_fold_kernel<3, 4>), dim3(w.n_chunks, 1), dim3(256), 0, st, w, f);
        else hipLaunchKernelGGL((pileup_fold_kernel<3, 2>), dim3(w.n_chunks, 1), dim3(256), 0, st, w, f);
    } else {
        const uint32_t rsplit = jl_pileup_rsplit(ctx);
        if (nq == 4) hipLaunchKernelGGL((pileup_planes_kernel<3, 4>), dim3(w.n_chunks, rsplit), dim3(256), 0, st, w.msa, w.plane_stride, w.n_cols, w.n_tiles, w.chunks, w.guess32, w.counts, w.hist);
        else hipLaunchKernelGGL((pileup_planes_kernel<3, 2>), dim3(w.n_chunks, rsplit), dim3(256), 0, st, w.msa, w.plane_stride, w.n_cols, w.n_tiles, w.chunks, w.guess32, w.counts, w.hist);
    }
}

// the index kernel for the windows of one chunk of a group (h_fold non-null: folded); the plane launch over their rest tables is the caller's
int jl_launch_pileup_index_group(jl_ctx *const *ctxs, uint32_t n_win, const jl_win_index *h_wins, const jl_win_fold *h_fold, uint32_t max_plain, hipStream_t st)
{
    (void)ctxs;
    if (n_win == 0 || n_win > JL_GROUP_MAX || max_plain == 0) return JL_ERR_ARG;
    if (h_fold) {
        jl_index_fold_group_args args;
        memset(&args, 0, sizeof args);
        memcpy(args.w, h_wins, sizeof(jl_win_index) * n_win);
        memcpy(args.f, h_fold, sizeof(jl_win_fold) * n_win);
        hipLaunchKernelGGL(pileup_index_fold_group_kernel, dim3(max_plain, 1, n_win), dim3(256), 0, st, args);
    } else {
        jl_index_group_args args;
        memset(&args, 0, sizeof args);
        memcpy(args.w, h_wins, sizeof(jl_win_index) * n_win);
        hipLaunchKernelGGL(pileup_index_group_kernel, dim3(max_plain, 1, n_win), dim3(256), 0, st, args);
    }
    return JL_OK;
}

#ifdef JL_TUNING
// test hook of the -DJL_TUNING build (beside jl_tuning_group_forms, capi_group.hip): the launch shape of a context whose plan is
// built, so that a test knows which kernel form it ran.  out[0..11] = chunk width; NQ and tiles of a single run; NQ and tiles of a
// grouped run; n_chunks; read splits of a single run (gridDim.y); can_fold; resident blocks per CU of the single run's kernel;
// chunks on the fast stream; chunks that load their halo; tiles per flush batch of a single run.
extern "C" __attribute__((visibility("default"))) int jl_tuning_pileup_shape(jl_ctx *ctx, uint32_t *out)
{
    if (!ctx || !out || !ctx->plan_valid) return JL_ERR_ARG;
    std::vector<uint2> recs(ctx->n_chunks);
    if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess ||
        (ctx->n_chunks && hipMemcpy(recs.data(), ctx->d_chunks.as<const uint2>(), recs.size() * sizeof(uint2), hipMemcpyDeviceToHost) != hipSuccess))
        return JL_ERR_DEVICE;
    uint32_t n_fast = 0, n_halo = 0;
    for (const uint2 &r : recs) {
        n_fast += ctx->pileup_w == 3 && r.y == JL_CHUNK_META(3, 1, 0);
        n_halo += (r.y >> 16) & 1u;
    }
    const uint32_t v[12] = {ctx->pileup_w, (uint32_t)planes_nq(ctx, false), planes_tiles(ctx, false), (uint32_t)planes_nq(ctx, true),
                            planes_tiles(ctx, true), ctx->n_chunks, jl_pileup_rsplit(ctx), (uint32_t)jl_pileup_can_fold(ctx),
                            (uint32_t)ctx->pileup_blocks_per_cu[planes_slot(ctx)], n_fast, n_halo, plane_flush_tiles(planes_nq(ctx, false))};
    memcpy(out, v, sizeof v);
    return JL_OK;
}
#endif
