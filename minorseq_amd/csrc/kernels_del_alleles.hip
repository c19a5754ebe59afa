// kernels_del_alleles.hip — the deletions of the resident matrix by extent (jl_deletion_alleles_async; docs/SPEC.md §25): every
// read's maximal runs of '-' (code 4), the bounded ones grouped exactly by (start column, length), the open ones counted per column.
// A read is one bit position in every plane row, so per 32 reads a column is three words and
//   is4 = b2 & ~b1 & ~b0          the cells that are '-'
//   unc = b2 & b1                 the uncovered cells (code 6)
//   start(c) = valid & is4(c) & ~is4(c - 1)      valid: the bits of the word that are reads (jl_valid_bits), is4(-1) = 0
// RUNS (deletion_runs_kernel).  A lane owns a WORD of 32 reads, a wave is a workgroup and owns 64 consecutive words (2048 reads: a
// wave's load of a plane row is 256 contiguous bytes) and a SEGMENT of columns; the grid is (word group, column segment).  The
// wave walks its segment's columns in order, four columns' loads (twelve) in flight at a time, with the column before the segment
// as a halo of one.  kCount: it only counts the starts — their total bounds the number of distinct alleles, the host sizes the
// table from it.  Otherwise, at a column s where any lane holds a start the WAVE follows all of them together: c = s + 1, s + 2, …
// while any lane's mask & is4(c) is left (a lane without a bit left loads nothing); the bits that drop out at c end there with
// len = c - s.  Such a run is open when s == 0, c == n_cols, or its bit is uncovered at s - 1 or at c; bounded otherwise.  Every
// run that ends in one step of a wave has the same s and the same c, hence the same key: the wave sums its lanes' popcounts and
// lane 0 alone adds them — an allele carried by a quarter of the reads costs an atomic a wave, not a read.  A run that begins in
// this segment is followed to its end wherever that lies; one that began before it is not this wave's.
// The bounded ones go into an open-addressing table of `slots` entries keyed col << 32 | len, all ones when empty (no key can
// be: col < n_cols), claimed by a 64-bit compare-and-swap with linear probing from a hash of the key — kernels_ins.hip's scheme
// with one key word.  A slot's key only ever changes from empty to its final value, so two waves with one key stop at the same
// slot: grouping is on the full key.  The wave whose swap claimed a slot lists it in occ[].  The host sizes the table at twice
// the distinct alleles there can be or more, so it is never more than half full and a probe always ends; the walk is bounded by
// the table's size all the same.  The open ones go into diff[]: + k at s, - k at c, modulo 2^32; open[c] is the prefix sum (the
// fetch forms it) — two atomics an open run however long it is.
// FLANKS (deletion_rows_kernel).  A workgroup per listed slot, striding over the list whose length only the device knows: the
// reads covered at s - 1 and at s + len (not plane 2 and plane 1), four plane rows, and the row {col, len, count, flank} written
// whole.  The list's order is the order in which the slots were claimed; the fetch sorts the rows.
// Every address is formed from sizes the host checked (capi_del_alleles.hip): a word w < n_words with 4 n_words <= plane_stride, a
// plane row < 3 n_cols.  Loads are typed as global memory.
#include <algorithm>

#include "jl_internal.h"
#include "planes.h"

namespace {

constexpr unsigned long long kEmptyKey = ~0ull;
constexpr uint32_t kBatch = 4;          // columns whose loads are in flight together

struct cell {
    uint32_t is4, unc;
};

__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// this lane's word of column c < n_cols; `base` = the word's bytes in plane row 0
__device__ __forceinline__ cell load_cell(const uint8_t JL_AS1 *base, uint64_t plane_stride, uint32_t c)
{
    const uint8_t JL_AS1 *p = base + 3ull * c * plane_stride;
    const uint32_t b0 = *(const uint32_t JL_AS1 *)p;
    const uint32_t b1 = *(const uint32_t JL_AS1 *)(p + plane_stride);
    const uint32_t b2 = *(const uint32_t JL_AS1 *)(p + 2u * plane_stride);
    return cell{b2 & ~b1 & ~b0, b2 & b1};
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (uint32_t d = 32u; d; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// `cnt` reads more of allele `key`
__device__ __forceinline__ void table_add(const jl_dal_args &a, unsigned long long key, uint32_t cnt)
{
    uint64_t s = mix64(key + 0x9E3779B97F4A7C15ull) & a.slots_mask;
    for (uint64_t probe = 0; probe <= a.slots_mask; ++probe, s = (s + 1u) & a.slots_mask) {
        unsigned long long o = __hip_atomic_load(&a.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (o == kEmptyKey) {
            o = atomicCAS(&a.keys[s], kEmptyKey, key);
            if (o == kEmptyKey) {
                const uint32_t at = atomicAdd(a.n_occ, 1u);
                if (at < a.occ_cap) a.occ[at] = (uint32_t)s;   // (never beyond: the host's bound on the distinct alleles)
                o = key;
            }
        }
        if (o != key) continue;
        atomicAdd(&a.count[s], cnt);
        return;
    }
}

// grid: x = group of 64 words (2048 reads), y = column segment of `seg_cols` columns
template <bool kCount>
__global__ __launch_bounds__(64) void deletion_runs_kernel(jl_dal_args a)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t w = blockIdx.x * 64u + lane;
    const bool live = w < a.n_words;
    const uint32_t valid = live ? jl_valid_bits(a.n_reads, w) : 0u;
    const uint32_t c0 = blockIdx.y * a.seg_cols, c1 = min(c0 + a.seg_cols, a.n_cols);
    const uint8_t JL_AS1 *base = (const uint8_t JL_AS1 *)a.msa + 4ull * w;   // (formed for a live lane's loads only)

    cell prev{0u, 0xFFFFFFFFu};    // before column 0: no '-', and nothing covered
    if (c0 && live) prev = load_cell(base, a.plane_stride, c0 - 1u);
    unsigned long long n_starts = 0, n_bounded = 0, n_open = 0;   // n_bounded, n_open: lane 0's

    for (uint32_t cb = c0; cb < c1; cb += kBatch) {
        cell x[kBatch];
#pragma unroll
        for (uint32_t j = 0; j < kBatch; ++j) x[j] = live && cb + j < c1 ? load_cell(base, a.plane_stride, cb + j) : cell{0u, 0u};
#pragma unroll
        for (uint32_t j = 0; j < kBatch; ++j) {
            const uint32_t s = cb + j;
            if (s >= c1) break;    // (wave-uniform)
            uint32_t m = valid & x[j].is4 & ~prev.is4;
            const uint32_t open_left = prev.unc;
            prev = x[j];
            if constexpr (kCount) {
                n_starts += __popc(m);
                continue;
            }
            if (!__ballot(m != 0u)) continue;
            for (uint32_t c = s + 1u;; ++c) {   // wave-uniform: one round per column until the wave's longest run has ended
                uint32_t ended = m, unc_c = 0xFFFFFFFFu;   // at n_cols everything ends, open
                if (c < a.n_cols && m) {
                    const cell y = load_cell(base, a.plane_stride, c);
                    ended = m & ~y.is4, unc_c = y.unc;
                }
                m &= ~ended;
                if (__ballot(ended != 0u)) {
                    const uint32_t opn = ended & (open_left | unc_c);
                    const uint32_t kb = wave_sum(__popc(ended & ~opn)), ko = wave_sum(__popc(opn));
                    if (lane == 0u) {
                        if (kb) {
                            table_add(a, (unsigned long long)s << 32 | (c - s), kb);
                            n_bounded += kb;
                        }
                        if (ko) {
                            atomicAdd(&a.diff[s], ko);
                            atomicAdd(&a.diff[c], 0u - ko);    // (c <= n_cols: diff has n_cols + 1 words)
                            n_open += ko;
                        }
                    }
                }
                if (!__ballot(m != 0u)) break;
            }
        }
    }

    if constexpr (kCount) {
        const uint32_t lo = wave_sum((uint32_t)n_starts);   // (a lane's starts: at most 32 a column, far below 2^32 / 64)
        if (lane == 0u && lo) atomicAdd(a.n_starts, (unsigned long long)lo);
    } else if (lane == 0u) {
        if (n_bounded) atomicAdd(&a.runs[0], n_bounded);
        if (n_open) atomicAdd(&a.runs[1], n_open);
    }
}

// grid: any x; workgroup b takes the listed slots b, b + gridDim.x, ...
__global__ __launch_bounds__(256) void deletion_rows_kernel(jl_dal_args a, jl_deletion_allele *__restrict__ rows)
{
    __shared__ uint32_t s_part[4];
    const uint32_t n = min(*a.n_occ, a.occ_cap);
    const uint8_t JL_AS1 *msa = (const uint8_t JL_AS1 *)a.msa;
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const uint32_t slot = a.occ[i];
        const unsigned long long key = a.keys[slot];
        const uint32_t s = (uint32_t)(key >> 32), len = (uint32_t)key;
        uint32_t flank = 0u;
        if (s >= 1u && (uint64_t)s + len < a.n_cols) {   // (a bounded run's: the rows at s - 1 and s + len exist)
            const uint8_t JL_AS1 *l1 = msa + (3ull * (s - 1u) + 1u) * a.plane_stride, *r1 = msa + (3ull * (s + len) + 1u) * a.plane_stride;
            for (uint32_t w = threadIdx.x; w < a.n_words; w += 256u) {
                const uint32_t x1 = *(const uint32_t JL_AS1 *)(l1 + 4ull * w), x2 = *(const uint32_t JL_AS1 *)(l1 + a.plane_stride + 4ull * w);
                const uint32_t y1 = *(const uint32_t JL_AS1 *)(r1 + 4ull * w), y2 = *(const uint32_t JL_AS1 *)(r1 + a.plane_stride + 4ull * w);
                flank += __popc(jl_valid_bits(a.n_reads, w) & ~((x1 & x2) | (y1 & y2)));
            }
        }
        flank = wave_sum(flank);
        if ((threadIdx.x & 63u) == 0u) s_part[threadIdx.x >> 6] = flank;
        __syncthreads();
        if (threadIdx.x == 0u) {
            jl_deletion_allele row;
            row.col = s, row.len = len, row.count = a.count[slot];
            row.flank = s_part[0] + s_part[1] + s_part[2] + s_part[3];
            rows[i] = row;
        }
        __syncthreads();
    }
}

// columns of a segment: word groups x segments fill the chip a few times over; a multiple of the batch
uint32_t seg_cols_for(uint32_t n_wgroups, uint32_t n_cols)
{
    const uint32_t want_blocks = 4096u;   // 256 CUs x 8 one-wave workgroups, twice
    const uint32_t segs = std::max(1u, want_blocks / std::max(1u, n_wgroups));
    const uint32_t cols = std::max(2u * kBatch, (n_cols + segs - 1u) / segs);
    return (cols + kBatch - 1u) / kBatch * kBatch;
}

template <bool kCount>
void launch_runs(const jl_dal_args *a, hipStream_t st)
{
    jl_dal_args A = *a;
    const uint32_t n_wgroups = (A.n_words + 63u) / 64u;
    A.seg_cols = seg_cols_for(n_wgroups, A.n_cols);
    hipLaunchKernelGGL(deletion_runs_kernel<kCount>, dim3(n_wgroups, (A.n_cols + A.seg_cols - 1u) / A.seg_cols), dim3(64), 0, st, A);
}

}  // namespace

// *a->n_starts zeroed; n_reads > 0, n_cols >= 1
void jl_launch_deletion_starts(const jl_dal_args *a, hipStream_t st) { launch_runs<true>(a, st); }

// a->runs, a->diff, a->count, *a->n_occ zeroed, the keys all ones
void jl_launch_deletion_runs(const jl_dal_args *a, hipStream_t st) { launch_runs<false>(a, st); }

// rows [a->occ_cap]
void jl_launch_deletion_rows(const jl_dal_args *a, jl_deletion_allele *rows, hipStream_t st)
{
    const uint32_t blocks = std::max(1u, std::min(a->occ_cap, 2048u));
    hipLaunchKernelGGL(deletion_rows_kernel, dim3(blocks), dim3(256), 0, st, *a, rows);
}
