// kernels_ins.hip — the in-frame insertion alleles of a record build (jl_msa_track_insertion_alleles; docs/SPEC.md §17): which
// inserted sequences the reads carry at every junction of the window, how many reads carry each, and out of how many.
//
// RECORD WALK (insertion_alleles_kernel).  A lane owns a read and walks its cigar, as insertions_kernel (kernels_util.hip) does.
// Between two non-empty reference-consuming ops it gathers the bases of ALL 'I' ops — 'S', 'H', 'P' and empty ops do not separate
// them — up to 30 of them as 2-bit codes in one 64-bit word, and whether each was readable (exactly A, C, G or T, and past the QV
// filter in force: quality bytes, a bit per base, or none, as the planes kernel has it).  When the second of the two ops arrives
// and both are D, = or X (not N) and the junction c lies in 1 .. n_cols - 1, the read has an EVENT at c of one of three kinds:
// in-frame and readable (an allele), out of frame, in frame but too long or unreadable.
// Events are counted a wave at a time: every lane advances to its next event, then the wave groups its (at most 64) events by the
// FULL key — junction, kind, length, sequence: two 64-bit words, compared as they are — and the first lane of every group adds the
// group's size with one atomic.  One allele carried by every read — a true variant — costs an atomic a wave, not a read.
// The alleles go into an open-addressing table of `slots` entries, keyed by the two words: key0 = c << 32 | length, key1 =
// sequence, both all ones when empty (neither word of a key can be: c < n_cols, the sequence has 60 bits).  A slot is claimed by a
// 64-bit compare-and-swap on key0, THEN on key1: a thread that finds its key0 in a slot swaps its key1 in if that is still empty
// and owns the slot when the swap returns empty or its own key1; anything else is another key's slot, on to the next (linear
// probing from a hash of both words).  Nobody waits for anybody: the thread that claimed key0 may find another key1 there — one
// with the same junction and length — and moves on as well.  Both words of a slot only ever change from empty to their final
// value, so two threads with one key stop at the same slot: the grouping is exact, never by hash equality.  The thread whose swap
// claimed key0 lists the slot in occ[].  The host sizes the table at twice the records' 'I' ops or more (an event needs one), so
// it is never more than half full and a probe always ends; the walk is bounded by the table's size all the same.
// Everything a lane reads lies inside its read's own bytes: a base index is checked against the read's bases, a quality index
// against its qualities (a record whose cigar consumes more than it holds is refused by the build's verdict anyway).
// EVENTS (the kEvents instantiation: jl_msa_track_insertion_reads, docs/SPEC.md §19).  In the round where lanes hold an event, the
// first of them reserves popc(todo) rows of a->events with ONE atomic add on *a->n_events, and every lane with an event writes its
// own row at base + its rank among them — an atomic a wave round, not a read.  The counter counts every event; a row at or beyond
// events_cap is never written (the host sizes the rows by the records' 'I' ops: an event needs one).  The other instantiation
// holds none of this.
//
// SPAN PASS (junction_span_kernel).  span[c] = reads whose cells at c - 1 and c are both covered (code != 6, i.e. not plane 2 and
// plane 1 both set).  The tile walk of plane_walk.h with two planes and a halo of one: a lane owns a junction, and staged are the
// planes 1 and 2 of the group's 65 columns, a column's two rows next to each other in LDS (span_cols).  The loads of the next
// tile are issued before the current one is counted.
#include "jl_internal.h"
#include "plane_walk.h"

namespace {

using namespace jl_walk;

constexpr unsigned long long kEmptyKey = ~0ull;
constexpr uint32_t kInframe = 1u, kFrameshift = 2u, kUnread = 3u;   // an event's kind: its column of jcnt

__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// `cnt` reads more of allele (k0, k1)
__device__ __forceinline__ void table_add(const jl_insal_args &a, unsigned long long k0, unsigned long long k1, uint32_t cnt)
{
    uint64_t s = mix64(mix64(k0 + 0x9E3779B97F4A7C15ull) ^ k1) & a.slots_mask;
    for (uint64_t probe = 0; probe <= a.slots_mask; ++probe, s = (s + 1u) & a.slots_mask) {
        unsigned long long o0 = __hip_atomic_load(&a.key0[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (o0 == kEmptyKey) {
            o0 = atomicCAS(&a.key0[s], kEmptyKey, k0);
            if (o0 == kEmptyKey) {
                a.occ[atomicAdd(a.n_occ, 1u)] = (uint32_t)s;   // (at most `slots` of them: one a slot)
                o0 = k0;
            }
        }
        if (o0 != k0) continue;
        unsigned long long o1 = __hip_atomic_load(&a.key1[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (o1 == kEmptyKey) {
            o1 = atomicCAS(&a.key1[s], kEmptyKey, k1);
            if (o1 == kEmptyKey) o1 = k1;
        }
        if (o1 != k1) continue;
        atomicAdd(&a.count[s], cnt);
        return;
    }
}

template <bool kEvents>
__global__ __launch_bounds__(256) void insertion_alleles_kernel(jl_insal_args a)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t k = 0, k_end = 0, n_bases = 0, n_quals = 0, so = 0, qo = 0;
    int64_t c = 0;          // window column of the next reference base
    uint64_t qp = 0;        // query offset of the next base
    if (r < a.n_reads) {
        k = a.cig_off[r], k_end = a.cig_off[r + 1];
        so = a.seq_off[r], n_bases = (a.seq_off[r + 1] - so) * 2u;
        if (a.qual) qo = a.qual_off[r], n_quals = a.qual_off[r + 1] - qo;
        c = (int64_t)a.pos[r] - (int64_t)a.win_begin;
    }
    uint32_t prev = 0;      // the last non-empty reference-consuming op: 0 none yet, 1 D = X, 2 N
    uint64_t len_acc = 0, seq = 0;   // the insertion being gathered: its length so far, its first 30 bases
    bool bad = false;                // ... one of them unreadable

    for (;;) {   // wave-uniform: one round per event of the lane with the most
        bool have = false;
        unsigned long long k0 = 0, k1 = 0;
        uint32_t kind = 0, col = 0;
        while (k < k_end && !have) {
            const uint32_t w = a.cigar[k++];
            const uint32_t op = w & 15u, len = w >> 4;
            if (len == 0u) continue;
            if (op == 1u) {
                for (uint32_t j = 0; j < len && len_acc + j < JL_INSAL_MAX_BASES; ++j) {
                    const uint64_t q = qp + j;
                    uint32_t b = 5u;
                    if (q < n_bases) {
                        const uint32_t by = a.seq4[so + (q >> 1)];
                        const uint32_t b16 = (q & 1u) ? (by & 15u) : (by >> 4);
                        b = (uint32_t)((0x5555555355525105ull >> (4u * b16)) & 15ull);   // A=1 C=2 G=4 T=8 -> 0..3, else 5
                        if (a.qual) {
                            const uint32_t qv = q < n_quals ? a.qual[qo + q] : 0u;
                            if (qv != 0xFFu && qv < a.min_qv) b = 5u;
                        }
                        if (a.qmask) {
                            const uint64_t i = 2u * so + q;      // (the mask is laid out by the resident bases: a bit a nibble)
                            if ((a.qmask[i >> 3] >> (uint32_t)(i & 7u)) & 1u) b = 5u;
                        }
                    }
                    if (b < 4u) seq |= (uint64_t)b << (2u * (uint32_t)(len_acc + j));
                    else bad = true;
                }
                len_acc += len;
                qp += len;
            } else if (op == 4u) {
                qp += len;
            } else if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) {   // ('M' is refused by the build: walked as '=')
                const uint32_t now = op == 3u ? 2u : 1u;
                if (len_acc) {
                    if (prev == 1u && now == 1u && c >= 1 && c < (int64_t)a.n_cols) {
                        have = true;
                        col = (uint32_t)c;
                        kind = len_acc % 3u != 0u ? kFrameshift : (len_acc > JL_INSAL_MAX_BASES || bad) ? kUnread : kInframe;
                        k0 = (unsigned long long)col << 32 | (kind == kInframe ? (unsigned long long)len_acc : 0ull);
                        k1 = kind == kInframe ? seq : 0ull;
                    }
                    len_acc = 0, seq = 0, bad = false;
                }
                prev = now;
                c += len;
                if (op != 2u && op != 3u) qp += len;
                if (c >= (int64_t)a.n_cols) k = k_end;   // every junction to come lies beyond the window
            }
        }
        uint64_t todo = __ballot(have);
        if (!todo) break;   // no lane has an event: every lane has reached its cigar's end
        if constexpr (kEvents) {
            const int first = __ffsll((unsigned long long)todo) - 1;
            uint32_t base = 0;
            if ((int)lane == first) base = atomicAdd(a.n_events, (uint32_t)__popcll(todo));
            base = __shfl(base, first, 64);
            const uint64_t row = (uint64_t)base + (uint32_t)__popcll(todo & ((1ull << lane) - 1ull));
            if (have && row < a.events_cap) {
                jl_insertion_event ev;
                ev.read = (uint32_t)r, ev.col = col, ev.len = (uint32_t)k0, ev.kind = kind;   // (k0's low word: the length of an allele, else 0)
                ev.seq = k1;
                a.events[row] = ev;
            }
        }
        while (todo) {      // wave-uniform: one round per distinct event of the wave
            const int leader = __ffsll((unsigned long long)todo) - 1;
            const unsigned long long l0 = __shfl(k0, leader, 64), l1 = __shfl(k1, leader, 64);
            const uint32_t lkind = __shfl(kind, leader, 64);
            const uint64_t grp = __ballot(have && k0 == l0 && k1 == l1 && kind == lkind);
            if ((int)lane == leader) {
                const uint32_t cnt = (uint32_t)__popcll(grp);
                atomicAdd(&a.jcnt[(uint64_t)col * 4u + kind], cnt);
                if (kind == kInframe) table_add(a, k0, k1, cnt);
            }
            todo &= ~grp;
        }
    }
}

__global__ __launch_bounds__(256) void insertion_rows_kernel(const unsigned long long *__restrict__ key0, const unsigned long long *__restrict__ key1,
                                                             const uint32_t *__restrict__ count, const uint32_t *__restrict__ occ, uint32_t n,
                                                             jl_insertion_allele *__restrict__ rows)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = occ[i];
    jl_insertion_allele row;
    row.col = (uint32_t)(key0[s] >> 32), row.len = (uint32_t)key0[s];
    row.seq = key1[s];
    row.count = count[s], row.pad_ = 0u;
    rows[i] = row;
}

// ---------------------------------------------------------------------------------------- span
constexpr uint32_t kJunctions = 64;     // junctions of a group: one a lane
constexpr uint32_t kCols = kJunctions + 1u;          // columns staged: the junctions' own and the one before the first
constexpr uint32_t kRows = 2u * kCols;               // ... their planes 1 and 2

// the layout of the span's tile: staged row 2 k + p is plane 1 + p of column cb + k, the first n_here columns exist
struct span_cols {
    static constexpr uint32_t kColVec = 9;   // a staged column in LDS, in 16-byte units: plane 1 (4), plane 2 (4), 1 of padding
    uint32_t cb, n_here;
    __device__ __forceinline__ bool exists(uint32_t r) const { return (r >> 1) < n_here; }
    __device__ __forceinline__ uint64_t plane_row(uint32_t r) const { return 3ull * (cb + (r >> 1)) + 1u + (r & 1u); }
    __device__ __forceinline__ static constexpr uint32_t slot(uint32_t r) { return (r >> 1) * kColVec + (r & 1u) * 4u; }
};

// grid: x = group of 64 junctions (junction cb + 1 + lane, cb = 64 x), y = read segment of `seg_tiles` tiles
__global__ __launch_bounds__(64) void junction_span_kernel(jl_insal_span_args a)
{
    __shared__ u32x4 s_cols[span_cols::slot(kRows)];
    const uint32_t lane = threadIdx.x;
    const uint32_t cb = blockIdx.x * kJunctions;
    const range seg = segment(a.n_reads, a.seg_tiles);
    const span_cols staged{cb, min(kCols, a.n_cols - cb)};   // ... the columns of this group that exist
    const uint8_t JL_AS1 *planes = (const uint8_t JL_AS1 *)a.msa;

    uint32_t span = 0u;
    tile<kRows, span_cols> v;
    if (seg.t0 < seg.t1) v.load(staged, planes, a.plane_stride, seg.t0, lane);
    for (uint32_t t = seg.t0; t < seg.t1; ++t) {
        v.store(s_cols, lane);
        if (t + 1u < seg.t1) v.load(staged, planes, a.plane_stride, t + 1u, lane);   // in flight while this tile is counted
#pragma unroll
        for (uint32_t q = 0; q < kTileWords / 4u; ++q) {
            const u32x4 x1 = s_cols[span_cols::slot(2u * lane) + q], x2 = s_cols[span_cols::slot(2u * lane + 1u) + q];        // column c - 1
            const u32x4 y1 = s_cols[span_cols::slot(2u * lane + 2u) + q], y2 = s_cols[span_cols::slot(2u * lane + 3u) + q];   // column c
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) {
                const uint32_t valid = jl_valid_bits(a.n_reads, t * kTileWords + 4u * q + j);   // (wave-uniform)
                span += __popc(valid & ~((x1[j] & x2[j]) | (y1[j] & y2[j])));
            }
        }
    }
    const uint64_t c = (uint64_t)cb + 1u + lane;
    if (c < a.n_cols && span) atomicAdd(a.jcnt + c * 4u, span);
}

}  // namespace

// a->jcnt, a->count, *a->n_occ zeroed, the keys all ones; a->n_reads > 0; with a->events: *a->n_events zeroed
void jl_launch_insertion_alleles(const jl_insal_args *a, hipStream_t st)
{
    const dim3 grid((uint32_t)((a->n_reads + 255u) / 256u));
    if (a->events) hipLaunchKernelGGL(insertion_alleles_kernel<true>, grid, dim3(256), 0, st, *a);
    else hipLaunchKernelGGL(insertion_alleles_kernel<false>, grid, dim3(256), 0, st, *a);
}

void jl_launch_insertion_rows(const unsigned long long *key0, const unsigned long long *key1, const uint32_t *count, const uint32_t *occ,
                              uint32_t n, jl_insertion_allele *rows, hipStream_t st)
{
    hipLaunchKernelGGL(insertion_rows_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, key0, key1, count, occ, n, rows);
}

// a->n_cols >= 2
void jl_launch_junction_span(const jl_insal_span_args *a, hipStream_t st)
{
    jl_insal_span_args A = *a;
    const uint32_t n_groups = (A.n_cols - 1u + kJunctions - 1u) / kJunctions;
    const jl_walk_shape shape = jl_walk_shape_for(A.n_reads, n_groups);
    A.seg_tiles = shape.seg_tiles;
    hipLaunchKernelGGL(junction_span_kernel, dim3(n_groups, shape.n_segs), dim3(64), 0, st, A);
}
