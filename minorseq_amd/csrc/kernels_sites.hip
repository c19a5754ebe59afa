// kernels_sites.hip — the site matrix of jl_sites_assemble (docs/SPEC.md §18): site k of the table becomes columns 3k..3k+2 of the
// destination, the three source columns at its `col` with the reads of two of §16's classes RECODED so that the phasing that
// follows groups over codon and deletion sites alike:
//   JL_SITE_DELETION         codon reads -> A A A (codon JL_SITE_PRESENT), del3 reads -> A A C (codon JL_SITE_DELETED), others copied
//   JL_SITE_CODON, fill f    del3 reads -> the three bases of codon f, others copied;  fill JL_SITE_NO_FILL: all copied
// A read is one bit position in every plane row, so per 32 reads the classes are bit words, kernels_del.hip's:
//   b2 of a column = its cells with code 4, 5 or 6;  b2 & b1 = uncovered (6);  b2 & b0 = N once the uncovered ones are out
//   codon = ~(b2 | b2 | b2)        del3 = (b2 & b2 & b2) & ~(uncovered of any) & ~(N of any)
// and a destination plane word is one select:  (source & ~(zeroed | del3')) | (del3' where the recoded codon has the bit),
// zeroed = codon reads of a deletion site, del3' = del3 where the site recodes them.
// Shape: nothing is shared between reads or between sites, so a lane owns one 16-byte piece (128 reads) of ONE site: nine
// non-temporal 16-byte loads (the nine plane rows 3 col .. 3 col + 8 of the source lie one after the other), nine 16-byte stores;
// consecutive lanes take consecutive pieces, a wave 1 KB of every row.  The grid is (pieces / 256, sites): the site is
// blockIdx.y, its table entry a wave-uniform load.  No LDS.  18 n_sites dst_stride bytes move in all.
// Addresses are formed from the sizes the host checked only (capi_sites.hip): a load reads source row 3 col + r < 3 n_cols at
// bytes [at, at + 16) with at + 16 <= src_stride; a store writes destination row 9 k + r < 9 n_sites at [at, at + 16) with
// at + 16 <= dst_stride.  Bytes of a source row that do not exist (its stride is its own: an adopted matrix) read as
// uncovered; the bits of a word at or beyond n_reads — padding, and whatever an adopted source holds there — are cut by `valid`
// and written as code 6 (plane 0 clear, planes 1 and 2 set) out to the end of every destination row.
//
// INSERTION SITES (jl_sites_assemble_alleles; docs/SPEC.md §19).  A site of kind JL_SITE_INSERTION is none of that kernel's (its
// workgroups leave at once).  Its nine rows are made in two launches behind it:
//   sites_ins_init_kernel     the same shape over the insertion sites only: a lane owns a 16-byte piece of one site and reads the
//                             planes 1 and 2 of source columns c - 1 and c (four loads).  A read that does not span the junction
//                             (either cell is code 6), a bit at or beyond n_reads, a source byte that does not exist: code 6;
//                             every other read: all nine bits zero (A A A, codon JL_SITE_INS_NONE).
//   sites_ins_scatter_kernel  a thread an event of the source's record build.  Its column is searched among the insertion sites
//                             (ascending, at most 4096: a binary search in global memory), its allele among the site's (ascending
//                             by length, sequence); the nine-bit code of the read — the bases of codon 1 + rank, T T T for an
//                             allele that is not listed, 4 4 4 for a frame-shifting and 5 5 5 for an unreadable insertion — is
//                             ORed into the read's bit of the nine rows, 32 bits at a time.  The cells of a spanning read are zero
//                             and a read has one event a junction, so OR writes the code whatever the order.
// The scatter forms its addresses from read < n_reads (checked), the site index and allele range of the host's table, and
// dst_stride >= ceil(n_reads / 8) rounded up to 16; an event is read only below min(*n_events, events_cap).
#include "jl_internal.h"
#include "planes.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kLanes = 256;   // pieces a workgroup takes of one site: 4 KB of each of its nine rows

// grid: x = run of 256 pieces of 16 bytes, y = site
__global__ __launch_bounds__(kLanes) void sites_assemble_kernel(jl_sites_args a)
{
    const uint32_t k = blockIdx.y;
    const uint64_t piece = (uint64_t)blockIdx.x * kLanes + threadIdx.x;
    const uint64_t at = piece * 16u;
    if (at + 16u > a.dst_stride) return;
    const jl_site s = a.sites[k];   // (wave-uniform)
    if (s.kind == JL_SITE_INSERTION) return;   // (sites_ins_init_kernel's)
    const uint32_t is_del = s.kind == JL_SITE_DELETION ? 0xFFFFFFFFu : 0u;
    const uint32_t recode = (s.kind == JL_SITE_DELETION || s.fill != JL_SITE_NO_FILL) ? 0xFFFFFFFFu : 0u;
    const uint32_t val = s.kind == JL_SITE_DELETION ? (uint32_t)JL_SITE_DELETED : (uint32_t)(s.fill & 63u);   // the codon del3 reads become

    // p[3 j + b] = plane b of column col + j
    u32x4 p[9];
    const uint8_t JL_AS1 *src = (const uint8_t JL_AS1 *)a.src + 3ull * s.col * a.src_stride + at;
    const bool have = at + 16u <= a.src_stride;
#pragma unroll
    for (uint32_t r = 0; r < 9u; ++r) {
        const uint32_t none = (r % 3u) ? 0xFFFFFFFFu : 0u;   // code 6
        p[r] = u32x4{none, none, none, none};
        if (have) p[r] = __builtin_nontemporal_load((const u32x4 JL_AS1 *)(src + (uint64_t)r * a.src_stride));
    }

    u32x4 o[9];
#pragma unroll
    for (uint32_t w = 0; w < 4u; ++w) {
        const uint32_t valid = jl_valid_bits(a.n_reads, 4u * piece + w);
        const uint32_t x0 = p[0][w], x1 = p[1][w], x2 = p[2][w];
        const uint32_t y0 = p[3][w], y1 = p[4][w], y2 = p[5][w];
        const uint32_t z0 = p[6][w], z1 = p[7][w], z2 = p[8][w];
        const uint32_t any2 = x2 | y2 | z2, all2 = x2 & y2 & z2;
        const uint32_t in = ~((x2 & x1) | (y2 & y1) | (z2 & z1));      // no uncovered cell
        const uint32_t clean = in & ~((x2 & x0) | (y2 & y0) | (z2 & z0));   // ... and no N: bases and '-' only
        const uint32_t del3 = clean & all2 & recode;
        const uint32_t keep = ~((~any2 & is_del) | del3);
#pragma unroll
        for (uint32_t j = 0; j < 3u; ++j) {
            const uint32_t base = (val >> (4u - 2u * j)) & 3u;   // base j of the codon: index 16 s0 + 4 s1 + s2
#pragma unroll
            for (uint32_t b = 0; b < 3u; ++b) {
                const uint32_t set = (b < 2u && ((base >> b) & 1u)) ? del3 : 0u;
                const uint32_t v = (p[3u * j + b][w] & keep) | set;
                o[3u * j + b][w] = (v & valid) | (b ? ~valid : 0u);
            }
        }
    }

    uint8_t JL_AS1 *dst = (uint8_t JL_AS1 *)a.dst + 9ull * k * a.dst_stride + at;
#pragma unroll
    for (uint32_t r = 0; r < 9u; ++r) *(u32x4 JL_AS1 *)(dst + (uint64_t)r * a.dst_stride) = o[r];
}

// grid: x = run of 256 pieces of 16 bytes, y = insertion site
__global__ __launch_bounds__(kLanes) void sites_ins_init_kernel(jl_sites_ins_args a)
{
    const uint64_t piece = (uint64_t)blockIdx.x * kLanes + threadIdx.x;
    const uint64_t at = piece * 16u;
    if (at + 16u > a.dst_stride) return;
    const jl_ins_site s = a.isites[blockIdx.y];   // (wave-uniform)

    // p[2 j + b] = plane 1 + b of column col - 1 + j
    u32x4 p[4];
    const uint8_t JL_AS1 *src = (const uint8_t JL_AS1 *)a.src + 3ull * (s.col - 1u) * a.src_stride + at;
    const bool have = at + 16u <= a.src_stride;
#pragma unroll
    for (uint32_t r = 0; r < 4u; ++r) {
        p[r] = u32x4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};   // code 6
        if (have) p[r] = __builtin_nontemporal_load((const u32x4 JL_AS1 *)(src + (uint64_t)(3u * (r >> 1) + 1u + (r & 1u)) * a.src_stride));
    }
    u32x4 out;
#pragma unroll
    for (uint32_t w = 0; w < 4u; ++w) {
        const uint32_t valid = jl_valid_bits(a.n_reads, 4u * piece + w);
        out[w] = (p[0][w] & p[1][w]) | (p[2][w] & p[3][w]) | ~valid;   // does not span, or no read at all
    }
    const u32x4 zero = u32x4{0u, 0u, 0u, 0u};
    uint8_t JL_AS1 *dst = (uint8_t JL_AS1 *)a.dst + 9ull * s.k * a.dst_stride + at;
#pragma unroll
    for (uint32_t r = 0; r < 9u; ++r) *(u32x4 JL_AS1 *)(dst + (uint64_t)r * a.dst_stride) = (r % 3u) ? out : zero;
}

// grid: x = run of 256 events, up to events_cap
__global__ __launch_bounds__(256) void sites_ins_scatter_kernel(jl_sites_ins_args a)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= min(*a.n_events, a.events_cap)) return;
    const jl_insertion_event ev = a.events[i];
    if (ev.read >= a.n_reads) return;
    uint32_t lo = 0, hi = a.n_isites;   // the first site at or beyond the event's column
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2u;
        if (a.isites[mid].col < ev.col) lo = mid + 1u;
        else hi = mid;
    }
    if (lo == a.n_isites) return;
    const jl_ins_site s = a.isites[lo];
    if (s.col != ev.col) return;   // an event at a junction that is no site
    uint32_t bits;                  // bit 3 j + b: plane b of cell j
    if (ev.kind == 1u) {
        uint32_t l = s.a_begin, h = s.a_end;   // the first allele at or beyond (len, seq)
        while (l < h) {
            const uint32_t mid = (l + h) / 2u;
            const jl_insertion_allele &q = a.alleles[mid];
            if (q.len < ev.len || (q.len == ev.len && q.seq < ev.seq)) l = mid + 1u;
            else h = mid;
        }
        uint32_t codon = JL_SITE_INS_OTHER;
        if (l < s.a_end && a.alleles[l].len == ev.len && a.alleles[l].seq == ev.seq) codon = 1u + (l - s.a_begin);
        bits = ((codon >> 4) & 3u) | (((codon >> 2) & 3u) << 3) | ((codon & 3u) << 6);
    } else if (ev.kind == 2u) {
        bits = 0x124u;   // 4 4 4: plane 2 of every cell
    } else if (ev.kind == 3u) {
        bits = 0x16Du;   // 5 5 5: planes 0 and 2
    } else {
        return;
    }
    uint8_t *dst = a.dst + 9ull * s.k * a.dst_stride + (uint64_t)(ev.read >> 5) * 4u;
    const uint32_t bit = 1u << (ev.read & 31u);
    for (uint32_t r = 0; r < 9u; ++r)
        if ((bits >> r) & 1u) atomicOr((uint32_t *)(dst + (uint64_t)r * a.dst_stride), bit);
}

}  // namespace

// a->n_isites in 1 .. JL_SITES_MAX, every site's col in 1 .. the source's n_cols - 1 and k below the destination's sites,
// a->dst_stride a multiple of 16 below 2^36 that holds n_reads bits; behind jl_launch_sites_assemble on `st`
void jl_launch_sites_insertions(const jl_sites_ins_args *a, hipStream_t st)
{
    const uint64_t pieces = a->dst_stride / 16u;
    hipLaunchKernelGGL(sites_ins_init_kernel, dim3((uint32_t)((pieces + kLanes - 1u) / kLanes), a->n_isites), dim3(kLanes), 0, st, *a);
    if (a->events_cap)
        hipLaunchKernelGGL(sites_ins_scatter_kernel, dim3((uint32_t)(((uint64_t)a->events_cap + 255u) / 256u)), dim3(256), 0, st, *a);
}

// a->n_sites in 1 .. JL_SITES_MAX, a->dst_stride a multiple of 16 below 2^36
void jl_launch_sites_assemble(const jl_sites_args *a, hipStream_t st)
{
    const uint64_t pieces = a->dst_stride / 16u;
    hipLaunchKernelGGL(sites_assemble_kernel, dim3((uint32_t)((pieces + kLanes - 1u) / kLanes), a->n_sites), dim3(kLanes), 0, st, *a);
}
