// kernels_ingest.hip — aligned BAM records -> the resident bit planes, entirely on the device.
//
// Behaviour: doc/JULIET.md:26-27 (insertions dropped, deletions '-'), :53 (PacBio cigars = X I D S H N; M is refused),
// :256-259 (a QV-filtered base shows up as N).  Reads past n_reads (the padding of a plane up to its stride) and columns
// outside a read's span are 'not covered' (code 6).
//
// Four launches at most, three for a CCS sample (the upload looks at the cigars of the few reads that could be long ones —
// jl_ingest_read_is_long — and the long-read launch is made only if there may be one; the planes kernel's second size finds nothing
// to do on CCS reads); no by-row scratch in HBM:
//   cigar_walk_kernel   every read: a workgroup takes 64 reads.  One thread a read walks its cigar, sixteen ops a step in registers ->
//                       the read's RUNS in WINDOW columns (stretches of '=' / 'X' merge into one run of aligned bases; D and N are
//                       runs of their own; I / S / H / P only end a run), 8 bytes each, between a leading 'not covered from column
//                       0' entry and two trailing ones (the read's end; 'never'), so that every column of the window lies in exactly
//                       one entry's interval — into LDS.  Then a thread a (read, sweep) pair: ONE 16-byte descriptor per read and
//                       column sweep: where the sweep's entries are, how many, the dword the first 16-byte piece of packed bases
//                       the sweep needs begins on, how many pieces, the query offset of that piece — everything
//                       ingest_planes_kernel needs to ask for its input in one round trip.  Reads of more than 192 ops or 37 runs
//                       are left to
//   cigar_runs_kernel   the long-read launch: the reads cigar_walk_kernel left to it, a row of sixteen lanes a read, prefix sums
//                       over the cigar, 512 entries a read in LDS and what is beyond read back from HBM.
//   ingest_planes_kernel  a workgroup = 128 reads x one sweep of 256 columns.  One request per read (the descriptor), then
//                       the entries and the pieces together.  The pieces become nibbles in QUERY order in LDS with plain
//                       16-byte stores — no run search, no masks.  Meanwhile a thread per read fills a table: for every block
//                       of 8 columns, the LDS nibble address its eight codes begin at — inside the read's bases when one
//                       aligned run covers the block, a constant dword of '-' or of 'not covered' when a deletion / nothing
//                       does; the few blocks with a run boundary inside are put together into a side dword, a thread per
//                       entry, and the table points there.  GATHER AT THE TRANSPOSE: a thread takes 32 reads x 8 columns,
//                       picks each read's dword by the table (two LDS reads + one v_alignbit), transposes four 8 x 8 nibble
//                       blocks in registers, turns BAM's base codes into symbol codes as bit planes and stores a dword of
//                       each plane of each column; the eight workgroups that share the 128-byte lines of a sweep run on one
//                       XCD next to each other (blockIdx mapping), so the lines are completed in that XCD's L2.
//                       The first launch has room for four entries a read on average; a (tile, sweep) unit with more is
//                       handed on to a second launch of the same kernel with room for sixteen (three workgroups a CU
//                       instead of five).  A read the workgroup has no room for at all — more inserted bases in a sweep than
//                       a staging row holds, more than 254 entries in a sweep, entries beyond the second size — is written
//                       column by column from its entries in HBM by a wave of the SAME workgroup behind its stores (slow_pair).
//                       With qualities a workgroup of the first size takes TWO sibling tiles one after the other and stores
//                       their plane words together, 32 bytes of a line a request (round 6: the L2 takes a write request per row
//                       and tile, 7 x 10^6 a window — the stores were 34 us of the launch's 111, 70 of 184 with qualities).
//                       The QV filter comes in two forms: qualities, a byte a base, compared with min_qv here (two unaligned 16-byte
//                       loads a piece, eight registers), or the caller's decision, a BIT a base (jl_records_append_masked): the mask is
//                       laid out by the resident bases, bit 2 x byte + nibble, so the 32 flags of a piece are the four bytes at a
//                       quarter of the piece's byte offset — one register a piece, asked for with the piece.
//                       (Rounds 1-3 expanded every read into a by-row matrix in HBM: 870 MB moved for the 316 MB needed;
//                       round 4 scattered the codes into a by-row LDS tile with masked, shifted XORs: 137 us.)
// Where things are: what a cigar op means, the entries' fields, the verdict on a record and the long-read rule — cigar_rules.h, shared
// with the host (jl_ingest_read_is_long); the descriptor — make_desc and the desc_… readers, below its layout; a planes workgroup's
// LDS — planes_lds; block number -> (tile, sweep) — place_of; a unit of the planes kernel — planes_unit = pieces_stage | read_stage,
// barrier, the hand-on check, table_stage, barrier, gather_stage, store_block_words, the slow tail (slow_pair).

#include <algorithm>

#include "cigar_rules.h"
#include "jl_internal.h"

#ifndef JL_NT_QM     // sibling tiles a workgroup of the planes kernel's mask mode (jl_launch_ingest): 1 or 2
#define JL_NT_QM 2
#endif

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4a4 __attribute__((ext_vector_type(4), aligned(4)));

constexpr uint32_t kSweep = 256u;                   // columns per workgroup (448-column sweeps: 144 us against 140, round 4)
constexpr uint32_t kBlocks = kSweep / 8u;           // blocks of 8 columns = dwords of 8 codes
constexpr uint32_t kTileReads = 128u;               // reads per workgroup (64-read tiles: 182 us against 176, round 5)
constexpr uint32_t kTileGroups = kTileReads / 32u;  // groups of 32 reads = dwords of a plane the tile writes per column
constexpr uint32_t kSubTiles = 1024u / kTileReads;  // tiles that share the 128-byte lines of the planes
constexpr uint32_t kThreads = 2u * kTileReads;      // a thread per read in the prologue, two in the table fill
static_assert(kSweep % 16u == 0 && kTileReads % 32u == 0 && kThreads <= 1024u, "whole blocks for both table threads, whole plane dwords");
static_assert(kTileGroups * kBlocks <= kThreads, "a thread per 32 reads x 8 columns in the transposing phase");

// the cigar rules, the entries' fields and makers, the verdict on a record, the long-read rule's kWalkOps and kWalkEnt: cigar_rules.h
using namespace jl_cigar;
__device__ __forceinline__ uint2 as_uint2(entry_t e) { return make_uint2(e.x, e.y); }

// ---------------------------------------------------------------------------------------- runs
// inclusive prefix sum within the DPP rows of sixteen lanes (four shifts)
__device__ __forceinline__ uint32_t row_scan(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);   // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);   // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);   // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);   // row_shr:8
    return v;
}
// ... and over the 64 lanes: the rows' sums go on by two row broadcasts
__device__ __forceinline__ uint32_t wave_scan(uint32_t v)
{
    v = row_scan(v);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);  // row_bcast:15 -> rows 1, 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);  // row_bcast:31 -> rows 2, 3
    return v;
}
// Entries of read r: runs[cig_off[r] + 3 r + i], i = 0 .. n_runs + 2, each {window column | kind << 30, query offset}; entry i
// says what the read shows in the columns [its column, the next entry's column): kind 1 aligned bases (column c holds the
// base at query offset + c - column), 2 deletion, 3 nothing ('not covered': before the read, a reference skip, behind it).
// Entry 0 = {0, nothing}; entries 1 .. n_runs the read's runs, columns clamped to [0, n_cols] (a run that begins before the
// window begins at column 0 with its query offset moved along); entry n_runs + 1 = the read's end {column, nothing, query
// length}; entry n_runs + 2 = {kRunMask, nothing}: never reached.  The columns never decrease.
// entries of a long read kept in LDS for the descriptors: 512 — 64 KB, two workgroups a CU (what is beyond is read back from HBM,
// a trip an entry: 1 ms instead of 0.12 for 100k reads with 1 % of indels, 236 ops a read, when they all did)
constexpr uint32_t kRunsLds = 512u;
constexpr uint32_t kRunsDeferred = 0xFFFFFFFFu;   // nruns[r] of a read cigar_walk_kernel leaves to the long-read launch
constexpr uint32_t kRunsLongGrid = 1024u;     // workgroups of the long-read launch at most: its waves take 64 reads at a time, in turns
constexpr uint32_t kDescSweeps = 15u;       // sweeps a row of sixteen lanes describes per pass (it needs sixteen bounds)
constexpr uint32_t kDescMax = 255u;         // "more than the planes kernel takes": pieces or entries of a (read, sweep)

// Descriptor of (sweep s, read r) at desc[s * n_reads + r]:
//   x  where the first 16-byte piece of packed bases begins (byte offset / 4: on a dword), low 32 bits
//   y  index of the sweep's first entry in runs[], low 32 bits
//   z  query offset of the first piece's first base (>= -6: the piece may begin before the read's bases)
//   w  x's bits 32-39 | entry index bits 32-39 << 8 | pieces << 16 | entries << 24   (255 = too many)
// The entries of a sweep: from the one that contains its first column to the first one that begins behind its last column.
// Two entries = ONE entry covers the whole sweep, the common case: then `entries` reads 1, y = the query offset of the sweep's
// first column and bits 8-9 of w = the entry's kind — the planes kernel never asks for the entries.
// a row of the planes kernel's staging area: a sweep's pieces and one more — its first piece may begin seven bases before the sweep,
// which leaves room for 25 inserted bases (a read with more of them in a sweep goes to slow_pair)
constexpr uint32_t kRowPieces = (kSweep + 31u) / 32u + 1u;
// the aligned bases of a sweep's entries in the query, [q_lo, q_hi): empty until an entry adds to it
struct query_range {
    uint32_t q_lo = 0xFFFFFFFFu, q_hi = 0;
};
// entry e (the one behind it: nx) within the sweep's columns [X, Xend)
__device__ __forceinline__ void range_add(query_range &g, uint2 e, uint2 nx, uint32_t X, uint32_t Xend)
{
    if (entry_kind(e.x) != kAligned) return;
    const uint32_t W = entry_col(e.x), ca = max(W, X), cbv = min(entry_col(nx.x), Xend);
    if (ca < cbv) {
        g.q_lo = min(g.q_lo, e.y + (ca - W));
        g.q_hi = max(g.q_hi, e.y + (cbv - W));
    }
}
// the descriptor of a sweep that begins at column X: its first entry and that entry's index in runs[], its entries (kDescMax: too
// many), the query range they take; seq_off: the read's first byte of packed bases
__device__ __forceinline__ uint4 make_desc(uint2 first, uint64_t first_idx, uint32_t n_ent, query_range g, uint32_t X, uint64_t seq_off)
{
    // the 16-byte pieces of packed bases the sweep takes: from the DWORD that holds its first base on — at most seven bases
    // before it, so that a row of the planes kernel (a sweep + 32 bases) has room for 25 inserted ones (byte offsets are
    // even in bases: all of this in 32 bits relative to the read's first byte, the one 64-bit sum at the end)
    uint64_t piece = 0;
    uint32_t np = 0;
    int32_t q0 = 0;
    if (g.q_lo < g.q_hi) {
        const uint32_t al = (uint32_t)seq_off & 3u;                          // the read's first byte within its dword
        const uint32_t b_lo = al + (g.q_lo >> 1), b_hi = al + (g.q_hi + 1u) / 2u;   // bytes from that dword's first on
        const uint32_t d_lo = b_lo >> 2;
        piece = (seq_off >> 2) + d_lo;
        np = min((b_hi + 15u - 4u * d_lo) >> 4, kDescMax);
        q0 = 2 * ((int32_t)(4u * d_lo) - (int32_t)al);
    }
    uint4 d;
    d.x = (uint32_t)piece;
    d.z = (uint32_t)q0;
    if (n_ent == 2u) {
        // ONE entry covers the whole sweep (three reads in four of a CCS sample): the planes kernel needs no entries for it —
        // what the entry is, and the query offset of the sweep's first column
        d.y = first.y + (X - entry_col(first.x));
        d.w = (uint32_t)((piece >> 32) & 0xFFu) | (entry_kind(first.x) << 8) | (np << 16) | (1u << 24);
    } else {
        d.y = (uint32_t)first_idx;
        d.w = (uint32_t)((piece >> 32) & 0xFFu) | ((uint32_t)((first_idx >> 32) & 0xFFu) << 8) | (np << 16) | (n_ent << 24);
    }
    return d;
}
// ... and as the planes kernel reads it
__device__ __forceinline__ uint4 desc_of_no_read() { return make_uint4(0, 0, 0, kNothing << 8 | 1u << 24); }   // one entry of nothing
__device__ __forceinline__ uint32_t desc_pieces(const uint4 &d) { return (d.w >> 16) & 0xFFu; }
__device__ __forceinline__ uint32_t desc_entries(const uint4 &d) { return d.w >> 24; }
__device__ __forceinline__ bool desc_simple(const uint4 &d) { return desc_entries(d) == 1u; }
__device__ __forceinline__ uint32_t desc_simple_kind(const uint4 &d) { return (d.w >> 8) & 3u; }
__device__ __forceinline__ uint32_t desc_simple_q(const uint4 &d) { return d.y; }      // query offset of the sweep's first column
__device__ __forceinline__ uint64_t desc_piece_dw(const uint4 &d) { return (((uint64_t)d.w & 0xFFu) << 32) | d.x; }
__device__ __forceinline__ uint64_t desc_entry_idx(const uint4 &d) { return (((uint64_t)(d.w >> 8) & 0xFFu) << 32) | d.y; }
__device__ __forceinline__ int32_t desc_q0(const uint4 &d) { return (int32_t)d.z; }
// more pieces than a staging row holds, or more entries than a descriptor counts: the pair is left to slow_pair
__device__ __forceinline__ bool desc_slow(const uint4 &d) { return desc_pieces(d) > kRowPieces || desc_entries(d) == kDescMax; }

// The records are untrusted: a cigar with an 'M' (forbidden in PacBio BAM, doc/JULIET.md:53), one that consumes more bases
// (or qualities) than the record holds, or one that spans 2^30 reference bases or more is reported — *bad = min over such reads
// of (read << 8 | code), code 1 'M', 2 bases, 3 qualities, 4 span (5: see cigar_walk_kernel) — and the read is treated as covering nothing, so no later
// kernel follows its offsets anywhere.  Lengths add up in 64 bits (a step that holds an op of 2^24 bases or more is summed
// exactly, lane by lane), so no crafted cigar wraps a sum back into range.
// The long-read launch takes the reads cigar_walk_kernel left to it (nruns[r] = kRunsDeferred): a wave finds them among
// sixty-four reads at a time and takes them four at a time, with room for kRunsLds entries each in LDS.
__global__ __launch_bounds__(256) void cigar_runs_kernel(uint64_t n_reads, const int32_t *__restrict__ pos, const uint32_t *__restrict__ cigar,
                                                         const uint64_t *__restrict__ cig_off, const uint64_t *__restrict__ seq_off,
                                                         const uint64_t *__restrict__ qual_off, uint32_t win_begin, uint32_t n_cols,
                                                         uint32_t n_sweeps, uint2 *__restrict__ runs, uint32_t *__restrict__ nruns,
                                                         uint4 *__restrict__ desc, unsigned long long *__restrict__ bad)
{
    // A ROW OF SIXTEEN LANES PER READ — a wave takes four reads at once — and EIGHT CONSECUTIVE OPS PER LANE (128 ops a step: a CCS
    // read's cigar in one or two steps): a lane adds its eight ops up itself, the sixteen lanes' sums are scanned within the DPP
    // row (four row_shr steps, no row broadcast), and a second pass over the lane's ops puts the entries out.  (One read at a
    // time over the whole wave, two ops a lane, was 450 wave instructions a read; the scans, the ballots and the bookkeeping
    // per step are now shared by four reads and eight ops a lane.  Several batches of four a wave, the next one's words asked
    // for ahead, measured slower: 63 against 51 us.)
    __shared__ uint2 s_run_all[4][4][kRunsLds];      // [wave][its four reads]
    const uint32_t wid = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint2 (*s_run)[kRunsLds] = s_run_all[wid];
    const uint32_t q = lane >> 4, sl = lane & 15u;
    struct head_t { uint64_t cb, c_end, so, so1, qlen; int32_t pos; };
    auto ask_head = [&](uint64_t rr) -> head_t {     // (the sixteen lanes of a row ask for the same words: one request)
        head_t h = {0, 0, 0, 0, ~0ull, 0};
        if (rr < n_reads) {
            h.cb = cig_off[rr];
            h.c_end = cig_off[rr + 1];
            h.so = seq_off[rr];
            h.so1 = seq_off[rr + 1];
            if (qual_off) h.qlen = qual_off[rr + 1] - qual_off[rr];
            h.pos = pos[rr];
        }
        return h;
    };
    auto ask_words = [&](const head_t &h, uint32_t k, u32x4a4 &wa, u32x4a4 &wb) {
        const uint32_t n = (uint32_t)min(h.c_end - h.cb, (uint64_t)0xFFFFFF00u);
        const u32x4a4 z = {0, 0, 0, 0};
        wa = k < n ? *reinterpret_cast<const u32x4a4 *>(cigar + h.cb + k) : z;           // (words past the read's ops are masked where they are used)
        wb = k + 4u < n ? *reinterpret_cast<const u32x4a4 *>(cigar + h.cb + k + 4u) : z;
    };
    const uint64_t turn = (uint64_t)gridDim.x * 4u * 64u;
    for (uint64_t i0 = ((uint64_t)blockIdx.x * 4u + wid) * 64u; i0 < n_reads; i0 += turn) {
    // which of the sixty-four reads from i0 on are long ones, taken four at a time
    uint64_t todo = __ballot(i0 + lane < n_reads && nruns[min(i0 + lane, n_reads - 1u)] == kRunsDeferred);   // (left to this launch by cigar_walk_kernel)
    while (todo) {
    uint32_t at[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        at[t] = todo ? (uint32_t)__builtin_ctzll(todo) : 64u;
        todo &= todo - 1u;
    }
    const uint32_t mine = q == 0u ? at[0] : q == 1u ? at[1] : q == 2u ? at[2] : at[3];
    const uint64_t r = mine < 64u ? i0 + mine : n_reads;
    const bool live = r < n_reads;
    const head_t h = ask_head(r);
    u32x4a4 wa_first, wb_first;
    ask_words(h, 8u * sl, wa_first, wb_first);
    const uint64_t my_cb = h.cb, c_end = h.c_end, my_so = h.so, so1 = h.so1, qlen = h.qlen;
    const int64_t base = (int64_t)h.pos - (int64_t)win_begin;
    const uint64_t ent0 = my_cb + 3u * r;     // index of the read's entry 0 in runs[]
    uint2 *out = runs + ent0;
    const uint32_t *cig = cigar + my_cb;
    const uint32_t n_ops = (uint32_t)min(c_end - my_cb, (uint64_t)0xFFFFFF00u);   // (a record's cigar has fewer than 2^32 ops)
    uint32_t max_ops = n_ops;                  // of the wave's four reads
#pragma unroll
    for (int t = 0; t < 4; ++t) max_ops = max(max_ops, (uint32_t)__builtin_amdgcn_readlane((int)n_ops, 16 * t));
    auto row_last = [&](uint32_t v) -> uint32_t {   // lane 15 of the row's value, in all of its lanes
        return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(4u * (lane | 15u)), (int)v);
    };
    auto put = [&](uint32_t idx, uint2 e) {
        out[idx] = e;
        if (idx < kRunsLds) s_run[q][idx] = e;
    };
    uint64_t ref_total = 0, q_total = 0;       // (the row's: the same in its sixteen lanes)
    uint32_t n_runs = 0, prev_kind = 0;
    bool has_m = false;
    for (uint32_t k0 = 0; k0 < max_ops; k0 += 128u) {
        const uint32_t k = k0 + 8u * sl;
        u32x4a4 wa = wa_first, wb = wb_first;
        if (k0 != 0u) {
            const u32x4a4 z = {0, 0, 0, 0};
            wa = k < n_ops ? *reinterpret_cast<const u32x4a4 *>(cig + k) : z;           // (words past the read's ops are masked below)
            wb = k + 4u < n_ops ? *reinterpret_cast<const u32x4a4 *>(cig + k + 4u) : z;
        }
        const uint32_t w8[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
        uint32_t kinds = 0, rsum = 0, qsum = 0, big = 0;      // kinds: the ops' kinds (cigar_rules.h), two bits an op
#pragma unroll
        for (uint32_t t = 0; t < 8u; ++t) {
            const bool in = k + t < n_ops;
            const uint32_t op = w8[t] & 15u, len = in ? w8[t] >> 4 : 0u;
            kinds |= kind_of(op, len) << (2u * t);
            has_m = has_m || (op == 0u && in);
            rsum += consumes_ref(op) ? len : 0u;
            qsum += consumes_query(op) ? len : 0u;
            big |= len;
        }
        // the kind of the op before this lane's first one: the lane before's last (the row's first lane: the step before's)
        uint32_t before = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(kinds >> 14), 0x111, 0xF, 0xF, true);   // row_shr:1
        if (sl == 0u) before = prev_kind;
        // bit 2 t: op t begins an entry — begins_entry(its kind, the kind before), the eight at once: it has a kind, and not both it
        // and the op before are aligned bases (kind 1 = 01: the low bit without the high one)
        const uint32_t prevs = (kinds << 2) | before;
        const uint32_t any = (kinds | (kinds >> 1)) & 0x5555u, both1 = (kinds & ~(kinds >> 1)) & (prevs & ~(prevs >> 1)) & 0x5555u;
        const uint32_t starts = any & ~both1;
        const uint32_t n_st = (uint32_t)__popc(starts);
        const uint32_t ri = row_scan(rsum), qi = row_scan(qsum), ni = row_scan(n_st);
        // the row's sums so far, in 64 bits; a step that holds an op of 2^24 bases or more is summed exactly, lane by lane (a
        // 32-bit scan of sixteen lanes of eight such ops could wrap)
        uint64_t r_step = row_last(ri), q_step = row_last(qi);
        if (__ballot(big >= (1u << 24)) != 0ull) {
            r_step = 0;
            q_step = 0;
            for (uint32_t l = 0; l < 16u; ++l) {
                r_step += (uint32_t)__builtin_amdgcn_ds_bpermute((int)(4u * ((lane & 48u) | l)), (int)rsum);
                q_step += (uint32_t)__builtin_amdgcn_ds_bpermute((int)(4u * ((lane & 48u) | l)), (int)qsum);
            }
        }
        // the entries
        uint64_t ref_at = ref_total + (ri - rsum), q_at = q_total + (qi - qsum);
        uint32_t idx = 1u + n_runs + (ni - n_st);
#pragma unroll
        for (uint32_t t = 0; t < 8u; ++t) {
            const uint32_t op = w8[t] & 15u, len = k + t < n_ops ? w8[t] >> 4 : 0u;
            if ((starts >> (2u * t)) & 1u) {
                const col_t c = window_col(base, ref_at, n_cols);
                put(idx, as_uint2(entry_run(c.col, (kinds >> (2u * t)) & 3u, (uint32_t)q_at + c.before)));
                ++idx;
            }
            ref_at += consumes_ref(op) ? len : 0u;
            q_at += consumes_query(op) ? len : 0u;
        }
        n_runs += row_last(ni);
        prev_kind = row_last(kinds >> 14);   // (only a full step has a successor)
        ref_total += r_step;
        q_total += q_step;
    }
    // M anywhere in the row?  (a ballot's sixteen bits)
    const uint64_t bm = __ballot(has_m);
    uint32_t code = verdict(((bm >> (16u * q)) & 0xFFFFull) != 0ull, q_total, so1 - my_so, qlen, ref_total);
    if (!live) code = 0;
    uint32_t end_col = 0;
    if (code) {
        n_runs = 0;
        if (sl == 0u) atomicMin(bad, ((unsigned long long)r << 8) | code);
    } else end_col = window_col(base, ref_total, n_cols).col;
    if (live && sl < 3u) {
        const uint32_t idx = sl == 0u ? 0u : n_runs + sl;
        put(idx, as_uint2(sl == 0u ? entry_before() : sl == 1u ? entry_end(end_col, (uint32_t)q_total) : entry_never()));
        if (sl == 0u) nruns[r] = n_runs;
    }
    // ---- the descriptors: a lane per sweep (fifteen sweeps a pass: a sweep needs the bound of the next one too).  Entries
    // beyond the LDS copy are read back from HBM: past this wave's own stores.
    uint32_t n_max = n_runs;
#pragma unroll
    for (int t = 0; t < 4; ++t) n_max = max(n_max, (uint32_t)__builtin_amdgcn_readlane((int)n_runs, 16 * t));
    if (n_max + 3u > kRunsLds) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __builtin_amdgcn_wave_barrier();
    const uint32_t n_ent_all = n_runs + 3u;          // entries of this lane's read
    uint32_t top = 1u;                         // the highest power of two not above the longest list
    while (2u * top <= n_max + 3u) top *= 2u;
    // (`entry`: the read's i-th entry — out of the wave's LDS copy, or, for the lists that are longer than it, read back)
    auto describe = [&](auto entry) {
        for (uint32_t s0 = 0; s0 < n_sweeps; s0 += kDescSweeps) {
            const uint32_t s = s0 + sl;
            // f = the number of entries that begin at or before the sweep's first column (entry 0 always does, the last never)
            const uint32_t X = min(s, n_sweeps) * kSweep;   // (lanes past the last bound repeat it)
            // The bound BEHIND the window's last sweep is the window's last column, not n_sweeps * kSweep: every run beyond the
            // window is clamped to column n_cols, and counted up to there all of a long read's runs behind the window were
            // entries of its last sweep (six of them and the unit went to the second size, 255 and the read to slow_pair: right
            // cells, but `juliet --windows N` paid for it in every window).  Up to n_cols - 1 the first clamped entry closes the list.
            const uint32_t X_bound = s >= n_sweeps ? n_cols - 1u : X;
            uint32_t f = 0;
            for (uint32_t step = top; step; step >>= 1) {
                const uint32_t t = f + step;
                if (live && t <= n_ent_all && entry_col(entry(t - 1u).x) <= X_bound) f = t;
            }
            const uint32_t f_next = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)f, 0x101, 0xF, 0xF, false);   // row_shl:1
            if (!live || sl == kDescSweeps || s >= n_sweeps) continue;
            const uint32_t Xend = min(n_cols, X + kSweep);
            const uint32_t lo = f - 1u;
            uint32_t n_ent = f_next - f + 2u;
            query_range g;
            uint2 e = entry(lo);
            const uint2 first = e;
            if (n_ent >= kDescMax) n_ent = kDescMax;
            else {
                for (uint32_t i = lo; i + 1u < lo + n_ent; ++i) {
                    const uint2 nx = entry(i + 1u);
                    range_add(g, e, nx, X, Xend);
                    e = nx;
                }
            }
            desc[(uint64_t)s * n_reads + r] = make_desc(first, ent0 + lo, n_ent, g, X, my_so);
        }
    };
    const uint2 *s_mine = s_run[q];
    if (n_max + 3u <= kRunsLds) describe([&](uint32_t i) -> uint2 { return s_mine[i]; });
    else
        describe([&](uint32_t i) -> uint2 {
            if (i < kRunsLds) return s_mine[i];
            const unsigned long long v = __hip_atomic_load(reinterpret_cast<const unsigned long long *>(runs + ent0 + i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return make_uint2((uint32_t)v, (uint32_t)(v >> 32));
        });
    __builtin_amdgcn_wave_barrier();      // (the next four reads write the LDS copy these ones' descriptors were made from)
    }
    }
}

// ---------------------------------------------------------------------------------------- runs, a thread a read
// The first launch of a build (round 6; it replaced a first launch of cigar_runs_kernel, which gave a row of sixteen lanes to every read:
// 24 x 10^6 wave instructions and 47-50 us for 100k reads of 127 ops, 36 us for the ten ops of a `ccs --richQVs` read — the scans,
// the LDS copy of the entries and a binary search per sweep done by every row, for lists a dozen entries long).  A workgroup takes
// 64 reads:
//   1  ONE THREAD a read (the first wave): the ops, sixteen a step in registers (four 16-byte loads in flight, the next step's
//      asked for before this one's are looked at) -> the read's ENTRIES in LDS.  No store to HBM in this pass: vmcnt counts loads
//      and stores in one order, and forms of this kernel that stored entries while walking waited for every store's
//      acknowledgement at each new load of ops (32-61 us for ten ops, 144-720 us for 127).
//   2  a thread a (read, sweep) pair, all four waves — the 64 lanes of a wave write one sweep's descriptors of the 64 reads, 1 KB a
//      store: the last entry that begins at or before the sweep's first column by bisection, then the sweep's entries up to the
//      first that begins behind its last column.  Then the entries go out.
// (One thread a read for BOTH passes — a dozen descriptors one after the other — was 25 us for ten ops: a wave is alone on its
// SIMD then, 1563 waves for 1024 SIMDs, and the length of the dependent chain is all that counts.)
// A read with more than kWalkOps ops or more than kWalkEnt entries is left, whole, to the long-read launch (cigar_runs_kernel):
// nruns[r] = kRunsDeferred.
// (kWalkOps, kWalkEnt: cigar_rules.h, with the host's statement of this rule)
constexpr uint32_t kWalkReads = 64u;    // reads of a workgroup

__global__ __launch_bounds__(256) void cigar_walk_kernel(uint64_t n_reads, const int32_t *__restrict__ pos, const uint32_t *__restrict__ cigar,
                                                         const uint64_t *__restrict__ cig_off, const uint64_t *__restrict__ seq_off,
                                                         const uint64_t *__restrict__ qual_off, uint32_t win_begin, uint32_t n_cols,
                                                         uint32_t n_sweeps, uint2 *__restrict__ runs, uint32_t *__restrict__ nruns,
                                                         uint4 *__restrict__ desc, unsigned long long *__restrict__ bad,
                                                         uint32_t *__restrict__ count, uint32_t second)
{
    // second = 0: the host has looked at the cigars (jl_ingest_read_is_long, at the upload) and found no read for the other launch, which
    // is then not made (6 us of a build).  Should this kernel find one all the same, the read covers nothing and the build fails with
    // code 5 — never descriptors nobody wrote.
    // (the build's counters — [0] retired: it counted the pairs of a list no kernel makes any more, and is zeroed with [1] only because
    // the block's layout is shared with jl_ingest_verdict; [1] units handed on — begin at zero: the planes kernels, which count, come behind this
    // launch on the stream; a launch of its own for this was 4 us of a build)
    if (blockIdx.x == 0 && threadIdx.x < 2u) count[threadIdx.x] = 0u;
    __shared__ uint2 s_ent[kWalkEnt * kWalkReads];      // entry i of read j at [i * 64 + j]
    __shared__ uint32_t s_nruns[kWalkReads];            // kRunsDeferred: no descriptors from here
    __shared__ uint64_t s_ent0[kWalkReads], s_so[kWalkReads];
    const uint32_t tid = threadIdx.x, j = tid & (kWalkReads - 1u);
    const uint64_t r = (uint64_t)blockIdx.x * kWalkReads + j;
    if (tid < kWalkReads) {
        uint32_t n_runs = kRunsDeferred;
        if (r < n_reads) {
            const uint64_t my_cb = cig_off[r], c_end = cig_off[r + 1], my_so = seq_off[r], so1 = seq_off[r + 1];
            const uint64_t qlen = qual_off ? qual_off[r + 1] - qual_off[r] : ~0ull;
            const int64_t base = (int64_t)pos[r] - (int64_t)win_begin;
            const uint32_t n_ops = (uint32_t)min(c_end - my_cb, (uint64_t)0xFFFFFF00u);
            s_ent0[j] = my_cb + 3u * r;
            s_so[j] = my_so;
            if (n_ops > kWalkOps && !second) {
                atomicMin(bad, ((unsigned long long)r << 8) | 5u);
                n_runs = 0;
                s_ent[j] = as_uint2(entry_before());
                s_ent[kWalkReads + j] = as_uint2(entry_end(0u, 0u));
                s_ent[2u * kWalkReads + j] = as_uint2(entry_never());
            }
            if (n_ops <= kWalkOps) {
                const uint32_t *cig = cigar + my_cb;
                // (the loads take sixteen words from the step's first op on whatever the read's length: words past its ops are the
                // next read's or the array's slack, and are not looked at)
                struct ops16 { u32x4a4 a, b, c, d; };
                auto ask = [&](uint32_t k0) -> ops16 {
                    ops16 o;
                    const uint32_t *p = cig + k0;
                    o.a = *reinterpret_cast<const u32x4a4 *>(p);
                    o.b = *reinterpret_cast<const u32x4a4 *>(p + 4);
                    o.c = *reinterpret_cast<const u32x4a4 *>(p + 8);
                    o.d = *reinterpret_cast<const u32x4a4 *>(p + 12);
                    return o;
                };
                uint64_t ref_at = 0, q_at = 0;
                uint32_t prev_kind = 0;
                bool has_m = false;
                n_runs = 0;
                s_ent[j] = as_uint2(entry_before());
                ops16 cur = ask(0);
                for (uint32_t k0 = 0; k0 < n_ops; k0 += 16u) {
                    const ops16 nxt = ask(k0 + 16u < n_ops ? k0 + 16u : 0u);
                    const uint32_t w16[16] = {cur.a.x, cur.a.y, cur.a.z, cur.a.w, cur.b.x, cur.b.y, cur.b.z, cur.b.w,
                                              cur.c.x, cur.c.y, cur.c.z, cur.c.w, cur.d.x, cur.d.y, cur.d.z, cur.d.w};
#pragma unroll
                    for (uint32_t t = 0; t < 16u; ++t) {
                        const bool in = k0 + t < n_ops;
                        const uint32_t op = w16[t] & 15u, len = in ? w16[t] >> 4 : 0u;
                        const uint32_t kind = kind_of(op, len);
                        has_m = has_m || (in && op == 0u);
                        if (begins_entry(kind, prev_kind)) {
                            const col_t c = window_col(base, ref_at, n_cols);
                            ++n_runs;
                            if (n_runs < kWalkEnt) s_ent[n_runs * kWalkReads + j] = as_uint2(entry_run(c.col, kind, (uint32_t)q_at + c.before));
                        }
                        if (in) prev_kind = kind;
                        ref_at += consumes_ref(op) ? len : 0u;
                        q_at += consumes_query(op) ? len : 0u;
                    }
                    cur = nxt;
                }
                if (n_runs + 3u > kWalkEnt && second) n_runs = kRunsDeferred;
                else {
                    const uint32_t code = n_runs + 3u > kWalkEnt ? 5u : verdict(has_m, q_at, so1 - my_so, qlen, ref_at);
                    uint32_t end_col = 0;
                    if (code) {      // a malformed record covers nothing (see cigar_runs_kernel)
                        atomicMin(bad, ((unsigned long long)r << 8) | code);
                        n_runs = 0;
                    } else end_col = window_col(base, ref_at, n_cols).col;
                    s_ent[(n_runs + 1u) * kWalkReads + j] = as_uint2(entry_end(end_col, (uint32_t)q_at));
                    s_ent[(n_runs + 2u) * kWalkReads + j] = as_uint2(entry_never());
                }
            }
            nruns[r] = n_runs;
        }
        s_nruns[j] = n_runs;
    }
    __syncthreads();
    const uint32_t n_runs = s_nruns[j];
    if (n_runs == kRunsDeferred) return;       // (no read, or one for the other launch; no barrier follows)
    const uint32_t n_ent_all = n_runs + 3u;
    const uint64_t ent0 = s_ent0[j], my_so = s_so[j];
    auto ent = [&](uint32_t i) -> uint2 { return s_ent[i * kWalkReads + j]; };
    // ---- 2: the descriptors, sweeps wave, wave + 4, ... of the 64 reads (see cigar_runs_kernel's `describe`)
    for (uint32_t s = tid >> 6; s < n_sweeps; s += 4u) {
        const uint32_t X = s * kSweep, Xend = min(n_cols, X + kSweep);
        // (the window's last sweep ends at its last column: the runs behind the window are all clamped to column n_cols)
        const uint32_t bound = s + 1u < n_sweeps ? X + kSweep : n_cols - 1u;
        // lo: the last entry that begins at or before X (entry 0 does, the last one never)
        uint32_t lo = 0, hi = n_ent_all - 1u;
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (entry_col(ent(mid).x) <= X) lo = mid;
            else hi = mid;
        }
        const uint2 first = ent(lo);
        uint2 e = first;
        query_range g;
        uint32_t i = lo;
        for (;;) {
            ++i;
            const uint2 nx = ent(i);
            range_add(g, e, nx, X, Xend);
            if (entry_col(nx.x) > bound) break;      // it begins behind the sweep: the closing entry
            e = nx;
        }
        // (i - lo + 1 entries: < kWalkEnt < kDescMax)
        desc[(uint64_t)s * n_reads + r] = make_desc(first, ent0 + lo, i - lo + 1u, g, X, my_so);
    }
    // ---- the entries: thread (read, part) writes entries part, part + 4, ...
    uint2 *out = runs + ent0;
    for (uint32_t i = tid >> 6; i < n_ent_all; i += 4u) out[i] = ent(i);
}

// ---------------------------------------------------------------------------------------- the planes of one sweep
// 8 x 8 nibbles held as 8 dwords (row i = m[i], element j at bits 4j) -> their transpose
__device__ __forceinline__ void transpose_nibbles_8x8(uint32_t (&m)[8])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t a = m[i], b = m[i + 4];
        m[i] = (a & 0x0000FFFFu) | (b << 16);
        m[i + 4] = (a >> 16) | (b & 0xFFFF0000u);
    }
#pragma unroll
    for (int h = 0; h < 8; h += 4)
#pragma unroll
        for (int i = h; i < h + 2; ++i) {
            const uint32_t a = m[i], b = m[i + 2];
            m[i] = (a & 0x00FF00FFu) | ((b & 0x00FF00FFu) << 8);
            m[i + 2] = ((a >> 8) & 0x00FF00FFu) | (b & 0xFF00FF00u);
        }
#pragma unroll
    for (int i = 0; i < 8; i += 2) {
        const uint32_t a = m[i], b = m[i + 1];
        m[i] = (a & 0x0F0F0F0Fu) | ((b & 0x0F0F0F0Fu) << 4);
        m[i + 1] = ((a >> 4) & 0x0F0F0F0Fu) | (b & 0xF0F0F0F0u);
    }
}

// 32 reads x 8 columns, R[i] = the 8 nibbles of read i -> out[j][k] = plane k of column j, bit i = read i.
// Four 8 x 8 nibble transposes — block g holds reads g, g + 4, ..., g + 28, so that after it nibble n of M[g][j] is read
// 4 n + g at column j — then the bits of the four blocks' nibbles change places: the four bit planes of the nibbles.
// A read's nibbles are symbol codes already where its bit in `codes` is set (planes 0-2 are the answer); everywhere else they
// are BAM's 4-bit bases, one plane per letter A C G T, and the symbol code is made HERE, 32 reads an instruction: exactly one
// letter -> its index, anything else (N, '=', the ambiguity codes) -> 5, a filtered base.
__device__ __forceinline__ void nibble_rows_to_plane_words(const uint32_t (&R)[32], uint32_t codes, uint32_t (&out)[8][3])
{
    uint32_t M[4][8];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
        for (int i = 0; i < 8; ++i) M[g][i] = R[4 * i + g];
        transpose_nibbles_8x8(M[g]);
    }
    // Plane k of column j wants, in nibble n, bit k of the four blocks' nibbles n (reads 4 n .. 4 n + 3): a 4 x 4 bit transpose
    // between the four words, in every nibble at once — two rounds of masked swaps.
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        uint32_t a0 = M[0][j], a1 = M[1][j], a2 = M[2][j], a3 = M[3][j], t;
        t = ((a0 >> 1) ^ a1) & 0x55555555u; a1 ^= t; a0 ^= t << 1;
        t = ((a2 >> 1) ^ a3) & 0x55555555u; a3 ^= t; a2 ^= t << 1;
        t = ((a0 >> 2) ^ a2) & 0x33333333u; a2 ^= t; a0 ^= t << 2;
        t = ((a1 >> 2) ^ a3) & 0x33333333u; a3 ^= t; a1 ^= t << 2;
        // (three-input boolean functions are one v_bitop3 each)
        const uint32_t one3 = (a0 ^ a1 ^ a2) & ~(a0 & a1 & a2), none3 = ~(a0 | a1 | a2);   // exactly one / none of A C G
        const uint32_t letter = (one3 & ~a3) | (none3 & a3);                               // exactly one of A C G T
        const uint32_t c0 = ~letter | a1 | a3, c1 = letter & (a2 | a3);                    // C T N odd; G T have bit 1; N has bit 2
        out[j][0] = (codes & a0) | (~codes & c0);
        out[j][1] = (codes & a1) | (~codes & c1);
        out[j][2] = (codes & a2) | (~codes & ~letter);
    }
}

struct ingest_args {
    uint64_t n_reads;
    uint32_t n_cols, n_sweeps, n_groups;   // n_groups: groups of 1024 reads (the tiles that share lines)
    uint32_t min_qv;
    const uint64_t *cig_off;     // (slow_pair: where a read's entries begin)
    const uint8_t *seq4;
    const uint64_t *seq_off;     // (slow_pair)
    const uint8_t *qual;         // null: no QV masking
    const uint64_t *qual_off;
    const uint8_t *qmask;        // the filter as one bit a base (jl_records_append_masked), bit 2 x seq byte + base of the byte; null: none
    const uint2 *runs;
    const uint32_t *nruns;
    const uint4 *desc;
    uint32_t *slow_count;        // the 64-byte block of counters: [1] units handed on
    uint32_t *big_list;          // the units (block numbers) handed on to the kernel's second size; their number in slow_count[1]
    uint8_t *msa;
    uint64_t plane_stride;
};

// LDS of a planes workgroup.  The staging area holds dwords of eight codes; a NIBBLE address into it fits 16 bits:
//   dwords 0-1 'not covered' twice, 2-3 '-' twice (what a table entry of a block nothing / a deletion covers points at),
//   4 .. 4 + kEntCap   the blocks with a boundary inside, put together (a dword for every entry: the block it begins inside),
//   kRowBase ..        the reads' codes in query order: a row of kRowPieces 16-byte pieces per read — a sweep's bases from a
//                      16-byte boundary on, + 8 dwords between the 32-read groups, so that the four reads a wave gathers from
//                      at a time lie 8 banks apart.
constexpr uint32_t kReadWaves = kTileReads / 64u;     // waves of read threads, with a part of the entry area each
constexpr uint32_t kMinWgs = 4u;      // workgroups a CU must be able to hold: 128 registers for the first size (two tiles a workgroup with qualities: 129 without the bound)
// (the mask mode with two tiles a workgroup takes 126 under the same bound; bounded to the five workgroups the LDS leaves room for —
// 96 registers — it spills 88 bytes a lane: the kept plane words of the first tile are 48 of them.  With one tile: 75, five by itself.)
// pieces whose qualities a thread has asked for ahead of their turn (8 registers each; with all seven ahead one tile a workgroup is
// 5 us faster, two tiles a workgroup 11 us slower)
constexpr uint32_t kQualAhead = 3u;
// a row: kRowPieces pieces (above, with the descriptor)
constexpr uint32_t kRowDw = 4u * kRowPieces, kGroupPadDw = 8u;
// The kernel comes in two sizes of its entry area (entries of the reads that need them, 4 bytes each in LDS: column - sweep's first
// (0..256: 9 bits) | kind << 9 | (query offset there - the row's first) << 11): four entries a read on average — a CCS read has 4
// in a sweep with an indel — with five workgroups to a CU, and sixteen, with three: for the (tile, sweep) units whose reads have
// more (an indel every 50 columns), which the first size hands on (ingest_args::big_list) instead of leaving read after read
// to the column-by-column kernel (7 ms for 100k reads with 1 % of indels).
constexpr uint32_t kEntPerRead = 4u, kEntPerReadBig = 16u;
template <uint32_t EPR>
struct planes_shape {
    static constexpr uint32_t kEntCap = EPR * kTileReads, kEntCapWave = kEntCap / kReadWaves;
    static constexpr uint32_t kRowBase = 4u + kEntCap;     // (a side dword per entry: an entry begins inside one block at most)
    static constexpr uint32_t kStageDw = kRowBase + kRowDw * kTileReads + kGroupPadDw * kTileGroups + 4u;
    static __device__ __forceinline__ uint32_t row_dw(uint32_t j) { return kRowBase + kRowDw * j + kGroupPadDw * (j >> 5); }
    static_assert(kRowBase % 4u == 0 && kStageDw * 8u <= 65536u, "16-byte pieces; 16-bit nibble addresses");
};
// the table: 32 entries (16 bits) a read — rows on 8-byte boundaries for the four-entries-at-a-time stores —
// and 8 dwords of padding per 32 reads: the four 32-read groups of a wave's lanes read it 8 banks apart
constexpr uint32_t kTabRow = kBlocks > 16u ? 32u : 16u, kTabGroupPad = 16u;
static_assert(kBlocks <= kTabRow && kBlocks % 4u == 0, "a sweep is at most 32 blocks wide, whole chunks of four");
constexpr uint32_t kTabSize = kTileReads * kTabRow + kTileGroups * kTabGroupPad;
__device__ __forceinline__ uint32_t tab_row(uint32_t j) { return j * kTabRow + (j >> 5) * kTabGroupPad; }
// ... and within a row the chunks of four blocks change places by the read's number: the rows are 16 dwords apart, so that sixty-four
// reads storing the same chunk of their rows met in two bank phases (8 b64 stores of a one-entry row took a sixteenth of their rate:
// 13 of the kernel's 21 x 10^6 LDS cycles were bank conflicts)
__device__ __forceinline__ uint32_t tab_at(uint32_t j, uint32_t blk) { return tab_row(j) + ((((blk >> 2) ^ j) & (kTabRow / 4u - 1u)) << 2) + (blk & 3u); }
static_assert((kTabRow / 4u & (kTabRow / 4u - 1u)) == 0, "chunks of a row: a power of two");
static_assert(kTileReads % 64u == 0 && kThreads == 2u * kTileReads && kBlocks <= 32u, "whole waves of read threads; a block index fits five bits");
// the pieces of a tile: the upper half of the threads take kPieceRoundsB rounds of kTileReads pieces, the read threads — who have
// their rows of the table to make as well — the rest
constexpr uint32_t kPieceRoundsA = kRowPieces >= 8u ? 2u : 1u, kPieceRoundsB = kRowPieces - kPieceRoundsA;

// All the LDS of a planes workgroup: declared once, in ingest_planes_kernel, and handed down.
template <uint32_t EPR>
struct planes_lds {
    using shape = planes_shape<EPR>;
    __attribute__((aligned(16))) uint32_t stage[shape::kStageDw];
    __attribute__((aligned(16))) uint16_t tab[kTabSize];
    uint32_t ent[shape::kEntCap];          // the entries of the reads with several in the sweep, a half per read wave
    uint8_t own[shape::kEntCap];           // whose: the read | 0x80 for its last one
    uint32_t nent[2u * kReadWaves];        // entries in each part; [kReadWaves + w]: wave w hands the unit on
    uint32_t nslow;                        // reads left to slow_pair
    uint8_t slow[kTileReads];
};
static_assert(kTileReads <= 128u, "a read of the tile and a flag in a byte");

// block -> (read tile, sweep).  Blocks b, b + 8, b + 16, ... are dealt to the same XCD one after the other; an XCD takes
// whole groups of 1024 reads (group = xcd, xcd + 8, ...), and of a group all sweeps in turn, the tiles of the group
// innermost.  So (a) the tiles that share the 128-byte lines of a sweep's planes meet in one L2, and (b) what the
// sweeps of a group read again — the reads' entries, the 128-byte lines of packed bases that straddle two sweeps — is
// in that L2 when the next sweep asks for it.
struct unit_place {
    uint32_t xcd, group, tile, sweep;
    uint32_t X, width;       // the sweep's first column, its columns (the window's last sweep: fewer than kSweep)
    uint64_t r0;             // the tile's first read
    bool in_range;           // false: a group past the window's (the grid is whole rounds of the eight XCDs)
};
__device__ __forceinline__ unit_place place_of(const ingest_args &a, uint32_t b)
{
    unit_place p;
    const uint32_t jb = b >> 3, sub = jb % kSubTiles, qq = jb / kSubTiles;
    p.xcd = b & 7u;
    p.group = p.xcd + 8u * (qq / a.n_sweeps);
    p.sweep = qq % a.n_sweeps;
    p.in_range = p.group < a.n_groups;
    p.tile = kSubTiles * p.group + sub;
    p.X = p.sweep * kSweep;
    p.width = min(a.n_cols, p.X + kSweep) - p.X;
    p.r0 = (uint64_t)p.tile * kTileReads;
    return p;
}
// the descriptors of the unit's sweep, by read
__device__ __forceinline__ const uint4 *descs_of(const ingest_args &a, const unit_place &pl) { return a.desc + (uint64_t)pl.sweep * a.n_reads; }


// Eight of BAM's 4-bit bases, one per nibble -> eight symbol codes: A C G T (1 2 4 8) -> 0..3, everything else (N = 15, '=' = 0, the
// IUPAC ambiguity codes) -> N, a filtered base.  v_perm_b32 looks four bytes up in an 8-byte table: the low three bits of a
// base select in the table of the codes 0..7 and in that of 8..15, bit 3 picks between the two results.  (Only the few blocks
// with a run boundary inside go through this: everything else is converted as bit planes, behind the transposition.)
__device__ __forceinline__ uint32_t codes_of_bases8(uint32_t x)
{
    constexpr uint32_t kLo03 = 0x05010005u, kLo47 = 0x05050502u;   // codes of 0..3 (bytes 0..3), of 4..7
    constexpr uint32_t kHi03 = 0x05050503u, kHi47 = 0x05050505u;   // codes of 8..11, of 12..15
    auto lookup4 = [&](uint32_t y) -> uint32_t {   // four bases, one per byte (0..15) -> four codes
        const uint32_t sel = y & 0x07070707u;
        const uint32_t lo = __builtin_amdgcn_perm(kLo47, kLo03, sel), hi = __builtin_amdgcn_perm(kHi47, kHi03, sel);
        const uint32_t b3 = y & 0x08080808u, pick = (b3 << 5) - (b3 >> 3);   // bytes of ones where bit 3 is set
        return (hi & pick) | (lo & ~pick);
    };
    return lookup4(x & 0x0F0F0F0Fu) | (lookup4((x >> 4) & 0x0F0F0F0Fu) << 4);
}

// 16 bytes of packed bases (BAM order: first base in the high nibble) -> the same 32 bases in QUERY order, base b in nibble
// b & 7 of S[b >> 3] — BAM's codes as they are: they become symbol codes as bit planes, behind the transposition, at an
// eighth of the price per base.  QV: bases whose quality is below min_qv become 15 (N).  Q = query offset of the piece's base 0
// (negative: the first -Q bases are not the read's own).
// The qualities of a piece's 32 bases, one byte each: two 16-byte loads at the BYTE address of the first (gfx950 takes unaligned
// dwordx4 loads; Q < 0 — the piece begins up to six bases before the read's own — reads the read before's last bytes, or the 16
// bytes in front of the first read's (jl_records_begin): those bases are nobody's, whatever mask they get).
struct piece_quals { u32x4 a, b; };
__device__ __forceinline__ piece_quals ask_quals(const ingest_args &a, int Q, uint64_t qual_base)
{
    typedef uint32_t u32x4a1 __attribute__((ext_vector_type(4), aligned(1)));
    const uint8_t *qp = a.qual + (int64_t)qual_base + (int64_t)Q;
    piece_quals q;
    q.a = *reinterpret_cast<const u32x4a1 *>(qp);
    q.b = *reinterpret_cast<const u32x4a1 *>(qp + 16);
    return q;
}

// 32 bases in query order (S) and their qualities (pq): a base is masked — becomes 15, N — when its quality is below min_qv (0xFF =
// absent, and anything above 127, never masks).  Eight bases a step, the byte-parallel compare done on the even and on the odd
// bases' bytes apart (v_perm), so that the two results interleave into one flag per NIBBLE — the bases' own layout — with one
// shift: 13 instructions for eight bases (round 5: nine dword loads, eight v_alignbyte, flags gathered into bits and spread again: 30).
__device__ __forceinline__ void mask_low_quals(const ingest_args &a, const piece_quals &pq, uint32_t (&S)[4])
{
    const uint32_t q8[8] = {pq.a.x, pq.a.y, pq.a.z, pq.a.w, pq.b.x, pq.b.y, pq.b.z, pq.b.w};
    const uint32_t T = a.min_qv * 0x01010101u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t ev = __builtin_amdgcn_perm(q8[2 * k + 1], q8[2 * k], 0x06040200u);   // qualities of bases 0 2 4 6 of the eight
        const uint32_t od = __builtin_amdgcn_perm(q8[2 * k + 1], q8[2 * k], 0x07050301u);   // of bases 1 3 5 7
        const uint32_t lt_e = ~((ev | 0x80808080u) - T) & ~ev & 0x80808080u;                // bit 7 of byte i: base 2 i is below min_qv
        const uint32_t lt_o = ~((od | 0x80808080u) - T) & ~od & 0x80808080u;
        const uint32_t c = lt_o | (lt_e >> 4);          // bit 3 of nibble j: base j is masked
        S[k] |= c | (c - (c >> 3));                     // 8 -> 15 (N) in those nibbles
    }
}

// The input modes of the planes kernel: no filter; qualities, a byte a base, compared with min_qv here; the filter made by the
// caller, a bit a base (jl_records_append_masked).
constexpr uint32_t kQvNone = JL_QV_NONE, kQvBytes = JL_QV_BYTES, kQvMask = JL_QV_MASK;   // (jl_internal.h jl_qv_mode)

// The filter of a piece's 32 bases as the caller made it, flag b = base b of the piece: byte k of `fl` goes onto the nibbles of S[k]
// (flag 8 k + j -> nibble j), 15 (N) where it is set — three masked shifts spread eight bits to the low bit of eight nibbles,
// and x 15 fills the nibble: nine instructions for eight bases, against mask_low_quals' thirteen and its eight registers of input.
__device__ __forceinline__ void mask_flagged(uint32_t fl, uint32_t (&S)[4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t t = (fl >> (8 * k)) & 0xFFu;
        t = (t | (t << 12)) & 0x000F000Fu;      // flags 0-3 in bits 0-3, 4-7 in bits 16-19
        t = (t | (t << 6)) & 0x03030303u;       // two a byte
        t = (t | (t << 3)) & 0x11111111u;       // one a nibble
        S[k] |= t * 15u;
    }
}

template <uint32_t QV>
__device__ __forceinline__ void piece_bases(const ingest_args &a, const u32x4 &v, const piece_quals &pq, uint32_t fl, uint32_t (&S)[4])
{
    const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) S[k] = ((w4[k] >> 4) & 0x0F0F0F0Fu) | ((w4[k] & 0x0F0F0F0Fu) << 4);
    if (QV == kQvBytes) mask_low_quals(a, pq, S);
    if (QV == kQvMask) mask_flagged(fl, S);
}

// An entry in LDS, 4 bytes: column - sweep's first (0..256: 9 bits) | kind << 9 | (query offset there - the row's first) << 11.
// From entry {x, y} of runs[], for the sweep that begins at column X and whose row begins at query offset q0:
__device__ __forceinline__ uint32_t ent_make(uint32_t x, uint32_t y, uint32_t X, int32_t q0)
{
    const uint32_t W = entry_col(x), kind = entry_kind(x);
    const uint32_t wr = W <= X ? 0u : min(W - X, 256u);
    const uint32_t yq = y + (W < X ? X - W : 0u);      // query offset at the sweep's first column of the entry
    const uint32_t yr = (kind == kAligned && wr < 256u) ? (yq - (uint32_t)q0) & 0x1FFFu : 0u;
    return wr | (kind << 9) | (yr << 11);
}
__device__ __forceinline__ uint32_t ent_col(uint32_t e) { return e & 511u; }
__device__ __forceinline__ uint32_t ent_kind(uint32_t e) { return (e >> 9) & 3u; }
// staging nibble address of column c (relative to the sweep's first) in entry e of a read whose row begins at nibble row8
__device__ __forceinline__ uint32_t ent_addr(uint32_t e, uint32_t row8, uint32_t c)
{
    const uint32_t kind = ent_kind(e);
    return kind == 1u ? row8 + (e >> 11) + (c - ent_col(e)) : kind == 2u ? 16u : 0u;
}

// ---------------------------------------------------------------------------------------- what a tile cannot take
// A (read, sweep) pair with more pieces or entries than a workgroup has room for, by ONE WAVE of the tile's own workgroup,
// behind its stores: a lane per column looks its entry up in HBM and flips the bits in which the symbol differs from 'not
// covered' — which is what the workgroup has stored for the read (the words are the tile's own: 32 reads of it each).
__device__ __forceinline__ void slow_pair(const ingest_args &a, uint64_t r, uint32_t sweep, uint32_t lane)
{
    const int X = (int)(sweep * kSweep), Xend = (int)min(a.n_cols, sweep * kSweep + kSweep);
    const uint2 *runs = a.runs + a.cig_off[r] + 3u * r;
    const uint32_t ne = a.nruns[r] + 3u;
    const uint64_t so = a.seq_off[r];
    const uint64_t qo = a.qual ? a.qual_off[r] : 0u;
    for (int c = X + (int)lane; c < Xend; c += 64) {
        uint32_t lo = 0, hi = ne - 1u;   // the last entry that begins at or before c (entry 0 does, the last one never)
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if ((int)entry_col(runs[mid].x) <= c) lo = mid;
            else hi = mid;
        }
        const uint2 e = runs[lo];
        const uint32_t kind = entry_kind(e.x);
        uint32_t sym = 6u;
        if (kind == kDeletion) sym = 4u;
        else if (kind == kAligned) {
            const uint64_t q = (uint64_t)e.y + (uint64_t)(c - (int)entry_col(e.x));
            const uint32_t by = a.seq4[so + (q >> 1)];
            const uint32_t b16 = (q & 1u) ? (by & 15u) : (by >> 4);
            sym = (uint32_t)((0x5555555355525105ull >> (4u * b16)) & 15ull);   // A=1 C=2 G=4 T=8 -> 0..3, else 5
            if (a.qual) {
                const uint32_t qv = a.qual[qo + q];
                if (qv != 0xFFu && qv < a.min_qv) sym = JL_SYM_MASK;
            }
            if (a.qmask) {
                const uint64_t i = 2u * so + q;      // (the mask is laid out by the resident bases: a bit a nibble)
                if ((a.qmask[i >> 3] >> (uint32_t)(i & 7u)) & 1u) sym = JL_SYM_MASK;
            }
        }
        const uint32_t flip = sym ^ 6u;
        const uint32_t bit = 1u << (uint32_t)(r & 31u);
#pragma unroll
        for (uint32_t k = 0; k < 3u; ++k)
            if ((flip >> k) & 1u)
                atomicXor(reinterpret_cast<uint32_t *>(a.msa + ((uint64_t)c * 3u + k) * a.plane_stride + (r >> 5) * 4u), bit);
    }
}

// A workgroup = 128 reads x one sweep, four waves with two jobs.  Nothing a thread asks HBM for depends on another thread: every
// thread reads the descriptors of the reads whose pieces it takes itself (neighbouring lanes share them), so the two trips —
// descriptor, then pieces / entries — are the only waits before the first barrier, and there are two barriers in all.
//   waves 2, 3  pieces: thread t takes pieces t, t + 128, ... of the tile's 128 x kRowPieces (7 of 9 rounds), 16 bytes = 32 bases
//               each -> codes -> the staging area in query order.
//   waves 0, 1  a thread per read: its descriptor -> the row of the table (one entry covers the sweep: at once; several: an entry
//               at a time when they have arrived), the boundary blocks listed; then the other 2 rounds of pieces.
//   barrier; the listed blocks put together, a thread each; barrier; gather at the transpose (waves 0, 1).
// (Device stamps of the form before this one — the read waves made the table while the others waited, then everybody staged:
// descriptor 0.75 us, prologue 0.9, table 4.7 of which 1.5 a third trip for the reads with more than four entries, staging 1.8,
// general 1.1, transposing 2.6; waves 2, 3 waited 5.2 us of 14.6 at the first barrier.)
// DEFER (the first size, several sibling tiles a workgroup: ingest_planes_kernel): the unit's plane words are handed back in `keep`
// instead of being stored — returns whether the unit made any (false: outside the window's groups, or handed on) — and a read
// the workgroup has no room for hands the unit on instead of going through slow_pair (whose bit flips need the stores done).
// ---- pieces.  The pieces p0, p0 + 128, ... (K of them) of the tile's 128 x kRowPieces: the descriptors of their reads, then the
// pieces, all of a thread's requests in flight together; a piece that is not there (the read has fewer) asks for the read's first
// one again — the same number of requests in every lane, so that a wait for something asked earlier does not wait for these.
struct piece_t { u32x4 v; uint32_t dst; int32_t Q; uint64_t qb; uint32_t fl; };    // dst: dword in the staging area, 0 = none; fl: the piece's 32 flags (kQvMask)
// (every load is asked for whatever the read's number — a read past the last asks for the first one's, and is set to nothing
// afterwards: loads inside a branch made the compiler wait for each before it asked for the next)
template <uint32_t QV>
__device__ __forceinline__ void ask_descs(const ingest_args &a, const unit_place &pl, uint32_t p0, uint32_t K, uint4 (&d)[kPieceRoundsB], uint64_t (&qo)[kPieceRoundsB])
{
    const uint4 *desc = descs_of(a, pl);
    bool in[kPieceRoundsB];
#pragma unroll
    for (uint32_t k = 0; k < kPieceRoundsB; ++k) {
        if (k >= K) break;
        const uint32_t j = (p0 + kTileReads * k) / kRowPieces;
        in[k] = pl.r0 + j < a.n_reads;
        const uint64_t at = in[k] ? pl.r0 + j : 0u;
        d[k] = desc[at];
        qo[k] = QV == kQvBytes ? a.qual_off[at] : 0u;
    }
#pragma unroll
    for (uint32_t k = 0; k < kPieceRoundsB; ++k) {
        if (k >= K) break;
        if (!in[k]) {
            d[k] = make_uint4(0, 0, 0, 0);
            qo[k] = 0;
        }
    }
}
template <uint32_t QV, uint32_t EPR>
__device__ __forceinline__ void ask_pieces(const ingest_args &a, uint32_t p0, uint32_t K, const uint4 (&d)[kPieceRoundsB], const uint64_t (&qo)[kPieceRoundsB], piece_t (&pc)[kPieceRoundsB])
{
    typedef uint32_t u32a1 __attribute__((aligned(1)));
#pragma unroll
    for (uint32_t k = 0; k < kPieceRoundsB; ++k) {
        if (k >= K) break;
        const uint32_t p = p0 + kTileReads * k, j = p / kRowPieces, i = p - kRowPieces * j;
        const uint32_t np = desc_slow(d[k]) ? 0u : desc_pieces(d[k]);      // (slow_pair's: none)
        const uint64_t at = desc_piece_dw(d[k]) + (i < np ? 4u * i : 0u);     // (in dwords)
        // (plain loads: neighbouring lanes' pieces share lines, and so do the sweeps of a read)
        pc[k].v = *reinterpret_cast<const u32x4a4 *>(a.seq4 + 4u * at);
        // (kQvMask: the piece begins at byte 4 at of the bases = bit 8 at of the mask, its 32 flags are the four bytes from byte
        // `at` on — one register a piece, asked for WITH the piece: all of a thread's requests are out before the first is used)
        if (QV == kQvMask) pc[k].fl = *reinterpret_cast<const u32a1 *>(a.qmask + at);
        pc[k].dst = i < np ? planes_shape<EPR>::row_dw(j) + 4u * i : 0u;
        pc[k].Q = desc_q0(d[k]) + (i < np ? 32 * (int32_t)i : 0);      // (a piece that is not there: its read's first one's qualities)
        pc[k].qb = qo[k];
    }
}
// (QV: a piece's qualities are asked for kQualAhead pieces ahead of its turn, outside any branch — the loads of a piece that is
// not there ask for its read's first piece's again.  Asked for inside the piece's own turn, as round 5 had it, every piece
// of a thread waited for its own trip to HBM, seven in a row: 184 us against 111 without qualities.)
template <uint32_t QV, uint32_t EPR>
__device__ __forceinline__ void stage_pieces(const ingest_args &a, planes_lds<EPR> &lds, uint32_t K, const piece_t (&pc)[kPieceRoundsB])
{
    piece_quals pq[kPieceRoundsB];
    if (QV == kQvBytes) {
#pragma unroll
        for (uint32_t k = 0; k < kPieceRoundsB; ++k)
            if (k < K && k < kQualAhead) pq[k] = ask_quals(a, pc[k].Q, pc[k].qb);
    }
#pragma unroll
    for (uint32_t k = 0; k < kPieceRoundsB; ++k) {
        if (k >= K) break;
        if (QV == kQvBytes && k + kQualAhead < K && k + kQualAhead < kPieceRoundsB) pq[k + kQualAhead] = ask_quals(a, pc[k + kQualAhead].Q, pc[k + kQualAhead].qb);
        if (pc[k].dst) {
            uint32_t S[4];
            piece_bases<QV>(a, pc[k].v, pq[k], pc[k].fl, S);
            u32x4 o = {S[0], S[1], S[2], S[3]};
            *reinterpret_cast<u32x4 *>(&lds.stage[pc[k].dst]) = o;
        }
    }
}

// ---- the stages of a unit (planes_unit below), in their order.  `tid` is the unit's own copy of the thread's number (planes_unit).
// pieces_stage — waves 2, 3, before the first barrier.  Reads the descriptors and the packed bases (qualities, flags) of the
// pieces tid - 128, + 128, ... (kPieceRoundsB rounds: 7 of 9); writes their codes, in query order, to lds.stage's rows.  Needs
// nothing of the workgroup to be complete: what it asks HBM for depends on no other thread.
template <uint32_t QV, uint32_t EPR>
__device__ __forceinline__ void pieces_stage(const ingest_args &a, const unit_place &pl, planes_lds<EPR> &lds, uint32_t tid)
{
    uint4 d[kPieceRoundsB];
    uint64_t qo[kPieceRoundsB];
    piece_t pc[kPieceRoundsB];
    const uint32_t p0 = tid - kTileReads;
    ask_descs<QV>(a, pl, p0, kPieceRoundsB, d, qo);
    ask_pieces<QV, EPR>(a, p0, kPieceRoundsB, d, qo, pc);
    stage_pieces<QV, EPR>(a, lds, kPieceRoundsB, pc);
}

// the table row of a read whose sweep ONE entry covers (or nothing the workgroup takes: kind 3): its blocks' addresses rise by
// eight codes a block (aligned bases, from nibble a0) or stay (the dword of '-', of 'not covered'), four blocks a store
template <uint32_t EPR>
__device__ __forceinline__ void table_row_of_one_entry(planes_lds<EPR> &lds, uint32_t tid, uint32_t kind, uint32_t first_nibble)
{
    const uint32_t a0 = kind == kAligned ? first_nibble : kind == kDeletion ? 16u : 0u, st = kind == kAligned ? 8u : 0u;
    uint32_t lo = a0 | ((a0 + st) << 16), hi = lo + 2u * (st | st << 16);
    const uint32_t step = 4u * (st | st << 16);
#pragma unroll
    for (uint32_t k = 0; k < kBlocks / 4u; ++k) {
        *reinterpret_cast<uint2 *>(lds.tab + tab_at(tid, 4u * k)) = make_uint2(lo, hi);
        lo += step;
        hi += step;
    }
}

// read_stage — waves 0, 1, a thread per read, before the first barrier.  Reads the read's descriptor, the sweep's entries of the
// read from runs[] and the other kPieceRoundsA rounds of pieces; writes the constant dwords in front of lds.stage, the counters
// (lds.nent, lds.nslow: zero before anybody adds), the read's row of lds.tab when one entry covers the sweep, otherwise its entries
// and their owners to its wave's part of lds.ent / lds.own, and its pieces' codes to lds.stage.  Needs nothing complete on entry
// (the barrier between units has passed).  Returns whether the read is left to slow_pair; a wave that hands the unit on says so in
// lds.nent[kReadWaves + wave].
template <uint32_t QV, uint32_t EPR, bool BIG, bool DEFER>
__device__ __forceinline__ bool read_stage(const ingest_args &a, const unit_place &pl, planes_lds<EPR> &lds, uint32_t tid)
{
    using shape = planes_shape<EPR>;
    typedef uint32_t u32x4a8 __attribute__((ext_vector_type(4), aligned(8)));
    const uint32_t wid = tid >> 6, lane = tid & 63u;
    uint4 dp[kPieceRoundsB];
    uint64_t qo[kPieceRoundsB];
    piece_t pc[kPieceRoundsB];
    const uint32_t p0 = kTileReads * kPieceRoundsB + tid;
    const uint64_t r = pl.r0 + tid;
    uint4 d = desc_of_no_read();
    if (r < a.n_reads) d = descs_of(a, pl)[r];
    ask_descs<QV>(a, pl, p0, kPieceRoundsA, dp, qo);
    if (tid < 4u) lds.stage[tid] = tid < 2u ? 0x66666666u : 0x44444444u;
    if (tid == 4u) lds.nslow = 0;
    if (lane == 0) lds.nent[wid] = 0, lds.nent[kReadWaves + wid] = 0;
    uint32_t n_ent = desc_entries(d);
    bool slow = desc_slow(d);
    const bool simple = desc_simple(d);
    if (simple || slow) n_ent = 0;
    // exclusive scan of the entries over the wave: each read wave has its own half of the entry area
    const uint32_t inc = wave_scan(n_ent);
    uint32_t off_e = inc - n_ent;
    if (n_ent && off_e + n_ent > shape::kEntCapWave) {
        // more entries than the wave's part holds: the first size hands the whole unit on to the second (nothing of it is
        // written here, and no read of it goes to the slow list: the second size lists its own); the second leaves the
        // reads past the part's end to slow_pair
        if (!BIG) lds.nent[kReadWaves + wid] = 1u;
        else slow = true;
        n_ent = 0;
    }
    if (DEFER && slow) {
        lds.nent[kReadWaves + wid] = 1u;
        slow = false;
    }
    off_e += wid * shape::kEntCapWave;
    // the sweep's entries of this read: the first eight in four 16-byte requests that go out together (entries past the
    // read's own belong to the next read or to the array's slack) — two deletions in a sweep are six entries, and a
    // wave in which ONE read needs a ninth makes another trip for it
    const uint2 *src = a.runs + (n_ent ? desc_entry_idx(d) : 0u);
    u32x4a8 e01 = {0, 0, 0, 0}, e23 = e01, e45 = e01, e67 = e01;
    if (n_ent) {
        e01 = *reinterpret_cast<const u32x4a8 *>(src);
        e23 = *reinterpret_cast<const u32x4a8 *>(src + 2);
    }
    if (n_ent > 4u) {
        e45 = *reinterpret_cast<const u32x4a8 *>(src + 4);
        e67 = *reinterpret_cast<const u32x4a8 *>(src + 6);
    }
    ask_pieces<QV, EPR>(a, p0, kPieceRoundsA, dp, qo, pc);
    const int32_t q0 = desc_q0(d);
    if (!n_ent) table_row_of_one_entry(lds, tid, (simple && !slow) ? desc_simple_kind(d) : kNothing, 8u * shape::row_dw(tid) + (desc_simple_q(d) - (uint32_t)q0));
    // several entries: -> LDS, four bytes each, with their owner; everybody makes table rows of them behind the barrier
    if (n_ent) {
        const uint32_t X = pl.X;
        const uint32_t e8[8] = {ent_make(e01.x, e01.y, X, q0), ent_make(e01.z, e01.w, X, q0), ent_make(e23.x, e23.y, X, q0), ent_make(e23.z, e23.w, X, q0),
                                ent_make(e45.x, e45.y, X, q0), ent_make(e45.z, e45.w, X, q0), ent_make(e67.x, e67.y, X, q0), ent_make(e67.z, e67.w, X, q0)};
        uint32_t *ent = lds.ent + off_e;
        uint8_t *own = lds.own + off_e;
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i)
            if (i < n_ent) {
                ent[i] = e8[i];
                own[i] = (uint8_t)(tid | (i + 1u == n_ent ? 0x80u : 0u));
            }
        for (uint32_t i = 8; i < n_ent; ++i) {
            const uint2 g = src[i];
            ent[i] = ent_make(g.x, g.y, X, q0);
            own[i] = (uint8_t)(tid | (i + 1u == n_ent ? 0x80u : 0u));
        }
        atomicMax(&lds.nent[wid], off_e - wid * shape::kEntCapWave + n_ent);
    }
    stage_pieces<QV, EPR>(a, lds, kPieceRoundsA, pc);
    return slow;
}

// table_stage — everybody, between the two barriers: a thread an entry.  Reads lds.nent, lds.ent, lds.own and, for the boundary
// blocks, the codes in lds.stage's rows; writes the table rows of the reads with several entries and the side dwords
// lds.stage[4 + slot].  Needs read_stage and pieces_stage complete in every wave: behind the first barrier.
// Entry i of a read covers the columns [its column, the next entry's column) and the read's last one only ends the one before
// it: the blocks that lie WHOLLY inside are the entry's — addresses that rise by eight codes a block, or the dword of '-' /
// of 'not covered' — and every block is wholly inside one entry or has an entry that begins inside it; those are put
// together, by the thread of the first such entry, in that entry's side dword.  No list, no search, no loop per block.
// (a) the whole blocks [bf, be) of entry e of read `own`, from nibble address av on: singly up to a multiple of four, four a store, singly again
template <uint32_t EPR>
__device__ __forceinline__ void table_whole_blocks(planes_lds<EPR> &lds, uint32_t own, uint32_t e, uint32_t bf, uint32_t be)
{
    const uint32_t st = ent_kind(e) == 1u ? 8u : 0u;
    uint32_t av = ent_addr(e, 8u * planes_shape<EPR>::row_dw(own), 8u * bf);
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k)
        if ((bf & 3u) && bf < be) {
            lds.tab[tab_at(own, bf)] = (uint16_t)av;
            av += st;
            ++bf;
        }
    uint32_t p01 = av | ((av + st) << 16);
    const uint32_t p_st = st | st << 16;
    for (; bf + 4u <= be; bf += 4u) {
        *reinterpret_cast<uint2 *>(lds.tab + tab_at(own, bf)) = make_uint2(p01, p01 + 2u * p_st);
        p01 += 4u * p_st;
    }
    av = p01 & 0xFFFFu;
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k)
        if (bf < be) {
            lds.tab[tab_at(own, bf)] = (uint16_t)av;
            av += st;
            ++bf;
        }
}
// (b) the block bb that the entry at `slot` begins inside, put together from the entries around it: the one before (an entry
// that begins inside a block is not its read's first) up to the first that ends behind the block
template <uint32_t EPR>
__device__ __forceinline__ void table_boundary_block(planes_lds<EPR> &lds, uint32_t slot, uint32_t own, uint32_t bb)
{
    const uint32_t row8 = 8u * planes_shape<EPR>::row_dw(own);
    uint32_t ee = lds.ent[slot - 1u];
    const uint32_t c0 = 8u * bb, c1 = c0 + 8u;
    uint32_t bases = 0, m_al = 0, m_del = 0;      // the block's aligned bases (BAM's codes), where they are, where a deletion is
    for (uint32_t kk = slot;; ++kk) {
        const uint32_t nn = lds.ent[kk];
        const uint32_t W = ent_col(ee), Wn = ent_col(nn);
        const uint32_t ca = max(W, c0), cb = min(Wn, c1);
        const uint32_t kind = ent_kind(ee);
        if (ca < cb && kind != 3u) {
            const uint32_t m = (cb - ca == 8u ? 0xFFFFFFFFu : ((1u << (4u * (cb - ca))) - 1u)) << (4u * (ca - c0));
            if (kind == 1u) {
                const uint32_t A = ent_addr(ee, row8, ca);
                bases |= (__builtin_amdgcn_alignbit(lds.stage[(A >> 3) + 1u], lds.stage[A >> 3], 4u * (A & 7u)) << (4u * (ca - c0))) & m;
                m_al |= m;
            } else m_del |= m;
        }
        if (Wn >= c1 || (lds.own[kk] & 0x80u)) break;     // (the read's last entry is nothing: 'not covered' stays)
        ee = nn;
    }
    const uint32_t R = (codes_of_bases8(bases) & m_al) | (0x44444444u & m_del) | (0x66666666u & ~(m_al | m_del));
    lds.stage[4u + slot] = R;
    lds.tab[tab_at(own, bb)] = (uint16_t)(8u * (4u + slot));
}
template <uint32_t EPR>
__device__ __forceinline__ void table_stage(planes_lds<EPR> &lds, uint32_t width, uint32_t tid)
{
    constexpr uint32_t kEntCapWave = planes_shape<EPR>::kEntCapWave;
    uint32_t n_e = 0;
#pragma unroll
    for (uint32_t w = 0; w < kReadWaves; ++w) n_e += lds.nent[w];
    for (uint32_t si = tid; si < n_e; si += kThreads) {
        uint32_t slot = 0, rem = si;      // the si-th entry of the parts one behind the other
        bool found = false;
#pragma unroll
        for (uint32_t w = 0; w < kReadWaves; ++w) {
            const uint32_t nw = lds.nent[w];
            if (!found && rem < nw) {
                slot = w * kEntCapWave + rem;
                found = true;
            }
            if (!found) rem -= nw;
        }
        const uint32_t own = lds.own[slot], e = lds.ent[slot], nx = lds.ent[slot + 1u];
        const uint32_t wr = ent_col(e);
        if ((own & 0x80u) || wr >= width) continue;
        const uint32_t wn = ent_col(nx);
        const uint32_t be = wn >= width ? kBlocks : wn >> 3, bf = (wr + 7u) >> 3;
        if (bf < be) table_whole_blocks(lds, own, e, bf, be);
        // ... the block it begins inside, if it is the first entry to do so
        if (!(wr & 7u)) continue;
        if (ent_col(lds.ent[slot - 1u]) > 8u * (wr >> 3)) continue;
        table_boundary_block(lds, slot, own, wr >> 3);
    }
}

// gather_stage — behind the second barrier: the table and the staging area are complete.  GATHER AT THE TRANSPOSE: thread = 32
// reads x 8 columns (group G = tid % kTileGroups of the tile's reads, block tid / kTileGroups); reads lds.tab and lds.stage only,
// writes out[j][k] = the dword of plane k of the block's column j.  Returns whether the thread has a block of the sweep (false: `out`
// is not written).
template <uint32_t EPR>
__device__ __forceinline__ bool gather_stage(const planes_lds<EPR> &lds, uint32_t width, uint32_t tid, uint32_t (&out)[8][3])
{
    const uint32_t G = tid % kTileGroups, blk = tid / kTileGroups;
    if (!(blk < kBlocks && 8u * blk < width)) return false;
    // (the dwords in front of the reads' rows — 'not covered', '-', the boundary blocks — hold symbol codes already; `codes`
    // collects, a bit a read, whose dword is one of those: v_alignbit shifts the sign of address - first row in)
    uint32_t R[32], codes = 0;
    // (the block's place in the rows of the reads i, i + 8, ...: eight offsets)
    uint32_t at[8];
#pragma unroll
    for (uint32_t i = 0; i < 8u; ++i) at[i] = tab_at(32u * G + i, blk);
#pragma unroll
    for (int i = 31; i >= 0; --i) {
        const uint32_t A = lds.tab[at[i & 7] + (uint32_t)(i & ~7) * kTabRow];
        R[i] = __builtin_amdgcn_alignbit(lds.stage[(A >> 3) + 1u], lds.stage[A >> 3], 4u * (A & 7u));
        codes = __builtin_amdgcn_alignbit(codes, A - 8u * planes_shape<EPR>::kRowBase, 31u);
    }
    nibble_rows_to_plane_words(R, codes, out);
    return true;
}

// The plane words of a block of eight columns -> the matrix: words[j][k] to row + (3 j + k) * stride, the first columns_valid (> 0)
// columns of the block.  A block of eight whole columns — all but the window's last — stores without a question per column (a
// predicate per store was a sixth of the single tile's store phase); the ragged one, the window's last, goes column by column.
__device__ __forceinline__ void store_block_words(uint8_t *row, uint64_t stride, const uint32_t (&words)[8][3], uint32_t columns_valid)
{
    if (columns_valid >= 8u) {
#pragma unroll
        for (uint32_t jj = 0; jj < 8u; ++jj)
#pragma unroll
            for (uint32_t k = 0; k < 3u; ++k) {
                *reinterpret_cast<uint32_t *>(row) = words[jj][k];
                row += stride;
            }
    } else {
        // (a loop over the columns there are, the word picked by comparisons: stores under a predicate each, unrolled, had the
        // compiler merge them behind a computed address — the words went to scratch)
        for (uint32_t jj = 0; jj < columns_valid; ++jj)
            for (uint32_t k = 0; k < 3u; ++k) {
                *reinterpret_cast<uint32_t *>(row) = jj == 0u ? words[0][k] : jj == 1u ? words[1][k] : jj == 2u ? words[2][k] : jj == 3u ? words[3][k] : jj == 4u ? words[4][k] : jj == 5u ? words[5][k] : words[6][k];
                row += stride;
            }
    }
}

// A workgroup = 128 reads x one sweep, four waves with two jobs.  Nothing a thread asks HBM for depends on another thread: every
// thread reads the descriptors of the reads whose pieces it takes itself (neighbouring lanes share them), so the two trips —
// descriptor, then pieces / entries — are the only waits before the first barrier, and there are two barriers in all (a third in
// front of the slow tail).
// (Device stamps of the form before this one — the read waves made the table while the others waited, then everybody staged:
// descriptor 0.75 us, prologue 0.9, table 4.7 of which 1.5 a third trip for the reads with more than four entries, staging 1.8,
// general 1.1, transposing 2.6; waves 2, 3 waited 5.2 us of 14.6 at the first barrier.)
// The unit's plane words come back in `out` (the thread's block of eight columns: gather_stage).  Returns whether the unit made
// any — false: outside the window's groups, or handed on to the second size (BIG: never); the same in every thread of the workgroup.
// DEFER (the first size, several sibling tiles a workgroup: ingest_planes_kernel): the words are NOT stored here, and a read the
// workgroup has no room for hands the unit on instead of going through slow_pair (whose bit flips need the stores done).
template <uint32_t QV, uint32_t EPR, bool BIG, bool DEFER = false>
__device__ __forceinline__ bool planes_unit(const ingest_args &a, const uint32_t b, planes_lds<EPR> &lds, uint32_t (&out)[8][3])
{
    uint32_t tid_ = threadIdx.x;
    if (DEFER) asm volatile("" : "+v"(tid_));      // (the units of a workgroup run in a loop: what follows from the thread's number is not to be
                                                   // kept in registers across it — hoisted, it was 110 of them)
    const uint32_t tid = tid_;
    const unit_place pl = place_of(a, b);
    if (!pl.in_range) return false;
    // WITHOUT QUALITIES a wave that still has its requests to HBM to make and its rows to stage goes before the waves that transpose
    // (s_setprio: the CU's arbiter picks by it among the waves ready to issue).  Without it the transposing waves of the CU's other
    // workgroups — three quarters of all instructions — hold up the few instructions that put the next tile's loads in flight: the
    // launch 110-113 -> 100-107 us, a whole build 171 -> 164 us on one stream and 159 -> 152 with two builds overlapping.  With
    // qualities the launch alone gains 3 us of 169 and the build LOSES 3-7 (two streams: 191 -> 198; in bench.py's once_through_qv
    // 185 -> 202): its raised waves also go before the waves of whatever else is on the device — the next build's cigar walk, the
    // pileup and the phasing of the windows before — so there it stays off.  (Raised only until the loads are out: the same;
    // raised for the transposing instead: 116 / 176.)
    constexpr bool kPrio = QV == kQvNone;
    if (kPrio) __builtin_amdgcn_s_setprio(3);
    bool slow_read = false;
    if (tid >= kTileReads) pieces_stage<QV, EPR>(a, pl, lds, tid);
    else slow_read = read_stage<QV, EPR, BIG, DEFER>(a, pl, lds, tid);
    __syncthreads();
    // ---- the hand-on check (the first size): a read wave had more entries than its part holds (DEFER: or a read for slow_pair)
    if (!BIG) {
        uint32_t handed = 0;
#pragma unroll
        for (uint32_t w = 0; w < kReadWaves; ++w) handed |= lds.nent[kReadWaves + w];
        if (handed) {
            if (tid == 0) a.big_list[atomicAdd(a.slow_count + 1, 1u)] = b;
            return false;
        }
    }
    if (slow_read) lds.slow[atomicAdd(&lds.nslow, 1u)] = (uint8_t)tid;      // (its row of the table says 'not covered')
    table_stage(lds, pl.width, tid);
    __syncthreads();
    const uint32_t n_slow = lds.nslow;
    if (kPrio) __builtin_amdgcn_s_setprio(0);
    const bool act = gather_stage(lds, pl.width, tid, out);
    if (!DEFER && act) {
        const uint32_t G = tid % kTileGroups, blk = tid / kTileGroups;
        const uint64_t byte = (uint64_t)pl.tile * (kTileReads / 8u) + (uint64_t)G * 4u;
        // (one 64-bit multiply for the first plane row, then a stride at a time)
        if (byte < a.plane_stride) store_block_words(a.msa + (uint64_t)((pl.X + 8u * blk) * 3u) * a.plane_stride + byte, a.plane_stride, out, pl.width - 8u * blk);
    }
    // ---- the slow tail, the reads left out (none, in a CCS sample): column by column behind the workgroup's own stores, a wave a read
    if (!DEFER && n_slow) {       // (the same in every thread)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (uint32_t i = tid >> 6; i < n_slow; i += kThreads / 64u) slow_pair(a, pl.r0 + lds.slow[i], pl.sweep, tid & 63u);
    }
    return true;
}

// The first size: a workgroup a unit (blockIdx -> unit: planes_unit).  The second: the units the first handed on, in the
// order they came, taken in turns by a grid that fills the chip once (an empty list costs a launch of 768 workgroups).
constexpr uint32_t kBigGrid = 768u;
// NT (the first size): sibling tiles a workgroup takes one after the other, their plane words kept in registers and stored
// TOGETHER at the end — NT x 16 bytes of a line a request instead of 16.  The L2 takes a write request per (row, tile): 7 x 10^6 a
// window, more than all its read requests; the same bytes as 64-byte requests (a probe, round 6) took 19 us off the
// launch's 113 and 29 off the 180 with qualities.  The tiles' words change places between the lanes of a DPP row (16 lanes = four
// blocks of 8 columns x four 32-read groups): the lane at position u of a pair of blocks ends up with tile u's words of both
// blocks (two DPP moves a word), and 4 NT neighbouring lanes write NT x 16 contiguous bytes of a row.  (Four tiles a workgroup
// were slower: see jl_launch_ingest.)
template <uint32_t QV, uint32_t EPR, bool BIG, uint32_t NT = 1u>
__global__ __launch_bounds__(kThreads, (BIG ? 1 : kMinWgs)) void ingest_planes_kernel(ingest_args a)
{
    static_assert(NT == 1u || NT == 2u, "one tile a workgroup, or two");
    __shared__ planes_lds<EPR> lds;
    if constexpr (BIG) {
        uint32_t none[8][3];
        const uint32_t n = a.slow_count[1];
        for (uint32_t u = blockIdx.x; u < n; u += gridDim.x) {
            planes_unit<QV, EPR, true>(a, a.big_list[u], lds, none);
            __syncthreads();      // (the next unit's LDS)
        }
    } else if constexpr (NT == 1u) {
        uint32_t none[8][3];
        planes_unit<QV, EPR, false>(a, blockIdx.x, lds, none);
    } else {
        // workgroup w -> the units (planes_unit's block numbers) of NT consecutive tiles of one (group, sweep), on w's XCD
        const uint32_t w = blockIdx.x, xcd = w & 7u, jw = w >> 3, h = jw % (kSubTiles / NT), qq = jw / (kSubTiles / NT);
        const uint32_t b0 = xcd + 8u * (qq * kSubTiles + NT * h);
        uint32_t D[NT][8][3];
        uint32_t ok = 0;
#pragma unroll 1
        for (uint32_t i = 0; i < NT; ++i) {
            // (the words kept so far move down a place: after the last tile D[t] is tile t's)
#pragma unroll
            for (uint32_t t = 0; t + 1u < NT; ++t)
#pragma unroll
                for (uint32_t jj = 0; jj < 8u; ++jj)
#pragma unroll
                    for (uint32_t k = 0; k < 3u; ++k) D[t][jj][k] = D[t + 1u][jj][k];
            const bool got = planes_unit<QV, EPR, false, true>(a, b0 + 8u * i, lds, D[NT - 1u]);
            ok = (ok >> 1) | (got ? 1u << (NT - 1u) : 0u);
            __syncthreads();      // (the next tile's LDS)
        }
        if (!ok) return;
        const uint32_t tid = threadIdx.x;
        if (tid >= kTileGroups * kBlocks) return;           // (the transposing threads)
        const uint32_t G = tid % kTileGroups, blk = tid / kTileGroups, u = blk & (NT - 1u);
        // ---- the two tiles' words change places between neighbouring blocks: lanes of an even block take the partner's (4 lanes
        // up) tile-0 words into slot 1, the others the partner's tile-1 words into slot 0 (bank = block within the row)
#pragma unroll
        for (uint32_t jj = 0; jj < 8u; ++jj)
#pragma unroll
            for (uint32_t k = 0; k < 3u; ++k) {
                const int x0 = (int)D[0][jj][k], x1 = (int)D[1][jj][k];
                D[1][jj][k] = (uint32_t)__builtin_amdgcn_update_dpp(x1, x0, 0x104, 0xF, 0x5, false);   // row_shl:4, banks 0 2
                D[0][jj][k] = (uint32_t)__builtin_amdgcn_update_dpp(x0, x1, 0x114, 0xF, 0xA, false);   // row_shr:4, banks 1 3
            }
        // ---- D[p] = this lane's tile's (tile u of the NT) words of block (blk & ~(NT - 1)) + p: NT x 4 lanes a row
        if (!((ok >> u) & 1u)) return;                      // (this lane's tile was handed on)
        const unit_place pl = place_of(a, b0);              // (the first of the sibling tiles: the lane's is u behind it)
        const uint64_t byte = (uint64_t)(pl.tile + u) * (kTileReads / 8u) + (uint64_t)G * 4u;
#pragma unroll
        for (uint32_t p = 0; p < NT; ++p) {
            const uint32_t bp = (blk & ~(NT - 1u)) + p;
            if (8u * bp >= pl.width) continue;
            store_block_words(a.msa + (uint64_t)((pl.X + 8u * bp) * 3u) * a.plane_stride + byte, a.plane_stride, D[p], pl.width - 8u * bp);
        }
    }
}

// the planes kernel's two launches of a build: the first size, NT sibling tiles a workgroup, and the second behind it
template <uint32_t QV, uint32_t NT>
void launch_planes(const ingest_args &a, uint32_t units, hipStream_t st)
{
    hipLaunchKernelGGL((ingest_planes_kernel<QV, kEntPerRead, false, NT>), dim3(units / NT), dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL((ingest_planes_kernel<QV, kEntPerReadBig, true>), dim3(kBigGrid), dim3(kThreads), 0, st, a);
}

}  // namespace

uint32_t jl_ingest_sweeps(uint32_t n_cols) { return (n_cols + kSweep - 1u) / kSweep; }

// the planes kernel's workgroups: (groups of 1024 reads per XCD, rounded up) x sweeps x 8 XCDs x tiles of a group
static uint32_t planes_units(const jl_ctx *ctx)
{
    const uint32_t groups = (uint32_t)(ctx->plane_stride * 8u / 1024u);    // (a multiple of 1024 reads: whole line groups of tiles)
    return (groups + 7u) / 8u * jl_ingest_sweeps(ctx->n_cols) * 8u * kSubTiles;
}

// pairs (8 bytes) of d_slow: the units handed on (a word each)
size_t jl_ingest_slow_room(const jl_ctx *ctx) { return (size_t)planes_units(ctx) / 2u + 8u; }

// cigar_walk_kernel's rule (cigar_rules.h: the same functions on the host) — which reads it leaves to the long-read launch (more than
// kWalkOps ops, or more entries than a read has room for in its LDS) — for the upload (jl_records_append), which looks at the few reads of a CCS sample with more
// ops than a read has entries: when it finds none, jl_launch_ingest does not make that launch.
uint32_t jl_ingest_short_ops() { return jl_cigar::kWalkEnt - 3u; }      // a read of so many ops at most cannot be a long one
bool jl_ingest_read_is_long(const uint32_t *cigar, uint64_t n_ops) { return jl_cigar::read_is_long(cigar, n_ops); }

// The scratch of `dst` (capi_records.hip records_build): runs, n_cig + 3 n_reads + 8 entries; nruns, n_reads; desc, n_reads x sweeps
// descriptors; slow, jl_ingest_slow_room() pairs.
// d_count, 64 bytes: [0] retired (zeroed, never read), [1] units handed on — zeroed by the first block of the build's first launch (cigar_walk_kernel);
// [2..3] the 64-bit word of the first malformed record (all ones: none — so it is set when the block is allocated, and again by
// jl_ingest_verdict when it has read one; a build whose predecessor's word has not been read yet folds its own into it, atomicMin).
// Everything is enqueued on dst->stream; nothing waits.  dst->n_reads is not zero: the matrix has been allocated.
void jl_launch_ingest(jl_ctx *dst, const jl_records &R, uint32_t min_qv)
{
    hipStream_t st = dst->stream;
    const jl_ingest_scratch &S = dst->ing;
    const uint32_t ns = jl_ingest_sweeps(dst->n_cols);
    const jl_qv_mode mode = jl_qv_mode_of(R.have_qual, R.masked, min_qv);
    unsigned long long *bad = reinterpret_cast<unsigned long long *>(S.d_count + 2);
    // (the cigar kernels check a read's quality COUNT: the offsets whenever the stream has qualities, whatever min_qv is)
    const uint64_t *qo = R.have_qual ? R.qo : nullptr;
    hipLaunchKernelGGL(cigar_walk_kernel, dim3((uint32_t)((dst->n_reads + kWalkReads - 1u) / kWalkReads)), dim3(256), 0, st,
                       dst->n_reads, R.pos, R.cig, R.co, R.so, qo, dst->win_begin, dst->n_cols, ns, S.runs, S.nruns, S.desc, bad, S.d_count, R.maybe_long ? 1u : 0u);
    // (the launch for the long reads: not when the upload has looked and found none — every CCS sample: 6 us of a build)
    if (R.maybe_long)
        hipLaunchKernelGGL(cigar_runs_kernel, dim3((uint32_t)std::min<uint64_t>(kRunsLongGrid, (dst->n_reads + 255u) / 256u)), dim3(256), 0, st,
                           dst->n_reads, R.pos, R.cig, R.co, R.so, qo, dst->win_begin, dst->n_cols, ns, S.runs, S.nruns, S.desc, bad);
    ingest_args a;
    a.n_reads = dst->n_reads;
    a.n_cols = dst->n_cols;
    a.n_sweeps = ns;
    const uint64_t reads_pad = dst->plane_stride * 8u;                 // a multiple of 1024: whole line groups of tiles
    a.n_groups = (uint32_t)(reads_pad / 1024u);
    a.min_qv = std::min<uint32_t>(min_qv, 127u);   // (the byte-parallel compare of the QV path; BAM qualities end at 93)
    a.cig_off = R.co;
    a.seq4 = R.seq;
    a.seq_off = R.so;
    // (null unless the mode is theirs: slow_pair tests these pointers)
    a.qual = mode == JL_QV_BYTES ? R.qual : nullptr;
    a.qual_off = mode == JL_QV_BYTES ? R.qo : nullptr;
    a.qmask = mode == JL_QV_MASK ? R.mask : nullptr;
    a.runs = S.runs;
    a.nruns = S.nruns;
    a.desc = S.desc;
    a.slow_count = S.d_count;
    a.big_list = S.slow.as<uint32_t>();
    a.msa = dst->d_msa;
    a.plane_stride = dst->plane_stride;
    const uint32_t grid = planes_units(dst);
    // sibling tiles a workgroup (round 6): with qualities two — 170 us against 179 with one, 213-219 with four (the registers leave two
    // workgroups a CU); without qualities one: 111-113 with one or two, 132 with four
    // (the mask mode: two — a whole build 140.7 us at the median, 137.5 at best, against 144.2 / 142.5 with one, the byte mode 193-195 in
    // the same runs: profiles/qmask_ingest_ab.txt; -DJL_NT_QM=1 through tools_tuning/build_tuning_lib.sh builds the other)
    constexpr uint32_t kNt = 1u, kNtQv = 2u, kNtQm = JL_NT_QM;
    switch (mode) {
    case JL_QV_BYTES: launch_planes<kQvBytes, kNtQv>(a, grid, st); break;
    case JL_QV_MASK: launch_planes<kQvMask, kNtQm>(a, grid, st); break;
    case JL_QV_NONE: launch_planes<kQvNone, kNt>(a, grid, st); break;
    }
}
