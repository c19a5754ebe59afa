// cigar_rules.h — what a cigar op means to the record ingest (kernels_ingest.hip), once, for the device kernels that walk cigars
// (cigar_walk_kernel, cigar_runs_kernel) and for the host's look at them at the upload (jl_ingest_read_is_long).  Pure functions,
// host and device; tests/test_cigar_rules_host.py compiles them for the CPU.  Private to libjuliet_hip.so.
// Behaviour: doc/JULIET.md:26-27 (insertions dropped, deletions '-'), :53 (PacBio cigars = X I D S H N P; M is refused).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define JL_CG_FN __host__ __device__ __forceinline__
#else
#define JL_CG_FN static inline
#endif

namespace jl_cigar {

// ---- an op (code in the low four bits of a cigar word, length above): three constants indexed by the code.  D N = X consume the
// reference, I S = X the query; an op's KIND is what its columns show: 1 aligned bases (= X), 2 a deletion (D), 3 nothing (N: a
// reference skip), 0 no columns at all (I S H P, and M, which is refused).  An op of length zero has no kind, whatever its code.
constexpr uint32_t kRefOps = (1u << 2) | (1u << 3) | (1u << 7) | (1u << 8);
constexpr uint32_t kQueryOps = (1u << 1) | (1u << 4) | (1u << 7) | (1u << 8);
constexpr uint32_t kKinds = (2u << 4) | (3u << 6) | (1u << 14) | (1u << 16);   // two bits per op
constexpr uint32_t kAligned = 1u, kDeletion = 2u, kNothing = 3u;

JL_CG_FN bool consumes_ref(uint32_t op) { return (kRefOps >> op) & 1u; }
JL_CG_FN bool consumes_query(uint32_t op) { return (kQueryOps >> op) & 1u; }
JL_CG_FN uint32_t kind_of(uint32_t op, uint32_t len) { return len == 0u ? 0u : (kKinds >> (2u * op)) & 3u; }

// An op begins an entry (a run) unless it has no kind, or it and the op before are both aligned bases: stretches of '=' / 'X'
// merge, D and N are runs of their own, and anything without a kind only ends a run.  (cigar_runs_kernel evaluates this for
// eight ops at once on kinds packed two bits an op: `starts` there.)
JL_CG_FN bool begins_entry(uint32_t kind, uint32_t prev_kind) { return kind != 0u && !(kind == kAligned && prev_kind == kAligned); }

// ---- window columns.  base = the read's position - the window's first column; ref = reference bases consumed so far (below 2^60:
// 28-bit lengths, fewer than 2^32 ops).  The column clamped to [0, n_cols], and how far in front of the window it lies (saturated):
// a run that begins before the window begins at column 0 with its query offset moved along by `before`.
struct col_t {
    uint32_t col, before;
};
JL_CG_FN col_t window_col(int64_t base, uint64_t ref, uint32_t n_cols)
{
    const int64_t w = base + (int64_t)ref;
    col_t c;
    c.before = w >= 0 ? 0u : (-w > (int64_t)0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)(-w));
    c.col = w < 0 ? 0u : (w > (int64_t)n_cols ? n_cols : (uint32_t)w);
    return c;
}

// ---- entries: {window column | kind << 30, query offset}, 8 bytes (the list of a read: kernels_ingest.hip)
constexpr uint32_t kRunMask = 0x3FFFFFFFu;          // window column of an entry; kind in the two bits above
struct entry_t {
    uint32_t x, y;
};
JL_CG_FN uint32_t entry_col(uint32_t x) { return x & kRunMask; }
JL_CG_FN uint32_t entry_kind(uint32_t x) { return x >> 30; }
JL_CG_FN entry_t entry_run(uint32_t col, uint32_t kind, uint32_t q) { return entry_t{col | (kind << 30), q}; }
// the three entries around a read's runs: 'not covered from column 0', the read's end (with the query length), and 'never'
JL_CG_FN entry_t entry_before() { return entry_t{kNothing << 30, 0u}; }
JL_CG_FN entry_t entry_end(uint32_t end_col, uint32_t q_total) { return entry_t{end_col | (kNothing << 30), q_total}; }
JL_CG_FN entry_t entry_never() { return entry_t{kRunMask | (kNothing << 30), 0u}; }

// ---- the verdict on an untrusted record: 0 fine; 1 an 'M'; 2 its cigar consumes more bases than the record holds (packed two a
// byte), or 2^31 and more; 3 more qualities than it holds (qual_len all ones: the stream has none); 4 it spans 2^30 reference bases
// or more.  The first that applies, in this order.  (5, 'a long read nobody expected', is cigar_walk_kernel's own.)
JL_CG_FN uint32_t verdict(bool has_m, uint64_t q_total, uint64_t packed_bytes, uint64_t qual_len, uint64_t ref_total)
{
    if (has_m) return 1u;
    if (q_total > 2u * packed_bytes || q_total > 0x7FFFFFFFull) return 2u;
    if (q_total > qual_len) return 3u;
    if (ref_total > (uint64_t)kRunMask) return 4u;
    return 0u;
}

// ---- which reads cigar_walk_kernel leaves to the long-read launch: more than kWalkOps ops, or more entries (runs + the three
// around them) than a read has room for in its LDS.
constexpr uint32_t kWalkOps = 192u;
// entries of a read in LDS: a CCS read has a dozen.  With 24 two reads in a thousand went to the other launch; with 32 two in 100 000
// (fifteen deletions) — enough for the upload to have to ask for that launch in every build; with 40 none of a CCS sample does
// (48: 26 KB of LDS a workgroup, six a CU — not all 1563 of a 100k-read build at once: 28 us instead of 22)
constexpr uint32_t kWalkEnt = 40u;
JL_CG_FN bool read_is_long(const uint32_t *cigar, uint64_t n_ops)
{
    if (n_ops > kWalkOps) return true;
    uint32_t n_runs = 0, prev_kind = 0;
    for (uint64_t t = 0; t < n_ops; ++t) {
        const uint32_t kind = kind_of(cigar[t] & 15u, cigar[t] >> 4);
        if (begins_entry(kind, prev_kind)) ++n_runs;
        prev_kind = kind;
    }
    return n_runs + 3u > kWalkEnt;
}

}  // namespace jl_cigar
