// narrow_entry_check.cpp — the stored form of a deviation-index entry (csrc/deviation_index.h) compiled for the host: 16 bits that
// carry the three codes and nothing of the read number, two to a dword as the counting kernel decodes them, the allocation in
// bytes, and the flush bounds at every walk depth the kernels use.  A stand-alone program (tests/test_narrow_entry_host.py builds
// and runs it, with the host sanitizers); exit status 0 = every check holds, else the number of the first that failed.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../minorseq_amd/csrc/deviation_index.h"

static int n_check = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        ++n_check;                                                         \
        if (!(cond)) { printf("check %d failed: %s\n", n_check, #cond); return n_check; } \
    } while (0)

// the walk of index_stream (kernels_pileup.hip) over one chunk's list inside a buffer of stored entries, on the host: rounds of 256
// lanes x 4 entries, a lane's round one 8-byte load decoded two entries to a dword, the tail test first + i >= E.  Returns the
// number of entries counted; per column the count of every code, and the valid codons.
// A COPY of the kernel's decode and tail test, not the kernel: it pins the format and the layout of lists lying against each other
// (the kernel itself is compared with the plane run and the oracle in tests/test_gpu_narrow_index.py).  Whoever changes the decode,
// the round or the tail test in index_stream changes this function with it.
struct walk_counts {
    uint64_t n, col[3][8], valid;
};
static walk_counts walk(const jl_ix_stored_t *buf, uint64_t first_entry, uint32_t E)
{
    walk_counts w;
    memset(&w, 0, sizeof w);
    const uint32_t n_rounds = (E + JL_IX_ROUND_ENTRIES * JL_IX_BLOCK_LANES - 1u) / (JL_IX_ROUND_ENTRIES * JL_IX_BLOCK_LANES);
    for (uint32_t r = 0; r < n_rounds; ++r)
        for (uint32_t tid = 0; tid < JL_IX_BLOCK_LANES; ++tid) {
            const uint32_t first = (r * JL_IX_BLOCK_LANES + tid) * JL_IX_ROUND_ENTRIES;
            if (first >= E) continue;   // the load is not made
            uint32_t d[2];
            memcpy(d, buf + first_entry + first, 8);   // (little endian, as the device)
            const uint32_t e4[4] = {d[0] & 0xFFFFu, d[0] >> 16, d[1] & 0xFFFFu, d[1] >> 16};
            for (uint32_t i = 0; i < 4; ++i) {
                if (first + i >= E) continue;
                const uint32_t e = e4[i];
                w.n++;
                w.col[0][(e >> 6) & 7u]++;
                w.col[1][(e >> 3) & 7u]++;
                w.col[2][e & 7u]++;
                if ((e & 0x124u) == 0u) w.valid++;
            }
        }
    return w;
}

int main(void)
{
    CHECK(sizeof(jl_ix_stored_t) == 2u && JL_IX_ENTRY_BYTES == 2u && JL_IX_ROUND_ENTRIES * JL_IX_ENTRY_BYTES == 8u);
    // ---- the stored entry: the nine code bits whatever the read number, the valid-codon test on it, the codes out of it
    const uint32_t reads[] = {0u, 1u, 31u, 32u, 127u, 128u, 1023u, 1024u, 99999u, (1u << 23) - 2u, (1u << 23) - 1u};
    for (uint32_t a = 0; a < 7; ++a)
        for (uint32_t b = 0; b < 7; ++b)
            for (uint32_t c = 0; c < 7; ++c) {
                const uint32_t codes = (a << 6) | (b << 3) | c;
                for (uint32_t r : reads) {
                    const jl_ix_stored_t s = jl_ix_stored(jl_ix_encode(r, a, b, c));
                    CHECK(s == codes && (s >> 9) == 0u);
                    CHECK(s == jl_ix_stored(jl_ix_encode(0u, a, b, c)));
                    CHECK(((s & 0x124u) == 0u) == (a < 4 && b < 4 && c < 4));
                    CHECK(jl_ix_code(s, 0) == a && jl_ix_code(s, 1) == b && jl_ix_code(s, 2) == c);
                }
                // two stored entries to a dword, this one in either half beside every other triple: both decode to themselves
                const uint32_t s = jl_ix_stored(jl_ix_encode((1u << 23) - 1u, a, b, c));
                for (uint32_t o = 0; o < 512u; ++o) {
                    if ((o & 7u) == 7u || ((o >> 3) & 7u) == 7u || (o >> 6) == 7u) continue;   // (codes are 0..6)
                    const uint32_t t = jl_ix_stored(jl_ix_encode((o * 16411u) & ((1u << 23) - 1u), o >> 6, (o >> 3) & 7u, o & 7u));
                    const uint32_t lo_hi = s | (t << 16), hi_lo = t | (s << 16);
                    CHECK((lo_hi & 0xFFFFu) == s && (lo_hi >> 16) == t && (hi_lo & 0xFFFFu) == t && (hi_lo >> 16) == s);
                    CHECK((((lo_hi >> 16) >> 6) & 7u) == (o >> 6) && (((hi_lo >> 16) >> 6) & 7u) == a);   // no mask on the high half
                }
            }
    // ---- the allocation: entries x 2 bytes; the benchmark's window (100 000 reads x 3000 columns) under 28.3 MB
    const uint64_t strides[] = {128u, 256u, 12544u, 14592u, 122880u, 1048576u};
    for (uint64_t st : strides)
        for (uint32_t cols : {3u, 7u, 33u, 36u, 3000u})
            CHECK(jl_ix_alloc_entries(st, cols, cols / 3u) * JL_IX_ENTRY_BYTES == jl_ix_alloc_entries(st, cols, cols / 3u) * 2u);
    CHECK(jl_ix_alloc_entries(12544u, 3000u, 1000u) * JL_IX_ENTRY_BYTES == (1000ull * 14112u + 4u) * 2u);
    CHECK(jl_ix_alloc_entries(12544u, 3000u, 1000u) * JL_IX_ENTRY_BYTES < 28300000ull);
    // a list of the chunk bound, stored, is at most a quarter of the chunk's nine plane rows
    for (uint64_t st : strides) CHECK(jl_ix_chunk_max_entries(st) * JL_IX_ENTRY_BYTES * 4u <= 9u * st);
    // ---- the walk's depths: between two flushes whole batches, never above JL_IX_FLUSH_ROUNDS; a field <= 511, a wave's sum < 2^16
    const uint32_t depths[] = {JL_IX_DEPTH, JL_IX_FOLD_DEPTH, 1u, 2u, 4u, 8u, 16u};   // what the kernels use, and what the sweep built
    for (uint32_t d : depths) {
        const uint32_t rounds = jl_ix_flush_rounds_at(d);
        CHECK(d >= 1u && d <= JL_IX_MAX_DEPTH);
        CHECK(rounds >= d && rounds % d == 0u && rounds <= JL_IX_FLUSH_ROUNDS && rounds + d > JL_IX_FLUSH_ROUNDS);
        CHECK(rounds * JL_IX_ROUND_ENTRIES <= jl_ix_field_max());
        CHECK(64u * rounds * JL_IX_ROUND_ENTRIES < 65536u);
    }
    CHECK(jl_ix_flush_rounds_at(1u) == 127u && jl_ix_flush_rounds_at(2u) == 126u && jl_ix_flush_rounds_at(16u) == 112u);
    CHECK(jl_ix_flush_rounds_at(2u) * 4u == 504u && jl_ix_flush_rounds_at(16u) * 4u == 448u);
    CHECK(JL_IX_DEPTH == 2u && JL_IX_FOLD_DEPTH == 16u);   // the figures DESIGN.md and the GPU test's batch edges are written for
    // ---- the walk on the host over lists that lie against each other: a list that ends inside a dword or inside an 8-byte load is
    // followed by padding slots (never written: any bits) and by the neighbour's first entry; neither is ever counted
    const uint32_t lens[] = {0u, 1u, 2u, 3u, 4u, 5u, 7u, 8u, 9u, 1023u, 1024u, 1025u, 2047u, 2048u, 2049u, 16383u, 16384u, 16385u};
    std::vector<uint64_t> at;
    uint64_t room = 0;
    for (uint32_t E : lens) { at.push_back(room); room += jl_ix_padded(E); }
    std::vector<jl_ix_stored_t> buf(room + 4u, (jl_ix_stored_t)0xFFFFu);   // padding and slack: all ones, every code 7, "a valid codon" never
    uint32_t x = 12345u;
    std::vector<walk_counts> want(sizeof lens / sizeof lens[0]);
    for (size_t k = 0; k < at.size(); ++k) {
        memset(&want[k], 0, sizeof want[k]);
        for (uint32_t i = 0; i < lens[k]; ++i) {
            x = x * 1664525u + 1013904223u;
            const uint32_t a = (x >> 8) % 7u, b = (x >> 16) % 7u, c = (x >> 24) % 7u;
            buf[at[k] + i] = jl_ix_stored(jl_ix_encode(x >> 9, a, b, c));
            want[k].n++;
            want[k].col[0][a]++, want[k].col[1][b]++, want[k].col[2][c]++;
            if (a < 4 && b < 4 && c < 4) want[k].valid++;
        }
    }
    for (size_t k = 0; k < at.size(); ++k) {
        CHECK(at[k] % 4u == 0u);   // a list begins on 8 bytes
        const walk_counts got = walk(buf.data(), at[k], lens[k]);
        CHECK(got.n == lens[k] && got.valid == want[k].valid && memcmp(got.col, want[k].col, sizeof got.col) == 0);
        CHECK(got.col[0][7] == 0u && got.col[1][7] == 0u && got.col[2][7] == 0u);   // no padding slot was counted
    }
    printf("ok %d checks\n", n_check);
    return 0;
}
