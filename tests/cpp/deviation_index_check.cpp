// deviation_index_check.cpp — csrc/deviation_index.h compiled for the host: the entry's encode / decode, the bounds of a chunk and
// of a whole index, and the counting kernel's field-overflow bound.  A stand-alone program (tests/test_deviation_index_host.py
// builds and runs it, with the host sanitizers); exit status 0 = every check holds, else the number of the first that failed.
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "../../minorseq_amd/csrc/deviation_index.h"

static int n_check = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        ++n_check;                                                         \
        if (!(cond)) { printf("check %d failed: %s\n", n_check, #cond); return n_check; } \
    } while (0)

int main(void)
{
    // ---- entries: every code triple at the read numbers' edges round-trips; the nine code bits are the low nine
    const uint32_t reads[] = {0u, 1u, 31u, 32u, 1023u, 1024u, 99999u, (1u << 23) - 2u, (1u << 23) - 1u};
    for (uint32_t r : reads)
        for (uint32_t a = 0; a < 7; ++a)
            for (uint32_t b = 0; b < 7; ++b)
                for (uint32_t c = 0; c < 7; ++c) {
                    const uint32_t e = jl_ix_encode(r, a, b, c);
                    CHECK(jl_ix_read(e) == r && jl_ix_code(e, 0) == a && jl_ix_code(e, 1) == b && jl_ix_code(e, 2) == c);
                    CHECK((e & 0x1FFu) == ((a << 6) | (b << 3) | c));
                    CHECK(((e & 0x124u) == 0u) == (a < 4 && b < 4 && c < 4));   // the kernel's "a valid codon" test
                }
    CHECK(JL_IX_MAX_READS == (1ull << 23) && ((JL_IX_MAX_READS - 1) << 9) <= 0xFFFFFFFFull);
    // ---- the chunk bound: 4 E <= 9 plane_stride / 2, at the strides of 1, 1024, 1025, 100000 and 2^23 reads
    const uint64_t strides[] = {128u, 256u, 12544u, 122880u, 1048576u};
    for (uint64_t s : strides) {
        const uint64_t m = jl_ix_chunk_max_entries(s);
        CHECK(4u * m * JL_IX_DENSITY_DEN <= 9u * s * JL_IX_DENSITY_NUM && 4u * (m + 1u) * JL_IX_DENSITY_DEN > 9u * s * JL_IX_DENSITY_NUM);
        CHECK(jl_ix_padded(m) >= m && jl_ix_padded(m) < m + 4u && jl_ix_padded(m) % 4u == 0u);
    }
    CHECK(jl_ix_chunk_max_entries(128u) == 144u && jl_ix_chunk_max_entries(12544u) == 14112u);
    CHECK(jl_ix_padded(0) == 0u && jl_ix_padded(1) == 4u && jl_ix_padded(4) == 4u && jl_ix_padded(5) == 8u);
    // ---- the whole index: half of the matrix's plane bytes; the allocation is the smaller bound (+ one round of slack) and fits
    // the benchmark's window in 56.5 MB
    CHECK(jl_ix_total_max_entries(12544u, 3000u) * 4u * 2u == 3ull * 3000u * 12544u);
    CHECK(jl_ix_alloc_entries(12544u, 3000u, 1000u) == 1000ull * 14112u + 4u);
    CHECK(jl_ix_alloc_entries(12544u, 3000u, 1000u) * 4u < 57000000ull);
    CHECK(jl_ix_alloc_entries(128u, 3u, 1u) == 144u + 4u);
    for (uint64_t s : strides)
        for (uint32_t cols : {3u, 7u, 33u, 3000u})
            CHECK(jl_ix_alloc_entries(s, cols, cols / 3u) <= jl_ix_padded(jl_ix_total_max_entries(s, cols)) + 4u);
    // ---- the accumulator fields: a batch adds at most FLUSH_ROUNDS x ROUND_ENTRIES to one field, a wave's sum of it fits 16 bits,
    // seven fields fit the 64-bit word
    CHECK(JL_IX_FLUSH_ROUNDS * JL_IX_ROUND_ENTRIES <= jl_ix_field_max());
    CHECK((JL_IX_FLUSH_ROUNDS + 1u) * JL_IX_ROUND_ENTRIES > jl_ix_field_max());
    CHECK(64u * JL_IX_FLUSH_ROUNDS * JL_IX_ROUND_ENTRIES < 65536u);
    CHECK(7u * JL_IX_FIELD_BITS <= 64u);
    CHECK(jl_ix_flush_entries() == 130048u);
    // the flush edge is reachable under the density bound only from 924 673 reads on (903 x 1024 + 1: what tests/test_gpu_deviation_index.py uses)
    CHECK(jl_ix_chunk_max_entries(122880u) > jl_ix_flush_entries() && jl_ix_chunk_max_entries(115584u) <= jl_ix_flush_entries());
    printf("ok %d checks\n", n_check);
    return 0;
}
