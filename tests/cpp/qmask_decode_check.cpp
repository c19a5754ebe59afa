// qmask_decode_check <in.bam> <min_qv>: the front end's record decoder in its two quality forms — the folded effective quality
// bytes, and the filter as one bit per base (IngestOptions::qv_mask, the layout of jl_records_append_masked) — through the
// sequential and the pipelined reader.  Every chunk's mask must be the threshold of that chunk's effective qualities: bit
// 2 * (seq_off[r] - seq_off[0]) + q for base q of read r, every other bit clear, (bases' bytes + 3) / 4 bytes.
#include <cstdio>
#include <cstdlib>

#include "juliet_hip.h"
#include "decode.hpp"

using namespace jlhost;

struct Flags {                       // per read, in file order: the filter of its bases
    std::vector<std::vector<uint8_t>> of_read;
    uint64_t set = 0, chunks = 0;
};

static int decode(const char *bam, uint32_t min_qv, bool mask, bool pipelined, Flags &out)
{
    IngestOptions io;
    io.min_qv = min_qv;
    io.qv_mask = mask;
    const uint8_t t = (uint8_t)std::min<uint32_t>(min_qv, 127u);
    int bad = 0;
    RecordSink sink;
    sink.chunk_reads = 97;
    sink.give = [&](RecordArrays &c) {
        const size_t n = c.pos.size();
        ++out.chunks;
        if (mask) {
            const uint64_t s0 = c.seq_off[0];
            if (c.qmask.size() != (c.seq_off[n] - s0 + 3) / 4) { fprintf(stderr, "mask of %zu bytes for %llu bytes of bases\n", c.qmask.size(), (unsigned long long)(c.seq_off[n] - s0)); ++bad; }
            uint64_t in_reads = 0, in_mask = 0;
            for (uint8_t b : c.qmask) in_mask += (uint64_t)__builtin_popcount(b);
            for (size_t r = 0; r < n; ++r) {
                // (the decoder checks that the cigar consumes l_seq bases; the bases' bytes say l_seq up to the spare nibble: from the cigar)
                uint64_t l_seq = 0;
                for (uint64_t k = c.cig_off[r]; k < c.cig_off[r + 1]; ++k) {
                    const uint32_t op = c.cigar[k] & 15u;
                    if (op == CIG_I || op == CIG_S || op == CIG_EQ || op == CIG_X) l_seq += c.cigar[k] >> 4;
                }
                std::vector<uint8_t> f(l_seq);
                for (uint64_t q = 0; q < l_seq; ++q) {
                    const uint64_t i = 2 * (c.seq_off[r] - s0) + q;
                    f[q] = (c.qmask[i >> 3] >> (i & 7u)) & 1u;
                    in_reads += f[q];
                }
                out.of_read.push_back(std::move(f));
            }
            if (in_reads != in_mask) { fprintf(stderr, "%llu bits set outside the reads' bases\n", (unsigned long long)(in_mask - in_reads)); ++bad; }
            out.set += in_reads;
        } else {
            for (size_t r = 0; r < n; ++r) {
                std::vector<uint8_t> f(c.qual_off[r + 1] - c.qual_off[r]);
                for (size_t q = 0; q < f.size(); ++q) {
                    const uint8_t v = c.qual[c.qual_off[r] + q];
                    f[q] = v < t && v != 0xFF;
                    out.set += f[q];
                }
                out.of_read.push_back(std::move(f));
            }
        }
        c.clear();
    };
    RecordArrays rec;
    std::vector<BamRef> refs;
    std::string text;
    if (pipelined) PipelinedBamReader::run(bam, io, -1, min_qv > 0, sink, &refs, &text, 5);
    else collect_records(bam, io, -1, min_qv > 0, rec, &refs, &text, &sink);
    return bad;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const uint32_t min_qv = (uint32_t)atoi(argv[2]);
    int bad = 0;
    Flags ref;
    bad += decode(argv[1], min_qv, false, false, ref);
    for (int pipelined = 0; pipelined < 2; ++pipelined) {
        Flags got;
        bad += decode(argv[1], min_qv, true, pipelined != 0, got);
        if (got.of_read.size() != ref.of_read.size()) { fprintf(stderr, "reads: %zu against %zu\n", got.of_read.size(), ref.of_read.size()); return 1; }
        size_t differ = 0;
        for (size_t r = 0; r < ref.of_read.size(); ++r) differ += got.of_read[r] != ref.of_read[r];
        if (differ) { fprintf(stderr, "%s reader: %zu reads differ\n", pipelined ? "pipelined" : "sequential", differ); ++bad; }
        printf("%s: %zu reads, %llu chunks, %llu of the bases filtered\n", pipelined ? "pipelined" : "sequential", got.of_read.size(),
               (unsigned long long)got.chunks, (unsigned long long)got.set);
    }
    {   // the byte form through the pipelined reader gives the same flags as through the sequential one
        Flags pb;
        bad += decode(argv[1], min_qv, false, true, pb);
        if (pb.of_read != ref.of_read) { fprintf(stderr, "byte form: the readers differ\n"); ++bad; }
    }
    if (!ref.set) { fprintf(stderr, "no base below the threshold: nothing tested\n"); ++bad; }
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
