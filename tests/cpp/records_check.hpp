// records_check.hpp — what tests/cpp/records_dump.cpp and tests/cpp/bam_fuzz.cpp share: run one of the front end's two BAM readers,
// check on every chunk it hands over what the device takes on trust, and keep everything it handed over, concatenated in file order.
// Host only: minorseq_amd/host/decode.hpp and minorseq_amd/csrc/cigar_rules.h, neither the device library nor the HIP runtime.
#pragma once
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "juliet_hip.h"
#include "decode.hpp"
#include "cigar_rules.h"

namespace rcheck {

struct Violation : std::runtime_error {   // an invariant of the hand-over does not hold: never the input's fault
    using std::runtime_error::runtime_error;
};

struct Handed {
    std::vector<int32_t> pos;
    std::vector<uint32_t> cigar;
    std::vector<uint64_t> cig_off{0}, seq_off{0}, qual_off{0};
    std::vector<uint8_t> seq4, qual;
    std::vector<uint8_t> qmask2;   // mask form: a byte per byte of seq4, bit 0 = its first base is filtered, bit 1 = its second
    std::string names;             // NUL-terminated, in order
    std::vector<uint64_t> chunk_reads;
    jlhost::ReadExtent extent;
    std::vector<jlhost::BamRef> refs;
    std::string text;
    bool same_records(const Handed &o) const
    {
        return pos == o.pos && cigar == o.cigar && cig_off == o.cig_off && seq_off == o.seq_off && qual_off == o.qual_off && seq4 == o.seq4 &&
               qual == o.qual && qmask2 == o.qmask2 && names == o.names && extent.n_reads == o.extent.n_reads &&
               extent.min_pos == o.extent.min_pos && extent.max_end == o.extent.max_end && extent.ref_id == o.extent.ref_id &&
               text == o.text && refs.size() == o.refs.size() &&
               std::equal(refs.begin(), refs.end(), o.refs.begin(),
                          [](const jlhost::BamRef &a, const jlhost::BamRef &b) { return a.name == b.name && a.length == b.length; });
    }
};

enum class Form { none, bytes, mask };

// The invariants of one chunk (offsets relative to the chunk), then its records appended to `h`.
inline void take_chunk(const jlhost::RecordArrays &c, Form form, Handed &h)
{
    const size_t n = c.pos.size();
    auto bad = [&](size_t r, const std::string &what) {
        throw Violation("read " + (r < c.names.size() ? c.names[r] : std::string("?")) + " (#" + std::to_string(h.pos.size() + r) + "): " + what);
    };
    if (c.cig_off.size() != n + 1 || c.seq_off.size() != n + 1 || c.names.size() != n) bad(0, "offset arrays do not match the read count");
    if (c.cig_off[0] != 0 || c.seq_off[0] != 0) bad(0, "offsets do not begin at 0");
    if (c.cig_off[n] != c.cigar.size() || c.seq_off[n] != c.seq4.size()) bad(n ? n - 1 : 0, "last offset is not the array size");
    const bool quals = form == Form::bytes;
    if (quals && (c.qual_off.size() != n + 1 || c.qual_off[0] != 0 || c.qual_off[n] != c.qual.size())) bad(0, "quality offsets do not match");
    if (form == Form::mask && c.qmask.size() != (c.seq4.size() + 3) / 4) bad(0, "mask size is not (seq4 + 3) / 4");
    if (form != Form::bytes && c.qual_off.size() != 1) bad(0, "quality offsets without qualities");
    for (size_t r = 0; r < n; ++r) {
        if (c.cig_off[r + 1] < c.cig_off[r] || c.seq_off[r + 1] < c.seq_off[r]) bad(r, "offsets decrease");
        if (c.cig_off[r + 1] > c.cigar.size() || c.seq_off[r + 1] > c.seq4.size()) bad(r, "offset beyond the array");
        if (c.pos[r] < 0) bad(r, "negative position");
        bool has_m = false;
        uint64_t q = 0, ref = 0;
        for (uint64_t k = c.cig_off[r]; k < c.cig_off[r + 1]; ++k) {
            const uint32_t op = c.cigar[k] & 15u, len = c.cigar[k] >> 4;
            has_m |= op == 0;
            if (jl_cigar::consumes_query(op)) q += len;
            if (jl_cigar::consumes_ref(op)) ref += len;
        }
        const uint64_t packed = c.seq_off[r + 1] - c.seq_off[r];
        if (packed != (q + 1) / 2) bad(r, "packed bases are not (l_seq + 1) / 2 bytes");
        uint64_t qual_len = ~(uint64_t)0;
        if (quals) {
            if (c.qual_off[r + 1] < c.qual_off[r] || c.qual_off[r + 1] > c.qual.size()) bad(r, "quality offsets decrease or overrun");
            qual_len = c.qual_off[r + 1] - c.qual_off[r];
            if (qual_len != q) bad(r, "qualities are not l_seq bytes");
        }
        const uint32_t v = jl_cigar::verdict(has_m, q, packed, qual_len, ref);
        if (v != 0) bad(r, "the device would refuse it: verdict " + std::to_string(v));
    }
    const uint64_t c0 = h.cigar.size(), s0 = h.seq4.size(), q0 = h.qual.size();
    h.pos.insert(h.pos.end(), c.pos.begin(), c.pos.end());
    h.cigar.insert(h.cigar.end(), c.cigar.begin(), c.cigar.end());
    h.seq4.insert(h.seq4.end(), c.seq4.begin(), c.seq4.end());
    for (size_t r = 0; r < n; ++r) {
        h.cig_off.push_back(c0 + c.cig_off[r + 1]);
        h.seq_off.push_back(s0 + c.seq_off[r + 1]);
        h.names.append(c.names[r]);
        h.names.push_back('\0');
    }
    if (quals) {
        h.qual.insert(h.qual.end(), c.qual.begin(), c.qual.end());
        for (size_t r = 0; r < n; ++r) h.qual_off.push_back(q0 + c.qual_off[r + 1]);
    }
    if (form == Form::mask)
        for (size_t b = 0; b < c.seq4.size(); ++b) h.qmask2.push_back((uint8_t)((c.qmask[b >> 2] >> (2 * (b & 3))) & 3u));
    h.chunk_reads.push_back(n);
}

struct Run {
    bool pipelined = false;   // PipelinedBamReader::run on a BGZF file (any other file takes the sequential reader, as in the product)
    unsigned threads = 1;
    size_t chunk_reads = 8192;
    uint32_t min_qv = 0;
    double min_rq = 0.0;
    Form form = Form::none;
    int ref_id = -1;
};

// Everything one reader hands over for `bam`; the extent's sums are checked against the records.
inline Handed read_all(const std::string &bam, const Run &run)
{
    using namespace jlhost;
    Handed h;
    IngestOptions io;
    io.ref_id = run.ref_id;
    io.min_qv = run.min_qv;
    io.min_rq = run.min_rq;
    io.qv_mask = run.form == Form::mask;
    const bool want_qual = run.form != Form::none;
    RecordSink sink;
    sink.chunk_reads = run.chunk_reads;
    sink.give = [&](RecordArrays &c) {
        take_chunk(c, run.form, h);
        c.clear();
    };
    RecordArrays rec;
    h.extent = (run.pipelined && PipelinedBamReader::is_bgzf(bam))
                   ? PipelinedBamReader::run(bam, io, run.ref_id, want_qual, sink, &h.refs, &h.text, run.threads)
                   : collect_records(bam, io, run.ref_id, want_qual, rec, &h.refs, &h.text, &sink);
    if (h.extent.n_reads != h.pos.size()) throw Violation("the extent counts " + std::to_string(h.extent.n_reads) + " reads, " +
                                                          std::to_string(h.pos.size()) + " were handed over");
    int64_t lo = std::numeric_limits<int64_t>::max(), hi = 0;
    for (size_t r = 0; r < h.pos.size(); ++r) {
        uint64_t ref = 0;
        for (uint64_t k = h.cig_off[r]; k < h.cig_off[r + 1]; ++k)
            if (jl_cigar::consumes_ref(h.cigar[k] & 15u)) ref += h.cigar[k] >> 4;
        lo = std::min<int64_t>(lo, h.pos[r]);
        hi = std::max<int64_t>(hi, (int64_t)h.pos[r] + (int64_t)ref);
    }
    if (lo != h.extent.min_pos || hi != h.extent.max_end) throw Violation("the extent is not the records' extent");
    return h;
}

}  // namespace rcheck
