// bam_fuzz.cpp — seeded mutation fuzz of the BAM front end's two readers (collect_records and PipelinedBamReader), in one process,
// meant for AddressSanitizer + UBSan (tests/test_bam_fuzz_host.py builds it so; nothing of HIP is linked).
//
//   bam_fuzz <seed> <count> <tmp-dir> <seed.bam>...
//
// Every case mutates one seed file, writes it to <tmp-dir>, runs both readers on it (records_check.hpp: the invariants of the
// hand-over are checked on every chunk) and requires: both accept or both refuse; on accept, byte-identical hand-overs; for mutations
// of the inflated stream, equal refusal messages.  Level (i) mutates the inflated BAM stream and wraps it into BGZF again with correct
// CRCs, one class per field; level (ii) mutates the compressed bytes.  Prints "class accepted refused" per class; exit 0, or 1 with
// the failing case kept in <tmp-dir>/failed.bam.
#include <zlib.h>

#include <cstring>
#include <random>

#include "records_check.hpp"

namespace {
enum Class { BLOCK_SIZE, L_READ_NAME, N_CIGAR, L_SEQ, CIGAR_WORD, AUX_TYPE, B_COUNT, REF_ID, POS, FLAG, HDR_L_TEXT, HDR_N_REF, HDR_L_NAME,
             TRUNCATION, BYTE_FLIP, Z_HEADER, Z_BSIZE, Z_ISIZE, Z_CRC, Z_PAYLOAD, N_CLASSES };
const char *kNames[N_CLASSES] = {"block_size", "l_read_name", "n_cigar", "l_seq", "cigar_word", "aux_type", "b_count", "ref_id", "pos", "flag",
                                 "hdr_l_text", "hdr_n_ref", "hdr_l_name", "truncation", "byte_flip", "bgzf_header", "bgzf_bsize", "bgzf_isize",
                                 "bgzf_crc", "bgzf_payload"};
using Bytes = std::vector<uint8_t>;

struct Seed {
    Bytes raw;                       // the inflated stream
    size_t o_nref = 0, o_lname = 0;  // header fields (o_lname = 0: no reference)
    std::vector<size_t> rec;         // block_size words, and the stream's end
    struct Aux { size_t type_at, count_at; };   // count_at = 0: no array
    std::vector<std::vector<Aux>> aux;
};

uint32_t u32(const Bytes &b, size_t o) { uint32_t v; memcpy(&v, b.data() + o, 4); return v; }
void put32(Bytes &b, size_t o, uint32_t v) { memcpy(b.data() + o, &v, 4); }

Seed load(const char *path)
{
    Seed s;
    gzFile g = gzopen(path, "rb");
    if (!g) throw std::runtime_error(std::string("cannot open seed ") + path);
    uint8_t buf[1 << 16];
    for (int n; (n = gzread(g, buf, sizeof buf)) > 0;) s.raw.insert(s.raw.end(), buf, buf + n);
    gzclose(g);
    const Bytes &b = s.raw;
    s.o_nref = 8 + u32(b, 4);
    size_t o = s.o_nref + 4;
    const uint32_t n_ref = u32(b, s.o_nref);
    if (n_ref) s.o_lname = o;
    for (uint32_t i = 0; i < n_ref; ++i) o += 8 + u32(b, o);
    while (o < b.size()) {
        s.rec.push_back(o);
        const size_t p = o + 4, end = p + u32(b, o);
        uint16_t n_cigar;
        memcpy(&n_cigar, b.data() + p + 12, 2);
        const uint32_t l_seq = u32(b, p + 16);
        size_t a = p + 32 + b[p + 8] + 4 * (size_t)n_cigar + (l_seq + 1) / 2 + l_seq;
        std::vector<Seed::Aux> tags;
        while (a + 3 <= end) {
            Seed::Aux t{a + 2, 0};
            const char ty = (char)b[a + 2];
            a += 3;
            if (ty == 'A' || ty == 'c' || ty == 'C') a += 1;
            else if (ty == 's' || ty == 'S') a += 2;
            else if (ty == 'i' || ty == 'I' || ty == 'f') a += 4;
            else if (ty == 'Z' || ty == 'H') a += strlen((const char *)b.data() + a) + 1;
            else if (ty == 'B') {
                const char sub = (char)b[a];
                t.count_at = a + 1;
                a += 5 + (size_t)u32(b, a + 1) * ((sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4);
            } else throw std::runtime_error("seed with an unknown aux type");
            tags.push_back(t);
        }
        s.aux.push_back(tags);
        o = end;
    }
    s.rec.push_back(b.size());
    if (s.rec.size() < 3) throw std::runtime_error("seed with fewer than two records");
    return s;
}

// one BGZF member of `in` (at most 64 KiB)
void member(const uint8_t *in, size_t n, int level, Bytes &out)
{
    Bytes body(compressBound((uLong)n) + 64);
    z_stream z;
    memset(&z, 0, sizeof z);
    if (deflateInit2(&z, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) throw std::runtime_error("deflateInit2");
    z.next_in = const_cast<uint8_t *>(in);
    z.avail_in = (uInt)n;
    z.next_out = body.data();
    z.avail_out = (uInt)body.size();
    if (deflate(&z, Z_FINISH) != Z_STREAM_END) throw std::runtime_error("deflate");
    const size_t clen = z.total_out;
    deflateEnd(&z);
    const uint16_t bsize = (uint16_t)(clen + 25);
    const uint8_t hdr[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)(bsize & 0xff), (uint8_t)(bsize >> 8)};
    out.insert(out.end(), hdr, hdr + 18);
    out.insert(out.end(), body.begin(), body.begin() + (long)clen);
    const uint32_t tail[2] = {(uint32_t)crc32(0L, in, (uInt)n), (uint32_t)n};
    out.insert(out.end(), (const uint8_t *)tail, (const uint8_t *)tail + 8);
}
// `raw` as BGZF in blocks of `block` bytes; the offset of every member to `at` when given
Bytes wrap(const Bytes &raw, size_t block, int level, std::vector<size_t> *at = nullptr)
{
    Bytes out;
    for (size_t o = 0; o < raw.size(); o += block) {
        if (at) at->push_back(out.size());
        member(raw.data() + o, std::min(block, raw.size() - o), level, out);
    }
    if (at) at->push_back(out.size());
    member(nullptr, 0, 6, out);   // the EOF block
    return out;
}

struct Outcome {
    bool ok = false;
    std::string what;
    rcheck::Handed h;
};
Outcome run_reader(const std::string &path, const rcheck::Run &run)
{
    Outcome o;
    try {
        o.h = rcheck::read_all(path, run);
        o.ok = true;
    } catch (const rcheck::Violation &) {
        throw;
    } catch (const std::exception &ex) {
        o.what = ex.what();
    }
    return o;
}
}  // namespace

int main(int argc, char **argv)
{
    if (argc < 5) { fprintf(stderr, "usage: bam_fuzz seed count tmp-dir seed.bam...\n"); return 2; }
    const uint64_t seed = strtoull(argv[1], nullptr, 10);
    const long count = atol(argv[2]);
    const std::string dir = argv[3], path = dir + "/case.bam";
    std::vector<Seed> seeds;
    for (int i = 4; i < argc; ++i) seeds.push_back(load(argv[i]));
    std::mt19937_64 g(seed);
    auto below = [&](uint64_t n) { return (size_t)(g() % n); };
    long accepted[N_CLASSES] = {0}, refused[N_CLASSES] = {0};
    static const uint32_t kEdge[] = {0, 1, 2, 31, 32, 33, 255, 256, 65535, 65536, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu, 0xFFFFFFF0u};

    for (long c = 0; c < count; ++c) {
        const Seed &s = seeds[below(seeds.size())];
        const int cls = (int)(c % N_CLASSES);   // every class in turn: the counts do not depend on luck
        Bytes raw = s.raw, file;
        const size_t n_rec = s.rec.size() - 1;
        size_t r = below(n_rec);
        if ((cls == REF_ID || cls == POS || cls == FLAG) && below(2)) {
            // half of the time a record that the field now drops (it may hold what a kept record must not: the refusals of these classes)
            std::vector<size_t> dropped;
            for (size_t k = 0; k < n_rec; ++k) {
                const size_t q = s.rec[k] + 4;
                const bool d = cls == REF_ID ? (int32_t)u32(raw, q) < 0 : cls == POS ? (int32_t)u32(raw, q + 4) < 0 : (raw[q + 14] & 0x4) || (raw[q + 15] & 0x1);
                if (d) dropped.push_back(k);
            }
            if (!dropped.empty()) r = dropped[below(dropped.size())];
        }
        const size_t at = s.rec[r], p = at + 4;
        // a value for a length field: an edge, or the old value nudged
        auto nudged = [&](uint32_t old) { return below(2) ? kEdge[below(sizeof kEdge / sizeof *kEdge)] : old + (uint32_t)below(9) - 4u; };
        switch (cls) {
        case BLOCK_SIZE: put32(raw, at, nudged(u32(raw, at))); break;
        case L_READ_NAME: raw[p + 8] = (uint8_t)(below(2) ? below(256) : raw[p + 8] + below(5) - 2); break;
        case N_CIGAR: { const uint16_t v = (uint16_t)nudged(raw[p + 12] | raw[p + 13] << 8); memcpy(raw.data() + p + 12, &v, 2); break; }
        case L_SEQ: put32(raw, p + 16, nudged(u32(raw, p + 16))); break;
        case CIGAR_WORD: {
            uint16_t n_cigar;
            memcpy(&n_cigar, raw.data() + p + 12, 2);
            if (!n_cigar) break;
            const size_t w = p + 32 + raw[p + 8] + 4 * below(n_cigar);
            const uint32_t old = u32(raw, w), kind = (uint32_t)below(4);
            static const uint32_t same_side[16] = {0, 4, 3, 2, 1, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 15};   // I<->S, D<->N, H<->P, =<->X: the query length stays
            if (kind == 0) put32(raw, w, (old & ~15u) | same_side[old & 15]);
            else if (kind == 1) put32(raw, w, (old & ~15u) | (uint32_t)below(16));
            else if (kind == 2) put32(raw, w, (nudged(old >> 4) << 4) | (old & 15));
            else put32(raw, w, (uint32_t)g());
            break;
        }
        case AUX_TYPE:
        case B_COUNT: {
            std::vector<size_t> where;
            for (size_t k = 0; k < n_rec; ++k)
                for (const Seed::Aux &t : s.aux[k])
                    if (cls == AUX_TYPE || t.count_at) where.push_back(cls == AUX_TYPE ? t.type_at : t.count_at);
            if (where.empty()) break;
            const size_t w = where[below(where.size())];
            if (cls == B_COUNT) { put32(raw, w, nudged(u32(raw, w))); break; }
            static const char swap_a[] = "AcCsSiIfZHB", swap_b[] = "cCAsSIifHZB";   // a type of the same size, or any byte
            const char *f = strchr(swap_a, (char)raw[w]);
            raw[w] = (below(2) && f) ? (uint8_t)swap_b[f - swap_a] : (uint8_t)below(256);
            break;
        }
        case REF_ID: put32(raw, p, below(2) ? (uint32_t)below(4) - 1u : (uint32_t)g()); break;
        case POS: put32(raw, p + 4, below(2) ? (uint32_t)below(600) - 1u : (uint32_t)g()); break;
        case FLAG: { const uint16_t v = below(2) ? (uint16_t)(1u << below(12)) : (uint16_t)g(); memcpy(raw.data() + p + 14, &v, 2); break; }
        case HDR_L_TEXT: put32(raw, 4, nudged(u32(raw, 4))); break;
        case HDR_N_REF: put32(raw, s.o_nref, nudged(u32(raw, s.o_nref))); break;
        case HDR_L_NAME: if (s.o_lname) put32(raw, s.o_lname, nudged(u32(raw, s.o_lname))); break;
        case TRUNCATION: raw.resize(below(2) ? s.rec[1 + below(n_rec)] : below(raw.size())); break;   // at a record boundary, or anywhere
        case BYTE_FLIP: {   // two of three inside a record's variable part (a record may have none: then anywhere), else anywhere
            const size_t var = s.rec[r + 1] - at > 36 ? s.rec[r + 1] - at - 36 : 0;
            raw[(below(3) && var) ? at + 36 + below(var) : below(raw.size())] ^= (uint8_t)(1u << below(8));
            break;
        }
        default: break;
        }
        static const size_t kBlocks[] = {61, 1000, 4096, 0xff00};
        if (cls < Z_HEADER) file = wrap(raw, kBlocks[below(4)], (int)below(3));
        else {
            std::vector<size_t> m;
            file = wrap(raw, 4096, 1, &m);
            const size_t k = below(m.size() - 1), b0 = m[k], b1 = m[k + 1];
            if (cls == Z_HEADER) file[b0 + below(16)] ^= (uint8_t)(1u << below(8));
            else if (cls == Z_BSIZE) file[b0 + 16 + below(2)] ^= (uint8_t)(1u << below(8));
            else if (cls == Z_ISIZE) file[b1 - 4 + below(4)] ^= (uint8_t)(1u << below(8));
            else if (cls == Z_CRC) file[b1 - 8 + below(4)] ^= (uint8_t)(1u << below(8));
            else file[b0 + 18 + below(b1 - b0 - 26)] ^= (uint8_t)(1u << below(8));
        }
        FILE *f = fopen(path.c_str(), "wb");
        if (!f || fwrite(file.data(), 1, file.size(), f) != file.size() || fclose(f) != 0) { fprintf(stderr, "bam_fuzz: cannot write %s\n", path.c_str()); return 2; }

        rcheck::Run a, b;
        a.form = b.form = (rcheck::Form)below(3);
        a.min_qv = b.min_qv = 20;
        a.min_rq = b.min_rq = below(2) ? 0.95 : 0.0;
        a.ref_id = b.ref_id = below(4) ? -1 : (int)below(3);
        a.chunk_reads = 1 + below(50);
        b.pipelined = true;
        b.threads = 1 + (unsigned)below(4);
        std::string fail;
        try {
            const Outcome sa = run_reader(path, a), sb = run_reader(path, b);
            if (sa.ok != sb.ok) fail = "one reader accepts, the other refuses: seq '" + sa.what + "', pipe '" + sb.what + "'";
            else if (sa.ok && !sa.h.same_records(sb.h)) fail = "the readers hand over different records";
            else if (!sa.ok && cls < Z_HEADER && sa.what != sb.what) fail = "refusal messages differ: seq '" + sa.what + "', pipe '" + sb.what + "'";
            ++(sa.ok ? accepted : refused)[cls];
        } catch (const rcheck::Violation &v) {
            fail = std::string("invariant: ") + v.what();
        }
        if (!fail.empty()) {
            rename(path.c_str(), (dir + "/failed.bam").c_str());
            for (int k = 0; k < N_CLASSES; ++k) printf("%s %ld %ld\n", kNames[k], accepted[k], refused[k]);   // the counts so far
            printf("FAILED case %ld class %s (seed %llu): %s\n", c, kNames[cls], (unsigned long long)seed, fail.c_str());
            return 1;
        }
    }
    for (int k = 0; k < N_CLASSES; ++k) printf("%s %ld %ld\n", kNames[k], accepted[k], refused[k]);
    remove(path.c_str());
    return 0;
}
