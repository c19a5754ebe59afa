// records_dump.cpp — everything one of the front end's BAM readers hands over for a file, as flat little-endian arrays (a test
// reads them with numpy), after checking on every record what the device takes on trust (records_check.hpp).
//
//   records_dump <in.bam> <out.bin> [--reader seq|pipe] [--threads N] [--chunk-reads N] [--min-qv N] [--min-rq X]
//                [--form none|bytes|mask] [--ref N]
//
// out.bin: sections {char name[8]; uint64 bytes; data}: pos i32, cigar u32, cig_off / seq_off / qual_off u64, seq4, qual, qmask2 (a byte
// per byte of seq4, two bits), names (NUL-terminated), chunks u64 (reads per hand-over), extent {n_reads, min_pos, max_end, ref_id} i64,
// refs ({u32 length, name NUL} each), text.
// Exit 0; 2 with one message line on a std::exception (the input's fault); 4 when an invariant does not hold (names the read).
#include <cstring>

#include "records_check.hpp"

namespace {
void section(FILE *f, const char *name, const void *p, size_t bytes)
{
    char tag[8] = {0};
    strncpy(tag, name, 8);
    const uint64_t n = bytes;
    fwrite(tag, 1, 8, f);
    fwrite(&n, 8, 1, f);
    if (bytes) fwrite(p, 1, bytes, f);
}
template <typename V> void section(FILE *f, const char *name, const V &v) { section(f, name, v.data(), v.size() * sizeof(v[0])); }
}  // namespace

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: records_dump in.bam out.bin [options]\n"); return 1; }
    rcheck::Run run;
    for (int i = 3; i < argc; ++i) {
        const std::string a = argv[i];
        auto need = [&]() -> const char * { if (i + 1 >= argc) { fprintf(stderr, "records_dump: %s needs a value\n", a.c_str()); exit(1); } return argv[++i]; };
        if (a == "--reader") run.pipelined = std::string(need()) == "pipe";
        else if (a == "--threads") run.threads = (unsigned)atoi(need());
        else if (a == "--chunk-reads") run.chunk_reads = (size_t)atoll(need());
        else if (a == "--min-qv") run.min_qv = (uint32_t)atoi(need());
        else if (a == "--min-rq") run.min_rq = atof(need());
        else if (a == "--ref") run.ref_id = atoi(need());
        else if (a == "--form") {
            const std::string v = need();
            run.form = v == "mask" ? rcheck::Form::mask : v == "bytes" ? rcheck::Form::bytes : rcheck::Form::none;
        } else { fprintf(stderr, "records_dump: unknown option %s\n", a.c_str()); return 1; }
    }
    try {
        const rcheck::Handed h = rcheck::read_all(argv[1], run);
        FILE *f = fopen(argv[2], "wb");
        if (!f) { fprintf(stderr, "records_dump: cannot create %s\n", argv[2]); return 1; }
        section(f, "pos", h.pos);
        section(f, "cigar", h.cigar);
        section(f, "cig_off", h.cig_off);
        section(f, "seq4", h.seq4);
        section(f, "seq_off", h.seq_off);
        section(f, "qual", h.qual);
        section(f, "qual_off", h.qual_off);
        section(f, "qmask2", h.qmask2);
        section(f, "names", h.names);
        section(f, "chunks", h.chunk_reads);
        const int64_t ext[4] = {(int64_t)h.extent.n_reads, h.extent.min_pos, h.extent.max_end, h.extent.ref_id};
        section(f, "extent", ext, sizeof ext);
        std::string refs;
        for (const jlhost::BamRef &r : h.refs) {
            refs.append((const char *)&r.length, 4);
            refs.append(r.name);
            refs.push_back('\0');
        }
        section(f, "refs", refs);
        section(f, "text", h.text);
        if (fclose(f) != 0) { fprintf(stderr, "records_dump: short write\n"); return 1; }
    } catch (const rcheck::Violation &v) {
        fprintf(stderr, "records_dump: invariant: %s\n", v.what());
        return 4;
    } catch (const std::exception &ex) {
        fprintf(stderr, "records_dump: %s\n", ex.what());
        return 2;
    }
    return 0;
}
