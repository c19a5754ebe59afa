// juliet — command-line front end over libjuliet_hip.so: aligned CCS BAM in, JSON (and a plain HTML
// rendering of it) out.  Keeps the documented surface of the reference tool:
//   juliet [--config/-c CFG] [--mode-phasing/-p] [--region/-r B-E] [--min-perc X] [--max-perc X] [--drm-only]
//          in.align.bam out.{json,html} [out2.{json,html}]
//   juliet [options] --batch samples.tsv   (many per-barcode BAMs in one process: BatchRunner below)
// (doc/JULIET.md:62-66, 121, 160-163, 195, 270-271, 342-344, 352-354, 370).  Everything the reference text
// leaves open is an explicit flag with the docs/SPEC.md default.  All compute happens on the GPU through
// the C ABI; without a gfx950 device the tool exits with status 3.
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <future>
#include <cstdlib>
#include <ctime>
#include <filesystem>
#include <fstream>
#include <functional>
#include <iostream>
#include <map>
#include <memory>

#include "config.hpp"
#include "decode.hpp"
#include "format.hpp"
#include "fuse.hpp"
#include "html.hpp"
#include "msa_builder.hpp"

using namespace jlhost;

namespace {

const char *kVersion = "0.1.0 (minorseq_amd, MI355X)";

struct Options {
    std::string bam, config;
    std::vector<std::string> outputs;
    bool phasing = false, drm_only = false;
    bool have_region = false;
    uint32_t region_b = 0, region_e = 0;
    double min_perc = -1.0, max_perc = -1.0;
    double alpha = 0.01, n_tests = 0.0;
    std::string chemistry = "auto";
    double match = -1.0, substitution = -1.0;
    int expected_round = 0;
    int fisher_tail = 0;             // --fisher-tail greater|two-sided (doc/JULIET.md:38-42 leaves the sidedness open)
    uint32_t min_reads = 10, min_qv = 0;
    bool qv_upload_mask = false;     // --qv-upload mask|bytes: what --min-qv sends to the device (bytes: DESIGN.md, the record ingest)
    double min_rq = 0.0;
    int device = 0;
    uint32_t windows = 1;            // column windows the reference is cut into (doc/JULIET.md:261-264: the split never shows)
    std::vector<int> devices;        // --devices a,b,...: one rank (thread) per device, consecutive windows each
    std::string dump_msa, dump_config, consensus;
    std::string hap_fasta;           // --haplotype-fasta: one consensus per reported haplotype (docs/SPEC.md §13)
    bool rescue = false;             // --rescue-damaged: which reported haplotype each damaged read agrees with (docs/SPEC.md §14)
    uint32_t rescue_min = 1;         // --rescue-min-positions K: informative positions a read needs to be judged at all
    bool have_rescue_min = false;
    bool linkage = false;            // --linkage: every pair of called variants over the reads covering both (docs/SPEC.md §15)
    bool fuse_only = false;        // invoked as `fuse in.bam out.fasta` (doc/FUSE.md:26-31): the consensus and nothing else
    double ins_min_frac = 0.5;     // an insertion enters the consensus when more than this share of the covering reads carries it
    uint32_t ins_min_distance = 10;  // ... and the previous included insertion lies at least this many columns back (UNPINNED)
    bool timing = false;
    std::string exchange;            // --exchange rccl|inproc: how the rank threads exchange (default: rccl, inproc when a device repeats)
    // Sampling (docs/SPEC.md §12): the window is ingested whole, then replaced by chosen reads of it on the device (jl_msa_take)
    bool have_downsample = false;
    uint64_t downsample = 0;         // --downsample N: keep N reads (with --mix: the mixture's coverage, default 3000 as mixdata's COVERAGE)
    uint64_t sample_seed = 0;        // --sample-seed S (source m of a mixture is sampled with S + m)
    std::vector<std::string> mix;    // --mix b.bam[,c.bam...]: the minor clones; the positional BAM is the major one (doc/MIXDATA.md)
    double mix_perc = 1.0;           // --mix-perc P: percent of the mixture each minor clone gets
    bool sampling() const { return have_downsample || !mix.empty(); }
    std::string batch;               // --batch samples.tsv: one `in.bam<TAB>out1[<TAB>out2]` per line, every other option for all of them
    struct BatchLine { unsigned line; std::string bam; std::vector<std::string> outputs; };
    std::vector<BatchLine> batch_lines;
};

[[noreturn]] void usage(int code)
{
    std::cerr <<
        "juliet " << kVersion << "\n"
        "usage: juliet [options] in.align.bam out.json|out.html [second output]\n"
        "       juliet [options] --batch samples.tsv\n"
        "  -c, --config <HIV|ABL1|file.json>   target config (doc/JULIET.md:109-180)\n"
        "  -p, --mode-phasing                  cluster reads into haplotypes (doc/JULIET.md:192-211)\n"
        "  -r, --region <begin-end>            1-based [begin,end) window of the config to call\n"
        "      --min-perc <x> / --max-perc <x> only calls above / below x percent\n"
        "  -k, --drm-only                      only known DRM positions of the config\n"
        "  parameters the reference text leaves open (docs/SPEC.md):\n"
        "      --alpha 0.01  --n-tests <auto>  --chemistry auto|sequel|permissive\n"
        "      --match-rate <r> --substitution-rate <r> --expected-round ceil|floor|nearest\n"
        "      --fisher-tail greater|two-sided  sidedness of Fisher's exact test (default greater: an excess of observed codons)\n"
        "      --min-reads 10  --min-qv 0  --min-rq 0  --device 0\n"
        "      --qv-upload mask|bytes          what --min-qv sends to the device: the filter decided while decoding, one bit per\n"
        "                                      base, or the folded qualities, one byte per base, and the threshold (default);\n"
        "                                      the same output\n"
        "      --windows K [--devices a,b,...] cut the reference into K column windows (2-column overlap, global Bonferroni\n"
        "                                      factor), consecutive windows per device; phasing runs across the windows with\n"
        "                                      the reads sharded over the devices.  The output is that of one window.\n"
        "      --exchange rccl|inproc          how the rank threads exchange: RCCL (default), or device copies between the ranks'\n"
        "                                      buffers (peer copies over xGMI; the default when a device is named twice,\n"
        "                                      which RCCL refuses)\n"
        "      --consensus <out.fasta>         also write the window's consensus as `fuse` would (doc/FUSE.md:17-20):\n"
        "                                      majority base, major deletions removed, in-frame majority insertions kept\n"
        "      --ins-min-frac 0.5  --ins-min-distance 10   when an insertion enters the consensus\n"
        "      --haplotype-fasta <out.fasta>   with --mode-phasing: one consensus record per reported haplotype, in the JSON's\n"
        "                                      order, from the column pileup of that haplotype's reads alone (docs/SPEC.md section\n"
        "                                      13): majority base, major deletions removed, N where none of its reads covers the\n"
        "                                      column.  Insertions are not included (their counters are per window, not per\n"
        "                                      read).  Follows --downsample / --mix.  Not with --windows, --devices a,b, --batch\n"
        "                                      or as fuse\n"
        "      --rescue-damaged [--rescue-min-positions K]  with --mode-phasing: every damaged read (a deletion, a filtered N or an\n"
        "                                      uncovered cell at some variant position) is compared with the reported haplotypes at\n"
        "                                      the positions where it can be read, K of them at least (default 1; docs/SPEC.md\n"
        "                                      section 14): it is assigned to the one haplotype that agrees there, or counted as\n"
        "                                      ambiguous, incompatible or uninformative.  The haplotype block gains `rescue`, every\n"
        "                                      haplotype rescued_reads, rescued_read_names and frequency_with_rescued; with\n"
        "                                      --haplotype-fasta the rescued reads join their haplotype's consensus.  Follows\n"
        "                                      --downsample / --mix.  Not with --windows, --devices a,b, --batch or as fuse\n"
        "      --linkage                       pairwise linkage of the called variants over every read covering both (docs/SPEC.md\n"
        "                                      section 15), with and without --mode-phasing: read i is informative at a position iff\n"
        "                                      its three codes there are all < 4; it carries a variant iff it is informative at its\n"
        "                                      position and its codon there equals the variant's.  The JSON root gains `linkage`:\n"
        "                                      one entry per pair of variants at different positions with reads_both > 0 — the 2 x 2\n"
        "                                      table n11 n10 n01 n00 of the reads informative at both, r2, d_prime and the two\n"
        "                                      one-sided Fisher tests p_positive, p_negative, not Bonferroni-corrected\n"
        "                                      (n_pairs_tested is there to correct with).  At most 1024 variants at 1024 positions:\n"
        "                                      beyond, a warning and \"skipped\": true.  Follows --downsample / --mix.  Not with\n"
        "                                      --windows, --devices a,b, --batch or as fuse\n"
        "      --downsample N [--sample-seed S]  call on N reads of the sample (\"downsample it to 6000x\", doc/JULIETFLOW.md:23-25):\n"
        "                                      the reads are chosen by docs/SPEC.md section 12 (seed default 0; samples of one seed are\n"
        "                                      nested) and gathered on the device; N at or above the read count changes nothing.\n"
        "                                      With --batch: every sample.  Not with --windows, --devices a,b or --consensus\n"
        "      --mix b.bam[,c.bam...] [--mix-perc P]  a mixture as mixdata makes it (doc/MIXDATA.md): in.bam is the major clone, every\n"
        "                                      listed BAM a minor clone with P percent (default 1) of --downsample C reads (default\n"
        "                                      3000); source m is sampled with seed S + m.  A source with too few reads is an input\n"
        "                                      error (2).  Not with --batch, --windows, --devices a,b or --consensus\n"
        "      --batch <samples.tsv>           many samples in one process: one `in.bam<TAB>out1[<TAB>out2]` per line (blank lines\n"
        "                                      and lines starting with # skipped); every other option applies to every sample and\n"
        "                                      each sample gets the files a single run would write.  A sample that fails is named\n"
        "                                      on stderr and the others go on (exit status 2 if any failed); a GPU error stops\n"
        "                                      the batch (3).  Not with --windows, --devices a,b, --consensus or --dump-*\n"
        "      --timing                        wall time of each stage on stderr\n"
        "  diagnostics (no GPU needed): --dump-msa <file>  --dump-config <file>\n";
    std::exit(code);
}

bool output_kind_ok(const std::string &out)   // the outputs are told apart by their extension (doc/JULIET.md:61-66)
{
    return out.size() > 5 && (out.substr(out.size() - 5) == ".json" || out.substr(out.size() - 5) == ".html");
}

// The --batch list: `in.bam<TAB>out1[<TAB>out2 ...]` per line; blank lines and lines starting with # are skipped.  Anything
// wrong with it ends the process with status 1 before any BAM is read.
std::vector<Options::BatchLine> read_batch_list(const std::string &path)
{
    auto bad = [&](unsigned line, const std::string &why) {
        std::cerr << "juliet: --batch " << path;
        if (line) std::cerr << " line " << line;
        std::cerr << ": " << why << "\n";
        std::exit(1);
    };
    std::error_code ec;
    if (std::filesystem::is_directory(path, ec)) bad(0, "is a directory");
    std::ifstream f(path);
    if (!f) bad(0, "cannot be read");
    std::vector<Options::BatchLine> lines;
    std::map<std::string, unsigned> written;   // output path (absolute, normalised) -> the line that names it
    std::string text;
    unsigned no = 0;
    while (std::getline(f, text)) {
        ++no;
        if (!text.empty() && text.back() == '\r') text.pop_back();
        if (text.find_first_not_of(" \t") == std::string::npos || text[0] == '#') continue;
        std::vector<std::string> fields;
        for (size_t b = 0;;) {
            const size_t e = text.find('\t', b);
            fields.push_back(text.substr(b, e == std::string::npos ? std::string::npos : e - b));
            if (e == std::string::npos) break;
            b = e + 1;
        }
        if (fields.size() < 2) bad(no, "wants an input BAM and at least one output, separated by tabs");
        for (const std::string &fld : fields)
            if (fld.empty()) bad(no, "has an empty field");
        Options::BatchLine l{no, fields[0], std::vector<std::string>(fields.begin() + 1, fields.end())};
        for (const std::string &out : l.outputs) {
            if (!output_kind_ok(out)) bad(no, "output '" + out + "' must end in .json or .html (doc/JULIET.md:61-66)");
            const std::string key = std::filesystem::absolute(out, ec).lexically_normal().string();
            const auto it = written.find(key);
            if (it != written.end())
                bad(no, "output '" + out + "' is also written by line " + std::to_string(it->second) + " (every output once)");
            written.emplace(key, no);
        }
        lines.push_back(std::move(l));
    }
    if (f.bad()) bad(0, "cannot be read");
    if (lines.empty()) bad(0, "names no sample");
    return lines;
}

Options parse(int argc, char **argv)
{
    Options o;
    auto need = [&](int &i) -> std::string {
        if (i + 1 >= argc) { std::cerr << "juliet: " << argv[i] << " needs a value\n"; usage(1); }
        return argv[++i];
    };
    std::vector<std::string> pos;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "-h" || a == "--help") usage(0);
        else if (a == "--version") { std::cout << kVersion << "\n"; std::exit(0); }
        else if (a == "-c" || a == "--config") o.config = need(i);
        else if (a == "-p" || a == "--mode-phasing") o.phasing = true;
        else if (a == "-k" || a == "--drm-only") o.drm_only = true;
        else if (a == "-r" || a == "--region") {
            const std::string v = need(i);
            const size_t d = v.find('-');
            if (d == std::string::npos) { std::cerr << "juliet: --region wants begin-end\n"; usage(1); }
            o.region_b = (uint32_t)std::stoul(v.substr(0, d));
            o.region_e = (uint32_t)std::stoul(v.substr(d + 1));
            o.have_region = true;
        }
        else if (a == "--min-perc") o.min_perc = std::stod(need(i));
        else if (a == "--max-perc") o.max_perc = std::stod(need(i));
        else if (a == "--alpha") o.alpha = std::stod(need(i));
        else if (a == "--n-tests") o.n_tests = std::stod(need(i));
        else if (a == "--chemistry") o.chemistry = need(i);
        else if (a == "--match-rate") o.match = std::stod(need(i));
        else if (a == "--substitution-rate") o.substitution = std::stod(need(i));
        else if (a == "--expected-round") {
            const std::string v = need(i);
            o.expected_round = v == "floor" ? 1 : v == "nearest" ? 2 : 0;
        }
        else if (a == "--fisher-tail") {
            const std::string v = need(i);
            if (v == "greater") o.fisher_tail = 0;
            else if (v == "two-sided") o.fisher_tail = 1;
            else { std::cerr << "juliet: --fisher-tail takes greater or two-sided\n"; usage(1); }
        }
        else if (a == "--min-reads") o.min_reads = (uint32_t)std::stoul(need(i));
        else if (a == "--min-qv") o.min_qv = (uint32_t)std::stoul(need(i));
        else if (a == "--qv-upload") {
            const std::string v = need(i);
            if (v != "mask" && v != "bytes") { std::cerr << "juliet: --qv-upload takes mask or bytes\n"; usage(1); }
            o.qv_upload_mask = v == "mask";
        }
        else if (a == "--min-rq") o.min_rq = std::stod(need(i));
        else if (a == "--device") o.device = std::stoi(need(i));
        else if (a == "--windows") o.windows = (uint32_t)std::stoul(need(i));
        else if (a == "--exchange") {
            o.exchange = need(i);
            if (o.exchange != "rccl" && o.exchange != "inproc") { std::cerr << "juliet: --exchange wants rccl or inproc\n"; usage(1); }
        }
        else if (a == "--devices") {
            const std::string v = need(i);
            size_t b = 0;
            while (b <= v.size()) {
                const size_t e = std::min(v.find(',', b), v.size());
                if (e > b) o.devices.push_back(std::stoi(v.substr(b, e - b)));
                b = e + 1;
            }
        }
        else if (a == "--consensus") o.consensus = need(i);
        else if (a == "--haplotype-fasta") o.hap_fasta = need(i);
        else if (a == "--rescue-damaged") o.rescue = true;
        else if (a == "--linkage") o.linkage = true;
        else if (a == "--rescue-min-positions") { o.rescue_min = (uint32_t)std::stoul(need(i)); o.have_rescue_min = true; }
        else if (a == "--ins-min-frac") o.ins_min_frac = std::stod(need(i));
        else if (a == "--ins-min-distance") o.ins_min_distance = (uint32_t)std::stoul(need(i));
        else if (a == "--dump-msa") o.dump_msa = need(i);
        else if (a == "--dump-config") o.dump_config = need(i);
        else if (a == "--timing") o.timing = true;
        else if (a == "--batch") o.batch = need(i);
        else if (a == "--downsample") { o.downsample = std::stoull(need(i)); o.have_downsample = true; }
        else if (a == "--sample-seed") o.sample_seed = std::stoull(need(i));
        else if (a == "--mix") {
            const std::string v = need(i);
            for (size_t b = 0; b <= v.size();) {
                const size_t e = std::min(v.find(',', b), v.size());
                if (e > b) o.mix.push_back(v.substr(b, e - b));
                b = e + 1;
            }
            if (o.mix.empty()) { std::cerr << "juliet: --mix names no BAM\n"; std::exit(1); }
        }
        else if (a == "--mix-perc") o.mix_perc = std::stod(need(i));
        else if (!a.empty() && a[0] == '-') { std::cerr << "juliet: unknown option " << a << "\n"; usage(1); }
        else pos.push_back(a);
    }
    const std::string prog = argv[0];
    const size_t slash = prog.find_last_of('/');
    const bool as_fuse = (slash == std::string::npos ? prog : prog.substr(slash + 1)) == "fuse";
    if (!o.hap_fasta.empty()) {   // refused here, before any file is read or any GPU work
        auto refuse = [](const char *why) { std::cerr << "juliet: --haplotype-fasta " << why << "\n"; std::exit(1); };
        if (as_fuse) refuse("is not an option of fuse");
        if (!o.phasing) refuse("writes the haplotypes of a phasing run (add --mode-phasing)");
        if (o.windows > 1 || o.devices.size() > 1) refuse("works on one window of one device (drop --windows / --devices a,b)");
        if (!o.batch.empty()) refuse("writes one file for one sample (not with --batch)");
    }
    if (o.rescue || o.have_rescue_min) {   // refused here, before any file is read or any GPU work
        auto refuse = [](const char *why) { std::cerr << "juliet: --rescue-damaged [--rescue-min-positions K] " << why << "\n"; std::exit(1); };
        if (!o.rescue) refuse("--rescue-min-positions sets a threshold of --rescue-damaged (add it)");
        if (o.rescue_min == 0) refuse("wants at least one informative position (--rescue-min-positions 0)");
        if (as_fuse) refuse("are not options of fuse");
        if (!o.phasing) refuse("assigns reads to the haplotypes of a phasing run (add --mode-phasing)");
        if (o.windows > 1 || o.devices.size() > 1) refuse("works on one window of one device (drop --windows / --devices a,b)");
        if (!o.batch.empty()) refuse("is not part of a batch (not with --batch)");
    }
    if (o.linkage) {   // refused here, before any file is read or any GPU work
        auto refuse = [](const char *why) { std::cerr << "juliet: --linkage " << why << "\n"; std::exit(1); };
        if (as_fuse) refuse("is not an option of fuse");
        if (o.windows > 1 || o.devices.size() > 1) refuse("works on one window of one device (drop --windows / --devices a,b)");
        if (!o.batch.empty()) refuse("is not part of a batch (not with --batch)");
    }
    if (o.sampling()) {   // what sampling cannot be combined with is refused here, before any file is read or any GPU work
        auto refuse = [&](const char *why) { std::cerr << "juliet: " << (o.mix.empty() ? "--downsample " : "--mix ") << why << "\n"; std::exit(1); };
        if (o.have_downsample && o.downsample == 0) refuse("wants at least one read (--downsample 0)");
        if (o.windows > 1 || o.devices.size() > 1) refuse("works on one window of one device (drop --windows / --devices a,b)");
        if (!o.consensus.empty() || as_fuse) refuse("carries no insertion counters into the sample: no consensus (drop --consensus)");
        if (!o.mix.empty()) {
            if (!o.batch.empty()) refuse("mixes into one sample (not with --batch)");
            if (o.mix.size() + 1 > (size_t)JL_TAKE_MAX_PARTS) refuse("takes at most 15 minor clones");
            if (!o.have_downsample) o.downsample = 3000;   // mixdata's COVERAGE (doc/MIXDATA.md)
            std::vector<uint64_t> counts(o.mix.size() + 1);
            if (jl_mix_counts((uint32_t)counts.size(), o.downsample, o.mix_perc, counts.data()) != JL_OK)
                refuse("wants --mix-perc inside (0, 100) and minor clones that together stay within the coverage");
        }
    }
    if (!o.batch.empty()) {   // everything a batch cannot do is refused here, before any file is read or any GPU work
        auto refuse = [](const char *why) { std::cerr << "juliet: --batch " << why << "\n"; std::exit(1); };
        if (as_fuse) refuse("is not an option of fuse");
        if (!pos.empty()) refuse("takes no input BAM or outputs on the command line: they are the lines of the list");
        if (o.windows > 1) refuse("runs one window per sample (drop --windows)");
        if (o.devices.size() > 1) refuse("runs on one device (--device, not a --devices list)");
        if (!o.consensus.empty()) refuse("writes no consensus (drop --consensus)");
        if (!o.dump_msa.empty() || !o.dump_config.empty()) refuse("does not combine with --dump-msa or --dump-config");
        if (!o.devices.empty()) o.device = o.devices[0];
        o.devices.assign(1, o.device);
        o.batch_lines = read_batch_list(o.batch);
        return o;
    }
    if (!o.dump_config.empty() && pos.empty()) { if (o.devices.empty()) o.devices.push_back(o.device); return o; }
    {   // `fuse in.bam out.fasta` (doc/FUSE.md:26-31): the same front end, asked for the consensus only
        if (as_fuse) {
            if (pos.size() != 2) { std::cerr << "fuse: usage: fuse in.align.bam out.fasta\n"; std::exit(1); }
            o.bam = pos[0];
            o.consensus = pos[1];
            o.fuse_only = true;
            o.devices.assign(1, o.device);
            o.windows = 1;
            return o;
        }
    }
    if (o.devices.empty()) o.devices.push_back(o.device);
    if (o.windows == 0 || o.windows > 32u * o.devices.size()) { std::cerr << "juliet: --windows wants 1 .. 32 per device\n"; usage(1); }
    if (o.windows < o.devices.size()) { std::cerr << "juliet: fewer windows than devices\n"; usage(1); }
    if ((o.windows > 1 || o.devices.size() > 1) && !o.consensus.empty()) {
        std::cerr << "juliet: --consensus works on one window (drop --windows / --devices)\n";
        usage(1);
    }
    if (pos.size() < 2 && o.dump_msa.empty()) { std::cerr << "juliet: need an input BAM and at least one output\n"; usage(1); }
    if (pos.empty()) usage(1);
    o.bam = pos[0];
    o.outputs.assign(pos.begin() + 1, pos.end());
    for (const std::string &out : o.outputs) {
        if (!output_kind_ok(out)) { std::cerr << "juliet: output '" << out << "' must end in .json or .html (doc/JULIET.md:61-66)\n"; usage(1); }
    }
    return o;
}

std::string iso_now()
{
    using namespace std::chrono;
    const auto now = system_clock::now();
    const std::time_t t = system_clock::to_time_t(now);
    const int ms = (int)(duration_cast<milliseconds>(now.time_since_epoch()).count() % 1000);
    std::tm tm;
    gmtime_r(&t, &tm);
    char buf[80];
    snprintf(buf, sizeof buf, "%04d-%02d-%02dT%02d:%02d:%02d.%03dZ", tm.tm_year + 1900, tm.tm_mon + 1, tm.tm_mday,
             tm.tm_hour, tm.tm_min, tm.tm_sec, ms);
    return buf;
}

std::string haplotype_name(uint32_t h)  // [A-Z]{1}[a-z]?  (doc/JULIET.md:198)
{
    if (h < 26) return std::string(1, (char)('A' + h));
    h -= 26;
    return std::string{(char)('A' + h / 26), (char)('a' + h % 26)};
}

void die_jl(jl_ctx *ctx, const char *what)
{
    std::cerr << "juliet: " << what << ": " << jl_last_error(ctx) << "\n";
    std::exit(3);
}

// A few threads that copy: the uploader's gather is 0.45 GB into pages nobody has touched yet (1.35 GB of a 100k-read rich-QV BAM's
// records become 0.45 GB of arrays).  As range inserts on the uploader thread it was 120-140 ms — a vector with an allocator of its own
// inserts element by element — more than the whole decode takes since the quality tracks are folded sixteen bases an instruction;
// as memcpy in 1 MB pieces by these threads and the uploader 18-34 ms.  add() splits a copy; wait() helps until every piece is done.
class CopyCrew {
public:
    explicit CopyCrew(unsigned n)
    {
        for (unsigned i = 0; i < n; ++i) th_.emplace_back([this] { work(false); });
    }
    ~CopyCrew()
    {
        {
            std::lock_guard<std::mutex> lk(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
    void add(void *dst, const void *src, size_t bytes)
    {
        const size_t piece = (size_t)1 << 20;
        {
            std::lock_guard<std::mutex> lk(m_);
            for (size_t o = 0; o < bytes; o += piece) {
                q_.push_back({(uint8_t *)dst + o, (const uint8_t *)src + o, std::min(piece, bytes - o)});
                ++pending_;
            }
        }
        cv_.notify_all();
    }
    void wait() { work(true); }

private:
    struct Job { uint8_t *dst; const uint8_t *src; size_t n; };
    void work(bool until_idle)
    {
        std::unique_lock<std::mutex> lk(m_);
        for (;;) {
            if (!q_.empty()) {
                const Job j = q_.front();
                q_.pop_front();
                lk.unlock();
                memcpy(j.dst, j.src, j.n);
                lk.lock();
                if (--pending_ == 0) done_.notify_all();
                continue;
            }
            if (until_idle) {
                done_.wait(lk, [this] { return pending_ == 0; });
                return;
            }
            if (stop_) return;
            cv_.wait(lk, [this] { return stop_ || !q_.empty(); });
        }
    }
    std::mutex m_;
    std::condition_variable cv_, done_;
    std::deque<Job> q_;
    size_t pending_ = 0;
    bool stop_ = false;
    std::vector<std::thread> th_;
};

// Hands decoded records to the device chunk by chunk while the parser works on the next chunk: the upload (0.03 s for
// 100k reads) hides under the decode whenever the GPU context is up before the file ends; chunks that arrive earlier
// simply wait.  One consumer thread: chunks stay in file order.
class RecordUploader {
public:
    // one records context per device: every chunk goes to each of them (one rank per device reads its windows out of it)
    // want_qual: the chunks carry the folded quality bytes; qv_mask: the filter as one bit per base instead (IngestOptions::qv_mask)
    RecordUploader(std::vector<std::shared_future<std::pair<int, jl_ctx *>>> ctx_up, uint64_t file_bytes, bool want_qual, bool qv_mask = false)
        : ctx_up_(std::move(ctx_up)), file_bytes_(file_bytes), want_qual_(want_qual && !qv_mask), qv_mask_(want_qual && qv_mask), th_([this] { run(); })
    {
    }
    ~RecordUploader() { finish(); }
    RecordUploader(const RecordUploader &) = delete;
    RecordUploader &operator=(const RecordUploader &) = delete;

    // parser side: trade the full chunk for an empty one
    void give(RecordArrays &chunk)
    {
        RecordArrays fresh;
        const size_t want_seq = chunk.seq4.size() + chunk.seq4.size() / 4, want_cig = chunk.cigar.size() + chunk.cigar.size() / 4,
                     want_qual = chunk.qual.size() + chunk.qual.size() / 4, want_reads = chunk.pos.size() + 1;
        {
            std::lock_guard<std::mutex> lk(m_);
            if (!pool_.empty()) {
                fresh = std::move(pool_.back());
                pool_.pop_back();
            }
            q_.push_back(std::move(chunk));
        }
        cv_.notify_one();
        chunk = std::move(fresh);
        chunk.clear();
        // a new chunk starts at the size of the one before it instead of growing by doubling
        chunk.seq4.reserve(want_seq);
        chunk.cigar.reserve(want_cig);
        chunk.qual.reserve(want_qual);
        chunk.pos.reserve(want_reads);
        chunk.cig_off.reserve(want_reads);
        chunk.seq_off.reserve(want_reads);
        if (want_qual) chunk.qual_off.reserve(want_reads);
        chunk.names.reserve(want_reads);
    }
    // no more chunks: waits for the uploads; the records are on the device when this returns JL_OK
    int finish()
    {
        if (th_.joinable()) {
            {
                std::lock_guard<std::mutex> lk(m_);
                done_ = true;
            }
            cv_.notify_one();
            th_.join();
        }
        return rc_;
    }
    jl_ctx *ctx(size_t k = 0) const { return k < ctxs_.size() ? ctxs_[k] : nullptr; }
    jl_ctx *failed() const { return failed_; }
    std::vector<std::string> names;
    uint64_t n_reads = 0;
    double ms_begin = 0, ms_append = 0, ms_append_max = 0, ms_names = 0, ms_gather = 0;   // --timing
    unsigned n_appends = 0;

private:
    static double ms_since(std::chrono::steady_clock::time_point t)
    {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
    }
    // Chunk after chunk (offsets relative to the chunk) behind each other in `big_`: what the decoder hands over while the
    // GPU runtime is still starting goes to the device as a few LARGE copies once the contexts exist — a pageable copy pins its
    // source range first, and sixty-one chunks of a few MB, each a buffer the runtime has not seen, cost 16-25 ms where the same
    // 200 MB out of five arrays cost 5-6 (tools_tuning/h2d_threads.cpp: 21 against 36 GB/s on first touch).  The gathering
    // itself runs beside the decode, on this thread.
    // (the large arrays — bases, qualities, cigar words — by the copy crew: the chunk and `big_` must stay as they are until crew_.wait())
    template <typename V, typename W> void gather_array(V &dst, const W &src)
    {
        const size_t at = dst.size();
        if (at + src.size() > dst.capacity()) crew_.wait();      // (it moves: nobody may be copying into the old place)
        dst.resize(at + src.size());
        crew_.add(dst.data() + at, src.data(), src.size() * sizeof(src[0]));
    }
    void gather(const RecordArrays &c)
    {
        const size_t n = c.pos.size();
        if (qv_mask_ && (big_.seq4.size() & 3u)) {
            // a chunk's mask begins at its first base: every chunk begins on four bytes of the gathered bases, a whole byte of the
            // gathered mask (the read before ends where the gap does: offsets may leave gaps)
            const size_t padded = (big_.seq4.size() + 3u) & ~(size_t)3u;
            if (padded > big_.seq4.capacity()) crew_.wait();      // (it moves: nobody may be copying into the old place)
            big_.seq4.resize(padded, 0);
            big_.seq_off.back() = big_.seq4.size();
        }
        const uint64_t cb = big_.cigar.size(), sb = big_.seq4.size(), qb = big_.qual.size();
        big_.pos.insert(big_.pos.end(), c.pos.begin(), c.pos.end());
        gather_array(big_.cigar, c.cigar);
        gather_array(big_.seq4, c.seq4);
        for (size_t i = 1; i <= n; ++i) {
            big_.cig_off.push_back(cb + c.cig_off[i] - c.cig_off[0]);
            big_.seq_off.push_back(sb + c.seq_off[i] - c.seq_off[0]);
        }
        if (qv_mask_) gather_array(big_.qmask, c.qmask);
        if (want_qual_) {
            gather_array(big_.qual, c.qual);
            for (size_t i = 1; i <= n; ++i) big_.qual_off.push_back(qb + c.qual_off[i] - c.qual_off[0]);
        }
    }
    size_t gathered_bytes() const { return big_.seq4.size() + big_.qual.size() + big_.qmask.size() + 4 * big_.cigar.size(); }
    bool contexts_ready() const
    {
        for (const auto &f : ctx_up_)
            if (f.wait_for(std::chrono::seconds(0)) != std::future_status::ready) return false;
        return true;
    }
    void open()   // waits for the contexts
    {
        for (auto &f : ctx_up_) {
            const auto up = f.get();
            ctxs_.push_back(up.second);
            if (up.first != JL_OK && rc_ == JL_OK) rc_ = up.first;
        }
        for (jl_ctx *c : ctxs_) {
            if (rc_ != JL_OK) break;
            // CCS BAMs inflate 5-10x; the packed bases are about a third of that, qualities twice the bases, a cigar word per
            // dozen bases when every filtered base is an X of its own (the arrays grow if not — each growth is an allocation, a
            // device copy and a free behind a synchronisation, so the hints err on the large side: memory is not the constraint)
            const uint64_t seq_hint = std::min<uint64_t>(file_bytes_ * 7 / 2, (uint64_t)4 << 30);
            const auto t = std::chrono::steady_clock::now();
            rc_ = jl_records_begin(c, seq_hint / 512 + 1024, seq_hint / 8 + 1024, seq_hint, want_qual_ ? seq_hint * 2 : 0);
            if (rc_ != JL_OK) failed_ = c;
            ms_begin += ms_since(t);
        }
        ready_ = true;
    }
    void flush()
    {
        if (big_.pos.empty()) return;
        const auto t = std::chrono::steady_clock::now();
        for (jl_ctx *dst : ctxs_) {
            if (rc_ != JL_OK) break;
            if (qv_mask_)
                rc_ = jl_records_append_masked(dst, big_.pos.size(), big_.pos.data(), big_.cigar.data(), big_.cig_off.data(),
                                               big_.seq4.data(), big_.seq_off.data(), big_.qmask.data());
            else
                rc_ = jl_records_append(dst, big_.pos.size(), big_.pos.data(), big_.cigar.data(), big_.cig_off.data(), big_.seq4.data(),
                                        big_.seq_off.data(), want_qual_ ? big_.qual.data() : nullptr,
                                        want_qual_ ? big_.qual_off.data() : nullptr);
            if (rc_ != JL_OK) failed_ = dst;
        }
        const double ms = ms_since(t);
        ms_append += ms;
        ms_append_max = std::max(ms_append_max, ms);
        ++n_appends;
        big_.clear();
    }
    void run()
    {
        // the gathered arrays at about the size the device arrays get (virtual until touched), at most kGatherCap at a time
        const size_t kGatherCap = (size_t)512 << 20;
        {
            const size_t seq_hint = (size_t)std::min<uint64_t>(file_bytes_ * 7 / 2, kGatherCap);
            big_.seq4.reserve(seq_hint);
            big_.cigar.reserve(seq_hint / 8);
            if (want_qual_) big_.qual.reserve(2 * seq_hint);
            if (qv_mask_) big_.qmask.reserve(seq_hint / 4 + 64);
        }
        for (;;) {
            std::deque<RecordArrays> got;
            bool finished = false;
            {
                std::unique_lock<std::mutex> lk(m_);
                if (ready_) cv_.wait(lk, [this] { return done_ || !q_.empty(); });
                else cv_.wait_for(lk, std::chrono::microseconds(250), [this] { return done_ || !q_.empty(); });   // (the contexts too)
                got.swap(q_);
                finished = done_ && got.empty();
            }
            auto t = std::chrono::steady_clock::now();
            for (RecordArrays &c : got) gather(c);
            ms_gather += ms_since(t);
            t = std::chrono::steady_clock::now();
            for (RecordArrays &c : got) {      // (beside the crew's copies)
                n_reads += c.pos.size();
                for (std::string &nm : c.names) names.push_back(std::move(nm));
            }
            ms_names += ms_since(t);
            t = std::chrono::steady_clock::now();
            crew_.wait();
            ms_gather += ms_since(t);
            for (RecordArrays &c : got) {
                c.clear();
                std::lock_guard<std::mutex> lk(m_);
                if (pool_.size() < 8) pool_.push_back(std::move(c));
            }
            if (!ready_ && (finished || gathered_bytes() >= kGatherCap || contexts_ready())) open();
            // on the device as soon as nothing more is waiting to be gathered (while the decode still runs: chunk by chunk,
            // hidden under it, as before)
            if (ready_) {
                bool idle;
                {
                    std::lock_guard<std::mutex> lk(m_);
                    idle = q_.empty();
                }
                if (idle || finished || gathered_bytes() >= kGatherCap / 2) flush();
            }
            if (finished) return;
        }
    }
    std::vector<std::shared_future<std::pair<int, jl_ctx *>>> ctx_up_;
    uint64_t file_bytes_;
    bool want_qual_, qv_mask_;
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<RecordArrays> q_;
    std::vector<RecordArrays> pool_;
    bool done_ = false, ready_ = false;
    RecordArrays big_;
    static unsigned crew_size()
    {
        if (const char *e = getenv("JL_COPY_THREADS")) return std::max(1, atoi(e));     // (tuning)
        return 3;      // (1, 3, 8 on the 16-thread box: 23-34, 18-25, 19-28 ms for the 0.45 GB — the uploader thread copies too)
    }
    CopyCrew crew_{crew_size()};
    int rc_ = JL_OK;
    std::vector<jl_ctx *> ctxs_;
    jl_ctx *failed_ = nullptr;
    std::thread th_;   // last: starts in the constructor's initialiser list
};


// What the device stage hands to the writers, whichever way it ran (one window, or K windows over R devices).
struct Results {
    std::vector<jl_variant> var;          // (gene, codon_pos, codon) order; col relative to the overall window
    std::vector<uint32_t> col_counts;     // [n_cols][6] of the overall window
    jl_phase_summary ps = {};
    std::vector<uint32_t> pos_cols, hap_count;   // pos_cols relative to the overall window
    std::vector<uint8_t> hap_pattern, hit;
    size_t pat_stride = 0, hit_stride = 0;       // hap_pattern[h * pat_stride + p], hit[v * hit_stride + h]
    std::vector<uint16_t> read_hap;
    // --rescue-damaged (docs/SPEC.md §14): rescue[i] of every read by the run's own positions and haplotypes; empty when no call
    // was made (no reported haplotype, or more positions asked for than the run has: every damaged read is uninformative then)
    bool rescued = false;
    uint32_t rescue_min = 0;
    std::vector<uint16_t> rescue;
    // --linkage (docs/SPEC.md §15): the three tables of ONE call over the table's distinct columns and its rows; link_var[k] = the
    // row of `var` that is variant k of the call (the rows by column: var_pos must not decrease, and genes may overlap)
    bool linked = false, link_skipped = false;
    std::vector<uint32_t> link_cols, link_var, link_var_pos, link_both, link_carry, link_joint;
    // the haplotype a damaged read was assigned to, or JL_HAP_DAMAGED; a read that is not damaged: its own id
    uint16_t hap_with_rescued(uint64_t i) const
    {
        if (read_hap[i] != (uint16_t)JL_HAP_DAMAGED || rescue.empty()) return read_hap[i];
        return rescue[i] < ps.n_haplotypes ? rescue[i] : (uint16_t)JL_HAP_DAMAGED;
    }
};

struct WindowPlan {
    uint32_t begin = 0, ncols = 0;   // reference columns [begin, begin + ncols)
    uint32_t own_begin = 0, own_end = 0;   // the columns whose pileup counts this window contributes (no overlap)
    int rank = 0;
};

// K windows with a 2-column overlap, so that every codon is evaluated by exactly one window whatever its frame
// (minorseq_amd/sharding.py window_bounds); consecutive windows per rank.
std::vector<WindowPlan> plan_windows(uint32_t win_begin, uint32_t n_cols, uint32_t k_windows, uint32_t n_ranks)
{
    std::vector<WindowPlan> w(k_windows);
    for (uint32_t k = 0; k < k_windows; ++k) {
        const uint32_t c0 = (uint32_t)((uint64_t)n_cols * k / k_windows), c1 = (uint32_t)((uint64_t)n_cols * (k + 1) / k_windows);
        w[k].begin = win_begin + c0;
        w[k].ncols = std::min(n_cols, c1 + (k + 1 < k_windows ? 2u : 0u)) - c0;
        w[k].own_begin = c0;
        w[k].own_end = c1;
        w[k].rank = (int)((uint64_t)k * n_ranks / k_windows);
    }
    return w;
}

struct DeviceStageInput {
    const Options *opt;
    const TargetConfig *cfg;
    const std::vector<jl_gene> *genes;
    const std::vector<uint8_t> *refcodes;
    jl_params prm;
    uint32_t win_begin, n_cols;
    uint64_t n_reads;
};

// --drm-only: the codons of the config's DRMs per evaluated position of one window (doc/JULIET.md:370)
int drm_masks_of(jl_ctx *ctx, const DeviceStageInput &in, std::vector<uint64_t> &masks)
{
    const uint8_t *refp = in.refcodes->empty() ? nullptr : in.refcodes->data();
    if (jl_pileup_async(ctx, in.genes->data(), (uint32_t)in.genes->size(), refp, (uint32_t)in.refcodes->size()) != JL_OK) return 1;
    const uint32_t P = jl_n_positions(ctx);
    std::vector<uint32_t> pg(P), pk(P);
    if (jl_pileup_fetch(ctx, nullptr, pg.data(), pk.data(), nullptr, nullptr, nullptr) != JL_OK) return 1;
    masks.assign(P, 0);
    for (uint32_t p = 0; p < P; ++p) {
        const GeneCfg &g = in.cfg->genes[pg[p]];
        for (unsigned cod = 0; cod < 64; ++cod)
            if (!in.cfg->known_drms(pg[p], pk[p] + g.first_codon, translate(cod)).empty()) masks[p] |= 1ull << cod;
    }
    return 0;
}

// One rank = one device: its windows out of the records uploaded to it, the call stage per window with the GLOBAL
// Bonferroni factor, then — with phasing — its share of the cross-window sequence (jl_xwin_phase_sharded: the ranks'
// collectives meet inside).  Every rank ends with the whole result; rank 0's is written.
// The rank threads of one process agree before they enter anything collective: a rank that failed on its own (context,
// ingest, call stage) must not leave its peers waiting inside the communicator's bootstrap or an exchange.  Every rank
// calls vote() exactly once; all of them learn whether all of them are fine.
struct RankVote {
    explicit RankVote(int n) : n_(n) {}
    bool vote(bool ok)
    {
        std::unique_lock<std::mutex> lk(m_);
        all_ok_ = all_ok_ && ok;
        if (++arrived_ == n_) cv_.notify_all();
        else cv_.wait(lk, [this] { return arrived_ == n_; });
        return all_ok_;
    }

private:
    std::mutex m_;
    std::condition_variable cv_;
    int n_, arrived_ = 0;
    bool all_ok_ = true;
};

struct RankJob {
    int rank = 0, world = 1, device = 0;
    jl_ctx *records = nullptr;
    std::vector<uint32_t> widx;          // this rank's windows (indices into the plan)
    std::vector<jl_ctx *> wins;
    jl_comm *comm = nullptr;
    bool inproc = false;                 // the ranks exchange by device copies, not over RCCL
    std::string error;                   // empty: fine
    std::vector<std::pair<const char *, double>> laps;   // --timing: milliseconds by stage of this rank (rank 0's are printed)
    // outputs
    std::vector<std::vector<jl_variant>> tables;   // per window (window-relative columns), call only
    Results res;                         // with phasing: the merged table and the haplotypes (rank 0's is used)
    uint64_t slice_begin = 0, slice_reads = 0;
    std::vector<uint16_t> ids;           // this rank's slice
};

// the stages of a rank that involve no other rank: window contexts, ingest, call stage, column counts
static void run_rank_local(RankJob &job, const DeviceStageInput &in, const std::vector<WindowPlan> &plan, std::vector<uint32_t> &col_counts,
                           std::chrono::steady_clock::time_point &t_last);

void run_rank(RankJob &job, const DeviceStageInput &in, const std::vector<WindowPlan> &plan, const uint8_t *comm_id,
              std::vector<uint32_t> &col_counts, const std::vector<uint64_t> &slice_begin, RankVote *vote)
{
    auto t_last = std::chrono::steady_clock::now();
    run_rank_local(job, in, plan, col_counts, t_last);
    const Options &opt = *in.opt;
    if (opt.phasing && job.world > 1 && vote) {
        // nothing collective has been touched yet: either every rank goes on, or none does
        if (!vote->vote(job.error.empty())) {
            if (job.error.empty()) job.error = "stopped: another rank failed before the exchange";
            return;
        }
    } else if (!job.error.empty()) {
        return;
    }
    if (!opt.phasing) return;
    auto lap = [&](const char *what) {
        const auto now = std::chrono::steady_clock::now();
        job.laps.emplace_back(what, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    };
    auto fail = [&](const char *what, jl_ctx *c) { job.error = std::string(what) + ": " + (c ? jl_last_error(c) : "failed"); };
    // The communicator's bootstrap is collective too: a rank that fails in it leaves the others to RCCL's own time-out.
    if (job.world > 1 && (job.inproc ? jl_comm_create_inproc(job.wins[0], comm_id, job.rank, job.world, &job.comm)
                                     : jl_comm_create(job.wins[0], comm_id, job.rank, job.world, &job.comm)) != JL_OK)
        return fail("communicator", job.wins[0]);
    std::vector<uint32_t> wb, wn;
    std::vector<int32_t> wr;
    for (const WindowPlan &wp : plan) { wb.push_back(wp.begin); wn.push_back(wp.ncols); wr.push_back(wp.rank); }
    jl_xwin *x = nullptr;
    if (jl_xwin_create(job.wins.data(), (uint32_t)job.wins.size(), job.comm, wb.data(), wn.data(), wr.data(), (uint32_t)plan.size(),
                       slice_begin.data(), &x) != JL_OK)
        return fail("cross-window session", nullptr);
    lap("communicator + session");
    jl_xwin_result r;
    if (jl_xwin_phase_sharded(x, opt.min_reads, &r) != JL_OK) {
        job.error = std::string("cross-window phasing: ") + jl_xwin_last_error(x);
        jl_xwin_destroy(x);
        return;
    }
    lap("cross-window phasing");
    Results &R = job.res;
    R.var.assign(r.merged, r.merged + r.n_variants);
    for (jl_variant &v : R.var) v.col -= in.win_begin;
    R.ps = r.summary;
    R.ps.n_positions = r.n_positions;
    R.ps.n_haplotypes = r.n_haplotypes;
    R.pos_cols.resize(r.n_positions);
    for (uint32_t p = 0; p < r.n_positions; ++p) R.pos_cols[p] = r.pos_global[p] - in.win_begin;
    if (r.n_positions) {
        R.hap_count.assign(r.hap_count, r.hap_count + r.n_haplotypes);
        R.hap_pattern.assign(r.hap_pattern, r.hap_pattern + (size_t)r.n_haplotypes * r.n_positions);
        R.hit.assign(r.hit, r.hit + (size_t)r.n_variants * r.n_haplotypes);
    }
    R.pat_stride = r.n_positions;
    R.hit_stride = r.n_haplotypes;
    job.slice_begin = r.slice_begin;
    job.slice_reads = r.slice_reads;
    job.ids.resize(r.slice_reads ? r.slice_reads : 1);
    if (jl_xwin_read_hap_fetch(x, job.ids.data()) != JL_OK) job.error = std::string("per-read ids: ") + jl_xwin_last_error(x);
    job.ids.resize(r.slice_reads);
    lap("per-read ids");
    jl_xwin_destroy(x);
    lap("session closed");
}

static void run_rank_local(RankJob &job, const DeviceStageInput &in, const std::vector<WindowPlan> &plan, std::vector<uint32_t> &col_counts,
                           std::chrono::steady_clock::time_point &t_last)
{
    auto fail = [&](const char *what, jl_ctx *c) { job.error = std::string(what) + ": " + (c ? jl_last_error(c) : "failed"); };
    auto lap = [&](const char *what) {
        const auto now = std::chrono::steady_clock::now();
        job.laps.emplace_back(what, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    };
    const Options &opt = *in.opt;
    const uint8_t *refp = in.refcodes->empty() ? nullptr : in.refcodes->data();
    for (uint32_t k : job.widx) {
        // a window's context orders its work on the stream of this rank's records context: a stream of its own is a hardware
        // queue the runtime takes 8 ms to create (tools_tuning/ctx_startup.cpp), eight windows 70 ms — and one rank drives its
        // windows one after the other anyway
        jl_ctx *w = nullptr;
        if (jl_ctx_create(job.device, jl_ctx_stream(job.records), &w) != JL_OK) return fail("context", nullptr);
        job.wins.push_back(w);
        if (jl_records_window(job.records, w, plan[k].ncols, plan[k].begin, opt.min_qv) != JL_OK) return fail("ingest", w);
    }
    lap("window contexts + device ingest");
    jl_records_drop(job.records);
    lap("records dropped");
    // the call stage of every window: enqueued one after the other on the windows' own streams (they overlap on the device)
    std::vector<std::vector<uint64_t>> masks(job.wins.size());
    for (size_t i = 0; i < job.wins.size(); ++i) {
        if (opt.drm_only && drm_masks_of(job.wins[i], in, masks[i])) return fail("pileup", job.wins[i]);
        if (jl_run_async(job.wins[i], in.genes->data(), (uint32_t)in.genes->size(), refp, (uint32_t)in.refcodes->size(), &in.prm,
                         opt.drm_only ? masks[i].data() : nullptr, 0, opt.min_reads, 0) != JL_OK)
            return fail("run", job.wins[i]);
    }
    lap("call stage enqueued");
    // column counts of the columns each window owns (the MSA context of the output, doc/JULIET.md:99-100)
    for (size_t i = 0; i < job.wins.size(); ++i) {
        const WindowPlan &wp = plan[job.widx[i]];
        std::vector<uint32_t> cc((size_t)wp.ncols * 6);
        if (jl_pileup_fetch(job.wins[i], cc.data(), nullptr, nullptr, nullptr, nullptr, nullptr) != JL_OK) return fail("pileup fetch", job.wins[i]);
        const uint32_t off = wp.own_begin - (wp.begin - in.win_begin);   // 0: a window starts where its own columns start
        std::copy(cc.begin() + (size_t)off * 6, cc.begin() + (size_t)(off + wp.own_end - wp.own_begin) * 6,
                  col_counts.begin() + (size_t)wp.own_begin * 6);
    }
    lap("column counts");
    if (!opt.phasing) {
        for (jl_ctx *w : job.wins) {
            std::vector<jl_variant> t(4096);
            uint32_t n = 0;
            if (jl_call_fetch(w, t.data(), 4096, &n) != JL_OK) return fail("call fetch", w);
            t.resize(n);
            job.tables.push_back(std::move(t));
        }
        return;
    }
}

// ---------------------------------------------------------------- one sample, step by step
// What `juliet in.bam out...` does to its file, cut into the steps that a batch (--batch) runs for each of its samples too:
// decode and upload, the sample's setup, the fetch of its results, its outputs.  Both paths call these, so a sample of a
// batch gets what a single run of the same file gets.

uint64_t file_bytes(const std::string &path)
{
    std::error_code ec;
    const uintmax_t n = std::filesystem::file_size(path, ec);
    return ec ? 0 : (uint64_t)n;
}

struct Decoded {
    ReadExtent ext;
    std::vector<BamRef> refs;
    std::string header_text;
};

// ONE pass over the file: records as decoded from BAM (cigar expansion, QV masking and the transpose run on the device) and
// the extent they cover.  With a device behind it (`uploader`): the pipelined reader — inflate and record parsing on every
// core, chunks to the uploader in file order; the GPU-free diagnostics and non-BGZF files take the sequential one (into `rec`).
Decoded decode_bam(const std::string &bam, const IngestOptions &io, RecordUploader *uploader, RecordArrays &rec)
{
    Decoded d;
    RecordSink sink;
    if (uploader) sink.give = [uploader](RecordArrays &c) { uploader->give(c); };
    const bool want_qual = io.min_qv > 0;
    d.ext = (uploader && PipelinedBamReader::is_bgzf(bam))
                ? PipelinedBamReader::run(bam, io, io.ref_id, want_qual, sink, &d.refs, &d.header_text)
                : collect_records(bam, io, io.ref_id, want_qual, rec, &d.refs, &d.header_text, uploader ? &sink : nullptr);
    return d;
}

// Everything a sample's device stage and outputs are derived from, besides its reads.
struct SampleSetup {
    TargetConfig cfg;                // the config, or the ORF "unknown" over the sample's reads
    uint32_t win_begin = 0, n_cols = 0;
    std::string chem;
    jl_params prm = {};
    std::vector<jl_gene> genes;
    std::vector<uint8_t> refcodes;
    const uint8_t *refp() const { return refcodes.empty() ? nullptr : refcodes.data(); }
};

// The genes and the window of one sample: 0, or 1 when --region leaves no gene of the config (message printed).
int sample_window(const Options &opt, const TargetConfig &config, const Decoded &d, SampleSetup &s)
{
    s.cfg = config;
    TargetConfig &cfg = s.cfg;
    int64_t ref_len = std::numeric_limits<int64_t>::max();
    if (d.ext.ref_id >= 0 && (size_t)d.ext.ref_id < d.refs.size()) ref_len = d.refs[(size_t)d.ext.ref_id].length;

    const bool have_cfg = !cfg.genes.empty();
    if (!have_cfg) {
        // no target config: one ORF over the covered window, labelled "unknown" (doc/JULIET.md:182-188);
        // --region marks the reading frame
        GeneCfg g;
        g.name = "unknown";
        g.begin = g.begin_eff = opt.have_region ? opt.region_b : (uint32_t)d.ext.min_pos + 1;
        g.end = g.end_eff = opt.have_region ? opt.region_e : (uint32_t)d.ext.max_end + 1;
        cfg.genes.push_back(g);
    } else if (opt.have_region) {
        cfg.apply_region(opt.region_b, opt.region_e);
        if (cfg.genes.empty()) { std::cerr << "juliet: --region leaves no gene of the config\n"; return 1; }
    }
    // window: the called genes plus the -3..+5 context columns (doc/JULIET.md:99-100), inside the reference
    int64_t gb = std::numeric_limits<int64_t>::max(), ge = 0;
    for (const GeneCfg &g : cfg.genes) { gb = std::min<int64_t>(gb, (int64_t)g.begin_eff - 1); ge = std::max<int64_t>(ge, (int64_t)g.end_eff - 1); }
    const int64_t wb = std::max<int64_t>(0, gb - 3);
    const int64_t we = std::max<int64_t>(wb + 1, std::min<int64_t>(ref_len, ge + 5));
    s.win_begin = (uint32_t)wb;
    s.n_cols = (uint32_t)(we - wb);
    return 0;
}

// Chemistry (from the sample's own @RG header with --chemistry auto), parameters, genes and reference codes of one sample.
void sample_params(const Options &opt, const Decoded &d, SampleSetup &s)
{
    std::string chem = opt.chemistry;
    if (chem == "auto") {
        // chemistry-keyed rates with a permissive fallback (doc/JULIET.md:221-225); the key here is the
        // platform model in the @RG line
        chem = (d.header_text.find("SEQUEL") != std::string::npos || d.header_text.find("S/P") != std::string::npos) ? "sequel" : "permissive";
        if (chem == "permissive") std::cerr << "juliet: chemistry not recognised, permissive mode is active (doc/JULIET.md:221-225)\n";
    }
    s.chem = chem;
    jl_params &prm = s.prm;
    prm.alpha = opt.alpha;
    prm.n_tests = opt.n_tests;
    if (chem == "sequel") prm.err = {0.998826, 5.8e-5, 1.0e-3};
    else prm.err = {0.99764, 1.2e-4, 2.0e-3};
    if (opt.match > 0) prm.err.match = opt.match;
    if (opt.substitution >= 0) prm.err.substitution = opt.substitution;
    prm.expected_round = opt.expected_round;
    prm.tail = opt.fisher_tail;
    prm.min_perc = opt.min_perc;
    prm.max_perc = opt.max_perc;

    s.genes.clear();
    for (const GeneCfg &g : s.cfg.genes) s.genes.push_back({g.begin_eff, g.end_eff});
    s.refcodes.clear();
    if (!s.cfg.reference_sequence.empty())
        for (char ch : s.cfg.reference_sequence) s.refcodes.push_back(base_code(ch));
}

using Tick = std::function<void(const char *)>;

// The variant table (unless `calls` is off: the pileup alone ran) and the column counts of the run last enqueued on `ctx`,
// whether it ran alone or in a group.  R.col_counts holds n_cols * 6 entries.  nullptr, or the step that failed.
const char *fetch_calls(jl_ctx *ctx, bool calls, Results &R, const Tick &tick)
{
    R.var.resize(4096);
    uint32_t nv = 0;
    if (calls && jl_call_fetch(ctx, R.var.data(), 4096, &nv) != JL_OK) return "call fetch";
    R.var.resize(nv);
    tick("  wait for the run + table");
    if (jl_pileup_fetch(ctx, R.col_counts.data(), nullptr, nullptr, nullptr, nullptr, nullptr) != JL_OK) return "pileup fetch";
    tick("  column counts");
    return nullptr;
}

// The haplotypes and the per-read ids of a phasing run, after fetch_calls.
const char *fetch_phase(jl_ctx *ctx, uint64_t n_reads, Results &R)
{
    const uint32_t cap_var = std::max<uint32_t>(1, (uint32_t)R.var.size());
    R.pos_cols.resize(cap_var);
    R.hap_count.resize(JL_MAX_HAPLOTYPES);
    R.hap_pattern.resize((size_t)JL_MAX_HAPLOTYPES * cap_var);
    R.hit.resize((size_t)cap_var * JL_MAX_HAPLOTYPES);
    R.read_hap.resize(n_reads);
    R.pat_stride = cap_var;
    R.hit_stride = JL_MAX_HAPLOTYPES;
    if (jl_phase_fetch(ctx, &R.ps, R.pos_cols.data(), R.hap_count.data(), R.hap_pattern.data(), R.hit.data(), R.read_hap.data(), nullptr, cap_var) != JL_OK)
        return "phase fetch";
    return nullptr;
}

// --rescue-damaged, after fetch_phase: one call of the rule of docs/SPEC.md §14 with the run's own positions and haplotypes.
const char *fetch_rescue(jl_ctx *ctx, uint32_t min_positions, Results &R)
{
    R.rescued = true;
    R.rescue_min = min_positions;
    R.rescue.clear();
    if (R.ps.n_haplotypes == 0 || min_positions > R.ps.n_positions) return nullptr;
    if (jl_phase_rescue_async(ctx, R.pos_cols.data(), R.ps.n_positions, R.hap_pattern.data(), (uint32_t)R.pat_stride, R.ps.n_haplotypes,
                              min_positions) != JL_OK)
        return "rescue";
    R.rescue.resize(R.read_hap.size());
    if (jl_phase_rescue_fetch(ctx, R.rescue.data(), nullptr, nullptr) != JL_OK) return "rescue fetch";
    return nullptr;
}

// --linkage, after fetch_calls: ONE call of docs/SPEC.md §15 with the table's distinct columns as positions and its rows as variants.
// No variant: no call.  More than JL_LINK_MAX variants or positions: a warning, no call, the block says "skipped".
const char *fetch_linkage(jl_ctx *ctx, Results &R)
{
    R.linked = true;
    R.link_skipped = false;
    const uint32_t V = (uint32_t)R.var.size();
    R.link_var.resize(V);
    for (uint32_t k = 0; k < V; ++k) R.link_var[k] = k;
    std::stable_sort(R.link_var.begin(), R.link_var.end(), [&](uint32_t a, uint32_t b) { return R.var[a].col < R.var[b].col; });
    R.link_cols.clear();
    R.link_var_pos.resize(V);
    std::vector<uint8_t> codon(V);
    for (uint32_t k = 0; k < V; ++k) {
        const jl_variant &f = R.var[R.link_var[k]];
        if (R.link_cols.empty() || R.link_cols.back() != f.col) R.link_cols.push_back(f.col);
        R.link_var_pos[k] = (uint32_t)R.link_cols.size() - 1u;
        codon[k] = f.codon;
    }
    if (V == 0) return nullptr;
    const uint32_t P = (uint32_t)R.link_cols.size();
    if (V > (uint32_t)JL_LINK_MAX || P > (uint32_t)JL_LINK_MAX) {
        std::cerr << "juliet: warning: --linkage takes at most " << (int)JL_LINK_MAX << " variants at " << (int)JL_LINK_MAX << " positions, the table has " << V
                  << " at " << P << ": no pair is tested (narrow the table with --min-perc / --max-perc / --region)\n";
        R.link_skipped = true;
        return nullptr;
    }
    if (jl_variant_linkage_async(ctx, R.link_cols.data(), P, R.link_var_pos.data(), codon.data(), V) != JL_OK) return "linkage";
    R.link_both.resize((size_t)P * P), R.link_carry.resize((size_t)V * P), R.link_joint.resize((size_t)V * V);
    if (jl_variant_linkage_fetch(ctx, R.link_both.data(), R.link_carry.data(), R.link_joint.data()) != JL_OK) return "linkage fetch";
    return nullptr;
}

// What --downsample / --mix did to a sample: the `sampling` block of the JSON's input section, present only when reads were chosen.
struct SamplingInfo {
    bool acted = false;
    uint64_t seed = 0;
    struct Source { std::string file; uint64_t reads, kept; };
    std::vector<Source> sources;
};

// --downsample on a window that is resident on `ctx` (its reads' names in `names`): when it holds more than opt.downsample reads,
// the reads of jl_sample_reads are gathered into `taken` — a second context of the device, on the same stream — and names / n_reads
// follow the indices.  JL_OK, or the status of the call that failed (jl_last_error(taken)); *acted: the window to run is `taken` now.
int downsample_window(const Options &opt, const std::string &bam, jl_ctx *ctx, jl_ctx *taken, std::vector<std::string> &names, uint64_t &n_reads,
                      SamplingInfo &info, bool *acted)
{
    *acted = false;
    if (!opt.have_downsample || n_reads <= opt.downsample) return JL_OK;
    std::vector<uint32_t> idx((size_t)opt.downsample);
    uint64_t kept = 0;
    if (const int rc = jl_sample_reads(n_reads, opt.downsample, opt.sample_seed, idx.data(), &kept)) return rc;
    const jl_take_part part = {ctx, idx.data(), kept};
    if (const int rc = jl_msa_take(taken, &part, 1)) return rc;
    std::vector<std::string> chosen((size_t)kept);
    for (uint64_t j = 0; j < kept; ++j) chosen[(size_t)j].swap(names[idx[(size_t)j]]);
    names.swap(chosen);
    info.acted = true;
    info.seed = opt.sample_seed;
    info.sources.assign(1, {bam, n_reads, kept});
    n_reads = kept;
    *acted = true;
    return JL_OK;
}

// --mix: the mixture of doc/MIXDATA.md in `taken`.  `major` holds the positional BAM's window; every BAM of the list is decoded and
// ingested into a context of its own over the same window (same device and stream), jl_mix_counts says how many reads each source
// gives, source m is sampled with seed S + m, and ONE jl_msa_take with the parts in argument order builds the mixture; names and
// n_reads become the mixture's.  0, or the process's exit status (message printed): 2 an input error, 3 a device error.
int mix_window(const Options &opt, const IngestOptions &io, jl_ctx *major, jl_ctx *taken, uint32_t n_cols, uint32_t win_begin,
               std::vector<std::string> &names, uint64_t &n_reads, SamplingInfo &info)
{
    const size_t n_src = opt.mix.size() + 1;
    std::vector<jl_ctx *> ctxs(1, major);
    std::vector<std::vector<std::string>> src_names(n_src);
    std::vector<uint64_t> reads(1, n_reads);
    src_names[0].swap(names);
    for (const std::string &file : opt.mix) {
        jl_ctx *c = nullptr;
        if (jl_ctx_create(opt.device, jl_ctx_stream(major), &c) != JL_OK) die_jl(nullptr, "context of a minor clone");
        std::promise<std::pair<int, jl_ctx *>> ready;
        ready.set_value(std::make_pair((int)JL_OK, c));
        RecordUploader up({ready.get_future().share()}, file_bytes(file), opt.min_qv > 0, io.qv_mask);
        RecordArrays rec;
        const Decoded d = decode_bam(file, io, &up, rec);
        if (up.finish() != JL_OK) die_jl(up.failed() ? up.failed() : c, "record upload");
        if (d.ext.n_reads == 0) { std::cerr << "juliet: no primary or supplementary alignments in " << file << "\n"; return 2; }
        if (up.n_reads != d.ext.n_reads) die_jl(nullptr, "record upload lost reads");
        if (jl_records_finish(c, n_cols, win_begin, opt.min_qv) != JL_OK) die_jl(c, "ingest");
        src_names[ctxs.size()].swap(up.names);
        ctxs.push_back(c);
        reads.push_back(d.ext.n_reads);
    }
    std::vector<uint64_t> counts(n_src);
    if (jl_mix_counts((uint32_t)n_src, opt.downsample, opt.mix_perc, counts.data()) != JL_OK) die_jl(nullptr, "mixture counts");
    for (size_t m = 0; m < n_src; ++m)
        if (reads[m] < counts[m]) {
            std::cerr << "juliet: --mix: " << (m ? opt.mix[m - 1] : opt.bam) << " has " << reads[m] << " reads, the mixture wants " << counts[m] << " of it\n";
            return 2;
        }
    std::vector<std::vector<uint32_t>> idx(n_src);
    std::vector<jl_take_part> parts(n_src);
    info.acted = true;
    info.seed = opt.sample_seed;
    info.sources.clear();
    for (size_t m = 0; m < n_src; ++m) {
        idx[m].resize((size_t)std::max<uint64_t>(counts[m], 1));
        uint64_t kept = 0;
        if (jl_sample_reads(reads[m], counts[m], opt.sample_seed + m, idx[m].data(), &kept) != JL_OK || kept != counts[m]) die_jl(nullptr, "sample of a clone");
        parts[m] = {ctxs[m], idx[m].data(), kept};
        info.sources.push_back({m ? opt.mix[m - 1] : opt.bam, reads[m], kept});
        for (uint64_t j = 0; j < kept; ++j) names.push_back(std::move(src_names[m][idx[m][(size_t)j]]));
    }
    if (jl_msa_take(taken, parts.data(), (uint32_t)n_src) != JL_OK) die_jl(taken, "mixture");
    n_reads = names.size();
    return 0;
}

// The JSON document of one sample (doc/JULIET.md:61-107, 207-211); the HTML output is its rendering.
Json build_json(const Options &opt, const SampleSetup &s, const std::string &bam, const std::string &cmdline,
                const std::vector<std::string> &names, uint64_t n_reads, const Results &R, const SamplingInfo *sampling = nullptr)
{
    const TargetConfig &cfg = s.cfg;
    const uint32_t win_begin = s.win_begin, n_cols = s.n_cols;
    const std::string &chem = s.chem;
    const std::vector<jl_variant> &var = R.var;
    const std::vector<uint32_t> &col_counts = R.col_counts;
    const jl_phase_summary &ps = R.ps;
    const std::vector<uint32_t> &pos_cols = R.pos_cols, &hap_count = R.hap_count;
    const std::vector<uint8_t> &hap_pattern = R.hap_pattern, &hit = R.hit;
    const std::vector<uint16_t> &read_hap = R.read_hap;

    Json root = Json::object();
    root.set("input", Json::object()
                          .set("timestamp", Json::of(iso_now()))
                          .set("input_file", Json::of(bam))
                          .set("command_line", Json::of(cmdline))
                          .set("juliet_version", Json::of(kVersion)));
    if (sampling && sampling->acted) {   // (only then: a run whose flags chose nothing writes what a run without them writes)
        Json srcs = Json::array();
        for (const SamplingInfo::Source &x : sampling->sources)
            srcs.push(Json::object().set("file", Json::of(x.file)).set("reads", Json::of((int64_t)x.reads)).set("kept", Json::of((int64_t)x.kept)));
        Json sj = Json::object();
        sj.set("seed", Json::of((int64_t)sampling->seed)).set("sources", std::move(srcs));
        root.obj.back().second.set("sampling", std::move(sj));
    }
    Json tc = cfg.echo();
    tc.set("n_reads", Json::of((int64_t)n_reads));
    tc.set("window_begin", Json::of(win_begin + 1)).set("window_end", Json::of(win_begin + n_cols + 1));
    tc.set("chemistry_model", Json::of(chem));
    root.set("target_config", tc);

    Json genes_json = Json::array();
    const uint32_t H = ps.n_haplotypes;
    for (size_t g = 0; g < cfg.genes.size(); ++g) {
        Json gj = Json::object();
        gj.set("name", Json::of(cfg.genes[g].name));
        Json vps = Json::array();
        size_t v = 0;
        while (v < var.size()) {
            if (var[v].gene != g) { ++v; continue; }
            size_t e = v;
            while (e < var.size() && var[e].gene == g && var[e].codon_pos == var[v].codon_pos) ++e;
            const jl_variant &f = var[v];
            Json vp = Json::object();
            vp.set("ref_codon", Json::of(codon_string(f.ref_codon)));
            vp.set("ref_amino_acid", Json::of(std::string(1, translate(f.ref_codon))));
            const uint32_t aa_pos = f.codon_pos + cfg.genes[g].first_codon;
            vp.set("ref_position", Json::of(aa_pos));
            vp.set("coverage", Json::of(f.coverage));
            // variant codons grouped by amino acid (position 223 with two rows)
            Json aas = Json::array();
            std::vector<char> order;
            for (size_t k = v; k < e; ++k) {
                const char aa = translate(var[k].codon);
                if (std::find(order.begin(), order.end(), aa) == order.end()) order.push_back(aa);
            }
            // amino acids in alphabetical order: juliet_abl-nohaplotype.png prints "A GCC" above "P CCA" at ABL1 223
            std::sort(order.begin(), order.end());
            for (char aa : order) {
                Json aj = Json::object();
                aj.set("amino_acid", Json::of(std::string(1, aa)));
                Json cods = Json::array();
                for (size_t k = v; k < e; ++k) {
                    if (translate(var[k].codon) != aa) continue;
                    Json cj = Json::object();
                    cj.set("codon", Json::of(codon_string(var[k].codon)));
                    cj.set("frequency", Json::of((double)var[k].count / (double)var[k].coverage));
                    cj.set("count", Json::of(var[k].count));
                    cj.set("expected", Json::of(var[k].expected));
                    cj.set("pValue", Json::of(var[k].p_value));
                    cj.set("log_pValue", Json::of(var[k].log_p));
                    cj.set("known_drm", Json::of(cfg.known_drms(g, aa_pos, aa)));
                    if (opt.phasing) {
                        Json hh = Json::array();
                        for (uint32_t h = 0; h < H; ++h) hh.push(Json::of(hit[(size_t)k * R.hit_stride + h] != 0));
                        cj.set("haplotype_hit", hh);  // doc/JULIET.md:207-209
                    }
                    cods.push(cj);
                }
                aj.set("variant_codons", cods);
                aas.push(aj);
            }
            vp.set("variant_amino_acids", aas);
            // MSA context: -3 .. +5 around the codon's first base (doc/JULIET.md:99-100)
            Json msa = Json::array();
            for (int rel = -3; rel <= 5; ++rel) {
                const int64_t c = (int64_t)f.col + rel;
                if (c < 0 || c >= (int64_t)n_cols) continue;
                const uint32_t *cc = &col_counts[(size_t)c * 6];
                Json mj = Json::object();
                mj.set("rel_pos", Json::of((int64_t)rel)).set("abs_pos", Json::of((int64_t)(win_begin + c + 1)));
                static const char *sym[6] = {"A", "C", "G", "T", "-", "N"};
                for (int s = 0; s < 6; ++s) mj.set(sym[s], Json::of(cc[s]));
                const size_t r = (size_t)win_begin + (size_t)c;
                if (r < cfg.reference_sequence.size()) mj.set("wt", Json::of(std::string(1, (char)std::toupper((unsigned char)cfg.reference_sequence[r]))));
                msa.push(mj);
            }
            vp.set("msa", msa);
            vps.push(vp);
            v = e;
        }
        gj.set("variant_positions", vps);
        genes_json.push(gj);
    }
    root.set("genes", genes_json);

    // Section 4, drug summaries: variants grouped by annotated drug (doc/JULIET.md:104-107)
    {
        std::vector<std::pair<std::string, Json>> by_drug;
        for (const jl_variant &f : var) {
            const GeneCfg &g = cfg.genes[f.gene];
            const uint32_t aa_pos = f.codon_pos + g.first_codon;
            const char aa = translate(f.codon);
            for (const Drm &d : g.drms) {
                bool hit_drm = false;
                for (const DrmPosition &dp : d.positions) hit_drm = hit_drm || dp.matches(aa_pos, aa);
                if (!hit_drm) continue;
                Json e = Json::object();
                e.set("gene", Json::of(g.name));
                e.set("mutation", Json::of(std::string(1, translate(f.ref_codon)) + std::to_string(aa_pos) + std::string(1, aa)));
                e.set("codon", Json::of(codon_string(f.codon)));
                e.set("frequency", Json::of((double)f.count / (double)f.coverage));
                auto it = std::find_if(by_drug.begin(), by_drug.end(), [&](const std::pair<std::string, Json> &kv) { return kv.first == d.name; });
                if (it == by_drug.end()) { by_drug.emplace_back(d.name, Json::array()); it = by_drug.end() - 1; }
                it->second.push(e);
            }
        }
        Json ds = Json::array();
        for (auto &kv : by_drug) ds.push(Json::object().set("drug", Json::of(kv.first)).set("variants", kv.second));
        root.set("drug_summaries", ds);
    }

    if (opt.phasing) {  // root `haplotype` block: counts and read names, same order as haplotype_hit (doc/JULIET.md:209-211)
        Json hb = Json::object();
        hb.set("reported_reads", Json::of(ps.reported_reads)).set("insufficient_coverage_reads", Json::of(ps.insufficient_reads));
        hb.set("damaged_reads", Json::of(ps.damaged_reads)).set("marginal_gaps", Json::of(ps.marginal_gap));
        hb.set("marginal_heteroduplexes", Json::of(ps.marginal_heteroduplex)).set("marginal_partial", Json::of(ps.marginal_partial));
        std::vector<std::vector<uint32_t>> members(H);
        for (uint64_t i = 0; i < n_reads; ++i)
            if (read_hap[i] < H) members[read_hap[i]].push_back((uint32_t)i);
        // --rescue-damaged: the damaged reads by what the rule of docs/SPEC.md §14 says of them
        std::vector<std::vector<uint32_t>> rescued_members(H);
        uint64_t rescue_cat[4] = {0, 0, 0, 0};   // assigned, ambiguous, incompatible, uninformative
        uint64_t with_rescued_total = 0;
        if (R.rescued && ps.n_positions) {   // (no variant position: nothing was phased, no read is damaged, §8)
            for (uint64_t i = 0; i < n_reads; ++i) {
                if (read_hap[i] != (uint16_t)JL_HAP_DAMAGED) continue;
                const uint32_t r = R.rescue.empty() ? (uint32_t)JL_RESCUE_UNINFORMATIVE : R.rescue[i];
                if (r < H) rescued_members[r].push_back((uint32_t)i), rescue_cat[0]++;
                else rescue_cat[r == (uint32_t)JL_RESCUE_AMBIGUOUS ? 1 : r == (uint32_t)JL_RESCUE_NONE ? 2 : 3]++;
            }
            for (uint32_t h = 0; h < H; ++h) with_rescued_total += (uint64_t)hap_count[h] + rescued_members[h].size();
        }
        Json hs = Json::array();
        for (uint32_t h = 0; h < H; ++h) {
            Json hj = Json::object();
            hj.set("name", Json::of(haplotype_name(h))).set("reads", Json::of(hap_count[h]));
            hj.set("frequency", Json::of(ps.reported_reads ? (double)hap_count[h] / (double)ps.reported_reads : 0.0));
            Json cods = Json::array();
            for (uint32_t p = 0; p < ps.n_positions; ++p) cods.push(Json::of(codon_string(hap_pattern[(size_t)h * R.pat_stride + p])));
            hj.set("codons", std::move(cods));
            Json rn = Json::array();      // (moved on, level by level: a copy of this list per level was most of the stage at a million reads)
            rn.arr.reserve(members[h].size());
            for (uint32_t i : members[h]) rn.push(Json::of(names[i]));
            hj.set("read_names", std::move(rn));
            if (R.rescued) {
                const uint64_t with = (uint64_t)hap_count[h] + rescued_members[h].size();
                hj.set("rescued_reads", Json::of((uint32_t)rescued_members[h].size()));
                Json rr = Json::array();
                rr.arr.reserve(rescued_members[h].size());
                for (uint32_t i : rescued_members[h]) rr.push(Json::of(names[i]));
                hj.set("rescued_read_names", std::move(rr));
                hj.set("frequency_with_rescued", Json::of(with_rescued_total ? (double)with / (double)with_rescued_total : 0.0));
            }
            hs.push(std::move(hj));
        }
        hb.set("haplotypes", std::move(hs));
        Json pc = Json::array();
        for (uint32_t p = 0; p < ps.n_positions; ++p) pc.push(Json::of(win_begin + pos_cols[p] + 1));
        hb.set("variant_positions_abs", std::move(pc));
        if (R.rescued)
            hb.set("rescue", Json::object()
                                 .set("min_positions", Json::of(R.rescue_min))
                                 .set("assigned_reads", Json::of((uint32_t)rescue_cat[0]))
                                 .set("ambiguous_reads", Json::of((uint32_t)rescue_cat[1]))
                                 .set("incompatible_reads", Json::of((uint32_t)rescue_cat[2]))
                                 .set("uninformative_reads", Json::of((uint32_t)rescue_cat[3])));
        root.set("haplotype", std::move(hb));
    }
    if (R.linked) {   // --linkage (docs/SPEC.md §15): one entry per pair of rows v < w at different positions that some read covers both of
        const uint32_t V = (uint32_t)var.size(), P = (uint32_t)R.link_cols.size();
        Json lb = Json::object();
        Json pc = Json::array();
        for (uint32_t c : R.link_cols) pc.push(Json::of(win_begin + c + 1));
        lb.set("variant_positions_abs", std::move(pc)).set("n_variants", Json::of(V));
        Json pairs = Json::array();
        if (!R.link_skipped && V) {
            std::vector<uint32_t> at(V);   // row of the table -> variant of the call
            for (uint32_t k = 0; k < V; ++k) at[R.link_var[k]] = k;
            auto side = [&](const jl_variant &f) {
                return Json::object().set("gene", Json::of(cfg.genes[f.gene].name)).set("ref_position", Json::of(f.codon_pos + cfg.genes[f.gene].first_codon))
                    .set("codon", Json::of(codon_string(f.codon)));
            };
            for (uint32_t v = 0; v < V; ++v)
                for (uint32_t w = v + 1; w < V; ++w) {
                    if (var[v].col == var[w].col) continue;
                    jl_link_pair lp;
                    if (jl_linkage_stats(R.link_both.data(), R.link_carry.data(), R.link_joint.data(), R.link_var_pos.data(), P, V, at[v], at[w], &lp) != JL_OK)
                        die_jl(nullptr, "linkage statistics");
                    if (lp.n == 0) continue;
                    pairs.push(Json::object().set("a", side(var[v])).set("b", side(var[w])).set("reads_both", Json::of(lp.n))
                                   .set("n11", Json::of(lp.n11)).set("n10", Json::of(lp.n10)).set("n01", Json::of(lp.n01)).set("n00", Json::of(lp.n00))
                                   .set("r2", Json::of(lp.r2)).set("d_prime", Json::of(lp.d_prime))
                                   .set("p_positive", Json::of(lp.p_positive)).set("p_negative", Json::of(lp.p_negative)));
                }
        }
        lb.set("n_pairs_tested", Json::of((uint32_t)pairs.arr.size())).set("pairs", std::move(pairs));
        if (R.link_skipped) lb.set("skipped", Json::of(true));
        root.set("linkage", std::move(lb));
    }
    return root;
}

// --haplotype-fasta (docs/SPEC.md §13): one record per reported haplotype, in the JSON's order, from ONE class pileup of the window
// resident on `ctx` with the phasing run's own per-read ids as labels.  No reported haplotype: an empty file.  0, or the exit code.
int write_haplotype_fasta(const Options &opt, jl_ctx *ctx, const Results &R, uint32_t win_begin, uint32_t n_cols)
{
    const uint32_t H = R.ps.n_haplotypes;
    std::vector<uint32_t> counts((size_t)H * n_cols * 6);
    std::vector<uint32_t> rescued(H, 0u);
    if (H) {
        std::vector<uint16_t> with_rescued;   // --rescue-damaged: the damaged reads count for the haplotype they were assigned to
        if (R.rescued) {
            with_rescued.resize(R.read_hap.size());
            for (size_t i = 0; i < with_rescued.size(); ++i) {
                with_rescued[i] = R.hap_with_rescued(i);
                if (with_rescued[i] != R.read_hap[i]) rescued[with_rescued[i]]++;
            }
        }
        if (jl_class_pileup_async(ctx, R.rescued ? with_rescued.data() : R.read_hap.data(), H) != JL_OK) die_jl(ctx, "class pileup");
        if (jl_class_pileup_fetch(ctx, counts.data(), nullptr) != JL_OK) die_jl(ctx, "class pileup fetch");
    }
    std::ofstream f(opt.hap_fasta);
    if (!f) { std::cerr << "juliet: cannot write " << opt.hap_fasta << "\n"; return 2; }
    std::vector<uint8_t> cons(n_cols);
    for (uint32_t h = 0; h < H; ++h) {
        if (jl_consensus_of_counts(counts.data() + (size_t)h * n_cols * 6, n_cols, cons.data()) != JL_OK) die_jl(nullptr, "consensus of counts");
        std::string freq, seq;
        Json::of(R.ps.reported_reads ? (double)R.hap_count[h] / (double)R.ps.reported_reads : 0.0).write(freq);
        for (uint32_t c = 0; c < n_cols; ++c)
            if (cons[c] != 4) seq += "ACGT?N"[cons[c]];   // (4: a major deletion, the column is removed)
        f << ">" << haplotype_name(h) << " reads=" << R.hap_count[h] << (R.rescued ? " rescued=" + std::to_string(rescued[h]) : std::string())
          << " frequency=" << freq << " window=" << (win_begin + 1) << "-"
          << (win_begin + n_cols) << " source=" << opt.bam << "\n";
        for (size_t i = 0; i < seq.size(); i += 70) f << seq.substr(i, 70) << "\n";
    }
    f.close();
    if (!f) { std::cerr << "juliet: cannot write " << opt.hap_fasta << "\n"; return 2; }
    return 0;
}

// Every output of one run — the JSON text, or its HTML rendering, by extension — each file closed and its stream checked:
// a short write or a full disk is a failed output, not a quiet success.  "" or the first output that failed.
std::string write_outputs(const std::vector<std::string> &outputs, const Json &root)
{
    std::string text;
    root.write(text);
    text += "\n";
    for (const std::string &out : outputs) {
        std::ofstream f(out);
        if (!f) return out;
        if (out.substr(out.size() - 5) == ".json") f << text;
        else f << render_html(root);
        f.close();
        if (!f) return out;
    }
    return "";
}

// ---------------------------------------------------------------- --batch: many samples in one process
// One device and ONE pool of contexts, made once and refilled sample after sample (jl_records_begin drops what a context held
// before), so the runtime start and the contexts are paid once per list instead of once per file.  A decoding thread takes the
// list in order: decode + upload into a free context of the pool (the first context comes up while the first file decodes, as
// in a single run), the sample's setup, the device ingest, the --drm-only masks; the sample is then READY.  The main thread
// runs the ready samples: those that share a group key (genes, reference codes, parameters, window, drm masks or none) up to
// eight at a time through one group run (one launch per stage for all of them), any other alone (jl_run_async); a group that
// refuses its windows (pileup chunk widths, a window that needs the two- or multi-word phasing pipeline) runs them alone too.
// Each sample's results are fetched with the calls of a single run, its context goes back to the pool and its outputs are
// written while the next samples decode.  The pool bounds what is resident: at most kPool samples, whatever the list's length.
class BatchRunner {
public:
    BatchRunner(const Options &opt, const TargetConfig &cfg, const std::string &cmdline) : opt_(opt), cfg_(cfg), cmdline_(cmdline) {}

    int run()
    {
        const auto t_start = std::chrono::steady_clock::now();
        const size_t n_pool = std::min<size_t>(kPool, opt_.batch_lines.size());
        const int dev = opt_.device;
        first_ = std::async(std::launch::async, [dev]() {
                     jl_ctx *c = nullptr;
                     const int rc = jl_ctx_create(dev, nullptr, &c);
                     return std::make_pair(rc, c);
                 }).share();
        std::thread creator([this, n_pool] { create_pool(n_pool); });
        std::thread producer([this] { produce(); });
        for (;;) {
            std::vector<std::unique_ptr<Sample>> take;
            {
                // what is ready runs once a whole group is, or when nothing more comes soon: the list is through, or the decoding
                // thread waits for a context that only this thread can give back (the whole pool exists and is taken)
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] {
                    return ready_.size() >= kGroupMax || producer_done_ || (producer_waiting_ && created_ + 1 >= n_pool && !ready_.empty());
                });
                if (ready_.empty() && producer_done_) break;
                while (!ready_.empty()) {
                    take.push_back(std::move(ready_.front()));
                    ready_.pop_front();
                }
            }
            dispatch(take);
        }
        producer.join();
        creator.join();
        const unsigned failed = n_failed_.load();
        if (opt_.timing)
            fprintf(stderr, "juliet: timing batch total  %zu samples  %u failed  %.1f ms\n", opt_.batch_lines.size(), failed,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count());
        // every output is written, closed and checked: the same fast end as a single run (JL_SLOW_EXIT=1: the long way)
        if (!getenv("JL_SLOW_EXIT")) {
            std::cout.flush();
            std::cerr.flush();
            fflush(nullptr);
            _exit(failed ? 2 : 0);
        }
        for (auto &g : groups_) jl_group_destroy(g.second);
        for (auto &t : taken_) jl_ctx_destroy(t.second);
        for (jl_ctx *c : pool_) jl_ctx_destroy(c);
        return failed ? 2 : 0;
    }

private:
    static constexpr size_t kPool = 16;       // contexts, i.e. samples resident at once
    static constexpr size_t kGroupMax = 8;    // samples per group run (one launch per stage for the eight)
    static constexpr size_t kGroupCache = 16;

    struct Sample {
        const Options::BatchLine *line = nullptr;
        jl_ctx *ctx = nullptr;       // of the pool: the sample's records and its window as ingested
        jl_ctx *run = nullptr;       // the window that is called: ctx, or — downsampled — the pool context's companion (taken_)
        SamplingInfo sampling;
        SampleSetup s;
        std::vector<std::string> names;
        uint64_t n_reads = 0;
        bool drm_only = false;
        std::vector<uint64_t> drm_masks;
        Results R;
        // what the run gets, as in a single run (empty masks — no evaluated position — are none)
        const uint64_t *masks() const { return drm_only ? drm_masks.data() : nullptr; }
    };

    // A GPU error is no failure of one sample: the batch stops here and writes nothing more (an output being written is finished
    // first, so that none is left half written).
    [[noreturn]] void gpu_error(const std::string &what)
    {
        std::lock_guard<std::mutex> lk(io_m_);
        std::cerr << "juliet: batch stopped by a GPU error: " << what << "\n";
        std::cerr.flush();
        fflush(nullptr);
        _exit(3);
    }
    void sample_failed(const Options::BatchLine &l, const std::string &why)
    {
        const std::string msg = "juliet: batch line " + std::to_string(l.line) + " (" + l.bam + "): " + why + "\n";
        fputs(msg.c_str(), stderr);
        ++n_failed_;
    }

    // ---- the pool
    void create_pool(size_t n)   // contexts 1 .. n-1, once the first is up (the runtime starts once)
    {
        if (first_.get().first != JL_OK) return;   // (the decoding thread reports it)
        for (size_t k = 1; k < n; ++k) {
            jl_ctx *c = nullptr;
            if (jl_ctx_create(opt_.device, nullptr, &c) != JL_OK) gpu_error(std::string("context: ") + jl_last_error(c));
            {
                std::lock_guard<std::mutex> lk(m_);
                pool_.push_back(c);
                free_.push_back(c);
                ++created_;
            }
            cv_.notify_all();
        }
    }
    jl_ctx *acquire()
    {
        std::unique_lock<std::mutex> lk(m_);
        producer_waiting_ = true;
        cv_.notify_all();
        cv_.wait(lk, [&] { return !free_.empty(); });
        producer_waiting_ = false;
        jl_ctx *c = free_.front();
        free_.pop_front();
        return c;
    }
    void release(jl_ctx *c)
    {
        {
            std::lock_guard<std::mutex> lk(m_);
            free_.push_back(c);
        }
        cv_.notify_all();
    }

    // ---- the decoding thread
    void produce()
    {
        for (size_t i = 0; i < opt_.batch_lines.size(); ++i) {
            std::unique_ptr<Sample> smp(new Sample);
            smp->line = &opt_.batch_lines[i];
            smp->drm_only = opt_.drm_only;
            std::shared_future<std::pair<int, jl_ctx *>> up;
            if (i == 0) {
                up = first_;
            } else {
                std::promise<std::pair<int, jl_ctx *>> p;
                p.set_value(std::make_pair((int)JL_OK, acquire()));
                up = p.get_future().share();
            }
            const std::string why = prepare(*smp, up);
            if (!smp->ctx) smp->ctx = context_of(up);   // (a sample that failed before it asked for its context)
            if (i == 0) {
                std::lock_guard<std::mutex> lk(m_);
                pool_.push_back(smp->ctx);
            }
            if (!why.empty()) {
                sample_failed(*smp->line, why);
                release(smp->ctx);
                continue;
            }
            {
                std::lock_guard<std::mutex> lk(m_);
                ready_.push_back(std::move(smp));
            }
            cv_.notify_all();
        }
        {
            std::lock_guard<std::mutex> lk(m_);
            producer_done_ = true;
        }
        cv_.notify_all();
    }
    // The context a pool context's downsampled window goes into: same device, same stream, made when first needed and kept.
    jl_ctx *companion_of(jl_ctx *c)   // (decoding thread only)
    {
        jl_ctx *&t = taken_[c];
        if (!t && jl_ctx_create(opt_.device, jl_ctx_stream(c), &t) != JL_OK) gpu_error("context of a downsampled window");
        return t;
    }
    jl_ctx *context_of(const std::shared_future<std::pair<int, jl_ctx *>> &up)
    {
        const auto r = up.get();
        if (r.first != JL_OK) gpu_error("no usable GPU (this tool has no CPU fallback)");
        return r.second;
    }
    // Decode + upload, setup, device ingest and masks of one sample: "" (ready), or why the sample failed.
    std::string prepare(Sample &smp, const std::shared_future<std::pair<int, jl_ctx *>> &up)
    {
        const auto t0 = std::chrono::steady_clock::now();
        const Options::BatchLine &l = *smp.line;
        IngestOptions io;
        io.min_qv = opt_.min_qv;
        io.min_rq = opt_.min_rq;
        io.qv_mask = opt_.qv_upload_mask;
        std::unique_ptr<RecordUploader> uploader(new RecordUploader({up}, file_bytes(l.bam), opt_.min_qv > 0, io.qv_mask));
        Decoded dec;
        try {
            RecordArrays rec;
            dec = decode_bam(l.bam, io, uploader.get(), rec);
        } catch (const std::exception &e) {
            return e.what();
        }
        smp.ctx = context_of(up);
        if (const int rc = uploader->finish()) {
            jl_ctx *c = uploader->failed() ? uploader->failed() : smp.ctx;
            if (rc == JL_ERR_ARG) return std::string("record upload: ") + jl_last_error(c);   // (the records, not the device)
            gpu_error(std::string("record upload: ") + jl_last_error(c));
        }
        if (dec.ext.n_reads == 0) return "no primary or supplementary alignments";
        if (uploader->n_reads != dec.ext.n_reads) gpu_error("record upload lost reads");
        smp.names.swap(uploader->names);
        uploader.reset();   // (its threads and its gathered arrays)
        smp.n_reads = dec.ext.n_reads;
        if (sample_window(opt_, cfg_, dec, smp.s)) return "--region leaves no gene of the config";
        sample_params(opt_, dec, smp.s);
        const int rc = jl_records_finish(smp.ctx, smp.s.n_cols, smp.s.win_begin, opt_.min_qv);
        if (rc == JL_ERR_ARG || rc == JL_ERR_STATE) return std::string("ingest: ") + jl_last_error(smp.ctx);   // (a malformed record)
        if (rc != JL_OK) gpu_error(std::string("ingest: ") + jl_last_error(smp.ctx));
        smp.run = smp.ctx;
        if (opt_.have_downsample && smp.n_reads > opt_.downsample) {   // (every sample of the list goes to the same depth)
            jl_ctx *taken = companion_of(smp.ctx);
            bool acted = false;
            if (downsample_window(opt_, l.bam, smp.ctx, taken, smp.names, smp.n_reads, smp.sampling, &acted) != JL_OK)
                gpu_error(std::string("downsample: ") + jl_last_error(taken));
            if (acted) smp.run = taken;
        }
        if (opt_.drm_only) {
            const DeviceStageInput in{&opt_, &smp.s.cfg, &smp.s.genes, &smp.s.refcodes, smp.s.prm, smp.s.win_begin, smp.s.n_cols, smp.n_reads};
            if (drm_masks_of(smp.run, in, smp.drm_masks)) gpu_error(std::string("pileup: ") + jl_last_error(smp.run));
        }
        if (opt_.timing)
            fprintf(stderr, "juliet: timing batch decode  line %u  %llu reads  %.1f ms\n", l.line, (unsigned long long)smp.n_reads,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        return "";
    }

    // ---- the device stage, on the main thread
    static bool same_key(const Sample &a, const Sample &b)
    {
        const SampleSetup &x = a.s, &y = b.s;
        if (x.win_begin != y.win_begin || x.n_cols != y.n_cols || x.genes.size() != y.genes.size() || x.refcodes != y.refcodes ||
            (a.masks() == nullptr) != (b.masks() == nullptr))
            return false;
        for (size_t g = 0; g < x.genes.size(); ++g)
            if (x.genes[g].begin != y.genes[g].begin || x.genes[g].end != y.genes[g].end) return false;
        return memcmp(&x.prm, &y.prm, sizeof(jl_params)) == 0;
    }
    void dispatch(std::vector<std::unique_ptr<Sample>> &take)
    {
        std::vector<std::vector<Sample *>> classes;   // samples of one group key, in list order
        for (auto &p : take) {
            auto it = std::find_if(classes.begin(), classes.end(), [&](const std::vector<Sample *> &c) { return same_key(*c[0], *p); });
            if (it == classes.end()) classes.push_back({p.get()});
            else it->push_back(p.get());
        }
        for (const std::vector<Sample *> &c : classes)
            for (size_t o = 0; o < c.size(); o += kGroupMax)
                run_chunk(std::vector<Sample *>(c.begin() + (ptrdiff_t)o, c.begin() + (ptrdiff_t)std::min(c.size(), o + kGroupMax)));
        for (auto &p : take) write(*p);
        take.clear();
    }
    void run_chunk(std::vector<Sample *> chunk)
    {
        auto t0 = std::chrono::steady_clock::now();
        if (chunk.size() >= 2) {
            // the contexts in one order whatever the samples' order: a group of the same contexts is used again
            std::sort(chunk.begin(), chunk.end(), [](const Sample *a, const Sample *b) { return std::less<jl_ctx *>()(a->run, b->run); });
            jl_group *g = group_of(chunk);
            const SampleSetup &s = chunk[0]->s;
            std::vector<const uint64_t *> masks;
            for (const Sample *x : chunk) masks.push_back(x->masks());
            const int rc = jl_group_run_masked_async(g, s.genes.data(), (uint32_t)s.genes.size(), s.refp(), (uint32_t)s.refcodes.size(), &s.prm,
                                                     masks.data(), opt_.phasing, opt_.min_reads, opt_.phasing);
            if (rc == JL_OK) {
                for (const Sample *x : chunk) last_group_[x->run] = g;
                fetch(chunk);
                timing_line("group ", chunk, t0);
                return;
            }
            // JL_ERR_ARG: the group refuses these windows together; each runs alone (a refusal never fails a sample)
            if (rc != JL_ERR_ARG) gpu_error(std::string("group run: ") + jl_group_last_error(g));
            if (opt_.timing) fprintf(stderr, "juliet: timing batch refused  %zu samples: %s\n", chunk.size(), jl_group_last_error(g));
        }
        for (Sample *x : chunk) {
            if (x != chunk[0]) t0 = std::chrono::steady_clock::now();
            const SampleSetup &s = x->s;
            if (jl_run_async(x->run, s.genes.data(), (uint32_t)s.genes.size(), s.refp(), (uint32_t)s.refcodes.size(), &s.prm, x->masks(),
                             opt_.phasing, opt_.min_reads, opt_.phasing) != JL_OK)
                gpu_error(std::string("run: ") + jl_last_error(x->run));
            last_group_[x->run] = nullptr;
            fetch({x});
            timing_line("single", {x}, t0);
        }
    }
    // the results of each sample with the fetch calls of a single run; then its context goes back to the pool
    void fetch(const std::vector<Sample *> &chunk)
    {
        const Tick quiet = [](const char *) {};
        for (Sample *x : chunk) {
            x->R.col_counts.assign((size_t)x->s.n_cols * 6, 0);
            const char *what = fetch_calls(x->run, true, x->R, quiet);
            if (!what && opt_.phasing) what = fetch_phase(x->run, x->n_reads, x->R);
            if (!what && jl_sync(x->run) != JL_OK) what = "sync";   // (the group's stream too: nothing of the run is left on the device)
            if (what) gpu_error(std::string(what) + ": " + jl_last_error(x->run));
            release(x->ctx);
        }
    }
    void timing_line(const char *kind, const std::vector<Sample *> &chunk, std::chrono::steady_clock::time_point t0)
    {
        if (!opt_.timing) return;
        std::string lines;
        for (const Sample *x : chunk) lines += (lines.empty() ? "" : ",") + std::to_string(x->line->line);
        fprintf(stderr, "juliet: timing batch %s %2zu samples  lines %s  run + fetch %.2f ms\n", kind, chunk.size(), lines.c_str(),
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    // A group of exactly these contexts, made once and kept.  When the cache is full, one goes that is no context's last group
    // run (a context's next run waits for the stream of its last group run, which must still exist).
    jl_group *group_of(const std::vector<Sample *> &chunk)
    {
        std::vector<jl_ctx *> ctxs;
        for (const Sample *x : chunk) ctxs.push_back(x->run);
        for (auto &e : groups_)
            if (e.first == ctxs) return e.second;
        if (groups_.size() >= kGroupCache)
            for (auto it = groups_.begin(); it != groups_.end(); ++it) {
                bool in_use = false;
                for (const auto &lg : last_group_) in_use = in_use || lg.second == it->second;
                if (in_use) continue;
                jl_group_destroy(it->second);
                groups_.erase(it);
                break;
            }
        jl_group *g = nullptr;
        if (jl_group_create(ctxs.data(), (uint32_t)ctxs.size(), &g) != JL_OK) gpu_error("cannot create a group of " + std::to_string(ctxs.size()) + " contexts");
        groups_.emplace_back(ctxs, g);
        return g;
    }
    void write(Sample &x)
    {
        try {
            const Json root = build_json(opt_, x.s, x.line->bam, cmdline_, x.names, x.n_reads, x.R, &x.sampling);
            std::lock_guard<std::mutex> lk(io_m_);
            const std::string failed = write_outputs(x.line->outputs, root);
            if (!failed.empty()) sample_failed(*x.line, "cannot write " + failed);
        } catch (const std::exception &e) {
            sample_failed(*x.line, e.what());
        }
    }

    const Options &opt_;
    const TargetConfig &cfg_;
    const std::string &cmdline_;
    std::shared_future<std::pair<int, jl_ctx *>> first_;
    std::mutex m_, io_m_;
    std::condition_variable cv_;
    std::vector<jl_ctx *> pool_;           // every context of the pool
    std::deque<jl_ctx *> free_;
    size_t created_ = 0;                   // contexts the pool thread made (the first is not counted)
    bool producer_waiting_ = false, producer_done_ = false;
    std::deque<std::unique_ptr<Sample>> ready_;
    std::atomic<unsigned> n_failed_{0};
    std::vector<std::pair<std::vector<jl_ctx *>, jl_group *>> groups_;   // main thread only
    std::map<jl_ctx *, jl_group *> last_group_;                          // main thread only
    std::map<jl_ctx *, jl_ctx *> taken_;                                 // decoding thread only: pool context -> its companion
};

int run_batch(const Options &opt, const TargetConfig &cfg, const std::string &cmdline)
{
    BatchRunner b(opt, cfg, cmdline);
    return b.run();
}

}  // namespace

int main(int argc, char **argv)
{
    // eight hardware queues instead of the runtime's four (the rank threads' streams beside the exchange): read by the HIP
    // runtime at the process's first HIP call, so set here, before any thread exists and before that call
    setenv("GPU_MAX_HW_QUEUES", "8", 0);
    Options opt;
    std::string cmdline;
    for (int i = 0; i < argc; ++i) cmdline += (i ? " " : "") + std::string(argv[i]);
    try {
        opt = parse(argc, argv);
        const auto t_start = std::chrono::steady_clock::now();
        auto t_last = t_start;
        const Tick tick = [&](const char *what) {
            if (!opt.timing) return;
            const auto now = std::chrono::steady_clock::now();
            fprintf(stderr, "juliet: timing %-26s %9.1f ms  (at %9.1f ms)\n", what,
                    std::chrono::duration<double, std::milli>(now - t_last).count(),
                    std::chrono::duration<double, std::milli>(now - t_start).count());
            t_last = now;
        };
        // ---------------------------------------------------------------- target config
        TargetConfig cfg;
        if (!opt.config.empty()) cfg = TargetConfig::load(opt.config);
        if (!opt.batch.empty()) return run_batch(opt, cfg, cmdline);
        if (!opt.dump_config.empty() && opt.bam.empty()) {
            if (opt.have_region) cfg.apply_region(opt.region_b, opt.region_e);
            Json j = cfg.echo();
            Json eff = Json::array();
            for (const GeneCfg &g : cfg.genes)
                eff.push(Json::object().set("name", Json::of(g.name)).set("begin", Json::of(g.begin_eff)).set("end", Json::of(g.end_eff)).set("first_codon", Json::of(g.first_codon)));
            j.set("effective_genes", eff);
            std::string s;
            j.write(s);
            std::ofstream(opt.dump_config) << s << "\n";
            return 0;
        }
        // ---------------------------------------------------------------- ingest
        IngestOptions io;
        io.min_qv = opt.min_qv;
        io.min_rq = opt.min_rq;
        io.qv_mask = opt.qv_upload_mask;
        // the GPU context comes up (runtime start, stream, pinned blocks) while the host reads the BAM
        const bool need_gpu = !opt.outputs.empty() || opt.fuse_only;
        std::vector<std::shared_future<std::pair<int, jl_ctx *>>> ctx_ups;
        std::unique_ptr<RecordUploader> uploader;
        if (need_gpu) {
            for (int dev : opt.devices)
                ctx_ups.push_back(std::async(std::launch::async, [dev]() {
                    jl_ctx *c = nullptr;
                    const int rc = jl_ctx_create(dev, nullptr, &c);
                    return std::make_pair(rc, c);
                }).share());
            uploader.reset(new RecordUploader(ctx_ups, file_bytes(opt.bam), opt.min_qv > 0, io.qv_mask));
        }
        RecordArrays rec;
        const Decoded dec = decode_bam(opt.bam, io, uploader.get(), rec);
        const ReadExtent &ext = dec.ext;
        tick("bam decode");
        if (ext.n_reads == 0) { std::cerr << "juliet: no primary or supplementary alignments in " << opt.bam << "\n"; return 2; }

        SampleSetup smp;
        if (sample_window(opt, cfg, dec, smp)) return 1;
        const uint32_t win_begin = smp.win_begin, n_cols = smp.n_cols;

        std::vector<std::string> names;
        uint64_t n_reads = 0;
        if (!opt.dump_msa.empty()) {  // host-side ingest check, no GPU involved
            std::vector<uint8_t> rows;
            n_reads = build_rows(opt.bam, io, ext.ref_id, win_begin, n_cols, ext.n_reads, rows, nullptr);
            std::ofstream f(opt.dump_msa, std::ios::binary);
            const uint64_t hdr[3] = {n_reads, n_cols, win_begin};
            f.write((const char *)hdr, sizeof hdr);
            f.write((const char *)rows.data(), (std::streamsize)((size_t)n_reads * n_cols));
            if (opt.outputs.empty()) return 0;
        }
        n_reads = ext.n_reads;

        // ---------------------------------------------------------------- parameters
        sample_params(opt, dec, smp);
        const std::vector<jl_gene> &genes = smp.genes;
        const std::vector<uint8_t> &refcodes = smp.refcodes;

        // ---------------------------------------------------------------- device
        jl_ctx *ctx = nullptr;
        for (auto &f : ctx_ups) {
            const auto up = f.get();
            if (up.first != JL_OK) die_jl(nullptr, "no usable GPU (this tool has no CPU fallback)");
            if (!ctx) ctx = up.second;
        }
        tick("context ready");
        if (uploader->finish() != JL_OK) die_jl(uploader->failed() ? uploader->failed() : ctx, "record upload");
        if (uploader->n_reads != n_reads) die_jl(nullptr, "record upload lost reads");
        names.swap(uploader->names);
        tick("rest of the upload");
        if (opt.timing)
            fprintf(stderr, "juliet: timing   uploader thread: gather %.1f ms, begin %.1f ms, %u appends %.1f ms (longest %.1f), names %.1f ms\n",
                    uploader->ms_gather, uploader->ms_begin, uploader->n_appends, uploader->ms_append, uploader->ms_append_max, uploader->ms_names);
        const uint8_t *refp = smp.refp();
        Results R;
        SamplingInfo sampling;
        R.col_counts.assign((size_t)n_cols * 6, 0);
        DeviceStageInput in{&opt, &smp.cfg, &genes, &refcodes, smp.prm, win_begin, n_cols, n_reads};
        const size_t n_ranks = opt.devices.size();
        if (opt.windows > 1 || n_ranks > 1) {
            // ---- K column windows over R devices (doc/JULIET.md:261-264: each gene is treated separately, so the split
            // never shows): one rank (thread) per device; the Bonferroni factor counts the codons of ALL genes in every window
            const uint32_t K = std::min<uint32_t>(opt.windows, std::max<uint32_t>(1, n_cols / 8));
            if (K < n_ranks) { std::cerr << "juliet: the window is too narrow for " << n_ranks << " devices\n"; return 1; }
            const std::vector<WindowPlan> plan = plan_windows(win_begin, n_cols, K, (uint32_t)n_ranks);
            // read slices for phasing: starts on multiples of 256 reads (a 128-byte line of every column)
            std::vector<uint64_t> slices(n_ranks + 1, n_reads);
            {
                uint64_t per = (n_reads + n_ranks - 1) / n_ranks;
                per = (per + 255) / 256 * 256;
                for (size_t r = 0; r < n_ranks; ++r) slices[r] = std::min<uint64_t>(n_reads, r * per);
            }
            uint8_t comm_id[128] = {0};
            if (opt.phasing && n_ranks > 1 && jl_comm_unique_id(comm_id) != JL_OK) die_jl(nullptr, "communicator id");
            // RCCL refuses two ranks on one device; ranks that are threads of one process can exchange by device copies
            bool inproc = opt.exchange == "inproc";
            if (opt.exchange.empty())
                for (size_t a = 0; a < n_ranks; ++a)
                    for (size_t b = a + 1; b < n_ranks; ++b) inproc = inproc || opt.devices[a] == opt.devices[b];
            {   // distinct devices: the exchanges between them (RCCL, or peer copies in process) have never run on hardware
                bool distinct = false;
                for (size_t a = 0; a < n_ranks; ++a)
                    for (size_t b = a + 1; b < n_ranks; ++b) distinct = distinct || opt.devices[a] != opt.devices[b];
                if (distinct)
                    fprintf(stderr, "juliet: warning: --devices with more than one distinct device is experimental: the exchange between devices is "
                                    "covered by one-device tests only (in-process ranks, one-rank RCCL)\n");
            }
            std::vector<RankJob> jobs(n_ranks);
            for (size_t r = 0; r < n_ranks; ++r) {
                jobs[r].inproc = inproc;
                jobs[r].rank = (int)r;
                jobs[r].world = (int)n_ranks;
                jobs[r].device = opt.devices[r];
                jobs[r].records = uploader->ctx(r);
                for (uint32_t k = 0; k < K; ++k)
                    if (plan[k].rank == (int)r) jobs[r].widx.push_back(k);
            }
            RankVote vote((int)n_ranks);
            std::vector<std::thread> threads;
            for (size_t r = 1; r < n_ranks; ++r)
                threads.emplace_back([&, r] { run_rank(jobs[r], in, plan, comm_id, R.col_counts, slices, &vote); });
            run_rank(jobs[0], in, plan, comm_id, R.col_counts, slices, &vote);
            for (std::thread &t : threads) t.join();
            for (const RankJob &j : jobs)
                if (!j.error.empty()) { std::cerr << "juliet: rank " << j.rank << " (device " << j.device << "): " << j.error << "\n"; return 3; }
            tick("windows: ingest + call + phase");
            if (opt.timing)
                for (const auto &l : jobs[0].laps) fprintf(stderr, "juliet: timing   rank 0: %-34s %6.1f ms\n", l.first, l.second);
            std::vector<uint32_t> cc;
            cc.swap(R.col_counts);
            if (opt.phasing) {
                R = std::move(jobs[0].res);
                R.read_hap.assign(n_reads, (uint16_t)JL_HAP_DAMAGED);
                for (const RankJob &j : jobs) std::copy(j.ids.begin(), j.ids.end(), R.read_hap.begin() + (ptrdiff_t)j.slice_begin);
            } else {
                std::vector<const jl_variant *> tabs;
                std::vector<uint32_t> cnt, begins;
                for (const RankJob &j : jobs)
                    for (size_t i = 0; i < j.tables.size(); ++i) {
                        tabs.push_back(j.tables[i].data());
                        cnt.push_back((uint32_t)j.tables[i].size());
                        begins.push_back(plan[j.widx[i]].begin - win_begin);
                    }
                uint64_t total = 0;
                for (uint32_t c : cnt) total += c;
                R.var.resize(total ? total : 1);
                uint32_t n = 0;
                if (jl_merge_tables(tabs.data(), cnt.data(), begins.data(), (uint32_t)tabs.size(), R.var.data(), (uint32_t)R.var.size(), &n) != JL_OK)
                    die_jl(nullptr, "merge of the windows' tables");
                R.var.resize(n);
            }
            R.col_counts.swap(cc);
            for (RankJob &j : jobs)
                if (j.comm) jl_comm_destroy(j.comm);   // (RCCL wants its communicators closed; contexts end with the process)
            tick("kernels + fetch");
        } else {
        if (!opt.consensus.empty()) jl_msa_track_insertions(ctx, 1);   // fuse keeps in-frame insertions (doc/FUSE.md:19)
        if (jl_records_finish(ctx, n_cols, win_begin, opt.min_qv) != JL_OK) die_jl(ctx, "ingest");
        tick("device ingest");
        if (opt.sampling()) {   // the window to call is made of chosen reads, in a second context on the same device and stream
            jl_ctx *taken = nullptr;
            if (jl_ctx_create(opt.device, jl_ctx_stream(ctx), &taken) != JL_OK) die_jl(nullptr, "context of the sample");
            if (!opt.mix.empty()) {
                if (const int code = mix_window(opt, io, ctx, taken, n_cols, win_begin, names, n_reads, sampling)) return code;
                ctx = taken;
            } else {
                bool acted = false;
                if (downsample_window(opt, opt.bam, ctx, taken, names, n_reads, sampling, &acted) != JL_OK) die_jl(taken, "downsample");
                if (acted) ctx = taken;
            }
            tick("sample");
        }

        // --drm-only needs the position list, which the plan of a first pileup provides
        std::vector<uint64_t> drm_masks;
        if (opt.drm_only && drm_masks_of(ctx, in, drm_masks)) die_jl(ctx, "pileup");
        if (opt.fuse_only) {   // the column pileup is all a consensus needs
            if (jl_pileup_async(ctx, genes.data(), (uint32_t)genes.size(), refp, (uint32_t)refcodes.size()) != JL_OK) die_jl(ctx, "pileup");
        } else if (jl_run_async(ctx, genes.data(), (uint32_t)genes.size(), refp, (uint32_t)refcodes.size(), &smp.prm,
                                opt.drm_only ? drm_masks.data() : nullptr, opt.phasing, opt.min_reads, opt.phasing) != JL_OK)
            die_jl(ctx, "run");
        tick("plan + enqueue");

        if (const char *what = fetch_calls(ctx, !opt.fuse_only, R, tick)) die_jl(ctx, what);

        if (!opt.consensus.empty()) {  // what `fuse` writes for this window (doc/FUSE.md:17-24)
            std::vector<uint32_t> len_hist((size_t)n_cols * 32), base_counts((size_t)n_cols * 120);
            if (jl_insertions_fetch(ctx, len_hist.data(), base_counts.data()) != JL_OK) die_jl(ctx, "insertions");
            const std::string seq = fuse_consensus(n_cols, R.col_counts, len_hist, base_counts, opt.ins_min_frac, opt.ins_min_distance);
            std::ofstream f(opt.consensus);
            if (!f) { std::cerr << "juliet: cannot write " << opt.consensus << "\n"; return 2; }
            f << ">consensus window=" << (win_begin + 1) << "-" << (win_begin + n_cols) << " source=" << opt.bam << "\n";
            for (size_t i = 0; i < seq.size(); i += 70) f << seq.substr(i, 70) << "\n";
        }
        if (opt.fuse_only) {
            tick("pileup + consensus");
            jl_ctx_destroy(ctx);
            return 0;
        }
        if (opt.phasing)
            if (const char *what = fetch_phase(ctx, n_reads, R)) die_jl(ctx, what);
        tick("  haplotypes + ids");
        if (opt.rescue) {
            if (const char *what = fetch_rescue(ctx, opt.rescue_min, R)) die_jl(ctx, what);
            tick("rescue");
        }
        if (opt.linkage) {
            if (const char *what = fetch_linkage(ctx, R)) die_jl(ctx, what);
            tick("linkage");
        }
        if (!opt.hap_fasta.empty()) {
            if (const int code = write_haplotype_fasta(opt, ctx, R, win_begin, n_cols)) return code;
            tick("haplotype fasta");
        }
        // (the context is not torn down: the process is about to end, and freeing two dozen device buffers one by one took
        // 4-6 ms of a 0.1 s run)
        }
        // ---------------------------------------------------------------- JSON / HTML (doc/JULIET.md:61-107, 207-211)
        const Json root = build_json(opt, smp, opt.bam, cmdline, names, n_reads, R, &sampling);
        const std::string failed = write_outputs(opt.outputs, root);
        if (!failed.empty()) { std::cerr << "juliet: cannot write " << failed << "\n"; return 2; }
        tick("json / html");
        // Everything is written and closed.  What a `return` would still do — free a gigabyte of record arrays page by page, take down
        // the uploader and the decode pool, destroy the GPU contexts and the HIP runtime's own state — the operating system does at
        // once when the process ends: 40-60 ms of the wall time of a 100k-read run (JL_SLOW_EXIT=1: the long way, for leak checkers).
        if (!getenv("JL_SLOW_EXIT")) {
            std::cout.flush();
            std::cerr.flush();
            fflush(nullptr);
            _exit(0);
        }
        return 0;
    } catch (const std::exception &e) {
        std::cerr << "juliet: " << e.what() << "\n";
        return 2;
    }
}
