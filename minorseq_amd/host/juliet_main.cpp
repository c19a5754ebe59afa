// juliet — command-line front end over libjuliet_hip.so: aligned CCS BAM in, JSON (and a plain HTML
// rendering of it) out.  Keeps the documented surface of the reference tool:
//   juliet [--config/-c CFG] [--mode-phasing/-p] [--region/-r B-E] [--min-perc X] [--max-perc X] [--drm-only]
//          in.align.bam out.{json,html} [out2.{json,html}]
//   juliet [options] --batch samples.tsv   (many per-barcode BAMs in one process: batch.hpp)
// (doc/JULIET.md:62-66, 121, 160-163, 195, 270-271, 342-344, 352-354, 370).  Everything the reference text
// leaves open is an explicit flag with the docs/SPEC.md default.  All compute happens on the GPU through
// the C ABI; without a gfx950 device the tool exits with status 3.
//
// This file is the one translation unit of the front end and holds main() and one function per mode; the rest is cut into
// headers by what they own: options.hpp (the command line), record_upload.hpp (decode + upload), sample.hpp (one sample, step
// by step), report.hpp (JSON / HTML / FASTA), windows.hpp (--windows / --devices), batch.hpp (--batch).
#include "batch.hpp"
#include "msa_builder.hpp"
#include "options.hpp"
#include "report.hpp"
#include "sample.hpp"
#include "windows.hpp"

using namespace jlhost;

namespace {

// --dump-config without a BAM: the config as read, and the genes --region leaves of it (no GPU involved)
int dump_config(const Options &opt, TargetConfig cfg)
{
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

// --dump-msa: host-side ingest check, no GPU involved
void dump_msa(const Options &opt, const IngestOptions &io, const ReadExtent &ext, const SampleSetup &smp)
{
    std::vector<uint8_t> rows;
    const uint64_t n_reads = build_rows(opt.bam, io, ext.ref_id, smp.win_begin, smp.n_cols, ext.n_reads, rows, nullptr);
    std::ofstream f(opt.dump_msa, std::ios::binary);
    const uint64_t hdr[3] = {n_reads, smp.n_cols, smp.win_begin};
    f.write((const char *)hdr, sizeof hdr);
    f.write((const char *)rows.data(), (std::streamsize)((size_t)n_reads * smp.n_cols));
}

// One run of one sample: what its steps hand on, from the loaded records to the written outputs.
struct Run {
    const Options &opt;
    const std::string &cmdline;
    const Tick &tick;
    IngestOptions io;
    SampleLoad load;     // the records, the reads' names and their count (--downsample / --mix replace the last two)
    SampleSetup smp;
    Results R;
    SamplingInfo sampling;
    ReadFilterInfo read_filter;
    HypermutInfo hypermut;
    OrfInfo orf;
    ControlInfo control;
};

// JSON / HTML (doc/JULIET.md:61-107, 207-211), and the end of the process
int write_run(Run &run)
{
    const Json root = build_json(run.opt, run.smp, run.opt.bam, run.cmdline, run.load.names, run.load.n_reads, run.R, &run.sampling, &run.read_filter, &run.control, &run.hypermut, &run.orf);
    const std::string failed = write_outputs(run.opt.outputs, root);
    if (!failed.empty()) { std::cerr << "juliet: cannot write " << failed << "\n"; return 2; }
    run.tick("json / html");
    if (!getenv("JL_SLOW_EXIT")) end_process(0);
    return 0;
}

// `fuse in.bam out.fasta`, the early leg of the one-window run: the column pileup is all a consensus needs
int run_fuse(Run &run, jl_ctx *ctx)
{
    const SampleSetup &smp = run.smp;
    if (jl_pileup_async(ctx, smp.genes.data(), (uint32_t)smp.genes.size(), smp.refp(), (uint32_t)smp.refcodes.size()) != JL_OK) die_jl(ctx, "pileup");
    run.tick("plan + enqueue");
    if (const char *what = fetch_calls(ctx, false, run.R, run.tick)) die_jl(ctx, what);
    if (const int code = write_consensus(run.opt, ctx, run.R, smp.win_begin, smp.n_cols)) return code;
    run.tick("pileup + consensus");
    jl_ctx_destroy(ctx);
    return 0;
}

// One window on one device: ingest, the read filter, the hypermutation filter, the reading-frame filter, --downsample / --mix, the run, its results, the outputs.
int run_one_window(Run &run)
{
    const Options &opt = run.opt;
    const Tick &tick = run.tick;
    const SampleSetup &smp = run.smp;
    const uint32_t win_begin = smp.win_begin, n_cols = smp.n_cols;
    std::vector<std::string> &names = run.load.names;
    uint64_t &n_reads = run.load.n_reads;
    Results &R = run.R;
    jl_ctx *ctx = run.load.uploader->ctx();
    const DeviceStageInput in{&opt, &smp.cfg, &smp.genes, &smp.refcodes, smp.prm, win_begin, n_cols, n_reads};
    if (const int code = exit_code_of(ingest_window(ctx, n_cols, win_begin, opt), opt.bam)) return code;
    tick("device ingest");
    if (opt.read_filter()) {   // the reads a rule keeps, in a second context on the same device and stream (docs/SPEC.md §20)
        jl_ctx *kept = nullptr;
        if (jl_ctx_create(opt.device, jl_ctx_stream(ctx), &kept) != JL_OK) die_jl(nullptr, "context of the kept reads");
        bool acted = false;
        if (const int code = exit_code_of(read_filter_window(opt, smp, ctx, kept, names, n_reads, run.read_filter, &acted), opt.bam)) return code;
        if (acted) ctx = kept;
        tick("read filter");
    }
    if (opt.hypermut()) {   // the reads that are not hypermutated, of those the read filter kept (docs/SPEC.md §26)
        jl_ctx *kept = nullptr;
        if (jl_ctx_create(opt.device, jl_ctx_stream(ctx), &kept) != JL_OK) die_jl(nullptr, "context of the kept reads");
        bool acted = false;
        if (const int code = exit_code_of(hypermut_window(opt, smp, ctx, kept, &run.read_filter, names, n_reads, run.hypermut, &acted), opt.bam)) return code;
        if (acted) ctx = kept;
        tick("hypermutation filter");
    }
    if (opt.orf()) {   // the reads whose reading frames are whole, of those the two filters before kept (docs/SPEC.md §27)
        jl_ctx *kept = nullptr;
        if (jl_ctx_create(opt.device, jl_ctx_stream(ctx), &kept) != JL_OK) die_jl(nullptr, "context of the kept reads");
        bool acted = false, reference = false;
        const std::vector<uint8_t> *row = earlier_row(run.read_filter, run.hypermut, &reference);
        if (const int code = exit_code_of(orf_window(opt, smp, ctx, kept, row, reference, names, n_reads, run.orf, &acted), opt.bam)) return code;
        if (acted) ctx = kept;
        tick("reading-frame filter");
    }
    if (opt.sampling()) {   // the window to call is made of chosen reads, in a second context on the same device and stream
        jl_ctx *taken = nullptr;
        if (jl_ctx_create(opt.device, jl_ctx_stream(ctx), &taken) != JL_OK) die_jl(nullptr, "context of the sample");
        if (!opt.mix.empty()) {
            if (const int code = mix_window(opt, run.io, ctx, taken, n_cols, win_begin, names, n_reads, run.sampling)) return code;
            ctx = taken;
        } else {
            bool acted = false;
            if (downsample_window(opt, opt.bam, ctx, taken, names, n_reads, run.sampling, &acted) != JL_OK) die_jl(taken, "downsample");
            if (acted) ctx = taken;
        }
        tick("sample");
    }

    // --drm-only needs the position list, which the plan of a first pileup provides
    std::vector<uint64_t> drm_masks;
    if (opt.drm_only && drm_masks_of(ctx, in, drm_masks)) die_jl(ctx, "pileup");
    if (opt.fuse_only) return run_fuse(run, ctx);
    if (!opt.control.empty()) {   // the codons against a control's counts (docs/SPEC.md §21), in the place of the error-model run
        jl_ctx *control = nullptr, *failed = nullptr;
        if (const int code = control_window(opt, run.io, smp, ctx, &control, run.control)) return code;
        tick("control");
        if (const char *what = run_control_calls(ctx, control, smp, opt.drm_only ? drm_masks.data() : nullptr, opt.phasing, opt.min_reads, R, tick, &failed))
            die_jl(failed, what);
    } else {
        if (jl_run_async(ctx, smp.genes.data(), (uint32_t)smp.genes.size(), smp.refp(), (uint32_t)smp.refcodes.size(), &smp.prm,
                         opt.drm_only ? drm_masks.data() : nullptr, opt.phasing, opt.min_reads, opt.phasing) != JL_OK)
            die_jl(ctx, "run");
        tick("plan + enqueue");
        if (const char *what = fetch_calls(ctx, true, R, tick)) die_jl(ctx, what);
    }
    if (!opt.consensus.empty())
        if (const int code = write_consensus(opt, ctx, R, win_begin, n_cols)) return code;
    if (opt.phasing)
        if (const char *what = fetch_phase(ctx, n_reads, R)) die_jl(ctx, what);
    tick("  haplotypes + ids");
    if (opt.rescue) {
        if (const char *what = fetch_rescue(ctx, opt.rescue_min, R)) die_jl(ctx, what);
        tick("rescue");
    }
    if (opt.have_absorb) {
        if (const char *what = fetch_absorb(ctx, opt.absorb_min, opt.absorb_distance, R)) die_jl(ctx, what);
        tick("absorb");
    }
    if (opt.flag_recombinants) {
        if (const char *what = fetch_recombinants(ctx, opt.recomb_min, opt.recomb_ratio, R)) die_jl(ctx, what);
        tick("recombinants");
    }
    if (opt.linkage) {
        if (const char *what = fetch_linkage(ctx, R)) die_jl(ctx, what);
        tick("linkage");
    }
    if (opt.call_deletions) {
        if (const char *what = fetch_deletions(ctx, opt, smp.prm, smp.genes, smp.refcodes, win_begin, n_cols, R)) die_jl(ctx, what);
        tick("deletions");
    }
    if (opt.call_insertions) {
        if (const char *what = fetch_insertions(ctx, opt, smp.prm, smp.genes, n_cols, R)) die_jl(ctx, what);
        tick("insertions");
    }
    if (opt.call_deletion_alleles) {
        if (const char *what = fetch_deletion_alleles(ctx, opt, smp.prm, smp.genes, R)) die_jl(ctx, what);
        tick("deletion_alleles");
    }
    if (opt.phase_deletions || opt.phase_insertions) {   // (the haplotypes, hit rows and per-read ids from here on are those of the site matrix)
        jl_ctx *pc = nullptr;
        if (const char *what = fetch_sites_phase(ctx, opt.device, opt.min_reads, n_reads, opt.phase_deletions, opt.phase_insertions, R, &pc)) die_jl(pc ? pc : ctx, what);
        tick("sites");
    }
    if (opt.hap_mutations) {
        if (const char *what = fetch_haplotype_mutations(ctx, smp.refcodes, win_begin, R)) die_jl(ctx, what);
        tick("class_codons");
    }
    if (!opt.hap_fasta.empty()) {
        if (const int code = write_haplotype_fasta(opt, ctx, R, win_begin, n_cols)) return code;
        tick("haplotype fasta");
    }
    // (the context is not torn down: the process is about to end, and freeing two dozen device buffers one by one took
    // 4-6 ms of a 0.1 s run)
    return write_run(run);
}

// `juliet in.bam out...`: the sample onto the device(s) — its setup and --dump-msa while the contexts come up — then the mode
int run_sample(const Options &opt, const TargetConfig &cfg, const std::string &cmdline, const Tick &tick)
{
    Run run{opt, cmdline, tick, ingest_options(opt), {}, {}, {}, {}, {}, {}, {}, {}};
    // the GPU context comes up (runtime start, stream, pinned blocks) while the host reads the BAM
    const bool need_gpu = !opt.outputs.empty() || opt.fuse_only;
    std::vector<CtxFuture> ctx_ups;
    if (need_gpu)
        for (int dev : opt.devices) ctx_ups.push_back(ctx_async(dev));
    run.load = load_begin(opt.bam, run.io, ctx_ups, opt, tick);
    if (const int code = exit_code_of(run.load, opt.bam)) return code;
    if (sample_window(opt, cfg, run.load.dec, run.smp)) return 1;
    if (!opt.dump_msa.empty()) {
        dump_msa(opt, run.io, run.load.dec.ext, run.smp);
        if (opt.outputs.empty()) return 0;
    }
    sample_params(opt, run.load.dec, run.smp);
    load_finish(run.load, ctx_ups, tick);
    if (const int code = exit_code_of(run.load, opt.bam)) return code;
    const RecordUploader &up = *run.load.uploader;
    if (opt.timing)
        fprintf(stderr, "juliet: timing   uploader thread: gather %.1f ms, begin %.1f ms, %u appends %.1f ms (longest %.1f), names %.1f ms\n",
                up.ms_gather, up.ms_begin, up.n_appends, up.ms_append, up.ms_append_max, up.ms_names);
    run.R.col_counts.assign((size_t)run.smp.n_cols * 6, 0);
    if (opt.windows > 1 || opt.devices.size() > 1) {
        const SampleSetup &smp = run.smp;
        const DeviceStageInput in{&opt, &smp.cfg, &smp.genes, &smp.refcodes, smp.prm, smp.win_begin, smp.n_cols, run.load.n_reads};
        if (const int code = run_windows(in, up, run.R, tick)) return code;
        return write_run(run);
    }
    return run_one_window(run);
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
            fprintf(stderr, "juliet: timing %-26s %9.1f ms  (at %9.1f ms)\n", what, ms_since(t_last, now), ms_since(t_start, now));
            t_last = now;
        };
        TargetConfig cfg;
        if (!opt.config.empty()) cfg = TargetConfig::load(opt.config);
        if (!opt.batch.empty()) return run_batch(opt, cfg, cmdline);
        if (!opt.dump_config.empty() && opt.bam.empty()) return dump_config(opt, cfg);
        return run_sample(opt, cfg, cmdline, tick);
    } catch (const std::exception &e) {
        std::cerr << "juliet: " << e.what() << "\n";
        return 2;
    }
}
