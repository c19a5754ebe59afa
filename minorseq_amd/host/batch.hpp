// batch.hpp — --batch: many per-barcode BAMs in one process (BatchRunner, run_batch), each sample through the steps of sample.hpp
// and the writers of report.hpp.
#pragma once
#include <atomic>
#include <condition_variable>
#include <deque>
#include <map>
#include <mutex>
#include <thread>

#include "report.hpp"
#include "sample.hpp"

namespace jlhost {
namespace {

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
        first_ = ctx_async(opt_.device);
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
                    ms_since(t_start));
        // every output is written, closed and checked: the same fast end as a single run (JL_SLOW_EXIT=1: the long way)
        if (!getenv("JL_SLOW_EXIT")) end_process(failed ? 2 : 0);
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
        ReadFilterInfo read_filter;
        HypermutInfo hypermut;
        OrfInfo orf;
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
            const CtxFuture up = i == 0 ? first_ : ctx_ready(acquire());
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
    // The context a pool context's filtered or downsampled window goes into (a filtered window's own companion, when both act): same device, same stream, made when first needed and kept.
    jl_ctx *companion_of(jl_ctx *c)   // (decoding thread only)
    {
        jl_ctx *&t = taken_[c];
        if (!t && jl_ctx_create(opt_.device, jl_ctx_stream(c), &t) != JL_OK) gpu_error("context of a downsampled window");
        return t;
    }
    jl_ctx *context_of(const CtxFuture &up)
    {
        const auto r = up.get();
        if (r.first != JL_OK) gpu_error("no usable GPU (this tool has no CPU fallback)");
        return r.second;
    }
    // Decode + upload, setup, device ingest and masks of one sample: "" (ready), or why the sample failed.
    std::string prepare(Sample &smp, const CtxFuture &up)
    {
        const auto t0 = std::chrono::steady_clock::now();
        const Options::BatchLine &l = *smp.line;
        SampleLoad load;
        try {
            load = load_sample(l.bam, ingest_options(opt_), {up}, opt_, quiet_tick);
        } catch (const std::exception &e) {
            return e.what();
        }
        // JL_ERR_ARG from the upload is the records' fault, not the device's
        if (load.outcome == Outcome::device && !(load.ctx && load.rc == JL_ERR_ARG)) gpu_error(load.text());
        if (load.outcome != Outcome::ok) return load.text();
        smp.ctx = context_of(up);
        smp.names.swap(load.names);
        load.uploader.reset();   // (its threads and its gathered arrays)
        smp.n_reads = load.n_reads;
        if (sample_window(opt_, cfg_, load.dec, smp.s)) return "--region leaves no gene of the config";
        sample_params(opt_, load.dec, smp.s);
        const Status ingest = ingest_window(smp.ctx, smp.s.n_cols, smp.s.win_begin, opt_);
        // ... and so are JL_ERR_ARG and JL_ERR_STATE from the ingest (a malformed record)
        if (ingest.outcome == Outcome::device && ingest.rc != JL_ERR_ARG && ingest.rc != JL_ERR_STATE) gpu_error(ingest.text());
        if (ingest.outcome != Outcome::ok) return ingest.text();
        smp.run = smp.ctx;
        if (opt_.read_filter()) {   // (every sample of the list by the same rule; docs/SPEC.md §20)
            jl_ctx *kept = companion_of(smp.ctx);
            bool acted = false;
            const Status rf = read_filter_window(opt_, smp.s, smp.ctx, kept, smp.names, smp.n_reads, smp.read_filter, &acted);
            if (rf.outcome == Outcome::device) gpu_error(rf.text());
            if (rf.outcome != Outcome::ok) return rf.text();
            if (acted) smp.run = kept;
        }
        if (opt_.hypermut()) {   // (every sample of the list at the same level; docs/SPEC.md §26)
            jl_ctx *kept = companion_of(smp.run);
            bool acted = false;
            const Status hs = hypermut_window(opt_, smp.s, smp.run, kept, &smp.read_filter, smp.names, smp.n_reads, smp.hypermut, &acted);
            if (hs.outcome == Outcome::device) gpu_error(hs.text());
            if (hs.outcome != Outcome::ok) return hs.text();
            if (acted) smp.run = kept;
        }
        if (opt_.orf()) {   // (every sample of the list under the same rule; docs/SPEC.md §27)
            jl_ctx *kept = companion_of(smp.run);
            bool acted = false, reference = false;
            const std::vector<uint8_t> *row = earlier_row(smp.read_filter, smp.hypermut, &reference);
            const Status os = orf_window(opt_, smp.s, smp.run, kept, row, reference, smp.names, smp.n_reads, smp.orf, &acted);
            if (os.outcome == Outcome::device) gpu_error(os.text());
            if (os.outcome != Outcome::ok) return os.text();
            if (acted) smp.run = kept;
        }
        if (opt_.have_downsample && smp.n_reads > opt_.downsample) {   // (every sample of the list goes to the same depth)
            jl_ctx *taken = companion_of(smp.run);
            bool acted = false;
            if (downsample_window(opt_, l.bam, smp.run, taken, smp.names, smp.n_reads, smp.sampling, &acted) != JL_OK)
                gpu_error(std::string("downsample: ") + jl_last_error(taken));
            if (acted) smp.run = taken;
        }
        if (opt_.drm_only) {
            const DeviceStageInput in{&opt_, &smp.s.cfg, &smp.s.genes, &smp.s.refcodes, smp.s.prm, smp.s.win_begin, smp.s.n_cols, smp.n_reads};
            if (drm_masks_of(smp.run, in, smp.drm_masks)) gpu_error(std::string("pileup: ") + jl_last_error(smp.run));
        }
        if (opt_.timing)
            fprintf(stderr, "juliet: timing batch decode  line %u  %llu reads  %.1f ms\n", l.line, (unsigned long long)smp.n_reads,
                    ms_since(t0));
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
        for (Sample *x : chunk) {
            x->R.col_counts.assign((size_t)x->s.n_cols * 6, 0);
            const char *what = fetch_calls(x->run, true, x->R, quiet_tick);
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
                ms_since(t0));
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
            const Json root = build_json(opt_, x.s, x.line->bam, cmdline_, x.names, x.n_reads, x.R, &x.sampling, &x.read_filter, nullptr, &x.hypermut, &x.orf);
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
    CtxFuture first_;
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
}  // namespace jlhost
