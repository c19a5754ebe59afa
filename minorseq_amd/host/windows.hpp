// windows.hpp — K column windows over R devices (--windows K [--devices a,b,...]): the plan (plan_windows), one rank (thread) per
// device with its windows out of the records uploaded to it (run_rank; RankVote keeps a failed rank from leaving its peers inside
// a collective), and run_windows, which drives the ranks and merges what they bring into the Results of one window.
#pragma once
#include <condition_variable>
#include <mutex>
#include <thread>

#include "sample.hpp"

namespace jlhost {
namespace {

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
        job.laps.emplace_back(what, ms_since(t_last, now));
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
        job.laps.emplace_back(what, ms_since(t_last, now));
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

// ---- K column windows over R devices (doc/JULIET.md:261-264: each gene is treated separately, so the split
// never shows): one rank (thread) per device; the Bonferroni factor counts the codons of ALL genes in every window.
// The records are on the uploader's contexts, one per device, and no window of them is ingested: run_rank ingests per
// window.  R.col_counts comes sized for the overall window; R leaves as one window's.  0, or the process's exit status.
int run_windows(const DeviceStageInput &in, const RecordUploader &uploader, Results &R, const Tick &tick)
{
    const Options &opt = *in.opt;
    const uint32_t win_begin = in.win_begin, n_cols = in.n_cols;
    const uint64_t n_reads = in.n_reads;
    const size_t n_ranks = opt.devices.size();
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
        jobs[r].records = uploader.ctx(r);
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
    return 0;
}

}  // namespace
}  // namespace jlhost
