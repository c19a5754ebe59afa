// capi_group.hip — group runs: the whole path for SEVERAL resident windows in a few launches.
//
// Why.  A 3 kb x 100k-read window is a 150 MB stream: too short to hide a launch's ramp and drain (one pileup launch
// reaches 0.61 of the HBM peak, a 1.2 GB stream 0.77), and its phasing stage is a chain of dependent memory round
// trips that keeps a hardware queue busy for tens of microseconds while doing almost nothing.  A group run gives each
// stage ONE launch for up to JL_GROUP_MAX windows (blockIdx.z = window, per-window argument blocks by value):
//   counting            pileup_planes_group_kernel, or pileup_fold_group_kernel: the same with the Fisher stage in its epilogue
//   Fisher              call_group_kernel, in the unfolded form only (see "Two forms" below)
//   phasing             phase_group_run_kernel (plan out of the call masks, keys, grouping, selection, result block)
//   per-read ids        phase_assign_group_kernel (small chunks have them inline, written by the phasing launch: jl_phase_ids_inline)
//   completion words    done_group_kernel
// A group of more windows is cut into chunks of JL_GROUP_MAX that are PIPELINED inside one captured graph: the
// pileups of consecutive chunks run back to back on the group's stream, each chunk's latency-bound tail runs on a
// side stream next to the following chunk's pileup, so only the last (smallest) chunk's tail is ever exposed.
//
// Results are per window, exactly those of jl_run_async on each context: every context keeps its own result block,
// per-read ids and completion word, so jl_run_wait / jl_run_view_get / jl_call_fetch / jl_phase_fetch work unchanged.
//
// Two forms, chosen per launch (group_pick_form -> group_form.h).  FOLDED: the Fisher stage rides in the counting launch's epilogue —
// one launch and one read-back of the histograms less in the tail, which is what a launch whose tail is exposed gains from.
// UNFOLDED: plain pileup + call_group_kernel — the pileup's workgroups leave as soon as they have counted, which is what a launch
// gains from whose tail runs beside other launches' pileups anyway (the epilogue then only holds workgroup slots those pileups want).
// Which of the two a tail is going to be is read off the completion words of the device's other group launches at enqueue
// time: a few loads from pinned host memory, no HIP call.  Both forms share call_eval.h and give the same bits; a group
// captures a graph per form (and exchange parity): both with the first launch of a configuration where both can be taken.
//
// Independently of that, the counting stage of a launch reads the planes or — every window of the group having a built deviation
// index (kernels_index.hip) — the windows' entry lists (pileup_index_(fold_)group_kernel over the plain chunks, the plane kernel over
// the rest tables where a window has one).  That choice is per launch and at enqueue time as well (group_pick_index); it is the
// second bit of a graph's index, and it is made FIRST: the form's threshold is the counting form's.  A launch from the planes is
// folded while fewer than JL_GROUP_FOLD_BELOW = 3 other group launches of the device are incomplete; a launch from the index while
// fewer than JL_GROUP_FOLD_BELOW_INDEX = 1 are, i.e. only when it is alone (group_form.h says why).  The index-form graphs are
// captured in the launch that enqueues the builds: see there.
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include <chrono>

#include "group_form.h"
#include "jl_comm_internal.h"
#include "jl_internal.h"

#define JL_GROUP_SIDE_STREAMS 2
#ifndef JL_COMM_TIMEOUT_S
#define JL_COMM_TIMEOUT_S 60
#endif
struct jl_group {
    int device = -1;
    hipStream_t stream = nullptr;
    hipStream_t side[JL_GROUP_SIDE_STREAMS] = {nullptr, nullptr};
    hipEvent_t ev_end = nullptr;
    hipEvent_t ev_fork[JL_GROUP_WINDOWS_MAX / JL_GROUP_MAX] = {};
    hipEvent_t ev_join[JL_GROUP_SIDE_STREAMS] = {};
    std::vector<jl_ctx *> ctxs;
    jl_done_ent *d_done = nullptr;
    std::vector<jl_win_pileup> h_pile;
    std::vector<jl_win_call> h_call;
    std::vector<jl_win_fold> h_fold;      // the Fisher stage as the pileup launch's epilogue (every chunk is counted by one workgroup)
    std::vector<jl_win_compact> h_compact;
    std::vector<jl_win_phase> h_phase;
    std::vector<jl_win_index> h_index;    // counting from the deviation index: the plain chunks of every window ...
    std::vector<jl_win_pileup> h_rest;    // ... and the plane kernel's blocks over the other chunks
    bool index_blocks = false;            // the two are filled: every window's index buffers are reserved
    struct chunk_t { uint32_t first, n, max_chunks, max_call_blocks, max_phase_blocks, max_plain, max_rest; bool ids_inline; };
    std::vector<chunk_t> chunks;
    bool phasing = true;
    // one captured graph per parity of a bound exchange (the heads' destination is baked in; unbound: [0] only) and per form
    // (second index: the form | 2 x counting from the deviation index)
    hipGraph_t graph[2][4] = {};
    hipGraphExec_t graph_exec[2][4] = {};
    bool graph_tried[2][4] = {};
    std::vector<uint8_t> sig;   // everything the captured graphs and the tables bake in (the form is the graphs' second index)
    // the last launch, for the other groups' choice of form (under g_live_mu): each window's runs_launched behind it
    bool fl_busy = false;
    uint32_t fl_seq[JL_GROUP_WINDOWS_MAX];
    std::string err;
    // ---- bound exchange (jl_group_exchange_bind): every run carries the all-gather of its windows' table heads
    jl_comm *xc = nullptr;
    bool x_staged = false;           // the all-gather works in device memory and is copied to the pinned region behind it
    uint8_t *x_host = nullptr;       // pinned [2][world][n][JL_PACK_HEAD_BYTES]: by run parity, [rank][window][head] each
    uint8_t *x_dev = nullptr;        // staged form: the same in device memory
    hipEvent_t x_done[2] = {nullptr, nullptr};
    bool x_pending[2] = {false, false};
    uint32_t x_run_seq[2][JL_GROUP_WINDOWS_MAX];   // each window's run number when the exchange went out
    uint64_t x_launched = 0, x_collected = 0;

    size_t x_part() const { return (size_t)JL_PACK_HEAD_BYTES * ctxs.size(); }                  // one rank's heads
    size_t x_region() const { return x_part() * (size_t)(xc ? xc->world : 1); }                 // one exchange
    uint8_t *x_work(uint32_t par) const { return (x_staged ? x_dev : x_host) + x_region() * par; }   // where the collective works
};

static void group_drop_graphs(jl_group *g)
{
    for (int p = 0; p < 2; ++p)
        for (int f = 0; f < 4; ++f) {
            if (g->graph_exec[p][f]) { hipGraphExecDestroy(g->graph_exec[p][f]); g->graph_exec[p][f] = nullptr; }
            if (g->graph[p][f]) { hipGraphDestroy(g->graph[p][f]); g->graph[p][f] = nullptr; }
            g->graph_tried[p][f] = false;
        }
}

// ---- the live groups of the process, for the choice of form.  A group is in the list from jl_group_create to
// jl_group_destroy; a context that is destroyed first takes the groups it is a window of out (jl_group_forget_ctx): nothing
// here reads a completion word that has been freed.
// (never destroyed: a context or a group may be closed while the process exits, after static destructors have run)
static std::mutex &g_live_mu = *new std::mutex();
static std::vector<jl_group *> &g_live = *new std::vector<jl_group *>();
#ifdef JL_TUNING
static uint64_t g_form_taken[2] = {0, 0};
static uint64_t g_form_by_count[4] = {0, 0, 0, 0};   // [form | 2 x counting from the deviation index]
#endif

// Group launches of g's device, other than g's own, that were incomplete a moment ago.  A launch is complete when every window's
// pinned completion word has reached the run number the launch gave it.
static uint32_t group_others_in_flight(const jl_group *g)
{
    uint32_t busy = 0;
    for (jl_group *o : g_live) {
        if (o == g || o->device != g->device || !o->fl_busy) continue;
        bool done = true;
        for (size_t k = 0; k < o->ctxs.size() && done; ++k)
            done = (int32_t)(*o->ctxs[k]->h_seq - o->fl_seq[k]) >= 0;
        if (done) o->fl_busy = false;
        else ++busy;
    }
    return busy;
}

// The form of a launch of g that counts from the planes (ix false) or from the deviation index (ix true), from what is in flight
// on g's device now: FOLDED while the launch's tail is likely to be exposed.  JL_NO_FOLD_CALL: never.  *index_choice: the same
// decision for an index-form launch, whatever this one counts from — what the launch that enqueues the builds captures by.
static jl_group_form_choice group_pick_form(const jl_group *g, bool ix, jl_group_form_choice *index_choice)
{
    const bool fold = jl_fold_enabled();
    uint32_t others = 0, busy = 0;
    if (fold) {
        std::lock_guard<std::mutex> lk(g_live_mu);
        for (const jl_group *o : g_live) others += o != g && o->device == g->device;
        busy = group_others_in_flight(g);
    }
    *index_choice = jl_group_form_decide(busy, others, true, fold);
    return ix ? *index_choice : jl_group_form_decide(busy, others, false, fold);
}

void jl_group_forget_ctx(const jl_ctx *ctx)
{
    std::lock_guard<std::mutex> lk(g_live_mu);
    for (size_t i = 0; i < g_live.size();)
        if (std::find(g_live[i]->ctxs.begin(), g_live[i]->ctxs.end(), ctx) != g_live[i]->ctxs.end()) g_live.erase(g_live.begin() + i);
        else ++i;
}

static int group_fail(jl_group *g, int status, const char *msg)
{
    if (g) g->err = msg;
    return status;
}

// the latency-bound stages of one chunk, on `st`
static void chunk_tail(jl_group *g, const jl_group::chunk_t &c, int form, hipStream_t st)
{
    // (folded form: the Fisher stage ran in the pileup launch's epilogue, kernels_pileup.hip FOLD.  Whichever of the two runs
    // first zeroes the window's run counters — the epilogue's block 0 or call_kernel's first block, never both)
    if (form == JL_FORM_UNFOLDED) jl_launch_call_group(g->h_call.data() + c.first, c.n, c.max_call_blocks, st);
    if (!g->phasing) {
        jl_launch_compact_group(g->h_compact.data() + c.first, c.n, st);
    } else {
        jl_launch_phase_group(g->h_phase.data() + c.first, c.n, c.max_phase_blocks, st);
        if (!c.ids_inline) {
            bool to_host = false;
            for (uint32_t k = 0; k < c.n; ++k) to_host = to_host || g->ctxs[c.first + k]->read_hap_out != nullptr;
            jl_launch_assign_group(g->h_phase.data() + c.first, c.n, c.max_phase_blocks, to_host, st);
        }
    }
    // completion words of the chunk's windows, behind the end of its last stage (see enqueue_path in capi.hip)
    jl_launch_done_group(g->d_done + c.first, c.n, st);
}

// From the deviation index iff EVERY window qualifies now: loads from the windows' pinned records, no HIP call.
static bool group_pick_index(const jl_group *g)
{
    if (!g->index_blocks) return false;
    for (const jl_ctx *c : g->ctxs)
        if (!jl_index_usable(c)) return false;
    return true;
}

// the counting launch(es) of one chunk
static int chunk_pileup(jl_group *g, const jl_group::chunk_t &c, int form, bool ix)
{
    const bool folded = form == JL_FORM_FOLDED;
    if (ix) {
        int rc = jl_launch_pileup_index_group(g->ctxs.data() + c.first, c.n, g->h_index.data() + c.first, folded ? g->h_fold.data() + c.first : nullptr, c.max_plain, g->stream);
        if (rc || !c.max_rest) return rc;
        return folded ? jl_launch_pileup_fold_group(g->ctxs.data() + c.first, c.n, g->h_rest.data() + c.first, g->h_fold.data() + c.first, c.max_rest, g->stream)
                      : jl_launch_pileup_group(g->ctxs.data() + c.first, c.n, g->h_rest.data() + c.first, c.max_rest, g->stream);
    }
    return folded ? jl_launch_pileup_fold_group(g->ctxs.data() + c.first, c.n, g->h_pile.data() + c.first, g->h_fold.data() + c.first, c.max_chunks, g->stream)
                  : jl_launch_pileup_group(g->ctxs.data() + c.first, c.n, g->h_pile.data() + c.first, c.max_chunks, g->stream);
}

static int group_enqueue(jl_group *g, int form, bool ix)
{
    for (jl_ctx *c : g->ctxs)
        if (!c->have_ref) jl_launch_guess(c, g->stream);   // majority-codon mode: seed bases per window
    const size_t nc = g->chunks.size();
    bool side_used[JL_GROUP_SIDE_STREAMS] = {false, false};
    for (size_t k = 0; k < nc; ++k) {
        const jl_group::chunk_t &c = g->chunks[k];
        if (int rc = chunk_pileup(g, c, form, ix)) return rc;
        if (k + 1 < nc) {   // the tail runs beside the next chunk's pileup
            hipStream_t st = g->side[k % JL_GROUP_SIDE_STREAMS];
            if (hipEventRecord(g->ev_fork[k], g->stream) != hipSuccess || hipStreamWaitEvent(st, g->ev_fork[k], 0) != hipSuccess)
                return JL_ERR_DEVICE;
            chunk_tail(g, c, form, st);
            side_used[k % JL_GROUP_SIDE_STREAMS] = true;
        } else {
            chunk_tail(g, c, form, g->stream);
        }
    }
    for (int i = 0; i < JL_GROUP_SIDE_STREAMS; ++i)
        if (side_used[i] && (hipEventRecord(g->ev_join[i], g->side[i]) != hipSuccess ||
                             hipStreamWaitEvent(g->stream, g->ev_join[i], 0) != hipSuccess))
            return JL_ERR_DEVICE;
    return JL_OK;
}

extern "C" {

int jl_group_create(jl_ctx *const *ctxs, uint32_t n_ctx, jl_group **out)
{
    if (!ctxs || !out || n_ctx == 0 || n_ctx > JL_GROUP_WINDOWS_MAX) return JL_ERR_ARG;
    *out = nullptr;
    for (uint32_t k = 0; k < n_ctx; ++k) {
        if (!ctxs[k] || ctxs[k]->device != ctxs[0]->device) return JL_ERR_ARG;
        for (uint32_t j = 0; j < k; ++j)
            if (ctxs[j] == ctxs[k]) return JL_ERR_ARG;
    }
    jl_group *g = new (std::nothrow) jl_group();
    if (!g) return JL_ERR_MEMORY;
    g->device = ctxs[0]->device;
    g->ctxs.assign(ctxs, ctxs + n_ctx);
    g->h_pile.resize(n_ctx);
    g->h_call.resize(n_ctx);
    g->h_fold.resize(n_ctx);
    g->h_compact.resize(n_ctx);
    g->h_phase.resize(n_ctx);
    g->h_index.resize(n_ctx);
    g->h_rest.resize(n_ctx);
    bool ok = hipSetDevice(g->device) == hipSuccess &&
              hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreateWithFlags(&g->ev_end, hipEventDisableTiming) == hipSuccess &&
              hipMalloc(&g->d_done, sizeof(jl_done_ent) * n_ctx) == hipSuccess;
    if (ok && n_ctx > JL_GROUP_MAX) {   // pipelined chunks: side streams for the tails
        for (int i = 0; ok && i < JL_GROUP_SIDE_STREAMS; ++i)
            ok = hipStreamCreateWithFlags(&g->side[i], hipStreamNonBlocking) == hipSuccess &&
                 hipEventCreateWithFlags(&g->ev_join[i], hipEventDisableTiming) == hipSuccess;
        for (auto &e : g->ev_fork)
            ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
    }
    if (!ok) {
        jl_group_destroy(g);
        return JL_ERR_MEMORY;
    }
    {
        std::lock_guard<std::mutex> lk(g_live_mu);
        g_live.push_back(g);
    }
    *out = g;
    return JL_OK;
}

void jl_group_destroy(jl_group *g)
{
    if (!g) return;
    bool live;   // still in the list: none of its contexts has been destroyed (jl_group_forget_ctx)
    {
        std::lock_guard<std::mutex> lk(g_live_mu);
        live = std::find(g_live.begin(), g_live.end(), g) != g_live.end();
        g_live.erase(std::remove(g_live.begin(), g_live.end(), g), g_live.end());
    }
    hipSetDevice(g->device);
    if (g->stream) hipStreamSynchronize(g->stream);
    // The windows outlive the group and their last run was enqueued on its stream, which goes away below: everything of that run
    // is done now, so their fetches (and whatever else waits on "the stream of the last run") go back to their own streams.
    if (live)
        for (jl_ctx *c : g->ctxs)
            if (c->run_stream == g->stream) c->run_stream = c->stream;
    group_drop_graphs(g);
    if (g->x_host) hipHostFree(g->x_host);
    if (g->x_dev) hipFree(g->x_dev);
    for (auto &e : g->x_done)
        if (e) hipEventDestroy(e);
    if (g->d_done) hipFree(g->d_done);
    if (g->ev_end) hipEventDestroy(g->ev_end);
    for (auto &e : g->ev_fork)
        if (e) hipEventDestroy(e);
    for (int i = 0; i < JL_GROUP_SIDE_STREAMS; ++i) {
        if (g->ev_join[i]) hipEventDestroy(g->ev_join[i]);
        if (g->side[i]) hipStreamDestroy(g->side[i]);
    }
    if (g->stream) hipStreamDestroy(g->stream);
    delete g;
}

const char *jl_group_last_error(const jl_group *g) { return g ? g->err.c_str() : ""; }

int jl_group_views(jl_group *g, jl_run_view *out, uint32_t cap, uint32_t *n)
{
    if (!g || !n || (!out && cap)) return JL_ERR_ARG;
    *n = (uint32_t)g->ctxs.size();
    if (g->ctxs.size() > cap) return group_fail(g, JL_ERR_OVERFLOW, "jl_group_views: more windows than the caller's array holds");
    for (size_t k = 0; k < g->ctxs.size(); ++k)
        if (int rc = jl_run_view_get(g->ctxs[k], &out[k])) {
            g->err = "window " + std::to_string(k) + ": " + jl_last_error(g->ctxs[k]);
            return rc;
        }
    return JL_OK;
}

int jl_group_run_async(jl_group *g, const jl_gene *genes, uint32_t n_genes, const uint8_t *refseq, uint32_t ref_len,
                       const jl_params *prm, int phasing, uint32_t min_reads, int want_read_hap)
{
    return jl_group_run_masked_async(g, genes, n_genes, refseq, ref_len, prm, nullptr, phasing, min_reads, want_read_hap);
}

int jl_group_run_masked_async(jl_group *g, const jl_gene *genes, uint32_t n_genes, const uint8_t *refseq, uint32_t ref_len,
                              const jl_params *prm, const uint64_t *const *drm_masks, int phasing, uint32_t min_reads,
                              int want_read_hap)
{
    if (!g || !prm) return JL_ERR_ARG;
    if (hipSetDevice(g->device) != hipSuccess) return group_fail(g, JL_ERR_DEVICE, "hipSetDevice failed");
    const uint32_t n = (uint32_t)g->ctxs.size();
    std::vector<double> n_tests(n);
    const uint32_t par = g->xc ? (uint32_t)(g->x_launched & 1u) : 0u;
    if (g->xc && g->x_pending[par])   // (the same on every rank: nobody issues a collective)
        return group_fail(g, JL_ERR_STATE, "two exchanges of this group are pending: collect one first (jl_group_exchange_collect)");
    // Bound exchange: this run's heads go to the region of its parity (this rank's part), whose magic words are cleared first —
    // whatever goes wrong below on THIS rank, on the host or on the device, the collective is still issued (the peers issue
    // theirs and would wait for ever) and carries empty heads, which every rank reads as this rank's failure.
    bool x_ok = true;
    if (g->xc) {
        uint8_t *mine = g->x_work(par) + g->x_part() * (size_t)g->xc->rank;
        if (!g->x_staged) {
            for (uint32_t k = 0; k < n; ++k) reinterpret_cast<jl_pack *>(mine + (size_t)JL_PACK_HEAD_BYTES * k)->magic = 0u;
        } else if (hipMemsetAsync(mine, 0, g->x_part(), g->stream) != hipSuccess) {
            x_ok = false;
        }
    }
    // ---- the run itself
    auto run_part = [&]() -> int {
    // per-window preparation (plans, buffers, parameter blocks): may allocate and wait, so it comes before any enqueue
    for (uint32_t k = 0; k < n; ++k) {
        jl_ctx *c = g->ctxs[k];
        int rc = jl_run_prepare(c, genes, n_genes, refseq, ref_len, prm, drm_masks ? drm_masks[k] : nullptr, phasing, min_reads,
                                want_read_hap, &n_tests[k]);
        if (rc) return group_fail(g, rc, jl_last_error(c));
        // a group run reads what the window's own stream wrote (uploads, ingest): that stream must be idle
        if (hipStreamSynchronize(c->stream) != hipSuccess) return group_fail(g, JL_ERR_DEVICE, "context stream failed");
        if (phasing && c->phase_form != jl_phase_form::one_word)
            return group_fail(g, JL_ERR_ARG, "a window needs the two-word or the multi-word phasing pipeline: run it with jl_run_async");
    }
    // signature: anything that changes an argument block or the launch shapes
    struct item { uint64_t alloc, plan; double n_tests; void *rh; uint32_t n_dw, drm; };
    std::vector<uint8_t> sig(sizeof(jl_params) + 16 + sizeof(item) * n);
    memcpy(sig.data(), prm, sizeof(jl_params));
    const uint32_t flags[4] = {(uint32_t)(phasing != 0) | (g->xc ? 2u : 0u) | (g->x_staged ? 4u : 0u), min_reads, (uint32_t)(want_read_hap != 0), n};
    memcpy(sig.data() + sizeof(jl_params), flags, 16);
    for (uint32_t k = 0; k < n; ++k) {
        jl_ctx *c = g->ctxs[k];
        item it;
        memset(&it, 0, sizeof it);
        it.alloc = c->alloc_version; it.plan = c->plan_version; it.n_tests = n_tests[k]; it.rh = c->read_hap_out;
        it.n_dw = (uint32_t)(c->col_stride / 4u);
        it.drm = (drm_masks && drm_masks[k]) ? 1u : 0u;
        memcpy(sig.data() + sizeof(jl_params) + 16 + sizeof(item) * k, &it, sizeof it);
    }
    if (sig != g->sig) {
        group_drop_graphs(g);
        g->sig.clear();
        if (hipStreamSynchronize(g->stream) != hipSuccess) return group_fail(g, JL_ERR_DEVICE, "group stream failed");
        g->phasing = phasing != 0;
        // same kernel variant everywhere?  (checked again by the launcher)
        for (uint32_t k = 1; k < n; ++k)
            if (g->ctxs[k]->pileup_w != g->ctxs[0]->pileup_w)
                return group_fail(g, JL_ERR_ARG, "the windows of a group must share the pileup chunk width (gene layouts too different)");
        // chunks of at most JL_GROUP_MAX windows; the remainder goes last (its tail is the exposed one)
        g->chunks.clear();
        g->index_blocks = true;
        for (jl_ctx *x : g->ctxs) g->index_blocks = g->index_blocks && x->ix_reserved;
        for (uint32_t o = 0; o < n; o += JL_GROUP_MAX) {
            jl_group::chunk_t c;
            memset(&c, 0, sizeof c);
            c.first = o;
            c.n = std::min<uint32_t>(JL_GROUP_MAX, n - o);
            // who writes the chunk's per-read ids: decided once, for the argument blocks below and for chunk_tail
            c.ids_inline = jl_phase_ids_inline(g->ctxs.data() + o, c.n);
            for (uint32_t k = o; k < o + c.n; ++k) {
                jl_ctx *x = g->ctxs[k];
                jl_fill_win_pileup(x, &g->h_pile[k]);
                jl_fill_win_call(x, prm, n_tests[k], drm_masks && drm_masks[k], phasing != 0, &g->h_call[k]);
                jl_fill_win_fold(x, &g->h_call[k], &g->h_fold[k]);
                jl_fill_win_compact(x, false, true, false, &g->h_compact[k]);
                jl_fill_win_phase(x, min_reads, false, c.ids_inline, jl_phase_plan::call_masks, &g->h_phase[k]);
                c.max_chunks = std::max(c.max_chunks, g->h_pile[k].n_chunks);
                c.max_call_blocks = std::max(c.max_call_blocks, g->h_call[k].n_blocks);
                c.max_phase_blocks = std::max(c.max_phase_blocks, g->h_phase[k].n_blocks);
                if (g->index_blocks) {
                    jl_fill_win_index(x, &g->h_index[k]);
                    jl_fill_win_pileup_rest(x, true, &g->h_rest[k]);
                    c.max_plain = std::max(c.max_plain, g->h_index[k].n_plain);
                    c.max_rest = std::max(c.max_rest, g->h_rest[k].n_chunks);
                }
            }
            g->chunks.push_back(c);
        }
        {
            std::vector<jl_done_ent> ents(n);
            for (uint32_t k = 0; k < n; ++k) { ents[k].seq_dev = g->ctxs[k]->d_sync; ents[k].seq_host = g->ctxs[k]->h_seq; }
            // (on the group's own stream, not the null stream: rank threads of one process run side by side, and a synchronous copy
            // on the null stream while another thread captures its graph failed once in a few hundred runs of the suite)
            hipError_t he = hipMemcpyAsync(g->d_done, ents.data(), sizeof(jl_done_ent) * n, hipMemcpyHostToDevice, g->stream);
            if (he == hipSuccess) he = hipStreamSynchronize(g->stream);
            if (he != hipSuccess) {
                g->err = std::string("argument tables: ") + hipGetErrorString(he);
                return JL_ERR_DEVICE;
            }
        }
        g->sig = sig;
    }
    for (uint32_t k = 0; k < n; ++k) {
        uint8_t *xh = g->xc ? g->x_work(par) + g->x_part() * (size_t)g->xc->rank + (size_t)JL_PACK_HEAD_BYTES * k : nullptr;
        g->h_phase[k].S.xhead = xh;
        g->h_compact[k].xhead = xh;
    }
    // where THIS launch counts from: the index iff every window's pinned record says "built" NOW; a launch never waits for a build
    const bool ix = group_pick_index(g);
    // ... and its form, from what is in flight now and by the threshold of that counting form (the argument blocks above hold both
    // forms' arguments)
    jl_group_form_choice ix_choice;
    const jl_group_form_choice choice = group_pick_form(g, ix, &ix_choice);
    const int form = choice.form;
#ifdef JL_TUNING
    __atomic_fetch_add(&g_form_taken[form], 1, __ATOMIC_RELAXED);
    __atomic_fetch_add(&g_form_by_count[form | (ix ? 2 : 0)], 1, __ATOMIC_RELAXED);
#endif
    const int gi = form | (ix ? 2 : 0);
    const bool graphs_on = !jl_env().no_graph;
    auto ensure_graph = [&](int f) {
        if (!graphs_on || g->graph_exec[par][f] || g->graph_tried[par][f]) return;
        g->graph_tried[par][f] = true;
        jl_capture_graph(g->stream, &g->graph[par][f], &g->graph_exec[par][f], [&] { return group_enqueue(g, f & 1, (f & 2) != 0); });
    };
    ensure_graph(gi);
    // The other form's graph too, with the first launch of a configuration rather than in the middle of a stream of launches
    // (a capture and its instantiation cost milliseconds) — where this group can ever take that form: the unfolded one needs
    // the counting form's threshold of other groups on the device.  A group whose neighbours are created later captures it at
    // first use.
    if (choice.other_reachable) ensure_graph(gi ^ 1);
    // The index-form graphs are captured by the launch that enqueues the builds (a window's second run), not by the first launch
    // that uses them: their pointers are known — the buffers were reserved at their bound in jl_run_prepare — and that launch is
    // set-up in every caller that has one, while the first use may fall into a stream of launches.  This launch counts from the
    // planes, so the graphs go by what an INDEX-form launch would take now and could take later (ix_choice): the unfolded index
    // graph as soon as ONE other group lives on the device.  bench.py --steps 20 --warmup 5: set-up runs every window alone
    // (run 1), then every full group once (run 2 of all its windows: build + this capture of both index graphs — the other
    // units' groups exist by then —, collected with a stream sync); the next use of unit 0's full group is inside the timed region.
    bool builds_due = false;
    for (const jl_ctx *c : g->ctxs) builds_due = builds_due || c->ix_build_due;
    if (builds_due && g->index_blocks) {
        ensure_graph(ix_choice.form | 2);
        if (ix_choice.other_reachable) ensure_graph((ix_choice.form ^ 1) | 2);
    }
    bool launched = g->graph_exec[par][gi] && hipGraphLaunch(g->graph_exec[par][gi], g->stream) == hipSuccess;
    if (!launched) {
        const int erc = group_enqueue(g, form, ix);
        if (erc != JL_OK || hipGetLastError() != hipSuccess) return group_fail(g, erc ? erc : JL_ERR_DEVICE, "group launch failed");
    }
    // behind the launch's last node, on the same stream: the index builds of the windows this was the second run of
    for (jl_ctx *c : g->ctxs) {
        c->ix_last_form = ix;
        jl_index_after_run(c, g->stream);
    }
    if (hipGetLastError() != hipSuccess) return group_fail(g, JL_ERR_DEVICE, "deviation index build could not be enqueued");
    return JL_OK;
    };
    const int run_rc = run_part();
    int xrc = x_ok ? JL_OK : JL_ERR_DEVICE;
    if (g->xc) {
        // The exchange of this run, behind it on the same stream: ONE collective, in place in the region the kernels have
        // written this rank's heads into — pinned host memory (nothing else to do: the event behind it says the heads of
        // all ranks are there), or its device stage and one copy.  Issued whatever happened above: the peers issue theirs.
        jl_comm *c = g->xc;
        uint8_t *work = g->x_work(par);
        jl_comm_direct_wait_begin(c);
        if (jl_tp_allgather(c, work + g->x_part() * (size_t)c->rank, work, g->x_part(), g->stream) != JL_OK && xrc == JL_OK) xrc = JL_ERR_COMM;
        jl_comm_direct_end(c);
        if (g->x_staged) {      // (the end of that kernel is what pushes its stores to the host out; the event behind it says so)
            jl_launch_heads_to_host(work, g->x_host + g->x_region() * par, (uint32_t)(g->x_region() / JL_PACK_HEAD_BYTES), g->stream);
            if (hipGetLastError() != hipSuccess && xrc == JL_OK) xrc = JL_ERR_DEVICE;
        }
        if (hipEventRecord(g->x_done[par], g->stream) != hipSuccess && xrc == JL_OK) xrc = JL_ERR_DEVICE;
        g->x_pending[par] = true;
        ++g->x_launched;
    } else if (g->ev_end && run_rc == JL_OK) {
        // An event behind the launch: the runtime retires a stream whose last command is an event marker without a marker of
        // its own (hipStreamSynchronize / the closing hipDeviceSynchronize of a short run: 12 instead of 20-30 us per stream).
        hipEventRecord(g->ev_end, g->stream);
    }
    if (run_rc != JL_OK) return run_rc;   // (its message stands; the exchange, if any, went out with empty heads and is pending)
    {
        std::lock_guard<std::mutex> lk(g_live_mu);   // (fl_seq / fl_busy are read by the other groups' threads)
        for (uint32_t k = 0; k < n; ++k) {
            jl_ctx *c = g->ctxs[k];
            jl_run_finish(c, phasing, want_read_hap);
            c->run_stream = g->stream;
            if (g->xc) g->x_run_seq[par][k] = c->runs_launched;
            g->fl_seq[k] = c->runs_launched;
        }
        g->fl_busy = true;
    }
    if (xrc != JL_OK) return group_fail(g, xrc, xrc == JL_ERR_COMM ? g->xc->tp_error.c_str() : "the run's exchange could not be enqueued");
    return JL_OK;
}

int jl_group_exchange_bind(jl_group *g, jl_comm *c)
{
    if (!g) return JL_ERR_ARG;
    if (hipSetDevice(g->device) != hipSuccess) return group_fail(g, JL_ERR_DEVICE, "hipSetDevice failed");
    if (g->x_pending[0] || g->x_pending[1]) return group_fail(g, JL_ERR_STATE, "an exchange of this group is pending: collect it first");
    if (c == g->xc) return JL_OK;
    if (hipStreamSynchronize(g->stream) != hipSuccess) return group_fail(g, JL_ERR_DEVICE, "group stream failed");
    group_drop_graphs(g);
    g->sig.clear();
    if (g->x_host) { hipHostFree(g->x_host); g->x_host = nullptr; }
    if (g->x_dev) { hipFree(g->x_dev); g->x_dev = nullptr; }
    g->xc = nullptr;
    g->x_launched = g->x_collected = 0;
    if (!c) return JL_OK;
    if (c->device != g->device) return group_fail(g, JL_ERR_ARG, "group and communicator are on different devices");
    if (g->ctxs.size() > JL_GATHER_MAX) return group_fail(g, JL_ERR_ARG, "a bound exchange carries at most 32 windows");
    g->xc = c;
    g->x_staged = jl_comm_host_gather(c) == 0;   // (a collective the first time a communicator is asked)
    bool ok = hipHostMalloc(&g->x_host, 2 * g->x_region(), hipHostMallocDefault) == hipSuccess;
    if (ok) memset(g->x_host, 0, 2 * g->x_region());
    if (ok && g->x_staged) ok = hipMalloc(&g->x_dev, 2 * g->x_region()) == hipSuccess && hipMemsetAsync(g->x_dev, 0, 2 * g->x_region(), g->stream) == hipSuccess &&
                                hipStreamSynchronize(g->stream) == hipSuccess;
    for (auto &e : g->x_done)
        if (ok && !e) ok = hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        g->xc = nullptr;
        return group_fail(g, JL_ERR_MEMORY, "exchange regions");
    }
    return JL_OK;
}

int jl_group_exchange_collect(jl_group *g, jl_variant *all_rows, uint32_t *all_counts, uint32_t cap_rows)
{
    if (!g || !all_rows || !all_counts) return JL_ERR_ARG;
    if (!g->xc) return group_fail(g, JL_ERR_STATE, "jl_group_exchange_collect: no exchange is bound to this group");
    if (cap_rows == 0 || cap_rows > JL_VARIANT_CAP) return group_fail(g, JL_ERR_ARG, "cap_rows must be 1..4096");
    const uint32_t par = (uint32_t)(g->x_collected & 1u);
    if (!g->x_pending[par]) return group_fail(g, JL_ERR_STATE, "jl_group_exchange_collect: no exchange of this group is pending");
    if (hipSetDevice(g->device) != hipSuccess) return group_fail(g, JL_ERR_DEVICE, "hipSetDevice failed");
    jl_comm *c = g->xc;
    {   // spin on the event (a blocking wait costs ~15 us of wake-up latency), but not for ever: a peer may have died
        hipError_t q;
        const auto deadline = std::chrono::steady_clock::now() + std::chrono::seconds(JL_COMM_TIMEOUT_S);
        uint32_t polls = 0;
        while ((q = hipEventQuery(g->x_done[par])) == hipErrorNotReady)
            if ((++polls & 0xFFFu) == 0 && std::chrono::steady_clock::now() > deadline)
                return group_fail(g, JL_ERR_COMM, "the group's exchange is not complete after the time-out: a peer has not issued its collective");
        if (q != hipSuccess) return group_fail(g, JL_ERR_DEVICE, "the group's exchange failed on the device");
    }
    g->x_pending[par] = false;
    ++g->x_collected;
    // a window whose matrix an enqueued record ingest made: what that ingest found wrong with the records is reported before
    // tables computed from it are handed out (the run is over: the verdict word is final)
    for (jl_ctx *ctx : g->ctxs)
        if (ctx->ing.check_pending)
            if (int vrc = jl_ingest_verdict(ctx)) return group_fail(g, vrc, ctx->err.c_str());
    const uint32_t n = (uint32_t)g->ctxs.size();
    const uint8_t *base = g->x_host + g->x_region() * par;
    auto head = [&](int r, uint32_t k) { return reinterpret_cast<const jl_pack *>(base + g->x_part() * (size_t)r + (size_t)JL_PACK_HEAD_BYTES * k); };
    bool compact = true;
    for (int r = 0; r < c->world; ++r)
        for (uint32_t k = 0; k < n; ++k) {
            // a head without the magic word: that rank's run did not reach its result block; every rank sees the same
            if (head(r, k)->magic != JL_PACK_MAGIC) {
                g->err = "rank " + std::to_string(r) + "'s run of window " + std::to_string(k) + " did not complete: its head of the exchange is empty";
                return JL_ERR_COMM;
            }
            if (!head(r, k)->fits_call) compact = false;
        }
    int rc = JL_OK;
    for (uint32_t k = 0; k < n; ++k) {
        jl_variant *rows = all_rows + (size_t)k * c->world * cap_rows;
        uint32_t *counts = all_counts + (size_t)k * c->world;
        if (compact) {
            for (int r = 0; r < c->world; ++r) {
                const jl_pack *pk = head(r, k);
                counts[r] = pk->nvar_total;
                if (pk->nvar_total > cap_rows) { rc = JL_ERR_OVERFLOW; continue; }
                memcpy(rows + (size_t)r * cap_rows, pk->variants, (size_t)pk->nvar_total * sizeof(jl_variant));
            }
            continue;
        }
        // Some rank's table has more rows than a head holds: the full stride from the resident tables, window by window —
        // every rank takes this branch (same heads everywhere).  The resident table is the LAST run's.
        jl_ctx *x = g->ctxs[k];
        if (x->runs_launched != g->x_run_seq[par][k])
            return group_fail(g, JL_ERR_STATE, "a rank called more than 128 variants: such a run's exchange must be collected before the "
                                               "group's next run (the full table is not double-buffered)");
        rc = jl_comm_allgather_full(x, c, rows, counts, cap_rows, g->x_run_seq[par][k]);
        if (rc) return group_fail(g, rc, jl_last_error(x));
    }
    if (rc) return group_fail(g, rc, "a rank produced more rows than cap_rows");
    return JL_OK;
}

// Average device time in ms of the grouped pileup launch alone — pileup_planes_group_kernel, the plain kernel of the unfolded
// form, over the launch of a group's FIRST chunk: the bytes the roofline counts against the kernel that only moves them.
// `reps` back-to-back launches rotating over the given groups (all on the first group's stream), one pair of HIP events
// around them.  Every group must have run at least once (its argument tables are what the launch reads).  The launch
// rewrites the windows' column counts and codon histograms with the values they hold already (the matrix has not
// changed) and touches nothing else: the last run's tables, run counters and results stay as they are and stay fetchable.
int jl_group_time_pileup(jl_group *const *groups, uint32_t n_groups, uint32_t reps, float *ms_avg, uint64_t *bytes_per_launch)
{
    if (!groups || n_groups == 0 || !ms_avg || reps == 0) return JL_ERR_ARG;
    jl_group *g0 = groups[0];
    for (uint32_t k = 0; k < n_groups; ++k)
        if (!groups[k] || groups[k]->sig.empty() || groups[k]->device != g0->device)
            return group_fail(g0, JL_ERR_STATE, "jl_group_time_pileup: every group must have run once");
    if (hipSetDevice(g0->device) != hipSuccess) return group_fail(g0, JL_ERR_DEVICE, "hipSetDevice failed");
    for (uint32_t k = 0; k < n_groups; ++k)
        if (hipStreamSynchronize(groups[k]->stream) != hipSuccess) return group_fail(g0, JL_ERR_DEVICE, "group stream failed");
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return group_fail(g0, JL_ERR_DEVICE, "events");
    auto launch = [&](jl_group *g) {
        const jl_group::chunk_t &c = g->chunks[0];
        return jl_launch_pileup_group(g->ctxs.data() + c.first, c.n, g->h_pile.data() + c.first, c.max_chunks, g0->stream);
    };
    int rc = JL_OK;
    for (uint32_t k = 0; k < n_groups && rc == JL_OK; ++k) rc = launch(groups[k]);   // warm-up, once per group
    hipEventRecord(e0, g0->stream);
    for (uint32_t r = 0; r < reps && rc == JL_OK; ++r) rc = launch(groups[r % n_groups]);
    hipEventRecord(e1, g0->stream);
    float total = 0.f;
    if (rc == JL_OK && (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&total, e0, e1) != hipSuccess)) rc = JL_ERR_DEVICE;
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    if (rc) return group_fail(g0, rc, "grouped pileup launch failed");
    *ms_avg = total / (float)reps;
    if (bytes_per_launch) {
        uint64_t b = 0;
        const jl_group::chunk_t &c = g0->chunks[0];
        for (uint32_t k = c.first; k < c.first + c.n; ++k) b += (uint64_t)g0->ctxs[k]->n_reads * g0->ctxs[k]->n_cols * 3u / 8u;   // 3 bits per cell
        *bytes_per_launch = b;
    }
    return JL_OK;
}

#ifdef JL_TUNING
// test hook of the -DJL_TUNING build: group launches of this process that took the folded / the unfolded form
__attribute__((visibility("default"))) void jl_tuning_group_forms(uint64_t *folded, uint64_t *unfolded)
{
    if (folded) *folded = __atomic_load_n(&g_form_taken[JL_FORM_FOLDED], __ATOMIC_RELAXED);
    if (unfolded) *unfolded = __atomic_load_n(&g_form_taken[JL_FORM_UNFOLDED], __ATOMIC_RELAXED);
}
// ... and the same by what the launch counted from: out[0..3] = folded from the planes, unfolded from the planes, folded from the
// deviation index, unfolded from the deviation index
__attribute__((visibility("default"))) void jl_tuning_group_forms_by_count(uint64_t out[4])
{
    for (int i = 0; i < 4; ++i) out[i] = __atomic_load_n(&g_form_by_count[i], __ATOMIC_RELAXED);
}
// ... and the device-resident scalars of a context's last phasing run (jl_phase_meta: run counters, overflow bits, summary) as
// bytes, behind everything on the run's stream: what a test compares before and after a call that must not touch them.
// Returns the number of bytes written, or a negative status.
__attribute__((visibility("default"))) int jl_tuning_ctx_meta(jl_ctx *ctx, void *out, uint32_t cap)
{
    if (!ctx || !out || cap < sizeof(jl_phase_meta)) return JL_ERR_ARG;
    hipStream_t st = ctx->run_stream ? ctx->run_stream : ctx->stream;
    if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(st) != hipSuccess ||
        hipMemcpyAsync(out, ctx->d_meta, sizeof(jl_phase_meta), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return JL_ERR_DEVICE;
    return (int)sizeof(jl_phase_meta);
}
// ... and the pipeline that phases the context (tests/phase_edges_child.py asserts which form a case ran): out[0..3] = the
// jl_phase_form, key words the key buffer holds, workgroups of the window's phasing grid, whether a launch of this window alone
// writes the per-read ids itself (inline ids).
__attribute__((visibility("default"))) int jl_tuning_phase_form(jl_ctx *ctx, uint32_t *out)
{
    if (!ctx || !out) return JL_ERR_ARG;
    out[0] = (uint32_t)ctx->phase_form;
    out[1] = ctx->keys_words;
    out[2] = jl_phase_grid_blocks(ctx);
    out[3] = jl_phase_ids_inline(&ctx, 1) ? 1u : 0u;
    return JL_OK;
}
// ... and who wrote the per-read ids of the group's last launch configuration: out[k] = 1 where chunk k's phasing launch wrote
// them itself (inline ids), 0 where the separate launch did.  Returns the number of chunks, or a negative status.
__attribute__((visibility("default"))) int jl_tuning_group_ids_inline(jl_group *g, uint32_t *out, uint32_t cap)
{
    if (!g || !out || g->chunks.size() > cap) return JL_ERR_ARG;
    for (size_t k = 0; k < g->chunks.size(); ++k) out[k] = g->chunks[k].ids_inline ? 1u : 0u;
    return (int)g->chunks.size();
}
#endif

}  // extern "C"
