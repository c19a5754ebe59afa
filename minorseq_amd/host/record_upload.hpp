// record_upload.hpp — a BAM's records on their way to the device: the one pass over the file (decode_bam), the uploader thread
// that gathers the decoder's chunks and appends them to the records context(s) beside the decode (RecordUploader, with its
// CopyCrew), and the future a context arrives in (CtxFuture: ctx_async starts one beside the decode, ctx_ready wraps one that
// exists).  ms_since is the front end's one clock reading.
#pragma once
#include <chrono>
#include <condition_variable>
#include <deque>
#include <filesystem>
#include <future>
#include <mutex>
#include <thread>

#include "../../include/juliet_hip.h"
#include "decode.hpp"

namespace jlhost {
namespace {

// milliseconds from `t` to `now`
double ms_since(std::chrono::steady_clock::time_point t, std::chrono::steady_clock::time_point now = std::chrono::steady_clock::now())
{
    return std::chrono::duration<double, std::milli>(now - t).count();
}

// A context on its way: the status of jl_ctx_create and the context.
using CtxFuture = std::shared_future<std::pair<int, jl_ctx *>>;

// the GPU context comes up (runtime start, stream, pinned blocks) on a thread of its own, while the host reads the BAM
CtxFuture ctx_async(int device)
{
    return std::async(std::launch::async, [device]() {
               jl_ctx *c = nullptr;
               const int rc = jl_ctx_create(device, nullptr, &c);
               return std::make_pair(rc, c);
           }).share();
}

// a context that exists already
CtxFuture ctx_ready(jl_ctx *c)
{
    std::promise<std::pair<int, jl_ctx *>> p;
    p.set_value(std::make_pair((int)JL_OK, c));
    return p.get_future().share();
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
    RecordUploader(std::vector<CtxFuture> ctx_up, uint64_t file_bytes, bool want_qual, bool qv_mask = false)
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
    std::vector<CtxFuture> ctx_up_;
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

}  // namespace
}  // namespace jlhost
