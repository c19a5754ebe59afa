// capi_index.hip — the deviation index of a resident window: its owner state, its policy and its one invalidation point.
//
// What it is and why: deviation_index.h and DESIGN.md "The deviation index"; the build's kernels: kernels_index.hip; the kernel
// that counts from it: pileup_index_body (kernels_pileup.hip).  The planes stay THE resident format; the index is derived from them
// behind a window's SECOND run (a window analysed once never pays) and read from the third run on — as soon as the record the
// build leaves in pinned host memory says "built" for the matrix generation in force.
#include <string.h>

#include "deviation_index.h"
#include "jl_internal.h"

static bool ix_chunk_is_plain(uint64_t rec) { return (uint32_t)(rec >> 32) == (3u | (1u << 4)); }   // JL_CHUNK_META(3, 1, 0), kernels_pileup.hip


// the index, its run counter and what refers to them go; buffers of a size worth giving back are freed
void jl_index_drop(jl_ctx *ctx)
{
    if (ctx->ix_enqueued && ctx->ix_ev.ev) hipEventSynchronize(ctx->ix_ev.ev);   // a build still on its stream writes what goes
    if (ctx->ix_reserved) {
        hipSetDevice(ctx->device);
        ctx->d_ix_entries.release();
    }
    ctx->ix_runs = 0;
    ctx->ix_reserved = ctx->ix_build_due = ctx->ix_enqueued = false;
    ctx->ix_last_form = 0;
    ctx->ix_n_plain = ctx->ix_n_rest = 0;
    if (ctx->h_ix) ctx->h_ix[0] = JL_IX_NONE;
}

// THE invalidation point of everything derived from the cells of d_msa.  Every writer of the planes reaches it:
//   set_shape              every producer that makes its matrix first: jl_msa_alloc(_strided), and through it jl_msa_upload,
//                          jl_msa_pack_rows, jl_msa_ingest_records(_masked), jl_records_finish, jl_records_window(_async)
//                          (records_build), jl_msa_take(_async), jl_sites_assemble(_alleles), the cross-window assemblies and
//                          sessions (capi_xwin.hip), and jl_msa_adopt
//   free_msa               an owned or adopted matrix goes (a failed upload, jl_msa_adopt, jl_ctx_destroy)
//   synth_fill             jl_synth_fill(_window): the one producer that rewrites a matrix in place
// It bumps the matrix generation (the pinned record of a build names the generation it belongs to), drops the index and its run
// counter, and makes every captured graph stale (they bake index pointers and the choice of form in).  The last is new for
// jl_synth_fill(_window), which used to leave the graphs alone: a caller that refills a matrix in place and runs it again now has
// its context's and its groups' graphs captured anew after every refill (milliseconds) — the price of one invalidation point.
void jl_msa_touched(jl_ctx *ctx)
{
    jl_index_drop(ctx);
    ctx->msa_gen++;
    ctx->alloc_version++;
}

int jl_index_count_run(jl_ctx *ctx)
{
    ctx->ix_runs++;
    ctx->ix_build_due = false;
    // The SECOND run of a generation and chunk table builds, if: the matrix is owned (an adopted one may change behind the
    // library's back), a read number fits an entry, the chunk table has a plain chunk, and nothing about the index is pending.
    if (ctx->ix_runs != 2u || ctx->ix_enqueued || !ctx->own_msa || ctx->n_reads > JL_IX_MAX_READS || ctx->pileup_w != 3u) return JL_OK;
    std::vector<uint4> tab;
    std::vector<uint64_t> rest;
    for (uint64_t rec : ctx->h_chunks) {
        if (ix_chunk_is_plain(rec)) tab.push_back(uint4{(uint32_t)rec, 0u, 0u, 0u});
        else rest.push_back(rec);
    }
    if (tab.empty() || tab.size() + rest.size() != ctx->n_chunks) return JL_OK;
    const uint64_t room = jl_ix_alloc_entries(ctx->plane_stride, ctx->n_cols, (uint32_t)tab.size());
    if (room >= 0xFFFFFFF0ull) return JL_OK;   // offsets are 32 bits
    bool moved = false, any = false;
    hipError_t e = ctx->d_ix_tab.reserve_exact(tab.size(), &moved);
    any |= moved;
    if (e == hipSuccess) { e = ctx->d_ix_rest.reserve_exact(std::max<size_t>(rest.size(), 1), &moved); any |= moved; }
    if (e == hipSuccess) { e = ctx->d_ix_seed.reserve_exact(ctx->n_cols, &moved); any |= moved; }
    if (e == hipSuccess) { e = ctx->d_ix_rec.reserve_exact(8, &moved); any |= moved; }
    if (e == hipSuccess) { e = ctx->h_ix.reserve_exact(8, &moved); any |= moved; }
    if (e == hipSuccess) { e = ctx->d_ix_entries.reserve_exact((size_t)room, &moved); any |= moved; }
    if (e == hipSuccess && !ctx->ix_ev.ev) e = hipEventCreateWithFlags(&ctx->ix_ev.ev, hipEventDisableTiming);
    if (any) ctx->alloc_version++;
    if (e == hipErrorOutOfMemory) {   // no room for the index: the window stays on its planes
        (void)hipGetLastError();
        ctx->d_ix_entries.release();
        return JL_OK;
    }
    if (e != hipSuccess) return jl_fail(ctx, jl_hip_status(e), "deviation index: %s", hipGetErrorString(e));
    JL_HIP(ctx, hipMemcpyAsync(ctx->d_ix_tab, tab.data(), tab.size() * sizeof(uint4), hipMemcpyHostToDevice, ctx->stream));
    if (!rest.empty()) JL_HIP(ctx, hipMemcpyAsync(ctx->d_ix_rest, rest.data(), rest.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    JL_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (the staging vectors are pageable)
    ctx->ix_n_plain = (uint32_t)tab.size();
    ctx->ix_n_rest = (uint32_t)rest.size();
    ctx->ix_reserved = ctx->ix_build_due = true;
    return JL_OK;
}

#ifdef JL_TUNING
// test hook of the -DJL_TUNING build: index builds this process has enqueued (a measurement shows with it that a leg builds none)
static uint64_t g_builds = 0;
extern "C" __attribute__((visibility("default"))) uint64_t jl_tuning_index_builds(void) { return __atomic_load_n(&g_builds, __ATOMIC_RELAXED); }
#endif

void jl_index_after_run(jl_ctx *ctx, hipStream_t st)
{
    if (!ctx->ix_build_due) return;
    ctx->ix_build_due = false;
    ctx->h_ix[3] = (uint32_t)ctx->msa_gen;
    ctx->h_ix[0] = JL_IX_PENDING;
    jl_launch_index_build(ctx, st);
    hipEventRecord(ctx->ix_ev.ev, st);
    ctx->ix_enqueued = true;
    ctx->ix_builds++;
#ifdef JL_TUNING
    __atomic_fetch_add(&g_builds, 1, __ATOMIC_RELAXED);
#endif
}

// a load from pinned host memory and no HIP call, as group_others_in_flight reads the completion words
bool jl_index_usable(const jl_ctx *ctx)
{
    return ctx->ix_enqueued && ctx->h_ix[0] == JL_IX_BUILT && ctx->h_ix[3] == (uint32_t)ctx->msa_gen;
}

extern "C" int jl_msa_index_info(jl_ctx *ctx, jl_index_info *info, int wait, uint8_t *chunk_flags, uint32_t cap_chunks)
{
    if (!ctx || !info) return JL_ERR_ARG;
    memset(info, 0, sizeof *info);
    if (ctx->ix_enqueued && (wait || chunk_flags)) {
        JL_HIP(ctx, hipSetDevice(ctx->device));
        JL_HIP(ctx, hipEventSynchronize(ctx->ix_ev.ev));
    }
    const bool mine = ctx->ix_enqueued && ctx->h_ix[3] == (uint32_t)ctx->msa_gen;
    info->state = mine ? ctx->h_ix[0] : JL_IX_NONE;
    info->generation = ctx->msa_gen;
    info->runs = ctx->ix_runs;
    info->builds = ctx->ix_builds;
    info->last_form = ctx->ix_last_form;
    info->plain_chunks = ctx->ix_n_plain;
    if (info->state == JL_IX_BUILT) {
        info->entries = ctx->h_ix[1];
        info->indexed_chunks = ctx->h_ix[2];
    }
    info->bytes = ctx->ix_reserved ? (uint64_t)ctx->d_ix_entries.cap * JL_IX_ENTRY_BYTES : 0u;
    if (chunk_flags) {
        if (!ctx->plan_valid || cap_chunks < ctx->n_chunks) return jl_fail(ctx, JL_ERR_ARG, "jl_msa_index_info: %u chunks, room for %u", ctx->n_chunks, cap_chunks);
        memset(chunk_flags, 0, ctx->n_chunks);
        if (info->state == JL_IX_BUILT) {
            std::vector<uint4> tab(ctx->ix_n_plain);
            JL_HIP(ctx, hipMemcpyAsync(tab.data(), ctx->d_ix_tab, tab.size() * sizeof(uint4), hipMemcpyDeviceToHost, ctx->stream));
            JL_HIP(ctx, hipStreamSynchronize(ctx->stream));
            uint32_t p = 0;
            for (uint32_t k = 0; k < ctx->n_chunks; ++k)
                if (ix_chunk_is_plain(ctx->h_chunks[k])) chunk_flags[k] = tab[p++].z == 0xFFFFFFFFu ? 2u : 1u;
        }
    }
    return JL_OK;
}
