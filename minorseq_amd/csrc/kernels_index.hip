// kernels_index.hip — the deviation index of a resident window: the kernels of its build (owner state and policy: capi_index.hip).
//
// What it is and why: deviation_index.h and DESIGN.md "The deviation index".  The planes stay THE resident format; the index is
// derived from them behind a window's SECOND run (a window analysed once never pays) and read by pileup_index_body
// (kernels_pileup.hip) from the third run on — as soon as the record the build leaves in pinned host memory says "built" for the
// matrix generation in force.  The build is five launches on the stream of the run it follows, no host round trip in between:
//   seed     the exact majority base among A C G T of every column (ties: the lowest code) — a property of the cells alone
//   count    per plain chunk, the reads that differ from the seed in some column: popcount of x | inv, as the plane kernel forms them
//   scan     which chunks stay under the density bound, their offsets in entries (a list begins on four entries = 8 bytes), the
//            total against its bound
//   fill     the entries, stored as their 16 code bits (jl_ix_stored): a wave's lanes take consecutive positions (prefix over the lanes), one atomic per wave and step for the place
//   publish  the record into the pinned block: state, entries, indexed chunks, generation
// The buffer is allocated before the build at the bound (jl_ix_alloc_entries), so the pointers a captured graph bakes in are known
// when the build is enqueued.
#include <string.h>

#include "deviation_index.h"
#include "jl_internal.h"
#include "planes.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void ix_seed_kernel(const uint8_t *__restrict__ planes, uint64_t plane_stride, uint64_t n_reads,
                                                      uint32_t n_cols, uint8_t *__restrict__ seed)
{
    __shared__ uint32_t s_n[4];
    const uint32_t c = blockIdx.x, tid = threadIdx.x;
    if (c >= n_cols) return;
    if (tid < 4) s_n[tid] = 0;
    __syncthreads();
    const uint32_t n_words = (uint32_t)((n_reads + 31u) / 32u);   // 4 n_words <= plane_stride (set_shape)
    const uint32_t *r0 = reinterpret_cast<const uint32_t *>(planes + (uint64_t)c * 3u * plane_stride);
    const uint32_t *r1 = reinterpret_cast<const uint32_t *>(planes + ((uint64_t)c * 3u + 1u) * plane_stride);
    const uint32_t *r2 = reinterpret_cast<const uint32_t *>(planes + ((uint64_t)c * 3u + 2u) * plane_stride);
    uint32_t n[4] = {0, 0, 0, 0};
    for (uint32_t w = tid; w < n_words; w += 256u) {
        const uint32_t b0 = r0[w], b1 = r1[w], base = ~r2[w] & jl_valid_bits(n_reads, w);
        n[0] += __popc(base & ~b1 & ~b0);
        n[1] += __popc(base & ~b1 & b0);
        n[2] += __popc(base & b1 & ~b0);
        n[3] += __popc(base & b1 & b0);
    }
    for (int k = 0; k < 4; ++k)
        if (n[k]) atomicAdd(&s_n[k], n[k]);
    __syncthreads();
    if (tid == 0) {
        uint32_t best = 0;
        for (uint32_t k = 1; k < 4; ++k)
            if (s_n[k] > s_n[best]) best = k;
        seed[c] = (uint8_t)best;
    }
}

// the reads of 16-byte unit `u` of a plain chunk's rows that deviate from the seed, as four words of bits; `d` = the nine loads
struct ix_unit {
    u32x4 d[3][3];
    uint32_t dev[4];
};
__device__ __forceinline__ void ix_load_unit(ix_unit &t, const uint8_t *planes, uint64_t plane_stride, uint64_t n_reads, uint32_t c0,
                                             const uint32_t (&g)[3], uint32_t u)
{
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k)
            t.d[j][k] = *reinterpret_cast<const u32x4 *>(planes + ((uint64_t)(c0 + j) * 3u + k) * plane_stride + (uint64_t)u * 16u);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint32_t x = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j)
            x |= (t.d[j][1][q] ^ ((g[j] & 2u) ? 0xFFFFFFFFu : 0u)) | (t.d[j][0][q] ^ ((g[j] & 1u) ? 0xFFFFFFFFu : 0u)) | t.d[j][2][q];
        t.dev[q] = x & jl_valid_bits(n_reads, (uint64_t)u * 4u + (uint32_t)q);   // padding reads are never in a list
    }
}

// grid (plain chunks, read splits): tab[p].z += deviating reads of chunk p
__global__ __launch_bounds__(256) void ix_count_kernel(const uint8_t *__restrict__ planes, uint64_t plane_stride, uint64_t n_reads,
                                                       const uint8_t *__restrict__ seed, uint4 *__restrict__ tab)
{
    __shared__ uint32_t s_total;
    const uint32_t p = blockIdx.x, tid = threadIdx.x;
    const uint32_t c0 = tab[p].x;
    const uint32_t g[3] = {seed[c0], seed[c0 + 1u], seed[c0 + 2u]};
    if (tid == 0) s_total = 0;
    __syncthreads();
    const uint32_t n_units = (uint32_t)(plane_stride / 16u);
    uint32_t n = 0;
    for (uint32_t u = blockIdx.y * 256u + tid; u < n_units; u += 256u * gridDim.y) {
        ix_unit t;
        ix_load_unit(t, planes, plane_stride, n_reads, c0, g, u);
        n += __popc(t.dev[0]) + __popc(t.dev[1]) + __popc(t.dev[2]) + __popc(t.dev[3]);
    }
    if (n) atomicAdd(&s_total, n);
    __syncthreads();
    if (tid == 0 && s_total) atomicAdd(&tab[p].z, s_total);
}

// one workgroup: offsets of the chunks under the density bound, the total against `limit`; rec[0..3] = state, entries, indexed chunks, -
__global__ __launch_bounds__(256) void ix_scan_kernel(uint4 *__restrict__ tab, uint32_t n_plain, uint32_t chunk_max, uint64_t limit,
                                                      uint32_t *__restrict__ rec)
{
    __shared__ uint32_t s_scan[256];
    __shared__ unsigned long long s_base, s_entries;
    __shared__ uint32_t s_indexed;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) s_base = 0, s_entries = 0, s_indexed = 0;
    __syncthreads();
    for (uint32_t p0 = 0; p0 < n_plain; p0 += 256u) {
        const uint32_t p = p0 + tid;
        const uint32_t E = p < n_plain ? tab[p].z : 0u;
        const bool ok = p < n_plain && E <= chunk_max;
        const uint32_t room = ok ? (uint32_t)jl_ix_padded(E) : 0u;
        s_scan[tid] = room;
        __syncthreads();
        for (uint32_t d = 1; d < 256u; d <<= 1) {   // inclusive scan (a window's chunk_max x 256 fits 32 bits: 2^23 reads -> 1.2M entries)
            const uint32_t v = tid >= d ? s_scan[tid - d] : 0u;
            __syncthreads();
            s_scan[tid] += v;
            __syncthreads();
        }
        const unsigned long long at = s_base + s_scan[tid] - room;
        if (p < n_plain) {
            // (an offset past 32 bits belongs to an index that is refused below: nobody reads it)
            tab[p].y = (uint32_t)at;
            tab[p].z = ok ? E : 0xFFFFFFFFu;
            tab[p].w = 0u;
        }
        if (ok) {
            atomicAdd(&s_entries, (unsigned long long)E);
            atomicAdd(&s_indexed, 1u);
        }
        __syncthreads();
        if (tid == 0) s_base += s_scan[255];
        __syncthreads();
    }
    if (tid == 0) {
        rec[0] = s_base > limit || s_indexed == 0u ? JL_IX_REFUSED : JL_IX_BUILT;
        rec[1] = (uint32_t)s_entries;
        rec[2] = s_indexed;
        rec[3] = (uint32_t)(s_entries >> 32);
    }
}

// grid (plain chunks, read splits): the entries of every indexed chunk
__global__ __launch_bounds__(256) void ix_fill_kernel(const uint8_t *__restrict__ planes, uint64_t plane_stride, uint64_t n_reads,
                                                      const uint8_t *__restrict__ seed, uint4 *__restrict__ tab, const uint32_t *__restrict__ rec,
                                                      jl_ix_stored_t *__restrict__ entries)
{
    const uint32_t p = blockIdx.x, tid = threadIdx.x, lane = tid & 63u;
    if (rec[0] != JL_IX_BUILT) return;
    const uint4 row = tab[p];
    if (row.z == 0xFFFFFFFFu) return;   // over the density bound: stays on the planes
    const uint32_t c0 = row.x;
    const uint32_t g[3] = {seed[c0], seed[c0 + 1u], seed[c0 + 2u]};
    uint32_t *cursor = &tab[p].w;
    const uint32_t n_units = (uint32_t)(plane_stride / 16u);
    for (uint32_t u0 = blockIdx.y * 256u; u0 < n_units; u0 += 256u * gridDim.y) {   // (uniform over the workgroup: the shuffles below)
        const uint32_t u = u0 + tid;
        ix_unit t;
        t.dev[0] = t.dev[1] = t.dev[2] = t.dev[3] = 0u;
        if (u < n_units) ix_load_unit(t, planes, plane_stride, n_reads, c0, g, u);
        const uint32_t n = __popc(t.dev[0]) + __popc(t.dev[1]) + __popc(t.dev[2]) + __popc(t.dev[3]);
        uint32_t incl = n;
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t v = __shfl_up(incl, d);
            if (lane >= d) incl += v;
        }
        const uint32_t total = __shfl(incl, 63);
        if (total == 0u) continue;   // (wave-uniform)
        uint32_t base = 0;
        if (lane == 63u) base = atomicAdd(cursor, total);
        base = __shfl(base, 63);
        // base + total <= E while the count pass saw the same cells (every writer of the planes waits for the build first:
        // jl_index_drop); `end` keeps a store inside the chunk's room whatever else is true
        uint32_t at = row.y + base + incl - n;
        const uint32_t end = row.y + row.z;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t rest = t.dev[q];
            while (rest) {
                const uint32_t b = (uint32_t)__ffs((int)rest) - 1u;
                rest &= rest - 1u;
                uint32_t code[3];
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    code[j] = (((t.d[j][2][q] >> b) & 1u) << 2) | (((t.d[j][1][q] >> b) & 1u) << 1) | ((t.d[j][0][q] >> b) & 1u);
                // (the entry names its read while it is formed; what is stored is its codes: deviation_index.h)
                if (at < end) entries[at] = jl_ix_stored(jl_ix_encode((u * 4u + (uint32_t)q) * 32u + b, code[0], code[1], code[2]));
                ++at;
            }
        }
    }
}

__global__ void ix_publish_kernel(const uint32_t *__restrict__ rec, uint32_t gen, volatile uint32_t *host)
{
    host[1] = rec[1];
    host[2] = rec[2];
    host[3] = gen;
    __threadfence_system();
    host[0] = rec[0];   // last: the host takes the rest as final once it reads "built" / "refused" for its generation
    __threadfence_system();
}

}  // namespace

// the five launches of a build on `st`; the buffers are reserved (capi_index.hip jl_index_count_run)
void jl_launch_index_build(jl_ctx *ctx, hipStream_t st)
{
    const uint32_t rounds = (uint32_t)((ctx->plane_stride / 16u + 255u) / 256u);
    const uint32_t want = 4096u / std::max(1u, ctx->ix_n_plain);
    const uint32_t splits = std::max(1u, std::min({rounds, want, 65535u}));   // read splits of the count and fill grids
    const uint64_t room = jl_ix_alloc_entries(ctx->plane_stride, ctx->n_cols, ctx->ix_n_plain);
    hipLaunchKernelGGL(ix_seed_kernel, dim3(ctx->n_cols), dim3(256), 0, st, ctx->d_msa, ctx->plane_stride, ctx->n_reads, ctx->n_cols, ctx->d_ix_seed.d);
    hipLaunchKernelGGL(ix_count_kernel, dim3(ctx->ix_n_plain, splits), dim3(256), 0, st, ctx->d_msa, ctx->plane_stride, ctx->n_reads,
                       ctx->d_ix_seed.d, ctx->d_ix_tab.d);
    hipLaunchKernelGGL(ix_scan_kernel, dim3(1), dim3(256), 0, st, ctx->d_ix_tab.d, ctx->ix_n_plain, (uint32_t)jl_ix_chunk_max_entries(ctx->plane_stride),
                       room - 4u, ctx->d_ix_rec.d);
    hipLaunchKernelGGL(ix_fill_kernel, dim3(ctx->ix_n_plain, splits), dim3(256), 0, st, ctx->d_msa, ctx->plane_stride, ctx->n_reads,
                       ctx->d_ix_seed.d, ctx->d_ix_tab.d, ctx->d_ix_rec.d, ctx->d_ix_entries.d);
    hipLaunchKernelGGL(ix_publish_kernel, dim3(1), dim3(1), 0, st, ctx->d_ix_rec.d, (uint32_t)ctx->msa_gen, ctx->h_ix.d);
}
