// kernels_take.hip — a resident matrix made of chosen reads of other resident matrices (jl_msa_take: downsampling, mixtures,
// bootstrap resampling).  A read is one bit position in the three planes of every column, so choosing reads is a bit gather:
//   take_kernel   destination read j = read idx[j] of the part that j falls into, every column, all three planes; destination
//                 reads past the last one are padding (code 6: plane 0 clear, planes 1 and 2 set) out to the end of the plane row
// A wave owns 1024 consecutive destination reads = ONE 128-byte line of each destination plane row (the library's plane stride
// is whole lines: jl_plane_stride).  Lane l holds destination reads 64 k + l (k = 0..15) of the line: where the source byte of
// each lies (a pointer that walks down the source's plane rows by the SOURCE's stride — an adopted source has its own) and
// which bit of it.  Per plane row: 16 gathered byte loads a lane, 16 ballots (ballot k = destination reads 64 k .. 64 k + 63 = the
// line's k-th 8 bytes), and lanes 0..15 store the line as one 128-byte write.  Sorted indices (a downsample) make the 64 bytes
// of one ballot neighbours in the source row: the gather then reads whole cache lines, the source's planes once.
// Nothing here checks an index: the host did (capi_take.hip), so no address outside a source's ceil(n_reads / 8) bytes is formed.
#include "jl_internal.h"

namespace {

constexpr uint32_t kTakeWaves = 4;   // waves of a workgroup: the same line, different columns
constexpr uint32_t kTakeCols = 4;    // columns a wave gathers with one set of source pointers (12 plane rows)

// grid: x = destination line (1024 reads), y = column chunk of kTakeWaves * kTakeCols columns (chunks beyond the grid's y: a loop)
__global__ __launch_bounds__(64 * kTakeWaves) void take_kernel(jl_take_args a)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t j0 = (uint64_t)blockIdx.x * 1024u + lane;
    // the sources of this lane's 16 destination reads, relative to plane row 0: byte, bit, the source's stride
    // (typed as global memory: a pointer out of the argument block is generic to the compiler otherwise, jl_internal.h JL_AS1)
    const uint8_t JL_AS1 *src[16];
    uint32_t stride[16], bit[16], valid = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16u; ++k) {
        const uint64_t j = j0 + 64u * k;
        src[k] = (const uint8_t JL_AS1 *)a.part[0].base;
        stride[k] = 0u, bit[k] = 0u;
        if (j < a.n_total) {
            const uint32_t s = ((const uint32_t JL_AS1 *)a.idx)[j];
            const uint8_t JL_AS1 *base = (const uint8_t JL_AS1 *)a.part[0].base;
            uint32_t st = a.part[0].stride;
#pragma unroll
            for (uint32_t p = 1; p < (uint32_t)JL_TAKE_MAX_PARTS; ++p)   // (the parts' first reads ascend: the last one at or below j)
                if (p < a.n_parts && j >= a.part[p].begin) base = (const uint8_t JL_AS1 *)a.part[p].base, st = a.part[p].stride;
            src[k] = base + (s >> 3);
            stride[k] = st, bit[k] = s & 7u;
            valid |= 1u << k;
        }
    }
    const uint32_t per_chunk = kTakeWaves * kTakeCols;
    const uint32_t n_chunks = (a.n_cols + per_chunk - 1u) / per_chunk;
    uint64_t row_at = 0;   // the plane row the pointers stand at
    for (uint32_t chunk = blockIdx.y; chunk < n_chunks; chunk += gridDim.y) {
        const uint32_t c0 = chunk * per_chunk + wave * kTakeCols;
        if (c0 >= a.n_cols) break;   // (this wave's columns only grow with the chunk)
        const uint32_t c1 = min(c0 + kTakeCols, a.n_cols);
        const uint64_t skip = 3ull * c0 - row_at;
#pragma unroll
        for (uint32_t k = 0; k < 16u; ++k) src[k] += skip * stride[k];
        uint8_t JL_AS1 *out = (uint8_t JL_AS1 *)a.dst + 3ull * c0 * a.dst_stride + (uint64_t)blockIdx.x * 128u + 8u * lane;
        for (uint32_t c = c0; c < c1; ++c) {
#pragma unroll
            for (uint32_t plane = 0; plane < 3u; ++plane) {
                uint32_t v[16];
#pragma unroll
                for (uint32_t k = 0; k < 16u; ++k) {
                    v[k] = 0u;
                    if ((valid >> k) & 1u) v[k] = *src[k];
                    src[k] += stride[k];
                }
                uint64_t mine = 0;
#pragma unroll
                for (uint32_t k = 0; k < 16u; ++k) {
                    // a padding read has code 6: its bit is set in planes 1 and 2
                    const bool set = ((valid >> k) & 1u) ? ((v[k] >> bit[k]) & 1u) != 0u : plane != 0u;
                    const uint64_t m = __ballot(set);
                    if (lane == k) mine = m;
                }
                if (lane < 16u) *(uint64_t JL_AS1 *)out = mine;
                out += a.dst_stride;
            }
        }
        row_at = 3ull * c1;
    }
}

}  // namespace

// `a->n_total` reads, at least one; enqueued on `st`
void jl_launch_take(const jl_take_args *a, hipStream_t st)
{
    const uint32_t n_lines = (uint32_t)((a->n_total + 1023u) / 1024u);
    const uint32_t per_chunk = kTakeWaves * kTakeCols;
    const uint32_t n_chunks = (a->n_cols + per_chunk - 1u) / per_chunk;
    dim3 grid(n_lines, std::min<uint32_t>(n_chunks, 65535u));
    hipLaunchKernelGGL(take_kernel, grid, dim3(64 * kTakeWaves), 0, st, *a);
}
