// kernels_phase.hip — read x variant co-occurrence phasing.
// Behaviour: doc/JULIET.md:192-211 (--mode-phasing, haplotype_hit, haplotype block), :253-254 (>= 10 reads),
// :372-381 (reported / insufficient / damaged, overlapping marginals); docs/SPEC.md §8.
//
// Stages (no host round trip):
//   plan    distinct variant columns, ascending, from the resident variant table (done by call_kernel's last block
//           in a whole-path run; phase_plan_kernel for a host-supplied table)
//   keys    per read: flags (gap / heteroduplex / partial) and the pattern of codon indices at the Vp
//           positions, 6 bits each, 10 positions per 64-bit word, first position most significant so that
//           word-wise unsigned comparison is the lexicographic order of patterns
//   group   exact grouping of clean reads into an open-addressing table
//   select  groups with >= min_reads ranked by (count desc, pattern asc), haplotype ids, patterns, hit matrix
//           + variant x variant co-occurrence, the result block, and emptying of the table slots used
//   assign  per-read haplotype id
// Vp <= 10 (one key word): ONE launch — phase_fused1_kernel (a window) / phase_group_run_kernel (several windows,
// blockIdx.z): keys + grouping in every block, the selection by the block that arrives last, and — when all
// workgroups of the launch are resident together (<= JL_INLINE_IDS_MAX_BLOCKS) — the per-read ids ("inline ids") by every block from the slots still
// in its registers (the others wait on a flag); larger launches leave the ids to a separate launch, phase_assign(_group)_kernel.
// A workgroup of these launches is phase_fused_body: its stages, in order, are fused_plan_stage, fused_keys_stage, group_round,
// fused_arrive, then fused_last (the last workgroup) or fused_wait (the others), and fused_ids_and_leave; its LDS is one fused_lds.
// 11 <= Vp <= 20: the same body with two key words, phase_fused2_kernel (jl_two_word).
// Vp > 20, or a context on the multi-word form: phase_keys_kernel, phase_group_kernel, phase_select_kernel, phase_assign_kernel.
// Every selection reads the window's argument block, jl_win_phase; the kernels take it by value.
#include <string.h>

#include <algorithm>

#include "call_eval.h"
#include "jl_internal.h"
#include "phase_plan.h"
#include "planes.h"
#include "result_pack.h"

namespace {

constexpr uint32_t kM1 = 0x11111111u;
constexpr uint32_t kEmpty = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t wave_sum_all(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ---------------------------------------------------------------------------------------- plan
// (the argument block of the compact launch, which makes the same plan behind a call stage: jl_fill_win_compact)
__global__ __launch_bounds__(1024) void phase_plan_kernel(jl_win_compact c)
{
    uint32_t nv = c.n_rows[0];
    if (nv > c.cap) nv = c.cap;
    jl_phase_plan_block(c.rows, nv, c.n_cols, c.varcol, c.vpcols, c.col2pos, c.kwords_cap, c.fast_only, c.meta);
}

// ---------------------------------------------------------------------------------------- keys
// One variant position of a lane's 8 reads: w[k] = the codes of column c + k, a nibble per read.  Adds the reads' flags (bit
// 4r of each mask) and appends the position's 6-bit codon index to every read's key word.
__device__ __forceinline__ void key_add_position(const uint32_t (&w)[3], uint32_t &gap, uint32_t &het, uint32_t &par, uint64_t (&key)[8])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t b0 = w[k] & kM1, b1 = (w[k] >> 1) & kM1, b2 = (w[k] >> 2) & kM1;
        gap |= b2 & ~b1 & ~b0;  // 4 = '-'
        het |= b2 & b0;         // 5 = 'N'
        par |= b2 & b1;         // 6 = not covered
    }
    const uint32_t hi2 = w[0] & 0x33333333u;
    const uint32_t lo4 = ((w[1] & 0x33333333u) << 2) | (w[2] & 0x33333333u);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint64_t code = (((hi2 >> (4 * r)) & 3u) << 4) | ((lo4 >> (4 * r)) & 15u);
        key[r] = (key[r] << 6) | code;
    }
}

// bit 4r: read r of the 8 reads of dword t exists (reads beyond n_reads are padding, not damaged reads)
__device__ __forceinline__ uint32_t valid_reads8(uint64_t t, uint64_t n_reads)
{
    uint32_t valid = 0;
#pragma unroll
    for (int r = 0; r < 8; ++r)
        if (t * 8u + r < n_reads) valid |= 1u << (4 * r);
    return valid;
}

// One lane = 8 consecutive reads = one byte of each plane of every variant column, put back together as a dword of eight codes.
__global__ __launch_bounds__(256) void phase_keys_kernel(const uint8_t *__restrict__ msa, uint64_t plane_stride,
                                                          uint64_t n_reads, uint64_t reads_pad,
                                                          const uint32_t *__restrict__ vpcols,
                                                          jl_phase_meta *__restrict__ meta,
                                                          uint64_t *__restrict__ keys, uint32_t *__restrict__ flagw)
{
    const uint32_t vp = meta->vp;
    if (vp == 0) return;   // (a context on the multi-word pipeline takes it for every run, whatever the run's key width)
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;  // byte index within a plane
    const bool live = t < plane_stride;
    uint32_t gap = 0, het = 0, par = 0;
    const uint32_t kwords = meta->kwords;
    for (uint32_t gw = 0; gw < kwords; ++gw) {
        uint64_t key[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const uint32_t p0 = gw * JL_POS_PER_WORD;
        const uint32_t p1 = min(vp, p0 + JL_POS_PER_WORD);
        for (uint32_t p = p0; p < p1; ++p) {
            const uint32_t c = vpcols[p];
            uint32_t w[3];
#pragma unroll
            for (int k = 0; k < 3; ++k)
                w[k] = live ? jl_load_codes8(msa + (uint64_t)(c + k) * 3u * plane_stride + t, plane_stride) : 0x66666666u;
            key_add_position(w, gap, het, par, key);
        }
        if (live) {
            uint64_t *dst = keys + (uint64_t)gw * reads_pad + t * 8u;
#pragma unroll
            for (int r = 0; r < 8; r += 2) {
                ulonglong2 v;
                v.x = key[r];
                v.y = key[r + 1];
                *reinterpret_cast<ulonglong2 *>(dst + r) = v;
            }
        }
    }
    const uint32_t valid = live ? valid_reads8(t, n_reads) : 0u;
    gap &= valid; het &= valid; par &= valid;
    if (live) flagw[t] = gap | (het << 1) | (par << 2) | ((valid ^ kM1) << 3);  // bit3: padding
    const uint32_t n_gap = wave_sum_all(__popc(gap));
    const uint32_t n_het = wave_sum_all(__popc(het));
    const uint32_t n_par = wave_sum_all(__popc(par));
    const uint32_t n_dam = wave_sum_all(__popc(gap | het | par));
    if ((threadIdx.x & 63u) == 0) {
        if (n_dam) atomicAdd(&meta->summary.damaged_reads, n_dam);
        if (n_gap) atomicAdd(&meta->summary.marginal_gap, n_gap);
        if (n_het) atomicAdd(&meta->summary.marginal_heteroduplex, n_het);
        if (n_par) atomicAdd(&meta->summary.marginal_partial, n_par);
    }
}

// ---------------------------------------------------------------------------------------- group
__device__ __forceinline__ bool keys_equal(const uint64_t *__restrict__ keys, uint64_t reads_pad, uint32_t kwords,
                                           uint64_t i, uint64_t j)
{
    for (uint32_t g = 0; g < kwords; ++g)
        if (keys[(uint64_t)g * reads_pad + i] != keys[(uint64_t)g * reads_pad + j]) return false;
    return true;
}

__global__ __launch_bounds__(256) void phase_group_kernel(jl_win_phase w)
{
    const uint64_t reads_pad = w.reads_pad, slots_mask = w.slots_mask;
    const uint64_t *__restrict__ keys = w.keys;
    const uint32_t kwords = w.meta->kwords;
    if (kwords == 0) return;  // nothing to phase
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    bool active = false;
    uint64_t k0 = 0;
    if (i < w.n_reads) {
        const uint32_t f = (w.flagw[i >> 3] >> (4u * (uint32_t)(i & 7u))) & 15u;
        active = f == 0;
        if (active) k0 = keys[i];
    }
    uint64_t todo = __ballot(active);
    while (todo) {  // wave-uniform: one iteration per distinct key in the wave
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const uint64_t lk0 = __shfl(k0, leader, 64);
        const uint64_t li = __shfl(i, leader, 64);
        bool same = active && k0 == lk0;
        if (same && kwords > 1) {
            for (uint32_t g = 1; g < kwords; ++g)
                if (keys[(uint64_t)g * reads_pad + i] != keys[(uint64_t)g * reads_pad + li]) { same = false; break; }
        }
        const uint64_t grp = __ballot(same);
        uint32_t slot = 0;
        if ((int)lane == leader) {
            uint64_t h = mix64(k0 + 0x9E3779B97F4A7C15ull);
            for (uint32_t g = 1; g < kwords; ++g) h = mix64(h ^ keys[(uint64_t)g * reads_pad + i]);
            uint64_t s = h & slots_mask;
            const uint32_t cnt = (uint32_t)__popcll(grp);
            for (;;) {
                uint32_t rep = __hip_atomic_load(&w.slot_rep[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (rep == kEmpty) {
                    rep = atomicCAS(&w.slot_rep[s], kEmpty, (uint32_t)i);
                    if (rep == kEmpty) {
                        w.occupied[atomicAdd(&w.meta->n_occupied, 1u)] = (uint32_t)s;
                        rep = (uint32_t)i;
                    }
                }
                if (rep == (uint32_t)i || keys_equal(keys, reads_pad, kwords, rep, i)) {
                    atomicAdd(&w.slot_count[s], cnt);
                    break;
                }
                s = (s + 1u) & slots_mask;
            }
            slot = (uint32_t)s;
        }
        slot = __shfl(slot, leader, 64);
        if (same) {
            w.read_slot[i] = slot;
            active = false;
        }
        todo &= ~grp;
    }
}

// width of the per-read ids for H reported haplotypes (jl_internal.h: JL_ID4_MAX_H / JL_ID8_MAX_H)
__device__ __forceinline__ uint32_t id_bits_for(uint32_t H) { return H <= JL_ID4_MAX_H ? 4u : (H <= JL_ID8_MAX_H ? 8u : 16u); }

// ---------------------------------------------------------------------------------------- patterns
// the one decode: the 6-bit code of position i of the n positions a key word holds (the first is the most significant)
__device__ __forceinline__ uint32_t key_code(uint64_t word, uint32_t n, uint32_t i) { return (uint32_t)(word >> (6u * (n - 1u - i))) & 63u; }
// position p of a vp-position pattern, out of the word that holds it (word p / JL_POS_PER_WORD, full but for the last)
__device__ __forceinline__ uint32_t word_code(uint64_t word, uint32_t vp, uint32_t p)
{
    const uint32_t g = p / JL_POS_PER_WORD;
    return key_code(word, min(JL_POS_PER_WORD, vp - g * JL_POS_PER_WORD), p - g * JL_POS_PER_WORD);
}
// the same for a pattern of up to 20 positions whose two words are at hand: positions 0..9 in w0, the rest in w1
__device__ __forceinline__ uint32_t key_code2(uint64_t w0, uint64_t w1, uint32_t vp, uint32_t p)
{
    const uint32_t n0 = vp < JL_POS_PER_WORD ? vp : JL_POS_PER_WORD;
    return p < n0 ? key_code(w0, n0, p) : key_code(w1, vp - n0, p - n0);
}

// leave the table empty for the next run: only the slots this run touched.  All threads of the block; no barrier.
__device__ __forceinline__ void empty_slot(const jl_win_phase &w, uint32_t s) { w.slot_key[s] = ~0ull; w.slot_rep[s] = 0xFFFFFFFFu; w.slot_count[s] = 0; }
__device__ __forceinline__ void empty_used_slots(const jl_win_phase &w, uint32_t n_occ)
{
    for (uint32_t q = threadIdx.x; q < n_occ; q += blockDim.x) empty_slot(w, jl_ld_coherent(&w.occupied[q]));
}

// ---------------------------------------------------------------------------------------- select
// code of position p of the pattern of group `id` (BYKEY: a table slot, else a read that carries the pattern)
template <bool BYKEY>
__device__ __forceinline__ uint32_t pattern_code(const jl_win_phase &w, uint32_t vp, uint32_t id, uint32_t p)
{
    const uint64_t k = BYKEY ? (uint64_t)jl_ld_coherent64(&w.slot_key[id])
                             : w.keys[(uint64_t)(p / JL_POS_PER_WORD) * w.reads_pad + id];
    return word_code(k, vp, p);
}

// Block-level (any block size that is a multiple of 64): groups with >= min_reads ranked by (count desc, pattern asc),
// haplotype ids, patterns, hit matrix, co-occurrence, the result block, and emptying of the table slots the run used.
// Every table / key / meta word it reads was written by other workgroups: the caller has acquired them.
// BYKEY: single-word pipeline — a group's pattern is its 64-bit table key (coherent: written by CAS), so no
// representative read has to be looked up in the key buffer another workgroup may have written in this launch.
// Everything but the LDS comes from the window's argument block.
#define JL_SELECT_LDS_WORDS (JL_CAND_CAP + 704u)
struct select_lds {   // the caller's LDS (the fused launch lends the tables its grouping is done with, and has no caches)
    uint32_t *scratch;               // [JL_SELECT_LDS_WORDS]
    uint32_t *cache;                 // [2 * JL_CAND_CAP] or null: see below
    unsigned long long *key_cache;   // [key_cache_words] or null
    uint32_t key_cache_words;
};

template <bool BYKEY>
__device__ __forceinline__ void phase_select_block(const jl_win_phase &w, const select_lds &lds)
{
    const jl_select_args &S = w.S;
    jl_phase_meta *meta = w.meta;
    uint32_t *s_cand = lds.scratch;                       // [JL_CAND_CAP] slot of each candidate
    uint32_t *s_hrep = lds.scratch + JL_CAND_CAP;         // [JL_MAX_HAPLOTYPES]
    uint32_t *const cache = lds.cache;
    unsigned long long *const key_cache = lds.key_cache;
    __shared__ uint32_t s_ncand, s_insufficient, s_reported, s_nhap;
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    const uint32_t vp = jl_ld_coherent(&meta->vp);
    const uint32_t kwords = jl_ld_coherent(&meta->kwords);
    const uint32_t nv = jl_ld_coherent(&meta->n_var);
    const uint32_t n_occ = jl_ld_coherent(&meta->n_occupied);
    if (vp != 0 && S.exp_count) {  // block-uniform: the groups go out as they are (see jl_select_args)
        if (tid == 0) s_insufficient = 0;
        __syncthreads();
        for (uint32_t q = tid; q < n_occ; q += nt) {
            const uint32_t s = jl_ld_coherent(&w.occupied[q]);
            const uint32_t c = jl_ld_coherent(&w.slot_count[s]);
            atomicAdd(&s_insufficient, c);
            // the slot remembers WHICH exported group it is: the merge answers per group (jl_phase_regroup, jl_xwin_phase_sharded)
            __hip_atomic_store(&S.slot_hap[s], q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (q < S.exp_cap) {
                S.exp_count[q] = c;
                // the group's key words once each, its row of codon codes stored 8 bytes at a time (exp_stride is a multiple
                // of 8: the rows may lie in pinned host memory, where every store is a transaction of its own)
                const uint32_t rep = BYKEY ? s : jl_ld_coherent(&w.slot_rep[s]);
                uint64_t word = 0;
                uint32_t have = 0xFFFFFFFFu;
                for (uint32_t p8 = 0; p8 < vp; p8 += 8u) {
                    unsigned long long out = 0;
                    for (uint32_t j = 0; j < 8u && p8 + j < vp; ++j) {
                        const uint32_t p = p8 + j, g = p / JL_POS_PER_WORD;
                        if (g != have) {
                            word = BYKEY ? (uint64_t)jl_ld_coherent64(&w.slot_key[s]) : w.keys[(uint64_t)g * w.reads_pad + rep];
                            have = g;
                        }
                        out |= (unsigned long long)word_code(word, vp, p) << (8u * j);
                    }
                    *reinterpret_cast<unsigned long long *>(S.exp_pattern + (uint64_t)q * S.exp_stride + p8) = out;
                }
            }
        }
        __syncthreads();
        if (tid == 0) {
            if (n_occ > S.exp_cap) meta->overflow |= JL_PHASE_OVF_EXPORT;
            meta->summary.reported_reads = 0;
            meta->summary.insufficient_reads = s_insufficient;   // clean reads: the merge decides which are reported
            meta->summary.n_haplotypes = 0;
            __hip_atomic_store(&meta->id_bits, 16u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (S.exp_head) {   // the scalars a merge needs, next to the groups (pinned host memory or an all-gather's send buffer)
                S.exp_head[0] = n_occ; S.exp_head[1] = vp; S.exp_head[2] = n_occ > S.exp_cap ? 1u : 0u;
                S.exp_head[3] = jl_ld_coherent(&meta->summary.damaged_reads); S.exp_head[4] = jl_ld_coherent(&meta->summary.marginal_gap);
                S.exp_head[5] = jl_ld_coherent(&meta->summary.marginal_heteroduplex); S.exp_head[6] = jl_ld_coherent(&meta->summary.marginal_partial);
                S.exp_head[7] = s_insufficient;
            }
        }
    } else if (vp != 0) {  // block-uniform
    if (tid == 0) { s_ncand = 0; s_insufficient = 0; s_reported = 0; s_nhap = 0; }
    __syncthreads();
    for (uint32_t q = tid; q < n_occ; q += nt) {
        const uint32_t s = jl_ld_coherent(&w.occupied[q]);
        const uint32_t c = jl_ld_coherent(&w.slot_count[s]);
        if (c >= S.min_reads) {
            const uint32_t k = atomicAdd(&s_ncand, 1u);
            if (k < JL_CAND_CAP) s_cand[k] = s;
            else { atomicAdd(&s_insufficient, c); __hip_atomic_store(&S.slot_hap[s], (uint32_t)JL_HAP_INSUFFICIENT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
        } else {
            atomicAdd(&s_insufficient, c);
            __hip_atomic_store(&S.slot_hap[s], (uint32_t)JL_HAP_INSUFFICIENT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    uint32_t ncand = s_ncand;
    if (ncand > JL_CAND_CAP) {
        if (tid == 0) meta->overflow |= JL_PHASE_OVF_CANDIDATES;
        ncand = JL_CAND_CAP;
    }
    // `cache` (2 * JL_CAND_CAP words of LDS, the general launch has them): every candidate's count and representative
    // once, instead of a trip past the L1 per comparison (300 candidates: 104 us of a 234 us run)
    uint32_t *s_ccnt = cache, *s_crep = cache ? cache + JL_CAND_CAP : nullptr;
    if (cache) {
        for (uint32_t a = tid; a < ncand; a += nt) {
            const uint32_t sa = s_cand[a];
            s_ccnt[a] = jl_ld_coherent(&w.slot_count[sa]);
            s_crep[a] = BYKEY ? sa : jl_ld_coherent(&w.slot_rep[sa]);
        }
        __syncthreads();
    }
    // ... and, when they fit, the candidates' keys: equal counts are common among the small groups, and every tie was two
    // more trips to the key buffer
    const bool keys_lds = !BYKEY && cache && key_cache && (uint64_t)ncand * kwords <= lds.key_cache_words;
    if (keys_lds) {
        for (uint32_t q = tid; q < ncand * kwords; q += nt) {
            const uint32_t a = q / kwords, g = q - a * kwords;
            key_cache[q] = w.keys[(uint64_t)g * w.reads_pad + s_crep[a]];
        }
        __syncthreads();
    }
    // rank sort: (count desc, pattern asc); patterns are unique so ranks are a permutation
    for (uint32_t a = tid; a < ncand; a += nt) {
        const uint32_t sa = s_cand[a], ca = cache ? s_ccnt[a] : jl_ld_coherent(&w.slot_count[sa]);
        const uint32_t ra = cache ? s_crep[a] : (BYKEY ? sa : jl_ld_coherent(&w.slot_rep[sa]));
        uint32_t rank = 0;
        if (cache && (BYKEY || keys_lds)) {
            // everything the comparison needs sits in LDS: one pass without a trip to memory
            const uint64_t ka0 = BYKEY ? jl_ld_coherent64(&w.slot_key[sa]) : key_cache[a * kwords];
            // eight candidates per trip, count and first key word of each read unconditionally (independent LDS reads in
            // flight: one at a time behind a data-dependent branch was 380 cycles per candidate, and equal counts are the
            // rule among small groups); only equal counts AND equal first words go on to the remaining words
            // (the caches arrive as generic pointers: typed as LDS here, or every read is a flat load)
            typedef __attribute__((address_space(3))) const uint32_t lds_u32;
            typedef __attribute__((address_space(3))) const unsigned long long lds_u64;
            lds_u32 *l_ccnt = (lds_u32 *)s_ccnt;
            lds_u32 *l_cand = (lds_u32 *)s_cand;
            lds_u64 *l_key = (lds_u64 *)key_cache;
            for (uint32_t b0 = 0; b0 < ncand; b0 += 8u) {
                uint32_t cb[8];
                uint64_t kb[8];
#pragma unroll
                for (uint32_t j = 0; j < 8u; ++j) {
                    const uint32_t b = b0 + j < ncand ? b0 + j : a;
                    cb[j] = l_ccnt[b];
                    kb[j] = BYKEY ? jl_ld_coherent64(&w.slot_key[l_cand[b]]) : l_key[b * kwords];
                }
                uint32_t ties = 0;
#pragma unroll
                for (uint32_t j = 0; j < 8u; ++j) {
                    const bool live = b0 + j < ncand && b0 + j != a;
                    rank += (live && (cb[j] > ca || (cb[j] == ca && kb[j] < ka0))) ? 1u : 0u;
                    ties |= (live && cb[j] == ca && kb[j] == ka0) ? 1u << j : 0u;
                }
                while (!BYKEY && ties) {   // same count, same first ten positions: the later words decide
                    const uint32_t b = b0 + (uint32_t)__ffs((int)ties) - 1u;
                    ties &= ties - 1u;
                    for (uint32_t g = 1; g < kwords; ++g) {
                        const uint64_t ka = key_cache[a * kwords + g], kbg = key_cache[b * kwords + g];
                        if (kbg != ka) { rank += kbg < ka ? 1u : 0u; break; }
                    }
                }
            }
        } else
        for (uint32_t b = 0; b < ncand; ++b) {
            if (b == a) continue;
            const uint32_t sb = s_cand[b], cb = cache ? s_ccnt[b] : jl_ld_coherent(&w.slot_count[sb]);
            if (cb > ca) { ++rank; continue; }
            if (cb < ca) continue;
            if (BYKEY) {
                const uint64_t ka = jl_ld_coherent64(&w.slot_key[sa]);
                const uint64_t kb = jl_ld_coherent64(&w.slot_key[sb]);
                if (kb < ka) ++rank;
                continue;
            }
            const uint32_t rb = cache ? s_crep[b] : jl_ld_coherent(&w.slot_rep[sb]);
            for (uint32_t g = 0; g < kwords; ++g) {
                const uint64_t ka = w.keys[(uint64_t)g * w.reads_pad + ra], kb = w.keys[(uint64_t)g * w.reads_pad + rb];
                if (kb != ka) { if (kb < ka) ++rank; break; }
            }
        }
        if (rank < JL_MAX_HAPLOTYPES) {
            S.hap_count[rank] = ca;
            s_hrep[rank] = ra;  // BYKEY: the slot, else a read carrying the pattern
            __hip_atomic_store(&S.slot_hap[sa], rank, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // write-through: read by other workgroups
            atomicAdd(&s_reported, ca);
            atomicAdd(&s_nhap, 1u);
        } else {
            __hip_atomic_store(&S.slot_hap[sa], (uint32_t)JL_HAP_INSUFFICIENT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            atomicAdd(&s_insufficient, ca);
        }
    }
    __syncthreads();
    const uint32_t H = s_nhap;
    if (tid == 0) {
        if (ncand > JL_MAX_HAPLOTYPES) meta->overflow |= JL_PHASE_OVF_HAPLOTYPES;
        meta->summary.reported_reads = s_reported;
        meta->summary.insufficient_reads = s_insufficient;
        meta->summary.n_haplotypes = H;
        __hip_atomic_store(&meta->id_bits, id_bits_for(H), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (uint32_t q = tid; q < H * vp; q += nt) {
        const uint32_t h = q / vp, p = q - h * vp;
        S.hap_pattern[(uint64_t)h * JL_VARIANT_CAP + p] = (uint8_t)pattern_code<BYKEY>(w, vp, s_hrep[h], p);
    }
    // With the cache (free again after the ranking) the co-occurrence sums run out of LDS: the haplotype counts and, per
    // variant, the set of haplotypes that carry it as a bit mask — filled by the hit loop below.  (Summing over two
    // global hit rows per pair was most of this launch at 49 variants x 125 haplotypes: 98 us.)
    const uint32_t nvc_l = nv < S.cooc_cap ? nv : S.cooc_cap;
    constexpr uint32_t kHapWords = (JL_MAX_HAPLOTYPES + 31u) / 32u;
    const bool cooc_lds = cache && (uint64_t)nvc_l * kHapWords + 1024u <= 2u * JL_CAND_CAP;
    uint32_t *s_hc = cache, *s_bits = cache ? cache + 1024 : nullptr;   // [JL_MAX_HAPLOTYPES <= 1024], [nvc][kHapWords]
    if (cooc_lds) {
        __syncthreads();   // every thread is done with the ranking's use of the cache
        for (uint32_t q = tid; q < nvc_l * kHapWords; q += nt) s_bits[q] = 0;
        __syncthreads();
    }
    for (uint32_t q = tid; q < nv * H; q += nt) {
        const uint32_t v = q / H, h = q - v * H;
        // BYKEY: the table (and col2pos) may come from another workgroup of this launch
        const uint32_t c = BYKEY ? jl_ld_coherent(&S.variants[v].col) : S.variants[v].col;
        uint8_t x = 0;
        if (c + 2u < S.n_cols) {  // rows outside this window never hit
            const uint32_t p = BYKEY ? jl_ld_coherent(&S.col2pos[c]) : S.col2pos[c];
            // ref_codon / codon / flags share one dword
            const uint32_t cw = BYKEY ? jl_ld_coherent(reinterpret_cast<const uint32_t *>(&S.variants[v]) + 3) : 0u;
            const uint32_t codon = BYKEY ? ((cw >> 8) & 0xFFu) : (uint32_t)S.variants[v].codon;
            x = pattern_code<BYKEY>(w, vp, s_hrep[h], p) == codon;
        }
        S.hit[(uint64_t)v * JL_MAX_HAPLOTYPES + h] = x;
        if (cooc_lds && x && v < nvc_l) atomicOr(&s_bits[v * kHapWords + (h >> 5)], 1u << (h & 31u));
    }
    __syncthreads();
    // co-occurrence over the reported haplotypes, for the first cooc_cap variants
    if (cooc_lds) {
        for (uint32_t h = tid; h < H; h += nt) s_hc[h] = S.hap_count[h];
        __syncthreads();
        for (uint32_t q = tid; q < nvc_l * nvc_l; q += nt) {
            const uint32_t v = q / nvc_l, w = q - v * nvc_l;
            uint32_t sum = 0;
            for (uint32_t j = 0; j < (H + 31u) / 32u; ++j) {
                uint32_t m = s_bits[v * kHapWords + j] & s_bits[w * kHapWords + j];
                while (m) {
                    sum += s_hc[32u * j + (uint32_t)__ffs((int)m) - 1u];
                    m &= m - 1u;
                }
            }
            S.cooc[(uint64_t)v * S.cooc_cap + w] = sum;
        }
    } else {
        const uint32_t nvc = nvc_l;
        for (uint32_t q = tid; q < nvc * nvc; q += nt) {
            const uint32_t v = q / nvc, w = q - v * nvc;
            uint32_t sum = 0;
            for (uint32_t h = 0; h < H; ++h)
                if (S.hit[(uint64_t)v * JL_MAX_HAPLOTYPES + h] && S.hit[(uint64_t)w * JL_MAX_HAPLOTYPES + h]) sum += S.hap_count[h];
            S.cooc[(uint64_t)v * S.cooc_cap + w] = sum;
        }
    }
    } else if (tid == 0) {
        __hip_atomic_store(&meta->id_bits, 4u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // nothing phased: every read is "damaged"
        if (S.exp_head) {
            S.exp_head[0] = 0; S.exp_head[1] = 0; S.exp_head[2] = 0;
            S.exp_head[3] = 0; S.exp_head[4] = 0; S.exp_head[5] = 0; S.exp_head[6] = 0; S.exp_head[7] = 0;
        }
    }
    __syncthreads();
    // device copy double-buffered by the parity of the run index (an exchange may still read run n's block while
    // run n+1 writes its own); an exporting run has no result block: its groups ARE the result
    if (!S.exp_count) {
        jl_pack *pk = S.pk + (__hip_atomic_load(S.seq_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 1u);
        jl_result_pack_block(S.variants, jl_ld_coherent(&S.n_rows[0]), meta, 1u, w.vpcols, S.hap_count, S.hap_pattern, S.hit, S.cooc,
                             S.cooc_cap, 1u, pk, S.mirror, BYKEY);
    }
    empty_used_slots(w, n_occ);
}

// The multi-word pipeline's selection.  The argument block travels by value, i.e. in the kernel-argument segment (see the
// comment above JL_GROUP_MAX: pointers loaded from there are known to be global ones).
__global__ __launch_bounds__(1024) void phase_select_kernel(jl_win_phase w)
{
    __shared__ uint32_t s_select[JL_SELECT_LDS_WORDS];
    __shared__ uint32_t s_cache[2u * JL_CAND_CAP];
    __shared__ unsigned long long s_keys[2048];
    phase_select_block<false>(w, select_lds{s_select, s_cache, s_keys, 2048u});
    if (w.S.seq_host) {  // last kernel of the run: the result block is on its way to the host
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) jl_signal_done(w.S.seq_dev, w.S.seq_host);
    }
}

// ---------------------------------------------------------------------------------------- fused keys + group
// Vp <= 10: the whole pattern is ONE 64-bit word, so the table can be keyed by value (64-bit CAS, no
// representative lookup) and a block can aggregate before it touches HBM:
//   0. (whole-path runs) every workgroup derives the variant columns from the call masks the Fisher stage left
//      (a few KB, L2-resident) — no launch or workgroup hand-off between calling and phasing; one EXTRA workgroup
//      meanwhile compacts the called rows into the ordered table,
//   1. every lane builds the keys and flags of its 8 reads (30 independent dword loads in flight),
//   2. the block's dominant key (that of its first clean read — the wild type for all but pathological
//      inputs) is counted with popcount-style compares and costs ONE global insert per block,
//   3. the remaining clean reads go through an LDS table (CAS on the 64-bit key), which is then flushed
//      with one global insert per distinct key per block.
// Global atomics on the hot slot drop from one per wave to one per 2048 reads.
constexpr uint32_t kLdsSlots = 1024;
constexpr uint64_t kNoKey = ~0ull;
constexpr uint32_t kPlanList = 256;   // called positions a workgroup can rank in LDS; more take the multi-word pipeline

struct plan_state {   // LDS: what the prologue derives — identical in every workgroup of a window
    uint32_t n_list, n_rows, vp, ovf;
    uint32_t cols[2u * JL_POS_PER_WORD];   // the variant columns, ascending (first 20: two key words)
    uint32_t list[kPlanList];
    uint8_t first[kPlanList];
};

// Distinct start columns of the called positions, ascending, from the call masks (SPEC §8).  All 256 threads.
__device__ __forceinline__ void plan_prologue(const jl_select_args &S, uint32_t n_cols, plan_state &L)
{
    const uint32_t tid = threadIdx.x;
    if (tid == 0) { L.n_list = 0; L.n_rows = 0; L.vp = 0; L.ovf = 0; }
    if (tid < 2u * JL_POS_PER_WORD) L.cols[tid] = 0;
    __syncthreads();
    const uint32_t P = S.P;
    for (uint32_t base = 0; base < P; base += 1024u) {
        unsigned long long m[4];
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {   // four independent loads in flight per lane
            const uint32_t q = base + k * 256u + tid;
            m[k] = q < P ? S.called[q] : 0ull;
        }
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            if (m[k]) {
                const uint32_t c = S.pos_col[base + k * 256u + tid];
                atomicAdd(&L.n_rows, (uint32_t)__popcll(m[k]));
                if (c + 2u < n_cols) {
                    const uint32_t i = atomicAdd(&L.n_list, 1u);
                    if (i < kPlanList) L.list[i] = c;
                }
            }
        }
    }
    __syncthreads();
    const uint32_t n = min(L.n_list, kPlanList);
    if (tid < n) {   // first occurrence of its column? (overlapping genes in one frame call the same column twice)
        const uint32_t c = L.list[tid];
        bool f = true;
        for (uint32_t j = 0; j < tid; ++j) f = f && L.list[j] != c;
        L.first[tid] = f;
    }
    __syncthreads();
    if (tid < n && L.first[tid]) {
        const uint32_t c = L.list[tid];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n; ++j) rank += (L.first[j] && L.list[j] < c) ? 1u : 0u;
        if (rank < 2u * JL_POS_PER_WORD) L.cols[rank] = c;
        atomicAdd(&L.vp, 1u);
    }
    if (tid == 0 && L.n_list > kPlanList) L.ovf = 1u;
    __syncthreads();
}

// Selection of the single-word pipeline out of LDS: every table word it needs is fetched ONCE (occupied list -> counts
// and keys: two dependent round trips), ranking, patterns, hit matrix and co-occurrence then run on LDS copies, and
// the result block is stored from there.  The general routine above chases each of them through memory again (a
// dozen dependent round trips on one CU: 10 us and more).  Handles what fits the result block (<= 128 candidates,
// <= 128 variant rows, hit matrix <= 4 KB); returns false — with nothing but idempotent side effects — otherwise.
// the half-key tables of a two-word launch, emptied of what the run put there (and their counters)
__device__ __forceinline__ void two_word_cleanup(const jl_two_word &tw)
{
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    const uint32_t na = jl_ld_coherent(&tw.n_occ[0]), nb = jl_ld_coherent(&tw.n_occ[1]);
    for (uint32_t q = tid; q < na; q += nt) tw.key_a[jl_ld_coherent(&tw.occ_a[q])] = ~0ull;
    for (uint32_t q = tid; q < nb; q += nt) tw.key_b[jl_ld_coherent(&tw.occ_b[q])] = ~0ull;
    __syncthreads();
    if (tid == 0) { tw.n_occ[0] = 0; tw.n_occ[1] = 0; }
}

constexpr uint32_t kSelCand = JL_PACK_MAX_HAP;
struct sel_lds {
    uint32_t slot[kSelCand], cnt[kSelCand];
    unsigned long long key[kSelCand], key1[kSelCand];     // key1 / hkey1: the second word of a two-word pattern
    uint32_t hcnt[kSelCand];
    unsigned long long hkey[kSelCand], hkey1[kSelCand];
    uint32_t vpos[JL_PACK_MAX_VAR];   // per variant row: how its position reads out of a pattern (see the selection)
    uint8_t hit[JL_SEL_HIT_BYTES];
    uint32_t hmask[JL_PACK_MAX_VAR][kSelCand / 32u];   // per variant: the haplotypes that carry it (co-occurrence sums)
    uint32_t ncand, insufficient, reported, bail;
};
static_assert(sizeof(sel_lds) <= kLdsSlots * 5u * 4u, "the selection's scratch must fit the grouping tables");
static_assert(offsetof(sel_lds, hmask) % 8 == 0, "a variant's haplotype set is read as two 64-bit words");

// All the LDS of a workgroup of the fused launch; NS table sets.  One set = the grouping tables (8 + 3 x 4 KB), lent to the
// selection once the grouping is done.  The two-word launch has two sets: its first two rounds — the two words of the
// patterns, independent of each other — run together, one set each.
template <uint32_t NS>
struct fused_lds {
    unsigned long long tables[NS][kLdsSlots * 5u / 2u];
    plan_state plan;
    unsigned long long dom[NS];                             // dominant key of the block, per set
    uint32_t domcnt[NS], domfirst, domslot[NS], nlist[NS];
    uint32_t last, cat[4], idbits, scan[4], running;
    uint16_t list[NS][kLdsSlots];                           // the occupied slots of a set, densely
    // a set's four tables, [kLdsSlots] each
    __device__ __forceinline__ unsigned long long *key(uint32_t z) { return tables[z]; }
    __device__ __forceinline__ uint32_t *cnt(uint32_t z) { return reinterpret_cast<uint32_t *>(tables[z] + kLdsSlots); }
    __device__ __forceinline__ uint32_t *first(uint32_t z) { return cnt(z) + kLdsSlots; }
    __device__ __forceinline__ uint32_t *gslot(uint32_t z) { return cnt(z) + 2u * kLdsSlots; }
    // what the selections take of set 0 once the grouping is done
    __device__ __forceinline__ sel_lds &selection() { return *reinterpret_cast<sel_lds *>(tables[0]); }
    // Empties the first n_sets sets and their dominant-key words.  All 256 threads; no barrier: the caller's follows.
    __device__ __forceinline__ void clear_sets(uint32_t n_sets)
    {
        const uint32_t tid = threadIdx.x;
        for (uint32_t z = 0; z < n_sets; ++z) {
            for (uint32_t i = tid; i < kLdsSlots; i += 256u) { key(z)[i] = kNoKey; cnt(z)[i] = 0; first(z)[i] = 0xFFFFFFFFu; }
            if (tid == 0) { dom[z] = kNoKey; domcnt[z] = 0; domslot[z] = 0; nlist[z] = 0; }
        }
        if (tid == 0) domfirst = 0xFFFFFFFFu;
    }
};

// what the last workgroup requests for the selection beside the read categories, one round trip for all of it
struct select_pre {
    uint32_t nv, n_rows;      // rows of the variant table in use / in all
    uint32_t n_occ, occ0;     // the group count and this thread's first entry of the group list (only meaningful below n_occ)
};

// KW = 2: the main table's key of a group is the pair (slot of its first word in table A, slot of its second word in
// table B); the words themselves are one more round trip away (jl_two_word).
// `ranked(bits)`: called by every thread once the slot -> haplotype table is complete and performed (the ids depend on nothing
// else): the caller releases the workgroups that wait for it and writes its own reads' ids THERE, so that the rest of the
// selection — hit matrix, co-occurrence, result block: 3.5 us at five positions, 11 at sixteen — runs beside the other
// workgroups' ids instead of in front of them.
template <int KW, uint32_t NS, typename Ranked>
__device__ __forceinline__ bool phase_select_lds(const jl_win_phase &w, const jl_two_word *tw, fused_lds<NS> &F, uint32_t vp,
                                                 const select_pre &pre, uint32_t *id_bits_out, Ranked &&ranked)
{
    // of the LDS: the plan's columns, the scratch, and the read categories of the whole window (summed by the caller)
    const plan_state &L = F.plan;
    sel_lds &T = F.selection();
    const uint32_t *cat = F.cat;
    const uint32_t nv = pre.nv, n_rows = pre.n_rows, n_occ = pre.n_occ, occ0 = pre.occ0;
    const jl_select_args &S = w.S;
    jl_phase_meta *meta = w.meta;
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    if (tid == 0) { T.ncand = 0; T.insufficient = 0; T.reported = 0; T.bail = (nv > JL_PACK_MAX_VAR || n_rows > JL_PACK_MAX_VAR) ? 1u : 0u; }
    __syncthreads();
    if (T.bail) return false;
    // The groups, four per thread and trip: all of a thread's list entries are loaded before any is used, then all their
    // counts and keys (one dependent round trip per 1024 groups each way instead of one per 256: at 725 groups the scan was
    // a quarter of the selection).
    // Same-address LDS atomics serialise: one per non-candidate group (616 of 725 at sixteen positions) was most of the
    // scan.  The read counts of those groups add up in registers (one atomic per wave at the end); candidates are numbered
    // a wave at a time (ballot + one atomic per wave and trip).
    uint32_t insufficient = 0;
    const uint32_t lane = tid & 63u;
    uint32_t sl_keep[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};   // the first 1024 groups' slots: emptied from registers below
    // the two-word launch's half-key lists, for the same purpose: counts and each thread's first entries, requested now
    // ... and what the selection needs further down and does not depend on the groups: this thread's variant row and the
    // run counter (the parity of the result block) — requested here, beside the groups, instead of one round trip each later
    uint32_t row_c = 0, row_cw = 0;
    if (tid < nv) {
        const uint32_t *row = reinterpret_cast<const uint32_t *>(S.variants + tid);
        row_c = jl_ld_coherent(row + 2);
        row_cw = jl_ld_coherent(row + 3);
    }
    const uint32_t seq_pre = __hip_atomic_load(S.seq_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t tw_n[2] = {0, 0}, tw_first[2] = {0, 0};
    if (KW == 2) {
        tw_n[0] = jl_ld_coherent(&tw->n_occ[0]);
        tw_n[1] = jl_ld_coherent(&tw->n_occ[1]);
        tw_first[0] = jl_ld_coherent(&tw->occ_a[tid]);   // (the lists hold at least 256 entries; used below the counts only)
        tw_first[1] = jl_ld_coherent(&tw->occ_b[tid]);
    }
    for (uint32_t q0 = 0; q0 < n_occ; q0 += 4u * nt) {
        uint32_t sl[4], cn[4];
        unsigned long long ky[4];
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t q = q0 + j * nt + tid;
            sl[j] = q < n_occ ? ((q0 == 0u && j == 0u) ? occ0 : jl_ld_coherent(&w.occupied[q])) : 0xFFFFFFFFu;
        }
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            cn[j] = 0;
            ky[j] = 0;
            if (sl[j] != 0xFFFFFFFFu) {
                cn[j] = jl_ld_coherent(&w.slot_count[sl[j]]);
                ky[j] = jl_ld_coherent64(&w.slot_key[sl[j]]);
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const bool have = sl[j] != 0xFFFFFFFFu;
            const bool cand = have && cn[j] >= S.min_reads;
            const unsigned long long m = __ballot(cand);
            if (m) {   // wave-uniform
                uint32_t base = 0;
                const uint32_t leader = (uint32_t)__ffsll((long long)m) - 1u;
                if (lane == leader) base = atomicAdd(&T.ncand, (uint32_t)__popcll(m));
                base = (uint32_t)__shfl((int)base, (int)leader, 64);
                if (cand) {
                    const uint32_t i = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                    if (i < kSelCand) { T.slot[i] = sl[j]; T.cnt[i] = cn[j]; T.key[i] = ky[j]; }
                    else T.bail = 1u;
                }
            }
            if (have && !cand) {
                insufficient += cn[j];
                __hip_atomic_store(&S.slot_hap[sl[j]], (uint32_t)JL_HAP_INSUFFICIENT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (q0 == 0u) {
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) sl_keep[j] = sl[j];
        }
    }
    insufficient = wave_sum_all(insufficient);
    if (lane == 0 && insufficient) atomicAdd(&T.insufficient, insufficient);
    // the variant rows: column -> position index, codon (the table may come from another workgroup of this launch)
    for (uint32_t v = tid; v < nv; v += nt) {
        const uint32_t *row = reinterpret_cast<const uint32_t *>(S.variants + v);
        const uint32_t c = v == tid ? row_c : jl_ld_coherent(row + 2), cw = v == tid ? row_cw : jl_ld_coherent(row + 3);
        uint32_t pos = 0xFFu;
        if (c + 2u < S.n_cols)
            for (uint32_t p = 0; p < vp; ++p) pos = L.cols[p] == c ? p : pos;
        // how the hit loop reads this variant's position out of a pattern: bits 0-5 the shift, bit 6 the word, bits 8-15
        // the codon; bit 31: no such position
        const uint32_t n0 = vp < JL_POS_PER_WORD ? vp : JL_POS_PER_WORD;
        uint32_t e = 0x80000000u;
        if (pos != 0xFFu)
            e = (pos < n0 ? 6u * (n0 - 1u - pos) : (64u | (6u * (vp - n0 - 1u - (pos - n0))))) | (((cw >> 8) & 0xFFu) << 8);
        T.vpos[v] = e;
    }
    __syncthreads();
    const uint32_t H = T.ncand;
    if (T.bail || nv * H > JL_SEL_HIT_BYTES) return false;
    if (KW == 2) {   // the candidates' two words, from the half-key tables
        for (uint32_t a = tid; a < H; a += nt) {
            const unsigned long long pair = T.key[a];
            T.key[a] = jl_ld_coherent64(&tw->key_a[(uint32_t)(pair >> 32)]);
            T.key1[a] = jl_ld_coherent64(&tw->key_b[(uint32_t)pair]);
        }
        __syncthreads();
    }
    // Nothing below gives the run back to the general routine, and nothing reads the tables again: they are left empty for
    // the next run now (only the slots this run touched) — stores that go out beside the ranking instead of behind it.
    // (the first 1024 groups' slots are still in registers from the scan: stores only)
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j)
        if (sl_keep[j] != 0xFFFFFFFFu) empty_slot(w, sl_keep[j]);
    for (uint32_t q = 4u * nt + tid; q < n_occ; q += nt) empty_slot(w, jl_ld_coherent(&w.occupied[q]));
    if (KW == 2) {
        if (tid < tw_n[0]) tw->key_a[tw_first[0]] = ~0ull;
        if (tid < tw_n[1]) tw->key_b[tw_first[1]] = ~0ull;
        for (uint32_t q = nt + tid; q < tw_n[0]; q += nt) tw->key_a[jl_ld_coherent(&tw->occ_a[q])] = ~0ull;
        for (uint32_t q = nt + tid; q < tw_n[1]; q += nt) tw->key_b[jl_ld_coherent(&tw->occ_b[q])] = ~0ull;
        if (tid == 0) { tw->n_occ[0] = 0; tw->n_occ[1] = 0; }   // (every thread has its copy of the counts)
    }
    // rank: (count desc, pattern asc); patterns are unique, so the ranks are a permutation.  Two threads per candidate
    // (at most 128 of them, 256 threads): each counts the competitors of one half that come before it.
    uint32_t *half_rank = reinterpret_cast<uint32_t *>(T.hit);   // [kSelCand] scratch: the hit matrix is filled later
    uint32_t my_rank = 0;
    {
        const uint32_t a = tid & 127u;
        if (a < H) {
            const uint32_t ca = T.cnt[a];
            const unsigned long long ka = T.key[a], ka1 = KW == 2 ? T.key1[a] : 0ull;
            const uint32_t b0 = tid < 128u ? 0u : H / 2u, b1 = tid < 128u ? H / 2u : H;
            uint32_t r = 0;
            // eight competitors' words are on their way from LDS before the first is compared (one at a time the loop
            // waited out an LDS round trip per competitor: 8 us at 109 candidates)
            for (uint32_t b = b0; b < b1; b += 8u) {
                uint32_t cb[8];
                unsigned long long kb[8], kb1[8];
#pragma unroll
                for (uint32_t j = 0; j < 8u; ++j) {
                    const uint32_t i = b + j < b1 ? b + j : b1 - 1u;
                    cb[j] = T.cnt[i];
                    kb[j] = T.key[i];
                    kb1[j] = KW == 2 ? T.key1[i] : 0ull;
                }
#pragma unroll
                for (uint32_t j = 0; j < 8u; ++j) {
                    const bool before = KW == 2 ? (kb[j] < ka || (kb[j] == ka && kb1[j] < ka1)) : kb[j] < ka;
                    r += (b + j < b1 && (cb[j] > ca || (cb[j] == ca && before))) ? 1u : 0u;
                }
            }
            if (tid < 128u) my_rank = r;
            else half_rank[a] = r;
        }
    }
    __syncthreads();
    {   // (H <= 128: the threads that hold my_rank)
        uint32_t ca = 0;
        if (tid < H) {
            ca = T.cnt[tid];
            const unsigned long long ka = T.key[tid], ka1 = KW == 2 ? T.key1[tid] : 0ull;
            const uint32_t rank = my_rank + half_rank[tid];
            T.hcnt[rank] = ca;
            T.hkey[rank] = ka;
            if (KW == 2) T.hkey1[rank] = ka1;
            __hip_atomic_store(&S.slot_hap[T.slot[tid]], rank, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // read by other workgroups
        }
        const uint32_t rs = wave_sum_all(ca);
        if ((tid & 63u) == 0 && rs) atomicAdd(&T.reported, rs);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the table's stores, the scan's among them, are performed)
    __syncthreads();
    ranked(id_bits_for(H));
    // hit[v][h] and, per variant, the set of haplotypes that carry it as bits: a lane per haplotype (its pattern words in
    // registers), a wave per variant (no division per element; the set makes the co-occurrence sums a walk over a few
    // common bits instead of H terms).  Beside it the patterns as bytes, [h][p], in the scratch the ranking is done with.
    uint8_t *pat = reinterpret_cast<uint8_t *>(T.slot);
    static_assert(offsetof(sel_lds, hcnt) >= kSelCand * 2u * JL_POS_PER_WORD + 8u, "the pattern bytes reuse slot/cnt/key/key1");
    for (uint32_t h0 = 0; h0 < H; h0 += 64u) {
        const uint32_t h = h0 + (tid & 63u);
        const unsigned long long k0 = h < H ? T.hkey[h] : 0ull, k1 = (KW == 2 && h < H) ? T.hkey1[h] : 0ull;
        for (uint32_t v = tid >> 6; v < nv; v += nt >> 6) {
            const uint32_t e = T.vpos[v];   // (wave-uniform)
            const unsigned long long word = (KW == 2 && (e & 64u)) ? k1 : k0;
            const bool x = h < H && !(e & 0x80000000u) && ((uint32_t)(word >> (e & 63u)) & 63u) == ((e >> 8) & 0xFFu);
            if (h < H) T.hit[v * H + h] = x ? 1 : 0;
            const unsigned long long m = __ballot(x);
            if ((tid & 63u) == 0) { T.hmask[v][h0 / 32u] = (uint32_t)m; T.hmask[v][h0 / 32u + 1u] = (uint32_t)(m >> 32); }
        }
    }
    for (uint32_t h = tid & 127u; h < H; h += 128u) {   // (slot / cnt / key / key1 are dead: the ranks are out)
        const unsigned long long k0 = T.hkey[h], k1 = KW == 2 ? T.hkey1[h] : 0ull;
        for (uint32_t p = tid >> 7; p < vp; p += 2u) pat[h * vp + p] = (uint8_t)(KW == 2 ? key_code2(k0, k1, vp, p) : key_code(k0, vp, p));
    }
    if (tid < 8u) {   // whole 8-byte words leave below: their tails are zeros
        pat[H * vp + tid] = 0;
        if (nv * H + tid < JL_SEL_HIT_BYTES) T.hit[nv * H + tid] = 0;
    }
    __syncthreads();
    const uint32_t bits = id_bits_for(H);
    *id_bits_out = bits;   // (every thread: a register of the caller)
    const uint32_t nvc = nv < S.cooc_cap ? nv : S.cooc_cap;
    const bool cooc_fits = nv <= JL_PACK_COOC_N;
    // ---- outputs.  The resident arrays are what the stage-API fetches read; a whole-path run whose results fit the result
    // block is read from that block alone (jl_phase_fetch, jl_run_view_get), so they are not written then (byte stores
    // with a division each: 6 us of the 36 the selection took at sixteen positions) ...
    const bool resident = S.called == nullptr || !cooc_fits;
    if (resident) {
        for (uint32_t h = tid; h < H; h += nt) S.hap_count[h] = T.hcnt[h];
        for (uint32_t h = tid & 127u; h < H; h += 128u)
            for (uint32_t p = tid >> 7; p < vp; p += 2u) S.hap_pattern[(uint64_t)h * JL_VARIANT_CAP + p] = pat[h * vp + p];
        for (uint32_t v = tid >> 6; v < nv; v += nt >> 6)
            for (uint32_t h = tid & 63u; h < H; h += 64u) S.hit[(uint64_t)v * JL_MAX_HAPLOTYPES + h] = T.hit[v * H + h];
    }
    jl_pack *pk = S.pk + (seq_pre & 1u);
    jl_pack *dsts[2] = {pk, S.mirror};
    // Co-occurrence C[v][x] = sum over the haplotypes that carry both of their read counts.  The counts are cut into bit
    // planes (plane b = the haplotypes whose count has bit b set, as a 128-bit set): C = sum_b 2^b popcount(set_v & set_x &
    // plane_b) — a fixed two dozen words per pair, no walk over the common haplotypes (7 us at 38 variants x 109
    // haplotypes).  The matrix is symmetric: a thread per pair v <= x of the upper triangle.
    unsigned long long *plane = T.hkey;   // [32][2]: the patterns are out as bytes, their words are dead
    static_assert(sizeof(T.hkey) >= 32u * 2u * 8u && kSelCand == 128u, "the bit planes reuse hkey; a set is two 64-bit words");
    const uint32_t n_planes = 32u - (uint32_t)__clz((int)(T.hcnt[0] | 1u));   // rank 0 holds the largest count
    if (tid < 128u) {
        const uint32_t c = tid < H ? T.hcnt[tid] : 0u;
        for (uint32_t b = 0; b < n_planes; ++b) {
            const unsigned long long m = __ballot((c >> b) & 1u);
            if ((tid & 63u) == 0) plane[b * 2u + (tid >> 6)] = m;
        }
    }
    __syncthreads();
    const uint32_t n_pairs = nvc * (nvc + 1u) / 2u;
    for (uint32_t q = tid; q < n_pairs; q += nt) {
        // q -> (v, x) of the upper triangle, rows v = 0 .. nvc-1 of lengths nvc, nvc-1, ...: the row from the closed form
        // (single precision is exact enough below 2^24 pairs), then at most one step either way
        const float nn = 2.0f * (float)nvc + 1.0f;
        uint32_t v = (uint32_t)((nn - __fsqrt_rn(nn * nn - 8.0f * (float)q)) * 0.5f);
        if (v >= nvc) v = nvc - 1u;
        while (v > 0u && v * nvc - v * (v - 1u) / 2u > q) --v;
        while ((v + 1u) * nvc - (v + 1u) * v / 2u <= q) ++v;
        const uint32_t x = v + (q - (v * nvc - v * (v - 1u) / 2u));
        const unsigned long long *mv = reinterpret_cast<const unsigned long long *>(T.hmask[v]);
        const unsigned long long *mx = reinterpret_cast<const unsigned long long *>(T.hmask[x]);
        const unsigned long long a0 = mv[0] & mx[0], a1 = mv[1] & mx[1];
        uint32_t sum = 0;
        if (a0 | a1)
            for (uint32_t b = 0; b < n_planes; ++b)
                sum += (uint32_t)(__popcll(a0 & plane[b * 2u]) + __popcll(a1 & plane[b * 2u + 1u])) << b;
        if (resident) {
            S.cooc[(uint64_t)v * S.cooc_cap + x] = sum;
            S.cooc[(uint64_t)x * S.cooc_cap + v] = sum;
        }
        if (cooc_fits)
#pragma unroll
            for (int t = 0; t < 2; ++t)
                if (dsts[t]) { dsts[t]->cooc[v * nv + x] = sum; dsts[t]->cooc[x * nv + v] = sum; }
    }
    // ... and the result block, device copy (all-gather source) and pinned host mirror, straight from LDS, eight bytes a store
    if (tid == 0) {
        jl_phase_summary sm;
        sm.reported_reads = T.reported;
        sm.insufficient_reads = T.insufficient;
        sm.damaged_reads = cat[0];
        sm.marginal_gap = cat[1];
        sm.marginal_heteroduplex = cat[2];
        sm.marginal_partial = cat[3];
        sm.n_positions = vp;
        sm.n_haplotypes = H;
        meta->summary.reported_reads = sm.reported_reads;
        meta->summary.insufficient_reads = sm.insufficient_reads;
        meta->summary.n_haplotypes = H;
        meta->summary.n_positions = vp;
        __hip_atomic_store(&meta->id_bits, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            jl_pack *o = dsts[t];
            if (!o) continue;
            o->magic = JL_PACK_MAGIC; o->nvar_total = n_rows; o->fits_call = 1u; o->fits_phase = 1u;
            o->phase_ran = 1u; o->overflow = 0u; o->vp = vp; o->H = H;
            o->nv_phase = nv; o->cooc_fits = cooc_fits ? 1u : 0u; o->id_bits = bits;
            o->summary = sm;
        }
    }
    static_assert(offsetof(jl_pack, hap_pattern) % 8 == 0 && offsetof(jl_pack, hit) % 8 == 0 && offsetof(jl_pack, hap_count) % 8 == 0 &&
                  offsetof(jl_pack, variants) % 8 == 0 && offsetof(sel_lds, hit) % 8 == 0 && offsetof(sel_lds, hcnt) % 8 == 0,
                  "the result block's arrays leave as 8-byte words");
    {
        const unsigned long long *pat8 = reinterpret_cast<const unsigned long long *>(pat);
        const unsigned long long *hit8 = reinterpret_cast<const unsigned long long *>(T.hit);
        const unsigned long long *cnt8 = reinterpret_cast<const unsigned long long *>(T.hcnt);
        const uint32_t n_pat8 = (H * vp + 7u) / 8u, n_hit8 = (nv * H + 7u) / 8u < JL_SEL_HIT_BYTES / 8u ? (nv * H + 7u) / 8u : JL_SEL_HIT_BYTES / 8u;
        const uint32_t n_cnt8 = (H + 1u) / 2u;   // (hcnt holds kSelCand words: an odd H takes one stale word along, never read)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            jl_pack *o = dsts[t];
            if (!o) continue;
            for (uint32_t i = tid; i < nv * (uint32_t)(sizeof(jl_variant) / 8); i += nt)
                reinterpret_cast<unsigned long long *>(o->variants)[i] =
                    jl_ld_coherent64(reinterpret_cast<const unsigned long long *>(S.variants) + i);
            for (uint32_t i = tid; i < vp; i += nt) o->pos_cols[i] = L.cols[i];
            for (uint32_t i = tid; i < n_cnt8; i += nt) reinterpret_cast<unsigned long long *>(o->hap_count)[i] = cnt8[i];
            for (uint32_t i = tid; i < n_pat8; i += nt) reinterpret_cast<unsigned long long *>(o->hap_pattern)[i] = pat8[i];
            for (uint32_t i = tid; i < n_hit8; i += nt) reinterpret_cast<unsigned long long *>(o->hit)[i] = hit8[i];
        }
    }
    return true;
}

// The exporting selection of the single-word pipeline (phasing sharded by reads: the groups go to the merge as they are),
// written for its latency: it is the tail of a launch the host waits for.  Everything it needs arrives in TWO dependent
// round trips — {group count, the first 256 entries of the occupied list, the run counter} and {count, key of each group} —
// where the general routine chases a dozen; the groups' rows leave 8 bytes at a time (they may lie in pinned host memory).
// `cat`: the read categories of the whole matrix, summed by the caller (LDS).
template <int KW>
__device__ __forceinline__ void phase_export_fast(const jl_win_phase &w, uint32_t vp, const uint32_t *cat, uint32_t *s_acc,
                                                  const jl_two_word *tw = nullptr)
{
    const jl_select_args &S = w.S;
    jl_phase_meta *meta = w.meta;
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    if (tid == 0) *s_acc = 0;
    // trip 1 (the occupied list always holds at least one entry per thread: it is sized by the reads)
    const uint32_t n_occ = jl_ld_coherent(&meta->n_occupied);
    uint32_t s_first = jl_ld_coherent(&w.occupied[tid]);
    __syncthreads();
    uint32_t clean = 0;
    for (uint32_t q = tid; q < n_occ; q += nt) {
        const uint32_t s = q == tid ? s_first : jl_ld_coherent(&w.occupied[q]);
        // trip 2: both words of the group before either is used
        const uint32_t c = jl_ld_coherent(&w.slot_count[s]);
        unsigned long long key = jl_ld_coherent64(&w.slot_key[s]), key_b = 0;
        if (KW == 2) {   // the pair of half-key slots -> the two words (one more round trip, all groups at once)
            const unsigned long long pair = key;
            key = jl_ld_coherent64(&tw->key_a[(uint32_t)(pair >> 32)]);
            key_b = jl_ld_coherent64(&tw->key_b[(uint32_t)pair]);
        }
        clean += c;
        // the slot remembers WHICH exported group it is: the merge answers per group
        __hip_atomic_store(&S.slot_hap[s], q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (q < S.exp_cap) {
            S.exp_count[q] = c;
            for (uint32_t p8 = 0; p8 < vp; p8 += 8u) {
                unsigned long long out = 0;
                for (uint32_t j = 0; j < 8u && p8 + j < vp; ++j)
                    out |= (unsigned long long)(KW == 2 ? key_code2(key, key_b, vp, p8 + j) : key_code(key, vp, p8 + j)) << (8u * j);
                *reinterpret_cast<unsigned long long *>(S.exp_pattern + (uint64_t)q * S.exp_stride + p8) = out;
            }
        }
        empty_slot(w, s);
    }
    clean = wave_sum_all(clean);
    if ((tid & 63u) == 0 && clean) atomicAdd(s_acc, clean);
    __syncthreads();
    if (tid == 0) {
        const uint32_t total_clean = *s_acc;
        if (S.exp_head) {
            S.exp_head[0] = n_occ; S.exp_head[1] = vp; S.exp_head[2] = n_occ > S.exp_cap ? 1u : 0u;
            S.exp_head[3] = cat[0]; S.exp_head[4] = cat[1]; S.exp_head[5] = cat[2]; S.exp_head[6] = cat[3];
            S.exp_head[7] = total_clean;
        }
        // the run's scalars for the stage API (jl_phase_groups_fetch reads them from here)
        if (n_occ > S.exp_cap) atomicOr(&meta->overflow, JL_PHASE_OVF_EXPORT);
        meta->summary.reported_reads = 0;
        meta->summary.insufficient_reads = total_clean;   // clean reads: the merge decides which are reported
        meta->summary.damaged_reads = cat[0];
        meta->summary.marginal_gap = cat[1];
        meta->summary.marginal_heteroduplex = cat[2];
        meta->summary.marginal_partial = cat[3];
        meta->summary.n_haplotypes = 0;
        meta->id_bits = 16u;
        // a session's next launch may come without a plan kernel in front (jl_direct_cols): the group list starts empty
        if (S.exp_head) { meta->n_occupied = 0; meta->overflow = 0; }
    }
    if (KW == 2) {
        __syncthreads();
        two_word_cleanup(*tw);
    }
}

// a global grouping table (rep / cnt null: a table that only numbers its keys — the half-key tables of the two-word launch)
struct table_t { unsigned long long *key; uint32_t *rep, *cnt, *occ, *nocc; uint64_t mask; };

__device__ __forceinline__ uint32_t global_insert64(uint64_t key, uint32_t cnt, uint32_t first, const table_t &T)
{
    uint64_t s = mix64(key + 0x9E3779B97F4A7C15ull) & T.mask;
    for (;;) {
        // Look first: a slot's key never changes within a run, so a resident key read past the L1 is final and needs no
        // atomic.  Same-address atomics serialise at the memory side (about 12 ns each): with one CAS per workgroup on
        // the wild type's slot a million reads queued 500 of them in front of every workgroup's arrival.
        unsigned long long old = jl_ld_coherent64(&T.key[s]);
        if (old == kNoKey) old = atomicCAS(&T.key[s], (unsigned long long)kNoKey, (unsigned long long)key);
        if (old == kNoKey) {
            // write-through stores: the selection may run in another workgroup of this launch
            if (T.rep) __hip_atomic_store(&T.rep[s], first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // any read carrying the key
            __hip_atomic_store(&T.occ[atomicAdd(T.nocc, 1u)], (uint32_t)s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            old = key;
        }
        if (old == key) {
            if (T.cnt) atomicAdd(&T.cnt[s], cnt);
            return (uint32_t)s;
        }
        s = (s + 1u) & T.mask;
    }
}

// ---- the stages of a workgroup of the fused launch, in the order phase_fused_body goes through them.  All of them are
// called by all 256 threads under block-uniform conditions; `L` is the workgroup's LDS.
struct fused_plan {   // block-uniform
    uint32_t vp, n_rows;   // variant positions; called rows (whole-path runs, else 0)
    bool work;             // there is something to phase, and this launch's key width covers it
};
struct own_reads {   // what a lane keeps of its 8 reads for their ids: registers
    uint64_t t;            // dword index within a column
    bool live;             // never for the extra workgroup
    uint32_t clean;        // bit 4r: read r is clean (and grouped)
    uint32_t gslot[1][8];  // global table slot of each clean read
};

// ---- 0. the plan, from one of three sources: the call masks (whole-path runs: every workgroup derives it; the compacting
// workgroup, `plan_block`, also writes the ordered table and the plan through to memory), the launch's direct columns, or
// the resident plan in meta / vpcols.  Reads S.called / S.pos_col or meta and w.vpcols; writes L.plan (cols, n_rows) and,
// in the compacting workgroup, S.rows, the *_out arrays and the run's scalars in meta with agent-scope stores.  Barriers:
// those of plan_prologue and jl_compact_rows_block, or one after L.plan.cols (resident plan), or none (direct columns).
// On entry nothing of this launch has to be complete.
template <int KW, uint32_t NS>
__device__ __forceinline__ fused_plan fused_plan_stage(const jl_win_phase &w, const jl_direct_cols *dc, bool plan_block, fused_lds<NS> &L)
{
    constexpr uint32_t NP = (uint32_t)KW * JL_POS_PER_WORD;   // positions this instantiation covers
    const jl_select_args &S = w.S;
    jl_phase_meta *meta = w.meta;
    const uint32_t tid = threadIdx.x;
    uint32_t vp, n_rows;
    bool work;
    if (S.called != nullptr) {
        plan_prologue(S, S.n_cols, L.plan);
        const uint32_t vpt = L.plan.vp;
        work = !L.plan.ovf && vpt >= 1u && vpt <= NP;
        vp = work ? vpt : 0u;
        n_rows = L.plan.n_rows;
        if (plan_block) {
            // the ordered table (SPEC §6) + what the fetch calls and a multi-word re-run read: written through, the
            // selection runs in whichever workgroup arrives last
            const uint32_t n = jl_compact_rows_block<false>(S.P, S.called, S.staged, S.rows, S.cap, L.scan, &L.running,
                                                            nullptr, 0u, true);
            if (tid < vp) {
                __hip_atomic_store(&S.vpcols_out[tid], L.plan.cols[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&S.col2pos_out[L.plan.cols[tid]], tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (tid == 0) {
                __hip_atomic_store(S.n_rows_out, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const uint32_t need_kw = (vpt + JL_POS_PER_WORD - 1u) / JL_POS_PER_WORD;
                uint32_t ovf = 0;
                if (!work && (vpt != 0u || L.plan.ovf)) ovf = (L.plan.ovf || need_kw <= S.kwords_cap) ? JL_PHASE_OVF_FORM : JL_PHASE_OVF_KEY_WORDS;
                __hip_atomic_store(&meta->n_var, n < S.cap ? n : S.cap, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&meta->vp_true, L.plan.ovf ? JL_POS_PER_WORD + 1u : vpt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&meta->vp, vp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&meta->kwords, work ? (uint32_t)KW : 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&meta->overflow, ovf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&meta->summary.n_positions, vp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    } else if (dc && dc->on) {   // columns by pointer, vp by value: nothing to read, no kernel in front
        work = dc->vp != 0;
        vp = dc->vp;
        n_rows = 0;
    } else {
        const uint32_t mvp = meta->vp, kw = meta->kwords;  // one scalar round trip for both; the plan kernel wrote them
        work = (mvp != 0) & (kw >= 1) & (kw <= (uint32_t)KW);   // block-uniform
        vp = work ? mvp : 0u;
        // all the column indices in one go (the array always holds JL_VARIANT_CAP words; entries past vp are never used)
        if (tid < NP) L.plan.cols[tid] = w.vpcols[tid];
        if (tid == 0) L.plan.n_rows = 0;
        n_rows = 0;
        __syncthreads();
    }
    return {vp, n_rows, work};
}

// ---- 1. keys and flags of this lane's 8 reads: kk[z][r] = word z of read r's pattern (positions 0 .. 9 in word 0, 10 .. 19
// in word 1 of the two-word launch).  Reads L.plan.cols and the plane rows (or the direct columns); writes kk, the wave sums
// of the read categories into L.cat (LDS atomics), and to memory the flag words (only for a separate id launch) and the
// keys (only for the multi-word pipeline's group launch).  No barrier.  On entry L.plan.cols is complete and L.cat is zero,
// both behind a barrier.  Returns the clean reads, bit 4r for read r.
template <int KW, uint32_t NS>
__device__ __forceinline__ uint32_t fused_keys_stage(const jl_win_phase &w, const jl_direct_cols *dc, uint32_t vp, uint64_t t, bool live,
                                                     fused_lds<NS> &L, uint64_t (&kk)[KW][8])
{
    constexpr uint32_t NP = (uint32_t)KW * JL_POS_PER_WORD;
    const jl_select_args &S = w.S;
    const uint32_t tid = threadIdx.x;
    // Lanes past the end of the columns load from a clamped address and drop the value, so the loads need no
    // per-lane branch.
    uint32_t cols[NP];
#pragma unroll
    for (uint32_t p = 0; p < NP; ++p) cols[p] = L.plan.cols[p];
    // (a lane whose eight reads are all past the last read loads nothing of its own: a slice read in place — `direct` —
    // ends where the window's rows may end too)
    const uint64_t t_ld = (live && t * 8u < w.n_reads) ? t : 0u;
    uint32_t wd[NP][3];
    const bool direct = dc && dc->on;   // block-uniform
#pragma unroll
    for (uint32_t p = 0; p < NP; ++p) {
        if (p < vp) {  // block-uniform
            // nine plane rows per position (three columns x three planes), one byte = 8 reads of each
            const uint64_t ps = direct ? dc->stride : w.col_stride / 4u;
            const uint8_t *c0 = (direct && p < JL_POS_PER_WORD) ? dc->col[p] : w.msa + (uint64_t)cols[p] * 3u * ps;
#pragma unroll
            for (int k = 0; k < 3; ++k) wd[p][k] = jl_load_codes8(c0 + (uint64_t)k * 3u * ps + t_ld, ps);
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) wd[p][k] = 0x66666666u;
        }
    }
    if (!live) {
#pragma unroll
        for (uint32_t p = 0; p < NP; ++p)
#pragma unroll
            for (int k = 0; k < 3; ++k) wd[p][k] = 0x66666666u;
    }
    uint32_t gap = 0, het = 0, par = 0;
    // (built in an array of its own and handed over at the end: a round of two picks the dominant key out of kk by a run-time
    // read number, which keeps kk in scratch there — and would send every step of the build through it)
    uint64_t key[KW][8];
#pragma unroll
    for (int z = 0; z < KW; ++z)
#pragma unroll
        for (int r = 0; r < 8; ++r) key[z][r] = 0;
#pragma unroll
    for (uint32_t p = 0; p < NP; ++p) {
        if (p < vp) key_add_position(wd[p], gap, het, par, key[p / JL_POS_PER_WORD]);
    }
    const uint32_t valid = live ? valid_reads8(t, w.n_reads) : 0u;
    gap &= valid; het &= valid; par &= valid;
    const uint32_t dirty = gap | het | par;
    const uint32_t cleanm = valid & ~dirty;  // bit 4r: read r is clean
    if (live && S.ids_mode == JL_IDS_SEPARATE) {
        // the flags and slots of every read are only needed by a later launch that writes the ids
        w.flagw[t] = gap | (het << 1) | (par << 2) | ((valid ^ kM1) << 3);
    }
    if (KW == 1 && live && !S.run) {   // the multi-word pipeline's own group launch reads the keys
        uint64_t *dst = w.keys + t * 8u;
#pragma unroll
        for (int r = 0; r < 8; r += 2) {
            ulonglong2 v;
            v.x = key[0][r];
            v.y = key[0][r + 1];
            *reinterpret_cast<ulonglong2 *>(dst + r) = v;
        }
    }
    {
        // read categories: wave sums into LDS here, ONE global atomic per block and counter further down (the four
        // counters share a cache line: 1564 waves adding to it serialise at the memory side)
        const uint32_t n_gap = wave_sum_all(__popc(gap)), n_het = wave_sum_all(__popc(het));
        const uint32_t n_par = wave_sum_all(__popc(par)), n_dam = wave_sum_all(__popc(dirty));
        if ((tid & 63u) == 0) {
            if (n_dam) atomicAdd(&L.cat[0], n_dam);
            if (n_gap) atomicAdd(&L.cat[1], n_gap);
            if (n_het) atomicAdd(&L.cat[2], n_het);
            if (n_par) atomicAdd(&L.cat[3], n_par);
        }
    }
#pragma unroll
    for (int z = 0; z < KW; ++z)
#pragma unroll
        for (int r = 0; r < 8; ++r) kk[z][r] = key[z][r];
    return cleanm;
}

// ---- 2-3. One ROUND of grouping: the clean reads' 64-bit keys kk[z] -> the slot of each in the global table T[z] (gs[z][r]), for N
// independent key words at once (they share the round's barriers and their trips to the global tables overlap: a round is
// 6.5 us whatever it carries).  The one-word launch runs one round of one, on the patterns themselves; the two-word
// launch a round of two — the words of the patterns — and a round of one on the pairs of their slots (jl_two_word).
// Reads kk and cleanm (registers); uses table sets 0 .. N-1 of L with their dominant-key words and lists; writes the global
// tables (atomics and write-through stores) and gs for the clean reads.  Barriers: one after the clearing (not in the
// first round), two around the dominant key, one after the LDS inserts, one after the lists, one after the global
// inserts, and in a two-word launch one at the end.  On entry, first round: sets 0 .. N-1 are cleared behind a barrier.
template <uint32_t N, uint32_t NS>
__device__ __forceinline__ void group_round(const uint64_t (&kk)[N][8], const table_t (&T)[N], uint32_t cleanm, uint64_t t,
                                            bool first_round, fused_lds<NS> &L, uint32_t (&gs)[N][8])
{
    const uint32_t tid = threadIdx.x;
    if (!first_round) {   // (the first round's tables were cleared while the columns were on their way)
        L.clear_sets(N);
        __syncthreads();
    }
    // ---- 2. dominant key of the block = key of its first clean read
    uint32_t myfirst = 0xFFFFFFFFu;
    if (cleanm) myfirst = (uint32_t)(t * 8u) + ((uint32_t)__ffs((int)cleanm) - 1u) / 4u;
    {
        uint32_t m = myfirst;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = min(m, (uint32_t)__shfl_xor((int)m, o, 64));
        if ((tid & 63u) == 0 && m != 0xFFFFFFFFu) atomicMin(&L.domfirst, m);
    }
    __syncthreads();
    const uint32_t domfirst = L.domfirst;
    if (domfirst != 0xFFFFFFFFu && (uint64_t)(domfirst >> 3) == t) {
#pragma unroll
        for (int r = 0; r < 8; ++r)  // static indices keep the keys in registers
            if ((domfirst & 7u) == (uint32_t)r) {
#pragma unroll
                for (uint32_t z = 0; z < N; ++z) L.dom[z] = kk[z][r];
            }
    }
    __syncthreads();
    unsigned long long dom[N];
    uint32_t isdom[N];  // bit 4r
#pragma unroll
    for (uint32_t z = 0; z < N; ++z) {
        dom[z] = L.dom[z];
        isdom[z] = 0;
#pragma unroll
        for (int r = 0; r < 8; ++r)
            if (((cleanm >> (4 * r)) & 1u) && kk[z][r] == dom[z]) isdom[z] |= 1u << (4 * r);
        const uint32_t c = wave_sum_all(__popc(isdom[z]));
        if ((tid & 63u) == 0 && c) atomicAdd(&L.domcnt[z], c);
    }
    // ---- 3. everything else through the LDS table
    uint32_t myslot[N][8];
#pragma unroll
    for (uint32_t z = 0; z < N; ++z) {
        const uint32_t rest = cleanm & ~isdom[z];
        unsigned long long *tk = L.key(z);
        uint32_t *tc = L.cnt(z), *tf = L.first(z);
#pragma unroll
        for (int r = 0; r < 8; ++r) myslot[z][r] = 0xFFFFFFFFu;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            if ((rest >> (4 * r)) & 1u) {
                const unsigned long long k = kk[z][r];
                uint32_t sl = (uint32_t)mix64(k) & (kLdsSlots - 1u);
                for (uint32_t probe = 0; probe < kLdsSlots; ++probe) {
                    const unsigned long long old = atomicCAS(&tk[sl], (unsigned long long)kNoKey, k);
                    if (old == kNoKey || old == k) {
                        atomicAdd(&tc[sl], 1u);
                        atomicMin(&tf[sl], (uint32_t)(t * 8u + r));
                        myslot[z][r] = sl;
                        break;
                    }
                    sl = (sl + 1u) & (kLdsSlots - 1u);
                }
            }
        }
    }
    __syncthreads();
    // One global insert per distinct key of the block, ALL AT ONCE: the keys are listed densely first, so thread i takes
    // the i-th (a sweep over the 1024 table slots, four per thread, made the thread that owned two occupied slots — and
    // thread 0, which also had the dominant key — do its inserts one after the other: 8.7 us of a 25 us launch at a
    // million reads, two to three dependent round trips each).  The lists of a round of two lie one behind the other.
    // The dominant keys go with the last threads, which have list entries of their own only in blocks with some 250
    // distinct keys or more.
    {
        // (the lists are made by a sweep over the tables: four LDS reads per thread and set, and a barrier)
#pragma unroll
        for (uint32_t z = 0; z < N; ++z)
            for (uint32_t sl = tid; sl < kLdsSlots; sl += 256u)
                if (L.cnt(z)[sl]) L.list[z][atomicAdd(&L.nlist[z], 1u)] = (uint16_t)sl;
        __syncthreads();
        const uint32_t n0 = L.nlist[0], n_all = n0 + (N == 2u ? L.nlist[N - 1u] : 0u);
        for (uint32_t i = tid; i < n_all; i += 256u) {
            const uint32_t z = (N == 2u && i >= n0) ? 1u : 0u;
            const uint32_t sl = L.list[z][i - (z ? n0 : 0u)];
            L.gslot(z)[sl] = global_insert64(L.key(z)[sl], L.cnt(z)[sl], L.first(z)[sl], T[z]);
        }
#pragma unroll
        for (uint32_t z = 0; z < N; ++z)
            if (tid == 255u - z && L.domcnt[z]) L.domslot[z] = global_insert64(dom[z], L.domcnt[z], L.domfirst, T[z]);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t z = 0; z < N; ++z)
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            if ((cleanm >> (4 * r)) & 1u) {
                uint32_t g;
                if ((isdom[z] >> (4 * r)) & 1u) g = L.domslot[z];
                else if (myslot[z][r] != 0xFFFFFFFFu) g = L.gslot(z)[myslot[z][r]];
                else  // LDS table full (> 1024 distinct keys in 2048 reads): straight to the global table
                    g = global_insert64(kk[z][r], 1u, (uint32_t)(t * 8u + r), T[z]);
                gs[z][r] = g;
            }
        }
    if (NS == 2u) __syncthreads();   // the next round clears the LDS tables this one still reads
}

// The per-read ids of this lane's reads, from the slots still in its registers and the slot -> haplotype table (agent-scope
// loads); bits = 0: none (the wait timed out).  No barrier.  On entry the table is complete and visible (see the callers).
__device__ __forceinline__ void write_own_ids(const jl_select_args &S, const own_reads &R, uint32_t bits)
{
    if (R.live && bits) {
        uint16_t h[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            h[r] = JL_HAP_DAMAGED;
            if ((R.clean >> (4 * r)) & 1u)
                h[r] = (uint16_t)__hip_atomic_load(&S.slot_hap[R.gslot[0][r]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        jl_store_ids(S.read_hap, R.t, h, bits);
    }
}

// ---- hand-off: the block that arrives last ranks the groups and writes the result block.  Everything the
// selection reads was written by agent-scope atomics or write-through stores (slot keys and counts, the occupied
// list, the read-category counters, the compacted rows): no release fence — an L2 write-back per block serialises
// in the L2.  Every wave drains its stores -> block barrier -> one lane: the arrival add; the last arriver reads
// with agent-scope loads (past its L1).  The counter is zero before the first launch and the last arriver leaves it zero.
// Reads and writes S.arrive; writes L.last.  Barriers: one before the add, one after.  On entry every store of this
// workgroup that the selection reads has been issued.  Returns whether this workgroup arrived last.
template <uint32_t NS>
__device__ __forceinline__ bool fused_arrive(const jl_select_args &S, uint32_t n_arrive, fused_lds<NS> &L)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t prev = __hip_atomic_fetch_add(S.arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t last = prev == n_arrive - 1u;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(S.arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        L.last = last;
    }
    __syncthreads();
    return L.last != 0;
}

// The last workgroup: the read categories of the window, every workgroup's four words (written through by their
// workgroups) summed into L.cat and, unless the fast export follows, stored to the run's scalars in meta.  Two barriers.
// On entry this workgroup has arrived last.
template <uint32_t NS>
__device__ __forceinline__ void sum_categories(const jl_win_phase &w, bool fast_export, fused_lds<NS> &L)
{
    jl_phase_meta *meta = w.meta;
    const uint32_t tid = threadIdx.x;
    uint32_t c4[4] = {0, 0, 0, 0};
    for (uint32_t b = tid; b < w.n_blocks; b += 256u) {
#pragma unroll
        for (int k = 0; k < 4; ++k) c4[k] += jl_ld_coherent(&w.blockcat[b * 4u + k]);   // written through by their workgroups
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) c4[k] = wave_sum_all(c4[k]);
    if (tid < 4u) L.cat[tid] = 0;
    __syncthreads();
    if ((tid & 63u) == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) atomicAdd(&L.cat[k], c4[k]);
    }
    __syncthreads();
    if (!fast_export && tid == 0) {   // the run's scalars (the general selection and the stage-API fetches read them there)
        __hip_atomic_store(&meta->summary.damaged_reads, L.cat[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&meta->summary.marginal_gap, L.cat[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&meta->summary.marginal_heteroduplex, L.cat[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&meta->summary.marginal_partial, L.cat[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The last workgroup of a two-word launch whose selection out of LDS did not run.  More candidates / rows than it holds
// (or nothing to phase): the general routine reads one-word keys, so the run is handed to the multi-word pipeline —
// tables emptied, the run flagged as one that needs it (the fetch calls re-run it, as they do for more than 20
// positions).  One barrier at the start, that of two_word_cleanup, and a drain of the stores at the end.
__device__ __forceinline__ void hand_down_two_word(const jl_win_phase &w, const jl_two_word &tw, bool work)
{
    jl_phase_meta *meta = w.meta;
    __syncthreads();
    if (work) {
        empty_used_slots(w, jl_ld_coherent(&meta->n_occupied));
        two_word_cleanup(tw);
        if (threadIdx.x == 0) {
            __hip_atomic_store(&meta->overflow, JL_PHASE_OVF_FORM, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&meta->vp_true, 2u * JL_POS_PER_WORD + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&meta->vp, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&meta->kwords, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&meta->n_occupied, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the general routine below reads these scalars back
}

// ---- the last workgroup: the selection — the fast export, or out of LDS, or (two-word launch) the hand-down, or the
// general routine — then the exchange head, the release of the result block, and the flag that releases the waiting
// workgroups.  Reads the tables, lists and scalars the other workgroups wrote; L.plan and L.cat; writes every result of the
// run, L.idbits and S.flag; sets ids_written when this lane's ids went out from within the selection.  Barriers: those of
// sum_categories and of the selection taken, one behind a drain after each of export / selection / head copy, one at the
// end.  On entry fused_arrive has returned true.  Returns false when the launch ends here for this workgroup (an export, or
// ids by a separate launch).
template <int KW, uint32_t NS>
__device__ __forceinline__ bool fused_last(const jl_win_phase &w, const jl_two_word *tw, const fused_plan &P, const own_reads &R,
                                           fused_lds<NS> &L, bool &ids_written)
{
    const jl_select_args &S = w.S;
    jl_phase_meta *meta = w.meta;
    const uint32_t tid = threadIdx.x;
    const bool from_called = S.called != nullptr, work = P.work;
    uint32_t seq_before = 0;
    const bool fast_export = work && S.exp_count != nullptr;
    // the selection's first loads go out beside those of the read categories (the list entry is used below the count only)
    select_pre pre = {0, P.n_rows, 0, 0};
    if (work && !S.exp_count) {
        pre.n_occ = jl_ld_coherent(&meta->n_occupied);
        pre.occ0 = jl_ld_coherent(&w.occupied[tid]);   // (the list holds at least 256 entries: reserve_phase)
    }
    if (!S.exp_count) {   // (an exporting selection needs neither: it ranks nothing)
        pre.nv = from_called ? (P.n_rows < S.cap ? P.n_rows : S.cap) : jl_ld_coherent(&meta->n_var);
        if (!from_called) pre.n_rows = jl_ld_coherent(&S.n_rows[0]);
    } else if (tid == 0 && S.seq_host) {
        seq_before = jl_ld_coherent(S.seq_dev);   // beside the loads below: not a round trip of its own at the end
    }
    if (work) sum_categories(w, fast_export, L);
    if (fast_export) {
        phase_export_fast<KW>(w, P.vp, L.cat, &L.running, tw);
        // every wave's stores (the groups may lie in host memory) are performed; ONE system-scope release, carried by
        // the completion word's store, pushes them out in front of it: data and word leave the same workgroup
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (S.seq_host && tid == 0) jl_signal_done_from(seq_before, S.seq_dev, S.seq_host);
        return false;
    }
    bool done = false;
    uint32_t sel_bits = 0;   // width of the ids, when the selection out of LDS ran
    if (work && !S.exp_count)
        done = phase_select_lds<KW>(w, tw, L, P.vp, pre, &sel_bits, [&](uint32_t bits) {
            if (S.ids_mode == JL_IDS_SEPARATE) return;
            if (tid == 0) __hip_atomic_store(S.flag, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            write_own_ids(S, R, bits);
            ids_written = true;
        });
    if constexpr (KW == 2) {
        if (!done) hand_down_two_word(w, *tw, work);
    }
    if (!done) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the read categories: it reads them from the run's scalars)
        __syncthreads();
        phase_select_block<true>(w, select_lds{reinterpret_cast<uint32_t *>(L.tables[0]), nullptr, nullptr, 0u});
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (S.xhead) {   // bound exchange: the head into the region the launch's all-gather works in
        jl_result_head_copy(S.pk + (__hip_atomic_load(S.seq_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 1u), S.xhead);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    // The result block went to pinned host memory from THIS compute die; the completion word will be stored by
    // whichever workgroup arrives last, possibly on another die.  A system-scope release here pushes the block
    // out of this die's L2 first — without it the host now and then saw the word before the block's header
    // (new per-read ids and variant rows beside the previous run's read categories: one group run in ten).
    if (tid == 0) __threadfence_system();
    if (S.ids_mode == JL_IDS_SEPARATE) {
        if (S.seq_host && tid == 0) jl_signal_done(S.seq_dev, S.seq_host);  // no per-read ids wanted: the run ends here
        return false;
    }
    // the slot -> haplotype table is complete (write-through stores, drained above): release the waiting
    // workgroups; the flag carries the width of the ids
    if (tid == 0) {
        const uint32_t bits = done ? sel_bits : jl_ld_coherent(&meta->id_bits);
        L.idbits = bits;
        if (!ids_written) {     // (the selection out of LDS released them as soon as it had ranked)
            __hip_atomic_store(S.flag, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    return true;
}

// ---- the other workgroups of a launch that writes the ids: wait for the selection.  Every workgroup of this launch is
// resident (the host asks only small grids for inline ids), so
// the flag does arrive; the bound turns a broken invariant into a loud failure, not a hang — and not a fault
// either (a trap can take the device down for every tenant): the run is marked failed where both ways of reading
// it look (the phase scalars for jl_phase_fetch, the pinned block's magic for jl_run_view_get), this workgroup
// writes no ids and goes on to the second arrival so that the launch still ends.
// Thread 0 spins on S.flag (agent-scope loads); writes L.idbits (0: timed out).  One barrier, at the end.  On entry
// fused_arrive has returned false.
template <uint32_t NS>
__device__ __forceinline__ void fused_wait(const jl_win_phase &w, fused_lds<NS> &L)
{
    const jl_select_args &S = w.S;
    jl_phase_meta *meta = w.meta;
    if (threadIdx.x == 0) {
        uint32_t spins = 0, bits;
        while ((bits = __hip_atomic_load(S.flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0u) {
            __builtin_amdgcn_s_sleep(8);
            if (++spins > (1u << 23)) {
                atomicOr(&meta->overflow, JL_PHASE_OVF_IDS_WAIT_TIMEOUT);
                if (S.mirror) __hip_atomic_store(&S.mirror->magic, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                break;
            }
        }
#ifdef JL_TUNING
        if (S.ids_mode == JL_IDS_INLINE_GIVE_UP && bits != 0u) {   // forced: behave as if the wait had run out just before the selection arrived
            atomicOr(&meta->overflow, JL_PHASE_OVF_IDS_WAIT_TIMEOUT);
            if (S.mirror) __hip_atomic_store(&S.mirror->magic, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            bits = 0u;
        }
#endif
        L.idbits = bits;   // 0: timed out
    }
    __syncthreads();
}

// ---- per-read haplotype ids of this workgroup's own reads, straight from the slots still in registers, and the
// second arrival: every workgroup is past the flag by now, so the one that arrives last resets it (and the
// counter) for the next launch and, when this launch ends a run, stores the completion word behind all the ids.
// Reads L.idbits, S.slot_hap; writes S.read_hap, S.arrive2, S.flag.  One barrier, behind a drain of the ids.  On entry
// L.idbits is set behind a barrier (fused_last or fused_wait).
template <uint32_t NS>
__device__ __forceinline__ void fused_ids_and_leave(const jl_win_phase &w, uint32_t n_arrive, const own_reads &R, bool ids_written,
                                                    const fused_lds<NS> &L)
{
    const jl_select_args &S = w.S;
    if (!ids_written) write_own_ids(S, R, L.idbits);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        if (S.seq_host) __threadfence_system();   // this workgroup's ids leave its die's L2 before it arrives (see fused_last)
        const uint32_t prev = __hip_atomic_fetch_add(S.arrive2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (prev == n_arrive - 1u) {
            __hip_atomic_store(S.arrive2, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(S.flag, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // A workgroup that gave up waiting marked the run failed; a selection that was only LATE has since written a
            // valid result block over that mark.  The mark in the run's scalars is the lasting one: whoever arrives last
            // makes the blocks say so again, just before the completion word.
            if (jl_ld_coherent(&w.meta->overflow) & JL_PHASE_OVF_IDS_WAIT_TIMEOUT) {
                if (S.mirror) __hip_atomic_store(&S.mirror->magic, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                jl_pack *pk = S.pk + (__hip_atomic_load(S.seq_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 1u);
                __hip_atomic_store(&pk->magic, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (S.seq_host) jl_signal_done(S.seq_dev, S.seq_host);
        }
    }
}

// A workgroup of the fused launch with KW key words: the one-word launch (a window, with or without direct columns), the
// group launch, the two-word launch.
template <int KW>
__device__ __forceinline__ void phase_fused_body(const jl_win_phase &w, const jl_direct_cols *dc = nullptr, const jl_two_word *tw = nullptr)
{
    constexpr uint32_t NS = KW == 2 ? 2u : 1u;
    __shared__ fused_lds<NS> L;
    const jl_select_args &S = w.S;
    const uint32_t tid = threadIdx.x;
    const bool from_called = S.called != nullptr;
    // whole-path runs launch one workgroup more than the reads need: it compacts the called rows meanwhile
    const uint32_t n_arrive = w.n_blocks + (from_called ? 1u : 0u);
    const bool plan_block = from_called && blockIdx.x == w.n_blocks;

    const fused_plan P = fused_plan_stage<KW>(w, dc, plan_block, L);
    const uint64_t t = (uint64_t)blockIdx.x * 256u + tid;  // dword index within a column = 8 reads
    own_reads R = {t, t * 4u < w.col_stride, 0u, {{0, 0, 0, 0, 0, 0, 0, 0}}};
    if (P.work && !plan_block) {
        L.clear_sets(NS);
        if (tid < 4) L.cat[tid] = 0;
        __syncthreads();
        uint64_t kk[KW][8];
        const uint32_t cleanm = fused_keys_stage<KW>(w, dc, P.vp, t, R.live, L, kk);
        const table_t T_main[1] = {{w.slot_key, w.slot_rep, w.slot_count, w.occupied, &w.meta->n_occupied, w.slots_mask}};
        if constexpr (KW == 1) {
            group_round(kk, T_main, cleanm, t, true, L, R.gslot);
        } else {   // the two words numbered in the half-key tables, then the pairs of their numbers in the window's table
            uint32_t g01[2][8] = {{0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}};
            const table_t T2[2] = {{tw->key_a, nullptr, nullptr, tw->occ_a, tw->n_occ, w.slots_mask},
                                   {tw->key_b, nullptr, nullptr, tw->occ_b, tw->n_occ + 1, w.slots_mask}};
            group_round(kk, T2, cleanm, t, true, L, g01);
            uint64_t kk3[1][8];
#pragma unroll
            for (int r = 0; r < 8; ++r) kk3[0][r] = ((uint64_t)g01[0][r] << 32) | g01[1][r];   // never all ones: slots are 31-bit numbers
            group_round(kk3, T_main, cleanm, t, false, L, R.gslot);
        }
        // read categories of this workgroup's reads: written through to its own four words; the selection adds the workgroups
        // up (four atomics per workgroup on ONE cache line were the longest queue of the launch at a million reads)
        if (tid >= 64u && tid < 68u)
            __hip_atomic_store(&w.blockcat[blockIdx.x * 4u + (tid - 64u)], L.cat[tid - 64u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (S.ids_mode == JL_IDS_SEPARATE) {
#pragma unroll
            for (int r = 0; r < 8; ++r)
                if ((cleanm >> (4 * r)) & 1u) w.read_slot[t * 8u + r] = R.gslot[0][r];
        }
        R.clean = cleanm;
    }
    if (!S.run) return;  // the generic pipeline has its own select launch
    const bool last = fused_arrive(S, n_arrive, L);
    if (!last && S.ids_mode == JL_IDS_SEPARATE) return;
    bool ids_written = false;
    if (last) {
        if (!fused_last<KW>(w, tw, P, R, L, ids_written)) return;
    } else {
        fused_wait(w, L);
    }
    fused_ids_and_leave(w, n_arrive, R, ids_written, L);
}

__global__ __launch_bounds__(256) void phase_fused1_kernel(jl_win_phase w) { phase_fused_body<1>(w); }
__global__ __launch_bounds__(256) void phase_fused1_direct_kernel(jl_win_phase w, jl_direct_cols dc) { phase_fused_body<1>(w, &dc); }
// 11 .. 20 variant positions: the same launch with two key words (jl_two_word)
__global__ __launch_bounds__(256) void phase_fused2_kernel(jl_win_phase w, jl_two_word tw) { phase_fused_body<2>(w, nullptr, &tw); }

// one launch for several windows: blockIdx.z = window
__global__ __launch_bounds__(256) void phase_group_run_kernel(jl_phase_group_args args)
{
    const jl_win_phase &w = args.w[blockIdx.z];
    if (blockIdx.x >= w.n_blocks + (w.S.called ? 1u : 0u)) return;
    phase_fused_body<1>(w);
}

// ---------------------------------------------------------------------------------------- assign
// Per-read ids by a launch of their own (launches too large for their workgroups to wait for each other, and the
// multi-word pipeline).  Eight reads per lane: one flag word, two 16-byte loads of slots, one store of packed ids.
__device__ __forceinline__ void assign_body(uint64_t n_dwords, const uint32_t *__restrict__ flagw,
                                            const jl_phase_meta *__restrict__ meta, const uint32_t *__restrict__ read_slot,
                                            const uint32_t *__restrict__ slot_hap, uint16_t *__restrict__ read_hap)
{
    const bool phased = meta->vp != 0;
    const uint32_t bits = meta->id_bits;
    // t = dword index within a column; the grid may be smaller than the window (see jl_launch_assign_group)
    for (uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x; t < n_dwords; t += (uint64_t)gridDim.x * 256u) {
        uint16_t h[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) h[r] = JL_HAP_DAMAGED;
        if (phased) {
            const uint32_t f = flagw[t];
            const uint4 s0 = *reinterpret_cast<const uint4 *>(read_slot + t * 8u);
            const uint4 s1 = *reinterpret_cast<const uint4 *>(read_slot + t * 8u + 4u);
            const uint32_t slot[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
#pragma unroll
            for (int r = 0; r < 8; ++r)
                if (((f >> (4 * r)) & 15u) == 0) h[r] = (uint16_t)slot_hap[slot[r]];   // clean reads only: their slot is valid
        }
        jl_store_ids(read_hap, t, h, bits);
    }
}

__global__ __launch_bounds__(256) void phase_assign_kernel(uint64_t n_dwords, const uint32_t *__restrict__ flagw,
                                                            const jl_phase_meta *__restrict__ meta,
                                                            const uint32_t *__restrict__ read_slot,
                                                            const uint32_t *__restrict__ slot_hap,
                                                            uint16_t *__restrict__ read_hap)
{
    assign_body(n_dwords, flagw, meta, read_slot, slot_hap, read_hap);
}

// the same for the windows of a group launch (blockIdx.z = window)
__global__ __launch_bounds__(256) void phase_assign_group_kernel(jl_phase_group_args args)
{
    const jl_win_phase &w = args.w[blockIdx.z];
    assign_body(w.col_stride / 4u, w.flagw, w.meta, w.read_slot, w.S.slot_hap, w.S.read_hap);
}

}  // namespace

// workgroups per window of a launch that writes per-read ids (see jl_launch_assign_group)
static uint32_t jl_assign_blocks(uint32_t n_win, uint32_t max_read_blocks, bool to_host)
{
    if (!to_host) return max_read_blocks;   // ids that stay in HBM: one workgroup per 2048 reads
    // to pinned host memory: 128 workgroups in all (see jl_launch_assign_group)
    const uint32_t cap = std::max(1u, 128u / std::max(1u, n_win));
    return std::min<uint32_t>(cap, max_read_blocks);
}

// a window's phasing grid: a workgroup per 2048 reads + the one that compacts the rows
uint32_t jl_phase_grid_blocks(const jl_ctx *ctx) { return (uint32_t)((ctx->col_stride / 4u + 255u) / 256u) + 1u; }
// this context may take inline ids: a fused launch that selects (an exporting run keeps every read's flags and slot:
// jl_phase_regroup maps them once the merge is known) and has never timed out waiting
static bool phase_ids_inline_ok(const jl_ctx *ctx) { return ctx->phase_form != jl_phase_form::multi_word && !ctx->phase_export && !ctx->ids_separate; }
// A launch over these windows (a single run: one) writes the per-read ids itself when every window may take them and ALL its
// workgroups are resident at once, so that they can wait for each other — also while more such launches run: at most
// JL_INLINE_IDS_MAX_BLOCKS per launch against 1536 places (six 75-register blocks per CU).
bool jl_phase_ids_inline(jl_ctx *const *ctxs, uint32_t n_win)
{
    uint32_t total_blocks = 0;
    for (uint32_t k = 0; k < n_win; ++k) total_blocks += jl_phase_grid_blocks(ctxs[k]);
    return total_blocks <= JL_INLINE_IDS_MAX_BLOCKS && std::all_of(ctxs, ctxs + n_win, phase_ids_inline_ok);
}

// Argument block of the fused phase launch for one window.  `plan`: call_masks, or the plan is in meta / vpcols already.
void jl_fill_win_phase(jl_ctx *ctx, uint32_t min_reads, bool signal, bool ids_inline, jl_phase_plan plan, jl_win_phase *w)
{
    memset(w, 0, sizeof *w);
    const bool ids_to_host = ctx->read_hap_out != nullptr;
    const bool signal_select = signal && !ids_to_host;   // no ids wanted on the host: the selection ends the run
    w->msa = ctx->d_msa; w->col_stride = ctx->col_stride; w->n_reads = ctx->n_reads; w->reads_pad = ctx->col_stride * 2u;
    w->vpcols = ctx->d_vpcols; w->meta = ctx->d_meta; w->keys = ctx->d_keys; w->flagw = ctx->d_flagw;
    w->slots_mask = ctx->table_slots - 1u; w->slot_key = ctx->d_slot_key.as<unsigned long long>();
    w->slot_rep = ctx->d_slot_rep; w->slot_count = ctx->d_slot_count; w->occupied = ctx->d_occupied;
    w->read_slot = ctx->d_read_slot;
    w->blockcat = ctx->d_blockcat;
    w->n_blocks = jl_phase_grid_blocks(ctx) - 1u;   // (the arrival counters do not count the compacting workgroup)
    jl_select_args &S = w->S;
    S.run = ctx->phase_form == jl_phase_form::multi_word ? 0u : 1u;
    S.min_reads = min_reads; S.n_cols = ctx->n_cols; S.cooc_cap = ctx->cooc_cap;
    S.slot_hap = ctx->d_slot_hap; S.variants = ctx->d_variants; S.col2pos = ctx->d_col2pos;
    S.hap_count = ctx->d_hap_count; S.hap_pattern = ctx->d_hap_pattern; S.hit = ctx->d_hit; S.n_rows = ctx->d_nvar;
    S.cooc = ctx->d_cooc; S.pk = ctx->d_pack; S.mirror = ctx->pack_mirror;
    S.arrive = ctx->d_sync + 2; S.seq_dev = ctx->d_sync;
    if (ctx->phase_export) {
        if (ctx->exp_ext_count) {   // a session's block (pinned host memory, or the send buffer of the all-gather)
            S.exp_count = ctx->exp_ext_count; S.exp_pattern = ctx->exp_ext_pattern; S.exp_head = ctx->exp_ext_head;
            S.exp_cap = ctx->exp_ext_cap; S.exp_stride = ctx->exp_ext_stride;
        } else {
            S.exp_count = ctx->d_exp_count; S.exp_pattern = ctx->d_exp_pattern;
            S.exp_cap = ctx->exp_cap; S.exp_stride = ctx->exp_stride;
        }
    }
    S.ids_mode = ids_inline ? JL_IDS_INLINE : JL_IDS_SEPARATE;   // one launch less
#ifdef JL_TUNING
    // tests of the re-run: the waiting workgroups give up at once (as if they had not been resident together)
    if (ids_inline && jl_env().force_ids_wait_timeout) S.ids_mode = JL_IDS_INLINE_GIVE_UP;
#endif
    S.flag = ctx->d_sync + 4; S.arrive2 = ctx->d_sync + 3;
    S.read_hap = ctx->read_hap_out ? ctx->read_hap_out : ctx->d_read_hap;
    S.seq_host = (ids_inline ? signal : signal_select) ? ctx->h_seq : nullptr;
    if (plan == jl_phase_plan::call_masks) {
        S.called = ctx->d_called; S.staged = ctx->d_staged; S.pos_col = ctx->d_pos_col; S.rows = ctx->d_variants;
        S.n_rows_out = ctx->d_nvar; S.vpcols_out = ctx->d_vpcols; S.col2pos_out = ctx->d_col2pos;
        S.P = ctx->P; S.cap = JL_VARIANT_CAP; S.kwords_cap = ctx->keys_words;
    }
}

// The phasing launches of ctx->phase_form (the fused ones flag inputs that need a larger form: JL_PHASE_OVF_FORM).  `signal`:
// this launch ends a jl_run_async.  Returns whether the launches store the run's completion word themselves (otherwise the
// caller adds done_kernel).
bool jl_launch_phase(jl_ctx *ctx, hipStream_t st, uint32_t min_reads, jl_phase_plan plan, bool signal)
{
    const uint64_t reads_pad = ctx->col_stride * 2u;
    const bool generic = ctx->phase_form == jl_phase_form::multi_word;
    const bool ids_to_host = ctx->read_hap_out != nullptr;
    // only the fused launches read call masks: behind them the multi-word pipeline finds the plan its compact launch wrote
    if (generic && plan == jl_phase_plan::call_masks) plan = jl_phase_plan::resident;
    if (plan == jl_phase_plan::plan_kernel) {
        jl_win_compact c;
        jl_fill_win_compact(ctx, true, false, false, &c);
        hipLaunchKernelGGL(phase_plan_kernel, dim3(1), dim3(1024), 0, st, c);
    }
    const uint32_t n_dwords = (uint32_t)(ctx->col_stride / 4u);
    jl_win_phase w;
    const bool ids_inline = jl_phase_ids_inline(&ctx, 1);   // a chunk of one window
    jl_fill_win_phase(ctx, min_reads, signal, ids_inline, plan, &w);
    if (generic) {
        hipLaunchKernelGGL(phase_keys_kernel, dim3((n_dwords + 255u) / 256u), dim3(256), 0, st, ctx->d_msa,
                           ctx->plane_stride, ctx->n_reads, reads_pad, ctx->d_vpcols, ctx->d_meta, ctx->d_keys,
                           ctx->d_flagw);
        hipLaunchKernelGGL(phase_group_kernel, dim3((uint32_t)((ctx->n_reads + 255u) / 256u)), dim3(256), 0, st, w);
        // (the selection ends the run when no ids are wanted on the host: w.S.seq_host is `signal && !ids_to_host ? h_seq :
        // null` here, as this form never takes inline ids — phase_ids_inline_ok)
        hipLaunchKernelGGL(phase_select_kernel, dim3(1), dim3(1024), 0, st, w);
    } else if (ctx->direct.on && !w.S.called) {
        hipLaunchKernelGGL(phase_fused1_direct_kernel, dim3(w.n_blocks), dim3(256), 0, st, w, ctx->direct);
    } else if (ctx->phase_form == jl_phase_form::two_word) {
        jl_two_word tw;
        tw.key_a = ctx->d_slot_key_a.as<unsigned long long>(); tw.key_b = ctx->d_slot_key_b.as<unsigned long long>();
        tw.occ_a = ctx->d_occ_a; tw.occ_b = ctx->d_occ_b; tw.n_occ = ctx->d_sync + 10;
        hipLaunchKernelGGL(phase_fused2_kernel, dim3(w.n_blocks + (w.S.called ? 1u : 0u)), dim3(256), 0, st, w, tw);
    } else {
        hipLaunchKernelGGL(phase_fused1_kernel, dim3(w.n_blocks + (w.S.called ? 1u : 0u)), dim3(256), 0, st, w);
    }
    if (ids_inline) return signal;
    if (ctx->phase_export) return false;   // the ids wait for the merge (jl_phase_regroup)
    hipLaunchKernelGGL(phase_assign_kernel, dim3(jl_assign_blocks(1, w.n_blocks, ids_to_host)), dim3(256), 0, st,
                       (uint64_t)n_dwords, ctx->d_flagw, ctx->d_meta, ctx->d_read_slot, ctx->d_slot_hap,
                       ctx->read_hap_out ? ctx->read_hap_out : ctx->d_read_hap);
    return false;
}

static void fill_phase_group_args(jl_phase_group_args *args, const jl_win_phase *h_wins, uint32_t n_win)
{
    memset(args, 0, sizeof *args);
    memcpy(args->w, h_wins, sizeof(jl_win_phase) * (n_win < JL_GROUP_MAX ? n_win : JL_GROUP_MAX));
}

void jl_launch_phase_group(const jl_win_phase *h_wins, uint32_t n_win, uint32_t max_blocks, hipStream_t st)
{
    jl_phase_group_args args;
    fill_phase_group_args(&args, h_wins, n_win);
    hipLaunchKernelGGL(phase_group_run_kernel, dim3(max_blocks + 1u, 1, n_win), dim3(256), 0, st, args);
}

void jl_launch_assign_group(const jl_win_phase *h_wins, uint32_t n_win, uint32_t max_read_blocks, bool to_host, hipStream_t st)
{
    jl_phase_group_args args;
    fill_phase_group_args(&args, h_wins, n_win);
    // The ids usually go to pinned host memory, i.e. over PCIe at a fiftieth of the HBM rate.  A launch that has all
    // of them in flight at once (49 workgroups per 100k reads) fills the L2's write queues with host-bound lines and the
    // pileups of the other launches on the chip wait behind them; about 32 workgroups looping over the reads keep PCIe
    // saturated all the same.
    const uint32_t bx = jl_assign_blocks(n_win, max_read_blocks, to_host);
    hipLaunchKernelGGL(phase_assign_group_kernel, dim3(bx, 1, n_win), dim3(256), 0, st, args);
}


// ---------------------------------------------------------------------------------------- sharded by reads: the merge's answer
// hap_of_group[q] = haplotype id (or JL_HAP_INSUFFICIENT) of the q-th group this matrix exported; every table slot holds
// its group's index since the exporting selection (kernels_xwin.hip maps the reads)
void jl_launch_regroup(jl_ctx *ctx, const uint16_t *d_hap_of_group, uint32_t n_groups, uint32_t n_haplotypes, bool phased)
{
    jl_xw_assign_args a;
    memset(&a, 0, sizeof a);
    a.n_dwords = ctx->col_stride / 4u;
    a.flagw = ctx->d_flagw; a.read_slot = ctx->d_read_slot; a.slot_hap = ctx->d_slot_hap; a.read_hap = ctx->d_read_hap;
    a.n_groups = n_groups;
    a.bits = n_haplotypes <= JL_ID4_MAX_H ? 4u : (n_haplotypes <= JL_ID8_MAX_H ? 8u : 16u);
    a.phased = phased ? 1u : 0u;   // no variant position: every read is "damaged", flags and slots were never written
    jl_launch_xw_assign(&a, nullptr, d_hap_of_group, ctx->stream);
}
