// hap_stage.h — the host front end of the calls that compare every read with a table of reported haplotypes (capi_rescue.hip,
// capi_nearest.hip, capi_recomb.hip; the kernels' side is hap_walk.h): what they refuse, in the order they refuse it, and the form
// the table streams in.  Plain host C++.  The includer brings jl_ctx (its d_msa and n_cols are read), jl_fail and
// JL_RESCUE_POS_MAX: jl_internal.h in the library, stand-ins in tests/cpp/hap_stage_check.cpp.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/juliet_hip.h"

// codon starts: each codon inside the window's columns, the columns strictly ascending (also capi_link.hip, capi_class_codons.hip)
static inline int jl_check_codon_columns(jl_ctx *ctx, const char *fn, const uint32_t *pos_cols, uint32_t n_pos)
{
    for (uint32_t p = 0; p < n_pos; ++p) {
        if ((uint64_t)pos_cols[p] + 2u >= ctx->n_cols)
            return jl_fail(ctx, JL_ERR_ARG, "%s: position %u: the codon at column %u ends beyond the window's %u columns", fn, p, pos_cols[p], ctx->n_cols);
        if (p && pos_cols[p] <= pos_cols[p - 1]) return jl_fail(ctx, JL_ERR_ARG, "%s: position %u: columns not strictly ascending", fn, p);
    }
    return JL_OK;
}

// the sizes of a table (ctx may be NULL: jl_haplotype_recombinants)
static inline int jl_check_hap_shape(jl_ctx *ctx, const char *fn, uint32_t n_pos, uint32_t pattern_stride, uint32_t n_hap)
{
    if (n_pos == 0 || n_pos > JL_RESCUE_POS_MAX) return jl_fail(ctx, JL_ERR_ARG, "%s: %u positions, 1 to %u", fn, n_pos, JL_RESCUE_POS_MAX);
    if (n_hap == 0 || n_hap > (uint32_t)JL_MAX_HAPLOTYPES)
        return jl_fail(ctx, JL_ERR_ARG, "%s: %u haplotypes, 1 to %d", fn, n_hap, (int)JL_MAX_HAPLOTYPES);
    if (pattern_stride < n_pos) return jl_fail(ctx, JL_ERR_ARG, "%s: pattern_stride %u below the %u positions of a row", fn, pattern_stride, n_pos);
    return JL_OK;
}

// What every call on a table checks first: a resident matrix, the arrays, the sizes, min_positions.  A call with arguments of its
// own checks them next (max_distance), then the table's contents with jl_check_hap_contents: that is the order a call that is
// wrong twice reports in.
static inline int jl_check_hap_table(jl_ctx *ctx, const char *fn, const uint32_t *pos_cols, uint32_t n_pos, const uint8_t *pattern,
                                     uint32_t pattern_stride, uint32_t n_hap, uint32_t min_positions)
{
    if (!ctx->d_msa) return jl_fail(ctx, JL_ERR_STATE, "%s: no resident matrix", fn);
    if (!pos_cols) return jl_fail(ctx, JL_ERR_ARG, "%s: no positions array", fn);
    if (!pattern) return jl_fail(ctx, JL_ERR_ARG, "%s: no pattern array", fn);
    if (int rc = jl_check_hap_shape(ctx, fn, n_pos, pattern_stride, n_hap)) return rc;
    if (min_positions == 0 || min_positions > n_pos)
        return jl_fail(ctx, JL_ERR_ARG, "%s: min_positions %u, 1 to the %u positions", fn, min_positions, n_pos);
    return JL_OK;
}

// ... and last: the columns, then every pattern byte a codon
static inline int jl_check_hap_contents(jl_ctx *ctx, const char *fn, const uint32_t *pos_cols, uint32_t n_pos, const uint8_t *pattern,
                                        uint32_t pattern_stride, uint32_t n_hap)
{
    if (int rc = jl_check_codon_columns(ctx, fn, pos_cols, n_pos)) return rc;
    for (uint32_t h = 0; h < n_hap; ++h)
        for (uint32_t p = 0; p < n_pos; ++p)
            if (pattern[(size_t)h * pattern_stride + p] > 63u)
                return jl_fail(ctx, JL_ERR_ARG, "%s: pattern byte %u of haplotype %u at position %u is no codon (0..63)", fn,
                               (unsigned)pattern[(size_t)h * pattern_stride + p], h, p);
    return JL_OK;
}

// The form a table streams in, one direction of it: pos_cols [n_pos], then pat4 [groups][hap_pad], a lane a haplotype and four
// positions a dword: byte q of dword [g][h] = pattern[h][4 g + q], 0 where either does not exist.
struct jl_pat4_shape {
    uint32_t hap_pad, groups;   // n_hap in whole chunks of 64; ceil(n_pos / 4)
    size_t pat_words;           // groups x hap_pad
    size_t dir_words;           // n_pos + pat_words
};
static inline jl_pat4_shape jl_pat4_shape_for(uint32_t n_pos, uint32_t n_hap)
{
    jl_pat4_shape s;
    s.hap_pad = (n_hap + 63u) / 64u * 64u, s.groups = (n_pos + 3u) / 4u;
    s.pat_words = (size_t)s.groups * s.hap_pad, s.dir_words = (size_t)n_pos + s.pat_words;
    return s;
}

// dst [ceil(n_pos / 4)][hap_pad]; reversed: of the pattern with every row reversed
static inline void jl_pack_pat4(uint32_t *dst, const uint8_t *pattern, uint32_t pattern_stride, uint32_t n_hap, uint32_t n_pos, uint32_t hap_pad,
                                bool reversed)
{
    memset(dst, 0, (size_t)((n_pos + 3u) / 4u) * hap_pad * sizeof(uint32_t));
    for (uint32_t h = 0; h < n_hap; ++h)
        for (uint32_t p = 0; p < n_pos; ++p)
            dst[(size_t)(p / 4u) * hap_pad + h] |= (uint32_t)pattern[(size_t)h * pattern_stride + (reversed ? n_pos - 1u - p : p)] << (8u * (p % 4u));
}

// one direction into staging: dst [s.dir_words]; reversed: the positions from the last to the first, and the pattern with them
static inline void jl_stage_hap_direction(uint32_t *dst, const jl_pat4_shape &s, const uint32_t *pos_cols, uint32_t n_pos, const uint8_t *pattern,
                                          uint32_t pattern_stride, uint32_t n_hap, bool reversed)
{
    for (uint32_t p = 0; p < n_pos; ++p) dst[p] = pos_cols[reversed ? n_pos - 1u - p : p];
    jl_pack_pat4(dst + n_pos, pattern, pattern_stride, n_hap, n_pos, s.hap_pad, reversed);
}
