// Stand-alone driver of csrc/hap_stage.h, the host front end of the read-against-haplotype calls (tests/test_hap_stage_host.py
// builds it with the host sanitizers and compares what it prints and writes):
//   hap_stage_check pack N_POS N_HAP STRIDE REVERSED IN OUT   pattern bytes [N_HAP][STRIDE] from IN; OUT gets one direction as
//                                                             jl_stage_hap_direction leaves it for the columns 7, 17, 27, ...
//   hap_stage_check refuse                                    one line "name<TAB>status<TAB>text" per refusal below
// jl_ctx, jl_fail and JL_RESCUE_POS_MAX are stand-ins for jl_internal.h's: the header reads d_msa and n_cols only.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../include/juliet_hip.h"

#define JL_RESCUE_POS_MAX 4096u   // JL_VARIANT_CAP of jl_internal.h
struct jl_ctx {
    const uint8_t *d_msa;
    uint32_t n_cols;
};
static char g_err[512];
static int jl_fail(jl_ctx *, int status, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return status;
}

#include "../../minorseq_amd/csrc/hap_stage.h"

static int pack(char **argv)
{
    const uint32_t n_pos = (uint32_t)atoi(argv[2]), n_hap = (uint32_t)atoi(argv[3]), stride = (uint32_t)atoi(argv[4]);
    const bool reversed = atoi(argv[5]) != 0;
    std::vector<uint8_t> pattern((size_t)n_hap * stride);
    FILE *in = fopen(argv[6], "rb");
    if (!in || fread(pattern.data(), 1, pattern.size(), in) != pattern.size()) return 2;
    fclose(in);
    std::vector<uint32_t> cols(n_pos);
    for (uint32_t p = 0; p < n_pos; ++p) cols[p] = 7u + 10u * p;
    const jl_pat4_shape s = jl_pat4_shape_for(n_pos, n_hap);
    std::vector<uint32_t> dst(s.dir_words, 0xDEADBEEFu);   // (whatever staging held before: every word must be written)
    jl_stage_hap_direction(dst.data(), s, cols.data(), n_pos, pattern.data(), stride, n_hap, reversed);
    FILE *out = fopen(argv[7], "wb");
    if (!out || fwrite(dst.data(), sizeof(uint32_t), dst.size(), out) != dst.size()) return 2;
    fclose(out);
    printf("%u %u %zu %zu\n", s.hap_pad, s.groups, s.pat_words, s.dir_words);
    return 0;
}

// the arguments of a call that passes, one of them spoilt per case
struct call {
    jl_ctx ctx;
    std::vector<uint32_t> cols;
    std::vector<uint8_t> pattern;
    const uint32_t *pos_cols;
    const uint8_t *pat;
    uint32_t n_pos, stride, n_hap, min_positions;
    call() : cols{10, 20, 30, 40}, pattern(3 * 5, 9)
    {
        static const uint8_t planes[1] = {0};
        ctx.d_msa = planes, ctx.n_cols = 100;
        pos_cols = cols.data(), pat = pattern.data(), n_pos = 4, stride = 5, n_hap = 3, min_positions = 2;
    }
    int run(const char *fn)
    {
        if (int rc = jl_check_hap_table(&ctx, fn, pos_cols, n_pos, pat, stride, n_hap, min_positions)) return rc;
        return jl_check_hap_contents(&ctx, fn, pos_cols, n_pos, pat, stride, n_hap);
    }
};

static void report(const char *name, int status)
{
    printf("%s\t%d\t%s\n", name, status, status ? g_err : "");
    g_err[0] = 0;
}

static int refuse()
{
    static const char *fn = "jl_phase_rescue_async";
    { call c; report("passes", c.run(fn)); }
    { call c; c.ctx.d_msa = nullptr; c.pos_cols = nullptr; report("no_matrix_first", c.run(fn)); }
    { call c; c.pos_cols = nullptr; c.pat = nullptr; report("no_positions", c.run(fn)); }
    { call c; c.pat = nullptr; c.n_pos = 0; report("no_pattern", c.run(fn)); }
    { call c; c.n_pos = 0; c.n_hap = 0; report("zero_positions", c.run(fn)); }
    { call c; c.n_pos = 4097; report("too_many_positions", c.run(fn)); }
    { call c; c.n_hap = 0; c.stride = 1; report("zero_haplotypes", c.run(fn)); }
    { call c; c.n_hap = 703; report("too_many_haplotypes", c.run(fn)); }
    { call c; c.stride = 3; c.min_positions = 0; report("short_stride", c.run(fn)); }
    { call c; c.min_positions = 0; c.cols[1] = 5; report("zero_min_positions", c.run(fn)); }
    { call c; c.min_positions = 5; report("min_positions_above", c.run(fn)); }
    { call c; c.cols[3] = 98; c.pattern[0] = 64; report("codon_beyond_window", c.run(fn)); }
    { call c; c.cols[2] = 20; c.pattern[0] = 64; report("not_ascending", c.run(fn)); }
    { call c; c.cols[1] = 98; c.cols[2] = 20; report("beyond_before_ascending", c.run(fn)); }
    { call c; c.pattern[1 * 5 + 2] = 64; c.pattern[2 * 5 + 0] = 200; report("no_codon", c.run(fn)); }
    { call c; c.pattern[4] = 255; c.pattern[9] = 255; report("stride_padding_is_not_read", c.run(fn)); }
    // the parts other calls use: the sizes alone with no context (jl_haplotype_recombinants), the columns alone (linkage, class codons)
    report("shape_passes", jl_check_hap_shape(nullptr, "jl_haplotype_recombinants", 4096, 4096, 702));
    report("shape_positions", jl_check_hap_shape(nullptr, "jl_haplotype_recombinants", 0, 0, 0));
    report("shape_haplotypes", jl_check_hap_shape(nullptr, "jl_haplotype_recombinants", 4, 3, 703));
    report("shape_stride", jl_check_hap_shape(nullptr, "jl_haplotype_recombinants", 4, 3, 3));
    { call c; c.cols[0] = 97; report("columns_last_codon_fits", jl_check_codon_columns(&c.ctx, "jl_variant_linkage_async", c.cols.data(), 1)); }
    { call c; c.cols[0] = 98; report("columns_beyond", jl_check_codon_columns(&c.ctx, "jl_variant_linkage_async", c.cols.data(), 1)); }
    { call c; c.cols[1] = 10; report("columns_equal", jl_check_codon_columns(&c.ctx, "jl_class_codons_async", c.cols.data(), 4)); }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 8 && !strcmp(argv[1], "pack")) return pack(argv);
    if (argc == 2 && !strcmp(argv[1], "refuse")) return refuse();
    fprintf(stderr, "usage: hap_stage_check pack N_POS N_HAP STRIDE REVERSED IN OUT | refuse\n");
    return 2;
}
