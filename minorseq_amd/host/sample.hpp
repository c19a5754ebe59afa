// sample.hpp — one sample, step by step.  What `juliet in.bam out...` does to its file, cut into the steps that a batch (--batch)
// runs for each of its samples too: decode and upload (load_sample: the ONE place a BAM gets onto a context), the sample's setup
// (sample_window, sample_params), the window ingest (ingest_window), --downsample / --mix on the resident window, the fetch of
// its results (Results, fetch_*).  Every path calls these, so a sample of a batch gets what a single run of the same file gets.
// Also here: what the modes share to end with (die_jl, end_process).
#pragma once
#include <unistd.h>

#include <functional>
#include <iostream>
#include <limits>
#include <memory>

#include "config.hpp"
#include "format.hpp"
#include "options.hpp"
#include "record_upload.hpp"

namespace jlhost {
namespace {

// Everything is written and closed.  What a `return` would still do — free a gigabyte of record arrays page by page, take down
// the uploader and the decode pool, destroy the GPU contexts and the HIP runtime's own state — the operating system does at
// once when the process ends: 40-60 ms of the wall time of a 100k-read run.  With JL_SLOW_EXIT set the callers do not come here:
// they return and run their teardown (the long way, for leak checkers).
[[noreturn]] void end_process(int code)
{
    std::cout.flush();
    std::cerr.flush();
    fflush(nullptr);
    _exit(code);
}

void die_jl(jl_ctx *ctx, const char *what)
{
    std::cerr << "juliet: " << what << ": " << jl_last_error(ctx) << "\n";
    std::exit(3);
}

// What the device stage hands to the writers, whichever way it ran (one window, or K windows over R devices).
struct Results {
    std::vector<jl_variant> var;          // (gene, codon_pos, codon) order; col relative to the overall window
    std::vector<uint32_t> col_counts;     // [n_cols][6] of the overall window
    jl_phase_summary ps = {};
    std::vector<uint32_t> pos_cols, hap_count;   // pos_cols relative to the overall window
    std::vector<uint8_t> hap_pattern, hit;
    size_t pat_stride = 0, hit_stride = 0;       // hap_pattern[h * pat_stride + p], hit[v * hit_stride + h]
    std::vector<uint16_t> read_hap;
    // --rescue-damaged (docs/SPEC.md §14): rescue[i] of every read by the run's own positions and haplotypes; empty when no call
    // was made (no reported haplotype, or more positions asked for than the run has: every damaged read is uninformative then)
    bool rescued = false;
    uint32_t rescue_min = 0;
    std::vector<uint16_t> rescue;
    // --absorb-distance (docs/SPEC.md §22): nearest[i] and dist[i] of every read by the run's own positions and haplotypes; empty
    // when no call was made (no reported haplotype, or more positions asked for than the run has: every read is uninformative then)
    bool absorbed = false;
    uint32_t absorb_distance = 0, absorb_min = 0;
    std::vector<uint16_t> nearest;
    std::vector<uint8_t> nearest_dist;
    // --flag-recombinants (docs/SPEC.md §23): left, right, prefix and suffix of every read by the run's own positions and haplotypes
    // (empty when no device call was made: no reported haplotype, or more positions asked for than the run has — every read is
    // uninformative then), and the haplotype-level verdicts (one per reported haplotype)
    bool recomb = false;
    uint32_t recomb_min = 0;
    double recomb_ratio = 0.0;
    std::vector<uint16_t> recomb_left, recomb_right, recomb_prefix, recomb_suffix;
    std::vector<jl_hap_recombinant> recomb_haps;
    // --linkage (docs/SPEC.md §15): the three tables of ONE call over the table's distinct columns and its rows; link_var[k] = the
    // row of `var` that is variant k of the call (the rows by column: var_pos must not decrease, and genes may overlap)
    bool linked = false, link_skipped = false;
    std::vector<uint32_t> link_cols, link_var, link_var_pos, link_both, link_carry, link_joint;
    // --control (docs/SPEC.md §21): `var` was called against a control; control_cov[k] = the control's coverage at the position of
    // var[k], and var[k].expected the control's count of the codon
    bool controlled = false;
    std::vector<uint32_t> control_cov;
    // --haplotype-mutations (docs/SPEC.md §24): the evaluated positions of every gene in (gene, codon) order with their §4
    // reference codon (ref < 0: none exists at the position) and their entry of hm_cols; hm_cols: their distinct columns,
    // ascending; hm_hist[h][entry][64]: ONE per-class codon table with the run's per-read ids as labels (empty: no haplotype)
    struct HapMutPos { uint32_t gene, codon_pos, col; int ref; uint32_t entry; };
    bool hap_mutations = false;
    std::vector<HapMutPos> hm_pos;
    std::vector<uint32_t> hm_cols, hm_hist;
    // the entry of hm_cols that window column `col` is, or -1
    int hm_entry(uint32_t col) const
    {
        const auto it = std::lower_bound(hm_cols.begin(), hm_cols.end(), col);
        return it != hm_cols.end() && *it == col ? (int)(it - hm_cols.begin()) : -1;
    }
    // --call-deletions (docs/SPEC.md §16): the called positions in (gene, codon) order; ref_codon < 0: none exists at the position
    struct Deletion { uint32_t gene, codon_pos, col; int ref_codon; jl_deletion_call call; };
    bool deletions = false;
    std::vector<Deletion> del_rows;
    // --phase-deletions (docs/SPEC.md §18), --phase-insertions (§19): the phasing results above are those of the site matrix then.
    // sites: ascending by (col, kind); site_rows: the phasing table on it; var_row[k]: the row of site_rows that is row k of `var`
    bool sites_phased = false;                      // either flag
    bool dels_phased = false, ins_phased = false;   // which kinds of site were asked for
    std::vector<jl_site> sites;
    std::vector<jl_variant> site_rows;
    std::vector<uint32_t> var_row;
    // the site of the deletion called at window column `col`: its index, or -1
    int deletion_site(uint32_t col) const
    {
        for (size_t k = 0; k < sites.size(); ++k)
            if (sites[k].col == col && sites[k].kind == (uint8_t)JL_SITE_DELETION) return (int)k;
        return -1;
    }
    // §19: the distinct called alleles, ascending by (col, len, seq) — by site, then code — as the site matrix takes them, and per
    // allele its site, its code there and the first row of ins_rows that names it
    struct SiteAllele { uint32_t site, code, row; };
    std::vector<jl_insertion_allele> site_allele_keys;
    std::vector<SiteAllele> site_alleles;
    // the listed allele that row `in` of ins_rows is: its index, or -1
    int site_allele_of(const jl_insertion_allele &a) const
    {
        for (size_t i = 0; i < site_allele_keys.size(); ++i)
            if (site_allele_keys[i].col == a.col && site_allele_keys[i].len == a.len && site_allele_keys[i].seq == a.seq) return (int)i;
        return -1;
    }
    // --call-insertions (docs/SPEC.md §17): the called alleles in (gene, codon, length, sequence) order; codon_pos: the position they precede
    struct Insertion { uint32_t gene, codon_pos; jl_insertion_allele allele; jl_insertion_call call; };
    bool insertions = false;
    std::vector<Insertion> ins_rows;
    // --call-deletion-alleles (docs/SPEC.md §25): the called alleles, ascending by (col, len), and the totals of the one stage call
    struct DeletionAllele { jl_deletion_allele allele; jl_deletion_allele_call call; };
    bool del_alleles = false;
    double dal_rate = 0.0;
    uint32_t dal_min_length = 1, dal_n_alleles = 0, dal_n_tested = 0;
    uint64_t dal_runs[2] = {0, 0};
    std::vector<DeletionAllele> dal_rows;
    // the haplotype a damaged read was assigned to, or JL_HAP_DAMAGED; a read that is not damaged: its own id
    uint16_t hap_with_rescued(uint64_t i) const
    {
        if (read_hap[i] != (uint16_t)JL_HAP_DAMAGED || rescue.empty()) return read_hap[i];
        return rescue[i] < ps.n_haplotypes ? rescue[i] : (uint16_t)JL_HAP_DAMAGED;
    }
};

struct DeviceStageInput {
    const Options *opt;
    const TargetConfig *cfg;
    const std::vector<jl_gene> *genes;
    const std::vector<uint8_t> *refcodes;
    jl_params prm;
    uint32_t win_begin, n_cols;
    uint64_t n_reads;
};

// --drm-only: the codons of the config's DRMs per evaluated position of one window (doc/JULIET.md:370)
int drm_masks_of(jl_ctx *ctx, const DeviceStageInput &in, std::vector<uint64_t> &masks)
{
    const uint8_t *refp = in.refcodes->empty() ? nullptr : in.refcodes->data();
    if (jl_pileup_async(ctx, in.genes->data(), (uint32_t)in.genes->size(), refp, (uint32_t)in.refcodes->size()) != JL_OK) return 1;
    const uint32_t P = jl_n_positions(ctx);
    std::vector<uint32_t> pg(P), pk(P);
    if (jl_pileup_fetch(ctx, nullptr, pg.data(), pk.data(), nullptr, nullptr, nullptr) != JL_OK) return 1;
    masks.assign(P, 0);
    for (uint32_t p = 0; p < P; ++p) {
        const GeneCfg &g = in.cfg->genes[pg[p]];
        for (unsigned cod = 0; cod < 64; ++cod)
            if (!in.cfg->known_drms(pg[p], pk[p] + g.first_codon, translate(cod)).empty()) masks[p] |= 1ull << cod;
    }
    return 0;
}

// Everything a sample's device stage and outputs are derived from, besides its reads.
struct SampleSetup {
    TargetConfig cfg;                // the config, or the ORF "unknown" over the sample's reads
    uint32_t win_begin = 0, n_cols = 0;
    std::string chem;
    jl_params prm = {};
    std::vector<jl_gene> genes;
    std::vector<uint8_t> refcodes;
    const uint8_t *refp() const { return refcodes.empty() ? nullptr : refcodes.data(); }
};

// The genes and the window of one sample: 0, or 1 when --region leaves no gene of the config (message printed).
int sample_window(const Options &opt, const TargetConfig &config, const Decoded &d, SampleSetup &s)
{
    s.cfg = config;
    TargetConfig &cfg = s.cfg;
    int64_t ref_len = std::numeric_limits<int64_t>::max();
    if (d.ext.ref_id >= 0 && (size_t)d.ext.ref_id < d.refs.size()) ref_len = d.refs[(size_t)d.ext.ref_id].length;

    const bool have_cfg = !cfg.genes.empty();
    if (!have_cfg) {
        // no target config: one ORF over the covered window, labelled "unknown" (doc/JULIET.md:182-188);
        // --region marks the reading frame
        GeneCfg g;
        g.name = "unknown";
        g.begin = g.begin_eff = opt.have_region ? opt.region_b : (uint32_t)d.ext.min_pos + 1;
        g.end = g.end_eff = opt.have_region ? opt.region_e : (uint32_t)d.ext.max_end + 1;
        cfg.genes.push_back(g);
    } else if (opt.have_region) {
        cfg.apply_region(opt.region_b, opt.region_e);
        if (cfg.genes.empty()) { std::cerr << "juliet: --region leaves no gene of the config\n"; return 1; }
    }
    // window: the called genes plus the -3..+5 context columns (doc/JULIET.md:99-100), inside the reference
    int64_t gb = std::numeric_limits<int64_t>::max(), ge = 0;
    for (const GeneCfg &g : cfg.genes) { gb = std::min<int64_t>(gb, (int64_t)g.begin_eff - 1); ge = std::max<int64_t>(ge, (int64_t)g.end_eff - 1); }
    const int64_t wb = std::max<int64_t>(0, gb - 3);
    const int64_t we = std::max<int64_t>(wb + 1, std::min<int64_t>(ref_len, ge + 5));
    s.win_begin = (uint32_t)wb;
    s.n_cols = (uint32_t)(we - wb);
    return 0;
}

// Chemistry (from the sample's own @RG header with --chemistry auto), parameters, genes and reference codes of one sample.
void sample_params(const Options &opt, const Decoded &d, SampleSetup &s)
{
    std::string chem = opt.chemistry;
    if (chem == "auto") {
        // chemistry-keyed rates with a permissive fallback (doc/JULIET.md:221-225); the key here is the
        // platform model in the @RG line
        chem = (d.header_text.find("SEQUEL") != std::string::npos || d.header_text.find("S/P") != std::string::npos) ? "sequel" : "permissive";
        if (chem == "permissive") std::cerr << "juliet: chemistry not recognised, permissive mode is active (doc/JULIET.md:221-225)\n";
    }
    s.chem = chem;
    jl_params &prm = s.prm;
    prm.alpha = opt.alpha;
    prm.n_tests = opt.n_tests;
    if (chem == "sequel") prm.err = {0.998826, 5.8e-5, 1.0e-3};
    else prm.err = {0.99764, 1.2e-4, 2.0e-3};
    if (opt.match > 0) prm.err.match = opt.match;
    if (opt.substitution >= 0) prm.err.substitution = opt.substitution;
    prm.expected_round = opt.expected_round;
    prm.tail = opt.fisher_tail;
    prm.min_perc = opt.min_perc;
    prm.max_perc = opt.max_perc;

    s.genes.clear();
    for (const GeneCfg &g : s.cfg.genes) s.genes.push_back({g.begin_eff, g.end_eff});
    s.refcodes.clear();
    if (!s.cfg.reference_sequence.empty())
        for (char ch : s.cfg.reference_sequence) s.refcodes.push_back(base_code(ch));
}

using Tick = std::function<void(const char *)>;

// The variant table (unless `calls` is off: the pileup alone ran) and the column counts of the run last enqueued on `ctx`,
// whether it ran alone or in a group.  R.col_counts holds n_cols * 6 entries.  nullptr, or the step that failed.
const char *fetch_calls(jl_ctx *ctx, bool calls, Results &R, const Tick &tick)
{
    R.var.resize(4096);
    uint32_t nv = 0;
    if (calls && jl_call_fetch(ctx, R.var.data(), 4096, &nv) != JL_OK) return "call fetch";
    R.var.resize(nv);
    tick("  wait for the run + table");
    if (jl_pileup_fetch(ctx, R.col_counts.data(), nullptr, nullptr, nullptr, nullptr, nullptr) != JL_OK) return "pileup fetch";
    tick("  column counts");
    return nullptr;
}

// The haplotypes and the per-read ids of a phasing run, after fetch_calls.
const char *fetch_phase(jl_ctx *ctx, uint64_t n_reads, Results &R)
{
    const uint32_t cap_var = std::max<uint32_t>(1, (uint32_t)R.var.size());
    R.pos_cols.resize(cap_var);
    R.hap_count.resize(JL_MAX_HAPLOTYPES);
    R.hap_pattern.resize((size_t)JL_MAX_HAPLOTYPES * cap_var);
    R.hit.resize((size_t)cap_var * JL_MAX_HAPLOTYPES);
    R.read_hap.resize(n_reads);
    R.pat_stride = cap_var;
    R.hit_stride = JL_MAX_HAPLOTYPES;
    if (jl_phase_fetch(ctx, &R.ps, R.pos_cols.data(), R.hap_count.data(), R.hap_pattern.data(), R.hit.data(), R.read_hap.data(), nullptr, cap_var) != JL_OK)
        return "phase fetch";
    return nullptr;
}

// --rescue-damaged, after fetch_phase: one call of the rule of docs/SPEC.md §14 with the run's own positions and haplotypes.
const char *fetch_rescue(jl_ctx *ctx, uint32_t min_positions, Results &R)
{
    R.rescued = true;
    R.rescue_min = min_positions;
    R.rescue.clear();
    if (R.ps.n_haplotypes == 0 || min_positions > R.ps.n_positions) return nullptr;
    if (jl_phase_rescue_async(ctx, R.pos_cols.data(), R.ps.n_positions, R.hap_pattern.data(), (uint32_t)R.pat_stride, R.ps.n_haplotypes,
                              min_positions) != JL_OK)
        return "rescue";
    R.rescue.resize(R.read_hap.size());
    if (jl_phase_rescue_fetch(ctx, R.rescue.data(), nullptr, nullptr) != JL_OK) return "rescue fetch";
    return nullptr;
}

// --absorb-distance, after fetch_phase: one call of the rule of docs/SPEC.md §22 with the run's own positions and haplotypes.
const char *fetch_absorb(jl_ctx *ctx, uint32_t min_positions, uint32_t max_distance, Results &R)
{
    R.absorbed = true;
    R.absorb_min = min_positions;
    R.absorb_distance = max_distance;
    R.nearest.clear();
    R.nearest_dist.clear();
    if (R.ps.n_haplotypes == 0 || min_positions > R.ps.n_positions) return nullptr;
    if (jl_phase_nearest_async(ctx, R.pos_cols.data(), R.ps.n_positions, R.hap_pattern.data(), (uint32_t)R.pat_stride, R.ps.n_haplotypes,
                               min_positions, max_distance) != JL_OK)
        return "absorb";
    R.nearest.resize(R.read_hap.size());
    R.nearest_dist.resize(R.read_hap.size());
    if (jl_phase_nearest_fetch(ctx, R.nearest.data(), R.nearest_dist.data(), nullptr, nullptr) != JL_OK) return "absorb fetch";
    return nullptr;
}

// --flag-recombinants, after fetch_phase: one device call of the rule of docs/SPEC.md §23 with the run's own positions and
// haplotypes, then the haplotype-level rule on the host with the run's own counts.
const char *fetch_recombinants(jl_ctx *ctx, uint32_t min_positions, double parent_ratio, Results &R)
{
    R.recomb = true;
    R.recomb_min = min_positions;
    R.recomb_ratio = parent_ratio;
    for (auto *v : {&R.recomb_left, &R.recomb_right, &R.recomb_prefix, &R.recomb_suffix}) v->clear();
    R.recomb_haps.clear();
    if (R.ps.n_haplotypes == 0) return nullptr;
    if (R.ps.n_positions) {
        R.recomb_haps.resize(R.ps.n_haplotypes);
        if (jl_haplotype_recombinants(R.hap_pattern.data(), (uint32_t)R.pat_stride, R.ps.n_haplotypes, R.ps.n_positions, R.hap_count.data(), parent_ratio,
                                      R.recomb_haps.data()) != JL_OK)
            return "haplotype recombinants";
    }
    if (min_positions > R.ps.n_positions) return nullptr;
    if (jl_phase_recombinants_async(ctx, R.pos_cols.data(), R.ps.n_positions, R.hap_pattern.data(), (uint32_t)R.pat_stride, R.ps.n_haplotypes,
                                    min_positions) != JL_OK)
        return "recombinants";
    for (auto *v : {&R.recomb_left, &R.recomb_right, &R.recomb_prefix, &R.recomb_suffix}) v->resize(R.read_hap.size());
    if (jl_phase_recombinants_fetch(ctx, R.recomb_left.data(), R.recomb_right.data(), R.recomb_prefix.data(), R.recomb_suffix.data(), nullptr,
                                    nullptr) != JL_OK)
        return "recombinants fetch";
    return nullptr;
}

// --linkage, after fetch_calls: ONE call of docs/SPEC.md §15 with the table's distinct columns as positions and its rows as variants.
// No variant: no call.  More than JL_LINK_MAX variants or positions: a warning, no call, the block says "skipped".
const char *fetch_linkage(jl_ctx *ctx, Results &R)
{
    R.linked = true;
    R.link_skipped = false;
    const uint32_t V = (uint32_t)R.var.size();
    R.link_var.resize(V);
    for (uint32_t k = 0; k < V; ++k) R.link_var[k] = k;
    std::stable_sort(R.link_var.begin(), R.link_var.end(), [&](uint32_t a, uint32_t b) { return R.var[a].col < R.var[b].col; });
    R.link_cols.clear();
    R.link_var_pos.resize(V);
    std::vector<uint8_t> codon(V);
    for (uint32_t k = 0; k < V; ++k) {
        const jl_variant &f = R.var[R.link_var[k]];
        if (R.link_cols.empty() || R.link_cols.back() != f.col) R.link_cols.push_back(f.col);
        R.link_var_pos[k] = (uint32_t)R.link_cols.size() - 1u;
        codon[k] = f.codon;
    }
    if (V == 0) return nullptr;
    const uint32_t P = (uint32_t)R.link_cols.size();
    if (V > (uint32_t)JL_LINK_MAX || P > (uint32_t)JL_LINK_MAX) {
        std::cerr << "juliet: warning: --linkage takes at most " << (int)JL_LINK_MAX << " variants at " << (int)JL_LINK_MAX << " positions, the table has " << V
                  << " at " << P << ": no pair is tested (narrow the table with --min-perc / --max-perc / --region)\n";
        R.link_skipped = true;
        return nullptr;
    }
    if (jl_variant_linkage_async(ctx, R.link_cols.data(), P, R.link_var_pos.data(), codon.data(), V) != JL_OK) return "linkage";
    R.link_both.resize((size_t)P * P), R.link_carry.resize((size_t)V * P), R.link_joint.resize((size_t)V * V);
    if (jl_variant_linkage_fetch(ctx, R.link_both.data(), R.link_carry.data(), R.link_joint.data()) != JL_OK) return "linkage fetch";
    return nullptr;
}

// --call-deletions, after fetch_calls: ONE call of docs/SPEC.md §16 on the window that was called, then the test of every evaluated
// codon position (§3's positions of the run's plan) with the run's own parameters and resolved Bonferroni factor.  --drm-only: no
// DRM notation names a deletion, nothing is tested.
const char *fetch_deletions(jl_ctx *ctx, const Options &opt, const jl_params &prm, const std::vector<jl_gene> &genes,
                            const std::vector<uint8_t> &refcodes, uint32_t win_begin, uint32_t n_cols, Results &R)
{
    R.deletions = true;
    R.del_rows.clear();
    if (opt.drm_only || n_cols < 3) return nullptr;
    if (jl_codon_deletions_async(ctx) != JL_OK) return "codon deletions";
    std::vector<uint32_t> cnt((size_t)(n_cols - 2) * 4);
    if (jl_codon_deletions_fetch(ctx, cnt.data()) != JL_OK) return "codon deletions fetch";
    const uint32_t P = jl_n_positions(ctx);
    std::vector<uint32_t> pg(P), pk(P), pc(P), hist;
    const bool majority = refcodes.empty();   // (§4: the reference codon is the majority codon then)
    if (majority) hist.resize((size_t)P * 64);
    if (P && jl_pileup_fetch(ctx, nullptr, pg.data(), pk.data(), pc.data(), majority ? hist.data() : nullptr, nullptr) != JL_OK) return "positions";
    double n_tests = prm.n_tests;
    if (!(n_tests > 0.0)) {   // §5: the codons of all genes
        n_tests = 0.0;
        for (const jl_gene &g : genes)
            if (g.begin != 0 && g.end > g.begin) n_tests += (double)((g.end - g.begin) / 3);
    }
    for (uint32_t p = 0; p < P; ++p) {
        jl_deletion_call dc;
        if (jl_deletion_test(&cnt[(size_t)pc[p] * 4], &prm, n_tests, &dc) != JL_OK) return "deletion test";
        if (!dc.called) continue;
        int ref = -1;
        if (majority) {
            const uint32_t *h = &hist[(size_t)p * 64];
            uint32_t best = 0;
            for (uint32_t k = 1; k < 64; ++k)
                if (h[k] > h[best]) best = k;
            if (h[best]) ref = (int)best;
        } else {
            const size_t r = (size_t)win_begin + pc[p];
            if (r + 2 < refcodes.size() && refcodes[r] < 4 && refcodes[r + 1] < 4 && refcodes[r + 2] < 4)
                ref = 16 * refcodes[r] + 4 * refcodes[r + 1] + refcodes[r + 2];
        }
        R.del_rows.push_back({pg[p], pk[p], pc[p], ref, dc});
    }
    return nullptr;
}

// --haplotype-mutations, after fetch_phase (and after the site matrix's phasing, whose ids are the labels then): the evaluated
// positions of the run's plan on `ctx` with their §4 reference codon, and ONE jl_class_codons_async (docs/SPEC.md §24) at their
// distinct columns with the plain per-read ids as labels and the reported haplotypes as classes.  No haplotype: no call.
const char *fetch_haplotype_mutations(jl_ctx *ctx, const std::vector<uint8_t> &refcodes, uint32_t win_begin, Results &R)
{
    R.hap_mutations = true;
    R.hm_pos.clear(), R.hm_cols.clear(), R.hm_hist.clear();
    const uint32_t P = jl_n_positions(ctx), H = R.ps.n_haplotypes;
    std::vector<uint32_t> pg(P), pk(P), pc(P), hist;
    const bool majority = refcodes.empty();   // (§4: the reference codon is the sample's majority codon then)
    if (majority) hist.resize((size_t)P * 64);
    if (P && jl_pileup_fetch(ctx, nullptr, pg.data(), pk.data(), pc.data(), majority ? hist.data() : nullptr, nullptr) != JL_OK) return "positions";
    R.hm_cols.assign(pc.begin(), pc.end());
    std::sort(R.hm_cols.begin(), R.hm_cols.end());
    R.hm_cols.erase(std::unique(R.hm_cols.begin(), R.hm_cols.end()), R.hm_cols.end());
    for (uint32_t p = 0; p < P; ++p) {
        int ref = -1;
        if (majority) {
            const uint32_t *h = &hist[(size_t)p * 64];
            uint32_t best = 0;
            for (uint32_t k = 1; k < 64; ++k)
                if (h[k] > h[best]) best = k;
            if (h[best]) ref = (int)best;
        } else {
            const size_t r = (size_t)win_begin + pc[p];
            if (r + 2 < refcodes.size() && refcodes[r] < 4 && refcodes[r + 1] < 4 && refcodes[r + 2] < 4)
                ref = 16 * refcodes[r] + 4 * refcodes[r + 1] + refcodes[r + 2];
        }
        R.hm_pos.push_back({pg[p], pk[p], pc[p], ref, (uint32_t)R.hm_entry(pc[p])});
    }
    std::stable_sort(R.hm_pos.begin(), R.hm_pos.end(), [](const Results::HapMutPos &a, const Results::HapMutPos &b) {
        return a.gene != b.gene ? a.gene < b.gene : a.codon_pos < b.codon_pos;
    });
    if (H == 0 || R.hm_cols.empty()) return nullptr;
    if (jl_class_codons_async(ctx, R.read_hap.data(), H, R.hm_cols.data(), (uint32_t)R.hm_cols.size()) != JL_OK) return "class codons";
    R.hm_hist.resize((size_t)H * R.hm_cols.size() * 64);
    if (jl_class_codons_fetch(ctx, R.hm_hist.data(), nullptr) != JL_OK) return "class codons fetch";
    return nullptr;
}

// --phase-deletions and / or --phase-insertions, after fetch_calls, fetch_deletions and fetch_insertions: the sites and the phasing
// table of docs/SPEC.md §18 and §19 from the variant table, the called deletions (`dels`) and the called insertion alleles (`ins`),
// the site matrix of the window on `ctx` in a context of its own on the same device and stream, and the phasing that exists on it.
// Its results replace the plain run's in R; the read order is the window's.  No site: nothing to phase, R keeps the plain run's.
const char *fetch_sites_phase(jl_ctx *ctx, int device, uint32_t min_reads, uint64_t n_reads, bool dels, bool ins, Results &R, jl_ctx **pc_out)
{
    R.sites_phased = true;
    R.dels_phased = dels, R.ins_phased = ins;
    R.sites.clear(), R.site_rows.clear(), R.site_allele_keys.clear(), R.site_alleles.clear();
    std::vector<uint32_t> order(R.var.size());   // the rows by column (genes may overlap), the rows of one column in the table's order
    for (uint32_t k = 0; k < order.size(); ++k) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return R.var[a].col < R.var[b].col; });
    R.var_row.assign(R.var.size(), 0);
    // the sites: the distinct columns of the variant rows, of the called deletions and of the called insertion alleles over all genes
    std::vector<std::pair<uint32_t, uint8_t>> keys;   // (col, kind)
    for (const jl_variant &v : R.var) keys.emplace_back(v.col, (uint8_t)JL_SITE_CODON);
    if (dels)
        for (const Results::Deletion &d : R.del_rows) keys.emplace_back(d.col, (uint8_t)JL_SITE_DELETION);
    if (ins)
        for (const Results::Insertion &in : R.ins_rows) {
            keys.emplace_back(in.allele.col, (uint8_t)JL_SITE_INSERTION);
            R.site_allele_keys.push_back(jl_insertion_allele{in.allele.col, in.allele.len, in.allele.seq, 0, 0});
        }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    auto allele_less = [](const jl_insertion_allele &x, const jl_insertion_allele &y) {
        return x.col != y.col ? x.col < y.col : x.len != y.len ? x.len < y.len : x.seq < y.seq;
    };
    std::sort(R.site_allele_keys.begin(), R.site_allele_keys.end(), allele_less);   // (an allele called for two genes: once)
    R.site_allele_keys.erase(std::unique(R.site_allele_keys.begin(), R.site_allele_keys.end(),
                                         [&](const jl_insertion_allele &x, const jl_insertion_allele &y) { return !allele_less(x, y) && !allele_less(y, x); }),
                             R.site_allele_keys.end());
    size_t v = 0, a = 0;
    for (size_t i = 0; i < keys.size(); ++i) {
        const uint32_t col = keys[i].first, k = (uint32_t)R.sites.size();
        if (keys[i].second == (uint8_t)JL_SITE_CODON) {   // filled with the reference codon where a deletion site follows
            const bool deleted_too = i + 1 < keys.size() && keys[i + 1] == std::make_pair(col, (uint8_t)JL_SITE_DELETION);
            R.sites.push_back(jl_site{col, (uint8_t)JL_SITE_CODON, deleted_too ? R.var[order[v]].ref_codon : (uint8_t)JL_SITE_NO_FILL, 0});
            for (; v < order.size() && R.var[order[v]].col == col; ++v) {
                R.var_row[order[v]] = (uint32_t)R.site_rows.size();
                R.site_rows.push_back(R.var[order[v]]);
                R.site_rows.back().col = 3u * k;
            }
        } else if (keys[i].second == (uint8_t)JL_SITE_DELETION) {   // a deletion site and its pseudo-row
            jl_variant row = {};
            row.col = 3u * k, row.codon = (uint8_t)JL_SITE_DELETED, row.ref_codon = (uint8_t)JL_SITE_PRESENT;
            R.sites.push_back(jl_site{col, (uint8_t)JL_SITE_DELETION, (uint8_t)JL_SITE_NO_FILL, 0});
            R.site_rows.push_back(row);
        } else {   // an insertion site and a pseudo-row per called allele, ascending by code
            R.sites.push_back(jl_site{col, (uint8_t)JL_SITE_INSERTION, (uint8_t)JL_SITE_NO_FILL, 0});
            for (uint32_t code = 1; a < R.site_allele_keys.size() && R.site_allele_keys[a].col == col; ++a, ++code) {
                if (code > (uint32_t)JL_SITE_INS_MAX_ALLELES) {
                    std::cerr << "juliet: --phase-insertions: more than " << (int)JL_SITE_INS_MAX_ALLELES << " called alleles at one junction (window column " << col
                              << "), a site holds that many (narrow the calls with --min-perc / --insertion-rate)\n";
                    std::exit(2);
                }
                jl_variant row = {};
                row.col = 3u * k, row.codon = (uint8_t)code, row.ref_codon = (uint8_t)JL_SITE_INS_NONE;
                R.site_rows.push_back(row);
                uint32_t first = 0;
                while (R.site_allele_of(R.ins_rows[first].allele) != (int)a) ++first;
                R.site_alleles.push_back({k, code, first});
            }
        }
    }
    if (R.sites.empty()) return nullptr;
    if (R.site_rows.size() > 4096) {
        std::cerr << "juliet: " << (dels ? "--phase-deletions" : "--phase-insertions") << ": " << R.site_rows.size()
                  << " variants and deletion sites, phasing takes 4096 (narrow the table with --min-perc / --max-perc / --region)\n";
        std::exit(2);
    }
    jl_ctx *pc = nullptr;
    if (jl_ctx_create(device, jl_ctx_stream(ctx), &pc) != JL_OK) return "context of the site matrix";
    *pc_out = pc;
    if (!ins) {
        if (jl_sites_assemble(pc, ctx, R.sites.data(), (uint32_t)R.sites.size()) != JL_OK) return "site matrix";
    } else if (jl_sites_assemble_alleles(pc, ctx, R.sites.data(), (uint32_t)R.sites.size(), R.site_allele_keys.data(), (uint32_t)R.site_allele_keys.size()) != JL_OK)
        return "site matrix";
    if (jl_phase_async(pc, R.site_rows.data(), (uint32_t)R.site_rows.size(), min_reads) != JL_OK) return "phasing of the site matrix";
    const uint32_t cap_var = (uint32_t)R.site_rows.size();
    R.pos_cols.assign(cap_var, 0);
    R.hap_count.assign(JL_MAX_HAPLOTYPES, 0);
    R.hap_pattern.assign((size_t)JL_MAX_HAPLOTYPES * cap_var, 0);
    R.hit.assign((size_t)cap_var * JL_MAX_HAPLOTYPES, 0);
    R.read_hap.assign(n_reads, 0);
    R.pat_stride = cap_var;
    R.hit_stride = JL_MAX_HAPLOTYPES;
    if (jl_phase_fetch(pc, &R.ps, R.pos_cols.data(), R.hap_count.data(), R.hap_pattern.data(), R.hit.data(), R.read_hap.data(), nullptr, cap_var) != JL_OK)
        return "phase fetch of the site matrix";
    return nullptr;
}

// --call-insertions, after fetch_calls: the junction counters and the allele table the record ingest of this window left (docs/SPEC.md
// §17), then the test of every allele whose junction is the start column of an evaluated codon position that is not its gene's
// first, with the run's own parameters and resolved Bonferroni factor.  An allele that splits a codon of a gene is none of that
// gene's.  --drm-only: no DRM notation names an insertion, nothing is tested.
const char *fetch_insertions(jl_ctx *ctx, const Options &opt, const jl_params &prm, const std::vector<jl_gene> &genes, uint32_t n_cols, Results &R)
{
    R.insertions = true;
    R.ins_rows.clear();
    if (opt.drm_only) return nullptr;
    std::vector<uint32_t> jcnt((size_t)n_cols * 4);
    uint32_t n = 0;
    if (jl_insertion_alleles_fetch(ctx, jcnt.data(), nullptr, 0, &n) != JL_OK) return "insertion alleles";
    std::vector<jl_insertion_allele> rows(n);
    if (n && jl_insertion_alleles_fetch(ctx, nullptr, rows.data(), n, &n) != JL_OK) return "insertion alleles fetch";
    const uint32_t P = jl_n_positions(ctx);
    std::vector<uint32_t> pg(P), pk(P), pc(P);
    if (P && jl_pileup_fetch(ctx, nullptr, pg.data(), pk.data(), pc.data(), nullptr, nullptr) != JL_OK) return "positions";
    double n_tests = prm.n_tests;
    if (!(n_tests > 0.0)) {   // §5: the codons of all genes
        n_tests = 0.0;
        for (const jl_gene &g : genes)
            if (g.begin != 0 && g.end > g.begin) n_tests += (double)((g.end - g.begin) / 3);
    }
    const double rate = opt.have_insertion_rate ? opt.insertion_rate : prm.err.deletion;
    auto by_col = [](const jl_insertion_allele &a, uint32_t col) { return a.col < col; };
    for (uint32_t p = 0; p < P; ++p) {
        if (pk[p] == 0 || pc[p] == 0) continue;   // in front of the gene's first codon: not inside the gene
        for (auto it = std::lower_bound(rows.begin(), rows.end(), pc[p], by_col); it != rows.end() && it->col == pc[p]; ++it) {
            jl_insertion_call ic;
            if (jl_insertion_test(it->count, &jcnt[(size_t)pc[p] * 4], &prm, rate, n_tests, &ic) != JL_OK) return "insertion test";
            if (ic.called) R.ins_rows.push_back({pg[p], pk[p], *it, ic});
        }
    }
    return nullptr;
}

// --call-deletion-alleles, after fetch_calls: ONE call of docs/SPEC.md §25 on the window that was called, then the test of every
// allele of --min-deletion-length bases or more with the run's own parameters and resolved Bonferroni factor.
const char *fetch_deletion_alleles(jl_ctx *ctx, const Options &opt, const jl_params &prm, const std::vector<jl_gene> &genes, Results &R)
{
    R.del_alleles = true;
    R.dal_rows.clear();
    R.dal_rate = opt.have_deletion_allele_rate ? opt.deletion_allele_rate : prm.err.deletion;
    R.dal_min_length = opt.min_deletion_length;
    if (jl_deletion_alleles_async(ctx) != JL_OK) return "deletion alleles";
    uint32_t n = 0;
    if (jl_deletion_alleles_fetch(ctx, R.dal_runs, nullptr, nullptr, 0, &n) != JL_OK) return "deletion alleles fetch";
    std::vector<jl_deletion_allele> rows(n);
    if (n && jl_deletion_alleles_fetch(ctx, nullptr, nullptr, rows.data(), n, &n) != JL_OK) return "deletion alleles fetch";
    double n_tests = prm.n_tests;
    if (!(n_tests > 0.0)) {   // §5: the codons of all genes
        n_tests = 0.0;
        for (const jl_gene &g : genes)
            if (g.begin != 0 && g.end > g.begin) n_tests += (double)((g.end - g.begin) / 3);
    }
    if (!(n_tests > 0.0)) n_tests = 1.0;
    R.dal_n_alleles = n, R.dal_n_tested = 0;
    for (const jl_deletion_allele &a : rows) {
        if (a.len < opt.min_deletion_length) continue;
        jl_deletion_allele_call dc;
        if (jl_deletion_allele_test(a.count, a.flank, &prm, R.dal_rate, n_tests, &dc) != JL_OK) return "deletion allele test";
        R.dal_n_tested++;
        if (dc.called) R.dal_rows.push_back({a, dc});
    }
    return nullptr;
}

const Tick quiet_tick = [](const char *) {};   // for the callers that print no laps (--batch, --mix)

IngestOptions ingest_options(const Options &opt)
{
    IngestOptions io;
    io.min_qv = opt.min_qv;
    io.min_rq = opt.min_rq;
    io.qv_mask = opt.qv_upload_mask;
    return io;
}

// How a step of loading a sample ended.  The callers keep their own policies and map this: a single run and --mix print and leave
// (exit_code_of), a batch fails the sample or stops (BatchRunner::prepare).
enum class Outcome { ok, input, device };   // input: the records or the file are at fault
struct Status {
    Outcome outcome = Outcome::ok;
    std::string what;          // the step that failed (device), or what is wrong with the input
    jl_ctx *ctx = nullptr;     // device: the context whose jl_last_error tells more (nullptr: none does)
    int rc = JL_OK;            // device: the status of the call that failed
    std::string text() const { return ctx ? what + ": " + jl_last_error(ctx) : what; }
};

// A sample on its context(s): what load_sample leaves.  The uploader stays (its contexts by index: ctx(k)) until the owner drops it.
struct SampleLoad : Status {
    Decoded dec;
    std::vector<std::string> names;
    uint64_t n_reads = 0;
    std::unique_ptr<RecordUploader> uploader;   // none: a GPU-free decode (no context asked for)
};

// Loading, first half: the uploader, the decode (a file that cannot be decoded throws), the no-alignments check.  The contexts
// may still be coming up: what needs no device (the sample's setup, --dump-msa) runs between the halves of a single run.
SampleLoad load_begin(const std::string &bam, const IngestOptions &io, const std::vector<CtxFuture> &ctxs, const Options &opt, const Tick &tick)
{
    SampleLoad l;
    if (!ctxs.empty()) l.uploader.reset(new RecordUploader(ctxs, file_bytes(bam), opt.min_qv > 0, io.qv_mask));
    RecordArrays rec;
    l.dec = decode_bam(bam, io, l.uploader.get(), rec);
    tick("bam decode");
    if (l.dec.ext.n_reads == 0) {
        l.outcome = Outcome::input;
        l.what = "no primary or supplementary alignments";
    }
    return l;
}

// Loading, second half: waits for the contexts and for the uploads, checks that every read arrived, takes the names.  The records
// are on every context when this leaves `l` ok; their window is not ingested yet (ingest_window, or per window: run_rank).
void load_finish(SampleLoad &l, const std::vector<CtxFuture> &ctxs, const Tick &tick)
{
    auto fail = [&](const char *what, jl_ctx *c, int rc) {
        l.outcome = Outcome::device;
        l.what = what;
        l.ctx = c;
        l.rc = rc;
    };
    jl_ctx *ctx = nullptr;
    for (const CtxFuture &f : ctxs) {
        const auto up = f.get();
        if (up.first != JL_OK) return fail("no usable GPU (this tool has no CPU fallback)", nullptr, up.first);
        if (!ctx) ctx = up.second;
    }
    tick("context ready");
    if (const int rc = l.uploader->finish()) return fail("record upload", l.uploader->failed() ? l.uploader->failed() : ctx, rc);
    if (l.uploader->n_reads != l.dec.ext.n_reads) return fail("record upload lost reads", nullptr, JL_OK);
    l.names.swap(l.uploader->names);
    l.n_reads = l.dec.ext.n_reads;
    tick("rest of the upload");
}

SampleLoad load_sample(const std::string &bam, const IngestOptions &io, const std::vector<CtxFuture> &ctxs, const Options &opt, const Tick &tick)
{
    SampleLoad l = load_begin(bam, io, ctxs, opt, tick);
    if (l.outcome == Outcome::ok) load_finish(l, ctxs, tick);
    return l;
}

// The window ingest of a loaded sample on ONE context (K windows ingest per window instead: run_rank).  With a consensus asked
// for, the insertion counters too: fuse keeps in-frame insertions (doc/FUSE.md:19); with --call-insertions the insertion alleles.
Status ingest_window(jl_ctx *ctx, uint32_t n_cols, uint32_t win_begin, const Options &opt)
{
    Status st;
    if (!opt.consensus.empty()) jl_msa_track_insertions(ctx, 1);
    if (opt.call_insertions) jl_msa_track_insertion_alleles(ctx, 1);
    if (opt.phase_insertions) jl_msa_track_insertion_reads(ctx, 1);   // (docs/SPEC.md §19: which read carries which insertion)
    if (const int rc = jl_records_finish(ctx, n_cols, win_begin, opt.min_qv)) {
        st.outcome = Outcome::device;
        st.what = "ingest";
        st.ctx = ctx;
        st.rc = rc;
    }
    return st;
}

// The policy of a single run and of --mix: 0 when the step went fine; an input failure is printed and is the exit status 2; a
// device failure ends the process (3).
int exit_code_of(const Status &st, const std::string &file)
{
    if (st.outcome == Outcome::ok) return 0;
    if (st.outcome == Outcome::device) die_jl(st.ctx, st.what.c_str());
    std::cerr << "juliet: " << st.what << " in " << file << "\n";
    return 2;
}

// What --downsample / --mix did to a sample: the `sampling` block of the JSON's input section, present only when reads were chosen.
struct SamplingInfo {
    bool acted = false;
    uint64_t seed = 0;
    struct Source { std::string file; uint64_t reads, kept; };
    std::vector<Source> sources;
};

// --downsample on a window that is resident on `ctx` (its reads' names in `names`): when it holds more than opt.downsample reads,
// the reads of jl_sample_reads are gathered into `taken` — a second context of the device, on the same stream — and names / n_reads
// follow the indices.  JL_OK, or the status of the call that failed (jl_last_error(taken)); *acted: the window to run is `taken` now.
int downsample_window(const Options &opt, const std::string &bam, jl_ctx *ctx, jl_ctx *taken, std::vector<std::string> &names, uint64_t &n_reads,
                      SamplingInfo &info, bool *acted)
{
    *acted = false;
    if (!opt.have_downsample || n_reads <= opt.downsample) return JL_OK;
    std::vector<uint32_t> idx((size_t)opt.downsample);
    uint64_t kept = 0;
    if (const int rc = jl_sample_reads(n_reads, opt.downsample, opt.sample_seed, idx.data(), &kept)) return rc;
    const jl_take_part part = {ctx, idx.data(), kept};
    if (const int rc = jl_msa_take(taken, &part, 1)) return rc;
    std::vector<std::string> chosen((size_t)kept);
    for (uint64_t j = 0; j < kept; ++j) chosen[(size_t)j].swap(names[idx[(size_t)j]]);
    names.swap(chosen);
    info.acted = true;
    info.seed = opt.sample_seed;
    info.sources.assign(1, {bam, n_reads, kept});
    n_reads = kept;
    *acted = true;
    return JL_OK;
}

// What the read filter did to a sample (docs/SPEC.md §20): the `read_filter` block of the JSON's input section, present when a rule
// or --read-stats was given.
struct ReadFilterInfo {
    bool ran = false;
    bool reference = false;      // the compare row: the config's referenceSequence over the window, or the majority consensus
    uint64_t reads = 0, kept = 0;
    uint64_t failed[5] = {0, 0, 0, 0, 0};
    std::vector<uint8_t> compare;   // the compare row it used, of the window as ingested (the hypermutation filter takes it over)
};

// The row a per-read stage compares with (docs/SPEC.md §20, §26): the config's referenceSequence over the window when it covers it
// (*reference), else the majority consensus of the window resident on `ctx`: a plain pileup, then its consensus.  JL_OK, or the
// status of the call that failed (*what says which).
int window_compare_row(const SampleSetup &smp, jl_ctx *ctx, std::vector<uint8_t> &compare, bool *reference, const char **what)
{
    const uint32_t n_cols = smp.n_cols;
    compare.resize(n_cols);
    *reference = smp.refcodes.size() >= (size_t)smp.win_begin + n_cols;
    if (*reference) {
        std::copy_n(smp.refcodes.begin() + smp.win_begin, n_cols, compare.begin());
        return JL_OK;
    }
    *what = "pileup of the compare row";
    if (const int rc = jl_pileup_async(ctx, smp.genes.data(), (uint32_t)smp.genes.size(), smp.refp(), (uint32_t)smp.refcodes.size())) return rc;
    *what = "consensus of the compare row";
    return jl_consensus_fetch(ctx, compare.data());
}

// The read filter on a window that is resident on `ctx` (its reads' names in `names`): the compare row, the per-read counters
// (jl_read_stats_async), --read-stats, the rule (jl_read_filter), and — when it drops a read — the kept reads gathered into `taken`,
// a second context of the device on the same stream; names / n_reads follow the indices.  *acted: the window to run is `taken` now.
// An input failure: no read is kept, or the --read-stats file cannot be written.
Status read_filter_window(const Options &opt, const SampleSetup &smp, jl_ctx *ctx, jl_ctx *taken, std::vector<std::string> &names, uint64_t &n_reads,
                          ReadFilterInfo &info, bool *acted)
{
    Status st;
    *acted = false;
    auto device = [&](const char *what, jl_ctx *c, int rc) {
        st.outcome = Outcome::device, st.what = what, st.ctx = c, st.rc = rc;
        return st;
    };
    std::vector<uint8_t> &compare = info.compare;
    const char *what = "";
    if (const int rc = window_compare_row(smp, ctx, compare, &info.reference, &what)) return device(what, ctx, rc);
    std::vector<uint32_t> stats((size_t)JL_READ_STATS * n_reads);
    if (const int rc = jl_read_stats_async(ctx, compare.data())) return device("read stats", ctx, rc);
    if (const int rc = jl_read_stats_fetch(ctx, stats.data())) return device("read stats fetch", ctx, rc);
    info.ran = true;
    info.reads = info.kept = n_reads;
    if (!opt.read_stats_out.empty()) {
        std::string text;
        for (uint64_t i = 0; i < n_reads; ++i) {
            text += names[(size_t)i];
            for (uint32_t k = 0; k < JL_READ_STATS; ++k) text += "\t" + std::to_string(stats[(size_t)(k * n_reads + i)]);
            text += "\n";
        }
        std::ofstream f(opt.read_stats_out, std::ios::binary);
        f << text;
        f.close();
        if (!f) {
            st.outcome = Outcome::input, st.what = "cannot write " + opt.read_stats_out + " for the reads";
            return st;
        }
    }
    if (!opt.read_rule_set) return st;
    std::vector<uint32_t> idx((size_t)n_reads);
    uint64_t kept = 0;
    if (const int rc = jl_read_filter(stats.data(), n_reads, &opt.read_rule, idx.data(), &kept, info.failed)) return device("read filter", nullptr, rc);
    info.kept = kept;
    if (kept == 0) {
        st.outcome = Outcome::input;
        st.what = "the read filter keeps none of " + std::to_string(n_reads) + " reads (failed min_bases " + std::to_string(info.failed[0]) + ", mismatches " +
                  std::to_string(info.failed[1]) + ", mismatch_perc " + std::to_string(info.failed[2]) + ", gap_perc " + std::to_string(info.failed[3]) +
                  ", n_perc " + std::to_string(info.failed[4]) + ")";
        return st;
    }
    if (kept == n_reads) return st;
    const jl_take_part part = {ctx, idx.data(), kept};
    if (const int rc = jl_msa_take(taken, &part, 1)) return device("take of the read filter", taken, rc);
    std::vector<std::string> chosen((size_t)kept);
    for (uint64_t j = 0; j < kept; ++j) chosen[(size_t)j].swap(names[idx[(size_t)j]]);
    names.swap(chosen);
    n_reads = kept;
    *acted = true;
    return st;
}

// What the hypermutation filter did to a sample (docs/SPEC.md §26): the `hypermutation` block of the JSON's input section, present
// when --drop-hypermutated or --hypermut-report was given.
struct HypermutInfo {
    bool ran = false;
    bool reference = false;      // the row whose G are the sites: the config's referenceSequence over the window, or the majority consensus
    bool dropped = false;        // --drop-hypermutated was given
    double alpha = 0.05;
    uint64_t reads = 0, flagged = 0, kept = 0;
    std::vector<uint8_t> ref;    // the row it used (the reading-frame filter takes it over)
};

// The hypermutation filter on a window that is resident on `ctx` (its reads' names in `names`) — what the read filter kept, when
// there is one: the reference row (`row`: the read filter's, when it ran; else chosen as the read filter chooses), the per-read
// counters and their test (jl_read_hypermut_async), --hypermut-report, the rule (jl_hypermut_filter) and — when it drops a read —
// the kept reads gathered into `taken`, a second context of the device on the same stream; names / n_reads follow the indices.
// *acted: the window to run is `taken` now.  An input failure: no read is kept, or the report cannot be written.
Status hypermut_window(const Options &opt, const SampleSetup &smp, jl_ctx *ctx, jl_ctx *taken, const ReadFilterInfo *row,
                       std::vector<std::string> &names, uint64_t &n_reads, HypermutInfo &info, bool *acted)
{
    Status st;
    *acted = false;
    auto device = [&](const char *what, jl_ctx *c, int rc) {
        st.outcome = Outcome::device, st.what = what, st.ctx = c, st.rc = rc;
        return st;
    };
    std::vector<uint8_t> &ref = info.ref;
    if (row && row->ran) ref = row->compare, info.reference = row->reference;
    else {
        const char *what = "";
        if (const int rc = window_compare_row(smp, ctx, ref, &info.reference, &what)) return device(what, ctx, rc);
    }
    std::vector<uint32_t> counts((size_t)JL_HM_COUNTERS * n_reads);
    std::vector<double> p((size_t)n_reads);
    if (const int rc = jl_read_hypermut_async(ctx, ref.data())) return device("hypermutation counters", ctx, rc);
    if (const int rc = jl_read_hypermut_fetch(ctx, counts.data(), p.data(), nullptr)) return device("hypermutation counters fetch", ctx, rc);
    info.ran = true;
    info.dropped = opt.drop_hypermutated;
    info.alpha = opt.hypermut_alpha;
    info.reads = info.kept = n_reads;
    std::vector<uint32_t> idx((size_t)n_reads);
    uint64_t kept = 0;
    if (const int rc = jl_hypermut_filter(p.data(), n_reads, opt.hypermut_alpha, idx.data(), &kept, &info.flagged)) return device("hypermutation filter", nullptr, rc);
    if (!opt.hypermut_report.empty()) {
        std::string text;
        char num[40];
        for (uint64_t i = 0; i < n_reads; ++i) {
            text += names[(size_t)i];
            for (uint32_t k = 0; k < JL_HM_COUNTERS; ++k) text += "\t" + std::to_string(counts[(size_t)(k * n_reads + i)]);
            snprintf(num, sizeof num, "\t%.17g\n", p[(size_t)i]);
            text += num;
        }
        std::ofstream f(opt.hypermut_report, std::ios::binary);
        f << text;
        f.close();
        if (!f) {
            st.outcome = Outcome::input, st.what = "cannot write " + opt.hypermut_report + " for the reads";
            return st;
        }
    }
    if (!opt.drop_hypermutated) return st;
    info.kept = kept;
    if (kept == 0) {
        st.outcome = Outcome::input;
        st.what = "the hypermutation filter keeps none of " + std::to_string(n_reads) + " reads (p below " + std::to_string(opt.hypermut_alpha) + " in every one)";
        return st;
    }
    if (kept == n_reads) return st;
    const jl_take_part part = {ctx, idx.data(), kept};
    if (const int rc = jl_msa_take(taken, &part, 1)) return device("take of the hypermutation filter", taken, rc);
    std::vector<std::string> chosen((size_t)kept);
    for (uint64_t j = 0; j < kept; ++j) chosen[(size_t)j].swap(names[idx[(size_t)j]]);
    names.swap(chosen);
    n_reads = kept;
    *acted = true;
    return st;
}

// What the reading-frame filter did to a sample (docs/SPEC.md §27): the `orf_integrity` block of the JSON's input section, present
// when --drop-defective or --orf-report was given.
struct OrfInfo {
    bool ran = false;
    bool reference = false;      // the row whose stops are no stops of a read: the config's referenceSequence over the window, or the majority consensus
    bool dropped = false;        // --drop-defective was given
    uint32_t kinds = 0, max_deletion = 0, tail_codons = 0;
    uint64_t reads = 0, defective = 0, kept = 0;
    struct Gene { std::string name; uint64_t partial = 0, stop = 0, frameshift = 0, deletion = 0; };
    std::vector<Gene> genes;     // reads per flag, in config order
};

// "stop,frameshift,deletion" of a mask of JL_ORF_STOP | JL_ORF_FRAMESHIFT | JL_ORF_DELETION
inline std::string orf_kinds_text(uint32_t kinds)
{
    std::string s;
    for (const auto &k : {std::make_pair((uint32_t)JL_ORF_STOP, "stop"), std::make_pair((uint32_t)JL_ORF_FRAMESHIFT, "frameshift"), std::make_pair((uint32_t)JL_ORF_DELETION, "deletion")})
        if (kinds & k.first) s += (s.empty() ? "" : ",") + std::string(k.second);
    return s;
}

// The reading-frame filter on a window that is resident on `ctx` (its reads' names in `names`) — what the read filter and the
// hypermutation filter kept, when there are any: the spans (the sample's genes as the pileup maps their codons to window columns,
// docs/SPEC.md §3), the reference row (`ref`: an earlier filter's, when one ran; else chosen as the read filter chooses), the
// per-read counters (jl_read_orf_async), the flags (jl_orf_classify), --orf-report, the rule (jl_orf_filter) and — when it drops a
// read — the kept reads gathered into `taken`, a second context of the device on the same stream; names / n_reads follow the
// indices.  *acted: the window to run is `taken` now.  An input failure: more than 64 genes, a gene without a codon in the window,
// no read kept, or a report that cannot be written.
Status orf_window(const Options &opt, const SampleSetup &smp, jl_ctx *ctx, jl_ctx *taken, const std::vector<uint8_t> *ref_row, bool ref_is_reference,
                  std::vector<std::string> &names, uint64_t &n_reads, OrfInfo &info, bool *acted)
{
    Status st;
    *acted = false;
    auto device = [&](const char *what, jl_ctx *c, int rc) {
        st.outcome = Outcome::device, st.what = what, st.ctx = c, st.rc = rc;
        return st;
    };
    auto input = [&](const std::string &what) {
        st.outcome = Outcome::input, st.what = what;
        return st;
    };
    const std::vector<GeneCfg> &genes = smp.cfg.genes;
    if (genes.size() > (size_t)JL_ORF_MAX_SPANS) return input("the reading-frame filter takes at most " + std::to_string((int)JL_ORF_MAX_SPANS) + " genes, the config has " + std::to_string(genes.size()));
    std::vector<jl_orf_span> spans;
    for (const GeneCfg &g : genes) {   // codon k of the gene: window column begin - 1 + 3 k - win_begin, evaluated while c + 2 < n_cols
        const uint64_t col = (uint64_t)g.begin_eff - 1u - smp.win_begin;
        const uint64_t fit = col + 3u <= smp.n_cols ? (smp.n_cols - col) / 3u : 0u;
        const uint64_t n = std::min<uint64_t>((g.end_eff - g.begin_eff) / 3u, fit);
        if (n == 0) return input("gene '" + g.name + "' has no codon in the window: nothing for the reading-frame filter to read");
        spans.push_back({(uint32_t)col, (uint32_t)n});
    }
    const uint32_t n_spans = (uint32_t)spans.size();
    std::vector<uint8_t> own;
    if (ref_row && !ref_row->empty()) info.reference = ref_is_reference;
    else {
        const char *what = "";
        if (const int rc = window_compare_row(smp, ctx, own, &info.reference, &what)) return device(what, ctx, rc);
        ref_row = &own;
    }
    const size_t per_kind = (size_t)n_spans * n_reads;
    std::vector<uint32_t> counts((size_t)JL_ORF_COUNTERS * per_kind), first(per_kind);
    std::vector<uint8_t> flags(per_kind);
    if (const int rc = jl_read_orf_async(ctx, spans.data(), n_spans, ref_row->data())) return device("reading-frame counters", ctx, rc);
    if (const int rc = jl_read_orf_fetch(ctx, counts.data(), first.data())) return device("reading-frame counters fetch", ctx, rc);
    const jl_orf_rule rule = {opt.defect_max_deletion, opt.defect_tail_codons};
    if (const int rc = jl_orf_classify(counts.data(), first.data(), spans.data(), n_spans, n_reads, &rule, flags.data())) return device("reading-frame flags", nullptr, rc);
    info.ran = true;
    info.dropped = opt.drop_defective;
    info.kinds = opt.defect_kinds, info.max_deletion = opt.defect_max_deletion, info.tail_codons = opt.defect_tail_codons;
    info.reads = info.kept = n_reads;
    info.genes.clear();
    for (uint32_t g = 0; g < n_spans; ++g) {
        OrfInfo::Gene gi;
        gi.name = genes[g].name;
        for (uint64_t i = 0; i < n_reads; ++i) {
            const uint8_t f = flags[(size_t)(g * n_reads + i)];
            gi.partial += (f & JL_ORF_PARTIAL) != 0, gi.stop += (f & JL_ORF_STOP) != 0;
            gi.frameshift += (f & JL_ORF_FRAMESHIFT) != 0, gi.deletion += (f & JL_ORF_DELETION) != 0;
        }
        info.genes.push_back(std::move(gi));
    }
    std::vector<uint32_t> idx((size_t)n_reads);
    uint64_t kept = 0;
    if (const int rc = jl_orf_filter(flags.data(), n_spans, n_reads, opt.defect_kinds, idx.data(), &kept, &info.defective)) return device("reading-frame filter", nullptr, rc);
    if (!opt.orf_report.empty()) {
        std::string text;
        for (uint64_t i = 0; i < n_reads; ++i)
            for (uint32_t g = 0; g < n_spans; ++g) {
                const size_t e = (size_t)(g * n_reads + i);
                text += names[(size_t)i] + "\t" + genes[g].name;
                for (uint32_t k = 0; k < JL_ORF_COUNTERS; ++k) text += "\t" + std::to_string(counts[k * per_kind + e]);
                text += "\t" + (first[e] == JL_ORF_NO_STOP ? std::string("-") : std::to_string((uint64_t)genes[g].first_codon + first[e] + 1u)) + "\t";
                std::string letters;
                for (const auto &b : {std::make_pair((int)JL_ORF_PARTIAL, 'P'), std::make_pair((int)JL_ORF_STOP, 'S'), std::make_pair((int)JL_ORF_FRAMESHIFT, 'F'), std::make_pair((int)JL_ORF_DELETION, 'D')})
                    if (flags[e] & b.first) letters += b.second;
                text += (letters.empty() ? "-" : letters) + "\n";
            }
        std::ofstream f(opt.orf_report, std::ios::binary);
        f << text;
        f.close();
        if (!f) return input("cannot write " + opt.orf_report + " for the reads");
    }
    if (!opt.drop_defective) {
        info.kept = n_reads;
        return st;
    }
    info.kept = kept;
    if (kept == 0) return input("the reading-frame filter keeps none of " + std::to_string(n_reads) + " reads (" + orf_kinds_text(opt.defect_kinds) + " in every one)");
    if (kept == n_reads) return st;
    const jl_take_part part = {ctx, idx.data(), kept};
    if (const int rc = jl_msa_take(taken, &part, 1)) return device("take of the reading-frame filter", taken, rc);
    std::vector<std::string> chosen((size_t)kept);
    for (uint64_t j = 0; j < kept; ++j) chosen[(size_t)j].swap(names[idx[(size_t)j]]);
    names.swap(chosen);
    n_reads = kept;
    *acted = true;
    return st;
}

// the row an earlier filter of the sample used, for the reading-frame filter: the read filter's, else the hypermutation filter's, else none
inline const std::vector<uint8_t> *earlier_row(const ReadFilterInfo &rf, const HypermutInfo &hm, bool *reference)
{
    if (rf.ran) { *reference = rf.reference; return &rf.compare; }
    if (hm.ran) { *reference = hm.reference; return &hm.ref; }
    *reference = false;
    return nullptr;
}

// --mix: the mixture of doc/MIXDATA.md in `taken`.  `major` holds the positional BAM's window; every BAM of the list is decoded and
// ingested into a context of its own over the same window (same device and stream), jl_mix_counts says how many reads each source
// gives, source m is sampled with seed S + m, and ONE jl_msa_take with the parts in argument order builds the mixture; names and
// n_reads become the mixture's.  0, or the process's exit status (message printed): 2 an input error, 3 a device error.
int mix_window(const Options &opt, const IngestOptions &io, jl_ctx *major, jl_ctx *taken, uint32_t n_cols, uint32_t win_begin,
               std::vector<std::string> &names, uint64_t &n_reads, SamplingInfo &info)
{
    const size_t n_src = opt.mix.size() + 1;
    std::vector<jl_ctx *> ctxs(1, major);
    std::vector<std::vector<std::string>> src_names(n_src);
    std::vector<uint64_t> reads(1, n_reads);
    src_names[0].swap(names);
    for (const std::string &file : opt.mix) {
        jl_ctx *c = nullptr;
        if (jl_ctx_create(opt.device, jl_ctx_stream(major), &c) != JL_OK) die_jl(nullptr, "context of a minor clone");
        SampleLoad load = load_sample(file, io, {ctx_ready(c)}, opt, quiet_tick);
        if (const int code = exit_code_of(load, file)) return code;
        if (const int code = exit_code_of(ingest_window(c, n_cols, win_begin, opt), file)) return code;
        src_names[ctxs.size()].swap(load.names);
        ctxs.push_back(c);
        reads.push_back(load.n_reads);
    }
    std::vector<uint64_t> counts(n_src);
    if (jl_mix_counts((uint32_t)n_src, opt.downsample, opt.mix_perc, counts.data()) != JL_OK) die_jl(nullptr, "mixture counts");
    for (size_t m = 0; m < n_src; ++m)
        if (reads[m] < counts[m]) {
            std::cerr << "juliet: --mix: " << (m ? opt.mix[m - 1] : opt.bam) << " has " << reads[m] << " reads, the mixture wants " << counts[m] << " of it\n";
            return 2;
        }
    std::vector<std::vector<uint32_t>> idx(n_src);
    std::vector<jl_take_part> parts(n_src);
    info.acted = true;
    info.seed = opt.sample_seed;
    info.sources.clear();
    for (size_t m = 0; m < n_src; ++m) {
        idx[m].resize((size_t)std::max<uint64_t>(counts[m], 1));
        uint64_t kept = 0;
        if (jl_sample_reads(reads[m], counts[m], opt.sample_seed + m, idx[m].data(), &kept) != JL_OK || kept != counts[m]) die_jl(nullptr, "sample of a clone");
        parts[m] = {ctxs[m], idx[m].data(), kept};
        info.sources.push_back({m ? opt.mix[m - 1] : opt.bam, reads[m], kept});
        for (uint64_t j = 0; j < kept; ++j) names.push_back(std::move(src_names[m][idx[m][(size_t)j]]));
    }
    if (jl_msa_take(taken, parts.data(), (uint32_t)n_src) != JL_OK) die_jl(taken, "mixture");
    n_reads = names.size();
    return 0;
}

// What --control loaded: the `control` block of the JSON's input section.
struct ControlInfo {
    bool used = false;
    std::string file;
    uint64_t reads = 0;   // of the control's window as it was counted: after --min-rq and the read filter
};

// --control: the control's BAM through the one loading path, into a context of its own on the device and stream of `sample`, over
// the sample's window, with the sample's read filter (and no --read-stats file of its own).  *control_out: the context that holds
// the control's window.  0, or the process's exit status (message printed): 2 an input error; a device error ends the process (3).
int control_window(const Options &opt, const IngestOptions &io, const SampleSetup &smp, jl_ctx *sample, jl_ctx **control_out, ControlInfo &info)
{
    jl_ctx *c = nullptr;
    if (jl_ctx_create(opt.device, jl_ctx_stream(sample), &c) != JL_OK) die_jl(nullptr, "context of the control");
    SampleLoad load = load_sample(opt.control, io, {ctx_ready(c)}, opt, quiet_tick);
    if (const int code = exit_code_of(load, opt.control)) return code;
    if (const int code = exit_code_of(ingest_window(c, smp.n_cols, smp.win_begin, opt), opt.control)) return code;
    uint64_t n_reads = load.n_reads;
    if (opt.read_filter()) {
        Options rules = opt;
        rules.read_stats_out.clear();
        jl_ctx *kept = nullptr;
        if (jl_ctx_create(opt.device, jl_ctx_stream(sample), &kept) != JL_OK) die_jl(nullptr, "context of the control's kept reads");
        ReadFilterInfo rf;
        bool acted = false;
        if (const int code = exit_code_of(read_filter_window(rules, smp, c, kept, load.names, n_reads, rf, &acted), opt.control)) return code;
        if (acted) c = kept;
    }
    if (opt.drop_hypermutated) {   // (and the sample's hypermutation filter, on a reference row of the control's own choosing)
        Options rules = opt;
        rules.hypermut_report.clear();
        jl_ctx *kept = nullptr;
        if (jl_ctx_create(opt.device, jl_ctx_stream(sample), &kept) != JL_OK) die_jl(nullptr, "context of the control's kept reads");
        HypermutInfo hm;
        bool acted = false;
        if (const int code = exit_code_of(hypermut_window(rules, smp, c, kept, nullptr, load.names, n_reads, hm, &acted), opt.control)) return code;
        if (acted) c = kept;
    }
    if (opt.drop_defective) {   // (and the sample's reading-frame filter, on a reference row of the control's own choosing)
        Options rules = opt;
        rules.orf_report.clear();
        jl_ctx *kept = nullptr;
        if (jl_ctx_create(opt.device, jl_ctx_stream(sample), &kept) != JL_OK) die_jl(nullptr, "context of the control's kept reads");
        OrfInfo oi;
        bool acted = false;
        if (const int code = exit_code_of(orf_window(rules, smp, c, kept, nullptr, false, load.names, n_reads, oi, &acted), opt.control)) return code;
        if (acted) c = kept;
    }
    info.used = true;
    info.file = opt.control;
    info.reads = n_reads;
    *control_out = c;
    return 0;
}

// --control, in the place of the run: the pileups of both windows, the control call (docs/SPEC.md §21), its table and the sample's
// column counts, and with `phasing` the phasing of that table.  nullptr, or the step that failed (*failed: the context to ask).
const char *run_control_calls(jl_ctx *ctx, jl_ctx *control, const SampleSetup &smp, const uint64_t *drm_masks, bool phasing, uint32_t min_reads,
                              Results &R, const Tick &tick, jl_ctx **failed)
{
    *failed = control;
    if (jl_pileup_async(control, smp.genes.data(), (uint32_t)smp.genes.size(), smp.refp(), (uint32_t)smp.refcodes.size()) != JL_OK) return "pileup of the control";
    *failed = ctx;
    if (jl_pileup_async(ctx, smp.genes.data(), (uint32_t)smp.genes.size(), smp.refp(), (uint32_t)smp.refcodes.size()) != JL_OK) return "pileup";
    if (jl_control_call_async(ctx, control, &smp.prm, drm_masks) != JL_OK) return "control call";
    tick("plan + enqueue");
    R.controlled = true;
    R.var.resize(4096);
    R.control_cov.resize(4096);
    uint32_t nv = 0;
    if (jl_control_call_fetch(ctx, R.var.data(), R.control_cov.data(), 4096, &nv) != JL_OK) return "control call fetch";
    R.var.resize(nv);
    R.control_cov.resize(nv);
    tick("  wait for the calls + table");
    if (jl_pileup_fetch(ctx, R.col_counts.data(), nullptr, nullptr, nullptr, nullptr, nullptr) != JL_OK) return "pileup fetch";
    tick("  column counts");
    if (phasing && jl_phase_async(ctx, R.var.data(), nv, min_reads) != JL_OK) return "phasing of the control-called table";
    return nullptr;
}

}  // namespace
}  // namespace jlhost
