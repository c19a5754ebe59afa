// report.hpp — what a run writes: the JSON document of one sample (build_json; the HTML output is its rendering, html.hpp),
// every output file closed and checked (write_outputs), the --haplotype-fasta records and the consensus FASTA of --consensus / fuse.
#pragma once
#include <chrono>
#include <ctime>
#include <fstream>
#include <map>

#include "fuse.hpp"
#include "html.hpp"
#include "sample.hpp"

namespace jlhost {
namespace {

std::string iso_now()
{
    using namespace std::chrono;
    const auto now = system_clock::now();
    const std::time_t t = system_clock::to_time_t(now);
    const int ms = (int)(duration_cast<milliseconds>(now.time_since_epoch()).count() % 1000);
    std::tm tm;
    gmtime_r(&t, &tm);
    char buf[80];
    snprintf(buf, sizeof buf, "%04d-%02d-%02dT%02d:%02d:%02d.%03dZ", tm.tm_year + 1900, tm.tm_mon + 1, tm.tm_mday,
             tm.tm_hour, tm.tm_min, tm.tm_sec, ms);
    return buf;
}

std::string haplotype_name(uint32_t h)  // [A-Z]{1}[a-z]?  (doc/JULIET.md:198)
{
    if (h < 26) return std::string(1, (char)('A' + h));
    h -= 26;
    return std::string{(char)('A' + h / 26), (char)('a' + h % 26)};
}

// The JSON document of one sample (doc/JULIET.md:61-107, 207-211); the HTML output is its rendering.
Json build_json(const Options &opt, const SampleSetup &s, const std::string &bam, const std::string &cmdline,
                const std::vector<std::string> &names, uint64_t n_reads, const Results &R, const SamplingInfo *sampling = nullptr,
                const ReadFilterInfo *read_filter = nullptr, const ControlInfo *control = nullptr, const HypermutInfo *hypermut = nullptr,
                const OrfInfo *orf = nullptr)
{
    const TargetConfig &cfg = s.cfg;
    const uint32_t win_begin = s.win_begin, n_cols = s.n_cols;
    const std::string &chem = s.chem;
    const std::vector<jl_variant> &var = R.var;
    const std::vector<uint32_t> &col_counts = R.col_counts;
    const jl_phase_summary &ps = R.ps;
    const std::vector<uint32_t> &pos_cols = R.pos_cols, &hap_count = R.hap_count;
    const std::vector<uint8_t> &hap_pattern = R.hap_pattern, &hit = R.hit;
    const std::vector<uint16_t> &read_hap = R.read_hap;

    Json root = Json::object();
    root.set("input", Json::object()
                          .set("timestamp", Json::of(iso_now()))
                          .set("input_file", Json::of(bam))
                          .set("command_line", Json::of(cmdline))
                          .set("juliet_version", Json::of(kVersion)));
    if (sampling && sampling->acted) {   // (only then: a run whose flags chose nothing writes what a run without them writes)
        Json srcs = Json::array();
        for (const SamplingInfo::Source &x : sampling->sources)
            srcs.push(Json::object().set("file", Json::of(x.file)).set("reads", Json::of((int64_t)x.reads)).set("kept", Json::of((int64_t)x.kept)));
        Json sj = Json::object();
        sj.set("seed", Json::of((int64_t)sampling->seed)).set("sources", std::move(srcs));
        root.obj.back().second.set("sampling", std::move(sj));
    }
    if (read_filter && read_filter->ran) {   // (only with a rule or --read-stats: docs/SPEC.md section 20)
        static const char *rules[5] = {"min_bases", "mismatches", "mismatch_perc", "gap_perc", "n_perc"};
        const double given[5] = {(double)opt.read_rule.min_bases, (double)opt.read_rule.max_mismatches, opt.read_rule.max_mismatch_perc,
                                 opt.read_rule.max_gap_perc, opt.read_rule.max_masked_perc};
        Json rule = Json::object(), failed = Json::object();
        for (uint32_t r = 0; r < 5; ++r) {
            if (opt.read_rule_set >> r & 1u) rule.set(rules[r], Json::of(given[r]));
            failed.set(rules[r], Json::of((int64_t)read_filter->failed[r]));
        }
        Json rf = Json::object();
        rf.set("compare", Json::of(std::string(read_filter->reference ? "reference" : "majority"))).set("rule", std::move(rule));
        rf.set("reads", Json::of((int64_t)read_filter->reads)).set("kept", Json::of((int64_t)read_filter->kept)).set("failed", std::move(failed));
        root.obj.back().second.set("read_filter", std::move(rf));
    }
    if (hypermut && hypermut->ran) {   // (only with --drop-hypermutated or --hypermut-report: docs/SPEC.md section 26)
        Json hj = Json::object();
        hj.set("reference", Json::of(std::string(hypermut->reference ? "reference" : "majority"))).set("alpha", Json::of(hypermut->alpha));
        hj.set("reads", Json::of((int64_t)hypermut->reads)).set("flagged", Json::of((int64_t)hypermut->flagged)).set("kept", Json::of((int64_t)hypermut->kept));
        hj.set("dropped", Json::of(hypermut->dropped));
        root.obj.back().second.set("hypermutation", std::move(hj));
    }
    if (orf && orf->ran) {   // (only with --drop-defective or --orf-report: docs/SPEC.md section 27)
        Json oj = Json::object();
        oj.set("reference", Json::of(std::string(orf->reference ? "reference" : "majority"))).set("kinds", Json::of(orf_kinds_text(orf->kinds)));
        oj.set("max_deletion", Json::of((int64_t)orf->max_deletion)).set("tail_codons", Json::of((int64_t)orf->tail_codons));
        oj.set("reads", Json::of((int64_t)orf->reads)).set("defective", Json::of((int64_t)orf->defective)).set("kept", Json::of((int64_t)orf->kept));
        oj.set("dropped", Json::of(orf->dropped));
        Json genes = Json::array();
        for (const OrfInfo::Gene &g : orf->genes)
            genes.push(Json::object().set("name", Json::of(g.name)).set("partial", Json::of((int64_t)g.partial)).set("stop", Json::of((int64_t)g.stop))
                           .set("frameshift", Json::of((int64_t)g.frameshift)).set("deletion", Json::of((int64_t)g.deletion)));
        oj.set("genes", std::move(genes));
        root.obj.back().second.set("orf_integrity", std::move(oj));
    }
    if (control && control->used)   // (only with --control: docs/SPEC.md section 21)
        root.obj.back().second.set("control", Json::object().set("file", Json::of(control->file)).set("reads", Json::of((int64_t)control->reads)));
    Json tc = cfg.echo();
    tc.set("n_reads", Json::of((int64_t)n_reads));
    tc.set("window_begin", Json::of(win_begin + 1)).set("window_end", Json::of(win_begin + n_cols + 1));
    tc.set("chemistry_model", Json::of(chem));
    root.set("target_config", tc);

    Json genes_json = Json::array();
    const uint32_t H = ps.n_haplotypes;
    for (size_t g = 0; g < cfg.genes.size(); ++g) {
        Json gj = Json::object();
        gj.set("name", Json::of(cfg.genes[g].name));
        Json vps = Json::array();
        size_t v = 0;
        while (v < var.size()) {
            if (var[v].gene != g) { ++v; continue; }
            size_t e = v;
            while (e < var.size() && var[e].gene == g && var[e].codon_pos == var[v].codon_pos) ++e;
            const jl_variant &f = var[v];
            Json vp = Json::object();
            vp.set("ref_codon", Json::of(codon_string(f.ref_codon)));
            vp.set("ref_amino_acid", Json::of(std::string(1, translate(f.ref_codon))));
            const uint32_t aa_pos = f.codon_pos + cfg.genes[g].first_codon;
            vp.set("ref_position", Json::of(aa_pos));
            vp.set("coverage", Json::of(f.coverage));
            // variant codons grouped by amino acid (position 223 with two rows)
            Json aas = Json::array();
            std::vector<char> order;
            for (size_t k = v; k < e; ++k) {
                const char aa = translate(var[k].codon);
                if (std::find(order.begin(), order.end(), aa) == order.end()) order.push_back(aa);
            }
            // amino acids in alphabetical order: juliet_abl-nohaplotype.png prints "A GCC" above "P CCA" at ABL1 223
            std::sort(order.begin(), order.end());
            for (char aa : order) {
                Json aj = Json::object();
                aj.set("amino_acid", Json::of(std::string(1, aa)));
                Json cods = Json::array();
                for (size_t k = v; k < e; ++k) {
                    if (translate(var[k].codon) != aa) continue;
                    Json cj = Json::object();
                    cj.set("codon", Json::of(codon_string(var[k].codon)));
                    cj.set("frequency", Json::of((double)var[k].count / (double)var[k].coverage));
                    cj.set("count", Json::of(var[k].count));
                    cj.set("expected", Json::of(var[k].expected));
                    if (R.controlled) {   // §21: the table's second row is the control's
                        cj.set("control_count", Json::of(var[k].expected)).set("control_coverage", Json::of(R.control_cov[k]));
                        cj.set("control_frequency", Json::of((double)var[k].expected / (double)R.control_cov[k]));
                    }
                    cj.set("pValue", Json::of(var[k].p_value));
                    cj.set("log_pValue", Json::of(var[k].log_p));
                    cj.set("known_drm", Json::of(cfg.known_drms(g, aa_pos, aa)));
                    if (opt.phasing) {
                        Json hh = Json::array();
                        const size_t row = R.sites_phased && !R.sites.empty() ? R.var_row[k] : k;   // (§18: the row of the site matrix's table)
                        for (uint32_t h = 0; h < H; ++h) hh.push(Json::of(hit[row * R.hit_stride + h] != 0));
                        cj.set("haplotype_hit", hh);  // doc/JULIET.md:207-209
                    }
                    if (R.hap_mutations) {   // §24: the codon's count and the coverage within each reported haplotype
                        Json hc = Json::array(), hv = Json::array();
                        const int entry = R.hm_entry(var[k].col);
                        for (uint32_t h = 0; h < H && entry >= 0 && !R.hm_hist.empty(); ++h) {
                            const uint32_t *row = &R.hm_hist[((size_t)h * R.hm_cols.size() + (size_t)entry) * 64];
                            uint32_t cov = 0;
                            for (uint32_t q = 0; q < 64; ++q) cov += row[q];
                            hc.push(Json::of(row[var[k].codon]));
                            hv.push(Json::of(cov));
                        }
                        cj.set("haplotype_count", std::move(hc)).set("haplotype_coverage", std::move(hv));
                    }
                    cods.push(cj);
                }
                aj.set("variant_codons", cods);
                aas.push(aj);
            }
            vp.set("variant_amino_acids", aas);
            // MSA context: -3 .. +5 around the codon's first base (doc/JULIET.md:99-100)
            Json msa = Json::array();
            for (int rel = -3; rel <= 5; ++rel) {
                const int64_t c = (int64_t)f.col + rel;
                if (c < 0 || c >= (int64_t)n_cols) continue;
                const uint32_t *cc = &col_counts[(size_t)c * 6];
                Json mj = Json::object();
                mj.set("rel_pos", Json::of((int64_t)rel)).set("abs_pos", Json::of((int64_t)(win_begin + c + 1)));
                static const char *sym[6] = {"A", "C", "G", "T", "-", "N"};
                for (int s = 0; s < 6; ++s) mj.set(sym[s], Json::of(cc[s]));
                const size_t r = (size_t)win_begin + (size_t)c;
                if (r < cfg.reference_sequence.size()) mj.set("wt", Json::of(std::string(1, (char)std::toupper((unsigned char)cfg.reference_sequence[r]))));
                msa.push(mj);
            }
            vp.set("msa", msa);
            vps.push(vp);
            v = e;
        }
        gj.set("variant_positions", vps);
        if (R.deletions) {   // --call-deletions (docs/SPEC.md §16): the called positions of this gene, ascending
            Json dps = Json::array();
            for (const Results::Deletion &d : R.del_rows) {
                if (d.gene != g) continue;
                Json dj = Json::object();
                dj.set("ref_position", Json::of(d.codon_pos + cfg.genes[g].first_codon));
                if (d.ref_codon >= 0) {
                    dj.set("ref_codon", Json::of(codon_string((uint8_t)d.ref_codon)));
                    dj.set("ref_amino_acid", Json::of(std::string(1, translate((uint8_t)d.ref_codon))));
                }
                dj.set("count", Json::of(d.call.count)).set("coverage", Json::of(d.call.coverage));
                dj.set("frequency", Json::of((double)d.call.count / (double)d.call.coverage));
                dj.set("expected", Json::of(d.call.expected));
                dj.set("pValue", Json::of(d.call.p_value)).set("log_pValue", Json::of(d.call.log_p));
                dj.set("frameshift_reads", Json::of(d.call.partial));
                if (R.dels_phased) {   // --phase-deletions (docs/SPEC.md §18): the haplotypes that have this codon deleted
                    const int site = R.deletion_site(d.col);
                    Json hh = Json::array();
                    for (uint32_t h = 0; h < H; ++h) hh.push(Json::of(site >= 0 && hap_pattern[(size_t)h * R.pat_stride + (size_t)site] == JL_SITE_DELETED));
                    dj.set("haplotype_hit", hh);
                }
                dps.push(dj);
            }
            gj.set("deletion_positions", dps);
        }
        if (R.insertions) {   // --call-insertions (docs/SPEC.md §17): the called alleles of this gene, by position, length, sequence
            Json ips = Json::array();
            for (const Results::Insertion &in : R.ins_rows) {
                if (in.gene != g) continue;
                Json ij = Json::object();
                ij.set("after_position", Json::of(in.codon_pos + cfg.genes[g].first_codon - 1));
                Json cods = Json::array();
                std::string aas;
                for (uint32_t k = 0; k + 3 <= in.allele.len; k += 3) {
                    const uint8_t codon = (uint8_t)(16u * ((in.allele.seq >> (2u * k)) & 3u) + 4u * ((in.allele.seq >> (2u * k + 2u)) & 3u) +
                                                    ((in.allele.seq >> (2u * k + 4u)) & 3u));
                    cods.push(Json::of(codon_string(codon)));
                    aas += translate(codon);
                }
                ij.set("inserted_codons", cods).set("inserted_amino_acids", Json::of(aas));
                ij.set("count", Json::of(in.call.count)).set("coverage", Json::of(in.call.coverage));
                ij.set("frequency", Json::of((double)in.call.count / (double)in.call.coverage));
                ij.set("expected", Json::of(in.call.expected));
                ij.set("pValue", Json::of(in.call.p_value)).set("log_pValue", Json::of(in.call.log_p));
                ij.set("frameshift_reads", Json::of(in.call.frameshift)).set("unread_reads", Json::of(in.call.unread));
                if (R.ins_phased) {   // --phase-insertions (docs/SPEC.md §19): the haplotypes that carry this allele
                    const int a = R.site_allele_of(in.allele);
                    Json hh = Json::array();
                    for (uint32_t h = 0; h < H; ++h)
                        hh.push(Json::of(a >= 0 && hap_pattern[(size_t)h * R.pat_stride + R.site_alleles[(size_t)a].site] == R.site_alleles[(size_t)a].code));
                    ij.set("haplotype_hit", hh);
                }
                ips.push(ij);
            }
            gj.set("insertion_positions", ips);
        }
        genes_json.push(gj);
    }
    root.set("genes", genes_json);

    // Section 4, drug summaries: variants grouped by annotated drug (doc/JULIET.md:104-107)
    {
        std::vector<std::pair<std::string, Json>> by_drug;
        for (const jl_variant &f : var) {
            const GeneCfg &g = cfg.genes[f.gene];
            const uint32_t aa_pos = f.codon_pos + g.first_codon;
            const char aa = translate(f.codon);
            for (const Drm &d : g.drms) {
                bool hit_drm = false;
                for (const DrmPosition &dp : d.positions) hit_drm = hit_drm || dp.matches(aa_pos, aa);
                if (!hit_drm) continue;
                Json e = Json::object();
                e.set("gene", Json::of(g.name));
                e.set("mutation", Json::of(std::string(1, translate(f.ref_codon)) + std::to_string(aa_pos) + std::string(1, aa)));
                e.set("codon", Json::of(codon_string(f.codon)));
                e.set("frequency", Json::of((double)f.count / (double)f.coverage));
                auto it = std::find_if(by_drug.begin(), by_drug.end(), [&](const std::pair<std::string, Json> &kv) { return kv.first == d.name; });
                if (it == by_drug.end()) { by_drug.emplace_back(d.name, Json::array()); it = by_drug.end() - 1; }
                it->second.push(e);
            }
        }
        Json ds = Json::array();
        for (auto &kv : by_drug) ds.push(Json::object().set("drug", Json::of(kv.first)).set("variants", kv.second));
        root.set("drug_summaries", ds);
    }

    if (opt.phasing) {  // root `haplotype` block: counts and read names, same order as haplotype_hit (doc/JULIET.md:209-211)
        Json hb = Json::object();
        hb.set("reported_reads", Json::of(ps.reported_reads)).set("insufficient_coverage_reads", Json::of(ps.insufficient_reads));
        hb.set("damaged_reads", Json::of(ps.damaged_reads)).set("marginal_gaps", Json::of(ps.marginal_gap));
        hb.set("marginal_heteroduplexes", Json::of(ps.marginal_heteroduplex)).set("marginal_partial", Json::of(ps.marginal_partial));
        std::vector<std::vector<uint32_t>> members(H);
        for (uint64_t i = 0; i < n_reads; ++i)
            if (read_hap[i] < H) members[read_hap[i]].push_back((uint32_t)i);
        // --rescue-damaged: the damaged reads by what the rule of docs/SPEC.md §14 says of them
        std::vector<std::vector<uint32_t>> rescued_members(H);
        uint64_t rescue_cat[4] = {0, 0, 0, 0};   // assigned, ambiguous, incompatible, uninformative
        uint64_t with_rescued_total = 0;
        if (R.rescued && ps.n_positions) {   // (no variant position: nothing was phased, no read is damaged, §8)
            for (uint64_t i = 0; i < n_reads; ++i) {
                if (read_hap[i] != (uint16_t)JL_HAP_DAMAGED) continue;
                const uint32_t r = R.rescue.empty() ? (uint32_t)JL_RESCUE_UNINFORMATIVE : R.rescue[i];
                if (r < H) rescued_members[r].push_back((uint32_t)i), rescue_cat[0]++;
                else rescue_cat[r == (uint32_t)JL_RESCUE_AMBIGUOUS ? 1 : r == (uint32_t)JL_RESCUE_NONE ? 2 : 3]++;
            }
            for (uint32_t h = 0; h < H; ++h) with_rescued_total += (uint64_t)hap_count[h] + rescued_members[h].size();
        }
        // --absorb-distance: the insufficient and the damaged reads by what the rule of docs/SPEC.md §22 says of them
        std::vector<std::vector<uint32_t>> absorbed_members(H);   // both kinds, in read order
        std::vector<uint32_t> absorbed_insufficient(H, 0u), absorbed_damaged(H, 0u);
        uint64_t absorb_cat[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};   // [insufficient, damaged][assigned, ambiguous, distant, uninformative]
        std::vector<uint64_t> absorb_by_distance[2];
        uint64_t with_absorbed_total = 0;
        if (R.absorbed) {
            for (auto &v : absorb_by_distance) v.assign(R.absorb_distance + 1u, 0);
            if (ps.n_positions)   // (no variant position: nothing was phased, no read is insufficient or damaged, §8)
                for (uint64_t i = 0; i < n_reads; ++i) {
                    if (read_hap[i] != (uint16_t)JL_HAP_INSUFFICIENT && read_hap[i] != (uint16_t)JL_HAP_DAMAGED) continue;
                    const uint32_t kind = read_hap[i] == (uint16_t)JL_HAP_DAMAGED ? 1u : 0u;
                    const uint32_t r = R.nearest.empty() ? (uint32_t)JL_RESCUE_UNINFORMATIVE : R.nearest[i];
                    if (r < H) {
                        absorbed_members[r].push_back((uint32_t)i);
                        (kind ? absorbed_damaged : absorbed_insufficient)[r]++;
                        absorb_cat[kind][0]++;
                        absorb_by_distance[kind][R.nearest_dist[i]]++;
                    } else
                        absorb_cat[kind][r == (uint32_t)JL_RESCUE_AMBIGUOUS ? 1 : r == (uint32_t)JL_RESCUE_NONE ? 2 : 3]++;
                }
            for (uint32_t h = 0; h < H; ++h) with_absorbed_total += (uint64_t)hap_count[h] + absorbed_members[h].size();
        }
        // --flag-recombinants: the insufficient and the damaged reads by what the rule of docs/SPEC.md §23 says of them, and the
        // (left, right) pairs of those with both parents unique
        struct RecombPair { uint32_t left, right, reads[2], bp_min, bp_max; };
        uint64_t recomb_cat[2][5] = {{0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}};   // [insufficient, damaged][recombinant, ambiguous parent, whole, unexplained, uninformative]
        std::vector<RecombPair> recomb_pairs;
        if (R.recomb && ps.n_positions) {   // (no variant position: nothing was phased, no read is insufficient or damaged, §8)
            std::map<std::pair<uint32_t, uint32_t>, size_t> at;
            for (uint64_t i = 0; i < n_reads; ++i) {
                if (read_hap[i] != (uint16_t)JL_HAP_INSUFFICIENT && read_hap[i] != (uint16_t)JL_HAP_DAMAGED) continue;
                const uint32_t kind = read_hap[i] == (uint16_t)JL_HAP_DAMAGED ? 1u : 0u;
                const uint32_t l = R.recomb_left.empty() ? (uint32_t)JL_RESCUE_UNINFORMATIVE : R.recomb_left[i];
                const uint32_t r = R.recomb_left.empty() ? (uint32_t)JL_RESCUE_UNINFORMATIVE : R.recomb_right[i];
                if (l < H && r < H) {
                    recomb_cat[kind][0]++;
                    const uint32_t lo = ps.n_positions - R.recomb_suffix[i], hi = R.recomb_prefix[i];
                    auto it = at.find({l, r});
                    if (it == at.end()) {
                        it = at.emplace(std::make_pair(l, r), recomb_pairs.size()).first;
                        recomb_pairs.push_back({l, r, {0u, 0u}, lo, hi});
                    }
                    RecombPair &pr = recomb_pairs[it->second];
                    pr.reads[kind]++;
                    pr.bp_min = std::min(pr.bp_min, lo), pr.bp_max = std::max(pr.bp_max, hi);
                } else
                    recomb_cat[kind][l == (uint32_t)JL_RECOMB_WHOLE ? 2 : l == (uint32_t)JL_RESCUE_NONE ? 3 : l == (uint32_t)JL_RESCUE_UNINFORMATIVE ? 4 : 1]++;
            }
            std::sort(recomb_pairs.begin(), recomb_pairs.end(), [](const RecombPair &a, const RecombPair &b) {
                const uint32_t ra = a.reads[0] + a.reads[1], rb = b.reads[0] + b.reads[1];
                return ra != rb ? ra > rb : a.left != b.left ? a.left < b.left : a.right < b.right;
            });
        }
        // --phase-deletions / --phase-insertions with at least one site (docs/SPEC.md §18, §19): position p of the run is site p
        const bool with_sites = R.sites_phased && !R.sites.empty();
        Json hs = Json::array();
        std::vector<std::vector<std::string>> hap_drugs(H);   // --haplotype-mutations (docs/SPEC.md §24)
        for (uint32_t h = 0; h < H; ++h) {
            Json hj = Json::object();
            Json muts = Json::array();
            if (R.hap_mutations) {   // every evaluated position whose majority codon within the haplotype is not the position's ref
                for (const Results::HapMutPos &q : R.hm_pos) {
                    if (q.ref < 0 || R.hm_hist.empty()) continue;
                    const uint32_t *row = &R.hm_hist[((size_t)h * R.hm_cols.size() + q.entry) * 64];
                    uint32_t best = 0, cov = 0;
                    for (uint32_t k = 0; k < 64; ++k) {
                        cov += row[k];
                        if (row[k] > row[best]) best = k;   // (ties: the lowest index)
                    }
                    if (cov == 0 || best == (uint32_t)q.ref) continue;
                    const GeneCfg &g = cfg.genes[q.gene];
                    const uint32_t aa_pos = q.codon_pos + g.first_codon;
                    const char aa = translate(best);
                    Json drms = Json::array();
                    for (const Drm &d : g.drms) {
                        bool hit_drm = false;
                        for (const DrmPosition &dp : d.positions) hit_drm = hit_drm || dp.matches(aa_pos, aa);
                        if (!hit_drm) continue;
                        drms.push(Json::of(d.name));
                        if (std::find(hap_drugs[h].begin(), hap_drugs[h].end(), d.name) == hap_drugs[h].end()) hap_drugs[h].push_back(d.name);
                    }
                    muts.push(Json::object()
                                  .set("gene", Json::of(g.name))
                                  .set("position", Json::of(aa_pos))
                                  .set("ref_codon", Json::of(codon_string((unsigned)q.ref)))
                                  .set("ref_amino_acid", Json::of(std::string(1, translate((unsigned)q.ref))))
                                  .set("codon", Json::of(codon_string(best)))
                                  .set("amino_acid", Json::of(std::string(1, aa)))
                                  .set("count", Json::of(row[best]))
                                  .set("coverage", Json::of(cov))
                                  .set("frequency", Json::of((double)row[best] / (double)cov))
                                  .set("drms", std::move(drms)));
                }
                std::sort(hap_drugs[h].begin(), hap_drugs[h].end());
            }
            hj.set("name", Json::of(haplotype_name(h))).set("reads", Json::of(hap_count[h]));
            hj.set("frequency", Json::of(ps.reported_reads ? (double)hap_count[h] / (double)ps.reported_reads : 0.0));
            Json cods = Json::array();
            const uint8_t *pat = &hap_pattern[(size_t)h * R.pat_stride];
            if (!with_sites)
                for (uint32_t p = 0; p < ps.n_positions; ++p) cods.push(Json::of(codon_string(pat[p])));
            else {   // the codon sites only; a codon whose companion deletion site says "deleted" prints ---
                Json dels = Json::array();
                for (size_t k = 0; k < R.sites.size(); ++k) {
                    if (R.sites[k].kind == (uint8_t)JL_SITE_INSERTION) continue;
                    if (R.sites[k].kind == (uint8_t)JL_SITE_DELETION) { dels.push(Json::of(pat[k] == JL_SITE_DELETED)); continue; }
                    const int companion = R.deletion_site(R.sites[k].col);
                    cods.push(Json::of(companion >= 0 && pat[companion] == JL_SITE_DELETED ? std::string("---") : codon_string(pat[k])));
                }
                if (R.dels_phased) hj.set("deletions", std::move(dels));
            }
            if (R.ins_phased) {   // a flag per listed allele; a pattern that is "another insertion" or none has none of its site's
                Json flags = Json::array();
                for (const Results::SiteAllele &a : R.site_alleles) flags.push(Json::of(pat[a.site] == a.code));
                hj.set("insertions", std::move(flags));
            }
            hj.set("codons", std::move(cods));
            Json rn = Json::array();      // (moved on, level by level: a copy of this list per level was most of the stage at a million reads)
            rn.arr.reserve(members[h].size());
            for (uint32_t i : members[h]) rn.push(Json::of(names[i]));
            hj.set("read_names", std::move(rn));
            if (R.rescued) {
                const uint64_t with = (uint64_t)hap_count[h] + rescued_members[h].size();
                hj.set("rescued_reads", Json::of((uint32_t)rescued_members[h].size()));
                Json rr = Json::array();
                rr.arr.reserve(rescued_members[h].size());
                for (uint32_t i : rescued_members[h]) rr.push(Json::of(names[i]));
                hj.set("rescued_read_names", std::move(rr));
                hj.set("frequency_with_rescued", Json::of(with_rescued_total ? (double)with / (double)with_rescued_total : 0.0));
            }
            if (R.absorbed) {
                const uint64_t with = (uint64_t)hap_count[h] + absorbed_members[h].size();
                hj.set("absorbed_reads", Json::of(absorbed_insufficient[h]));
                hj.set("absorbed_damaged_reads", Json::of(absorbed_damaged[h]));
                Json ar = Json::array();
                ar.arr.reserve(absorbed_members[h].size());
                for (uint32_t i : absorbed_members[h]) ar.push(Json::of(names[i]));
                hj.set("absorbed_read_names", std::move(ar));
                hj.set("frequency_with_absorbed", Json::of(with_absorbed_total ? (double)with / (double)with_absorbed_total : 0.0));
            }
            if (R.recomb) {
                const jl_hap_recombinant *hr = h < R.recomb_haps.size() ? &R.recomb_haps[h] : nullptr;
                hj.set("putative_recombinant", Json::of(hr && hr->flagged != 0u));
                if (hr && hr->flagged)
                    hj.set("recombinant_of", Json::object()
                                                 .set("left", Json::of(haplotype_name(hr->left)))
                                                 .set("right", Json::of(haplotype_name(hr->right)))
                                                 .set("prefix", Json::of(hr->prefix))
                                                 .set("suffix", Json::of(hr->suffix)));
            }
            if (R.hap_mutations) {
                Json dj = Json::array();
                for (const std::string &d : hap_drugs[h]) dj.push(Json::of(d));
                hj.set("mutations", std::move(muts)).set("drugs", std::move(dj));
            }
            hs.push(std::move(hj));
        }
        hb.set("haplotypes", std::move(hs));
        if (R.hap_mutations) {   // one entry per drug that any haplotype carries, ascending by name
            std::vector<std::string> all;
            for (const auto &v : hap_drugs) all.insert(all.end(), v.begin(), v.end());
            std::sort(all.begin(), all.end());
            all.erase(std::unique(all.begin(), all.end()), all.end());
            Json dp = Json::array();
            for (const std::string &drug : all) {
                Json flags = Json::array();
                uint64_t reads = 0;
                double freq = 0.0;
                for (uint32_t h = 0; h < H; ++h) {
                    const bool has = std::find(hap_drugs[h].begin(), hap_drugs[h].end(), drug) != hap_drugs[h].end();
                    flags.push(Json::of(has));
                    if (!has) continue;
                    reads += hap_count[h];
                    freq += ps.reported_reads ? (double)hap_count[h] / (double)ps.reported_reads : 0.0;
                }
                dp.push(Json::object().set("drug", Json::of(drug)).set("haplotypes", std::move(flags)).set("reads", Json::of((uint32_t)reads))
                            .set("frequency", Json::of(freq)));
            }
            hb.set("drug_profile", std::move(dp));
        }
        Json pc = Json::array();
        if (!with_sites)
            for (uint32_t p = 0; p < ps.n_positions; ++p) pc.push(Json::of(win_begin + pos_cols[p] + 1));
        else
            for (const jl_site &x : R.sites)
                if (x.kind == (uint8_t)JL_SITE_CODON) pc.push(Json::of(win_begin + x.col + 1));
        hb.set("variant_positions_abs", std::move(pc));
        if (R.dels_phased) {
            Json dp = Json::array();
            for (const jl_site &x : R.sites)
                if (x.kind == (uint8_t)JL_SITE_DELETION) dp.push(Json::of(win_begin + x.col + 1));
            hb.set("deletion_positions_abs", std::move(dp));
        }
        if (R.ins_phased) {   // the letters of the insertion sites: by site, then code (an allele called for two genes: under the first)
            Json ia = Json::array();
            for (const Results::SiteAllele &a : R.site_alleles) {
                const Results::Insertion &in = R.ins_rows[a.row];
                Json cods = Json::array();
                for (uint32_t k = 0; k + 3 <= in.allele.len; k += 3)
                    cods.push(Json::of(codon_string((uint8_t)(16u * ((in.allele.seq >> (2u * k)) & 3u) + 4u * ((in.allele.seq >> (2u * k + 2u)) & 3u) +
                                                              ((in.allele.seq >> (2u * k + 4u)) & 3u)))));
                ia.push(Json::object().set("gene", Json::of(cfg.genes[in.gene].name))
                            .set("after_position", Json::of(in.codon_pos + cfg.genes[in.gene].first_codon - 1)).set("inserted_codons", std::move(cods)));
            }
            hb.set("insertion_alleles", std::move(ia));
        }
        if (R.rescued)
            hb.set("rescue", Json::object()
                                 .set("min_positions", Json::of(R.rescue_min))
                                 .set("assigned_reads", Json::of((uint32_t)rescue_cat[0]))
                                 .set("ambiguous_reads", Json::of((uint32_t)rescue_cat[1]))
                                 .set("incompatible_reads", Json::of((uint32_t)rescue_cat[2]))
                                 .set("uninformative_reads", Json::of((uint32_t)rescue_cat[3])));
        if (R.absorbed) {
            Json ab = Json::object();
            ab.set("max_distance", Json::of(R.absorb_distance)).set("min_positions", Json::of(R.absorb_min));
            static const char *kinds[2] = {"insufficient", "damaged"};
            for (uint32_t kind = 0; kind < 2u; ++kind) {
                Json by = Json::array();
                for (uint64_t c : absorb_by_distance[kind]) by.push(Json::of((uint32_t)c));
                ab.set(kinds[kind], Json::object()
                                        .set("assigned_reads", Json::of((uint32_t)absorb_cat[kind][0]))
                                        .set("ambiguous_reads", Json::of((uint32_t)absorb_cat[kind][1]))
                                        .set("distant_reads", Json::of((uint32_t)absorb_cat[kind][2]))
                                        .set("uninformative_reads", Json::of((uint32_t)absorb_cat[kind][3]))
                                        .set("assigned_by_distance", std::move(by)));
            }
            hb.set("absorb", std::move(ab));
        }
        if (R.recomb) {
            Json rb = Json::object();
            rb.set("min_positions", Json::of(R.recomb_min)).set("parent_ratio", Json::of(R.recomb_ratio));
            static const char *kinds[2] = {"insufficient", "damaged"};
            for (uint32_t kind = 0; kind < 2u; ++kind)
                rb.set(kinds[kind], Json::object()
                                        .set("recombinant_reads", Json::of((uint32_t)recomb_cat[kind][0]))
                                        .set("ambiguous_parent_reads", Json::of((uint32_t)recomb_cat[kind][1]))
                                        .set("whole_reads", Json::of((uint32_t)recomb_cat[kind][2]))
                                        .set("unexplained_reads", Json::of((uint32_t)recomb_cat[kind][3]))
                                        .set("uninformative_reads", Json::of((uint32_t)recomb_cat[kind][4])));
            Json pairs = Json::array();
            for (const auto &pr : recomb_pairs)
                pairs.push(Json::object()
                               .set("left", Json::of(haplotype_name(pr.left)))
                               .set("right", Json::of(haplotype_name(pr.right)))
                               .set("reads", Json::of(pr.reads[0] + pr.reads[1]))
                               .set("insufficient_reads", Json::of(pr.reads[0]))
                               .set("damaged_reads", Json::of(pr.reads[1]))
                               .set("breakpoint_min", Json::of(pr.bp_min))
                               .set("breakpoint_max", Json::of(pr.bp_max)));
            rb.set("pairs", std::move(pairs));
            hb.set("recombinants", std::move(rb));
        }
        root.set("haplotype", std::move(hb));
    }
    if (R.linked) {   // --linkage (docs/SPEC.md §15): one entry per pair of rows v < w at different positions that some read covers both of
        const uint32_t V = (uint32_t)var.size(), P = (uint32_t)R.link_cols.size();
        Json lb = Json::object();
        Json pc = Json::array();
        for (uint32_t c : R.link_cols) pc.push(Json::of(win_begin + c + 1));
        lb.set("variant_positions_abs", std::move(pc)).set("n_variants", Json::of(V));
        Json pairs = Json::array();
        if (!R.link_skipped && V) {
            std::vector<uint32_t> at(V);   // row of the table -> variant of the call
            for (uint32_t k = 0; k < V; ++k) at[R.link_var[k]] = k;
            auto side = [&](const jl_variant &f) {
                return Json::object().set("gene", Json::of(cfg.genes[f.gene].name)).set("ref_position", Json::of(f.codon_pos + cfg.genes[f.gene].first_codon))
                    .set("codon", Json::of(codon_string(f.codon)));
            };
            for (uint32_t v = 0; v < V; ++v)
                for (uint32_t w = v + 1; w < V; ++w) {
                    if (var[v].col == var[w].col) continue;
                    jl_link_pair lp;
                    if (jl_linkage_stats(R.link_both.data(), R.link_carry.data(), R.link_joint.data(), R.link_var_pos.data(), P, V, at[v], at[w], &lp) != JL_OK)
                        die_jl(nullptr, "linkage statistics");
                    if (lp.n == 0) continue;
                    pairs.push(Json::object().set("a", side(var[v])).set("b", side(var[w])).set("reads_both", Json::of(lp.n))
                                   .set("n11", Json::of(lp.n11)).set("n10", Json::of(lp.n10)).set("n01", Json::of(lp.n01)).set("n00", Json::of(lp.n00))
                                   .set("r2", Json::of(lp.r2)).set("d_prime", Json::of(lp.d_prime))
                                   .set("p_positive", Json::of(lp.p_positive)).set("p_negative", Json::of(lp.p_negative)));
                }
        }
        lb.set("n_pairs_tested", Json::of((uint32_t)pairs.arr.size())).set("pairs", std::move(pairs));
        if (R.link_skipped) lb.set("skipped", Json::of(true));
        root.set("linkage", std::move(lb));
    }
    if (R.del_alleles) {   // --call-deletion-alleles (docs/SPEC.md §25): one entry per called allele, ascending by (begin_abs, length)
        Json db = Json::object();
        db.set("rate", Json::of(R.dal_rate)).set("min_length", Json::of(R.dal_min_length))
            .set("bounded_runs", Json::of((int64_t)R.dal_runs[0])).set("open_runs", Json::of((int64_t)R.dal_runs[1]))
            .set("n_alleles", Json::of(R.dal_n_alleles)).set("n_alleles_tested", Json::of(R.dal_n_tested));
        Json alleles = Json::array();
        for (const Results::DeletionAllele &d : R.dal_rows) {
            const uint32_t begin_abs = win_begin + d.allele.col + 1, end_abs = begin_abs + d.allele.len;   // 1-based [begin_abs, end_abs)
            Json gs = Json::array();
            for (const GeneCfg &g : cfg.genes) {   // the part of the extent inside the gene: amino-acid positions count from the gene's begin
                const uint32_t lo = std::max(begin_abs, g.begin_eff), hi = std::min(end_abs, g.end_eff);
                if (lo >= hi) continue;
                gs.push(Json::object().set("name", Json::of(g.name)).set("first_position", Json::of((lo - g.begin) / 3 + 1))
                            .set("last_position", Json::of((hi - 1 - g.begin) / 3 + 1))
                            .set("codon_aligned", Json::of((lo - g.begin) % 3 == 0 && (hi - g.begin) % 3 == 0)));
            }
            alleles.push(Json::object().set("begin_abs", Json::of(begin_abs)).set("length", Json::of(d.allele.len))
                             .set("count", Json::of(d.call.count)).set("coverage", Json::of(d.call.coverage))
                             .set("frequency", Json::of((double)d.call.count / (double)d.call.coverage))
                             .set("expected", Json::of(d.call.expected)).set("pValue", Json::of(d.call.p_value))
                             .set("log_pValue", Json::of(d.call.log_p)).set("in_frame", Json::of(d.allele.len % 3 == 0))
                             .set("genes", std::move(gs)));
        }
        db.set("alleles", std::move(alleles));
        root.set("deletion_alleles", std::move(db));
    }
    return root;
}

// --haplotype-fasta (docs/SPEC.md §13): one record per reported haplotype, in the JSON's order, from ONE class pileup of the window
// resident on `ctx` with the phasing run's own per-read ids as labels.  No reported haplotype: an empty file.  0, or the exit code.
int write_haplotype_fasta(const Options &opt, jl_ctx *ctx, const Results &R, uint32_t win_begin, uint32_t n_cols)
{
    const uint32_t H = R.ps.n_haplotypes;
    std::vector<uint32_t> counts((size_t)H * n_cols * 6);
    std::vector<uint32_t> rescued(H, 0u);
    if (H) {
        std::vector<uint16_t> with_rescued;   // --rescue-damaged: the damaged reads count for the haplotype they were assigned to
        if (R.rescued) {
            with_rescued.resize(R.read_hap.size());
            for (size_t i = 0; i < with_rescued.size(); ++i) {
                with_rescued[i] = R.hap_with_rescued(i);
                if (with_rescued[i] != R.read_hap[i]) rescued[with_rescued[i]]++;
            }
        }
        if (jl_class_pileup_async(ctx, R.rescued ? with_rescued.data() : R.read_hap.data(), H) != JL_OK) die_jl(ctx, "class pileup");
        if (jl_class_pileup_fetch(ctx, counts.data(), nullptr) != JL_OK) die_jl(ctx, "class pileup fetch");
    }
    std::ofstream f(opt.hap_fasta);
    if (!f) { std::cerr << "juliet: cannot write " << opt.hap_fasta << "\n"; return 2; }
    std::vector<uint8_t> cons(n_cols);
    for (uint32_t h = 0; h < H; ++h) {
        if (jl_consensus_of_counts(counts.data() + (size_t)h * n_cols * 6, n_cols, cons.data()) != JL_OK) die_jl(nullptr, "consensus of counts");
        std::string freq, seq;
        Json::of(R.ps.reported_reads ? (double)R.hap_count[h] / (double)R.ps.reported_reads : 0.0).write(freq);
        for (uint32_t c = 0; c < n_cols; ++c)
            if (cons[c] != 4) seq += "ACGT?N"[cons[c]];   // (4: a major deletion, the column is removed)
        f << ">" << haplotype_name(h) << " reads=" << R.hap_count[h] << (R.rescued ? " rescued=" + std::to_string(rescued[h]) : std::string())
          << " frequency=" << freq << " window=" << (win_begin + 1) << "-"
          << (win_begin + n_cols) << " source=" << opt.bam << "\n";
        for (size_t i = 0; i < seq.size(); i += 70) f << seq.substr(i, 70) << "\n";
    }
    f.close();
    if (!f) { std::cerr << "juliet: cannot write " << opt.hap_fasta << "\n"; return 2; }
    return 0;
}

// --consensus, and all of `fuse`: what `fuse` writes for the window resident on `ctx` (doc/FUSE.md:17-24), from the column counts
// in R and the insertion counters.  0, or the exit code.
int write_consensus(const Options &opt, jl_ctx *ctx, const Results &R, uint32_t win_begin, uint32_t n_cols)
{
    std::vector<uint32_t> len_hist((size_t)n_cols * 32), base_counts((size_t)n_cols * 120);
    if (jl_insertions_fetch(ctx, len_hist.data(), base_counts.data()) != JL_OK) die_jl(ctx, "insertions");
    const std::string seq = fuse_consensus(n_cols, R.col_counts, len_hist, base_counts, opt.ins_min_frac, opt.ins_min_distance);
    std::ofstream f(opt.consensus);
    if (!f) { std::cerr << "juliet: cannot write " << opt.consensus << "\n"; return 2; }
    f << ">consensus window=" << (win_begin + 1) << "-" << (win_begin + n_cols) << " source=" << opt.bam << "\n";
    for (size_t i = 0; i < seq.size(); i += 70) f << seq.substr(i, 70) << "\n";
    return 0;
}

// Every output of one run — the JSON text, or its HTML rendering, by extension — each file closed and its stream checked:
// a short write or a full disk is a failed output, not a quiet success.  "" or the first output that failed.
std::string write_outputs(const std::vector<std::string> &outputs, const Json &root)
{
    std::string text;
    root.write(text);
    text += "\n";
    for (const std::string &out : outputs) {
        std::ofstream f(out);
        if (!f) return out;
        if (out.substr(out.size() - 5) == ".json") f << text;
        else f << render_html(root);
        f.close();
        if (!f) return out;
    }
    return "";
}

}  // namespace
}  // namespace jlhost
