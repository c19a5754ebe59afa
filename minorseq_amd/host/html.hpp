// html.hpp — the HTML output: "a 1:1 conversion of the JSON file [that] contains the identical information, but more
// human-readable" (doc/JULIET.md:68-69), in the four sections of doc/JULIET.md:71-107 (Input data, Target config,
// Variant Discovery with the -3..+5 context counts and, with --mode-phasing, the haplotype columns, Drug Summaries)
// plus the root `haplotype` block (read categories of the tooltips, doc/JULIET.md:372-389; counts and read names,
// :209-211).  Every leaf of the JSON object is rendered; tests/test_gpu_cli.py parses the page back and compares it
// cell by cell.  Numbers are displayed as the reference's screenshots print them (format.hpp).
#pragma once
#include <string>

#include "format.hpp"
#include "json.hpp"

namespace jlhost {

inline std::string html_escape(const std::string &s)
{
    std::string o;
    for (char c : s) {
        if (c == '<') o += "&lt;";
        else if (c == '>') o += "&gt;";
        else if (c == '&') o += "&amp;";
        else if (c == '"') o += "&quot;";
        else o += c;
    }
    return o;
}

inline std::string num_str(const Json *j)
{
    if (!j) return "";
    if (j->type == Json::String) return j->str;
    if (j->type == Json::Bool) return j->b ? "true" : "false";
    std::string s;
    j->write(s);
    return s;
}

inline std::string td(const std::string &s, const char *cls = nullptr)
{
    return std::string("<td") + (cls ? std::string(" class=\"") + cls + "\"" : std::string()) + ">" + html_escape(s) + "</td>";
}

inline std::string render_html(const Json &root)
{
    std::string h = "<!DOCTYPE html><html><head><meta charset=\"utf-8\"><title>Minor Variants Summary (Juliet)</title>"
                    "<style>body{font-family:sans-serif}table{border-collapse:collapse;margin:4px 0}td,th{border:1px solid #999;padding:2px 8px;"
                    "text-align:center}td.hit{background:#e8381b;color:#fff}td.nohit{background:#4a4a4a}summary{font-weight:bold;font-size:120%}"
                    "table.msa td.wt{font-weight:bold}</style></head><body>\n<h1>Minor Variants Summary (Juliet)</h1>\n";
    // ---- 1. Input data (doc/JULIET.md:73-79)
    if (const Json *in = root.get("input")) {
        h += "<details open id=\"input\"><summary>Input data</summary><table id=\"input-table\">\n";
        for (auto &kv : in->obj)
            if (kv.first != "sampling" && kv.first != "read_filter" && kv.first != "hypermutation" && kv.first != "orf_integrity" && kv.first != "control") h += "<tr><th>" + html_escape(kv.first) + "</th>" + td(num_str(&kv.second)) + "</tr>\n";
        h += "</table>\n";
        // --downsample / --mix: the seed and, per source, its file, its reads and how many of them were kept (docs/SPEC.md section 12)
        if (const Json *sp = in->get("sampling")) {
            h += "<table id=\"sampling-table\" data-seed=\"" + num_str(sp->get("seed")) + "\">\n<tr><th>sampling (seed " + num_str(sp->get("seed")) +
                 ")</th><th>reads</th><th>kept</th></tr>\n";
            if (const Json *srcs = sp->get("sources"))
                for (const Json &x : srcs->arr)
                    h += "<tr>" + td(x.get_str("file")) + td(num_str(x.get("reads"))) + td(num_str(x.get("kept"))) + "</tr>\n";
            h += "</table>\n";
        }
        // --control: the control sample the codons were called against (docs/SPEC.md section 21)
        if (const Json *ct = in->get("control"))
            h += "<table id=\"control-table\">\n<tr><th>control</th><th>reads</th></tr>\n<tr>" + td(ct->get_str("file")) + td(num_str(ct->get("reads"))) +
                 "</tr>\n</table>\n";
        // the read filter: its compare row, the rules that were given, and the reads each rule failed (docs/SPEC.md section 20)
        if (const Json *rf = in->get("read_filter")) {
            h += "<table id=\"read-filter-table\" data-compare=\"" + html_escape(rf->get_str("compare")) + "\">\n<tr><th>read filter (compare: " +
                 html_escape(rf->get_str("compare")) + ")</th><th>bound</th><th>failed</th></tr>\n";
            h += "<tr class=\"reads\">" + td("reads") + td("") + td(num_str(rf->get("reads"))) + "</tr>\n";
            h += "<tr class=\"kept\">" + td("kept") + td("") + td(num_str(rf->get("kept"))) + "</tr>\n";
            const Json *rule = rf->get("rule");
            if (const Json *failed = rf->get("failed"))
                for (auto &kv : failed->obj)
                    h += "<tr class=\"rule\">" + td(kv.first) + td(rule ? num_str(rule->get(kv.first)) : "") + td(num_str(&kv.second)) + "</tr>\n";
            h += "</table>\n";
        }
        // the hypermutation filter: its reference row, its level, and the reads it flagged and kept (docs/SPEC.md section 26)
        if (const Json *hj = in->get("hypermutation")) {
            h += "<table id=\"hypermutation-table\" data-reference=\"" + html_escape(hj->get_str("reference")) + "\">\n<tr><th>hypermutation filter (G of: " +
                 html_escape(hj->get_str("reference")) + ")</th><th>value</th></tr>\n";
            for (const char *leaf : {"alpha", "reads", "flagged", "kept", "dropped"})
                h += std::string("<tr class=\"") + leaf + "\">" + td(leaf) + td(num_str(hj->get(leaf))) + "</tr>\n";
            h += "</table>\n";
        }
        // the reading-frame filter: its reference row, its rule, the reads it found defective and kept, and per gene the reads of every flag (docs/SPEC.md section 27)
        if (const Json *oj = in->get("orf_integrity")) {
            h += "<table id=\"orf-integrity-table\" data-reference=\"" + html_escape(oj->get_str("reference")) + "\">\n<tr><th>reading-frame filter (stops of: " +
                 html_escape(oj->get_str("reference")) + ")</th><th>value</th></tr>\n";
            for (const char *leaf : {"kinds", "max_deletion", "tail_codons", "reads", "defective", "kept", "dropped"})
                h += std::string("<tr class=\"") + leaf + "\">" + td(leaf) + td(num_str(oj->get(leaf))) + "</tr>\n";
            h += "</table>\n<table id=\"orf-integrity-genes\">\n<tr><th>gene</th><th>partial</th><th>stop</th><th>frameshift</th><th>deletion</th></tr>\n";
            if (const Json *genes = oj->get("genes"))
                for (const Json &g : genes->arr) {
                    h += "<tr class=\"gene\">" + td(html_escape(g.get_str("name")));
                    for (const char *leaf : {"partial", "stop", "frameshift", "deletion"}) h += td(num_str(g.get(leaf)));
                    h += "</tr>\n";
                }
            h += "</table>\n";
        }
        h += "</details>\n";
    }
    // ---- 2. Target config (doc/JULIET.md:83-88)
    if (const Json *tc = root.get("target_config")) {
        h += "<details open id=\"target\"><summary>Target config</summary><table id=\"target-table\">\n";
        for (auto &kv : tc->obj)
            if (kv.first != "genes") h += "<tr><th>" + html_escape(kv.first) + "</th>" + td(num_str(&kv.second)) + "</tr>\n";
        h += "</table>\n<ul id=\"target-genes\">\n";
        if (const Json *gs = tc->get("genes"))
            for (const Json &g : gs->arr) {
                h += "<li data-begin=\"" + num_str(g.get("begin")) + "\" data-end=\"" + num_str(g.get("end")) + "\"><b>" +
                     html_escape(g.get_str("name")) + "</b> (" + num_str(g.get("begin")) + "-" + num_str(g.get("end")) + ")";
                const Json *ds = g.get("drms");
                if (ds && !ds->arr.empty()) {
                    h += "<ul>";
                    for (const Json &d : ds->arr) {
                        h += "<li class=\"drm\"><span class=\"drm-name\">" + html_escape(d.get_str("name")) + "</span>:";
                        if (const Json *ps = d.get("positions"))
                            for (const Json &p : ps->arr) h += " <span class=\"drm-pos\">" + html_escape(p.str) + "</span>";
                        h += "</li>";
                    }
                    h += "</ul>";
                }
                h += "</li>\n";
            }
        h += "</ul></details>\n";
    }
    // haplotype header shared by every gene table: names and percentages (columns are global across genes,
    // juliet_hiv-phasing.png)
    const Json *hb = root.get("haplotype");
    const Json *haps = hb ? hb->get("haplotypes") : nullptr;
    // ---- 3. Variant Discovery (doc/JULIET.md:92-102)
    if (const Json *genes = root.get("genes")) {
        h += "<details open id=\"variants\"><summary>Variant Discovery</summary>\n";
        const std::string ref_name = root.get("target_config") ? root.get("target_config")->get_str("referenceName") : "";
        for (const Json &g : genes->arr) {
            h += "<table class=\"gene\" data-gene=\"" + html_escape(g.get_str("name")) + "\"><caption>" + html_escape(g.get_str("name")) +
                 "</caption>\n<tr><th colspan=\"3\">" + html_escape(ref_name.empty() ? "Majority Call" : ref_name) +
                 "</th><th colspan=\"5\">Sample Variants</th>";
            if (haps)
                for (const Json &hp : haps->arr) h += "<th class=\"hapname\">" + html_escape(hp.get_str("name")) + "</th>";
            h += "</tr>\n<tr><th>Codon</th><th>AA</th><th>Pos</th><th>AA</th><th>Codon</th><th>%</th><th>Coverage</th><th>Affected Drugs</th>";
            if (haps)
                for (const Json &hp : haps->arr) h += "<th class=\"happerc\">" + format_hap_percent(100.0 * hp.get("frequency")->num) + "</th>";
            h += "</tr>\n";
            if (const Json *vps = g.get("variant_positions"))
                for (const Json &vp : vps->arr) {
                    for (const Json &aa : vp.get("variant_amino_acids")->arr)
                        for (const Json &vc : aa.get("variant_codons")->arr) {
                            h += "<tr class=\"variant\" title=\"count=" + num_str(vc.get("count")) + " expected=" + num_str(vc.get("expected")) +
                                 " pValue=" + num_str(vc.get("pValue")) + " log_pValue=" + num_str(vc.get("log_pValue")) +
                                 (vc.get("control_count") ? " control_count=" + num_str(vc.get("control_count")) + " control_coverage=" +
                                                                num_str(vc.get("control_coverage")) + " control_frequency=" + num_str(vc.get("control_frequency"))
                                                          : std::string()) +
                                 "\">" +
                                 td(vp.get_str("ref_codon")) + td(vp.get_str("ref_amino_acid")) + td(num_str(vp.get("ref_position"))) +
                                 td(aa.get_str("amino_acid")) + td(vc.get_str("codon")) + td(format_percent(100.0 * vc.get("frequency")->num)) +
                                 td(num_str(vp.get("coverage"))) + td(vc.get_str("known_drm"));
                            const Json *hcnt = vc.get("haplotype_count"), *hcov = vc.get("haplotype_coverage");   // --haplotype-mutations (docs/SPEC.md §24)
                            if (const Json *hh = vc.get("haplotype_hit"))
                                for (size_t x = 0; x < hh->arr.size(); ++x) {
                                    if (!hcnt || x >= hcnt->arr.size()) { h += hh->arr[x].b ? "<td class=\"hit\">x</td>" : "<td class=\"nohit\"></td>"; continue; }
                                    h += std::string("<td class=\"") + (hh->arr[x].b ? "hit" : "nohit") + "\" data-count=\"" + num_str(&hcnt->arr[x]) +
                                         "\" data-coverage=\"" + num_str(&hcov->arr[x]) + "\">" + (hh->arr[x].b ? "x" : "") + "</td>";
                                }
                            h += "</tr>\n";
                        }
                    // "Clicking the row will show counts of the multiple-sequence alignment counts of the -3 to +3 context positions"
                    if (const Json *msa = vp.get("msa")) {
                        h += "<tr class=\"context\"><td colspan=\"8\"><details><summary>context</summary><table class=\"msa\" data-pos=\"" +
                             num_str(vp.get("ref_position")) + "\"><tr><th>Pos</th><th>Abs</th><th>A</th><th>C</th><th>G</th><th>T</th><th>-</th><th>N</th><th>wt</th></tr>\n";
                        for (const Json &m : msa->arr) {
                            const std::string wt = m.get_str("wt");
                            h += "<tr>" + td(num_str(m.get("rel_pos"))) + td(num_str(m.get("abs_pos")));
                            static const char *sym[6] = {"A", "C", "G", "T", "-", "N"};
                            for (int s = 0; s < 6; ++s) h += td(num_str(m.get(sym[s])), wt == sym[s] ? "wt" : nullptr);
                            h += td(wt) + "</tr>\n";
                        }
                        h += "</table></details></td></tr>\n";
                    }
                }
            h += "</table>\n";
        }
        h += "</details>\n";
    }
    // ---- --call-deletions (docs/SPEC.md §16): the called codon deletions, a table per gene; doubles as the JSON prints them
    if (const Json *genes = root.get("genes")) {
        bool any = false;
        for (const Json &g : genes->arr) any = any || g.get("deletion_positions");
        if (any) {
            h += "<details open id=\"deletions\"><summary>Codon Deletions</summary>\n";
            for (const Json &g : genes->arr) {
                const Json *dps = g.get("deletion_positions");
                if (!dps) continue;
                h += "<table class=\"deletions\" data-gene=\"" + html_escape(g.get_str("name")) + "\"><caption>" + html_escape(g.get_str("name")) +
                     "</caption>\n<tr><th>Pos</th><th>Codon</th><th>AA</th><th>#Reads</th><th>Coverage</th><th>Frequency</th><th>Expected</th>"
                     "<th>pValue</th><th>log_pValue</th><th>#Frame-shift reads</th>";
                if (haps && hb->get("deletion_positions_abs"))   // --phase-deletions (docs/SPEC.md §18): a column per haplotype
                    for (const Json &hp : haps->arr) h += "<th class=\"hapname\">" + html_escape(hp.get_str("name")) + "</th>";
                h += "</tr>\n";
                for (const Json &d : dps->arr) {
                    h += "<tr class=\"deletion\">" + td(num_str(d.get("ref_position"))) + td(d.get_str("ref_codon")) + td(d.get_str("ref_amino_acid"));
                    for (const char *key : {"count", "coverage", "frequency", "expected", "pValue", "log_pValue", "frameshift_reads"}) h += td(num_str(d.get(key)));
                    if (const Json *hh = d.get("haplotype_hit"))
                        for (const Json &x : hh->arr) h += x.b ? "<td class=\"hit\">x</td>" : "<td class=\"nohit\"></td>";
                    h += "</tr>\n";
                }
                h += "</table>\n";
            }
            h += "</details>\n";
        }
    }
    // ---- --call-insertions (docs/SPEC.md §17): the called insertion alleles, a table per gene; doubles as the JSON prints them
    if (const Json *genes = root.get("genes")) {
        bool any = false;
        for (const Json &g : genes->arr) any = any || g.get("insertion_positions");
        if (any) {
            h += "<details open id=\"insertions\"><summary>Codon Insertions</summary>\n";
            for (const Json &g : genes->arr) {
                const Json *ips = g.get("insertion_positions");
                if (!ips) continue;
                h += "<table class=\"insertions\" data-gene=\"" + html_escape(g.get_str("name")) + "\"><caption>" + html_escape(g.get_str("name")) +
                     "</caption>\n<tr><th>After pos</th><th>Codons</th><th>AA</th><th>#Reads</th><th>Coverage</th><th>Frequency</th><th>Expected</th>"
                     "<th>pValue</th><th>log_pValue</th><th>#Frame-shift reads</th><th>#Unread reads</th>";
                if (haps && hb->get("insertion_alleles"))   // --phase-insertions (docs/SPEC.md §19): a column per haplotype
                    for (const Json &hp : haps->arr) h += "<th class=\"hapname\">" + html_escape(hp.get_str("name")) + "</th>";
                h += "</tr>\n";
                for (const Json &d : ips->arr) {
                    std::string cods;
                    for (const Json &c : d.get("inserted_codons")->arr) cods += (cods.empty() ? "" : " ") + c.str;
                    h += "<tr class=\"insertion\">" + td(num_str(d.get("after_position"))) + td(cods) + td(d.get_str("inserted_amino_acids"));
                    for (const char *key : {"count", "coverage", "frequency", "expected", "pValue", "log_pValue", "frameshift_reads", "unread_reads"})
                        h += td(num_str(d.get(key)));
                    if (const Json *hh = d.get("haplotype_hit"))
                        for (const Json &x : hh->arr) h += x.b ? "<td class=\"hit\">x</td>" : "<td class=\"nohit\"></td>";
                    h += "</tr>\n";
                }
                h += "</table>\n";
            }
            h += "</details>\n";
        }
    }
    // ---- 4. Drug Summaries (doc/JULIET.md:104-107)
    if (const Json *ds = root.get("drug_summaries")) {
        h += "<details open id=\"drugs\"><summary>Drug Summaries</summary><table id=\"drug-table\"><tr><th>Drug</th><th>Gene</th><th>Mutation</th><th>Codon</th><th>%</th></tr>\n";
        for (const Json &d : ds->arr)
            for (const Json &v : d.get("variants")->arr)
                h += "<tr>" + td(d.get_str("drug")) + td(v.get_str("gene")) + td(v.get_str("mutation")) + td(v.get_str("codon")) +
                     td(format_percent(100.0 * v.get("frequency")->num)) + "</tr>\n";
        h += "</table></details>\n";
    }
    // ---- the root `haplotype` block (doc/JULIET.md:209-211, 372-389)
    if (hb) {
        h += "<details open id=\"haplotypes\"><summary>Haplotypes</summary><table id=\"hap-categories\"><tr><th>Haplotype Category</th><th>#Reads</th></tr>\n";
        static const char *cat[6][2] = {{"reported_reads", "Reported"}, {"insufficient_coverage_reads", "Insufficient Coverage (unreported)"},
                                        {"damaged_reads", "Overall Damaged (unreported)"}, {"marginal_gaps", "- Marginal Gaps"},
                                        {"marginal_heteroduplexes", "- Marginal Heteroduplexes"}, {"marginal_partial", "- Marginal Partial"}};
        for (auto &c : cat) h += "<tr data-key=\"" + std::string(c[0]) + "\"><th>" + c[1] + "</th>" + td(num_str(hb->get(c[0]))) + "</tr>\n";
        h += "</table>\n<p id=\"hap-positions\">";
        if (const Json *pc = hb->get("variant_positions_abs"))
            for (const Json &p : pc->arr) h += "<span>" + num_str(&p) + "</span> ";
        h += "</p>\n";
        const Json *dpa = hb->get("deletion_positions_abs");   // --phase-deletions (docs/SPEC.md §18)
        if (dpa) {
            h += "<p id=\"hap-deletion-positions\">";
            for (const Json &p : dpa->arr) h += "<span>" + num_str(&p) + "</span> ";
            h += "</p>\n";
        }
        const Json *ial = hb->get("insertion_alleles");        // --phase-insertions (docs/SPEC.md §19)
        if (ial) {
            h += "<p id=\"hap-insertion-alleles\">";
            for (const Json &a : ial->arr) {
                std::string cods;
                for (const Json &c : a.get("inserted_codons")->arr) cods += (cods.empty() ? "" : " ") + c.str;
                h += "<span data-gene=\"" + html_escape(a.get_str("gene")) + "\" data-after=\"" + num_str(a.get("after_position")) + "\">" + cods + "</span> ";
            }
            h += "</p>\n";
        }
        h += std::string("<table id=\"hap-table\"><tr><th>Haplotype</th><th>%</th><th>#Reads</th><th>Codons</th>") + (dpa ? "<th>Deletions</th>" : "") +
             (ial ? "<th>Insertions</th>" : "") + "<th>Read names</th></tr>\n";
        if (haps)
            for (const Json &hp : haps->arr) {
                h += "<tr>" + td(hp.get_str("name")) + td(format_hap_percent(100.0 * hp.get("frequency")->num)) + td(num_str(hp.get("reads"))) + "<td>";
                if (const Json *cs = hp.get("codons"))
                    for (size_t i = 0; i < cs->arr.size(); ++i) h += (i ? " " : "") + cs->arr[i].str;
                h += "</td>";
                if (const Json *ds = hp.get("deletions")) {
                    h += "<td class=\"hap-deletions\">";
                    for (size_t i = 0; i < ds->arr.size(); ++i) h += std::string(i ? " " : "") + (ds->arr[i].b ? "x" : "-");
                    h += "</td>";
                }
                if (const Json *is = hp.get("insertions")) {
                    h += "<td class=\"hap-insertions\">";
                    for (size_t i = 0; i < is->arr.size(); ++i) h += std::string(i ? " " : "") + (is->arr[i].b ? "x" : "-");
                    h += "</td>";
                }
                h += "<td><details><summary>" + std::to_string(hp.get("read_names") ? hp.get("read_names")->arr.size() : 0) + "</summary>";
                if (const Json *rn = hp.get("read_names"))
                    for (const Json &r : rn->arr) h += "<span class=\"rn\">" + html_escape(r.str) + "</span> ";
                h += "</details></td></tr>\n";
            }
        h += "</table>";
        if (const Json *dp = hb->get("drug_profile")) {   // --haplotype-mutations (docs/SPEC.md §24); doubles as the JSON prints them
            h += "\n<table id=\"hap-mutations\"><tr><th>Haplotype</th><th>Gene</th><th>Pos</th><th>Ref codon</th><th>Ref AA</th><th>Codon</th><th>AA</th>"
                 "<th>#Reads</th><th>Coverage</th><th>Frequency</th><th>Affected Drugs</th></tr>\n";
            if (haps)
                for (const Json &hp : haps->arr)
                    if (const Json *ms = hp.get("mutations"))
                        for (const Json &m : ms->arr) {
                            h += "<tr data-haplotype=\"" + html_escape(hp.get_str("name")) + "\">" + td(hp.get_str("name")) + td(m.get_str("gene")) +
                                 td(num_str(m.get("position"))) + td(m.get_str("ref_codon")) + td(m.get_str("ref_amino_acid")) + td(m.get_str("codon")) +
                                 td(m.get_str("amino_acid")) + td(num_str(m.get("count"))) + td(num_str(m.get("coverage"))) + td(num_str(m.get("frequency"))) + "<td>";
                            for (const Json &d : m.get("drms")->arr) h += "<span class=\"drm-name\">" + html_escape(d.str) + "</span> ";
                            h += "</td></tr>\n";
                        }
            h += "</table>\n<table id=\"hap-drugs\"><tr><th>Haplotype</th><th>Drugs</th></tr>\n";
            if (haps)
                for (const Json &hp : haps->arr) {
                    h += "<tr>" + td(hp.get_str("name")) + "<td>";
                    if (const Json *ds = hp.get("drugs"))
                        for (const Json &d : ds->arr) h += "<span class=\"drm-name\">" + html_escape(d.str) + "</span> ";
                    h += "</td></tr>\n";
                }
            h += "</table>\n<table id=\"hap-drug-profile\"><tr><th>Drug</th>";
            if (haps)
                for (const Json &hp : haps->arr) h += "<th class=\"hapname\">" + html_escape(hp.get_str("name")) + "</th>";
            h += "<th>#Reads</th><th>Frequency</th></tr>\n";
            for (const Json &d : dp->arr) {
                h += "<tr>" + td(d.get_str("drug"));
                for (const Json &x : d.get("haplotypes")->arr) h += x.b ? "<td class=\"hit\">x</td>" : "<td class=\"nohit\"></td>";
                h += td(num_str(d.get("reads"))) + td(num_str(d.get("frequency"))) + "</tr>\n";
            }
            h += "</table>\n";
        }
        if (const Json *rs = hb->get("rescue")) {   // --rescue-damaged (docs/SPEC.md §14): the damaged reads, judged where they can be read
            h += "\n<table id=\"hap-rescue\"><tr><th>Damaged reads, rescued (at least " + num_str(rs->get("min_positions")) +
                 " informative positions)</th><th>#Reads</th></tr>\n";
            static const char *rc[4][2] = {{"assigned_reads", "Assigned to one haplotype"}, {"ambiguous_reads", "Ambiguous (several agree)"},
                                           {"incompatible_reads", "Incompatible (none agrees)"}, {"uninformative_reads", "Uninformative"}};
            for (auto &c : rc) h += "<tr data-key=\"" + std::string(c[0]) + "\"><th>" + c[1] + "</th>" + td(num_str(rs->get(c[0]))) + "</tr>\n";
            h += "</table>\n<table id=\"hap-rescued\"><tr><th>Haplotype</th><th>% with rescued</th><th>#Rescued</th><th>Rescued read names</th></tr>\n";
            if (haps)
                for (const Json &hp : haps->arr) {
                    if (!hp.get("rescued_reads")) continue;
                    h += "<tr>" + td(hp.get_str("name")) + td(format_hap_percent(100.0 * hp.get("frequency_with_rescued")->num)) +
                         td(num_str(hp.get("rescued_reads"))) + "<td><details><summary>" +
                         std::to_string(hp.get("rescued_read_names")->arr.size()) + "</summary>";
                    for (const Json &r : hp.get("rescued_read_names")->arr) h += "<span class=\"rn\">" + html_escape(r.str) + "</span> ";
                    h += "</details></td></tr>\n";
                }
            h += "</table>\n";
        }
        if (const Json *ab = hb->get("absorb")) {   // --absorb-distance (docs/SPEC.md §22): the reads phasing left out, by their nearest haplotype
            h += "\n<table id=\"hap-absorb\" data-max-distance=\"" + num_str(ab->get("max_distance")) + "\" data-min-positions=\"" +
                 num_str(ab->get("min_positions")) + "\"><tr><th>Reads absorbed (at most " + num_str(ab->get("max_distance")) +
                 " codons away, at least " + num_str(ab->get("min_positions")) + " informative positions)</th><th>#Insufficient</th><th>#Damaged</th></tr>\n";
            static const char *ac[4][2] = {{"assigned_reads", "Assigned to the nearest haplotype"}, {"ambiguous_reads", "Ambiguous (several are nearest)"},
                                           {"distant_reads", "Distant (none within the budget)"}, {"uninformative_reads", "Uninformative"}};
            const Json *ins = ab->get("insufficient"), *dam = ab->get("damaged");
            for (auto &c : ac)
                h += "<tr data-key=\"" + std::string(c[0]) + "\"><th>" + c[1] + "</th>" + td(num_str(ins->get(c[0]))) + td(num_str(dam->get(c[0]))) + "</tr>\n";
            for (size_t d = 0; d < ins->get("assigned_by_distance")->arr.size(); ++d)
                h += "<tr data-key=\"assigned_by_distance\" data-distance=\"" + std::to_string(d) + "\"><th>- assigned at distance " + std::to_string(d) +
                     "</th>" + td(num_str(&ins->get("assigned_by_distance")->arr[d])) + td(num_str(&dam->get("assigned_by_distance")->arr[d])) + "</tr>\n";
            h += "</table>\n<table id=\"hap-absorbed\"><tr><th>Haplotype</th><th>% with absorbed</th><th>#Absorbed</th><th>#Absorbed damaged</th>"
                 "<th>Absorbed read names</th></tr>\n";
            if (haps)
                for (const Json &hp : haps->arr) {
                    if (!hp.get("absorbed_reads")) continue;
                    h += "<tr>" + td(hp.get_str("name")) + td(format_hap_percent(100.0 * hp.get("frequency_with_absorbed")->num)) +
                         td(num_str(hp.get("absorbed_reads"))) + td(num_str(hp.get("absorbed_damaged_reads"))) + "<td><details><summary>" +
                         std::to_string(hp.get("absorbed_read_names")->arr.size()) + "</summary>";
                    for (const Json &r : hp.get("absorbed_read_names")->arr) h += "<span class=\"rn\">" + html_escape(r.str) + "</span> ";
                    h += "</details></td></tr>\n";
                }
            h += "</table>\n";
        }
        if (const Json *rc = hb->get("recombinants")) {   // --flag-recombinants (docs/SPEC.md §23): reads and haplotypes that are one haplotype, then another
            h += "\n<table id=\"hap-recombinants\" data-min-positions=\"" + num_str(rc->get("min_positions")) + "\" data-parent-ratio=\"" +
                 num_str(rc->get("parent_ratio")) + "\"><tr><th>Reads as recombinants of two haplotypes (at least " + num_str(rc->get("min_positions")) +
                 " informative positions)</th><th>#Insufficient</th><th>#Damaged</th></tr>\n";
            static const char *cc[5][2] = {{"recombinant_reads", "Recombinant (both parents unique)"}, {"ambiguous_parent_reads", "Recombinant, a parent ambiguous"},
                                           {"whole_reads", "Whole (a haplotype agrees throughout)"}, {"unexplained_reads", "Unexplained by one breakpoint"},
                                           {"uninformative_reads", "Uninformative"}};
            const Json *ins = rc->get("insufficient"), *dam = rc->get("damaged");
            for (auto &c : cc)
                h += "<tr data-key=\"" + std::string(c[0]) + "\"><th>" + c[1] + "</th>" + td(num_str(ins->get(c[0]))) + td(num_str(dam->get(c[0]))) + "</tr>\n";
            h += "</table>\n<table id=\"hap-recombinant-pairs\"><tr><th>Left</th><th>Right</th><th>#Reads</th><th>#Insufficient</th><th>#Damaged</th>"
                 "<th>Breakpoint from</th><th>Breakpoint to</th></tr>\n";
            for (const Json &pr : rc->get("pairs")->arr)
                h += "<tr>" + td(pr.get_str("left")) + td(pr.get_str("right")) + td(num_str(pr.get("reads"))) + td(num_str(pr.get("insufficient_reads"))) +
                     td(num_str(pr.get("damaged_reads"))) + td(num_str(pr.get("breakpoint_min"))) + td(num_str(pr.get("breakpoint_max"))) + "</tr>\n";
            h += "</table>\n<table id=\"hap-putative-recombinants\"><tr><th>Haplotype</th><th>Putative recombinant</th><th>Left</th><th>Right</th>"
                 "<th>Prefix</th><th>Suffix</th></tr>\n";
            if (haps)
                for (const Json &hp : haps->arr) {
                    const Json *of = hp.get("recombinant_of");
                    h += "<tr>" + td(hp.get_str("name")) + td(of ? "yes" : "no") + td(of ? of->get_str("left") : "") + td(of ? of->get_str("right") : "") +
                         td(of ? num_str(of->get("prefix")) : "") + td(of ? num_str(of->get("suffix")) : "") + "</tr>\n";
                }
            h += "</table>\n";
        }
        h += "</details>\n";
    }
    // ---- --linkage (docs/SPEC.md §15): every pair of variants over the reads covering both; doubles as the JSON prints them
    if (const Json *lb = root.get("linkage")) {
        h += "<details open id=\"linkage\"><summary>Linkage</summary><table id=\"linkage-summary\">\n";
        for (const char *key : {"n_variants", "n_pairs_tested", "skipped"})
            if (lb->get(key)) h += "<tr data-key=\"" + std::string(key) + "\"><th>" + key + "</th>" + td(num_str(lb->get(key))) + "</tr>\n";
        h += "</table>\n<p id=\"linkage-positions\">";
        if (const Json *pc = lb->get("variant_positions_abs"))
            for (const Json &p : pc->arr) h += "<span>" + num_str(&p) + "</span> ";
        h += "</p>\n<table id=\"linkage-table\"><tr><th>Gene</th><th>Pos</th><th>Codon</th><th>Gene</th><th>Pos</th><th>Codon</th><th>#Reads both</th>"
             "<th>n11</th><th>n10</th><th>n01</th><th>n00</th><th>r2</th><th>D'</th><th>p positive</th><th>p negative</th></tr>\n";
        if (const Json *pairs = lb->get("pairs"))
            for (const Json &pr : pairs->arr) {
                h += "<tr>";
                for (const char *s : {"a", "b"}) h += td(pr.get(s)->get_str("gene")) + td(num_str(pr.get(s)->get("ref_position"))) + td(pr.get(s)->get_str("codon"));
                for (const char *key : {"reads_both", "n11", "n10", "n01", "n00", "r2", "d_prime", "p_positive", "p_negative"}) h += td(num_str(pr.get(key)));
                h += "</tr>\n";
            }
        h += "</table></details>\n";
    }
    // ---- --call-deletion-alleles (docs/SPEC.md §25): the called deletions by extent, one table; doubles as the JSON prints them
    if (const Json *db = root.get("deletion_alleles")) {
        h += "<details open id=\"deletion-alleles\"><summary>Deletion alleles</summary><table id=\"deletion-alleles-summary\">\n";
        for (const char *key : {"rate", "min_length", "bounded_runs", "open_runs", "n_alleles", "n_alleles_tested"})
            h += "<tr data-key=\"" + std::string(key) + "\"><th>" + key + "</th>" + td(num_str(db->get(key))) + "</tr>\n";
        h += "</table>\n<table id=\"deletion-alleles-table\"><tr><th>Begin</th><th>Length</th><th>#Reads</th><th>Coverage</th><th>Frequency</th>"
             "<th>Expected</th><th>p</th><th>ln p</th><th>In frame</th><th>Genes</th></tr>\n";
        if (const Json *al = db->get("alleles"))
            for (const Json &a : al->arr) {
                h += "<tr class=\"deletion-allele\">";
                for (const char *key : {"begin_abs", "length", "count", "coverage", "frequency", "expected", "pValue", "log_pValue", "in_frame"}) h += td(num_str(a.get(key)));
                std::string gs;   // name first-last aligned|unaligned, the genes separated by "; "
                if (const Json *genes = a.get("genes"))
                    for (const Json &g : genes->arr)
                        gs += (gs.empty() ? "" : "; ") + g.get_str("name") + " " + num_str(g.get("first_position")) + "-" + num_str(g.get("last_position")) +
                              (g.get("codon_aligned") && g.get("codon_aligned")->b ? " aligned" : " unaligned");
                h += td(gs) + "</tr>\n";
            }
        h += "</table></details>\n";
    }
    h += "</body></html>\n";
    return h;
}

}  // namespace jlhost
