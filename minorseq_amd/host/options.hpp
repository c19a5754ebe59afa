// options.hpp — the command line of `juliet` / `fuse`: Options, the usage text, parse() with everything it refuses before any
// file is read or any GPU work starts, and the --batch list (read_batch_list, output_kind_ok).  Like the headers below it, a part
// of juliet_main.cpp's one translation unit: internal linkage, as in the file it was cut from.
#pragma once
#include <cstdlib>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <map>
#include <string>
#include <vector>

#include "../../include/juliet_hip.h"

namespace jlhost {
namespace {

const char *kVersion = "0.1.0 (minorseq_amd, MI355X)";

struct Options {
    std::string bam, config;
    std::vector<std::string> outputs;
    bool phasing = false, drm_only = false;
    bool have_region = false;
    uint32_t region_b = 0, region_e = 0;
    double min_perc = -1.0, max_perc = -1.0;
    double alpha = 0.01, n_tests = 0.0;
    std::string chemistry = "auto";
    double match = -1.0, substitution = -1.0;
    int expected_round = 0;
    int fisher_tail = 0;             // --fisher-tail greater|two-sided (doc/JULIET.md:38-42 leaves the sidedness open)
    uint32_t min_reads = 10, min_qv = 0;
    bool qv_upload_mask = false;     // --qv-upload mask|bytes: what --min-qv sends to the device (bytes: DESIGN.md, the record ingest)
    double min_rq = 0.0;
    int device = 0;
    uint32_t windows = 1;            // column windows the reference is cut into (doc/JULIET.md:261-264: the split never shows)
    std::vector<int> devices;        // --devices a,b,...: one rank (thread) per device, consecutive windows each
    std::string dump_msa, dump_config, consensus;
    std::string hap_fasta;           // --haplotype-fasta: one consensus per reported haplotype (docs/SPEC.md §13)
    bool hap_mutations = false;      // --haplotype-mutations: per-haplotype codon tables and drug profile (docs/SPEC.md §24)
    bool rescue = false;             // --rescue-damaged: which reported haplotype each damaged read agrees with (docs/SPEC.md §14)
    uint32_t rescue_min = 1;         // --rescue-min-positions K: informative positions a read needs to be judged at all
    bool have_rescue_min = false;
    uint32_t absorb_distance = 0;    // --absorb-distance D: reads join the one reported haplotype nearest to them, D codons away at most (docs/SPEC.md §22)
    bool have_absorb = false;
    uint32_t absorb_min = 0;         // --absorb-min-positions K: informative positions a read needs to be judged at all (default D + 1)
    bool have_absorb_min = false;
    bool flag_recombinants = false;  // --flag-recombinants: reads and haplotypes that are one haplotype up to a breakpoint and another from there on (docs/SPEC.md §23)
    uint32_t recomb_min = 2;         // --recombinant-min-positions K: informative positions a read needs to be judged at all
    bool have_recomb_min = false;
    double recomb_ratio = 2.0;       // --recombinant-parent-ratio r: a parent of a haplotype has r times its reads at least
    bool have_recomb_ratio = false;
    bool linkage = false;            // --linkage: every pair of called variants over the reads covering both (docs/SPEC.md §15)
    bool call_deletions = false;     // --call-deletions: in-frame codon deletions at every evaluated position (docs/SPEC.md §16)
    bool phase_deletions = false;    // --phase-deletions: the called deletions as sites of the haplotypes (docs/SPEC.md §18)
    bool phase_insertions = false;   // --phase-insertions: the called insertion alleles as sites of the haplotypes (docs/SPEC.md §19)
    bool call_insertions = false;    // --call-insertions: in-frame insertion alleles before every evaluated position (docs/SPEC.md §17)
    bool have_insertion_rate = false;
    double insertion_rate = 0.0;     // --insertion-rate r: a read shows an in-frame insertion at a junction by error (default: the chemistry's deletion rate)
    bool call_deletion_alleles = false;   // --call-deletion-alleles: deletions by (start, length) over the whole window (docs/SPEC.md §25)
    bool have_deletion_allele_rate = false;
    double deletion_allele_rate = 0.0;    // --deletion-allele-rate r: a read shows one given deletion by error (default: the chemistry's deletion rate)
    bool have_min_deletion_length = false;
    uint32_t min_deletion_length = 1;     // --min-deletion-length K: shorter alleles are neither tested nor listed
    bool fuse_only = false;        // invoked as `fuse in.bam out.fasta` (doc/FUSE.md:26-31): the consensus and nothing else
    double ins_min_frac = 0.5;     // an insertion enters the consensus when more than this share of the covering reads carries it
    uint32_t ins_min_distance = 10;  // ... and the previous included insertion lies at least this many columns back (UNPINNED)
    bool timing = false;
    std::string exchange;            // --exchange rccl|inproc: how the rank threads exchange (default: rccl, inproc when a device repeats)
    // Sampling (docs/SPEC.md §12): the window is ingested whole, then replaced by chosen reads of it on the device (jl_msa_take)
    bool have_downsample = false;
    uint64_t downsample = 0;         // --downsample N: keep N reads (with --mix: the mixture's coverage, default 3000 as mixdata's COVERAGE)
    uint64_t sample_seed = 0;        // --sample-seed S (source m of a mixture is sampled with S + m)
    std::vector<std::string> mix;    // --mix b.bam[,c.bam...]: the minor clones; the positional BAM is the major one (doc/MIXDATA.md)
    double mix_perc = 1.0;           // --mix-perc P: percent of the mixture each minor clone gets
    bool sampling() const { return have_downsample || !mix.empty(); }
    // The read filter (docs/SPEC.md §20): per-read counters of the ingested window on the device, a rule over them on the host, the
    // kept reads gathered on the device (jl_msa_take) before --downsample
    jl_read_rule read_rule = {0u, 0xFFFFFFFFu, -1.0, -1.0, -1.0};   // every rule off
    uint32_t read_rule_set = 0;      // bit r: rule r (the order of jl_read_filter's failed[]) was given
    std::string read_stats_out;      // --read-stats out.tsv: the counters of every read of the loaded sample
    bool read_filter() const { return read_rule_set != 0 || !read_stats_out.empty(); }
    bool drop_hypermutated = false;  // --drop-hypermutated: drop the reads whose G->A test gives p < hypermut_alpha (docs/SPEC.md §26)
    bool have_hypermut_alpha = false;
    double hypermut_alpha = 0.05;    // Hypermut's
    std::string hypermut_report;     // --hypermut-report out.tsv: the counters and p of every read of the loaded sample
    bool hypermut() const { return drop_hypermutated || !hypermut_report.empty(); }
    bool drop_defective = false;     // --drop-defective: drop the reads with a premature stop, a frameshift or a large deletion in a gene (docs/SPEC.md §27)
    bool have_defect_option = false; // any --defect-* option was given
    uint32_t defect_kinds = 2u | 4u; // JL_ORF_STOP | JL_ORF_FRAMESHIFT: --defect-kinds
    uint32_t defect_max_deletion = 0;// --defect-max-deletion K: gap cells of a gene from which a read has the DELETION flag (0: off)
    uint32_t defect_tail_codons = 0; // --defect-tail-codons T: a stop in the last T codons of a gene is none
    std::string orf_report;          // --orf-report out.tsv: the counters and flags of every (read, gene) of the loaded sample
    bool orf() const { return drop_defective || !orf_report.empty(); }
    std::string control;             // --control control.bam: the codons are called against this sample's counts, not the error model (docs/SPEC.md §21)
    std::string batch;               // --batch samples.tsv: one `in.bam<TAB>out1[<TAB>out2]` per line, every other option for all of them
    struct BatchLine { unsigned line; std::string bam; std::vector<std::string> outputs; };
    std::vector<BatchLine> batch_lines;
};

[[noreturn]] void usage(int code)
{
    std::cerr <<
        "juliet " << kVersion << "\n"
        "usage: juliet [options] in.align.bam out.json|out.html [second output]\n"
        "       juliet [options] --batch samples.tsv\n"
        "  -c, --config <HIV|ABL1|file.json>   target config (doc/JULIET.md:109-180)\n"
        "  -p, --mode-phasing                  cluster reads into haplotypes (doc/JULIET.md:192-211)\n"
        "  -r, --region <begin-end>            1-based [begin,end) window of the config to call\n"
        "      --min-perc <x> / --max-perc <x> only calls above / below x percent\n"
        "  -k, --drm-only                      only known DRM positions of the config\n"
        "  parameters the reference text leaves open (docs/SPEC.md):\n"
        "      --alpha 0.01  --n-tests <auto>  --chemistry auto|sequel|permissive\n"
        "      --match-rate <r> --substitution-rate <r> --expected-round ceil|floor|nearest\n"
        "      --fisher-tail greater|two-sided  sidedness of Fisher's exact test (default greater: an excess of observed codons)\n"
        "      --min-reads 10  --min-qv 0  --min-rq 0  --device 0\n"
        "      --qv-upload mask|bytes          what --min-qv sends to the device: the filter decided while decoding, one bit per\n"
        "                                      base, or the folded qualities, one byte per base, and the threshold (default);\n"
        "                                      the same output\n"
        "      --windows K [--devices a,b,...] cut the reference into K column windows (2-column overlap, global Bonferroni\n"
        "                                      factor), consecutive windows per device; phasing runs across the windows with\n"
        "                                      the reads sharded over the devices.  The output is that of one window.\n"
        "      --exchange rccl|inproc          how the rank threads exchange: RCCL (default), or device copies between the ranks'\n"
        "                                      buffers (peer copies over xGMI; the default when a device is named twice,\n"
        "                                      which RCCL refuses)\n"
        "      --consensus <out.fasta>         also write the window's consensus as `fuse` would (doc/FUSE.md:17-20):\n"
        "                                      majority base, major deletions removed, in-frame majority insertions kept\n"
        "      --ins-min-frac 0.5  --ins-min-distance 10   when an insertion enters the consensus\n"
        "      --haplotype-mutations           with --mode-phasing: per reported haplotype every evaluated codon whose majority\n"
        "                                      within the haplotype differs from the reference (mutations[], drugs[]), a\n"
        "                                      drug_profile over the haplotypes, and per-haplotype counts on every variant codon\n"
        "                                      (docs/SPEC.md section 24).  Allowed and refused as --haplotype-fasta is\n"
        "      --haplotype-fasta <out.fasta>   with --mode-phasing: one consensus record per reported haplotype, in the JSON's\n"
        "                                      order, from the column pileup of that haplotype's reads alone (docs/SPEC.md section\n"
        "                                      13): majority base, major deletions removed, N where none of its reads covers the\n"
        "                                      column.  Insertions are not included (their counters are per window, not per\n"
        "                                      read).  Follows --downsample / --mix.  Not with --windows, --devices a,b, --batch\n"
        "                                      or as fuse\n"
        "      --rescue-damaged [--rescue-min-positions K]  with --mode-phasing: every damaged read (a deletion, a filtered N or an\n"
        "                                      uncovered cell at some variant position) is compared with the reported haplotypes at\n"
        "                                      the positions where it can be read, K of them at least (default 1; docs/SPEC.md\n"
        "                                      section 14): it is assigned to the one haplotype that agrees there, or counted as\n"
        "                                      ambiguous, incompatible or uninformative.  The haplotype block gains `rescue`, every\n"
        "                                      haplotype rescued_reads, rescued_read_names and frequency_with_rescued; with\n"
        "                                      --haplotype-fasta the rescued reads join their haplotype's consensus.  Follows\n"
        "                                      --downsample / --mix.  Not with --windows, --devices a,b, --batch or as fuse\n"
        "      --absorb-distance D [--absorb-min-positions K]  with --mode-phasing: every read phasing leaves out — with a pattern of\n"
        "                                      fewer than --min-reads reads (insufficient coverage), or damaged — is compared with\n"
        "                                      the reported haplotypes at the positions where it can be read, K of them at least\n"
        "                                      (default D + 1; docs/SPEC.md section 22): it is assigned to the haplotype it differs\n"
        "                                      from at the fewest codon positions, when that is one haplotype alone and D positions\n"
        "                                      (1 .. 7) at most; else it is ambiguous, distant or uninformative.  The haplotype\n"
        "                                      block gains `absorb`, every haplotype absorbed_reads, absorbed_damaged_reads,\n"
        "                                      absorbed_read_names and frequency_with_absorbed.  Independent of --rescue-damaged.\n"
        "                                      Follows --downsample / --mix.  Not with --windows, --devices a,b, --batch,\n"
        "                                      --phase-deletions, --phase-insertions or as fuse\n"
        "      --flag-recombinants [--recombinant-min-positions K] [--recombinant-parent-ratio r]  with --mode-phasing: flags the\n"
        "                                      products of PCR recombination (docs/SPEC.md section 23).  Every read phasing leaves\n"
        "                                      out that can be read at K positions at least (default 2) is a recombinant when one\n"
        "                                      reported haplotype agrees with it from the first position up to a breakpoint and\n"
        "                                      another from there to the last, and none agrees throughout; a reported haplotype is\n"
        "                                      a putative recombinant when two others with r times its reads at least (default 2)\n"
        "                                      cover it in that way.  The haplotype block gains `recombinants`, every haplotype\n"
        "                                      putative_recombinant (and recombinant_of).  Nothing is filtered.  Independent of\n"
        "                                      --rescue-damaged and --absorb-distance.  Follows --downsample / --mix.  Not with\n"
        "                                      --windows, --devices a,b, --batch, --phase-deletions, --phase-insertions or as fuse\n"
        "      --linkage                       pairwise linkage of the called variants over every read covering both (docs/SPEC.md\n"
        "                                      section 15), with and without --mode-phasing: read i is informative at a position iff\n"
        "                                      its three codes there are all < 4; it carries a variant iff it is informative at its\n"
        "                                      position and its codon there equals the variant's.  The JSON root gains `linkage`:\n"
        "                                      one entry per pair of variants at different positions with reads_both > 0 — the 2 x 2\n"
        "                                      table n11 n10 n01 n00 of the reads informative at both, r2, d_prime and the two\n"
        "                                      one-sided Fisher tests p_positive, p_negative, not Bonferroni-corrected\n"
        "                                      (n_pairs_tested is there to correct with).  At most 1024 variants at 1024 positions:\n"
        "                                      beyond, a warning and \"skipped\": true.  Follows --downsample / --mix.  Not with\n"
        "                                      --windows, --devices a,b, --batch or as fuse\n"
        "      --call-deletions                in-frame codon deletions (docs/SPEC.md section 16), with and without --mode-phasing:\n"
        "                                      at every evaluated codon position the reads whose three bases there are all\n"
        "                                      deleted are tested against the error model's deletion rate by the codon test's own\n"
        "                                      Fisher test, Bonferroni factor and --min-perc / --max-perc, over coverage = reads\n"
        "                                      with a whole codon + reads with the whole codon deleted.  Every gene of the JSON\n"
        "                                      gains `deletion_positions`: ref_position, ref_codon, ref_amino_acid, count,\n"
        "                                      coverage, frequency, expected, pValue, log_pValue and frameshift_reads (reads whose\n"
        "                                      deletion breaks the codon: not part of the test).  Empty with --drm-only.  Phasing\n"
        "                                      is unchanged.  Follows --downsample / --mix.  Not with --windows, --devices a,b,\n"
        "                                      --batch or as fuse\n"
        "      --phase-deletions               with --mode-phasing --call-deletions: the called deletions are sites of the\n"
        "                                      haplotypes (docs/SPEC.md section 18).  Phasing runs on a site matrix of the variant\n"
        "                                      positions and the called deletion positions: reads with the codon deleted carry the\n"
        "                                      allele instead of being damaged, a deletion at a position without a codon variant\n"
        "                                      splits the haplotypes that differ by it.  The haplotype block gains\n"
        "                                      deletion_positions_abs and every haplotype `deletions`; a codon prints --- where\n"
        "                                      the haplotype has it deleted; every deletion_positions entry gains haplotype_hit.\n"
        "                                      Not with --rescue-damaged, nor where --call-deletions is refused\n"
        "      --call-insertions [--insertion-rate r]  in-frame insertions by inserted sequence (docs/SPEC.md section 17), with and\n"
        "                                      without --mode-phasing: during the record ingest the device forms the distinct\n"
        "                                      (junction, length, sequence) among the reads whose insertion between two aligned\n"
        "                                      bases is 3 .. 30 bases long, a multiple of 3 and readable (A C G T past --min-qv), with\n"
        "                                      their read counts, and the reads spanning every junction.  Every allele in front of an\n"
        "                                      evaluated codon position (not a gene's first) is tested by the codon test's own Fisher\n"
        "                                      test, Bonferroni factor and --min-perc / --max-perc against r, the rate of in-frame\n"
        "                                      insertions by error (default: the chemistry's deletion rate), over coverage = reads\n"
        "                                      spanning the junction - frame-shifting - unreadable ones.  Every gene of the JSON gains\n"
        "                                      `insertion_positions`: after_position, inserted_codons, inserted_amino_acids, count,\n"
        "                                      coverage, frequency, expected, pValue, log_pValue, frameshift_reads, unread_reads.  An\n"
        "                                      insertion that splits a codon of a gene is not reported for it.  Empty with\n"
        "                                      --drm-only.  Not with --windows, --devices a,b, --batch, --downsample, --mix or as fuse\n"
        "      --phase-insertions              with --mode-phasing --call-insertions: the called insertion alleles are sites of the\n"
        "                                      haplotypes (docs/SPEC.md section 19), with and without --call-deletions\n"
        "                                      --phase-deletions.  The record ingest keeps which read carries which insertion; every\n"
        "                                      junction with a called allele is a site of the site matrix whose letters are its\n"
        "                                      called alleles, \"none\" and \"another in-frame insertion\"; reads with a frame-shifting\n"
        "                                      or unreadable insertion there are damaged.  The haplotype block gains\n"
        "                                      insertion_alleles (gene, after_position, inserted_codons) and every haplotype\n"
        "                                      `insertions`, a flag per allele; every insertion_positions entry gains haplotype_hit.\n"
        "                                      Not with --rescue-damaged, nor where --call-insertions is refused\n"
        "      --call-deletion-alleles [--deletion-allele-rate r] [--min-deletion-length K]  deletions by extent (docs/SPEC.md\n"
        "                                      section 25), with and without --mode-phasing: the device groups every read's maximal\n"
        "                                      runs of deleted bases by (start, length) over the whole window.  A run that touches the\n"
        "                                      window's edge or an uncovered base is open and is no allele.  Every allele of K bases\n"
        "                                      or more (default 1) is tested by the codon test's own Fisher test, Bonferroni factor\n"
        "                                      and --min-perc / --max-perc against r, the rate of one such deletion by error (default:\n"
        "                                      the chemistry's deletion rate), over coverage = the reads covering the base before and\n"
        "                                      the base after it.  The JSON root gains `deletion_alleles`: rate, min_length,\n"
        "                                      bounded_runs, open_runs, n_alleles, n_alleles_tested (to correct with) and one entry\n"
        "                                      per called allele: begin_abs, length, count, coverage, frequency, expected, pValue,\n"
        "                                      log_pValue, in_frame and the genes it overlaps (first_position, last_position,\n"
        "                                      codon_aligned).  Follows --downsample / --mix.  Not with --windows, --devices a,b,\n"
        "                                      --batch, --control or as fuse\n"
        "      --downsample N [--sample-seed S]  call on N reads of the sample (\"downsample it to 6000x\", doc/JULIETFLOW.md:23-25):\n"
        "                                      the reads are chosen by docs/SPEC.md section 12 (seed default 0; samples of one seed are\n"
        "                                      nested) and gathered on the device; N at or above the read count changes nothing.\n"
        "                                      With --batch: every sample.  Not with --windows, --devices a,b or --consensus\n"
        "      --min-read-bases K  --max-read-mismatches K  --max-read-mismatch-perc x  --max-read-gap-perc x  --max-read-n-perc x\n"
        "                                      the read filter (docs/SPEC.md section 20): the device counts, per read over the whole\n"
        "                                      window, its bases, gaps, N cells, the bases in compared columns and the mismatches\n"
        "                                      among those; a read is kept when bases >= K, mismatches <= K, 100 mismatches <= x\n"
        "                                      compared, 100 gaps <= x (bases + gaps), 100 N <= x (bases + gaps + N), for every rule\n"
        "                                      given.  The compare row is the config's referenceSequence over the window, else the\n"
        "                                      majority consensus of the unfiltered window.  The kept reads are gathered on the\n"
        "                                      device; --downsample then samples them.  The JSON gains input.read_filter.  No read\n"
        "                                      kept is an input error (2).  With --batch: every sample.  Not with --windows,\n"
        "                                      --devices a,b, --consensus, --mix, --call-insertions or as fuse\n"
        "      --read-stats <out.tsv>          name, bases, gaps, masked, compared, mismatches of every read of the loaded sample,\n"
        "                                      tab-separated, in input order, before any filter; needs no rule.  Refused where the\n"
        "                                      read filter is, and with --batch\n"
        "      --drop-hypermutated [--hypermut-alpha a]  drop APOBEC-hypermutated reads (docs/SPEC.md section 26): the device counts,\n"
        "                                      per read, its G->A sites in the target context GRD and in the control contexts\n"
        "                                      GYN / GRC, taken from the read's own two cells downstream, and tests the two one-sided\n"
        "                                      (Fisher, as Hypermut 2.0); a read with p < a (default 0.05) is dropped.  G is the\n"
        "                                      config's referenceSequence over the window, else the majority consensus.  After the\n"
        "                                      read filter, before --downsample.  The JSON gains input.hypermutation.  No read kept is\n"
        "                                      an input error (2).  With --batch: every sample.  Refused where the read filter is\n"
        "      --hypermut-report <out.tsv>     name, target_sites, target_mut, control_sites, control_mut, p of every read of the\n"
        "                                      loaded sample, tab-separated, in input order; needs no --drop-hypermutated.  Refused\n"
        "                                      where the read filter is, and with --batch\n"
        "      --drop-defective [--defect-kinds stop,frameshift,deletion] [--defect-max-deletion K] [--defect-tail-codons T]\n"
        "                                      drop reads whose reading frame is broken in any gene (docs/SPEC.md section 27): the device\n"
        "                                      counts, per read and gene of the config (without one: the one `unknown` gene), covered\n"
        "                                      cells, gap cells, codons read and stop codons the reference row does not have.  stop: a\n"
        "                                      stop before the gene's last T codons (default 0); frameshift: gap cells not a multiple\n"
        "                                      of 3; deletion: K gap cells or more (needs K).  Default kinds: stop,frameshift.  After\n"
        "                                      --drop-hypermutated, before --downsample.  The JSON gains input.orf_integrity.  No read\n"
        "                                      kept is an input error (2).  With --batch: every sample.  Refused where the read filter is\n"
        "      --orf-report <out.tsv>          name, gene, covered, gap_cells, codons_read, stops, first_stop, flags (P S F D) of every\n"
        "                                      read and gene of the loaded sample, tab-separated, reads in input order, genes in config\n"
        "                                      order; needs no --drop-defective.  Refused where the read filter is, and with --batch\n"
        "      --mix b.bam[,c.bam...] [--mix-perc P]  a mixture as mixdata makes it (doc/MIXDATA.md): in.bam is the major clone, every\n"
        "                                      listed BAM a minor clone with P percent (default 1) of --downsample C reads (default\n"
        "                                      3000); source m is sampled with seed S + m.  A source with too few reads is an input\n"
        "                                      error (2).  Not with --batch, --windows, --devices a,b or --consensus\n"
        "      --control <control.bam>         call the codons against a control sample instead of the error model (docs/SPEC.md\n"
        "                                      section 21): the control is loaded as in.bam is (--min-qv, --min-rq, --region, the read\n"
        "                                      filter) over the same window, and every codon is tested one-sided by Fisher's exact\n"
        "                                      test on its counts in the sample and in the control, times the Bonferroni factor.\n"
        "                                      --min-perc, --max-perc and --drm-only act on the sample's frequency; --downsample\n"
        "                                      samples in.bam only; --mode-phasing phases the control-called table.  The JSON gains\n"
        "                                      input.control and, per variant codon, control_count (also `expected`),\n"
        "                                      control_coverage and control_frequency.  Refused with exit status 2: --windows,\n"
        "                                      --devices a,b, --batch, --mix, --call-deletions, --call-insertions, --fisher-tail\n"
        "                                      two-sided, and as fuse\n"
        "      --batch <samples.tsv>           many samples in one process: one `in.bam<TAB>out1[<TAB>out2]` per line (blank lines\n"
        "                                      and lines starting with # skipped); every other option applies to every sample and\n"
        "                                      each sample gets the files a single run would write.  A sample that fails is named\n"
        "                                      on stderr and the others go on (exit status 2 if any failed); a GPU error stops\n"
        "                                      the batch (3).  Not with --windows, --devices a,b, --consensus or --dump-*\n"
        "      --timing                        wall time of each stage on stderr\n"
        "  diagnostics (no GPU needed): --dump-msa <file>  --dump-config <file>\n";
    std::exit(code);
}

bool output_kind_ok(const std::string &out)   // the outputs are told apart by their extension (doc/JULIET.md:61-66)
{
    return out.size() > 5 && (out.substr(out.size() - 5) == ".json" || out.substr(out.size() - 5) == ".html");
}

// The --batch list: `in.bam<TAB>out1[<TAB>out2 ...]` per line; blank lines and lines starting with # are skipped.  Anything
// wrong with it ends the process with status 1 before any BAM is read.
std::vector<Options::BatchLine> read_batch_list(const std::string &path)
{
    auto bad = [&](unsigned line, const std::string &why) {
        std::cerr << "juliet: --batch " << path;
        if (line) std::cerr << " line " << line;
        std::cerr << ": " << why << "\n";
        std::exit(1);
    };
    std::error_code ec;
    if (std::filesystem::is_directory(path, ec)) bad(0, "is a directory");
    std::ifstream f(path);
    if (!f) bad(0, "cannot be read");
    std::vector<Options::BatchLine> lines;
    std::map<std::string, unsigned> written;   // output path (absolute, normalised) -> the line that names it
    std::string text;
    unsigned no = 0;
    while (std::getline(f, text)) {
        ++no;
        if (!text.empty() && text.back() == '\r') text.pop_back();
        if (text.find_first_not_of(" \t") == std::string::npos || text[0] == '#') continue;
        std::vector<std::string> fields;
        for (size_t b = 0;;) {
            const size_t e = text.find('\t', b);
            fields.push_back(text.substr(b, e == std::string::npos ? std::string::npos : e - b));
            if (e == std::string::npos) break;
            b = e + 1;
        }
        if (fields.size() < 2) bad(no, "wants an input BAM and at least one output, separated by tabs");
        for (const std::string &fld : fields)
            if (fld.empty()) bad(no, "has an empty field");
        Options::BatchLine l{no, fields[0], std::vector<std::string>(fields.begin() + 1, fields.end())};
        for (const std::string &out : l.outputs) {
            if (!output_kind_ok(out)) bad(no, "output '" + out + "' must end in .json or .html (doc/JULIET.md:61-66)");
            const std::string key = std::filesystem::absolute(out, ec).lexically_normal().string();
            const auto it = written.find(key);
            if (it != written.end())
                bad(no, "output '" + out + "' is also written by line " + std::to_string(it->second) + " (every output once)");
            written.emplace(key, no);
        }
        lines.push_back(std::move(l));
    }
    if (f.bad()) bad(0, "cannot be read");
    if (lines.empty()) bad(0, "names no sample");
    return lines;
}

Options parse(int argc, char **argv)
{
    Options o;
    auto need = [&](int &i) -> std::string {
        if (i + 1 >= argc) { std::cerr << "juliet: " << argv[i] << " needs a value\n"; usage(1); }
        return argv[++i];
    };
    std::vector<std::string> pos;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "-h" || a == "--help") usage(0);
        else if (a == "--version") { std::cout << kVersion << "\n"; std::exit(0); }
        else if (a == "-c" || a == "--config") o.config = need(i);
        else if (a == "-p" || a == "--mode-phasing") o.phasing = true;
        else if (a == "-k" || a == "--drm-only") o.drm_only = true;
        else if (a == "-r" || a == "--region") {
            const std::string v = need(i);
            const size_t d = v.find('-');
            if (d == std::string::npos) { std::cerr << "juliet: --region wants begin-end\n"; usage(1); }
            o.region_b = (uint32_t)std::stoul(v.substr(0, d));
            o.region_e = (uint32_t)std::stoul(v.substr(d + 1));
            o.have_region = true;
        }
        else if (a == "--min-perc") o.min_perc = std::stod(need(i));
        else if (a == "--max-perc") o.max_perc = std::stod(need(i));
        else if (a == "--alpha") o.alpha = std::stod(need(i));
        else if (a == "--n-tests") o.n_tests = std::stod(need(i));
        else if (a == "--chemistry") o.chemistry = need(i);
        else if (a == "--match-rate") o.match = std::stod(need(i));
        else if (a == "--substitution-rate") o.substitution = std::stod(need(i));
        else if (a == "--expected-round") {
            const std::string v = need(i);
            o.expected_round = v == "floor" ? 1 : v == "nearest" ? 2 : 0;
        }
        else if (a == "--fisher-tail") {
            const std::string v = need(i);
            if (v == "greater") o.fisher_tail = 0;
            else if (v == "two-sided") o.fisher_tail = 1;
            else { std::cerr << "juliet: --fisher-tail takes greater or two-sided\n"; usage(1); }
        }
        else if (a == "--min-reads") o.min_reads = (uint32_t)std::stoul(need(i));
        else if (a == "--min-qv") o.min_qv = (uint32_t)std::stoul(need(i));
        else if (a == "--qv-upload") {
            const std::string v = need(i);
            if (v != "mask" && v != "bytes") { std::cerr << "juliet: --qv-upload takes mask or bytes\n"; usage(1); }
            o.qv_upload_mask = v == "mask";
        }
        else if (a == "--min-rq") o.min_rq = std::stod(need(i));
        else if (a == "--device") o.device = std::stoi(need(i));
        else if (a == "--windows") o.windows = (uint32_t)std::stoul(need(i));
        else if (a == "--exchange") {
            o.exchange = need(i);
            if (o.exchange != "rccl" && o.exchange != "inproc") { std::cerr << "juliet: --exchange wants rccl or inproc\n"; usage(1); }
        }
        else if (a == "--devices") {
            const std::string v = need(i);
            size_t b = 0;
            while (b <= v.size()) {
                const size_t e = std::min(v.find(',', b), v.size());
                if (e > b) o.devices.push_back(std::stoi(v.substr(b, e - b)));
                b = e + 1;
            }
        }
        else if (a == "--consensus") o.consensus = need(i);
        else if (a == "--haplotype-fasta") o.hap_fasta = need(i);
        else if (a == "--haplotype-mutations") o.hap_mutations = true;
        else if (a == "--rescue-damaged") o.rescue = true;
        else if (a == "--linkage") o.linkage = true;
        else if (a == "--call-deletions") o.call_deletions = true;
        else if (a == "--phase-deletions") o.phase_deletions = true;
        else if (a == "--phase-insertions") o.phase_insertions = true;
        else if (a == "--call-insertions") o.call_insertions = true;
        else if (a == "--insertion-rate") {
            const std::string v = need(i);
            char *end = nullptr;
            o.insertion_rate = std::strtod(v.c_str(), &end);
            o.have_insertion_rate = true;
            if (v.empty() || *end || !(o.insertion_rate >= 0.0 && o.insertion_rate <= 1.0)) {
                std::cerr << "juliet: --insertion-rate wants a probability in [0, 1], not '" << v << "'\n";
                std::exit(1);
            }
        }
        else if (a == "--call-deletion-alleles") o.call_deletion_alleles = true;
        else if (a == "--deletion-allele-rate") {
            const std::string v = need(i);
            char *end = nullptr;
            o.deletion_allele_rate = std::strtod(v.c_str(), &end);
            o.have_deletion_allele_rate = true;
            if (v.empty() || *end || !(o.deletion_allele_rate >= 0.0 && o.deletion_allele_rate <= 1.0)) {
                std::cerr << "juliet: --deletion-allele-rate wants a probability in [0, 1], not '" << v << "'\n";
                std::exit(1);
            }
        }
        else if (a == "--min-deletion-length") {
            const std::string v = need(i);
            char *end = nullptr;
            const unsigned long long k = std::strtoull(v.c_str(), &end, 10);
            o.have_min_deletion_length = true;
            if (v.empty() || *end || v[0] == '-' || k == 0 || k > 0xFFFFFFFFull) {
                std::cerr << "juliet: --min-deletion-length wants a length of 1 base or more, not '" << v << "'\n";
                std::exit(1);
            }
            o.min_deletion_length = (uint32_t)k;
        }
        else if (a == "--rescue-min-positions") { o.rescue_min = (uint32_t)std::stoul(need(i)); o.have_rescue_min = true; }
        else if (a == "--absorb-distance") { o.absorb_distance = (uint32_t)std::stoul(need(i)); o.have_absorb = true; }
        else if (a == "--flag-recombinants") o.flag_recombinants = true;
        else if (a == "--recombinant-min-positions") { o.recomb_min = (uint32_t)std::stoul(need(i)); o.have_recomb_min = true; }
        else if (a == "--recombinant-parent-ratio") { o.recomb_ratio = std::stod(need(i)); o.have_recomb_ratio = true; }
        else if (a == "--absorb-min-positions") { o.absorb_min = (uint32_t)std::stoul(need(i)); o.have_absorb_min = true; }
        else if (a == "--ins-min-frac") o.ins_min_frac = std::stod(need(i));
        else if (a == "--ins-min-distance") o.ins_min_distance = (uint32_t)std::stoul(need(i));
        else if (a == "--dump-msa") o.dump_msa = need(i);
        else if (a == "--dump-config") o.dump_config = need(i);
        else if (a == "--timing") o.timing = true;
        else if (a == "--batch") o.batch = need(i);
        else if (a == "--downsample") { o.downsample = std::stoull(need(i)); o.have_downsample = true; }
        else if (a == "--sample-seed") o.sample_seed = std::stoull(need(i));
        else if (a == "--mix") {
            const std::string v = need(i);
            for (size_t b = 0; b <= v.size();) {
                const size_t e = std::min(v.find(',', b), v.size());
                if (e > b) o.mix.push_back(v.substr(b, e - b));
                b = e + 1;
            }
            if (o.mix.empty()) { std::cerr << "juliet: --mix names no BAM\n"; std::exit(1); }
        }
        else if (a == "--mix-perc") o.mix_perc = std::stod(need(i));
        else if (a == "--min-read-bases") { o.read_rule.min_bases = (uint32_t)std::stoul(need(i)); o.read_rule_set |= 1u; }
        else if (a == "--max-read-mismatches") { o.read_rule.max_mismatches = (uint32_t)std::stoul(need(i)); o.read_rule_set |= 2u; }
        else if (a == "--max-read-mismatch-perc" || a == "--max-read-gap-perc" || a == "--max-read-n-perc") {
            const std::string v = need(i);
            char *end = nullptr;
            const double x = std::strtod(v.c_str(), &end);
            if (v.empty() || *end || !(x >= 0.0 && x <= 100.0)) { std::cerr << "juliet: " << a << " wants a percentage in [0, 100], not '" << v << "'\n"; std::exit(1); }
            if (a == "--max-read-mismatch-perc") o.read_rule.max_mismatch_perc = x, o.read_rule_set |= 4u;
            else if (a == "--max-read-gap-perc") o.read_rule.max_gap_perc = x, o.read_rule_set |= 8u;
            else o.read_rule.max_masked_perc = x, o.read_rule_set |= 16u;
        }
        else if (a == "--read-stats") o.read_stats_out = need(i);
        else if (a == "--drop-hypermutated") o.drop_hypermutated = true;
        else if (a == "--hypermut-alpha") {
            const std::string v = need(i);
            char *end = nullptr;
            const double x = std::strtod(v.c_str(), &end);
            if (v.empty() || *end || !(x > 0.0 && x <= 1.0)) { std::cerr << "juliet: --hypermut-alpha wants a level in (0, 1], not '" << v << "'\n"; std::exit(1); }
            o.hypermut_alpha = x, o.have_hypermut_alpha = true;
        }
        else if (a == "--hypermut-report") o.hypermut_report = need(i);
        else if (a == "--drop-defective") o.drop_defective = true;
        else if (a == "--orf-report") o.orf_report = need(i);
        else if (a == "--defect-kinds") {
            const std::string v = need(i);
            o.have_defect_option = true;
            o.defect_kinds = 0;
            for (size_t b = 0; b <= v.size();) {
                const size_t e = std::min(v.find(',', b), v.size());
                const std::string kind = v.substr(b, e - b);
                const uint32_t bit = kind == "stop" ? 2u : kind == "frameshift" ? 4u : kind == "deletion" ? 8u : 0u;   // JL_ORF_STOP, _FRAMESHIFT, _DELETION
                if (!bit) { std::cerr << "juliet: --defect-kinds wants a list of stop, frameshift, deletion, not '" << v << "'\n"; std::exit(1); }
                o.defect_kinds |= bit;
                b = e + 1;
            }
        }
        else if (a == "--defect-max-deletion" || a == "--defect-tail-codons") {
            const bool tail = a == "--defect-tail-codons";
            const std::string v = need(i);
            char *end = nullptr;
            const unsigned long long k = std::strtoull(v.c_str(), &end, 10);
            o.have_defect_option = true;
            if (v.empty() || *end || v[0] == '-' || (!tail && k == 0) || k > 0xFFFFFFFFull) {
                std::cerr << "juliet: " << a << (tail ? " wants a number of codons, not '" : " wants 1 gap cell or more, not '") << v << "'\n";
                std::exit(1);
            }
            (tail ? o.defect_tail_codons : o.defect_max_deletion) = (uint32_t)k;
        }
        else if (a == "--control") o.control = need(i);
        else if (!a.empty() && a[0] == '-') { std::cerr << "juliet: unknown option " << a << "\n"; usage(1); }
        else pos.push_back(a);
    }
    const std::string prog = argv[0];
    const size_t slash = prog.find_last_of('/');
    const bool as_fuse = (slash == std::string::npos ? prog : prog.substr(slash + 1)) == "fuse";
    if (!o.hap_fasta.empty()) {   // refused here, before any file is read or any GPU work
        auto refuse = [](const char *why) { std::cerr << "juliet: --haplotype-fasta " << why << "\n"; std::exit(1); };
        if (as_fuse) refuse("is not an option of fuse");
        if (!o.phasing) refuse("writes the haplotypes of a phasing run (add --mode-phasing)");
        if (o.windows > 1 || o.devices.size() > 1) refuse("works on one window of one device (drop --windows / --devices a,b)");
        if (!o.batch.empty()) refuse("writes one file for one sample (not with --batch)");
    }
    if (o.hap_mutations) {   // refused as --haplotype-fasta is, before any file is read or any GPU work
        auto refuse = [](const char *why) { std::cerr << "juliet: --haplotype-mutations " << why << "\n"; std::exit(1); };
        if (as_fuse) refuse("is not an option of fuse");
        if (!o.phasing) refuse("describes the haplotypes of a phasing run (add --mode-phasing)");
        if (o.windows > 1 || o.devices.size() > 1) refuse("works on one window of one device (drop --windows / --devices a,b)");
        if (!o.batch.empty()) refuse("describes one sample (not with --batch)");
    }
    if (o.rescue || o.have_rescue_min) {   // refused here, before any file is read or any GPU work
        auto refuse = [](const char *why) { std::cerr << "juliet: --rescue-damaged [--rescue-min-positions K] " << why << "\n"; std::exit(1); };
        if (!o.rescue) refuse("--rescue-min-positions sets a threshold of --rescue-damaged (add it)");
        if (o.rescue_min == 0) refuse("wants at least one informative position (--rescue-min-positions 0)");
        if (as_fuse) refuse("are not options of fuse");
        if (!o.phasing) refuse("assigns reads to the haplotypes of a phasing run (add --mode-phasing)");
        if (o.windows > 1 || o.devices.size() > 1) refuse("works on one window of one device (drop --windows / --devices a,b)");
        if (!o.batch.empty()) refuse("is not part of a batch (not with --batch)");
    }
    if (o.have_absorb || o.have_absorb_min) {   // refused here, before any file is read or any GPU work
        auto refuse = [](const char *why) { std::cerr << "juliet: --absorb-distance D [--absorb-min-positions K] " << why << "\n"; std::exit(1); };
        if (!o.have_absorb) refuse("--absorb-min-positions sets a threshold of --absorb-distance (add it)");
        if (o.absorb_distance == 0 || o.absorb_distance > (uint32_t)JL_NEAREST_MAX_DISTANCE) refuse("wants a budget D of 1 to 7 codon positions");
        if (o.have_absorb_min && o.absorb_min == 0) refuse("wants at least one informative position (--absorb-min-positions 0)");
        if (as_fuse) refuse("are not options of fuse");
        if (!o.phasing) refuse("assigns reads to the haplotypes of a phasing run (add --mode-phasing)");
        if (o.windows > 1 || o.devices.size() > 1) refuse("works on one window of one device (drop --windows / --devices a,b)");
        if (!o.batch.empty()) refuse("is not part of a batch (not with --batch)");
        if (o.phase_deletions || o.phase_insertions) refuse("measures distances in codons; the sites of --phase-deletions / --phase-insertions are none (drop them)");
        if (!o.have_absorb_min) o.absorb_min = o.absorb_distance + 1u;
    }
    if (o.flag_recombinants || o.have_recomb_min || o.have_recomb_ratio) {   // refused here, before any file is read or any GPU work
        auto refuse = [](const char *why) {
            std::cerr << "juliet: --flag-recombinants [--recombinant-min-positions K] [--recombinant-parent-ratio r] " << why << "\n";
            std::exit(1);
        };
        if (!o.flag_recombinants) refuse("--recombinant-min-positions and --recombinant-parent-ratio set thresholds of --flag-recombinants (add it)");
        if (o.recomb_min == 0) refuse("wants at least one informative position (--recombinant-min-positions 0)");
        if (!(o.recomb_ratio >= 1.0)) refuse("wants a parent with as many reads as the haplotype at least (--recombinant-parent-ratio below 1)");
        if (as_fuse) refuse("are not options of fuse");
        if (!o.phasing) refuse("looks for recombinants of the haplotypes of a phasing run (add --mode-phasing)");
        if (o.windows > 1 || o.devices.size() > 1) refuse("works on one window of one device (drop --windows / --devices a,b)");
        if (!o.batch.empty()) refuse("is not part of a batch (not with --batch)");
        if (o.phase_deletions || o.phase_insertions) refuse("compares codons; the sites of --phase-deletions / --phase-insertions are none (drop them)");
    }
    if (o.linkage) {   // refused here, before any file is read or any GPU work
        auto refuse = [](const char *why) { std::cerr << "juliet: --linkage " << why << "\n"; std::exit(1); };
        if (as_fuse) refuse("is not an option of fuse");
        if (o.windows > 1 || o.devices.size() > 1) refuse("works on one window of one device (drop --windows / --devices a,b)");
        if (!o.batch.empty()) refuse("is not part of a batch (not with --batch)");
    }
    if (o.call_deletions) {   // refused here, before any file is read or any GPU work
        auto refuse = [](const char *why) { std::cerr << "juliet: --call-deletions " << why << "\n"; std::exit(1); };
        if (as_fuse) refuse("is not an option of fuse");
        if (o.windows > 1 || o.devices.size() > 1) refuse("works on one window of one device (drop --windows / --devices a,b)");
        if (!o.batch.empty()) refuse("is not part of a batch (not with --batch)");
    }
    if (o.phase_deletions) {   // refused here, before any file is read or any GPU work
        auto refuse = [](const char *why) { std::cerr << "juliet: --phase-deletions " << why << "\n"; std::exit(1); };
        if (as_fuse) refuse("is not an option of fuse");
        if (!o.phasing) refuse("adds sites to the haplotypes of a phasing run (add --mode-phasing)");
        if (!o.call_deletions) refuse("phases the deletions that --call-deletions calls (add it)");
        if (o.rescue) refuse("leaves no deletion for --rescue-damaged to judge as damage (drop one of the two)");
    }
    if (o.call_insertions || o.have_insertion_rate) {   // refused here, before any file is read or any GPU work
        auto refuse = [](const char *why) { std::cerr << "juliet: --call-insertions [--insertion-rate r] " << why << "\n"; std::exit(1); };
        if (!o.call_insertions) refuse("--insertion-rate sets the error rate of --call-insertions (add it)");
        if (as_fuse) refuse("are not options of fuse");
        if (o.windows > 1 || o.devices.size() > 1) refuse("works on one window of one device (drop --windows / --devices a,b)");
        if (!o.batch.empty()) refuse("is not part of a batch (not with --batch)");
        if (o.sampling()) refuse("reads the insertions of the records that were ingested, not of a sample of them (drop --downsample / --mix)");
        if (o.read_filter()) refuse("reads the insertions of the records that were ingested, not of the reads a filter keeps (drop the read filter / --read-stats)");
        if (o.hypermut() || o.have_hypermut_alpha) refuse("reads the insertions of the records that were ingested, not of the reads a filter keeps (drop --drop-hypermutated / --hypermut-report)");
        if (o.orf() || o.have_defect_option) refuse("reads the insertions of the records that were ingested, not of the reads a filter keeps (drop --drop-defective / --orf-report)");
    }
    if (o.phase_insertions) {   // refused here, before any file is read or any GPU work (what --call-insertions refuses: above)
        auto refuse = [](const char *why) { std::cerr << "juliet: --phase-insertions " << why << "\n"; std::exit(1); };
        if (as_fuse) refuse("is not an option of fuse");
        if (!o.phasing) refuse("adds sites to the haplotypes of a phasing run (add --mode-phasing)");
        if (!o.call_insertions) refuse("phases the insertions that --call-insertions calls (add it)");
        if (o.rescue) refuse("leaves no insertion for --rescue-damaged to judge as damage (drop one of the two)");
    }
    if (o.call_deletion_alleles || o.have_deletion_allele_rate || o.have_min_deletion_length) {   // refused here, before any file is read or any GPU work
        auto refuse = [](const char *why) {
            std::cerr << "juliet: --call-deletion-alleles [--deletion-allele-rate r] [--min-deletion-length K] " << why << "\n";
            std::exit(1);
        };
        if (!o.call_deletion_alleles) refuse("--deletion-allele-rate and --min-deletion-length set the test of --call-deletion-alleles (add it)");
        if (as_fuse) refuse("are not options of fuse");
        if (o.windows > 1 || o.devices.size() > 1) refuse("works on one window of one device (drop --windows / --devices a,b)");
        if (!o.batch.empty()) refuse("is not part of a batch (not with --batch)");
        if (!o.control.empty()) refuse("tests against the error model, not a control (drop --control)");
    }
    if (!o.control.empty()) {   // refused here, before any file is read or any GPU work
        auto refuse = [](const char *why) { std::cerr << "juliet: --control " << why << "\n"; std::exit(2); };
        if (as_fuse) refuse("is not an option of fuse");
        if (o.windows > 1 || o.devices.size() > 1) refuse("works on one window of one device (drop --windows / --devices a,b)");
        if (!o.batch.empty()) refuse("is the control of one sample (not with --batch)");
        if (!o.mix.empty()) refuse("tests a sample, not a mixture made for the error model (drop --mix)");
        if (o.call_deletions || o.call_insertions) refuse("calls codons; deletions and insertions are tested against the error model only (drop --call-deletions / --call-insertions)");
        if (o.fisher_tail != 0) refuse("tests an excess over the control, one-sided (drop --fisher-tail two-sided)");
    }
    if (o.read_filter()) {   // refused here, before any file is read or any GPU work: what --downsample refuses, and --mix
        auto refuse = [](const char *why) { std::cerr << "juliet: the read filter (--min-read-bases, --max-read-*, --read-stats) " << why << "\n"; std::exit(1); };
        if (as_fuse) refuse("is not an option of fuse");
        if (o.windows > 1 || o.devices.size() > 1) refuse("works on one window of one device (drop --windows / --devices a,b)");
        if (!o.consensus.empty()) refuse("carries no insertion counters into the kept reads: no consensus (drop --consensus)");
        if (!o.mix.empty()) refuse("filters one sample, not the sources of a mixture (drop --mix)");
        if (!o.batch.empty() && !o.read_stats_out.empty()) refuse("writes one --read-stats file for one sample (not with --batch)");
    }
    if (o.hypermut() || o.have_hypermut_alpha) {   // refused here, before any file is read or any GPU work: what the read filter refuses
        auto refuse = [](const char *why) { std::cerr << "juliet: the hypermutation filter (--drop-hypermutated, --hypermut-alpha, --hypermut-report) " << why << "\n"; std::exit(1); };
        if (!o.drop_hypermutated && o.have_hypermut_alpha) refuse("--hypermut-alpha sets the level of --drop-hypermutated (add it)");
        if (as_fuse) refuse("is not an option of fuse");
        if (o.windows > 1 || o.devices.size() > 1) refuse("works on one window of one device (drop --windows / --devices a,b)");
        if (!o.consensus.empty()) refuse("carries no insertion counters into the kept reads: no consensus (drop --consensus)");
        if (!o.mix.empty()) refuse("filters one sample, not the sources of a mixture (drop --mix)");
        if (!o.batch.empty() && !o.hypermut_report.empty()) refuse("writes one --hypermut-report file for one sample (not with --batch)");
    }
    if (o.orf() || o.have_defect_option) {   // refused here, before any file is read or any GPU work: what the hypermutation filter refuses
        auto refuse = [](const char *why) { std::cerr << "juliet: the reading-frame filter (--drop-defective, --defect-*, --orf-report) " << why << "\n"; std::exit(1); };
        if (!o.drop_defective && o.have_defect_option) refuse("--defect-kinds, --defect-max-deletion and --defect-tail-codons are the rule of --drop-defective (add it)");
        if ((o.defect_kinds & 8u) && o.defect_max_deletion == 0) refuse("kind deletion needs its bound (add --defect-max-deletion K)");
        if (as_fuse) refuse("is not an option of fuse");
        if (o.windows > 1 || o.devices.size() > 1) refuse("works on one window of one device (drop --windows / --devices a,b)");
        if (!o.consensus.empty()) refuse("carries no insertion counters into the kept reads: no consensus (drop --consensus)");
        if (!o.mix.empty()) refuse("filters one sample, not the sources of a mixture (drop --mix)");
        if (!o.batch.empty() && !o.orf_report.empty()) refuse("writes one --orf-report file for one sample (not with --batch)");
    }
    if (o.sampling()) {   // what sampling cannot be combined with is refused here, before any file is read or any GPU work
        auto refuse = [&](const char *why) { std::cerr << "juliet: " << (o.mix.empty() ? "--downsample " : "--mix ") << why << "\n"; std::exit(1); };
        if (o.have_downsample && o.downsample == 0) refuse("wants at least one read (--downsample 0)");
        if (o.windows > 1 || o.devices.size() > 1) refuse("works on one window of one device (drop --windows / --devices a,b)");
        if (!o.consensus.empty() || as_fuse) refuse("carries no insertion counters into the sample: no consensus (drop --consensus)");
        if (!o.mix.empty()) {
            if (!o.batch.empty()) refuse("mixes into one sample (not with --batch)");
            if (o.mix.size() + 1 > (size_t)JL_TAKE_MAX_PARTS) refuse("takes at most 15 minor clones");
            if (!o.have_downsample) o.downsample = 3000;   // mixdata's COVERAGE (doc/MIXDATA.md)
            std::vector<uint64_t> counts(o.mix.size() + 1);
            if (jl_mix_counts((uint32_t)counts.size(), o.downsample, o.mix_perc, counts.data()) != JL_OK)
                refuse("wants --mix-perc inside (0, 100) and minor clones that together stay within the coverage");
        }
    }
    if (!o.batch.empty()) {   // everything a batch cannot do is refused here, before any file is read or any GPU work
        auto refuse = [](const char *why) { std::cerr << "juliet: --batch " << why << "\n"; std::exit(1); };
        if (as_fuse) refuse("is not an option of fuse");
        if (!pos.empty()) refuse("takes no input BAM or outputs on the command line: they are the lines of the list");
        if (o.windows > 1) refuse("runs one window per sample (drop --windows)");
        if (o.devices.size() > 1) refuse("runs on one device (--device, not a --devices list)");
        if (!o.consensus.empty()) refuse("writes no consensus (drop --consensus)");
        if (!o.dump_msa.empty() || !o.dump_config.empty()) refuse("does not combine with --dump-msa or --dump-config");
        if (!o.devices.empty()) o.device = o.devices[0];
        o.devices.assign(1, o.device);
        o.batch_lines = read_batch_list(o.batch);
        return o;
    }
    if (!o.dump_config.empty() && pos.empty()) { if (o.devices.empty()) o.devices.push_back(o.device); return o; }
    {   // `fuse in.bam out.fasta` (doc/FUSE.md:26-31): the same front end, asked for the consensus only
        if (as_fuse) {
            if (pos.size() != 2) { std::cerr << "fuse: usage: fuse in.align.bam out.fasta\n"; std::exit(1); }
            o.bam = pos[0];
            o.consensus = pos[1];
            o.fuse_only = true;
            o.devices.assign(1, o.device);
            o.windows = 1;
            return o;
        }
    }
    if (o.devices.empty()) o.devices.push_back(o.device);
    if (o.windows == 0 || o.windows > 32u * o.devices.size()) { std::cerr << "juliet: --windows wants 1 .. 32 per device\n"; usage(1); }
    if (o.windows < o.devices.size()) { std::cerr << "juliet: fewer windows than devices\n"; usage(1); }
    if ((o.windows > 1 || o.devices.size() > 1) && !o.consensus.empty()) {
        std::cerr << "juliet: --consensus works on one window (drop --windows / --devices)\n";
        usage(1);
    }
    if (pos.size() < 2 && o.dump_msa.empty()) { std::cerr << "juliet: need an input BAM and at least one output\n"; usage(1); }
    if (pos.empty()) usage(1);
    o.bam = pos[0];
    o.outputs.assign(pos.begin() + 1, pos.end());
    for (const std::string &out : o.outputs) {
        if (!output_kind_ok(out)) { std::cerr << "juliet: output '" << out << "' must end in .json or .html (doc/JULIET.md:61-66)\n"; usage(1); }
    }
    return o;
}

}  // namespace
}  // namespace jlhost
