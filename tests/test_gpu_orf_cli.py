"""The front end's reading-frame filter (docs/SPEC.md §27): --orf-report, --drop-defective [--defect-kinds, --defect-max-deletion,
--defect-tail-codons], the JSON's input.orf_integrity block and its HTML tables, its place after --drop-hypermutated, and --batch.
The BAMs are written by the suite's independent writer (tests/bam_py.py): a few hundred reads over a reference with two overlapping
genes in different frames, chosen reads carrying a premature stop, a 1-base deletion, a -1/-2 pair of deletions, a 3-base deletion,
a stop in a gene's last codon, or APOBEC-style G->A edits.  Every expectation is tests/orf_mirror.py over the rows the records spell.
Without one of the flags the JSON is, byte for byte, what the commit before this feature wrote for the same input
(tests/golden/orf_cli_plain_parent.json, but for the time stamp and the path of the binary)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import bam_py
import hypermut_mirror as hm
import orf_mirror as om

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JULIET = os.path.join(ROOT, "minorseq_amd", "bin", "juliet")
GOLDEN = os.path.join(ROOT, "tests", "golden", "orf_cli_plain_parent.json")
N, L = 330, 300
GENES = [("gag", 1, 151), ("pol", 101, 281)]      # 1-based [begin, end): 50 codons from column 0 (frame 0), 60 from column 100 (frame 1)
N_COLS = 285                                      # the window: the genes' last base + 5 (docs/SPEC.md §3), inside the reference
SPANS = [(b - 1, (e - b) // 3) for _, b, e in GENES]
STOP_READS = np.arange(4, N, 30)                  # TAA at codon 11 of gag
DEL1_READS = np.arange(9, N, 30)                  # one base of gag deleted
PAIR_READS = np.arange(14, N, 30)                 # a -1 and a -2 deletion where both genes overlap: in frame again
DEL3_READS = np.arange(19, N, 30)                 # one codon's worth of pol deleted
LAST_READS = np.arange(24, N, 30)                 # TAG in the last codon of pol
HYPER_READS = np.arange(29, N, 30)                # G->A at most target sites, and one base of pol deleted
MINOR = np.arange(3, N, 6)                        # carriers of a minor codon
TEXT = "@HD\tVN:1.5\tSO:unknown\tpb:3.0.1\n@SQ\tSN:main\tLN:%d\n@RG\tID:x\tPL:PACBIO\tPM:SEQUEL\tDS:READTYPE=CCS\n" % L


def sample():
    """(ref codes, rows[N, L])."""
    rng = np.random.default_rng(27)
    ref = rng.integers(0, 4, size=L, dtype=np.uint8)
    ref[rng.random(L) < 0.3] = hm.G
    for col, nc in SPANS:                          # no stop in either gene's frame (a C makes none)
        for k in range(nc):
            if tuple(ref[col + 3 * k:col + 3 * k + 3].tolist()) in om.STOP_CODONS:
                ref[col + 3 * k] = om.C
    rows = np.repeat(ref[None, :], N, axis=0)
    rows[(rng.random((N, L)) < 0.01) & (ref != hm.G)[None, :]] = om.C
    rows[MINOR, 27:30] = (om.C, om.T, om.C)
    for r in HYPER_READS:
        x, y, z = rows[r, :-2], rows[r, 1:-1], rows[r, 2:]
        tgt = np.flatnonzero((x == hm.G) & ((y == hm.A) | (y == hm.G)) & (z != hm.C))
        rows[r, tgt[rng.random(len(tgt)) < 0.7]] = hm.A
    rows[HYPER_READS, 250] = om.GAP
    rows[STOP_READS, 30:33] = (om.T, om.A, om.A)
    rows[DEL1_READS, 50] = om.GAP
    rows[PAIR_READS, 120] = om.GAP
    rows[PAIR_READS, 130:132] = om.GAP
    rows[DEL3_READS, 200:203] = om.GAP
    rows[LAST_READS, 277:280] = (om.T, om.A, om.G)
    for i in range(0, N, 7):
        b, e = int(rng.integers(1, 20)), L - int(rng.integers(1, 20))
        rows[i, :b], rows[i, e:] = 6, 6
    return ref, rows


def records_of(rows, ref, which):
    """The reads as records: = and X runs against the reference, D where the read has a gap (a PacBio BAM has no M)."""
    out = []
    for i in which:
        cov = np.flatnonzero(rows[i] != 6)
        b, e = int(cov[0]), int(cov[-1]) + 1
        cells = rows[i, b:e]
        seq = "".join("ACGT"[c] for c in cells if c < 4)
        kind = np.where(cells == om.GAP, 2, np.where(cells == ref[b:e], 0, 1))
        cuts = [0, *(np.flatnonzero(kind[1:] != kind[:-1]) + 1).tolist(), e - b]
        ops = [("=XD"[kind[lo]], hi - lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
        out.append(dict(ref_id=0, pos=b, flag=0, mapq=60, name="m/%d/ccs" % i, cigar=ops, seq=seq, qual=bytes([60]) * len(seq),
                        tags=[("rq", "f", 0.999), ("np", "i", 12)]))
    return out


def expectation(rows, ref, kinds=om.STOP | om.FRAMESHIFT, max_deletion=0, tail=0):
    """(counts, first, flags, idx, n_defective) of the window's columns."""
    cnt, first = om.counters(rows[:, :N_COLS], SPANS, ref[:N_COLS])
    flags = om.classify(cnt, first, SPANS, max_deletion, tail)
    idx, bad = om.keep(flags, kinds)
    return cnt, first, flags, idx, bad


def write_inputs(d):
    """in.bam, ref.json, maj.json and the sample they spell, in directory d."""
    ref, rows = sample()
    bam_py.write_bam(os.path.join(d, "in.bam"), TEXT, [("main", L)], records_of(rows, ref, range(N)), block=20000)
    cfg = {"genes": [dict(name=n, begin=b, end=e, drms=[]) for n, b, e in GENES], "referenceName": "main", "version": "tests/test_gpu_orf_cli.py", "databaseVersion": "none"}
    json.dump(dict(cfg, referenceSequence="".join("ACGT"[c] for c in ref)), open(os.path.join(d, "ref.json"), "w"))
    json.dump(cfg, open(os.path.join(d, "maj.json"), "w"))
    return ref, rows


PLAIN_ARGS = ("-c", "ref.json", "--mode-phasing", "in.bam", "plain.json")


def normalised(text):
    """The JSON text without what differs from run to run: the time stamp and the path of the binary in the command line."""
    text = re.sub(r'("timestamp":\s*)"[^"]*"', r'\1"T"', text, count=1)
    return re.sub(r'("command_line":\s*")[^" ]*', r"\1juliet", text, count=1)


def juliet(d, *args):
    return subprocess.run([JULIET, *args], cwd=d, capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    if not os.path.exists(JULIET):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "host")])
    d = tmp_path_factory.mktemp("orf_cli")
    ref, rows = write_inputs(str(d))
    _, _, _, idx, _ = expectation(rows, ref)
    bam_py.write_bam(str(d / "kept.bam"), TEXT, [("main", L)], records_of(rows, ref, idx), block=20000)
    for args in (("-c", "ref.json", "--mode-phasing", "--drop-defective", "--orf-report", "r.tsv", "in.bam", "drop.json", "drop.html"),
                 ("-c", "ref.json", "--mode-phasing", "kept.bam", "kept.json"),
                 PLAIN_ARGS):
        r = juliet(d, *args)
        assert r.returncode == 0, (args, r.stderr)
    return d, ref, rows


def strip(path):
    j = json.load(open(path))
    j["input"].pop("timestamp")
    j["input"].pop("command_line")
    return j


def gene_counts(flags):
    return [dict(name=GENES[g][0], partial=int((flags[g] & om.PARTIAL != 0).sum()), stop=int((flags[g] & om.STOP != 0).sum()),
                 frameshift=int((flags[g] & om.FRAMESHIFT != 0).sum()), deletion=int((flags[g] & om.DELETION != 0).sum())) for g in range(len(GENES))]


def test_the_sample_is_what_it_claims():
    ref, rows = sample()
    cnt, first, flags, idx, bad = expectation(rows, ref)
    assert (flags[0, STOP_READS] & om.STOP).all() and (first[0, STOP_READS] == 10).all() and not (flags[1, STOP_READS] & om.STOP).any()
    assert (flags[0, DEL1_READS] & om.FRAMESHIFT).all() and not (flags[1, DEL1_READS] & om.FRAMESHIFT).any()
    assert (cnt[om.GAP_CELLS][:, PAIR_READS] == 3).all() and not (flags[:, PAIR_READS] & om.FRAMESHIFT).any()      # -1 and -2 cancel, in both genes
    assert (cnt[om.GAP_CELLS, 1, DEL3_READS] == 3).all() and not (flags[:, DEL3_READS] & (om.FRAMESHIFT | om.STOP)).any()
    assert (first[1, LAST_READS] == SPANS[1][1] - 1).all() and (flags[1, LAST_READS] & om.STOP).all()
    dropped = set(np.setdiff1d(np.arange(N), idx).tolist())
    assert dropped >= set(STOP_READS) | set(DEL1_READS) | set(LAST_READS) | set(HYPER_READS) and not dropped & (set(PAIR_READS) | set(DEL3_READS))
    assert SPANS[0][0] % 3 != SPANS[1][0] % 3 and SPANS[0][0] + 3 * SPANS[0][1] > SPANS[1][0]      # overlapping, in different frames


def test_report_equals_the_mirror(cli):
    d, ref, rows = cli
    cnt, first, flags, _, _ = expectation(rows, ref)
    lines = open(d / "r.tsv").read().splitlines()
    assert len(lines) == N * len(GENES)
    for i in range(N):
        for g, (gene, _, _) in enumerate(GENES):
            exp = ["m/%d/ccs" % i, gene, *(str(int(cnt[q, g, i])) for q in range(4)),
                   "-" if first[g, i] == om.NO_STOP else str(int(first[g, i]) + 1), om.letters(int(flags[g, i]))]
            assert lines[i * len(GENES) + g].split("\t") == exp, (i, gene)
    assert {ln.split("\t")[-1] for ln in lines} >= {"-", "P", "S", "F"}


def test_drop_equals_a_run_on_the_kept_reads(cli):
    d, ref, rows = cli
    _, _, flags, idx, bad = expectation(rows, ref)
    drop, kept_run, plain = strip(d / "drop.json"), strip(d / "kept.json"), strip(d / "plain.json")
    block = drop["input"].pop("orf_integrity")
    assert list(block) == ["reference", "kinds", "max_deletion", "tail_codons", "reads", "defective", "kept", "dropped", "genes"]
    assert block == dict(reference="reference", kinds="stop,frameshift", max_deletion=0, tail_codons=0, reads=N, defective=bad, kept=len(idx),
                         dropped=True, genes=gene_counts(flags))
    assert 0 < bad < N // 2 and drop["target_config"]["n_reads"] == len(idx)
    drop["input"].pop("input_file"), kept_run["input"].pop("input_file")
    assert drop == kept_run                                         # the variant table, the haplotypes and their reads' names
    assert sum(len(g["variant_positions"]) for g in drop["genes"]) >= 1 and drop["genes"] != plain["genes"]
    names = [n for h in drop["haplotype"]["haplotypes"] for n in h["read_names"]]
    assert names and {int(n.split("/")[1]) for n in names} <= set(idx.tolist())      # names follow the kept indices
    html = open(d / "drop.html").read()
    m = re.search(r'<table id="orf-integrity-table" data-reference="reference">.*?</table>', html, flags=re.S)
    assert m
    for leaf, text in (("kinds", "stop,frameshift"), ("max_deletion", "0"), ("tail_codons", "0"), ("reads", str(N)), ("defective", str(bad)),
                       ("kept", str(len(idx))), ("dropped", "true")):
        assert f"<td>{leaf}</td><td>{text}</td>" in m.group(0), (leaf, m.group(0))
    m = re.search(r'<table id="orf-integrity-genes">.*?</table>', html, flags=re.S)
    for gc in gene_counts(flags):
        assert "<td>" + "</td><td>".join(str(gc[k]) for k in ("name", "partial", "stop", "frameshift", "deletion")) + "</td>" in m.group(0)


def test_without_the_flags_the_json_is_the_parents(cli):
    d, ref, rows = cli
    assert "orf_integrity" not in json.load(open(d / "plain.json"))["input"]
    assert normalised(open(d / "plain.json").read()) == open(GOLDEN).read()


KIND_NAMES = {om.STOP: "stop", om.FRAMESHIFT: "frameshift", om.DELETION: "deletion"}


@pytest.mark.parametrize("kinds", [2, 4, 8, 6, 10, 12, 14])
def test_every_choice_of_kinds(cli, kinds):
    d, ref, rows = cli
    text = ",".join(name for bit, name in KIND_NAMES.items() if kinds & bit)
    K = 3
    r = juliet(d, "-c", "ref.json", "--drop-defective", "--defect-kinds", text, "--defect-max-deletion", str(K), "in.bam", "k%d.json" % kinds)
    assert r.returncode == 0, r.stderr
    _, _, flags, idx, bad = expectation(rows, ref, kinds, K)
    j = json.load(open(d / ("k%d.json" % kinds)))
    assert j["input"]["orf_integrity"] == dict(reference="reference", kinds=text, max_deletion=K, tail_codons=0, reads=N, defective=bad, kept=len(idx),
                                               dropped=True, genes=gene_counts(flags))
    assert j["target_config"]["n_reads"] == len(idx) and 0 < bad < N
    if kinds & om.DELETION:      # three gap cells reach the bound: the -1/-2 pair and the 3-base deletion go
        assert not set(idx.tolist()) & (set(PAIR_READS) | set(DEL3_READS))


def test_tail_codons_keep_the_stop_in_the_last_codon(cli):
    d, ref, rows = cli
    r = juliet(d, "-c", "ref.json", "--mode-phasing", "--drop-defective", "--defect-tail-codons", "1", "in.bam", "tail.json")
    assert r.returncode == 0, r.stderr
    _, _, flags, idx, bad = expectation(rows, ref, tail=1)
    _, _, _, idx0, bad0 = expectation(rows, ref)
    assert set(LAST_READS) <= set(idx.tolist()) and not set(LAST_READS) & set(idx0.tolist()) and bad < bad0
    j = json.load(open(d / "tail.json"))
    assert j["input"]["orf_integrity"] == dict(reference="reference", kinds="stop,frameshift", max_deletion=0, tail_codons=1, reads=N, defective=bad,
                                               kept=len(idx), dropped=True, genes=gene_counts(flags))
    names = {int(n.split("/")[1]) for h in j["haplotype"]["haplotypes"] for n in h["read_names"]}
    assert names <= set(idx.tolist())


def test_after_the_hypermutation_filter_and_on_the_majority_row(cli):
    """--drop-hypermutated first, the reading-frame counters on what it kept; without a referenceSequence both take the majority."""
    d, ref, rows = cli
    for cfg, out in (("ref.json", "two.json"), ("maj.json", "two_maj.json")):
        r = juliet(d, "-c", cfg, "--drop-hypermutated", "--drop-defective", "--orf-report", out + ".tsv", "in.bam", out)
        assert r.returncode == 0, r.stderr
    import readstats_mirror as rm
    for out, row, which in (("two.json", ref, "reference"), ("two_maj.json", np.concatenate([rm.consensus(rows[:, :N_COLS]), ref[N_COLS:]]), "majority")):
        _, _, frs = hm.p_values(hm.counts(rows[:, :N_COLS], row[:N_COLS]))
        clean, flagged = hm.keep(frs, hm.Fraction(0.05))
        assert set(np.setdiff1d(np.arange(N), clean).tolist()) == set(HYPER_READS)
        _, _, flags, idx, bad = expectation(rows[clean], row)
        j = json.load(open(d / out))
        assert j["input"]["hypermutation"]["kept"] == len(clean) == N - len(HYPER_READS)
        assert j["input"]["orf_integrity"] == dict(reference=which, kinds="stop,frameshift", max_deletion=0, tail_codons=0, reads=len(clean), defective=bad,
                                                   kept=len(idx), dropped=True, genes=gene_counts(flags))
        assert j["target_config"]["n_reads"] == len(idx)
        lines = open(d / (out + ".tsv")).read().splitlines()            # the report lists the reads the earlier filter kept
        assert [ln.split("\t")[0] for ln in lines[::2]] == ["m/%d/ccs" % i for i in clean]


def test_batch_filters_every_sample(cli):
    d, ref, rows = cli
    (d / "l.tsv").write_text("in.bam\tb1.json\nin.bam\tb2.json\n")
    r = juliet(d, "-c", "ref.json", "--mode-phasing", "--drop-defective", "--batch", "l.tsv")
    assert r.returncode == 0, r.stderr
    single = strip(d / "drop.json")
    for name in ("b1.json", "b2.json"):
        assert strip(d / name) == single


def test_no_read_kept_is_an_input_error(cli):
    d, ref, rows = cli
    bam_py.write_bam(str(d / "bad.bam"), TEXT, [("main", L)], records_of(rows, ref, STOP_READS), block=20000)
    r = juliet(d, "-c", "ref.json", "--drop-defective", "bad.bam", "none.json")
    assert r.returncode == 2 and "keeps none" in r.stderr, (r.returncode, r.stderr)
    assert not (d / "none.json").exists()
