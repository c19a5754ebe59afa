"""The front end's hypermutation filter (docs/SPEC.md §26): --hypermut-report, --drop-hypermutated [--hypermut-alpha], the JSON's
input.hypermutation block and its HTML table, and what is refused.  The BAMs are written by the suite's independent writer
(tests/bam_py.py), not by the project's synthesiser: a few hundred reads over a reference with planted G, a chosen minority of the
reads carrying G->A at most of their target sites.  Every expectation is tests/hypermut_mirror.py over the rows the records spell."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import bam_py
import hypermut_mirror as hm
import readstats_mirror as rm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JULIET = os.path.join(ROOT, "minorseq_amd", "bin", "juliet")
N, L = 400, 300
PLANTED = np.arange(7, N, 10)            # the hypermutated reads: every tenth
MINOR = np.arange(3, N, 6)               # carriers of a minor codon
TEXT = "@HD\tVN:1.5\tSO:unknown\tpb:3.0.1\n@SQ\tSN:main\tLN:%d\n@RG\tID:x\tPL:PACBIO\tPM:SEQUEL\tDS:READTYPE=CCS\n" % L


def sample():
    """(ref codes, rows[N, L]): the reference with G at nearly half of its columns; every read the reference with substitutions at 1 % of
    the columns that are no G; the MINOR reads with CTC at codon 10; the PLANTED reads with A at 70 % of their target-context G;
    every seventh read covers only a part of the window."""
    rng = np.random.default_rng(26)
    ref = rng.integers(0, 4, size=L, dtype=np.uint8)
    ref[rng.random(L) < 0.3] = hm.G
    rows = np.repeat(ref[None, :], N, axis=0)
    sub = (rng.random((N, L)) < 0.01) & (ref != hm.G)[None, :]
    rows[sub] = ((rows + 1 + rng.integers(0, 3, size=(N, L))) % 4).astype(np.uint8)[sub]
    rows[MINOR, 27:30] = (hm.C, hm.T, hm.C)
    for r in PLANTED:
        x, y, z = rows[r, :-2], rows[r, 1:-1], rows[r, 2:]
        tgt = np.flatnonzero((x == hm.G) & ((y == hm.A) | (y == hm.G)) & (z != hm.C))
        rows[r, tgt[rng.random(len(tgt)) < 0.7]] = hm.A
    for i in range(0, N, 7):
        b, e = int(rng.integers(1, 20)), L - int(rng.integers(1, 20))
        rows[i, :b], rows[i, e:] = 6, 6
    return ref, rows


def records_of(rows, ref, which):
    """The reads as records: = and X runs against the reference (a PacBio BAM has no M)."""
    out = []
    for i in which:
        cov = np.flatnonzero(rows[i] != 6)
        b, e = int(cov[0]), int(cov[-1]) + 1
        seq = "".join("ACGT"[c] for c in rows[i, b:e])
        same = rows[i, b:e] == ref[b:e]
        cuts = [0, *(np.flatnonzero(same[1:] != same[:-1]) + 1).tolist(), e - b]
        ops = [("=" if same[lo] else "X", hi - lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
        out.append(dict(ref_id=0, pos=b, flag=0, mapq=60, name="m/%d/ccs" % i, cigar=ops, seq=seq, qual=bytes([60]) * len(seq),
                        tags=[("rq", "f", 0.999), ("np", "i", 12)]))
    return out


def juliet(d, *args):
    return subprocess.run([JULIET, *args], cwd=d, capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    if not os.path.exists(JULIET):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "host")])
    d = tmp_path_factory.mktemp("hypermut_cli")
    ref, rows = sample()
    clean = np.setdiff1d(np.arange(N), PLANTED)
    bam_py.write_bam(str(d / "in.bam"), TEXT, [("main", L)], records_of(rows, ref, range(N)), block=20000)
    bam_py.write_bam(str(d / "clean.bam"), TEXT, [("main", L)], records_of(rows, ref, clean), block=20000)
    bam_py.write_bam(str(d / "all.bam"), TEXT, [("main", L)], records_of(rows, ref, PLANTED), block=20000)
    cfg = {"genes": [dict(name="G", begin=1, end=L + 1, drms=[])], "referenceName": "main", "version": "tests/test_gpu_hypermut_cli.py", "databaseVersion": "none"}
    json.dump(dict(cfg, referenceSequence="".join("ACGT"[c] for c in ref)), open(d / "ref.json", "w"))
    json.dump(cfg, open(d / "maj.json", "w"))                      # no reference sequence: the G are the majority's
    for args in (("-c", "ref.json", "--mode-phasing", "--drop-hypermutated", "--hypermut-report", "r.tsv", "in.bam", "drop.json", "drop.html"),
                 ("-c", "ref.json", "--mode-phasing", "clean.bam", "clean.json"),
                 ("-c", "ref.json", "--mode-phasing", "in.bam", "plain.json"),
                 ("-c", "maj.json", "--hypermut-report", "m.tsv", "in.bam", "majority.json")):
        r = juliet(d, *args)
        assert r.returncode == 0, (args, r.stderr)
    return d, ref, rows


def expectation(rows, ref, alpha=0.05):
    cnt = hm.counts(rows, ref)
    p, _, frs = hm.p_values(cnt)
    fa = hm.Fraction(alpha)
    assert all(abs(f - fa) > fa / 10**9 for f in frs)               # no exact p close enough to alpha for a rounding to decide
    idx, flagged = hm.keep(frs, fa)
    return cnt, p, idx, flagged


def check_report(path, rows, ref):
    cnt, p, _, _ = expectation(rows, ref)
    lines = open(path).read().splitlines()
    assert len(lines) == N
    for i, line in enumerate(lines):
        name, *nums = line.split("\t")
        assert name == "m/%d/ccs" % i and len(nums) == 5, line
        assert [int(x) for x in nums[:4]] == cnt[:, i].tolist(), (i, line)
        assert abs(float(nums[4]) - p[i]) <= 5e-12 * p[i], (i, line)
    return cnt


def test_report_equals_the_mirror(cli):
    d, ref, rows = cli
    cnt = check_report(d / "r.tsv", rows, ref)
    assert cnt[hm.TARGET_MUT][PLANTED].min() > 10 and cnt[hm.CONTROL_SITES].min() > 5
    check_report(d / "m.tsv", rows, rm.consensus(rows))             # ... and on the majority's G
    assert (rm.consensus(rows) == ref).mean() > 0.95
    j = json.load(open(d / "majority.json"))
    assert j["input"]["hypermutation"] == dict(reference="majority", alpha=0.05, reads=N, flagged=len(PLANTED), kept=N, dropped=False)
    assert j["target_config"]["n_reads"] == N                       # the report alone drops nothing


def strip(path):
    j = json.load(open(path))
    j["input"].pop("timestamp")
    j["input"].pop("command_line")
    return j


def test_drop_equals_a_run_without_the_planted_reads(cli):
    d, ref, rows = cli
    _, _, idx, flagged = expectation(rows, ref)
    clean = np.setdiff1d(np.arange(N), PLANTED)
    assert idx.tolist() == clean.tolist() and flagged == len(PLANTED)            # the mirror flags exactly the planted reads
    drop, ref_run, plain = strip(d / "drop.json"), strip(d / "clean.json"), strip(d / "plain.json")
    block = drop["input"].pop("hypermutation")
    assert list(block) == ["reference", "alpha", "reads", "flagged", "kept", "dropped"]
    assert block == dict(reference="reference", alpha=0.05, reads=N, flagged=flagged, kept=len(idx), dropped=True)
    assert drop["target_config"]["n_reads"] == len(idx)
    drop["input"].pop("input_file"), ref_run["input"].pop("input_file")
    assert drop == ref_run                                          # the variant table, the haplotypes and their reads' names
    assert sum(len(g["variant_positions"]) for g in drop["genes"]) >= 1 and drop["genes"] != plain["genes"]
    names = [n for h in drop["haplotype"]["haplotypes"] for n in h["read_names"]]
    assert names and {int(n.split("/")[1]) for n in names} <= set(clean.tolist())      # names follow the kept indices
    html = open(d / "drop.html").read()
    m = re.search(r'<table id="hypermutation-table" data-reference="reference">.*?</table>', html, flags=re.S)
    assert m
    for leaf, text in (("alpha", "%.17g" % 0.05), ("reads", str(N)), ("flagged", str(flagged)), ("kept", str(len(idx))), ("dropped", "true")):
        assert f"<td>{leaf}</td><td>{text}</td>" in m.group(0), (leaf, m.group(0))


def test_flags_that_drop_nothing_change_nothing_else(cli):
    d, ref, rows = cli
    for out, args in (("only", ("--hypermut-report", "only.tsv")), ("tiny", ("--drop-hypermutated", "--hypermut-alpha", "1e-300")),
                      ("both", ("--max-read-mismatch-perc", "100", "--drop-hypermutated", "--hypermut-alpha", "1e-300"))):
        r = juliet(d, "-c", "ref.json", "--mode-phasing", *args, "in.bam", out + ".json")
        assert r.returncode == 0, r.stderr
    plain = strip(d / "plain.json")
    assert "hypermutation" not in plain["input"]
    assert open(d / "only.tsv").read() == open(d / "r.tsv").read()
    for name, n_flagged, dropped in (("only", len(PLANTED), False), ("tiny", 0, True), ("both", 0, True)):
        other = strip(d / (name + ".json"))
        block = other["input"].pop("hypermutation")
        other["input"].pop("read_filter", None)
        assert block == dict(reference="reference", alpha=0.05 if name == "only" else 1e-300, reads=N, flagged=n_flagged, kept=N, dropped=dropped)
        assert other == plain, name


def test_after_a_read_filter_that_drops_reads(cli):
    """The read filter first, the hypermutation counters on what it kept: partial reads go to the read filter, planted ones here."""
    d, ref, rows = cli
    r = juliet(d, "-c", "ref.json", "--min-read-bases", str(L), "--drop-hypermutated", "in.bam", "two.json")
    assert r.returncode == 0, r.stderr
    full = np.flatnonzero((rows < 4).sum(axis=1) >= L)
    assert 0 < len(full) < N
    _, _, idx, flagged = expectation(rows[full], ref)
    j = json.load(open(d / "two.json"))
    assert j["input"]["read_filter"]["kept"] == len(full)
    assert j["input"]["hypermutation"] == dict(reference="reference", alpha=0.05, reads=len(full), flagged=flagged, kept=len(idx), dropped=True)
    assert j["target_config"]["n_reads"] == len(idx) == len(full) - len(np.intersect1d(full, PLANTED)) and flagged > 0


def test_batch_filters_every_sample(cli):
    d, ref, rows = cli
    (d / "l.tsv").write_text("in.bam\tb1.json\nin.bam\tb2.json\n")
    r = juliet(d, "-c", "ref.json", "--mode-phasing", "--drop-hypermutated", "--batch", "l.tsv")
    assert r.returncode == 0, r.stderr
    single = strip(d / "drop.json")
    for name in ("b1.json", "b2.json"):
        assert strip(d / name) == single


def test_no_read_kept_is_an_input_error(cli):
    d, ref, rows = cli
    r = juliet(d, "-c", "ref.json", "--drop-hypermutated", "all.bam", "none.json")
    assert r.returncode == 2 and "keeps none" in r.stderr, (r.returncode, r.stderr)
    assert not (d / "none.json").exists()


@pytest.mark.parametrize("args", [["--windows", "2"], ["--mix", "b.bam"], ["--devices", "0,0"], ["--consensus", "c.fasta"], ["--call-insertions"]])
def test_refused_combinations_open_nothing(tmp_path, args):
    for flags in (["--drop-hypermutated"], ["--hypermut-report", "r.tsv"], ["--drop-hypermutated", "--hypermut-alpha", "0.01"]):
        r = juliet(tmp_path, *flags, *args, "no_such.bam", "o.json")
        assert r.returncode == 1 and "hypermut" in r.stderr, (r.returncode, r.stderr)
        assert not list(tmp_path.iterdir())


def test_refused_as_fuse_with_batch_and_bad_levels(tmp_path):
    (tmp_path / "l.tsv").write_text("no_such.bam\ta.json\n")
    r = juliet(tmp_path, "--hypermut-report", "r.tsv", "--batch", "l.tsv")
    assert r.returncode == 1 and "--batch" in r.stderr
    r = subprocess.run([os.path.join(ROOT, "minorseq_amd", "bin", "fuse"), "--drop-hypermutated", "no_such.bam", "o.fasta"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "fuse" in r.stderr
    r = juliet(tmp_path, "--hypermut-alpha", "0.01", "no_such.bam", "o.json")
    assert r.returncode == 1 and "--drop-hypermutated" in r.stderr
    for level in ("0", "1.5", "-0.1", "x"):
        r = juliet(tmp_path, "--drop-hypermutated", "--hypermut-alpha", level, "no_such.bam", "o.json")
        assert r.returncode == 1 and "(0, 1]" in r.stderr, (level, r.stderr)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["l.tsv"]
