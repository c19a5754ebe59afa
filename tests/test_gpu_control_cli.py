"""`juliet --control control.bam` end to end on the GPU (docs/SPEC.md §21): two synthetic BAMs over one reference — a sample with
the 4 x 1 % mixture, and a control drawn from another seed with the minors switched off — through the front end; the JSON must
hold exactly the rows of the exact mirror (control_mirror.py) with the control's counts beside them, --mode-phasing must phase
that table, --downsample must touch the sample only, and the flag combinations the rule does not define must exit with 2."""
import json
import os
import subprocess

import numpy as np
import pytest

import control_mirror as cm
from minorseq_amd import capi, msa, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JULIET = os.path.join(ROOT, "minorseq_amd", "bin", "juliet")
SYNTH = os.path.join(ROOT, "minorseq_amd", "bin", "juliet-synth")
N_S, N_C, L, SEED, CONTROL_SEED = 3000, 2000, 300, 4, 9
MINOR = (10, 10, 10, 10)


@pytest.fixture(scope="module", autouse=True)
def built():
    """The binaries normally travel with the tree; build them only if they are missing (never under a loaded .so)."""
    if not os.path.exists(os.path.join(ROOT, "minorseq_amd", "libjuliet_hip.so")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "csrc")])
    if not (os.path.exists(JULIET) and os.path.exists(SYNTH)):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "host")])


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    d = tmp_path_factory.mktemp("control_cli")
    bam, ctl, cfg = str(d / "s.align.bam"), str(d / "c.align.bam"), str(d / "cfg.json")
    subprocess.check_call([SYNTH, "--reads", str(N_S), "--cols", str(L), "--seed", str(SEED), "--partial", "0.1",
                           "--minor-permille", *map(str, MINOR), "-o", bam, "--config-out", cfg])
    subprocess.check_call([SYNTH, "--reads", str(N_C), "--cols", str(L), "--seed", str(CONTROL_SEED), "--ref-seed", str(SEED),
                           "--partial", "0.1", "--minor-permille", "0", "0", "0", "0", "-o", ctl])
    ref = synth.reference(SEED, L)
    rows_s = synth.rows(synth.SynthParams(seed=SEED, partial_rate=0.1, minor_permille=MINOR), L, 0, N_S, ref)
    rows_c = synth.rows(synth.SynthParams(seed=CONTROL_SEED, partial_rate=0.1, minor_permille=(0, 0, 0, 0)), L, 0, N_C, ref)
    pos = cm.positions([(1, L + 1)], L, ref)
    want, want_cov = cm.call_rows(cm.hists(rows_s, pos[2]), cm.hists(rows_c, pos[2]), *pos[:4], 0.01, pos[4])
    return d, bam, ctl, cfg, rows_s, want, want_cov


def run_juliet(d, bam, *args, out="o.json"):
    o = str(d / out)
    subprocess.check_call([JULIET, *args, bam, o])
    return json.load(open(o)) if o.endswith(".json") else open(o).read()


def flat_variants(j):
    rows = []
    for gi, g in enumerate(j["genes"]):
        for vp in g["variant_positions"]:
            for aa in vp["variant_amino_acids"]:
                for vc in aa["variant_codons"]:
                    rows.append((gi, vp["ref_position"], msa.codon_index(vc["codon"]), vc, vp))
    return sorted(rows, key=lambda r: r[:3])


def assert_json_rows(j, want, want_cov):
    got = flat_variants(j)
    assert [r[:3] for r in got] == [(w[0], w[1], w[4]) for w in want]
    for (gi, pos, cod, vc, vp), w, cc in zip(got, want, want_cov):
        assert (vc["count"], vp["coverage"], vc["expected"], vc["control_count"], vc["control_coverage"]) == (w[5], w[6], w[7], w[7], cc)
        assert vc["frequency"] == w[5] / w[6] and vc["control_frequency"] == w[7] / cc
        assert vp["ref_codon"] == msa.codon_string(w[3])
        assert abs(vc["pValue"] - w[8]) <= 1e-10 and (w[8] <= 1e-300 or abs(vc["pValue"] - w[8]) <= 5e-12 * w[8])
        assert abs(vc["log_pValue"] - w[9]) <= 1e-12 * max(1.0, abs(w[9])) + 1e-13


def test_json_holds_the_mirrors_rows(pair):
    d, bam, ctl, cfg, rows_s, want, want_cov = pair
    assert len(want) >= 4                                   # the planted minors, called against a control that lacks them
    j = run_juliet(d, bam, "-c", cfg, "--control", ctl)
    assert_json_rows(j, want, want_cov)
    assert j["input"]["control"] == {"file": ctl, "reads": N_C} and j["target_config"]["n_reads"] == N_S
    assert "haplotype" not in j
    html = run_juliet(d, bam, "-c", cfg, "--control", ctl, out="o.html")
    assert 'id="control-table"' in html and ctl in html
    w = want[0]
    assert f"control_count={w[7]} control_coverage={want_cov[0]} control_frequency=" in html


def test_phasing_takes_the_control_called_table(pair, oracle):
    d, bam, ctl, cfg, rows_s, want, want_cov = pair
    j = run_juliet(d, bam, "-c", cfg, "--control", ctl, "--mode-phasing")
    assert_json_rows(j, want, want_cov)
    table = np.zeros(len(want), dtype=capi.VARIANT)
    for k, w in enumerate(want):
        table[k] = (w[0], w[1], w[2], w[3], w[4], 0, w[5], w[6], w[7], 0, w[8], w[9])
    ph = oracle.phase(rows_s, table)
    hb = j["haplotype"]
    assert [h["reads"] for h in hb["haplotypes"]] == ph["hap_count"].tolist() and len(hb["haplotypes"]) >= 2
    assert hb["reported_reads"] + hb["insufficient_coverage_reads"] + hb["damaged_reads"] == N_S
    for hi, h in enumerate(hb["haplotypes"]):
        assert [msa.codon_index(c) for c in h["codons"]] == ph["hap_pattern"][hi].tolist()
    for k, r in enumerate(flat_variants(j)):
        assert r[3]["haplotype_hit"] == [bool(x) for x in ph["hit"][k]]


def test_downsample_samples_the_sample_only(pair):
    d, bam, ctl, cfg, rows_s, want, want_cov = pair
    j = run_juliet(d, bam, "-c", cfg, "--control", ctl, "--downsample", "1500", "--sample-seed", "3")
    assert j["target_config"]["n_reads"] == 1500 and j["input"]["control"]["reads"] == N_C
    assert j["input"]["sampling"]["sources"][0]["kept"] == 1500
    for r in flat_variants(j):
        assert r[4]["coverage"] <= 1500 and r[3]["control_coverage"] > 1500


@pytest.mark.parametrize("flags", [("--windows", "2"), ("--devices", "0,0", "--windows", "2"), ("--mix", "x.bam"), ("--call-deletions",),
                                   ("--call-insertions",), ("--fisher-tail", "two-sided")])
def test_refused_combinations_exit_2(pair, flags):
    d, bam, ctl, cfg = pair[:4]
    r = subprocess.run([JULIET, "-c", cfg, "--control", ctl, *flags, bam, str(d / "r.json")], capture_output=True, text=True)
    assert r.returncode == 2 and "juliet: --control " in r.stderr, (r.returncode, r.stderr)


def test_refused_with_batch_and_as_fuse(pair):
    d, bam, ctl, cfg = pair[:4]
    lst = d / "batch.tsv"
    lst.write_text(f"{bam}\t{d / 'b.json'}\n")
    r = subprocess.run([JULIET, "-c", cfg, "--control", ctl, "--batch", str(lst)], capture_output=True, text=True)
    assert r.returncode == 2 and "juliet: --control " in r.stderr, (r.returncode, r.stderr)
    fuse = os.path.join(os.path.dirname(JULIET), "fuse")
    r = subprocess.run([fuse, "--control", ctl, bam, str(d / "f.fasta")], capture_output=True, text=True)
    assert r.returncode == 2 and "--control is not an option of fuse" in r.stderr, (r.returncode, r.stderr)
