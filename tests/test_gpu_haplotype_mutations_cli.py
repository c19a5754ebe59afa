"""`juliet --mode-phasing --haplotype-mutations` end to end (docs/SPEC.md §24): per-haplotype mutation tables, drugs and the drug
profile from ONE per-class codon table.  Every new leaf is compared with the mirror (tests/class_codons_mirror.py) computed from
the --dump-msa rows of the same BAM and the JSON's own per-read haplotype assignment."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import class_codons_mirror as mirror

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JULIET = os.path.join(ROOT, "minorseq_amd", "bin", "juliet")
FUSE = os.path.join(ROOT, "minorseq_amd", "bin", "fuse")
SYNTH = os.path.join(ROOT, "minorseq_amd", "bin", "juliet-synth")
N, L, SEED = 3000, 300, 41
MINOR = (150, 120, 100, 80)
NEW_HAP, NEW_ROW = ("mutations", "drugs"), ("haplotype_count", "haplotype_coverage")


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(os.path.join(ROOT, "minorseq_amd", "libjuliet_hip.so")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "csrc")])
    if not (os.path.exists(JULIET) and os.path.exists(SYNTH)):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "host")])


def juliet(d, *args, exe=JULIET):
    return subprocess.run([exe, *args], cwd=d, capture_output=True, text=True, timeout=120)


def read_msa(path):
    raw = open(path, "rb").read()
    n, l, wb = (int(x) for x in np.frombuffer(raw[:24], dtype=np.uint64))
    return np.frombuffer(raw[24:], dtype=np.uint8).reshape(n, l), wb


def codon_of(s):
    return 16 * "ACGT".index(s[0]) + 4 * "ACGT".index(s[1]) + "ACGT".index(s[2])


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    """The mixture, and a config of two drugs: `fixed` on a codon where the config's reference is changed so that every clone
    differs from it, `minor` on the first planted edit — a codon one minor clone carries."""
    d = tmp_path_factory.mktemp("hapmut_cli")
    subprocess.check_call([SYNTH, "--reads", str(N), "--cols", str(L), "--seed", str(SEED), "--partial", "0.1",
                           "--minor-permille", *map(str, MINOR), "-o", str(d / "in.bam"), "--config-out", str(d / "synth.json")])
    cfg = json.load(open(d / "synth.json"))
    (gene,) = cfg["genes"]
    planted = gene["drms"][0]["positions"]
    edited = {int(re.sub(r"\D", "", s)) for s in planted}
    fixed_pos = next(p for p in range(40, 60) if not {p - 1, p, p + 1} & edited)
    c = gene["begin"] - 1 + 3 * (fixed_pos - 1)
    ref = cfg["referenceSequence"]
    sample_codon = ref[c:c + 3]
    changed = next(x + sample_codon[1:] for x in "ACGT"                     # another first base that changes the amino acid
                   if mirror.CODON_AA[codon_of(x + sample_codon[1:])] != mirror.CODON_AA[codon_of(sample_codon)])
    cfg["referenceSequence"] = ref[:c] + changed + ref[c + 3:]
    sample_aa = mirror.CODON_AA[codon_of(sample_codon)]
    gene["drms"] = [dict(name="minor", positions=[planted[0]]),
                    dict(name="fixed", positions=["%s%d%s" % (mirror.CODON_AA[codon_of(changed)], fixed_pos, sample_aa)])]
    json.dump(cfg, open(d / "cfg.json", "w"))
    subprocess.check_call([JULIET, "-c", "cfg.json", "--dump-msa", "in.msa", "in.bam"], cwd=d)      # host only
    rows, wb = read_msa(d / "in.msa")
    assert rows.shape == (N, L)
    r = juliet(d, "-c", "cfg.json", "--mode-phasing", "--max-perc", "90", "--haplotype-mutations", "--timing", "in.bam", "out.json", "out.html")
    assert r.returncode == 0, r.stderr
    assert "class_codons" in r.stderr                         # the stage line of --timing
    return dict(d=d, cfg=cfg, rows=rows, wb=wb, fixed_pos=fixed_pos, sample_codon=sample_codon, minor_pos=int(re.sub(r"\D", "", planted[0])),
                out=json.load(open(d / "out.json")))


def mirror_of(cfg, rows, wb, j):
    """The §24 leaves from the rows and the JSON's own haplotypes (read names -> labels)."""
    haps = j["haplotype"]["haplotypes"]
    lab = np.full(len(rows), 0xFFFF, dtype=np.uint16)
    for h, hp in enumerate(haps):
        idx = [int(name.split("/")[1]) for name in hp["read_names"]]
        assert len(idx) == hp["reads"]
        lab[idx] = h
    ref = cfg["referenceSequence"]
    positions = []
    for gi, g in enumerate(cfg["genes"]):
        for k in range((g["end"] - g["begin"]) // 3):
            c = g["begin"] - 1 + 3 * k - wb
            if c < 0 or c + 2 >= rows.shape[1]:
                continue
            codon = ref[c + wb:c + wb + 3].upper()
            positions.append(dict(gene_index=gi, gene=g["name"], position=k + 1, col=c, drms=g.get("drms", []),
                                  ref=codon_of(codon) if len(codon) == 3 and set(codon) <= set("ACGT") else None))
    cols = sorted({q["col"] for q in positions})
    hist = mirror.class_codons(rows, lab, len(haps), cols)[0] if haps else np.zeros((0, len(cols), 64), dtype=np.uint32)
    variant_rows, where = [], {(q["gene"], q["position"]): q["col"] for q in positions}
    for g in j["genes"]:
        for vp in g["variant_positions"]:
            for aa in vp["variant_amino_acids"]:
                for vc in aa["variant_codons"]:
                    variant_rows.append(dict(col=where[(g["name"], vp["ref_position"])], codon=codon_of(vc["codon"])))
    return mirror.front_end(hist, cols, positions, [hp["reads"] for hp in haps], [hp["frequency"] for hp in haps], variant_rows)


def variant_codons(j):
    return [vc for g in j["genes"] for vp in g["variant_positions"] for aa in vp["variant_amino_acids"] for vc in aa["variant_codons"]]


def test_fixed_and_minor_drms(sample):
    j = sample["out"]
    haps = j["haplotype"]["haplotypes"]
    assert len(haps) >= 3                                      # the mixture was chosen so that the test cannot pass vacuously
    # the fixed codon is no variant position under --max-perc 90: no gene table row, no haplotype codon names it
    assert all(vp["ref_position"] != sample["fixed_pos"] for g in j["genes"] for vp in g["variant_positions"])
    for hp in haps:
        (m,) = [m for m in hp["mutations"] if m["position"] == sample["fixed_pos"]]
        assert m["codon"] == sample["sample_codon"] and m["drms"] == ["fixed"] and m["frequency"] > 0.9
        assert "fixed" in hp["drugs"]
    with_minor = [hp["name"] for hp in haps if "minor" in hp["drugs"]]
    assert len(with_minor) == 1 and with_minor != [haps[0]["name"]]          # one clone, and not the major one
    for hp in haps:
        assert ("minor" in hp["drugs"]) == any(m["position"] == sample["minor_pos"] and "minor" in m["drms"] for m in hp["mutations"])
    prof = {p["drug"]: p for p in j["haplotype"]["drug_profile"]}
    assert list(prof) == ["fixed", "minor"]
    assert prof["fixed"]["haplotypes"] == [True] * len(haps) and prof["fixed"]["reads"] == sum(hp["reads"] for hp in haps)
    assert prof["minor"]["haplotypes"] == [hp["name"] in with_minor for hp in haps]
    assert prof["minor"]["reads"] == next(hp["reads"] for hp in haps if hp["name"] in with_minor)


def test_every_new_leaf_equals_the_mirror(sample):
    j = sample["out"]
    exp = mirror_of(sample["cfg"], sample["rows"], sample["wb"], j)
    haps = j["haplotype"]["haplotypes"]
    assert [hp["mutations"] for hp in haps] == exp["mutations"]
    assert [hp["drugs"] for hp in haps] == exp["drugs"]
    assert j["haplotype"]["drug_profile"] == exp["drug_profile"]
    rows = variant_codons(j)
    assert rows and [vc["haplotype_count"] for vc in rows] == exp["haplotype_count"]
    assert [vc["haplotype_coverage"] for vc in rows] == exp["haplotype_coverage"]
    for vc in rows:                                            # a fractional haplotype_hit: a hit haplotype carries the codon in every read
        for hit, cnt, cov in zip(vc["haplotype_hit"], vc["haplotype_count"], vc["haplotype_coverage"]):
            assert cnt <= cov and (not hit or cnt == cov > 0)


def strip_json(j):
    j["input"].pop("timestamp")
    j["input"].pop("command_line")
    for hp in j["haplotype"]["haplotypes"]:
        for key in NEW_HAP:
            hp.pop(key, None)
    j["haplotype"].pop("drug_profile", None)
    for vc in variant_codons(j):
        for key in NEW_ROW:
            vc.pop(key, None)
    return j


def strip_html(text):
    text = re.sub(r'\n<table id="hap-mutations">.*?</table>\n<table id="hap-drugs">.*?</table>\n<table id="hap-drug-profile">.*?</table>\n', "", text, flags=re.S)
    text = re.sub(r' data-count="\d+" data-coverage="\d+"', "", text)
    return "\n".join(line for line in text.split("\n") if "<th>timestamp</th>" not in line and "<th>command_line</th>" not in line)


def test_without_the_flag_nothing_changes(sample):
    d = sample["d"]
    r = juliet(d, "-c", "cfg.json", "--mode-phasing", "--max-perc", "90", "in.bam", "plain.json", "plain.html")
    assert r.returncode == 0, r.stderr
    plain = open(d / "plain.json").read()
    for key in NEW_HAP + NEW_ROW + ("drug_profile",):
        assert '"%s"' % key not in plain
    assert strip_json(json.load(open(d / "out.json"))) == strip_json(json.loads(plain))
    html_flagged, html_plain = open(d / "out.html").read(), open(d / "plain.html").read()
    assert 'id="hap-mutations"' in html_flagged and 'id="hap-mutations"' not in html_plain
    assert strip_html(html_flagged) == strip_html(html_plain)


def test_html_renders_the_new_leaves(sample):
    j, html = sample["out"], open(sample["d"] / "out.html").read()
    haps = j["haplotype"]["haplotypes"]
    table = re.search(r'<table id="hap-mutations">(.*?)</table>', html, flags=re.S).group(1)
    assert table.count("<tr data-haplotype=") == sum(len(hp["mutations"]) for hp in haps)
    m = haps[0]["mutations"][0]
    assert "<td>%s</td><td>%d</td><td>%s</td>" % (m["gene"], m["position"], m["ref_codon"]) in table
    prof = re.search(r'<table id="hap-drug-profile">(.*?)</table>', html, flags=re.S).group(1)
    for p in j["haplotype"]["drug_profile"]:
        assert "<td>%s</td>" % p["drug"] in prof and "<td>%d</td>" % p["reads"] in prof
    drugs = re.search(r'<table id="hap-drugs">(.*?)</table>', html, flags=re.S).group(1)
    assert drugs.count("<tr>") == len(haps) + 1
    pairs = re.findall(r'data-count="(\d+)" data-coverage="(\d+)"', html)
    exp = [(str(c), str(v)) for vc in variant_codons(j) for c, v in zip(vc["haplotype_count"], vc["haplotype_coverage"])]
    assert pairs == exp


@pytest.mark.parametrize("exe,args,word", [
    (JULIET, ["--haplotype-mutations"], "--mode-phasing"),
    (JULIET, ["--mode-phasing", "--haplotype-mutations", "--windows", "2"], "--windows"),
    (JULIET, ["--mode-phasing", "--haplotype-mutations", "--devices", "0,1"], "--devices"),
    (JULIET, ["--mode-phasing", "--haplotype-mutations", "--batch", "list.tsv"], "--batch"),
    (FUSE, ["--mode-phasing", "--haplotype-mutations"], "fuse"),
])
def test_refusals_come_before_any_file(tmp_path, exe, args, word):
    r = juliet(tmp_path, "-c", "none.json", *args, "missing.bam", "out.json", exe=exe)
    assert r.returncode == 1
    assert "--haplotype-mutations" in r.stderr and word in r.stderr
    assert os.listdir(tmp_path) == []


def test_no_reported_haplotype_gives_empty_arrays(tmp_path):
    subprocess.check_call([SYNTH, "--reads", "400", "--cols", "90", "--seed", "3", "--minor-permille", "0", "0", "0", "0",
                           "-o", str(tmp_path / "in.bam"), "--config-out", str(tmp_path / "cfg.json")])
    r = juliet(tmp_path, "-c", "cfg.json", "--mode-phasing", "--haplotype-mutations", "in.bam", "out.json", "out.html")
    assert r.returncode == 0, r.stderr
    j = json.load(open(tmp_path / "out.json"))
    assert j["haplotype"]["haplotypes"] == [] and j["haplotype"]["drug_profile"] == []
    for vc in variant_codons(j):
        assert vc["haplotype_count"] == [] and vc["haplotype_coverage"] == []
