"""`juliet --batch samples.tsv`: many per-barcode BAMs in one process.  Every sample's files must equal what a single
`juliet [same options] in.bam out...` writes (up to the run's own timestamp and command line), whichever way the batch ran
the sample: in a group run with other samples of the same group key, or alone."""
import json
import os
import re
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JULIET = os.path.join(ROOT, "minorseq_amd", "bin", "juliet")
SYNTH = os.path.join(ROOT, "minorseq_amd", "bin", "juliet-synth")
L, REF_SEED = 900, 77
TIMING = re.compile(r"juliet: timing batch (group|single) +(\d+) samples +lines ([\d,]+) ")


@pytest.fixture(scope="module", autouse=True)
def built():
    """The binaries normally travel with the tree; build them only if they are missing (never under a loaded .so)."""
    if not os.path.exists(os.path.join(ROOT, "minorseq_amd", "libjuliet_hip.so")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "csrc")])
    if not (os.path.exists(JULIET) and os.path.exists(SYNTH)):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "host")])


def synth(d, name, reads, seed, *extra, cfg=None):
    """One sample over the shared reference (--ref-seed): one config fits every sample."""
    args = [SYNTH, "--reads", str(reads), "--cols", str(L), "--seed", str(seed), "--ref-seed", str(REF_SEED),
            "--partial", "0.1", *extra, "-o", str(d / name)]
    if cfg:
        args += ["--config-out", str(d / cfg)]
    subprocess.check_call(args)
    return name


def make_set(d, prefix, *extra):
    """12 samples, 2000 .. 9000 reads, two of them without any minor haplotype."""
    names = []
    for k in range(12):
        minor = ["--minor-permille", "0", "0", "0", "0"] if k in (3, 9) else ["--minor-permille", "60", "50", "40", "30"]
        names.append(synth(d, f"{prefix}{k:02d}.bam", 2000 + k * 7000 // 11, 100 + k, *minor, *extra,
                           cfg="cfg.json" if k == 0 else None))
    return names


@pytest.fixture(scope="module")
def samples(tmp_path_factory):
    d = tmp_path_factory.mktemp("batch")
    return d, make_set(d, "s"), make_set(d, "q", "--rich-qv")


def norm_json(path):
    j = json.load(open(path))
    j["input"].pop("timestamp")
    j["input"].pop("command_line")
    return j


def norm_html(path):
    return re.sub(r"(<tr><th>(?:timestamp|command_line)</th>)<td>.*?</td>", r"\1<td></td>", open(path).read())


def same_file(a, b):
    if a.endswith(".json"):
        return norm_json(a) == norm_json(b)
    return norm_html(a) == norm_html(b)


def write_list(d, name, rows):
    with open(d / name, "w") as f:
        f.write("# sample list\n\n")
        for bam, outs in rows:
            f.write("\t".join([bam, *outs]) + "\n")
    return name


def run_batch(d, opts, list_name):
    return subprocess.run([JULIET, *opts, "--timing", "--batch", list_name], cwd=d, capture_output=True, text=True, timeout=600)


def single(d, opts, bam, outs):
    r = subprocess.run([JULIET, *opts, bam, *outs], cwd=d, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def dispatches(stderr):
    """(kind, [list lines]) of every device dispatch the batch reported."""
    return [(m.group(1), [int(x) for x in m.group(3).split(",")]) for m in TIMING.finditer(stderr)]


def check_against_singles(d, opts, rows, tag):
    for bam, outs in rows:
        ref = [f"{tag}_ref_{o}" for o in outs]
        single(d, opts, bam, ref)
        for o, r in zip(outs, ref):
            assert os.path.exists(d / o), o
            assert same_file(str(d / o), str(d / r)), (bam, o)


def lines_of(d, list_name):
    """list line number of every sample line, in order"""
    out = []
    for no, text in enumerate(open(d / list_name).read().split("\n"), 1):
        if text.strip() and not text.startswith("#"):
            out.append(no)
    return out


CASES = {
    "phasing": (["-c", "cfg.json", "--mode-phasing"], "s"),
    "call": (["-c", "cfg.json"], "s"),
    "drm_phasing": (["-c", "cfg.json", "--drm-only", "--mode-phasing"], "s"),
    "richqv_minqv": (["-c", "cfg.json", "--min-qv", "20", "--mode-phasing"], "q"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_batch_equals_single_runs(samples, case):
    d, plain, rich = samples
    opts, which = CASES[case]
    bams = plain if which == "s" else rich
    rows = [(b, [f"{case}_{b}.json", f"{case}_{b}.html"]) for b in bams]
    lst = write_list(d, f"{case}.tsv", rows)
    r = run_batch(d, opts, lst)
    assert r.returncode == 0, r.stderr
    seen = sorted(x for _, ls in dispatches(r.stderr) for x in ls)
    assert seen == lines_of(d, lst), r.stderr          # every sample in exactly one group or single dispatch
    check_against_singles(d, opts, rows, case)
    j = json.load(open(d / rows[0][1][0]))
    assert j["input"]["input_file"] == bams[0] and "--batch" in j["input"]["command_line"]
    assert j["genes"][0]["variant_positions"]


def test_batch_groups_samples_of_one_key(samples):
    """With one config and one amplicon every sample has the same group key: the batch runs them in group runs."""
    d, plain, _ = samples
    rows = [(b, [f"grp_{b}.json"]) for b in plain]
    r = run_batch(d, ["-c", "cfg.json", "--mode-phasing"], write_list(d, "grp.tsv", rows))
    assert r.returncode == 0, r.stderr
    ds = dispatches(r.stderr)
    assert any(kind == "group" and len(ls) >= 2 for kind, ls in ds), r.stderr
    assert all(len(ls) <= 8 for _, ls in ds)
    assert sorted(x for _, ls in ds for x in ls) == lines_of(d, "grp.tsv")


def test_batch_without_config(samples):
    """No -c: each sample's ORF `unknown` spans its own reads; the outputs are still those of single runs."""
    d, plain, _ = samples
    rows = [(b, [f"nocfg_{b}.json", f"nocfg_{b}.html"]) for b in plain]
    r = run_batch(d, ["--mode-phasing"], write_list(d, "nocfg.tsv", rows))
    assert r.returncode == 0, r.stderr
    assert sorted(x for _, ls in dispatches(r.stderr) for x in ls) == lines_of(d, "nocfg.tsv")
    check_against_singles(d, ["--mode-phasing"], rows, "nocfg")
    assert json.load(open(d / rows[0][1][0]))["genes"][0]["name"] == "unknown"


def test_batch_longer_than_pool_and_group(tmp_path):
    """40 samples: more than the pool of contexts and than one group run; every context is refilled several times."""
    d = tmp_path
    bams = [synth(d, f"m{k:02d}.bam", 1500, 500 + k, "--minor-permille", "60", "50", "40", "30",
                  cfg="cfg.json" if k == 0 else None) for k in range(40)]
    rows = [(b, [f"long_{b}.json"]) for b in bams]
    opts = ["-c", "cfg.json", "--mode-phasing"]
    r = run_batch(d, opts, write_list(d, "long.tsv", rows))
    assert r.returncode == 0, r.stderr
    ds = dispatches(r.stderr)
    assert sorted(x for _, ls in ds for x in ls) == lines_of(d, "long.tsv")
    assert sum(1 for kind, ls in ds if kind == "group") >= 3, r.stderr
    check_against_singles(d, opts, rows, "long")


def test_batch_one_bad_sample(samples, tmp_path):
    """A truncated BAM, a BAM without alignments and an output that cannot be written, in the middle of the list: each is
    named on stderr by its line, every other sample is written as a single run writes it, and the exit status is 2."""
    d, plain, _ = samples
    shutil.copy(d / plain[4], tmp_path / "whole.bam")
    for b in plain[:8]:
        shutil.copy(d / b, tmp_path / b)
    shutil.copy(d / "cfg.json", tmp_path / "cfg.json")
    data = open(tmp_path / "whole.bam", "rb").read()
    open(tmp_path / "cut.bam", "wb").write(data[: len(data) // 2])
    synth(tmp_path, "empty.bam", 0, 3)
    rows = [(plain[0], ["bad_0.json"]), (plain[1], ["bad_1.json", "bad_1.html"]), ("cut.bam", ["bad_cut.json"]),
            (plain[2], ["bad_2.json"]), ("empty.bam", ["bad_empty.json"]), (plain[5], ["no_such_dir/bad_5.json"]),
            (plain[6], ["bad_6.json"]), ("missing.bam", ["bad_missing.json"]), (plain[7], ["bad_7.json"])]
    opts = ["-c", "cfg.json", "--mode-phasing"]
    lst = write_list(tmp_path, "bad.tsv", rows)
    r = run_batch(tmp_path, opts, lst)
    assert r.returncode == 2, r.stderr
    nos = lines_of(tmp_path, lst)
    for k, (bam, _) in enumerate(rows):
        named = f"batch line {nos[k]} ({bam})" in r.stderr
        assert named == (k in (2, 4, 5, 7)), (k, r.stderr)
    good = [row for k, row in enumerate(rows) if k not in (2, 4, 5, 7)]
    check_against_singles(tmp_path, opts, good, "bad")
    assert not os.path.exists(tmp_path / "bad_cut.json") and not os.path.exists(tmp_path / "bad_empty.json")
