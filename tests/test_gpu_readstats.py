"""jl_read_stats_async on the device (docs/SPEC.md §20): per read of the resident matrix its bases, gaps, masked cells, compared
bases and mismatches over the whole window; jl_read_filter and jl_msa_take on top of it; and the front end's read filter.  Every
expectation is tests/readstats_mirror.py — five comparisons and a sum in numpy — over the rows that were uploaded, compared for
equality on every entry; never another device result.  The sizes are the edges of the launch shape, named by the function the
launcher calls (tests/readstats_shape.py): a workgroup owns 2048 reads (a lane one 32-read word), a column segment at most 255
columns and, in a longer window, at least 64; the bit-sliced counters are flushed every F = 2^k - 1 columns."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import readstats_mirror as rm
import readstats_shape
from minorseq_amd import capi, msa, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JULIET = os.path.join(ROOT, "minorseq_amd", "bin", "juliet")
SYNTH = os.path.join(ROOT, "minorseq_amd", "bin", "juliet-synth")
F = readstats_shape.shape(97, 64)["flush"]
WG = readstats_shape.shape(97, 64)["wg_reads"]
SEG = readstats_shape.shape(1025, 3000)["seg_cols"]      # the columns of a segment at 1025 reads: the smallest a long window gets


@pytest.fixture(scope="module", autouse=True)
def built():
    """The binaries normally travel with the tree; build them only if they are missing (never under a loaded .so)."""
    if not os.path.exists(os.path.join(ROOT, "minorseq_amd", "libjuliet_hip.so")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "csrc")])
    if not (os.path.exists(JULIET) and os.path.exists(SYNTH)):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "host")])


@pytest.fixture(scope="module")
def ctx():
    j = capi.Juliet(0)
    yield j
    j.close()


def random_case(n, n_cols, seed):
    """All seven codes at random, and a compare row of all six meanings (0..3, 4, 5) with some bytes beyond."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 7, size=(n, n_cols), dtype=np.uint8)
    compare = rng.integers(0, 6, size=n_cols, dtype=np.uint8)
    compare[rng.random(n_cols) < 0.1] = 0xFF
    return rows, compare


def check(j, rows, compare):
    exp = rm.stats(rows, compare)
    got = j.read_stats(compare)
    assert got.dtype == np.uint32 and got.shape == (5, rows.shape[0])
    assert (got == exp).all(), np.argwhere(got != exp)[:8]
    return got


# ---------------------------------------------------------------------------------------------- the counters
@pytest.mark.parametrize("n_cols", [F - 1, F, F + 1, 2 * F + 1])
def test_staircase(ctx, n_cols):
    """Read r carries exactly r mod (n_cols + 1) mismatches, at its first columns; then the same staircase of gaps, and of N: every
    count value, every carry 2^j - 1 -> 2^j, and counts that straddle a flush (and, at 2F + 1, a segment)."""
    n = 97
    assert F == 2 ** readstats_shape.shape(n, n_cols)["k"] - 1 and n_cols > 0
    rng = np.random.default_rng(n_cols)
    compare = rng.integers(0, 4, size=n_cols, dtype=np.uint8)
    steps = (np.arange(n) % (n_cols + 1))[:, None] > np.arange(n_cols)[None, :]          # read r: its first r mod (n_cols + 1) columns
    wrong = ((compare + 1 + rng.integers(0, 3, size=n_cols)) % 4).astype(np.uint8)      # a base of the column that is not its compare code
    for kind in ("mismatch", "gap", "n"):
        rows = np.repeat(compare[None, :], n, axis=0)
        rows[steps] = {"mismatch": np.repeat(wrong[None, :], n, axis=0), "gap": np.full((n, n_cols), 4, dtype=np.uint8),
                       "n": np.full((n, n_cols), 5, dtype=np.uint8)}[kind][steps]
        ctx.upload_rows(rows)
        got = check(ctx, rows, compare)
        want = (np.arange(n) % (n_cols + 1)).astype(np.uint32)
        assert (got[{"mismatch": rm.MISMATCHES, "gap": rm.GAPS, "n": rm.MASKED}[kind]] == want).all()      # the staircase itself
        assert set(want.tolist()) == set(range(min(n, n_cols + 1)))


@pytest.mark.parametrize("n", [1, 31, 32, 33, 511, 512, 513, 1024, 1025, WG - 1, WG, WG + 1])
def test_read_edges(ctx, n):
    rows, compare = random_case(n, 7, 100 + n)
    ctx.upload_rows(rows, win_begin=5)
    check(ctx, rows, compare)
    assert (msa.unpack_columns(ctx.download_columns(), n) == rows).all()     # the matrix is untouched


@pytest.mark.parametrize("n_cols", [1, 2, SEG - 1, SEG, SEG + 1, 2 * SEG + 1])
def test_column_edges(ctx, n_cols):
    n = 1025
    s = readstats_shape.shape(n, n_cols)
    assert s["n_segs"] == -(-n_cols // SEG) and s["seg_cols"] == min(SEG, n_cols)       # the cases are the edges they claim to be
    rows, compare = random_case(n, n_cols, 200 + n_cols)
    ctx.upload_rows(rows)
    check(ctx, rows, compare)


def test_adopted_matrix_with_its_own_stride():
    """A torch tensor as the matrix: 2049 reads in planes of 272 bytes (the library's own stride is 384; 272 is no multiple of the
    64-byte tile); every bit past the last read holds a base that differs from the compare row.  None of it may show."""
    import torch
    n, n_cols, stride = 2049, 131, 272
    assert stride > (n + 7) // 8 and stride != msa.plane_stride(n) and stride % 64 != 0 and stride % 16 == 0
    rows, compare = random_case(n, n_cols, 99)
    compare = (compare % 4).astype(np.uint8)                                  # every column is compared
    pad = 8 * stride - n
    wrong = np.repeat(((compare + 1) % 4)[None, :], pad, axis=0)              # a base, and not the compare row's
    planes = msa.pack_planes(np.concatenate([rows, wrong]), stride)
    assert planes.shape == (n_cols, 3, stride)
    assert (msa.unpack_planes(planes, n + pad)[n:] == wrong).all()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t = torch.from_numpy(planes).cuda(non_blocking=False)
    stream.synchronize()
    j = capi.Juliet(0, stream=stream.cuda_stream)
    j.adopt(t.data_ptr(), n, n_cols, stride, keep_alive=t)
    check(j, rows, compare)
    j.close()


def test_compare_row(ctx):
    """Every meaning of a compare byte; no row at all; and the output of jl_consensus_fetch passed as it is."""
    n, n_cols = 700, 40
    rows, _ = random_case(n, n_cols, 7)
    rows[:, 3] = 6                                                            # a column nobody covers: consensus 5
    rows[:, 4] = 4                                                            # a majority deletion: consensus 4
    rows[:5, 4] = 2
    compare = np.array(([0, 1, 2, 3, 4, 5, 0xFF, 200] * 5), dtype=np.uint8)
    ctx.upload_rows(rows)
    got = check(ctx, rows, compare)
    assert got[rm.COMPARED].any() and got[rm.MISMATCHES].any() and (got[rm.COMPARED] < got[rm.BASES]).any()
    none = ctx.read_stats(None)
    assert (none == rm.stats(rows, None)).all() and not none[rm.COMPARED:].any() and none[rm.BASES].any()
    ctx.pileup_async(np.array([(1, n_cols + 1)], dtype=capi.GENE))
    cons = ctx.consensus()
    assert (cons == rm.consensus(rows)).all() and cons[3] == 5 and cons[4] == 4
    check(ctx, rows, cons)


def test_additivity_over_column_windows(ctx):
    n, n_cols = 1000, 300
    rows, compare = random_case(n, n_cols, 21)
    ctx.upload_rows(rows)
    whole = check(ctx, rows, compare).astype(np.int64)
    total = np.zeros_like(whole)
    for lo, hi in ((0, 150), (150, 300)):
        ctx.upload_rows(rows[:, lo:hi], win_begin=lo)
        total += check(ctx, rows[:, lo:hi], compare[lo:hi])
    assert (total == whole).all()


def test_longest_segments_of_a_deep_window():
    """So many reads that the chunks alone fill the chip: the segments are the longest a byte counter allows, 255 columns, and a
    read that is bases throughout counts 255 in one.  Filled on the device; no rows on the host at this size: 3000 reads of it are
    taken into a second window (jl_msa_take), downloaded, and their mirror compared with the same reads' entries of the deep table."""
    n, l = 2048 * 1025, 300
    s = readstats_shape.shape(n, l)
    assert s["seg_cols"] == readstats_shape.SEG_COLS_MAX == 255 and s["n_segs"] == 2 and s["n_chunks"] == 1025
    ref = synth.reference(3, l)
    j, part = capi.Juliet(0), capi.Juliet(0)
    j.alloc(n, l)
    j.synth_fill(synth.SynthParams(seed=3, del_rate=4e-3, mask_rate=1e-2, partial_rate=0.05, minor_permille=(60, 50, 40, 30)), ref)
    deep = j.read_stats(ref)
    idx = np.sort(np.random.default_rng(3).choice(n, size=3000, replace=False)).astype(np.uint32)
    idx[:3], idx[-3:] = (0, 1, 2), (n - 3, n - 2, n - 1)
    part.take([(j, idx)])
    rows = msa.unpack_columns(part.download_columns(), len(idx))
    exp = rm.stats(rows, ref)
    assert (deep[:, idx] == exp).all(), np.argwhere(deep[:, idx] != exp)[:8]
    assert exp[rm.MISMATCHES].any() and exp[rm.GAPS].any() and exp[rm.MASKED].any()
    assert int(deep[rm.BASES].max()) == l and (deep[:3].astype(np.int64).sum(axis=0) <= l).all()      # 255 + 45 in some read
    part.close()
    j.close()


def test_repeated_growing_and_deferred_calls(ctx):
    for n, n_cols in ((40, 9), (5000, 200), (40, 9)):
        rows, compare = random_case(n, n_cols, n + n_cols)
        ctx.upload_rows(rows)
        check(ctx, rows, compare)
        check(ctx, rows, compare)
    assert ctx.read_stats(compare, wait=False) is None
    assert (ctx.read_stats_fetch() == rm.stats(rows, compare)).all()


def test_refusals():
    lib = capi.load_library()
    j = capi.Juliet(0)
    assert lib.jl_read_stats_async(j.h, None) == -4 and "no resident matrix" in lib.jl_last_error(j.h).decode()
    rows, compare = random_case(40, 9, 1)
    j.upload_rows(rows)
    with pytest.raises(capi.JulietError) as e:                       # a fetch before any call
        j.read_stats_fetch()
    assert e.value.status == -4 and "before jl_read_stats_async" in str(e.value)
    good = check(j, rows, compare)
    assert lib.jl_read_stats_fetch(j.h, None) == 0                   # NULL: only wait
    assert (j.read_stats_fetch() == good).all()
    j.close()


def fetch_copy(j):
    out = j.run_fetch(True, True, cap_var=256)
    return dict(variants=out["variants"].copy(), phase={k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in out["phase"].items()})


def assert_same_run(a, b):
    assert (a["variants"] == b["variants"]).all()
    pa, pb = a["phase"], b["phase"]
    assert pa["summary"] == pb["summary"]
    for key in ("pos_cols", "hap_count", "hap_pattern", "hit", "read_hap", "cooc"):
        assert (pa[key] == pb[key]).all(), key


def test_nothing_else_moves(ctx):
    """A run, its results, the stage, the results again, and a replay of the captured graph: all identical.  A second call with
    another compare row replaces the first."""
    n, l = 5000, 300
    sp = synth.SynthParams(seed=5, del_rate=4e-3, mask_rate=2e-2, partial_rate=0.1, minor_permille=(150, 120, 100, 80))
    ref = synth.reference(sp.seed, l)
    genes = np.array([(1, l + 1)], dtype=capi.GENE)
    ctx.alloc(n, l)
    ctx.synth_fill(sp, ref)
    before = ctx.download_columns().copy()
    rows = msa.unpack_columns(before, n)
    ctx.run_async(genes, ref, capi.default_params(), None, True, 10, True)
    first = fetch_copy(ctx)
    assert len(first["variants"]) >= 4
    got = check(ctx, rows, ref)
    assert got[rm.MISMATCHES].any() and got[rm.GAPS].any() and got[rm.MASKED].any()
    assert_same_run(first, fetch_copy(ctx))
    assert (ctx.download_columns() == before).all()
    other = ((ref + 1) % 4).astype(np.uint8)
    replaced = check(ctx, rows, other)                               # another compare row: the first table is gone
    assert (replaced[rm.MISMATCHES] != got[rm.MISMATCHES]).any() and (replaced[:rm.COMPARED] == got[:rm.COMPARED]).all()
    ctx.run_async(genes, ref, capi.default_params(), None, True, 10, True)
    assert_same_run(first, fetch_copy(ctx))
    ctx.run_async(genes, ref, capi.default_params(), None, True, 10, True)   # (a configuration is captured on its second run: the replay)
    assert_same_run(first, fetch_copy(ctx))
    assert (ctx.read_stats_fetch() == replaced).all()                # ... and the runs left the stage's table alone


def test_composition_with_filter_and_take(ctx):
    """stats -> read_filter -> jl_msa_take: the pileup of the taken window is the mirror's pileup of the kept rows."""
    n, l = 3000, 120
    sp = synth.SynthParams(seed=8, del_rate=4e-3, mask_rate=2e-2, partial_rate=0.2, minor_permille=(80, 60, 50, 40))
    ref = synth.reference(sp.seed, l)
    rows = synth.rows(sp, l, 0, n, ref)
    ctx.upload_rows(rows)
    st = check(ctx, rows, ref)
    rule = dict(min_bases=100, max_mismatches=2, max_gap_perc=1.0, max_masked_perc=3.0)
    idx, failed = capi.read_filter(st, **rule)
    exp_idx, exp_failed = rm.read_filter(rm.stats(rows, ref), **rule)
    assert idx.tolist() == exp_idx.tolist() and failed.tolist() == exp_failed.tolist()
    assert 0 < len(idx) < n and (failed > 0).sum() >= 3
    taken = capi.Juliet(0)
    taken.take([(ctx, idx)])
    taken.pileup_async(np.array([(1, l + 1)], dtype=capi.GENE))
    assert (taken.pileup_fetch()["col_counts"] == rm.column_counts(rows[exp_idx])).all()
    check(taken, rows[exp_idx], ref)                                 # ... and the stage on the taken window
    taken.close()


# ---------------------------------------------------------------------------------------------- the command line
N_CLI, L_CLI, SEED_CLI, REF_SEED = 2000, 600, 41, 77
MINOR = (80, 60, 50, 40)


def juliet(d, *args):
    return subprocess.run([JULIET, *args], cwd=d, capture_output=True, text=True, timeout=120)


# the rule the tests run with: keep the reads that agree with the majority everywhere (no minor variant survives it: the called
# table of the kept window is empty), and a second rule of two bounds that leaves minor variants to call and phase
RULE_STRICT = (("--max-read-mismatches", "0"), dict(max_mismatches=0), {"mismatches": 0})
RULE_LOOSE = (("--max-read-mismatches", "2", "--max-read-gap-perc", "0.2"), dict(max_mismatches=2, max_gap_perc=0.2), {"mismatches": 2, "gap_perc": 0.2})


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    d = tmp_path_factory.mktemp("readstats_cli")
    subprocess.check_call([SYNTH, "--reads", str(N_CLI), "--cols", str(L_CLI), "--seed", str(SEED_CLI), "--ref-seed", str(REF_SEED),
                           "--partial", "0.1", "--minor-permille", *map(str, MINOR), "-o", str(d / "a.bam")])
    # a config without a reference sequence: the compare row is the majority of the window
    json.dump({"genes": [dict(name="G", begin=1, end=L_CLI + 1, drms=[])], "referenceName": "synthetic_ref",
               "version": "tests/test_gpu_readstats.py", "databaseVersion": "none"}, open(d / "cfg.json", "w"))
    rows = synth.rows(synth.SynthParams(seed=SEED_CLI, partial_rate=0.1, minor_permille=MINOR), L_CLI, 0, N_CLI, synth.reference(REF_SEED, L_CLI))
    r = juliet(d, "-c", "cfg.json", "--mode-phasing", *RULE_STRICT[0], "--read-stats", "s.tsv", "a.bam", "f.json", "f.html")
    assert r.returncode == 0, r.stderr
    r = juliet(d, "-c", "cfg.json", "--mode-phasing", *RULE_LOOSE[0], "a.bam", "g.json", "g.html")
    assert r.returncode == 0, r.stderr
    return d, rows


def json_number(v):
    """A number as the JSON writer prints it."""
    return "%.0f" % v if v == int(v) else "%.17g" % v


def python_path(rows, rule):
    """The same steps through the Python binding: the stats of every read, the kept reads, the rule counts, the run of the taken window."""
    j, taken = capi.Juliet(0), capi.Juliet(0)
    j.upload_rows(rows)
    genes = np.array([(1, L_CLI + 1)], dtype=capi.GENE)
    j.pileup_async(genes)
    st = j.read_stats(j.consensus())
    idx, failed = capi.read_filter(st, **rule)
    taken.take([(j, idx)])
    out = taken.run(genes, None, capi.default_params(), phasing=True)
    j.close()
    taken.close()
    return st, idx, failed, out


def assert_cli_is_python_path_and_mirror(d, rows, name, rule):
    """The JSON and HTML `name` of a run with `rule`; returns the stats of the Python path and the number of called variants."""
    st, idx, failed, out = python_path(rows, rule[1])
    exp_st = rm.stats(rows, rm.consensus(rows))
    exp_idx, exp_failed = rm.read_filter(exp_st, **rule[1])
    assert (st == exp_st).all() and idx.tolist() == exp_idx.tolist() and failed.tolist() == exp_failed.tolist()
    assert 0 < len(exp_idx) < N_CLI                                   # a filter that does nothing cannot pass
    j = json.load(open(d / (name + ".json")))
    rf = j["input"]["read_filter"]
    assert list(rf) == ["compare", "rule", "reads", "kept", "failed"]
    assert rf["compare"] == "majority" and rf["rule"] == rule[2] and rf["reads"] == N_CLI and rf["kept"] == len(exp_idx)
    assert rf["failed"] == dict(zip(rm.RULES, (int(x) for x in exp_failed)))
    assert j["target_config"]["n_reads"] == len(exp_idx)
    # the gene and haplotype blocks: those of the run on the taken window
    var, ph = out["variants"], out["phase"]
    got = sorted(((gi, vp["ref_position"], msa.codon_index(vc["codon"]), vc, vp) for gi, g in enumerate(j["genes"]) for vp in g["variant_positions"]
                  for aa in vp["variant_amino_acids"] for vc in aa["variant_codons"]), key=lambda r: r[:3])
    assert len(got) == len(var)
    for k, ((gi, pos, cod, vc, vp), e) in enumerate(zip(got, var)):
        assert (gi, pos, cod) == (e["gene"], e["codon_pos"], e["codon"])
        assert vc["count"] == e["count"] and vp["coverage"] == e["coverage"] and vc["expected"] == e["expected"]
        assert abs(vc["pValue"] - e["p_value"]) <= 1e-12 * max(e["p_value"], 1e-300)
        assert vc["haplotype_hit"] == [bool(x) for x in ph["hit"][k]]
    hb, s = j.get("haplotype", {}), ph["summary"]
    haps = hb.get("haplotypes", [])
    assert [h["reads"] for h in haps] == ph["hap_count"].tolist()
    if haps or len(var):
        assert (hb["reported_reads"], hb["insufficient_coverage_reads"], hb["damaged_reads"]) == (s["reported_reads"], s["insufficient_reads"], s["damaged_reads"])
    read_hap = np.asarray(ph["read_hap"])[:len(idx)]
    for hi, h in enumerate(haps):
        assert [msa.codon_index(c) for c in h["codons"]] == ph["hap_pattern"][hi].tolist()
        assert [int(n.split("/")[1]) for n in h["read_names"]] == idx[np.nonzero(read_hap == hi)[0]].tolist()      # names follow the kept indices
    # the HTML renders the same leaves
    html = open(d / (name + ".html")).read()
    m = re.search(r'<table id="read-filter-table" data-compare="majority">.*?</table>', html, flags=re.S)
    assert m and f"<td>reads</td><td></td><td>{N_CLI}</td>" in m.group(0) and f"<td>kept</td><td></td><td>{len(exp_idx)}</td>" in m.group(0)
    for r, rname in enumerate(rm.RULES):
        bound = json_number(rule[2][rname]) if rname in rule[2] else ""
        assert f"<td>{rname}</td><td>{bound}</td><td>{int(exp_failed[r])}</td>" in m.group(0), (rname, m.group(0))
    return st, len(var), len(haps)


def test_cli_equals_the_python_path_and_the_mirror(cli):
    d, rows = cli
    st, n_var, n_hap = assert_cli_is_python_path_and_mirror(d, rows, "f", RULE_STRICT)
    # the TSV: one line per read of the loaded sample, in input order
    lines = open(d / "s.tsv").read().splitlines()
    assert len(lines) == N_CLI
    for i, line in enumerate(lines):
        name, *nums = line.split("\t")
        assert int(name.split("/")[1]) == i and [int(x) for x in nums] == st[:, i].tolist(), (i, line)


def test_cli_two_rules_leave_variants_to_call_and_phase(cli):
    d, rows = cli
    st, n_var, n_hap = assert_cli_is_python_path_and_mirror(d, rows, "g", RULE_LOOSE)
    assert n_var >= 1 and n_hap >= 2


def strip(path):
    j = json.load(open(path))
    j["input"].pop("timestamp")
    j["input"].pop("command_line")
    return j


def test_cli_stats_alone_and_rules_that_drop_nothing_change_nothing_else(cli):
    d, rows = cli
    for out, args in (("plain", ()), ("only", ("--read-stats", "only.tsv")), ("loose", ("--max-read-mismatches", str(L_CLI)))):
        r = juliet(d, "-c", "cfg.json", "--mode-phasing", *args, "a.bam", out + ".json")
        assert r.returncode == 0, r.stderr
    plain, only, loose = strip(d / "plain.json"), strip(d / "only.json"), strip(d / "loose.json")
    assert "read_filter" not in plain["input"]
    assert open(d / "only.tsv").read() == open(d / "s.tsv").read()
    for other in (only, loose):
        rf = other["input"].pop("read_filter")
        assert rf["kept"] == rf["reads"] == N_CLI and not any(rf["failed"].values())
        assert other == plain


def test_cli_no_read_kept_is_an_input_error(cli):
    d, rows = cli
    r = juliet(d, "-c", "cfg.json", "--min-read-bases", str(L_CLI + 1), "a.bam", "none.json")
    assert r.returncode == 2 and "keeps none" in r.stderr and f"min_bases {N_CLI}" in r.stderr, (r.returncode, r.stderr)
    assert not (d / "none.json").exists()


def test_cli_batch_filters_every_sample(cli):
    d, rows = cli
    (d / "l.tsv").write_text("a.bam\tb1.json\na.bam\tb2.json\n")
    r = juliet(d, "-c", "cfg.json", "--mode-phasing", "--max-read-mismatches", "0", "--batch", "l.tsv")
    assert r.returncode == 0, r.stderr
    single = strip(d / "f.json")
    for name in ("b1.json", "b2.json"):
        assert strip(d / name) == single


@pytest.mark.parametrize("args", [["--windows", "2"], ["--mix", "b.bam"], ["--devices", "0,0"], ["--consensus", "c.fasta"], ["--call-insertions"]])
def test_cli_refused_combinations_open_nothing(tmp_path, args):
    for rule in (["--max-read-mismatches", "0"], ["--read-stats", "s.tsv"]):
        r = juliet(tmp_path, *rule, *args, "no_such.bam", "o.json")
        assert r.returncode == 1 and ("read filter" in r.stderr or "--read-stats" in r.stderr), (r.returncode, r.stderr)
        assert not list(tmp_path.iterdir())


def test_cli_refused_as_fuse_and_stats_with_batch(tmp_path):
    (tmp_path / "l.tsv").write_text("no_such.bam\ta.json\n")
    r = juliet(tmp_path, "--read-stats", "s.tsv", "--batch", "l.tsv")
    assert r.returncode == 1 and "--batch" in r.stderr
    r = subprocess.run([os.path.join(ROOT, "minorseq_amd", "bin", "fuse"), "--max-read-gap-perc", "5", "no_such.bam", "o.fasta"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "fuse" in r.stderr
    r = juliet(tmp_path, "--max-read-n-perc", "100.5", "no_such.bam", "o.json")
    assert r.returncode == 1 and "[0, 100]" in r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == ["l.tsv"]
