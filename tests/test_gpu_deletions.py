"""jl_codon_deletions_async on the device (docs/SPEC.md §16): at every codon start the reads with a whole codon, a whole-codon
deletion, a partly deleted codon and the reads spanning it, and `juliet --call-deletions` on top of it.  Every expectation is
tests/deletion_mirror.py — the rule in plain numpy, the test in exact arithmetic — over the rows that were uploaded, compared for
equality on every entry; never another device result."""
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import deletion_mirror as dm
from minorseq_amd import capi, msa, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JULIET = os.path.join(ROOT, "minorseq_amd", "bin", "juliet")
SYNTH = os.path.join(ROOT, "minorseq_amd", "bin", "juliet-synth")
GAP = 4


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


def make_case(n, n_cols, seed, n_hap=4):
    """Reads that are copies of a few haplotype rows of bases, with seeded damage by kind of read: a clean codon deletion at a
    start of any of the three frames, a one-base and a two-base deletion, a six-base deletion, scattered N cells, ragged code-6
    ends, code 6 throughout; four kinds in ten stay clean.  Then three cells are planted so that the smallest case has a whole
    codon, a deleted one and a partly deleted one: at columns 0..2 of reads 0, 1, 2, or along the only read."""
    rng = np.random.default_rng(seed)
    haps = rng.integers(0, 4, size=(n_hap, n_cols), dtype=np.uint8)
    rows = haps[rng.integers(0, n_hap, size=n)].copy()
    kind = rng.integers(0, 10, size=n)
    ci = np.arange(n_cols)[None, :]
    for k, length in ((0, 3), (1, 1), (2, 2), (3, 6)):
        if n_cols < length:
            continue
        start = rng.integers(0, n_cols - length + 1, size=n)[:, None]
        rows[(kind == k)[:, None] & (ci >= start) & (ci < start + length)] = GAP
    rows[(kind == 4)[:, None] & (rng.random(size=rows.shape) < 2.0 / n_cols)] = 5
    lo, hi = rng.integers(0, n_cols // 3 + 1, size=n), n_cols - rng.integers(0, n_cols // 3 + 1, size=n)
    rows[(kind == 5)[:, None] & ((ci < lo[:, None]) | (ci >= hi[:, None]))] = 6
    rows[kind == 6] = 6
    if n >= 3:
        rows[0, :3], rows[1, :3], rows[2, :3] = haps[0, :3], GAP, (GAP, haps[0, 1], haps[0, 2])
    else:
        assert n_cols >= 7
        rows[0, :7] = (haps[0, 0], haps[0, 1], haps[0, 2], GAP, GAP, GAP, haps[0, 6])
    return rows


def check(j, rows):
    exp = dm.counts(rows)
    assert exp[:, dm.CODON].any() and exp[:, dm.DEL3].any() and exp[:, dm.PARTIAL].any()      # nothing passes vacuously
    got = j.codon_deletions()
    assert got.dtype == np.uint32 and got.shape == (rows.shape[1] - 2, 4)
    assert (got == exp).all(), np.argwhere(got != exp)[:8]
    return got


# (reads, columns).  The sizes of the kernel (kernels_del.hip): a word is 32 reads, a tile 512 reads (16 words, 64 bytes of a plane
# row), a plane row whole 128-byte lines (1024 reads); a lane owns a codon start, a workgroup 64 of them and stages their 64 columns
# and a halo of two: n_cols = 66 is one full group, 67 the first of a second group, 129 / 130 / 131 end a group one short of, at
# and one past its last start, 3 / 4 / 5 are one, two, three starts.  The reads are split over workgroups in segments of an even
# number of tiles once there are more than two tiles: 1025 reads are segments of 2 + 1 tiles, 2049 reads 2 + 2 + 1, 5000 reads
# 2 + 2 + 2 + 2 + 2 next to four groups.  (Segments of more than two tiles need some 90 000 reads at 3000 columns: the same loop
# going round more often; test_deep_window_against_the_pileup runs it.)  A single read needs seven columns to show all three counters.
CASES = [
    (31, 3), (32, 4), (33, 5), (1, 63), (1023, 64), (1024, 65), (1025, 66), (2049, 67), (31, 129), (33, 130), (1025, 131),
    (1, 7), (3, 3), (2049, 5), (1023, 130), (1024, 66), (5000, 200),
]


@pytest.mark.parametrize("n,n_cols", CASES)
def test_counts_equal_mirror(ctx, n, n_cols):
    rows = make_case(n, n_cols, 1000 * n + n_cols)
    ctx.upload_rows(rows, win_begin=3)
    check(ctx, rows)
    assert (msa.unpack_columns(ctx.download_columns(), n) == rows).all()     # the matrix is untouched


def test_adopted_matrix_with_its_own_stride():
    """A torch tensor as the matrix: 2049 reads in planes of 272 bytes (the library's own stride is 384), garbage in the bytes
    past ceil(n / 8) of every plane row and in the bits of the last byte past the last read.  None of it may show in a count."""
    import torch
    n, n_cols, stride = 2049, 131, 272
    assert stride != msa.plane_stride(n) and stride % 16 == 0
    rows = make_case(n, n_cols, 99)
    planes = msa.pack_planes(rows, stride)
    rng = np.random.default_rng(1)
    planes[:, :, (n + 7) // 8:] = rng.integers(0, 256, size=(n_cols, 3, stride - (n + 7) // 8), dtype=np.uint8)
    assert n % 8 == 1
    last = planes[:, :, (n + 7) // 8 - 1]
    planes[:, :, (n + 7) // 8 - 1] = (last & 1) | (rng.integers(0, 256, size=last.shape, dtype=np.uint8) & 0xFE)   # bits 1..7: no read's
    # ... among them plane 2 CLEAR past the last read in half the columns (a base that does not exist) and plane 2 alone SET in
    # some (a '-' that does not exist)
    planes[::2, 2, (n + 7) // 8 - 1] &= 1
    planes[1::4, 2, (n + 7) // 8 - 1] |= 0xFE
    planes[1::4, :2, (n + 7) // 8 - 1] &= 1
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t = torch.from_numpy(planes).cuda(non_blocking=False)
    stream.synchronize()
    j = capi.Juliet(0, stream=stream.cuda_stream)
    j.adopt(t.data_ptr(), n, n_cols, stride, keep_alive=t)
    check(j, rows)
    j.close()


def test_repeated_and_growing_calls(ctx):
    """Small, large, small: the table grows and is reused, no stale count shows; a call that only enqueues, fetched later."""
    for n, n_cols in ((40, 9), (3000, 400), (40, 9), (700, 70)):
        rows = make_case(n, n_cols, n + n_cols)
        ctx.upload_rows(rows)
        check(ctx, rows)
        check(ctx, rows)
    assert ctx.codon_deletions(wait=False) is None
    assert (ctx.codon_deletions_fetch() == dm.counts(rows)).all()


def test_refusals():
    lib = capi.load_library()
    j = capi.Juliet(0)
    assert lib.jl_codon_deletions_async(j.h) == -4 and "no resident matrix" in lib.jl_last_error(j.h).decode()
    rows = make_case(40, 9, 1)
    j.upload_rows(rows)
    with pytest.raises(capi.JulietError) as e:                       # a fetch before any call
        j.codon_deletions_fetch()
    assert e.value.status == -4 and "before jl_codon_deletions_async" in str(e.value)
    buf = np.zeros((7, 4), dtype=np.uint32)
    assert lib.jl_codon_deletions_fetch(j.h, buf.ctypes.data) == -4
    good = check(j, rows)
    j2 = capi.Juliet(0)
    j2.upload_rows(rows[:, :2])                                      # two columns hold no codon
    with pytest.raises(capi.JulietError) as e:
        j2.codon_deletions()
    assert e.value.status == -1 and "2 columns" in str(e.value)
    j2.close()
    assert lib.jl_codon_deletions_fetch(j.h, None) == 0              # NULL: only wait
    assert (j.codon_deletions_fetch() == good).all()
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


def test_consequences_after_a_real_run(ctx):
    """A synthetic window with deletions, masked bases and partial reads (synth_fill, 5000 x 300): codon[col] is the coverage of
    every variant row and the diagonal of the linkage's `both`; the run's results and the matrix are what they were, and a second
    run equals the first."""
    n, l = 5000, 300
    sp = synth.SynthParams(seed=5, del_rate=4e-3, mask_rate=2e-2, partial_rate=0.1, minor_permille=(150, 120, 100, 80))
    ref = synth.reference(sp.seed, l)
    genes = np.array([(1, l + 1)], dtype=capi.GENE)
    ctx.alloc(n, l)
    ctx.synth_fill(sp, ref)
    before = ctx.download_columns().copy()
    ctx.run_async(genes, ref, capi.default_params(), None, True, 10, True)
    first = fetch_copy(ctx)
    var = first["variants"]
    assert 4 <= len(var) <= 256
    cnt = ctx.codon_deletions()
    assert cnt[:, dm.CODON].any() and cnt[:, dm.PARTIAL].any()       # (the generator deletes single bases: no whole codon goes)
    assert (cnt[var["col"], dm.CODON] == var["coverage"]).all()
    pos_cols = np.unique(var["col"]).astype(np.uint32)
    link = ctx.variant_linkage(pos_cols, np.searchsorted(pos_cols, var["col"]).astype(np.uint32), var["codon"].copy())
    assert (np.diag(link["both"]) == cnt[pos_cols, dm.CODON]).all()
    assert (cnt[:, :3].astype(np.int64).sum(axis=1) <= cnt[:, dm.SPAN]).all() and cnt[:, dm.SPAN].max() <= n
    rows = msa.unpack_columns(ctx.download_columns(), n)
    assert (cnt == dm.counts(rows)).all()
    assert_same_run(first, fetch_copy(ctx))
    assert (ctx.download_columns() == before).all()
    ctx.run_async(genes, ref, capi.default_params(), None, True, 10, True)
    assert_same_run(first, fetch_copy(ctx))
    ctx.run_async(genes, ref, capi.default_params(), None, True, 10, True)   # (a configuration is captured on its second run: the replay)
    assert_same_run(first, fetch_copy(ctx))


def test_deep_window_against_the_pileup():
    """100 000 reads x 3000 columns, filled on the device: read segments of four tiles.  No rows on the host at this size: codon[c]
    is compared with the pileup's codon coverage at all 1000 positions, and every count with the sum of the same call over the
    window's four blocks of 25 000 reads (jl_msa_take), which are launches of another shape."""
    n, l = 100_000, 3000
    j = capi.Juliet(0)
    j.alloc(n, l)
    j.synth_fill(synth.SynthParams(seed=7, del_rate=4e-3, mask_rate=1e-2, partial_rate=0.05, minor_permille=(60, 50, 40, 30)), synth.reference(7, l))
    whole = j.codon_deletions()
    j.pileup_async(np.array([(1, l + 1)], dtype=capi.GENE))
    pf = j.pileup_fetch()
    assert len(pf["pos_col"]) == 1000 and (whole[pf["pos_col"], dm.CODON] == pf["coverage"]).all()
    assert whole[:, dm.PARTIAL].any() and (whole[:, :3].astype(np.int64).sum(axis=1) <= whole[:, dm.SPAN]).all()
    part, total = capi.Juliet(0), np.zeros_like(whole, dtype=np.int64)
    for b in range(0, n, 25_000):                                    # (segments of two tiles here: another launch shape)
        part.take([(j, np.arange(b, b + 25_000, dtype=np.uint32))])
        total += part.codon_deletions()
    assert (total == whole).all()
    part.close()
    j.close()


# ---------------------------------------------------------------------------------------------- the command line
N_CLI, L_CLI = 3000, 90
DEL_CODON, N_HAP = 10, 60       # gene codon 11 (columns 30..32): 60 reads have it deleted, 60 others lose its last two bases


def to_bam(tmp, rows, ref, genes, name):
    mpath, bam, cfg = (str(tmp / f"{name}.{x}") for x in ("msa", "bam", "json"))
    with open(mpath, "wb") as f:
        f.write(np.array([rows.shape[0], rows.shape[1], 0], dtype=np.uint64).tobytes())
        f.write(np.ascontiguousarray(rows, dtype=np.uint8).tobytes())
    refs = "".join("ACGT"[b] for b in ref)
    subprocess.check_call([SYNTH, "--from-rows", mpath, "--ref", refs, "-o", bam])
    json.dump({"genes": [dict(name=n, begin=b, end=e, drms=[]) for n, b, e in genes], "referenceName": "printed",
               "referenceSequence": refs, "version": "tests/test_gpu_deletions.py", "databaseVersion": "none"}, open(cfg, "w"))
    return bam, cfg


def juliet(d, *args):
    return subprocess.run([JULIET, *args], cwd=d, capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    d = tmp_path_factory.mktemp("deletions_cli")
    rng = np.random.default_rng(17)
    ref = rng.integers(0, 4, size=L_CLI, dtype=np.uint8)
    rows = np.repeat(ref[None, :], N_CLI, axis=0)
    c = 3 * DEL_CODON
    rows[100:100 + N_HAP, c:c + 3] = GAP
    rows[500:500 + N_HAP, c + 1:c + 3] = GAP
    to_bam(d, rows, ref, [("G", 1, L_CLI + 1)], "in")
    r = juliet(d, "-c", "in.json", "--mode-phasing", "--call-deletions", "--timing", "in.bam", "d.json", "d.html")
    assert r.returncode == 0, r.stderr
    assert re.search(r"timing deletions\s", r.stderr)               # the stage line of --timing
    for args in (("--mode-phasing", "in.bam", "plain.json", "plain.html"), ("--call-deletions", "in.bam", "d0.json", "d0.html"),
                 ("in.bam", "plain0.json", "plain0.html")):
        p = juliet(d, "-c", "in.json", *args)
        assert p.returncode == 0, p.stderr
    return d, rows, ref


CODONS = [a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT"]


def expected_entries(rows, ref, n_tests, rate=1.0e-3):
    """deletion_positions of the one gene over all columns: the mirror's counts and the exact test (the BAM says SEQUEL)."""
    cnt = dm.counts(rows)
    out = []
    for k in range(rows.shape[1] // 3):
        t = dm.test(cnt[3 * k], rate, n_tests)
        if t["called"]:
            out.append((k + 1, CODONS[16 * ref[3 * k] + 4 * ref[3 * k + 1] + ref[3 * k + 2]], t))
    return out


def test_cli_block_equals_the_mirror_and_the_exact_test(cli):
    d, rows, ref = cli
    exp = expected_entries(rows, ref, L_CLI // 3)
    assert [e[0] for e in exp] == [DEL_CODON + 1]                      # the clean deletion and nothing else
    for name in ("d.json", "d0.json"):
        genes = json.load(open(d / name))["genes"]
        assert len(genes) == 1 and genes[0]["variant_positions"] == []
        got = genes[0]["deletion_positions"]
        assert len(got) == len(exp)
        for g, (pos, codon, t) in zip(got, exp):
            assert list(g) == ["ref_position", "ref_codon", "ref_amino_acid", "count", "coverage", "frequency", "expected", "pValue",
                               "log_pValue", "frameshift_reads"]
            assert (g["ref_position"], g["ref_codon"], g["count"], g["coverage"], g["expected"], g["frameshift_reads"]) == \
                (pos, codon, t["count"], t["coverage"], t["expected"], t["partial"])
            assert g["frequency"] == t["count"] / t["coverage"]
            p_adj, lp = float(t["p_adj"]), math.log(float(t["p"]))
            assert abs(g["pValue"] - p_adj) <= 5e-12 * p_adj and abs(g["log_pValue"] - lp) <= 1e-12 * max(1.0, abs(lp)) + 1e-13
        # the two-base deletion: frame-shift reads of the called position, called nowhere itself
        assert got[0]["count"] == N_HAP and got[0]["frameshift_reads"] == N_HAP and got[0]["coverage"] == N_CLI - N_HAP
    assert json.load(open(d / "d.json"))["genes"][0]["deletion_positions"] == json.load(open(d / "d0.json"))["genes"][0]["deletion_positions"]


def json_number(v):
    """A number as the JSON writer prints it."""
    return "%.0f" % v if v == int(v) else "%.17g" % v


def test_cli_html_holds_one_row_per_entry(cli):
    d, rows, ref = cli
    got = json.load(open(d / "d.json"))["genes"][0]["deletion_positions"]
    html = open(d / "d.html").read()
    block = re.search(r'<details open id="deletions">.*?</details>', html, flags=re.S).group(0)
    trs = [re.findall(r"<td>(.*?)</td>", tr) for tr in re.findall(r'<tr class="deletion">.*?</tr>', block)]
    assert len(trs) == len(got) == 1
    for cells, g in zip(trs, got):
        assert cells == [str(g["ref_position"]), g["ref_codon"], g["ref_amino_acid"]] + \
            [json_number(g[k]) for k in ("count", "coverage", "frequency", "expected", "pValue", "log_pValue", "frameshift_reads")]


def strip_json(text):
    j = json.loads(text)
    j["input"].pop("timestamp")
    j["input"].pop("command_line")
    for g in j["genes"]:
        g.pop("deletion_positions", None)
    return json.dumps(j, indent=1)


def strip_html(text):
    text = re.sub(r'<details open id="deletions">.*?</table>\n</details>\n', "", text, flags=re.S)
    return re.sub(r"<tr><th>(timestamp|command_line)</th>.*?</tr>\n", "", text)


def test_cli_without_the_flag_the_outputs_are_the_plain_run(cli):
    d, rows, ref = cli
    for with_flag, plain in (("d", "plain"), ("d0", "plain0")):
        assert "deletion_positions" in open(d / (with_flag + ".json")).read() and "deletion_positions" not in open(d / (plain + ".json")).read()
        assert strip_json(open(d / (with_flag + ".json")).read()) == strip_json(open(d / (plain + ".json")).read())
        html, plain_html = open(d / (with_flag + ".html")).read(), open(d / (plain + ".html")).read()
        assert 'id="deletions"' in html and 'id="deletions"' not in plain_html
        assert strip_html(html) == strip_html(plain_html)
    # ... and two runs without the flag differ in nothing but the time and the command line: the comparison above is a fair one
    again = juliet(d, "-c", "in.json", "--mode-phasing", "in.bam", "again.json", "again.html")
    assert again.returncode == 0
    plain = json.loads(open(d / "plain.json").read())
    other = json.loads(open(d / "again.json").read())
    for j in (plain, other):
        j["input"].pop("timestamp"), j["input"].pop("command_line")
    assert plain == other
    assert strip_html(open(d / "again.html").read()) == strip_html(open(d / "plain.html").read())


def test_cli_drm_only_and_downsample(cli):
    d, rows, ref = cli
    r = juliet(d, "-c", "in.json", "--call-deletions", "--drm-only", "in.bam", "drm.json")
    assert r.returncode == 0, r.stderr
    assert json.load(open(d / "drm.json"))["genes"][0]["deletion_positions"] == []          # no DRM notation names a deletion
    r = juliet(d, "-c", "in.json", "--call-deletions", "--downsample", "1000", "--sample-seed", "3", "in.bam", "ds.json")
    assert r.returncode == 0, r.stderr
    kept = capi.sample_reads(len(rows), 1000, 3)                     # docs/SPEC.md §12: host arithmetic, no device
    exp = expected_entries(rows[kept], ref, L_CLI // 3)
    got = json.load(open(d / "ds.json"))["genes"][0]["deletion_positions"]
    assert [(g["ref_position"], g["count"], g["coverage"], g["frameshift_reads"]) for g in got] == \
        [(pos, t["count"], t["coverage"], t["partial"]) for pos, _, t in exp]


@pytest.mark.parametrize("args", [["--windows", "2"], ["--devices", "0,0"], ["--mode-phasing", "--windows", "3"]])
def test_cli_refused_combinations_open_nothing(tmp_path, args):
    r = juliet(tmp_path, "--call-deletions", *args, "no_such.bam", "o.json")
    assert r.returncode == 1 and "--call-deletions" in r.stderr, (r.returncode, r.stderr)
    assert not list(tmp_path.iterdir())


def test_cli_refused_with_batch_and_as_fuse(tmp_path):
    (tmp_path / "l.tsv").write_text("no_such.bam\ta.json\n")
    r = juliet(tmp_path, "--call-deletions", "--batch", "l.tsv")
    assert r.returncode == 1 and "--call-deletions" in r.stderr and "--batch" in r.stderr
    r = subprocess.run([os.path.join(ROOT, "minorseq_amd", "bin", "fuse"), "--call-deletions", "no_such.bam", "o.fasta"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--call-deletions" in r.stderr and "fuse" in r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == ["l.tsv"]
