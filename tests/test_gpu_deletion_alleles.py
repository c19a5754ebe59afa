"""jl_deletion_alleles_async on the device (docs/SPEC.md §25): every read's maximal runs of '-', the bounded ones as a table of
(start, length) alleles with their reads and flank coverage, the open ones per column.  Every expectation is
tests/deletion_alleles_mirror.py — the rule as a per-read scan in plain numpy — over the rows that were uploaded, compared for
equality on every entry; never another device result, except where an identity of §25 against another stage is the point."""
import numpy as np
import pytest

import deletion_alleles_cases as cases
import deletion_alleles_mirror as am
import deletion_mirror as dm
from minorseq_amd import capi, msa, synth

pytestmark = pytest.mark.gpu

GAP = 4


@pytest.fixture(scope="module")
def ctx():
    j = capi.Juliet(0)
    yield j
    j.close()


def assert_equal(got, exp):
    assert got["runs"].dtype == np.uint64 and got["open"].dtype == np.uint32 and got["alleles"].dtype == capi.DELETION_ALLELE
    assert (got["runs"] == exp["runs"]).all(), (got["runs"], exp["runs"])
    assert got["open"].shape == exp["open"].shape and (got["open"] == exp["open"]).all(), np.flatnonzero(got["open"] != exp["open"])[:8]
    assert len(got["alleles"]) == len(exp["alleles"]), (len(got["alleles"]), len(exp["alleles"]))
    for k in ("col", "len", "count", "flank"):
        assert (got["alleles"][k] == exp["alleles"][k]).all(), (k, np.flatnonzero(got["alleles"][k] != exp["alleles"][k])[:8])


def check(j, rows):
    exp = am.alleles(rows)
    cases.assert_not_vacuous(rows, exp)
    got = j.deletion_alleles()
    assert_equal(got, exp)
    return got


@pytest.mark.parametrize("n,n_cols", cases.CASES)
def test_results_equal_mirror(ctx, n, n_cols):
    rows = cases.make_case(n, n_cols, 1000 * n + n_cols)
    ctx.upload_rows(rows, win_begin=3)
    check(ctx, rows)
    assert (msa.unpack_columns(ctx.download_columns(), n) == rows).all()     # the matrix is untouched


def test_table_a_different_allele_in_every_read(ctx):
    rows = cases.distinct_alleles(4096, 130)
    ctx.upload_rows(rows)
    got = ctx.deletion_alleles()
    assert len(got["alleles"]) == 4096 and (got["alleles"]["count"] == 1).all() and got["runs"].tolist() == [4096, 0]
    assert_equal(got, am.alleles(rows))


def test_table_one_allele_in_every_read(ctx):
    rows = cases.one_allele_everywhere(4096, 130)
    ctx.upload_rows(rows)
    got = ctx.deletion_alleles()
    first = got["alleles"][0]
    assert (int(first["col"]), int(first["len"]), int(first["count"]), int(first["flank"])) == (5, 9, 4096, 4096)
    assert got["runs"].tolist() == [8192, 0] and len(got["alleles"]) > 1000
    assert_equal(got, am.alleles(rows))


def test_table_every_possible_allele(ctx):
    rows = cases.every_allele(2048, 40)
    ctx.upload_rows(rows)
    got = ctx.deletion_alleles()
    assert len(got["alleles"]) == 39 * 38 // 2
    assert_equal(got, am.alleles(rows))


def test_adopted_matrix_with_its_own_stride():
    """A torch tensor as the matrix: 2049 reads in planes of 272 bytes (the library's own stride is 384), garbage in the bytes
    past ceil(n / 8) of every plane row and in the bits of the last byte past the last read, among them '-' codes that do not
    exist.  None of it may show in a result."""
    import torch
    n, n_cols, stride = 2049, 131, 272
    assert stride != msa.plane_stride(n) and stride % 16 == 0
    rows = cases.make_case(n, n_cols, 99)
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


def device_identities(j, n, res):
    """The four identities of §25 against this context's own pileup (§2) and codon deletions (§16)."""
    j.pileup_async(np.array([(1, j.n_cols + 1)], dtype=capi.GENE))
    col = j.pileup_fetch()["col_counts"]
    del3 = j.codon_deletions()[:, dm.DEL3] if j.n_cols >= 3 else None
    am.check_identities(res, col[:, GAP], col.astype(np.int64).sum(axis=1), del3)


def test_identities_against_the_pileup_and_the_codon_deletions(ctx):
    """A synthetic window (synth_fill, 5000 x 600: single-base deletions, masked bases, partial reads) with deletions of 3, 9 and
    40 columns planted through an upload of the downloaded rows."""
    n, l = 5000, 600
    sp = synth.SynthParams(seed=5, del_rate=4e-3, mask_rate=2e-2, partial_rate=0.1, minor_permille=(150, 120, 100, 80))
    ctx.alloc(n, l)
    ctx.synth_fill(sp, synth.reference(sp.seed, l))
    rows = msa.unpack_columns(ctx.download_columns(), n).copy()
    rows[100:400, 30:33], rows[1000:1100, 301:310], rows[2000:2100, 400:440] = GAP, GAP, GAP
    ctx.upload_rows(rows)
    before = ctx.download_columns().copy()
    got = ctx.deletion_alleles()
    assert got["runs"][0] > 1000 and got["runs"][1] >= 1
    device_identities(ctx, n, got)
    assert (ctx.download_columns() == before).all()
    assert_equal(got, am.alleles(rows))


def test_deep_window_identities():
    """100 000 reads x 3000 columns, filled on the device: 49 word groups and column segments of 40.  No rows on the host at this
    size: the identities against the pileup and the codon deletions, and every number against the sum of the same call over the
    window's four blocks of 25 000 reads (jl_msa_take), which are launches of another shape (segments of 12 columns)."""
    n, l = 100_000, 3000
    j = capi.Juliet(0)
    j.alloc(n, l)
    j.synth_fill(synth.SynthParams(seed=7, del_rate=4e-3, mask_rate=1e-2, partial_rate=0.05, minor_permille=(60, 50, 40, 30)), synth.reference(7, l))
    whole = j.deletion_alleles()
    assert whole["runs"][0] > 100_000
    device_identities(j, n, whole)
    part, runs, open_, table = capi.Juliet(0), np.zeros(2, dtype=np.uint64), np.zeros(l, dtype=np.int64), {}
    for b in range(0, n, 25_000):
        part.take([(j, np.arange(b, b + 25_000, dtype=np.uint32))])
        got = part.deletion_alleles()
        runs += got["runs"]
        open_ += got["open"]
        for a in got["alleles"]:
            key = (int(a["col"]), int(a["len"]))
            c, f, blocks = table.get(key, (0, 0, 0))
            table[key] = (c + int(a["count"]), f + int(a["flank"]), blocks + 1)
    assert (runs == whole["runs"]).all() and (open_ == whole["open"]).all()
    assert sorted(table) == [(int(a["col"]), int(a["len"])) for a in whole["alleles"]]
    assert [table[k][0] for k in sorted(table)] == [int(a["count"]) for a in whole["alleles"]]
    # (a block without the allele has no row to tell its flank coverage: the sums are equal where all four blocks hold it)
    in_all = [k for k in sorted(table) if table[k][2] == 4]
    flank = {(int(a["col"]), int(a["len"])): int(a["flank"]) for a in whole["alleles"]}
    assert len(in_all) > 100 and all(table[k][1] == flank[k] for k in in_all) and all(table[k][1] <= flank[k] for k in table)
    part.close()
    j.close()


def test_stage_semantics():
    lib = capi.load_library()
    j = capi.Juliet(0)
    assert lib.jl_deletion_alleles_async(j.h) == -4 and "no resident matrix" in lib.jl_last_error(j.h).decode()
    rows_a = cases.make_case(1025, 66, 11)
    j.upload_rows(rows_a)
    with pytest.raises(capi.JulietError) as e:                        # a fetch before any call
        j.deletion_alleles_fetch()
    assert e.value.status == -4 and "before jl_deletion_alleles_async" in str(e.value)
    exp_a = am.alleles(rows_a)
    # enqueue, replace the matrix by an upload of another shape, then fetch: the first matrix's result in its shape
    assert j.deletion_alleles(wait=False) is None
    rows_b = cases.make_case(33, 9, 12)
    j.upload_rows(rows_b)
    assert j.n_cols == 9
    assert_equal(j.deletion_alleles_fetch(), exp_a)
    # cap too small, then a correct fetch; rows == NULL: the count only
    n = capi.C.c_uint32(0)
    assert lib.jl_deletion_alleles_fetch(j.h, None, None, None, 0, capi.C.byref(n)) == 0 and n.value == len(exp_a["alleles"]) > 1
    buf = np.zeros(n.value, dtype=capi.DELETION_ALLELE)
    assert lib.jl_deletion_alleles_fetch(j.h, None, None, buf.ctypes.data, n.value - 1, capi.C.byref(n)) == -1
    assert "room for" in lib.jl_last_error(j.h).decode()
    assert lib.jl_deletion_alleles_fetch(j.h, None, None, buf.ctypes.data, n.value, capi.C.byref(n)) == 0
    assert (buf == exp_a["alleles"]).all()
    assert_equal(j.deletion_alleles(), am.alleles(rows_b))            # ... and the matrix that is resident now
    j.close()


def test_interleaved_with_the_codon_deletions_and_a_run(ctx):
    n, l = 4000, 300
    sp = synth.SynthParams(seed=9, del_rate=4e-3, mask_rate=1e-2, partial_rate=0.1, minor_permille=(150, 120, 100, 80))
    ref = synth.reference(sp.seed, l)
    genes = np.array([(1, l + 1)], dtype=capi.GENE)
    ctx.alloc(n, l)
    ctx.synth_fill(sp, ref)
    rows = msa.unpack_columns(ctx.download_columns(), n)
    exp = am.alleles(rows)

    def run():
        ctx.run_async(genes, ref, capi.default_params(), None, True, 10, True)
        out = ctx.run_fetch(True, True, cap_var=256)
        return out["variants"].copy(), out["phase"]["summary"], out["phase"]["read_hap"].copy()

    first = run()
    assert len(first[0]) >= 4
    ctx.deletion_alleles(wait=False)
    cnt = ctx.codon_deletions(wait=False)
    ctx.run_async(genes, ref, capi.default_params(), None, True, 10, True)
    assert cnt is None
    assert_equal(ctx.deletion_alleles_fetch(), exp)
    assert (ctx.codon_deletions_fetch() == dm.counts(rows)).all()
    out = ctx.run_fetch(True, True, cap_var=256)
    assert (out["variants"] == first[0]).all() and out["phase"]["summary"] == first[1] and (out["phase"]["read_hap"] == first[2]).all()
    assert_equal(ctx.deletion_alleles(), exp)
    again = run()
    assert (again[0] == first[0]).all() and again[1] == first[1] and (again[2] == first[2]).all()


def test_two_launches_give_identical_bytes(ctx):
    rows = cases.make_case(5000, 200, 77)
    ctx.upload_rows(rows)
    a, b = ctx.deletion_alleles(), ctx.deletion_alleles()
    for k in ("runs", "open", "alleles"):
        assert a[k].tobytes() == b[k].tobytes()
    assert len(a["alleles"]) > 10


def test_repeated_and_growing_calls(ctx):
    """Small, large, small: the table grows and is reused, no stale slot or count shows."""
    for n, n_cols in ((40, 9), (3000, 400), (40, 9), (700, 70)):
        rows = cases.make_case(n, n_cols, n + n_cols)
        ctx.upload_rows(rows)
        check(ctx, rows)
        check(ctx, rows)


# ---------------------------------------------------------------------------------------------- the command line
import json       # noqa: E402
import math       # noqa: E402
import os         # noqa: E402
import re         # noqa: E402
import subprocess  # noqa: E402

import bam_diff   # noqa: E402
import bam_py     # noqa: E402
import records_expand  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JULIET = os.path.join(ROOT, "minorseq_amd", "bin", "juliet")
N_CLI, L_CLI = 3000, 300
GENES = [("G", 1, 301), ("H", 12, 252)]      # H lies in another frame: 12 = 1 + 11
NINE = (30, 9, 90)                           # (column, length, reads): codons 11..13 of G, off-frame in H; 3 % of the reads
FORTY = (200, 40, 60)                        # ... and 40 bases in 2 %
ONE = (120, 1, 30)                           # ... and a one-base allele in 1 %: called, and dropped by --min-deletion-length 3
RATE = 1.0e-3                                # the SEQUEL model's err.deletion (§5's table)


def cli_records():
    """Reads that are copies of the reference over columns [b, e) with the two planted alleles in disjoint reads and one-base
    deletions at a seeded 0.1 % of the cells, never a read's first or last base; every deletion a D op."""
    rng = np.random.default_rng(25)
    ref = "".join("ACGT"[b] for b in rng.integers(0, 4, size=L_CLI))
    gap = rng.random(size=(N_CLI, L_CLI)) < 1.0e-3
    for (s, length, reads), first in ((NINE, 100), (FORTY, 1000), (ONE, 2000)):
        gap[first:first + reads, s - 1:s + length + 1] = False
        gap[first:first + reads, s:s + length] = True
    records = []
    for i in range(N_CLI):
        b, e = (0, L_CLI) if i % 7 else (int(rng.integers(0, 20)), L_CLI - int(rng.integers(0, 20)))
        gap[i, b], gap[i, e - 1] = False, False
        ops, seq, c = [], [], b
        while c < e:
            k = c
            while k < e and gap[i, k] == gap[i, c]:
                k += 1
            ops.append(("D" if gap[i, c] else "=", k - c))
            if not gap[i, c]:
                seq.append(ref[c:k])
            c = k
        seq = "".join(seq)
        records.append(dict(ref_id=0, pos=b, flag=0, mapq=60, name="m/%d/ccs" % i, cigar=ops, seq=seq, qual=bytes([60]) * len(seq),
                            tags=[("rq", "f", 0.999), ("np", "i", 12)]))
    return ref, records


def juliet(d, *args):
    return subprocess.run([JULIET, *args], cwd=d, capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    if not os.path.exists(JULIET):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "host")])
    d = tmp_path_factory.mktemp("deletion_alleles_cli")
    ref, records = cli_records()
    text = "@HD\tVN:1.5\tSO:unknown\tpb:3.0.1\n@SQ\tSN:main\tLN:%d\n@RG\tID:x\tPL:PACBIO\tPM:SEQUEL\tDS:READTYPE=CCS\n" % L_CLI
    bam_py.write_bam(str(d / "in.bam"), text, [("main", L_CLI)], records, block=20000)
    json.dump({"genes": [dict(name=n, begin=b, end=e, drms=[]) for n, b, e in GENES], "referenceName": "main", "referenceSequence": ref,
               "version": "tests/test_gpu_deletion_alleles.py", "databaseVersion": "none"}, open(d / "in.json", "w"))
    rows = records_expand.expand(bam_diff.expected(records), L_CLI, 0, 0)
    r = juliet(d, "-c", "in.json", "--mode-phasing", "--call-deletion-alleles", "--timing", "in.bam", "d.json", "d.html")
    assert r.returncode == 0, r.stderr
    assert re.search(r"timing deletion_alleles\s", r.stderr)              # the stage line of --timing
    for args in (("--mode-phasing", "in.bam", "plain.json", "plain.html"), ("--call-deletion-alleles", "in.bam", "d0.json", "d0.html"),
                 ("in.bam", "plain0.json", "plain0.html"),
                 ("--call-deletion-alleles", "--min-deletion-length", "3", "in.bam", "k3.json")):
        p = juliet(d, "-c", "in.json", *args)
        assert p.returncode == 0, p.stderr
    return d, rows


def expected_block(rows, min_length=1):
    """The block from the mirror: the totals and the called alleles with the exact test (n_tests: the codons of both genes)."""
    res = am.alleles(rows)
    n_tests = sum((e - b) // 3 for _, b, e in GENES)
    tested = [a for a in res["alleles"] if a["len"] >= min_length]
    called = []
    for a in tested:
        t = am.test(a["count"], a["flank"], RATE, n_tests)
        if t["called"]:
            called.append((int(a["col"]) + 1, int(a["len"]), t))
    return res, len(tested), called


def check_block(block, rows, min_length):
    res, n_tested, called = expected_block(rows, min_length)
    assert list(block) == ["rate", "min_length", "bounded_runs", "open_runs", "n_alleles", "n_alleles_tested", "alleles"]
    assert (block["rate"], block["min_length"], block["bounded_runs"], block["open_runs"], block["n_alleles"], block["n_alleles_tested"]) == \
        (RATE, min_length, int(res["runs"][0]), int(res["runs"][1]), len(res["alleles"]), n_tested)
    assert block["bounded_runs"] + block["open_runs"] == int(res["runs"].sum()) >= 100    # (a third of the reads, downsampled: some 390)
    assert len(block["alleles"]) == len(called)
    for g, (begin, length, t) in zip(block["alleles"], called):
        assert list(g) == ["begin_abs", "length", "count", "coverage", "frequency", "expected", "pValue", "log_pValue", "in_frame", "genes"]
        assert (g["begin_abs"], g["length"], g["count"], g["coverage"], g["expected"]) == (begin, length, t["count"], t["coverage"], t["expected"])
        assert g["frequency"] == t["count"] / t["coverage"] and g["in_frame"] is (length % 3 == 0)
        p_adj, lp = float(t["p_adj"]), math.log(float(t["p"]))
        assert abs(g["pValue"] - p_adj) <= 5e-12 * p_adj and abs(g["log_pValue"] - lp) <= 1e-12 * max(1.0, abs(lp)) + 1e-13
        assert g["genes"] == am.gene_overlaps(begin, length, GENES)
    return block["alleles"]


def test_cli_block_equals_the_mirror_and_the_exact_test(cli):
    d, rows = cli
    for name in ("d.json", "d0.json"):
        got = check_block(json.load(open(d / name))["deletion_alleles"], rows, 1)
        for s, length, reads in (NINE, FORTY):                           # each planted allele is called, once, as planted
            assert [(g["begin_abs"], g["length"], g["count"]) for g in got if g["begin_abs"] == s + 1 and g["length"] == length] == [(s + 1, length, reads)]
        nine = [g for g in got if g["length"] == 9][0]
        assert nine["in_frame"] and nine["genes"] == [dict(name="G", first_position=11, last_position=13, codon_aligned=True),
                                                       dict(name="H", first_position=7, last_position=10, codon_aligned=False)]
    assert json.load(open(d / "d.json"))["deletion_alleles"] == json.load(open(d / "d0.json"))["deletion_alleles"]


def test_cli_min_deletion_length_drops_exactly_the_shorter_entries(cli):
    d, rows = cli
    all_ = json.load(open(d / "d0.json"))["deletion_alleles"]
    k3 = check_block(json.load(open(d / "k3.json"))["deletion_alleles"], rows, 3)
    assert all_["n_alleles_tested"] > json.load(open(d / "k3.json"))["deletion_alleles"]["n_alleles_tested"] >= 2
    assert k3 == [g for g in all_["alleles"] if g["length"] >= 3] and 2 <= len(k3) < len(all_["alleles"])
    assert (ONE[0] + 1, 1) in [(g["begin_abs"], g["length"]) for g in all_["alleles"]]


def json_number(v):
    """A number as the JSON writer prints it."""
    if isinstance(v, bool):
        return "true" if v else "false"
    return "%.0f" % v if v == int(v) else "%.17g" % v


def test_cli_html_parses_back_to_the_same_cells(cli):
    d, rows = cli
    block = json.load(open(d / "d.json"))["deletion_alleles"]
    html = re.search(r'<details open id="deletion-alleles">.*?</details>', open(d / "d.html").read(), flags=re.S).group(0)
    summary = dict(re.findall(r'<tr data-key="(\w+)"><th>\w+</th><td>(.*?)</td></tr>', html))
    assert summary == {k: json_number(block[k]) for k in ("rate", "min_length", "bounded_runs", "open_runs", "n_alleles", "n_alleles_tested")}
    trs = [re.findall(r"<td>(.*?)</td>", tr) for tr in re.findall(r'<tr class="deletion-allele">.*?</tr>', html)]
    assert len(trs) == len(block["alleles"]) >= 2
    for cells, g in zip(trs, block["alleles"]):
        genes = "; ".join("%s %d-%d %s" % (x["name"], x["first_position"], x["last_position"], "aligned" if x["codon_aligned"] else "unaligned")
                          for x in g["genes"])
        assert cells == [json_number(g[k]) for k in ("begin_abs", "length", "count", "coverage", "frequency", "expected", "pValue",
                                                     "log_pValue", "in_frame")] + [genes]


def strip_json(text):
    j = json.loads(text)
    j["input"].pop("timestamp")
    j["input"].pop("command_line")
    j.pop("deletion_alleles", None)
    return json.dumps(j, indent=1)


def strip_html(text):
    text = re.sub(r'<details open id="deletion-alleles">.*?</table></details>\n', "", text, flags=re.S)
    return re.sub(r"<tr><th>(timestamp|command_line)</th>.*?</tr>\n", "", text)


def test_cli_without_the_flag_the_outputs_are_the_plain_run(cli):
    d, rows = cli
    for with_flag, plain in (("d", "plain"), ("d0", "plain0")):
        assert '"deletion_alleles"' in open(d / (with_flag + ".json")).read() and '"deletion_alleles"' not in open(d / (plain + ".json")).read()
        assert strip_json(open(d / (with_flag + ".json")).read()) == strip_json(open(d / (plain + ".json")).read())
        html, plain_html = open(d / (with_flag + ".html")).read(), open(d / (plain + ".html")).read()
        assert 'id="deletion-alleles"' in html and "deletion-alleles" not in plain_html
        assert strip_html(html) == strip_html(plain_html)


def test_cli_follows_downsample(cli):
    d, rows = cli
    r = juliet(d, "-c", "in.json", "--call-deletion-alleles", "--downsample", "1000", "--sample-seed", "3", "in.bam", "ds.json")
    assert r.returncode == 0, r.stderr
    kept = capi.sample_reads(len(rows), 1000, 3)                       # docs/SPEC.md §12: host arithmetic, no device
    check_block(json.load(open(d / "ds.json"))["deletion_alleles"], rows[kept], 1)
