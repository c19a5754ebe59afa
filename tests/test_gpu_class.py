"""jl_class_pileup_async on the device (docs/SPEC.md §13): the column pileup of the resident matrix by class of reads, and
`juliet --mode-phasing --haplotype-fasta` on top of it.  The expected counts are always numpy over the rows that were uploaded
— per class and symbol, (rows[label == k] == s).sum(0) — compared for equality on every cell, never with another device result."""
import json
import os
import subprocess

import numpy as np
import pytest

from minorseq_amd import capi, msa, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JULIET = os.path.join(ROOT, "minorseq_amd", "bin", "juliet")
SYNTH = os.path.join(ROOT, "minorseq_amd", "bin", "juliet-synth")


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


def code_rows(n, l, seed):
    """Seeded codes 0..5 with ragged code-6 ends, as reads that start late and end early have."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 6, size=(n, l), dtype=np.uint8)
    lo, hi = rng.integers(0, l // 3 + 1, size=n), l - rng.integers(0, l // 3 + 1, size=n)
    ci = np.arange(l)[None, :]
    rows[(ci < lo[:, None]) | (ci >= hi[:, None])] = 6
    return rows


def expected(rows, label, k):
    """counts[k][l][6] and class_reads[k] by the rule of §13, in numpy."""
    counts = np.zeros((k, rows.shape[1], 6), dtype=np.uint32)
    for c in range(k):
        sel = rows[label == c]
        for s in range(6):
            counts[c, :, s] = (sel == s).sum(axis=0)
    return counts, np.array([(label == c).sum() for c in range(k)], dtype=np.uint32)


def labels(name, n, k, seed):
    rng = np.random.default_rng(seed)
    if name == "all_one":          # every read in one class
        return np.zeros(n, dtype=np.uint16)
    if name == "outside":          # every read outside: all zeros
        return np.full(n, 0xFFFF, dtype=np.uint16)
    if name == "random":
        return rng.integers(0, k, size=n).astype(np.uint16)
    if name == "empty":            # classes with no read: one in the middle, the last of the first pass, the last of all
        lab = rng.integers(0, k, size=n).astype(np.uint16)
        for e in {k // 2, min(15, k - 1), k - 1}:
            lab[lab == e] = 0 if e else 0xFFFF
        return lab
    if name == "mixed":            # members beside the two read categories of a phasing run and n_classes itself
        pool = np.array(list(range(k)) + [0xFFFE, 0xFFFF, k], dtype=np.uint16)
        lab = pool[rng.integers(0, len(pool), size=n)]
        lab[: min(n, 3)] = [0xFFFE, 0xFFFF, k][: min(n, 3)]
        return lab
    if name == "one_and_rest":     # class sizes of 1 and of n - 1
        lab = np.full(n, 1, dtype=np.uint16)
        lab[n // 2] = 0
        return lab
    raise ValueError(name)


# (reads, columns, classes, labels): the byte / word / 128-byte line / 64-column group / 16-class pass edges, sparsely paired
CASES = [
    (1, 1, 1, "all_one"), (7, 2, 2, "random"), (8, 63, 15, "mixed"), (9, 64, 16, "empty"), (31, 65, 17, "random"),
    (32, 130, 33, "mixed"), (33, 1, 704, "random"), (1023, 2, 16, "one_and_rest"), (1024, 63, 17, "empty"), (1025, 64, 2, "mixed"),
    (2049, 65, 33, "empty"), (2049, 130, 704, "mixed"), (1025, 130, 1, "all_one"), (1024, 1, 15, "outside"), (33, 64, 2, "one_and_rest"),
    (1023, 65, 33, "random"), (7, 130, 17, "outside"), (2049, 2, 1, "mixed"), (9, 63, 704, "empty"), (31, 1, 16, "all_one"),
    (8, 2, 33, "one_and_rest"), (32, 65, 15, "random"),
]


def check(j, rows, lab, k):
    counts, reads = j.class_pileup(lab, k)
    exp_counts, exp_reads = expected(rows, lab, k)
    assert counts.shape == exp_counts.shape and counts.dtype == np.uint32
    assert (reads == exp_reads).all()
    assert (counts == exp_counts).all()
    # padding and uncovered cells count nowhere: a column sums to the labelled reads that cover it
    assert (counts.sum(axis=(0, 2)) == (rows[lab < k] != 6).sum(axis=0)).all()
    return counts


@pytest.mark.parametrize("n,l,k,name", CASES)
def test_class_pileup_equals_numpy(ctx, n, l, k, name):
    rows = code_rows(n, l, n * 1000 + l)
    lab = labels(name, n, k, n + 7 * l + k)
    if name == "one_and_rest":
        assert sorted(((lab == 0).sum(), (lab == 1).sum())) == [1, n - 1]
    if name == "empty":
        assert not (lab == k // 2).any() and not (lab == k - 1).any()
    ctx.upload_rows(rows, win_begin=3)
    counts = check(ctx, rows, lab, k)
    if name == "outside":
        assert not counts.any()
    assert (msa.unpack_columns(ctx.download_columns(), n) == rows).all()     # the matrix is untouched


def test_segments_of_four_tiles():
    """The smallest window at which a workgroup walks four tiles (jl_walk_shape_for: n_tiles * n_groups > 8192): 65 columns — two
    groups, the second of one column — and 4097 tiles in 1025 segments, the last of one tile that ends inside it.  The rows
    are a 1536-read block — three tiles, so that tiles t and t + 2 differ — repeated with a tail, the labels too; the counts are the block's times the repeats plus the
    tail's (tests/test_walk_host.py holds that property)."""
    import second_turn
    import walk_shape
    l, k = 65, 3
    n, seg_tiles, n_segs = walk_shape.deep_case(lambda n: walk_shape.walk(n, (l + 63) // 64))
    assert seg_tiles >= 4 and n_segs >= 2 and -(-n // 512) % seg_tiles != 0 and n % 512 == 300
    block, lab = code_rows(1536, l, 11), labels("mixed", 1536, k, 5)
    reps, tail = second_turn.split(n, 1536)
    c, r = expected(block, lab, k)
    tc, tr = expected(block[:tail], lab[:tail], k)
    exp_counts, exp_reads = reps * c + tc, reps * r + tr
    assert exp_counts[:, :, :6].any(axis=(0, 1)).all() and (exp_reads > 0).all() and tc.any()
    j = capi.Juliet(0)
    try:
        second_turn.adopt_tiled(j, block, n)
        counts, reads = j.class_pileup(second_turn.tiled(lab, n), k)
        assert (reads == exp_reads).all()
        assert (counts == exp_counts).all(), np.argwhere(counts != exp_counts)[:8]
    finally:
        j.close()


def test_padding_behind_the_last_read_counts_nowhere(ctx):
    """1025 reads: 1023 read positions of padding in the second line of every plane row.  With every read in class 0 the
    counts are the whole-matrix counts and not one more."""
    n, l = 1025, 5
    rows = code_rows(n, l, 77)
    rows[:, 2] = 0                         # a column every read covers
    ctx.upload_rows(rows)
    counts = check(ctx, rows, np.zeros(n, dtype=np.uint16), 3)
    assert counts[0, 2].tolist() == [n, 0, 0, 0, 0, 0] and not counts[1:].any()


def test_adopted_matrix_with_its_own_stride():
    """A torch tensor as the matrix: 2049 reads in planes of 272 bytes (the library's own stride, and that of the mask rows, is
    384), garbage in the bytes past ceil(n / 8) of every plane row.  None of it may count."""
    import torch
    n, l, stride = 2049, 67, 272
    assert stride != msa.plane_stride(n) and stride % 16 == 0
    rows = code_rows(n, l, 99)
    planes = msa.pack_planes(rows, stride)
    planes[:, :, (n + 7) // 8:] = np.random.default_rng(1).integers(0, 256, size=(l, 3, stride - (n + 7) // 8), dtype=np.uint8)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t = torch.from_numpy(planes).cuda(non_blocking=False)
    stream.synchronize()
    j = capi.Juliet(0, stream=stream.cuda_stream)
    j.adopt(t.data_ptr(), n, l, stride, keep_alive=t)
    for k, name in ((17, "random"), (2, "mixed"), (1, "all_one")):
        check(j, rows, labels(name, n, k, k), k)
    j.close()


def assert_same_run(a, b):
    assert (a["variants"] == b["variants"]).all()
    pa, pb = a["phase"], b["phase"]
    assert pa["summary"] == pb["summary"]
    for key in ("pos_cols", "hap_count", "hap_pattern", "hit", "read_hap", "cooc"):
        assert (pa[key] == pb[key]).all(), key


def fetch_copy(j):
    out = j.run_fetch(True, True, cap_var=64)
    return dict(variants=out["variants"].copy(), phase={k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in out["phase"].items()})


def test_stage_results_are_kept(ctx):
    """A run with phasing, its results fetched; the class pileup by the run's own ids; the run fetched again: the same."""
    n, l = 2049, 130
    sp = synth.SynthParams(seed=5, minor_permille=(150, 120, 100, 80))
    ref = synth.reference(sp.seed, l)
    rows = synth.rows(sp, l, 0, n, ref)
    genes = np.array([(1, l + 1)], dtype=capi.GENE)
    ctx.upload_rows(rows)
    ctx.run_async(genes, ref, capi.default_params(), None, True, 10, True)
    first = fetch_copy(ctx)
    pile = ctx.pileup_fetch()
    h = first["phase"]["summary"]["n_haplotypes"]
    assert len(first["variants"]) >= 2 and h >= 2          # the input was chosen so that there is something to keep
    read_hap = first["phase"]["read_hap"]
    counts = check(ctx, rows, read_hap, h)
    assert (counts.sum(axis=(1, 2)) > 0).all()             # every reported haplotype has reads that cover something
    again = fetch_copy(ctx)
    assert_same_run(first, again)
    pile2 = ctx.pileup_fetch()
    for key in pile:
        assert (pile[key] == pile2[key]).all(), key
    # every read labelled 0: the whole-matrix counts, which are also what the run's own pileup counted
    whole, reads = ctx.class_pileup(np.zeros(n, dtype=np.uint16), 1)
    assert (whole[0] == np.stack([(rows == s).sum(axis=0) for s in range(6)], axis=1)).all() and reads.tolist() == [n]
    assert (whole[0] == pile["col_counts"]).all()
    assert (msa.unpack_columns(ctx.download_columns(), n) == rows).all()
    # ... and a run after it is the run before it
    ctx.run_async(genes, ref, capi.default_params(), None, True, 10, True)
    assert_same_run(first, fetch_copy(ctx))


def test_repeat_on_one_context(ctx):
    """17 classes (two passes), then 2 with other labels, on the same matrix: no stale pass, mask or count shows."""
    n, l = 1025, 65
    rows = code_rows(n, l, 12)
    ctx.upload_rows(rows)
    check(ctx, rows, labels("random", n, 17, 1), 17)
    check(ctx, rows, labels("mixed", n, 2, 2), 2)
    check(ctx, rows, labels("random", n, 17, 3), 17)
    # the labels are copied before the call returns: the caller's array may be overwritten at once
    lab = labels("random", n, 5, 4)
    keep = lab.copy()
    ctx.class_pileup(lab, 5, wait=False)
    lab[:] = 0
    counts, reads = ctx.class_pileup_fetch()
    exp_counts, exp_reads = expected(rows, keep, 5)
    assert (counts == exp_counts).all() and (reads == exp_reads).all()


def test_staging_grows_and_is_reused(ctx):
    """1500, then 5000, then 1500 reads on one context: the label staging, the mask rows and the counts grow for the second call
    and serve the third, larger than it needs."""
    l = 60
    for seed, n in enumerate((1500, 5000, 1500)):
        rows = code_rows(n, l, 50 + seed)
        ctx.upload_rows(rows)
        check(ctx, rows, labels("random", n, 17, seed), 17)


def test_refusals_change_nothing():
    lib = capi.load_library()
    j = capi.Juliet(0)
    lab = np.zeros(40, dtype=np.uint16)

    def refused(status, ptr, k, word):
        rc = lib.jl_class_pileup_async(j.h, ptr, k)
        assert rc == status
        assert word in lib.jl_last_error(j.h).decode(), lib.jl_last_error(j.h)

    refused(-4, lab.ctypes.data, 3, "no resident matrix")
    rows = code_rows(40, 9, 1)
    j.upload_rows(rows)
    out = np.zeros((3, 9, 6), dtype=np.uint32)
    assert lib.jl_class_pileup_fetch(j.h, out.ctypes.data, None) == -4          # a fetch before any call
    assert "before jl_class_pileup_async" in lib.jl_last_error(j.h).decode()
    good = labels("random", 40, 3, 5)
    counts, reads = j.class_pileup(good, 3)
    refused(-1, lab.ctypes.data, 0, "no classes")
    refused(-1, lab.ctypes.data, 705, "at most 704")
    refused(-1, None, 3, "no labels")
    again, reads2 = j.class_pileup_fetch()                                      # what was enqueued before is still there
    assert (again == counts).all() and (reads2 == reads).all()
    assert (counts == expected(rows, good, 3)[0]).all()
    assert (j.class_pileup(good, 704)[0][:3] == counts).all()                   # 704 itself is accepted
    assert (msa.unpack_columns(j.download_columns(), 40) == rows).all()
    j.close()


# ---------------------------------------------------------------------------------------------- the command line
N_CLI, L_CLI, SEED_CLI = 3000, 300, 41
MINOR = (150, 120, 100, 80)


def read_msa(path):
    raw = open(path, "rb").read()
    n, l, wb = (int(x) for x in np.frombuffer(raw[:24], dtype=np.uint64))
    return np.frombuffer(raw[24:], dtype=np.uint8).reshape(n, l), wb


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    d = tmp_path_factory.mktemp("class_cli")
    subprocess.check_call([SYNTH, "--reads", str(N_CLI), "--cols", str(L_CLI), "--seed", str(SEED_CLI), "--partial", "0.1",
                           "--minor-permille", *map(str, MINOR), "-o", str(d / "in.bam"), "--config-out", str(d / "cfg.json")])
    subprocess.check_call([JULIET, "-c", "cfg.json", "--dump-msa", "in.msa", "in.bam"], cwd=d)      # host only: no GPU involved
    rows, wb = read_msa(d / "in.msa")
    assert rows.shape[0] == N_CLI
    return d, rows, wb


def juliet(d, *args):
    return subprocess.run([JULIET, *args], cwd=d, capture_output=True, text=True, timeout=120)


def json_number(v):
    """A number as the JSON writer prints it."""
    return "%.0f" % v if v == int(v) else "%.17g" % v


def expected_fasta(j, rows, wb, source):
    """§13 in numpy: per haplotype of the JSON, in its order, the consensus of the rows its read_names name."""
    out = []
    n_cols = rows.shape[1]
    assert (j["target_config"]["window_begin"], j["target_config"]["window_end"]) == (wb + 1, wb + n_cols + 1)
    for h in j["haplotype"]["haplotypes"]:
        members = rows[[int(name.split("/")[1]) for name in h["read_names"]]]
        assert len(members) == h["reads"]
        counts = np.stack([(members == s).sum(axis=0) for s in range(5)], axis=1)
        best = np.argmax(counts, axis=1)                    # the first maximum: the lowest code on ties
        seq = "".join("N" if counts[c].max() == 0 else "ACGT"[best[c]] for c in range(n_cols) if counts[c].max() == 0 or best[c] != 4)
        out.append(f">{h['name']} reads={h['reads']} frequency={json_number(h['frequency'])} window={wb + 1}-{wb + n_cols} source={source}\n")
        out.extend(seq[i:i + 70] + "\n" for i in range(0, len(seq), 70))
    return "".join(out)


def norm(path):
    j = json.load(open(path))
    j["input"].pop("timestamp")
    j["input"].pop("command_line")
    return j


def test_cli_haplotype_fasta_equals_numpy(cli):
    d, rows, wb = cli
    r = juliet(d, "-c", "cfg.json", "--mode-phasing", "--haplotype-fasta", "h.fasta", "--timing", "in.bam", "out.json")
    assert r.returncode == 0, r.stderr
    assert "haplotype fasta" in r.stderr                     # the stage line of --timing
    j = json.load(open(d / "out.json"))
    haps = j["haplotype"]["haplotypes"]
    assert len(haps) >= 3                                    # the mixture was chosen so that the test cannot pass vacuously
    got = open(d / "h.fasta").read()
    assert got == expected_fasta(j, rows, wb, "in.bam")
    assert [line[1:].split()[0] for line in got.splitlines() if line.startswith(">")] == [h["name"] for h in haps]
    body = [line for line in got.splitlines() if not line.startswith(">")]
    assert body and max(map(len, body)) == 70 and set("".join(body)) <= set("ACGTN")
    # the haplotypes differ somewhere: the records are not one sequence repeated
    seqs = got.split(">")[1:]
    assert len({s.split("\n", 1)[1] for s in seqs}) >= 2
    # JSON is what it is without the flag
    r = juliet(d, "-c", "cfg.json", "--mode-phasing", "in.bam", "plain.json")
    assert r.returncode == 0, r.stderr
    assert norm(d / "out.json") == norm(d / "plain.json")


def test_cli_haplotype_fasta_follows_the_taken_window(cli):
    d, rows, wb = cli
    r = juliet(d, "-c", "cfg.json", "--mode-phasing", "--downsample", "1000", "--haplotype-fasta", "ds.fasta", "in.bam", "ds.json")
    assert r.returncode == 0, r.stderr
    j = json.load(open(d / "ds.json"))
    assert j["target_config"]["n_reads"] == 1000 and len(j["haplotype"]["haplotypes"]) >= 2
    assert sum(h["reads"] for h in j["haplotype"]["haplotypes"]) <= 1000
    assert open(d / "ds.fasta").read() == expected_fasta(j, rows, wb, "in.bam")       # (the names follow the indices)


def test_cli_no_reported_haplotype_is_an_empty_file(tmp_path):
    """Reads without a minor clone: nothing is called, nothing is phased, the file is empty and the exit status 0."""
    subprocess.check_call([SYNTH, "--reads", "400", "--cols", "90", "--seed", "3", "--minor-permille", "0", "0", "0", "0",
                           "-o", str(tmp_path / "in.bam"), "--config-out", str(tmp_path / "cfg.json")])
    r = juliet(tmp_path, "-c", "cfg.json", "--mode-phasing", "--haplotype-fasta", "h.fasta", "in.bam", "out.json")
    assert r.returncode == 0, r.stderr
    assert json.load(open(tmp_path / "out.json"))["haplotype"]["haplotypes"] == []
    assert open(tmp_path / "h.fasta").read() == ""
