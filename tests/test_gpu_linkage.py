"""jl_variant_linkage_async on the device (docs/SPEC.md §15): for every pair of variants the reads that can be read at both
positions and what they carry there, and `juliet --linkage` on top of it.  Every expectation is tests/linkage_mirror.py — the rule
in plain numpy — over the rows that were uploaded, compared for equality on every entry; never another device result."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import linkage_mirror
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


def positions(vp):
    """Vp codon starts on a window just large enough: the first at column 0, the second overlapping it (columns 0 and 1, two
    frames), the last at n_cols - 3.  Returns (pos_cols, n_cols)."""
    cols = [0, 1][:vp] + [3 * k - 2 for k in range(2, vp)]
    return np.array(cols, dtype=np.uint32), cols[-1] + 3


def make_case(n, n_pos, n_var, seed, n_hap=6):
    """Seeded haplotype rows of bases — each a copy of one row with the third base of about half its codons changed, so that every
    pair of positions sees all four combinations of alleles — and reads that are copies of them with seeded damage: '-' and N
    cells, ragged code-6 ends, reads of code 6 throughout, single-base substitutions.  The variants: n_var of them spread evenly
    over the positions in table order (several at a position, none at some when there are fewer variants than positions); at a
    position the codons the haplotypes have there come first, then codons that no haplotype has; at every fifth position a codon
    that no haplotype has comes first.  Returns (rows, pos_cols, var_pos, var_codon)."""
    rng = np.random.default_rng(seed)
    pos_cols, n_cols = positions(n_pos)
    haps = np.repeat(rng.integers(0, 4, size=(1, n_cols), dtype=np.uint8), n_hap, axis=0)
    flip = rng.random(size=(n_hap, n_pos)) < 0.5
    third = pos_cols.astype(np.int64) + 2
    haps[:, third] = (haps[:, third] + flip * rng.integers(1, 4, size=(1, n_pos))).astype(np.uint8) % 4
    of = rng.integers(0, n_hap, size=n)
    rows = haps[of].copy()
    kind = rng.integers(0, 10, size=n)
    cell = rng.random(size=rows.shape)
    some = (kind == 0) | (kind == 1) | (kind == 2)                    # scattered damage, about one cell a read and more
    rows[some[:, None] & (cell < 1.5 / n_cols)] = 4
    rows[some[:, None] & (cell > 1.0 - 1.5 / n_cols)] = 5
    lo, hi = rng.integers(0, n_cols // 3 + 1, size=n), n_cols - rng.integers(0, n_cols // 3 + 1, size=n)
    ci = np.arange(n_cols)[None, :]
    rows[(kind == 3)[:, None] & ((ci < lo[:, None]) | (ci >= hi[:, None]))] = 6
    rows[kind == 4] = 6                                               # nothing of the read lies in the window
    for i in np.flatnonzero(kind == 5):                               # a substitution in a codon
        c = int(pos_cols[rng.integers(0, n_pos)]) + int(rng.integers(0, 3))
        rows[i, c] = (rows[i, c] + 1 + rng.integers(0, 3)) % 4
    c = pos_cols.astype(np.int64)
    hap_codons = 16 * haps[:, c].astype(np.int64) + 4 * haps[:, c + 1] + haps[:, c + 2]       # [n_hap][n_pos]
    var_pos, var_codon = [], []
    for p in range(n_pos):
        k = n_var * (p + 1) // n_pos - n_var * p // n_pos
        present = list(dict.fromkeys(hap_codons[:, p].tolist()))
        absent = [x for x in range(64) if x not in present]
        order = absent[:1] + present + absent[1:] if p % 5 == 4 else present + absent
        var_pos += [p] * k
        var_codon += order[:k]
    assert len(var_pos) == n_var
    return rows, pos_cols, np.array(var_pos, dtype=np.uint32), np.array(var_codon, dtype=np.uint8)


def some_pair_has_all_four(exp, var_pos):
    """Is there a pair of variants at different positions whose n11, n10, n01 and n00 are all non-zero?"""
    both, carry, joint = (exp[k].astype(np.int64) for k in ("both", "carry", "joint"))
    vp = np.asarray(var_pos, dtype=np.int64)
    n = both[vp][:, vp]
    n10 = carry[:, vp] - joint                       # [v][w]: carry[v][pos(w)] - joint[v][w]
    n01 = n10.T
    n00 = n - joint - n10 - n01
    return bool(((joint > 0) & (n10 > 0) & (n01 > 0) & (n00 > 0) & (vp[:, None] != vp[None, :])).any())


def check(j, rows, pos_cols, var_pos, var_codon, all_four=False):
    exp = linkage_mirror.linkage(rows, pos_cols, var_pos, var_codon)
    if all_four:
        assert some_pair_has_all_four(exp, var_pos)                   # nothing passes vacuously
    out = j.variant_linkage(pos_cols, var_pos, var_codon)
    for key, shape in (("both", (len(pos_cols),) * 2), ("carry", (len(var_pos), len(pos_cols))), ("joint", (len(var_pos),) * 2)):
        assert out[key].dtype == np.uint32 and out[key].shape == shape
        assert (out[key] == exp[key]).all(), key
    return out


# (reads, positions, variants, a pair with all four cells occurs).  The sizes of the kernels (kernels_link.hip, jl_internal.h): a
# lane of the row kernel owns a word of 32 reads, rows are whole 128-byte lines (1024 reads); a wave of the product owns 8 x 8
# rows of the stacked matrix [positions; variants] (JL_LINK_TILE), a workgroup 16 x 16 (JL_LINK_BLOCK_TILE), so positions, variants
# and their sum stand one below, at and one above 8 and 16; a lane walks the words 64 apart; the reads are split over workgroups
# in runs of at least 256 words = 8192 reads (JL_LINK_SPLIT_WORDS), whole multiples of 64 words: 8225 reads are runs of 192 + 66
# words, 16385 reads 320 + 193, 20000 reads 256 + 256 + 113, 16384 reads 256 + 256.  There is one product kernel and one row
# kernel: every case runs both; the split cases run the only other path, more than one run of a row.
CASES = [
    (1, 1, 1, False), (31, 2, 3, False), (32, 63, 64, False), (33, 64, 65, False), (1023, 65, 130, True), (1024, 2, 1, False),
    (1025, 130, 260, True), (2049, 1024, 1024, True), (2049, 17, 1024, True), (33, 1024, 1024, False),
    (33, 7, 8, False), (1025, 8, 9, True), (31, 9, 7, False), (1023, 15, 16, True), (33, 16, 17, False), (1024, 17, 15, True),
    (2049, 16, 16, True), (1023, 1, 7, False), (1025, 8, 8, True), (2049, 4, 4, True), (1024, 7, 9, True), (2049, 15, 17, True),
    (8225, 3, 5, True), (16385, 9, 17, True), (20000, 2, 2, True), (16384, 16, 1, False),
]


@pytest.mark.parametrize("n,n_pos,n_var,all_four", CASES)
def test_linkage_equals_mirror(ctx, n, n_pos, n_var, all_four):
    rows, pos_cols, var_pos, var_codon = make_case(n, n_pos, n_var, 1000 * n + 7 * n_pos + n_var)
    assert pos_cols[0] == 0 and pos_cols[-1] == rows.shape[1] - 3 and (n_pos < 2 or pos_cols[1] == 1)
    ctx.upload_rows(rows, win_begin=3)
    out = check(ctx, rows, pos_cols, var_pos, var_codon, all_four)
    assert (out["both"] == out["both"].T).all() and (out["joint"] == out["joint"].T).all()
    if n_pos >= 5 and n_var >= n_pos and n <= 2049:                   # (among more reads a substitution may make that codon)
        assert (np.diag(out["joint"]) == 0).any()                     # a codon that no read carries is among the variants
    assert (msa.unpack_columns(ctx.download_columns(), n) == rows).all()     # the matrix is untouched


def test_adopted_matrix_with_its_own_stride():
    """A torch tensor as the matrix: 2049 reads in planes of 272 bytes (the library's own stride is 384), garbage in the bytes
    past ceil(n / 8) of every plane row and in the bits of the last byte past the last read.  None of it may show in a count."""
    import torch
    n, n_pos, n_var, stride = 2049, 65, 130, 272
    assert stride != msa.plane_stride(n) and stride % 16 == 0
    rows, pos_cols, var_pos, var_codon = make_case(n, n_pos, n_var, 99)
    planes = msa.pack_planes(rows, stride)
    rng = np.random.default_rng(1)
    planes[:, :, (n + 7) // 8:] = rng.integers(0, 256, size=(rows.shape[1], 3, stride - (n + 7) // 8), dtype=np.uint8)
    assert n % 8 == 1
    last = planes[:, :, (n + 7) // 8 - 1]
    planes[:, :, (n + 7) // 8 - 1] = (last & 1) | (rng.integers(0, 256, size=last.shape, dtype=np.uint8) & 0xFE)   # bits 1..7: no read's
    # ... among them plane 2 CLEAR past the last read: such a bit reads as a base, an informative read that does not exist
    planes[:, 2, (n + 7) // 8 - 1] &= 1
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t = torch.from_numpy(planes).cuda(non_blocking=False)
    stream.synchronize()
    j = capi.Juliet(0, stream=stream.cuda_stream)
    j.adopt(t.data_ptr(), n, rows.shape[1], stride, keep_alive=t)
    check(j, rows, pos_cols, var_pos, var_codon, all_four=True)
    check(j, rows, pos_cols[:3], var_pos[:5], var_codon[:5])
    j.close()


def test_repeated_and_growing_calls(ctx):
    """Small, large, small on one matrix, then on matrices of other sizes: the staging and the tables grow and are reused, no stale
    row, position or count shows.  Then a call that only enqueues, its inputs overwritten at once: they were copied before it returned."""
    rows, pos_cols, var_pos, var_codon = make_case(1025, 130, 260, 12)
    ctx.upload_rows(rows)
    check(ctx, rows, pos_cols[:2], var_pos[:3], var_codon[:3])
    check(ctx, rows, pos_cols, var_pos, var_codon, all_four=True)
    check(ctx, rows, pos_cols[:2], var_pos[:3], var_codon[:3])
    check(ctx, rows, pos_cols[:65], var_pos[:129], var_codon[:129])
    for seed, (n, n_pos, n_var) in enumerate(((1500, 3, 4), (9000, 40, 70), (1500, 3, 4))):
        r2, pc, vp, vc = make_case(n, n_pos, n_var, 70 + seed)
        ctx.upload_rows(r2)
        check(ctx, r2, pc, vp, vc, all_four=True)
    ctx.upload_rows(rows)
    cols, vp, vc = pos_cols[:64].copy(), var_pos[:100].copy(), var_codon[:100].copy()
    exp = linkage_mirror.linkage(rows, cols, vp, vc)
    assert ctx.variant_linkage(cols, vp, vc, wait=False) is None
    cols[:] = 0
    vp[:] = 0
    vc[:] = 63
    out = ctx.variant_linkage_fetch()
    for key in exp:
        assert (out[key] == exp[key]).all(), key


def test_refusals_change_nothing():
    lib = capi.load_library()
    j = capi.Juliet(0)
    rows, pos_cols, var_pos, var_codon = make_case(40, 3, 4, 1)           # 8 columns: codons at 0, 1, 4
    n_cols = rows.shape[1]

    def refused(status, word, cols=pos_cols, n_pos=3, vp=var_pos, vc=var_codon, n_var=4):
        ptr = [None if a is None else a.ctypes.data for a in (cols, vp, vc)]
        rc = lib.jl_variant_linkage_async(j.h, ptr[0], n_pos, ptr[1], ptr[2], n_var)
        assert rc == status
        assert word in lib.jl_last_error(j.h).decode(), lib.jl_last_error(j.h)

    refused(-4, "no resident matrix")
    j.upload_rows(rows)
    buf = np.zeros(9, dtype=np.uint32)
    assert lib.jl_variant_linkage_fetch(j.h, buf.ctypes.data, None, None) == -4          # a fetch before any call
    assert "before jl_variant_linkage_async" in lib.jl_last_error(j.h).decode()
    good = j.variant_linkage(pos_cols, var_pos, var_codon)
    exp = linkage_mirror.linkage(rows, pos_cols, var_pos, var_codon)
    for key in exp:
        assert (good[key] == exp[key]).all(), key
    big = np.arange(1025, dtype=np.uint32)
    refused(-1, "no positions array", cols=None)
    refused(-1, "no variant positions array", vp=None)
    refused(-1, "no variant codons array", vc=None)
    refused(-1, "0 positions", n_pos=0)
    refused(-1, "1025 positions", cols=big, n_pos=1025)
    refused(-1, "0 variants", n_var=0)
    refused(-1, "1025 variants", vp=np.zeros(1025, dtype=np.uint32), vc=np.zeros(1025, dtype=np.uint8), n_var=1025)
    refused(-1, "ends beyond the window", cols=np.array([0, 1, n_cols - 2], dtype=np.uint32))
    refused(-1, "not strictly ascending", cols=np.array([0, 4, 4], dtype=np.uint32))
    refused(-1, "not strictly ascending", cols=np.array([1, 0, 4], dtype=np.uint32))
    refused(-1, "beyond the 3 positions", vp=np.array([0, 1, 2, 3], dtype=np.uint32))
    refused(-1, "decreasing", vp=np.array([0, 2, 1, 2], dtype=np.uint32))
    bad = var_codon.copy()
    bad[3] = 64
    refused(-1, "is no codon", vc=bad)
    again = j.variant_linkage_fetch()                                                   # what was enqueued before is still there
    for key in good:
        assert (again[key] == good[key]).all(), key
    # any pointer of the fetch may be NULL
    joint = np.zeros((4, 4), dtype=np.uint32)
    assert lib.jl_variant_linkage_fetch(j.h, None, None, joint.ctypes.data) == 0 and (joint == exp["joint"]).all()
    assert lib.jl_variant_linkage_fetch(j.h, None, None, None) == 0
    assert (msa.unpack_columns(j.download_columns(), 40) == rows).all()
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


def run_and_link(ctx, sp, min_reads):
    """A run with phasing on a synthetic window, then ONE linkage call with the run's own positions and variant rows."""
    n, l = 3000, 300
    ref = synth.reference(sp.seed, l)
    rows = synth.rows(sp, l, 0, n, ref)
    genes = np.array([(1, l + 1)], dtype=capi.GENE)
    ctx.upload_rows(rows)
    ctx.run_async(genes, ref, capi.default_params(), None, True, min_reads, True)
    first = fetch_copy(ctx)
    var, ph = first["variants"], first["phase"]
    pos_cols = ph["pos_cols"]
    assert len(var) >= 4 and len(pos_cols) >= 3 and len(var) <= 256
    assert (np.diff(var["col"].astype(np.int64)) >= 0).all()                 # one gene: the table's order is by column
    var_pos = np.searchsorted(pos_cols, var["col"]).astype(np.uint32)
    assert (pos_cols[var_pos] == var["col"]).all()
    out = check(ctx, rows, pos_cols, var_pos, var["codon"])
    return rows, genes, ref, first, var, var_pos, out


def test_after_a_real_run(ctx):
    """Reads with deletions, masked bases and partial reads: the consequences of §15 hold, the run's results are what they were,
    a second run (the captured graph) equals the first."""
    sp = synth.SynthParams(seed=5, del_rate=4e-3, mask_rate=2e-2, partial_rate=0.1, minor_permille=(150, 120, 100, 80))
    rows, genes, ref, first, var, var_pos, out = run_and_link(ctx, sp, 10)
    s = first["phase"]["summary"]
    assert s["damaged_reads"] > 0
    idx = np.arange(len(var))
    assert (out["carry"][idx, var_pos] == var["count"]).all()
    assert (np.diag(out["both"])[var_pos] == var["coverage"]).all()
    cooc = first["phase"]["cooc"]
    assert cooc.shape == out["joint"].shape and (out["joint"] >= cooc).all() and (out["joint"] > cooc).any()
    assert_same_run(first, fetch_copy(ctx))
    assert (msa.unpack_columns(ctx.download_columns(), len(rows)) == rows).all()
    ctx.run_async(genes, ref, capi.default_params(), None, True, 10, True)
    assert_same_run(first, fetch_copy(ctx))
    ctx.run_async(genes, ref, capi.default_params(), None, True, 10, True)   # (a configuration is captured on its second run: the replay)
    assert_same_run(first, fetch_copy(ctx))


def test_without_damage_joint_is_the_cooccurrence(ctx):
    """No deletion, no masked base, no partial read, every group reported (min_reads 1): every read counts in both tables."""
    sp = synth.SynthParams(seed=6, del_rate=0.0, mask_rate=0.0, partial_rate=0.0, minor_permille=(150, 120, 100, 80))
    rows, genes, ref, first, var, var_pos, out = run_and_link(ctx, sp, 1)
    s = first["phase"]["summary"]
    assert s["damaged_reads"] == 0 and s["insufficient_reads"] == 0 and s["reported_reads"] == len(rows)
    assert (out["joint"] == first["phase"]["cooc"]).all()


def test_the_limits_themselves_are_accepted(ctx):
    """P = V = JL_LINK_MAX is a case of test_linkage_equals_mirror; here the same on overlapping codons, every column a codon start."""
    n, n_cols = 70, capi.LINK_MAX + 2
    rng = np.random.default_rng(8)
    haps = rng.integers(0, 4, size=(3, n_cols), dtype=np.uint8)
    rows = haps[rng.integers(0, 3, size=n)].copy()
    rows[rng.random(size=rows.shape) < 2e-3] = 4
    rows[5] = 6
    pos_cols = np.arange(capi.LINK_MAX, dtype=np.uint32)
    var_codon = (16 * haps[0, :-2] + 4 * haps[0, 1:-1] + haps[0, 2:]).astype(np.uint8)
    ctx.upload_rows(rows)
    out = check(ctx, rows, pos_cols, pos_cols.copy(), var_codon)
    assert out["joint"].max() > 0 and out["both"].max() <= n - 1


# ---------------------------------------------------------------------------------------------- the command line
N_CLI, L_CLI, SEED_CLI = 3000, 300, 41
MINOR = (150, 120, 100, 80)


def read_msa(path):
    raw = open(path, "rb").read()
    n, l, wb = (int(x) for x in np.frombuffer(raw[:24], dtype=np.uint64))
    return np.frombuffer(raw[24:], dtype=np.uint8).reshape(n, l), wb


def juliet(d, *args):
    return subprocess.run([JULIET, *args], cwd=d, capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    """Reads with deletions and filtered bases (the generator's default rates) and one in ten partial; the rows from --dump-msa;
    runs with and without the flag, with and without phasing."""
    d = tmp_path_factory.mktemp("linkage_cli")
    subprocess.check_call([SYNTH, "--reads", str(N_CLI), "--cols", str(L_CLI), "--seed", str(SEED_CLI), "--partial", "0.1",
                           "--minor-permille", *map(str, MINOR), "-o", str(d / "in.bam"), "--config-out", str(d / "cfg.json")])
    subprocess.check_call([JULIET, "-c", "cfg.json", "--dump-msa", "in.msa", "in.bam"], cwd=d)      # host only: no GPU involved
    rows, wb = read_msa(d / "in.msa")
    assert rows.shape[0] == N_CLI
    r = juliet(d, "-c", "cfg.json", "--mode-phasing", "--linkage", "--timing", "in.bam", "l.json", "l.html")
    assert r.returncode == 0, r.stderr
    assert re.search(r"timing linkage\s", r.stderr)                # the stage line of --timing
    for args in (("--mode-phasing", "in.bam", "plain.json", "plain.html"), ("--linkage", "in.bam", "l0.json", "l0.html"),
                 ("in.bam", "plain0.json", "plain0.html")):
        p = juliet(d, "-c", "cfg.json", *args)
        assert p.returncode == 0, p.stderr
    return d, rows, wb


CODON = {a + b + c: 16 * i + 4 * k + m for i, a in enumerate("ACGT") for k, b in enumerate("ACGT") for m, c in enumerate("ACGT")}


def table_rows_of_json(j, wb):
    """The variant table of the JSON in table order: (gene, ref_position, codon string, window column of the codon start)."""
    out = []
    for g in j["genes"]:
        for vp in g["variant_positions"]:
            col = vp["msa"][[m["rel_pos"] for m in vp["msa"]].index(0)]["abs_pos"] - 1 - wb
            found = [(vc["codon"], col) for aa in vp["variant_amino_acids"] for vc in aa["variant_codons"]]
            out += [(g["name"], vp["ref_position"], c, col) for c, col in sorted(found, key=lambda x: CODON[x[0]])]
    return out


def check_block_against_mirror(j, rows, wb):
    """The `linkage` block pair for pair: the mirror over the rows with the JSON's own variant table."""
    table = table_rows_of_json(j, wb)
    lb = j["linkage"]
    cols = sorted({t[3] for t in table})
    assert lb["variant_positions_abs"] == [c + wb + 1 for c in cols] and lb["n_variants"] == len(table) and "skipped" not in lb
    assert cols == sorted(cols) and [t[3] for t in table] == sorted(t[3] for t in table)      # one gene: by column
    var_pos = [cols.index(t[3]) for t in table]
    exp = linkage_mirror.linkage(rows, cols, var_pos, [CODON[t[2]] for t in table])
    pairs = iter(lb["pairs"])
    n_pairs = 0
    for v in range(len(table)):
        for w in range(v + 1, len(table)):
            if var_pos[v] == var_pos[w]:
                continue
            n, n11, n10, n01, n00 = linkage_mirror.pair_table(exp, var_pos, v, w)
            if n == 0:
                continue
            pr = next(pairs)
            n_pairs += 1
            for side, t in (("a", table[v]), ("b", table[w])):
                assert pr[side] == dict(gene=t[0], ref_position=t[1], codon=t[2])
            assert (pr["reads_both"], pr["n11"], pr["n10"], pr["n01"], pr["n00"]) == (n, n11, n10, n01, n00)
            s = linkage_mirror.stats(n11, n10, n01, n00)
            for key in ("r2", "d_prime"):          # relative 1e-13 (tests/test_linkage_host.py)
                assert abs(pr[key] - float(s[key])) <= 1e-13 * abs(float(s[key])), (key, pr[key], float(s[key]))
            for key in ("p_positive", "p_negative"):
                assert abs(pr[key] - float(s[key])) <= 1e-10, (key, pr[key], float(s[key]))
    assert next(pairs, None) is None and lb["n_pairs_tested"] == n_pairs == len(lb["pairs"])
    return n_pairs


def test_cli_block_equals_the_mirror(cli):
    d, rows, wb = cli
    for name in ("l.json", "l0.json"):
        j = json.load(open(d / name))
        assert check_block_against_mirror(j, rows, wb) >= 3                      # nothing passes vacuously
    lb = json.load(open(d / "l.json"))["linkage"]
    assert any(min(p["n11"], p["n10"], p["n01"], p["n00"]) > 0 for p in lb["pairs"])
    assert lb == json.load(open(d / "l0.json"))["linkage"]                       # phasing has no say in it


def strip_json(text):
    j = json.loads(text)
    j["input"].pop("timestamp")
    j["input"].pop("command_line")
    j.pop("linkage", None)
    return json.dumps(j, indent=1)


def strip_html(text):
    text = re.sub(r'<details open id="linkage">.*?</table></details>\n', "", text, flags=re.S)
    return re.sub(r"<tr><th>(timestamp|command_line)</th>.*?</tr>\n", "", text)


def test_cli_without_the_block_the_outputs_are_the_plain_run(cli):
    d, rows, wb = cli
    for with_flag, plain in (("l", "plain"), ("l0", "plain0")):
        assert "linkage" in json.load(open(d / (with_flag + ".json"))) and "linkage" not in json.load(open(d / (plain + ".json")))
        assert strip_json(open(d / (with_flag + ".json")).read()) == strip_json(open(d / (plain + ".json")).read())
        html, plain_html = open(d / (with_flag + ".html")).read(), open(d / (plain + ".html")).read()
        assert 'id="linkage"' in html and 'id="linkage"' not in plain_html
        assert strip_html(html) == strip_html(plain_html)
    # ... and two runs without the flag differ in nothing but the time and the command line: the comparison above is a fair one
    again = juliet(d, "-c", "cfg.json", "--mode-phasing", "in.bam", "again.json", "again.html")
    assert again.returncode == 0
    assert strip_json(open(d / "again.json").read()) == strip_json(open(d / "plain.json").read())
    assert strip_html(open(d / "again.html").read()) == strip_html(open(d / "plain.html").read())


def json_number(v):
    """A number as the JSON writer prints it."""
    return "%.0f" % v if v == int(v) else "%.17g" % v


def test_cli_html_holds_every_leaf(cli):
    d, rows, wb = cli
    lb = json.load(open(d / "l.json"))["linkage"]
    html = open(d / "l.html").read()
    block = re.search(r'<details open id="linkage">.*?</table></details>', html, flags=re.S).group(0)
    assert re.findall(r'<tr data-key="(\w+)"><th>\w+</th><td>(\d+)</td>', block) == [("n_variants", str(lb["n_variants"])),
                                                                                     ("n_pairs_tested", str(lb["n_pairs_tested"]))]
    assert [int(x) for x in re.findall(r"<span>(\d+)</span>", block)] == lb["variant_positions_abs"]
    got = [re.findall(r"<td>(.*?)</td>", tr) for tr in re.findall(r"<tr><td>.*?</tr>", block)]
    assert len(got) == len(lb["pairs"])
    for cells, p in zip(got, lb["pairs"]):
        want = [p["a"]["gene"], str(p["a"]["ref_position"]), p["a"]["codon"], p["b"]["gene"], str(p["b"]["ref_position"]), p["b"]["codon"]]
        want += [json_number(p[k]) for k in ("reads_both", "n11", "n10", "n01", "n00", "r2", "d_prime", "p_positive", "p_negative")]
        assert cells == want


def test_cli_follows_the_taken_window(cli):
    d, rows, wb = cli
    r = juliet(d, "-c", "cfg.json", "--linkage", "--downsample", "1000", "--sample-seed", "3", "in.bam", "ds.json")
    assert r.returncode == 0, r.stderr
    j = json.load(open(d / "ds.json"))
    assert j["target_config"]["n_reads"] == 1000
    kept = capi.sample_reads(len(rows), 1000, 3)                 # docs/SPEC.md §12: host arithmetic, no device
    assert check_block_against_mirror(j, rows[kept], wb) >= 1
    assert j["linkage"] != json.load(open(d / "l0.json"))["linkage"]


def test_cli_no_variant_is_the_empty_block(tmp_path):
    """Reads without a minor clone: nothing is called, no call is made; the block has empty arrays and exit status 0."""
    subprocess.check_call([SYNTH, "--reads", "400", "--cols", "90", "--seed", "3", "--minor-permille", "0", "0", "0", "0",
                           "-o", str(tmp_path / "in.bam"), "--config-out", str(tmp_path / "cfg.json")])
    for phasing in ([], ["--mode-phasing"]):
        r = juliet(tmp_path, "-c", "cfg.json", *phasing, "--linkage", "in.bam", "out.json", "out.html")
        assert r.returncode == 0, r.stderr
        assert json.load(open(tmp_path / "out.json"))["linkage"] == dict(variant_positions_abs=[], n_variants=0, n_pairs_tested=0, pairs=[])
        assert 'id="linkage"' in open(tmp_path / "out.html").read()


@pytest.mark.parametrize("args", [["--windows", "2"], ["--devices", "0,0"], ["--mode-phasing", "--windows", "3"]])
def test_cli_refused_combinations_open_nothing(tmp_path, args):
    r = juliet(tmp_path, "--linkage", *args, "no_such.bam", "o.json")
    assert r.returncode == 1 and "--linkage" in r.stderr, (r.returncode, r.stderr)
    assert not list(tmp_path.iterdir())


def test_cli_refused_with_batch_and_as_fuse(tmp_path):
    (tmp_path / "l.tsv").write_text("no_such.bam\ta.json\n")
    r = juliet(tmp_path, "--linkage", "--batch", "l.tsv")
    assert r.returncode == 1 and "--linkage" in r.stderr and "--batch" in r.stderr
    r = subprocess.run([os.path.join(ROOT, "minorseq_amd", "bin", "fuse"), "--linkage", "no_such.bam", "o.fasta"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--linkage" in r.stderr and "fuse" in r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == ["l.tsv"]
