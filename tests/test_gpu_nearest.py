"""jl_phase_nearest_async on the device (docs/SPEC.md §22): which reported haplotype a read is nearest to within a budget of
differing codon positions, and `juliet --mode-phasing --absorb-distance` on top of it.  Every expectation is
tests/nearest_mirror.py — the rule in plain loops — over the rows that were uploaded, compared for equality on every read; never
another device result."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import nearest_mirror
import rescue_mirror
import second_turn as st
from minorseq_amd import capi, msa, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JULIET = os.path.join(ROOT, "minorseq_amd", "bin", "juliet")
SYNTH = os.path.join(ROOT, "minorseq_amd", "bin", "juliet-synth")

U, NONE, AMB = nearest_mirror.UNINFORMATIVE, nearest_mirror.NONE, nearest_mirror.AMBIGUOUS


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


def own_column(pos_cols, p):
    """The column of codon p that no other codon shares: changing it changes this codon position alone."""
    return 0 if p == 0 else int(pos_cols[p]) + 2


def codons_at(base_rows, pos_cols):
    c = pos_cols.astype(np.int64)
    return (16 * base_rows[:, c] + 4 * base_rows[:, c + 1] + base_rows[:, c + 2]).astype(np.uint8)


# Families of haplotype numbers, the base first: member j is the base changed at j codons.  Numbers that differ in the low six bits
# only (lanes of one chunk, neighbours and across DPP rows), in bit 6 and above only (one lane, several chunks), and in both; each
# kind once with the base at the lower number and once at the higher, so that the nearer haplotype is met first and last.
FAMILIES = [(0, 1, 2, 3), (5, 4), (18, 47), (7, 71, 135), (73, 9), (10, 97), (161, 34), (520, 8), (300, 690), (700, 701, 640)]


def make_case(n, vp, n_hap, d_budget, seed):
    """Seeded haplotype rows whose bases at every codon's own column are A, C or G — so a read with T there differs from every
    haplotype at that position — in FAMILIES; reads that are copies of a haplotype with, in turn: 0 .. D + 2 codon substitutions;
    8, 15, 16, 17, 32, 33 of them (distances a four-bit counter would wrap); T at every codon's own column (differs from every
    haplotype at all positions); the one codon changed or opened at which two members of a family differ (equidistant from both);
    scattered '-' and N cells; ragged code-6 ends; code 6 throughout.  Returns (rows, pos_cols, pattern)."""
    rng = np.random.default_rng(seed)
    pos_cols, n_cols = positions(vp)
    own = np.array([own_column(pos_cols, p) for p in range(vp)])
    haps = rng.integers(0, 4, size=(n_hap, n_cols), dtype=np.uint8)
    haps[:, own] = rng.integers(0, 3, size=(n_hap, vp), dtype=np.uint8)
    families = []
    for fam in FAMILIES:
        fam = [h for h in fam if h < n_hap]
        if len(fam) < 2:
            continue
        where = rng.permutation(vp)                                   # member j: the base changed at where[0 .. j - 1]
        for j, h in enumerate(fam[1:], 1):
            haps[h] = haps[fam[0]]
            for p in where[:j]:
                haps[h, own[p]] = (haps[fam[0], own[p]] + 1 + (int(p) + h) % 2) % 3
        families.append((fam, where))
    members = [h for fam, _ in families for h in fam]
    turns = [("sub", s) for s in range(d_budget + 3)] + [("sub", s) for s in (8, 15, 16, 17, 32, 33)] + \
            [("far", 0), ("tie", 1), ("tie", 0), ("scattered", 0), ("ragged", 0), ("out", 0)]
    rows = np.zeros((n, n_cols), dtype=np.uint8)
    for i in range(n):
        kind, s = turns[i % len(turns)]
        h = int(rng.choice(members)) if members and rng.random() < 0.5 else int(rng.integers(0, n_hap))
        rows[i] = haps[h]
        if kind == "sub":
            for p in rng.permutation(vp)[:s]:
                rows[i, own[p]] = (rows[i, own[p]] + 1 + rng.integers(0, 3)) % 4
        elif kind == "far":
            rows[i, own] = 3
        elif kind == "tie" and families:
            fam, where = families[(i // len(turns)) % len(families)]
            rows[i] = haps[fam[int(rng.integers(0, 2))]]                  # the base or its first copy: they differ at where[0]
            rows[i, own[where[0]]] = 3 if s else 4 + int(rng.integers(0, 3))
        elif kind == "scattered":
            cell = rng.random(size=n_cols)
            rows[i, cell < 1.5 / n_cols] = 4
            rows[i, cell > 1.0 - 1.5 / n_cols] = 5
            c = int(rng.integers(0, n_cols))
            rows[i, c] = (rows[i, c] + 1) % 4                             # ... and one substitution somewhere
        elif kind == "ragged":
            lo, hi = int(rng.integers(0, n_cols // 3 + 1)), n_cols - int(rng.integers(0, n_cols // 3 + 1))
            rows[i, :lo] = 6
            rows[i, hi:] = 6
        elif kind == "out":
            rows[i] = 6
    return rows, pos_cols, codons_at(haps, pos_cols)


def check(j, rows, pos_cols, pattern, min_positions, d_budget, expected=None):
    exp = expected or nearest_mirror.nearest(rows, pos_cols, pattern, min_positions, d_budget)
    out = j.phase_nearest(pos_cols, pattern, min_positions, d_budget)
    assert out["nearest"].dtype == np.uint16 and out["nearest"].shape == (len(rows),)
    assert out["dist"].dtype == np.uint8 and out["dist"].shape == (len(rows),)
    assert out["hap_reads"].shape == (len(pattern), d_budget + 1)
    assert (out["nearest"] == exp[0]).all()
    assert (out["dist"] == exp[1]).all()
    assert (out["hap_reads"] == exp[2]).all()
    assert (out["tally"] == exp[3]).all()
    assert int(out["tally"].sum()) == len(rows)
    return out


# (reads, positions, haplotypes, D, min_positions or "vp", what the case is asked to hold): the word / run of 64 / two-workgroup
# edges of the reads, the tile of 64 positions, the dword of four and the counter's 15 / 16 / 17, the chunk of 64 haplotypes (ids
# with bit 9 at 513 and 702), every budget; every value once and the corners together.  Held: "4" all four categories occur,
# "d" every distance 0 .. D occurs among the assigned, "far" some read is 16 or more from its nearest haplotype — asked of every
# shape that can hold it (not of one read, of one haplotype — nothing ties — of 33 reads that must be readable at all 65
# positions, nor "far" below 16 positions)
CASES = [
    (2049, 130, 702, 7, 1, "4 d far"), (1, 1, 1, 0, 1, "d"), (31, 2, 2, 1, 1, "4 d"), (32, 4, 63, 3, 2, "4 d"),
    (33, 5, 64, 3, "vp", "4 d"), (64, 15, 65, 7, 1, "4 d"), (65, 16, 128, 7, 2, "4 d far"), (1023, 17, 129, 3, 1, "4 d far"),
    (1024, 63, 513, 1, 2, "4 d far"), (1025, 64, 702, 0, 1, "4 d far"), (2049, 65, 2, 7, "vp", "4 d far"), (1025, 130, 1, 3, 1, "d far"),
    (1024, 1, 64, 0, 1, "4 d"), (1023, 2, 63, 1, 2, "4 d"), (2049, 16, 65, 3, 1, "4 d far"), (65, 130, 702, 1, 2, "4 d far"),
    (1, 130, 702, 7, 1, ""), (33, 65, 513, 0, "vp", "d far"), (64, 64, 129, 7, 1, "4 d far"), (1025, 17, 128, 7, 2, "4 d far"),
    (32, 63, 64, 1, 1, "4 d far"), (31, 15, 129, 3, 2, "4 d"), (1023, 5, 513, 1, 1, "4 d"), (2049, 4, 702, 0, 2, "4 d"),
]


def seed_of(n, vp, n_hap, d_budget):
    return 1000 * n + 7 * vp + n_hap + 100003 * d_budget


def assert_not_vacuous(rows, pos_cols, pattern, exp, d_budget, held):
    near, dist, hap_reads, tally = exp
    if "4" in held:
        assert (tally > 0).all(), tally
    if "d" in held:
        assert (hap_reads.sum(axis=0) > 0).all(), hap_reads.sum(axis=0)
    if "far" in held:
        assert nearest_mirror.true_distance(rows, pos_cols, pattern).max() >= 16


@pytest.mark.parametrize("n,vp,n_hap,d_budget,min_positions,held", CASES)
def test_nearest_equals_mirror(ctx, n, vp, n_hap, d_budget, min_positions, held):
    rows, pos_cols, pattern = make_case(n, vp, n_hap, d_budget, seed_of(n, vp, n_hap, d_budget))
    assert pos_cols[0] == 0 and pos_cols[-1] == rows.shape[1] - 3 and (vp < 2 or pos_cols[1] == 1)
    k = vp if min_positions == "vp" else min_positions
    exp = nearest_mirror.nearest(rows, pos_cols, pattern, k, d_budget)
    assert_not_vacuous(rows, pos_cols, pattern, exp, d_budget, held)
    ctx.upload_rows(rows, win_begin=3)
    check(ctx, rows, pos_cols, pattern, k, d_budget, exp)
    assert (msa.unpack_columns(ctx.download_columns(), n) == rows).all()     # the matrix is untouched


# (positions, haplotypes): two chunks of haplotypes at few positions, two tiles of positions at few haplotypes; D = 3
SECOND_TURN_SHAPES = [(5, 65), (65, 2)]
SECOND_TURN_D = 3


def second_turn_block(vp, n_hap):
    """The 2049-read case of this file's builder at the shape, cut to the block of st.BLOCK reads; (block, pos_cols, pattern)."""
    rows, pos_cols, pattern = make_case(2049, vp, n_hap, SECOND_TURN_D, seed_of(2049, vp, n_hap, SECOND_TURN_D))
    return rows[:st.BLOCK], pos_cols, pattern


def second_turn_expectation(block, pos_cols, pattern, n):
    """(nearest, dist, hap_reads, tally) of the n tiled reads from the mirror over the block and over the tail."""
    whole = nearest_mirror.nearest(block, pos_cols, pattern, 1, SECOND_TURN_D)
    tail = nearest_mirror.nearest(block[:st.split(n)[1]], pos_cols, pattern, 1, SECOND_TURN_D)
    return st.tiled(whole[0], n), st.tiled(whole[1], n), st.summed(whole[2], tail[2], n, st.BLOCK), st.summed(whole[3], tail[3], n, st.BLOCK)


@pytest.mark.parametrize("vp,n_hap", SECOND_TURN_SHAPES)
@pytest.mark.parametrize("n,what", st.COUNTS)
def test_a_workgroups_second_turn(n, what, vp, n_hap):
    """More than 4096 runs: a workgroup walks a second run — its distances and `informative` start again, its histogram and tallies
    are carried into one flush.  The rows are the block repeated (tests/second_turn.py)."""
    block, pos_cols, pattern = second_turn_block(vp, n_hap)
    exp = second_turn_expectation(block, pos_cols, pattern, n)
    assert int(exp[3].sum()) == n
    if n - st.ONE_TURN > 1:                                 # all four categories and every distance among the reads of the second turns
        late, late_d = exp[0][st.second_turn_reads(n)], exp[1][st.second_turn_reads(n)]
        assert (late < n_hap).any() and (late == AMB).any() and (late == NONE).any() and (late == U).any()
        assert set(late_d[late < n_hap].tolist()) == set(range(SECOND_TURN_D + 1))
    j = capi.Juliet(0)
    try:
        st.adopt_tiled(j, block, n)
        out = j.phase_nearest(pos_cols, pattern, 1, SECOND_TURN_D)
        assert out["nearest"].shape == (n,) and (out["nearest"] == exp[0]).all(), np.flatnonzero(out["nearest"] != exp[0])[:8]
        assert (out["dist"] == exp[1]).all(), np.flatnonzero(out["dist"] != exp[1])[:8]
        assert (out["hap_reads"] == exp[2]).all() and (out["tally"] == exp[3]).all()
        assert int(out["tally"].sum()) == n
    finally:
        j.close()


def test_the_counter_saturates(ctx):
    """33 positions, two haplotypes that differ everywhere, reads at exactly 7, 8, 15, 16, 17, 32 and 33 codons from haplotype 1 (and
    33 from haplotype 0), D = 7: a counter of four bits that wrapped would find 16, 17, 32 and 33 within the budget.  Only the first
    is assigned."""
    vp = 33
    pos_cols, n_cols = positions(vp)
    own = np.array([own_column(pos_cols, p) for p in range(vp)])
    haps = np.zeros((2, n_cols), dtype=np.uint8)
    haps[1, own] = 1
    steps = [7, 8, 15, 16, 17, 32, 33]
    rows = np.repeat(haps[1:2], len(steps), axis=0)
    for i, s in enumerate(steps):
        rows[i, own[:s]] = 2
    pattern = codons_at(haps, pos_cols)
    assert nearest_mirror.true_distance(rows, pos_cols, pattern).tolist() == steps
    ctx.upload_rows(rows)
    out = check(ctx, rows, pos_cols, pattern, 1, 7)
    assert out["nearest"].tolist() == [1] + [NONE] * 6 and out["dist"].tolist() == [7] + [8] * 6
    assert out["hap_reads"].tolist() == [[0] * 8, [0] * 7 + [1]] and out["tally"].tolist() == [1, 0, 6, 0]


def test_budget_zero_is_the_rescue_and_budgets_nest(ctx):
    """Consequences (a) and (b) of §22 on one upload: D = 0 equals the RESCUE's mirror on every read; dmin and the haplotype at it
    do not depend on D, so a read assigned at one budget is assigned to the same haplotype at distance dmin at every larger one."""
    n, vp, n_hap = 1025, 65, 129
    rows, pos_cols, pattern = make_case(n, vp, n_hap, 7, 31)
    ctx.upload_rows(rows)
    out0 = ctx.phase_nearest(pos_cols, pattern, 2, 0)
    exp_rescue, exp_reads, exp_tally = rescue_mirror.rescue(rows, pos_cols, pattern, 2)
    assert (exp_tally > 0).all()
    assert (out0["nearest"] == exp_rescue).all() and (out0["hap_reads"][:, 0] == exp_reads).all() and (out0["tally"] == exp_tally).all()
    outs = {d: check(ctx, rows, pos_cols, pattern, 2, d) for d in (1, 3, 7)}
    outs[0] = out0
    for lo, hi in ((0, 1), (1, 3), (3, 7)):
        a, b = outs[lo], outs[hi]
        was = a["nearest"] < n_hap
        assert was.sum() < (b["nearest"] < n_hap).sum()                       # the larger budget takes more reads in
        assert (b["nearest"][was] == a["nearest"][was]).all() and (b["dist"][was] == a["dist"][was]).all()
        amb = a["nearest"] == AMB
        assert (b["nearest"][amb] == AMB).all() and (b["dist"][amb] == a["dist"][amb]).all()
        assert ((a["nearest"] == U) == (b["nearest"] == U)).all()
        assert (b["hap_reads"][:, :lo + 1] == a["hap_reads"]).all()


def test_adopted_matrix_with_its_own_stride():
    """A torch tensor as the matrix: 2049 reads in planes of 272 bytes (the library's own stride is 384), garbage in the bytes
    past ceil(n / 8) of every plane row.  None of it may show in any read's answer or in a count."""
    import torch
    n, vp, n_hap, stride = 2049, 65, 129, 272
    assert stride != msa.plane_stride(n) and stride % 16 == 0
    rows, pos_cols, pattern = make_case(n, vp, n_hap, 3, 99)
    planes = msa.pack_planes(rows, stride)
    planes[:, :, (n + 7) // 8:] = np.random.default_rng(1).integers(0, 256, size=(rows.shape[1], 3, stride - (n + 7) // 8), dtype=np.uint8)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t = torch.from_numpy(planes).cuda(non_blocking=False)
    stream.synchronize()
    j = capi.Juliet(0, stream=stream.cuda_stream)
    j.adopt(t.data_ptr(), n, rows.shape[1], stride, keep_alive=t)
    out = check(j, rows, pos_cols, pattern, 1, 3)
    assert (out["tally"] > 0).all()
    check(j, rows, pos_cols[:3], pattern[:2, :3], 3, 7)
    j.close()


def test_repeat_on_one_context(ctx):
    """(130, 702, D = 7), then (2, 2, D = 0), then (65, 129, D = 3) on one matrix: no stale pattern, position, id, distance or count
    shows.  Then a call that only enqueues, its inputs overwritten at once: they were copied before it returned."""
    n = 1025
    rows, pos_cols, pattern = make_case(n, 130, 702, 7, 12)
    ctx.upload_rows(rows)
    check(ctx, rows, pos_cols, pattern, 1, 7)
    check(ctx, rows, pos_cols[:2], pattern[:2, :2].copy(), 2, 0)
    check(ctx, rows, pos_cols[:65], pattern[:129, :65].copy(), 1, 3)
    cols, pat = pos_cols[:64].copy(), pattern[:65, :64].copy()
    exp = nearest_mirror.nearest(rows, cols, pat, 2, 1)
    assert ctx.phase_nearest(cols, pat, 2, 1, wait=False) is None
    cols[:] = 0
    pat[:] = 63
    out = ctx.phase_nearest_fetch()
    for key, e in zip(("nearest", "dist", "hap_reads", "tally"), exp):
        assert (out[key] == e).all(), key


def test_staging_grows_and_is_reused(ctx):
    """1500 reads and 3 positions, then 5000 and 40, then 1500 and 3 again, at 60 columns on one context: the staging of positions
    and pattern and the buffers of ids and distances grow for the second call and serve the third, larger than it needs."""
    l, n_hap = 60, 9
    for seed, (n, cols) in enumerate(((1500, [0, 1, 57]), (5000, list(range(20)) + list(range(38, 58))), (1500, [0, 1, 57]))):
        rng = np.random.default_rng(70 + seed)
        pos_cols = np.array(cols, dtype=np.uint32)
        haps = rng.integers(0, 4, size=(n_hap, l), dtype=np.uint8)
        rows = haps[rng.integers(0, n_hap, size=n)]
        cell = rng.random(size=rows.shape)
        rows[cell < 0.01] = 4                       # scattered '-', N and uncovered cells
        rows[cell > 0.99] = 5
        rows[(cell > 0.49) & (cell < 0.50)] = 6
        sub = (cell > 0.200) & (cell < 0.210) & (rows < 4)      # substitutions: one read in two has one or more
        rows[sub] = (rows[sub] + 1) % 4
        ctx.upload_rows(rows)
        out = check(ctx, rows, pos_cols, codons_at(haps, pos_cols), 1 if len(cols) == 3 else 2, 2)
        assert out["hap_reads"][:, 1].sum() > 0


def fetch_copy(j):
    out = j.run_fetch(True, True, cap_var=64)
    return dict(variants=out["variants"].copy(), phase={k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in out["phase"].items()})


def assert_same_run(a, b):
    assert (a["variants"] == b["variants"]).all()
    pa, pb = a["phase"], b["phase"]
    assert pa["summary"] == pb["summary"]
    for key in ("pos_cols", "hap_count", "hap_pattern", "hit", "read_hap", "cooc"):
        assert (pa[key] == pb[key]).all(), key


def test_after_a_real_run(ctx):
    """A run with phasing over reads with a raised substitution rate, deletions, masked bases and partial reads; then the rule with the
    run's own positions and haplotypes, over all reads: consequences (c) and (d) of §22 hold, the run's results and the matrix are
    what they were, a second run equals the first."""
    n, l = 2049, 130
    sp = synth.SynthParams(seed=5, sub_rate=4e-3, del_rate=4e-3, mask_rate=2e-2, partial_rate=0.1, minor_permille=(150, 120, 100, 80))
    ref = synth.reference(sp.seed, l)
    rows = synth.rows(sp, l, 0, n, ref)
    genes = np.array([(1, l + 1)], dtype=capi.GENE)
    ctx.upload_rows(rows)
    ctx.run_async(genes, ref, capi.default_params(), None, True, 10, True)
    first = fetch_copy(ctx)
    ph = first["phase"]
    n_hap, vp = ph["summary"]["n_haplotypes"], ph["summary"]["n_positions"]
    read_hap, pos_cols, pattern = ph["read_hap"], ph["pos_cols"][:vp], ph["hap_pattern"][:n_hap, :vp]
    insufficient = read_hap == capi.HAP_INSUFFICIENT
    assert n_hap >= 2 and vp >= 2
    assert ph["summary"]["insufficient_reads"] >= 1 and ph["summary"]["damaged_reads"] >= 1
    assert insufficient.sum() == ph["summary"]["insufficient_reads"]
    for d_budget in (1, 3):
        out = check(ctx, rows, pos_cols, pattern, 1, d_budget)
        near, dist = out["nearest"], out["dist"]
        for h in range(n_hap):
            assert (near[read_hap == h] == h).all() and (dist[read_hap == h] == 0).all()      # (c)
            assert out["hap_reads"][h, 0] >= ph["hap_count"][h]
        assert (dist[insufficient] >= 1).all()                                                # (d)
        assert (insufficient & (near < n_hap)).sum() >= 1                                      # ... and some of them are taken in
    assert_same_run(first, fetch_copy(ctx))
    assert (msa.unpack_columns(ctx.download_columns(), n) == rows).all()
    ctx.run_async(genes, ref, capi.default_params(), None, True, 10, True)
    assert_same_run(first, fetch_copy(ctx))


def test_refusals_change_nothing():
    lib = capi.load_library()
    j = capi.Juliet(0)
    rows, pos_cols, pattern = make_case(40, 3, 4, 1, 1)           # 8 columns: codons at 0, 1, 4
    n_cols = rows.shape[1]

    def refused(status, word, cols=pos_cols, n_pos=3, pat=pattern, stride=3, n_hap=4, min_positions=1, max_distance=1):
        rc = lib.jl_phase_nearest_async(j.h, None if cols is None else cols.ctypes.data, n_pos, None if pat is None else pat.ctypes.data,
                                        stride, n_hap, min_positions, max_distance)
        assert rc == status
        assert word in lib.jl_last_error(j.h).decode(), lib.jl_last_error(j.h)

    refused(-4, "no resident matrix")
    j.upload_rows(rows)
    res = np.zeros(40, dtype=np.uint16)
    assert lib.jl_phase_nearest_fetch(j.h, res.ctypes.data, None, None, None) == -4     # a fetch before any call
    assert "before jl_phase_nearest_async" in lib.jl_last_error(j.h).decode()
    good = j.phase_nearest(pos_cols, pattern, 2, 1)
    exp = nearest_mirror.nearest(rows, pos_cols, pattern, 2, 1)
    assert (good["nearest"] == exp[0]).all() and (good["dist"] == exp[1]).all()
    big_cols = np.arange(4097, dtype=np.uint32)
    big_pat = np.zeros((703, 3), dtype=np.uint8)
    refused(-1, "no positions array", cols=None)
    refused(-1, "no pattern array", pat=None)
    refused(-1, "0 positions", n_pos=0)
    refused(-1, "4097 positions", cols=big_cols, n_pos=4097, stride=4097)
    refused(-1, "0 haplotypes", n_hap=0)
    refused(-1, "703 haplotypes", pat=big_pat, n_hap=703)
    refused(-1, "pattern_stride", stride=2)
    refused(-1, "min_positions 0", min_positions=0)
    refused(-1, "min_positions 4", min_positions=4)
    refused(-1, "max_distance 8", max_distance=8)
    refused(-1, "max_distance 4294967295", max_distance=0xFFFFFFFF)
    refused(-1, "ends beyond the window", cols=np.array([0, 1, n_cols - 2], dtype=np.uint32))
    refused(-1, "not strictly ascending", cols=np.array([0, 4, 4], dtype=np.uint32))
    refused(-1, "not strictly ascending", cols=np.array([1, 0, 4], dtype=np.uint32))
    bad = pattern.copy()
    bad[3, 2] = 64
    refused(-1, "is no codon", pat=bad)
    again = j.phase_nearest_fetch()                                                   # what was enqueued before is still there
    for key in good:
        assert (again[key] == good[key]).all(), key
    # any pointer of the fetch may be NULL
    tally = np.zeros(4, dtype=np.uint64)
    dist = np.zeros(40, dtype=np.uint8)
    assert lib.jl_phase_nearest_fetch(j.h, None, None, None, tally.ctypes.data) == 0 and (tally == exp[3]).all()
    assert lib.jl_phase_nearest_fetch(j.h, None, dist.ctypes.data, None, None) == 0 and (dist == exp[1]).all()
    assert lib.jl_phase_nearest_fetch(j.h, None, None, None, None) == 0
    assert (msa.unpack_columns(j.download_columns(), 40) == rows).all()
    j.close()


def test_the_limits_themselves_are_accepted(ctx):
    """H = 702 at D = 7 (here and in CASES), and the variant table's capacity itself: 4096 positions on 4098 columns, every codon
    overlapping its neighbours, 70 reads."""
    n, n_cols, n_hap = 70, 4098, 702
    rng = np.random.default_rng(8)
    haps = rng.integers(0, 4, size=(n_hap, n_cols), dtype=np.uint8)
    haps[3:] = haps[rng.integers(0, 3, size=n_hap - 3)]                 # three distinct rows and copies of them, each changed at a few bases
    for h in range(3, n_hap):
        haps[h, rng.integers(0, n_cols, size=40)] = rng.integers(0, 4, size=40)
    rows = haps[rng.integers(0, n_hap, size=n)].copy()
    for i in range(n):                                                  # i // 10 bases changed: up to three codons each
        for c in rng.integers(2, n_cols - 2, size=i // 10):
            rows[i, c] = (rows[i, c] + 1) % 4
    rows[rng.random(size=rows.shape) < 2e-4] = 4
    rows[5] = 6
    pos_cols = np.arange(4096, dtype=np.uint32)
    ctx.upload_rows(rows)
    out = check(ctx, rows, pos_cols, codons_at(haps, pos_cols), 4000, 7)
    assert out["tally"][0] > 0 and out["tally"][3] > 0 and out["hap_reads"][:, 1:].sum() > 0


def test_rescue_and_nearest_keep_their_own_results(ctx):
    """The last rescue's results are fetchable and unchanged after a nearest call, and the other way round."""
    rows, pos_cols, pattern = make_case(1025, 17, 65, 3, 5)
    ctx.upload_rows(rows)
    res = ctx.phase_rescue(pos_cols, pattern, 1)
    near = check(ctx, rows, pos_cols[:5], pattern[:9, :5].copy(), 2, 3)
    again = ctx.phase_rescue_fetch()
    for key in res:
        assert (again[key] == res[key]).all(), key
    exp = rescue_mirror.rescue(rows, pos_cols, pattern, 1)
    assert (again["rescue"] == exp[0]).all() and (again["hap_reads"] == exp[1]).all() and (again["tally"] == exp[2]).all()
    ctx.phase_rescue(pos_cols[:4], pattern[:3, :4].copy(), 1)
    after = ctx.phase_nearest_fetch()
    for key in near:
        assert (after[key] == near[key]).all(), key


# ---------------------------------------------------------------------------------------------- the command line
N_CLI, L_CLI, SEED_CLI = 3000, 300, 41
MINOR = (150, 120, 100, 80)
NEW_HAP_KEYS = ("absorbed_reads", "absorbed_damaged_reads", "absorbed_read_names", "frequency_with_absorbed")
RESCUE_HAP_KEYS = ("rescued_reads", "rescued_read_names", "frequency_with_rescued")
CATEGORIES = ("assigned_reads", "ambiguous_reads", "distant_reads", "uninformative_reads")


def read_msa(path):
    raw = open(path, "rb").read()
    n, l, wb = (int(x) for x in np.frombuffer(raw[:24], dtype=np.uint64))
    return np.frombuffer(raw[24:], dtype=np.uint8).reshape(n, l), wb


def juliet(d, *args):
    return subprocess.run([JULIET, *args], cwd=d, capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    """Reads with a raised substitution rate, deletions and filtered bases, one in ten partial; the rows from --dump-msa; runs
    with --absorb-distance 1 and 2, each with and without --rescue-damaged, one with --rescue-damaged alone and one plain."""
    d = tmp_path_factory.mktemp("absorb_cli")
    subprocess.check_call([SYNTH, "--reads", str(N_CLI), "--cols", str(L_CLI), "--seed", str(SEED_CLI), "--partial", "0.1", "--sub", "0.004",
                           "--minor-permille", *map(str, MINOR), "-o", str(d / "in.bam"), "--config-out", str(d / "cfg.json")])
    subprocess.check_call([JULIET, "-c", "cfg.json", "--dump-msa", "in.msa", "in.bam"], cwd=d)      # host only: no GPU involved
    rows, wb = read_msa(d / "in.msa")
    assert rows.shape[0] == N_CLI
    for name, flags in (("a1", ["--absorb-distance", "1", "--timing"]), ("a2", ["--absorb-distance", "2"]),
                        ("ar1", ["--absorb-distance", "1", "--rescue-damaged"]), ("ar2", ["--rescue-damaged", "--absorb-distance", "2"]),
                        ("r", ["--rescue-damaged"]), ("plain", [])):
        r = juliet(d, "-c", "cfg.json", "--mode-phasing", *flags, "in.bam", name + ".json", name + ".html")
        assert r.returncode == 0, r.stderr
        if "--timing" in flags:
            assert re.search(r"timing absorb\b", r.stderr), r.stderr                   # the stage line of --timing
    return d, rows, wb


def index_of(name):
    return int(name.split("/")[1])


def categories_of_json(j, rows, wb):
    """From the JSON's own positions, codons and read names: (pos_cols, pattern, insufficient per read, damaged per read)."""
    hb = j["haplotype"]
    pos_cols = np.array([p - wb - 1 for p in hb["variant_positions_abs"]], dtype=np.uint32)
    pattern = np.array([[16 * "ACGT".index(c[0]) + 4 * "ACGT".index(c[1]) + "ACGT".index(c[2]) for c in h["codons"]] for h in hb["haplotypes"]],
                       dtype=np.uint8).reshape(len(hb["haplotypes"]), len(pos_cols))
    damaged = np.zeros(len(rows), dtype=bool)                  # §8: a code above T at any cell of any variant codon
    for c in pos_cols:
        damaged |= (rows[:, c:c + 3] >= 4).any(axis=1)
    reported = np.zeros(len(rows), dtype=bool)
    for h in hb["haplotypes"]:
        reported[[index_of(name) for name in h["read_names"]]] = True
    assert not (reported & damaged).any()
    insufficient = ~reported & ~damaged
    assert damaged.sum() == hb["damaged_reads"] and insufficient.sum() == hb["insufficient_coverage_reads"]
    return pos_cols, pattern, insufficient, damaged


def check_absorb_against_mirror(j, rows, wb, d_budget):
    hb = j["haplotype"]
    haps = hb["haplotypes"]
    pos_cols, pattern, insufficient, damaged = categories_of_json(j, rows, wb)
    near, dist, _, _ = nearest_mirror.nearest(rows, pos_cols, pattern, d_budget + 1, d_budget)
    ab = hb["absorb"]
    assert sorted(ab) == ["damaged", "insufficient", "max_distance", "min_positions"]
    assert ab["max_distance"] == d_budget and ab["min_positions"] == d_budget + 1
    for key, of_kind, total in (("insufficient", insufficient, hb["insufficient_coverage_reads"]), ("damaged", damaged, hb["damaged_reads"])):
        blk = ab[key]
        assert sorted(blk) == sorted(CATEGORIES + ("assigned_by_distance",))
        assert blk["assigned_reads"] == (of_kind & (near < len(haps))).sum()
        assert blk["ambiguous_reads"] == (of_kind & (near == AMB)).sum()
        assert blk["distant_reads"] == (of_kind & (near == NONE)).sum()
        assert blk["uninformative_reads"] == (of_kind & (near == U)).sum()
        assert sum(blk[c] for c in CATEGORIES) == total
        assert blk["assigned_by_distance"] == [int((of_kind & (near < len(haps)) & (dist == d)).sum()) for d in range(d_budget + 1)]
        assert sum(blk["assigned_by_distance"]) == blk["assigned_reads"] > 0
    assert ab["insufficient"]["assigned_by_distance"][0] == 0          # a read that matches a reported haplotype is no insufficient read
    assert ab["damaged"]["assigned_by_distance"][0] > 0
    total = sum(h["reads"] + h["absorbed_reads"] + h["absorbed_damaged_reads"] for h in haps)
    for k, h in enumerate(haps):
        got = [index_of(name) for name in h["absorbed_read_names"]]
        assert got == np.flatnonzero((insufficient | damaged) & (near == k)).tolist()      # exactly the mirror's reads, in read order
        assert h["absorbed_reads"] == (insufficient & (near == k)).sum()
        assert h["absorbed_damaged_reads"] == (damaged & (near == k)).sum()
        assert h["frequency_with_absorbed"] == (h["reads"] + h["absorbed_reads"] + h["absorbed_damaged_reads"]) / total
        assert all(near[index_of(name)] == k and dist[index_of(name)] == 0 for name in h["read_names"])      # consequence (c)
    return ab


@pytest.mark.parametrize("name,d_budget", [("a1", 1), ("a2", 2), ("ar1", 1), ("ar2", 2)])
def test_cli_json_equals_the_mirror(cli, name, d_budget):
    d, rows, wb = cli
    j = json.load(open(d / (name + ".json")))
    hb = j["haplotype"]
    assert len(hb["haplotypes"]) >= 3 and hb["damaged_reads"] >= 100 and hb["insufficient_coverage_reads"] >= 20     # nothing passes vacuously
    check_absorb_against_mirror(j, rows, wb, d_budget)


def test_cli_the_haplotypes_are_the_same_at_either_budget(cli):
    d, rows, wb = cli
    one, two = (json.load(open(d / (name + ".json")))["haplotype"] for name in ("a1", "a2"))
    assert len(one["absorb"]["insufficient"]["assigned_by_distance"]) == 2 and len(two["absorb"]["insufficient"]["assigned_by_distance"]) == 3
    for h1, h2 in zip(one["haplotypes"], two["haplotypes"]):
        assert h1["read_names"] == h2["read_names"] and h1["codons"] == h2["codons"]


def strip(j):
    j["input"].pop("timestamp")
    j["input"].pop("command_line")
    j["haplotype"].pop("absorb", None)
    for h in j["haplotype"]["haplotypes"]:
        for key in NEW_HAP_KEYS:
            h.pop(key, None)
    return j


def test_cli_without_the_new_keys_the_json_is_the_plain_run(cli):
    d, rows, wb = cli
    for flagged, base in (("a1", "plain"), ("a2", "plain"), ("ar1", "r"), ("ar2", "r")):
        with_flag, plain = json.load(open(d / (flagged + ".json"))), json.load(open(d / (base + ".json")))
        assert "absorb" in with_flag["haplotype"] and "absorb" not in plain["haplotype"]
        assert all(key in h for h in with_flag["haplotype"]["haplotypes"] for key in NEW_HAP_KEYS)
        assert not any(key in h for h in plain["haplotype"]["haplotypes"] for key in NEW_HAP_KEYS)
        assert strip(with_flag) == strip(plain)


def test_cli_each_block_is_what_it_would_be_alone(cli):
    """--rescue-damaged and --absorb-distance together: the `rescue` block and the rescued reads of every haplotype are those of
    --rescue-damaged alone, the `absorb` block and the absorbed reads those of --absorb-distance alone."""
    d, rows, wb = cli
    r = json.load(open(d / "r.json"))["haplotype"]
    assert r["rescue"]["assigned_reads"] > 0
    for both, alone in (("ar1", "a1"), ("ar2", "a2")):
        b, a = json.load(open(d / (both + ".json")))["haplotype"], json.load(open(d / (alone + ".json")))["haplotype"]
        assert b["rescue"] == r["rescue"] and b["absorb"] == a["absorb"] and "rescue" not in a
        for hb, ha, hr in zip(b["haplotypes"], a["haplotypes"], r["haplotypes"]):
            assert all(hb[key] == hr[key] for key in RESCUE_HAP_KEYS)
            assert all(hb[key] == ha[key] for key in NEW_HAP_KEYS)


TABLES = re.compile(r'\n<table id="hap-absorb".*?</table>\n<table id="hap-absorbed">.*?</table>\n', flags=re.S)
RUN_ROWS = re.compile(r"<tr><th>(timestamp|command_line)</th>.*?</tr>\n")


def test_cli_html_outside_the_two_tables_is_the_plain_run(cli):
    d, rows, wb = cli
    for flagged, base in (("a1", "plain"), ("ar2", "r")):
        html, plain = open(d / (flagged + ".html")).read(), open(d / (base + ".html")).read()
        assert len(TABLES.findall(html)) == 1 and "hap-absorb" not in plain
        assert RUN_ROWS.sub("", TABLES.sub("", html, count=1)) == RUN_ROWS.sub("", plain)
        assert len(RUN_ROWS.findall(plain)) == 2


def test_cli_html_tables_parse_back_to_the_json(cli):
    d, rows, wb = cli
    for name in ("a2", "ar1"):
        hb = json.load(open(d / (name + ".json")))["haplotype"]
        ab = hb["absorb"]
        html = TABLES.search(open(d / (name + ".html")).read()).group(0)
        head = re.search(r'<table id="hap-absorb" data-max-distance="(\d+)" data-min-positions="(\d+)">', html)
        assert (int(head.group(1)), int(head.group(2))) == (ab["max_distance"], ab["min_positions"])
        for key in CATEGORIES:
            m = re.search(r'<tr data-key="%s"><th>[^<]*</th><td>(\d+)</td><td>(\d+)</td></tr>' % key, html)
            assert (int(m.group(1)), int(m.group(2))) == (ab["insufficient"][key], ab["damaged"][key])
        by = re.findall(r'<tr data-key="assigned_by_distance" data-distance="(\d+)"><th>[^<]*</th><td>(\d+)</td><td>(\d+)</td></tr>', html)
        assert [int(x[0]) for x in by] == list(range(ab["max_distance"] + 1))
        assert [int(x[1]) for x in by] == ab["insufficient"]["assigned_by_distance"] and [int(x[2]) for x in by] == ab["damaged"]["assigned_by_distance"]
        per_hap = re.findall(r"<tr><td>([A-Z][a-z]?)</td><td>([^<]*)</td><td>(\d+)</td><td>(\d+)</td><td><details><summary>(\d+)</summary>(.*?)</details></td></tr>",
                             html.split('<table id="hap-absorbed">')[1], flags=re.S)
        assert len(per_hap) == len(hb["haplotypes"])
        for row, h in zip(per_hap, hb["haplotypes"]):
            assert row[0] == h["name"] and int(row[2]) == h["absorbed_reads"] and int(row[3]) == h["absorbed_damaged_reads"]
            assert int(row[4]) == len(h["absorbed_read_names"]) and re.findall(r'<span class="rn">([^<]*)</span>', row[5]) == h["absorbed_read_names"]
            assert abs(float(row[1].rstrip("%")) - 100.0 * h["frequency_with_absorbed"]) <= 0.051      # (printed to a tenth of a percent at least)


def test_cli_follows_the_taken_window_and_the_threshold(cli):
    d, rows, wb = cli
    r = juliet(d, "-c", "cfg.json", "--mode-phasing", "--downsample", "1000", "--absorb-distance", "1", "--absorb-min-positions", "3", "in.bam", "ds.json")
    assert r.returncode == 0, r.stderr
    j = json.load(open(d / "ds.json"))
    hb = j["haplotype"]
    assert j["target_config"]["n_reads"] == 1000 and len(hb["haplotypes"]) >= 2
    ab = hb["absorb"]
    assert ab["max_distance"] == 1 and ab["min_positions"] == 3
    pos_cols = np.array([p - wb - 1 for p in hb["variant_positions_abs"]], dtype=np.uint32)
    pattern = np.array([[16 * "ACGT".index(c[0]) + 4 * "ACGT".index(c[1]) + "ACGT".index(c[2]) for c in h["codons"]] for h in hb["haplotypes"]], dtype=np.uint8)
    near, dist, _, _ = nearest_mirror.nearest(rows, pos_cols, pattern, 3, 1)
    for key, total in (("insufficient", hb["insufficient_coverage_reads"]), ("damaged", hb["damaged_reads"])):
        assert sum(ab[key][c] for c in CATEGORIES) == total
    assert ab["insufficient"]["assigned_reads"] + ab["damaged"]["assigned_reads"] > 0
    for k, h in enumerate(hb["haplotypes"]):
        got = [index_of(name) for name in h["absorbed_read_names"]]
        assert got == sorted(got) and len(got) == h["absorbed_reads"] + h["absorbed_damaged_reads"]
        assert all(near[i] == k and dist[i] <= 1 for i in got)                   # the taken reads, judged as the mirror judges them
    # more informative positions asked for than the run has: no call is made, nobody can be judged
    r = juliet(d, "-c", "cfg.json", "--mode-phasing", "--absorb-distance", "2", "--absorb-min-positions", "4000", "in.bam", "k.json")
    assert r.returncode == 0, r.stderr
    hb = json.load(open(d / "k.json"))["haplotype"]
    zero = dict(assigned_reads=0, ambiguous_reads=0, distant_reads=0, assigned_by_distance=[0, 0, 0])
    assert hb["absorb"] == dict(max_distance=2, min_positions=4000, insufficient=dict(zero, uninformative_reads=hb["insufficient_coverage_reads"]),
                                damaged=dict(zero, uninformative_reads=hb["damaged_reads"]))
    assert all(h["absorbed_reads"] == 0 and h["absorbed_damaged_reads"] == 0 and h["absorbed_read_names"] == [] for h in hb["haplotypes"])
    assert sum(h["frequency_with_absorbed"] for h in hb["haplotypes"]) == pytest.approx(1.0, abs=1e-12)


def test_cli_no_reported_haplotype_is_the_zero_block(tmp_path):
    """Reads without a minor clone: nothing is called, nothing is phased, no call is made; the block has zeros and exit status 0."""
    subprocess.check_call([SYNTH, "--reads", "400", "--cols", "90", "--seed", "3", "--minor-permille", "0", "0", "0", "0",
                           "-o", str(tmp_path / "in.bam"), "--config-out", str(tmp_path / "cfg.json")])
    r = juliet(tmp_path, "-c", "cfg.json", "--mode-phasing", "--absorb-distance", "1", "in.bam", "out.json")
    assert r.returncode == 0, r.stderr
    hb = json.load(open(tmp_path / "out.json"))["haplotype"]
    assert hb["haplotypes"] == []
    zero = dict(assigned_reads=0, ambiguous_reads=0, distant_reads=0, assigned_by_distance=[0, 0])
    assert hb["absorb"] == dict(max_distance=1, min_positions=2, insufficient=dict(zero, uninformative_reads=hb["insufficient_coverage_reads"]),
                                damaged=dict(zero, uninformative_reads=hb["damaged_reads"]))
