"""jl_phase_recombinants_async on the device (docs/SPEC.md §23): which reads are one reported haplotype up to a breakpoint and
another from there on, and `juliet --mode-phasing --flag-recombinants` on top of it.  Every expectation is
tests/recombinant_mirror.py — the rule in plain loops — over the rows that were uploaded, compared for equality on every read;
never another device result."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import nearest_mirror
import recombinant_mirror as rm
import rescue_mirror
import second_turn as st
from minorseq_amd import capi, msa, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JULIET = os.path.join(ROOT, "minorseq_amd", "bin", "juliet")
SYNTH = os.path.join(ROOT, "minorseq_amd", "bin", "juliet-synth")

U, NONE, AMB, WHOLE = rm.UNINFORMATIVE, rm.NONE, rm.AMBIGUOUS, rm.WHOLE
KEYS = ("left", "right", "prefix", "suffix", "parent_reads", "tally")


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


# Pairs of haplotype numbers (base, copy): the copy equals the base but for ONE run of positions, so the two tie as a left parent in
# front of it and as a right parent behind it.  Numbers that differ in the low six bits only (lanes of one chunk, neighbours and
# across DPP rows), in bit 6 and above only (one lane, several chunks), and in both; the base at the lower and at the higher number.
FAMILIES = [(0, 1), (5, 4), (18, 47), (7, 71), (73, 9), (10, 97), (161, 34), (520, 8), (300, 690), (700, 701)]


def make_case(n, vp, n_hap, seed):
    """All haplotypes share one seeded backbone and differ at every codon's OWN column only, where they hold A, C or G — so the codon
    of haplotype h at position p is a function of its own-column base alone, a read with T there differs from every haplotype at that
    position, and `pattern[a][:b] + pattern[c][b:]` is a row of bases.  With three positions or fewer the haplotypes are AAA, CCC, GGG,
    ACG, ... in turn, distinct while they last (nine).  Reads, in turn: a | c at a seeded breakpoint; the same with a from a
    family and the breakpoint in front of the family's difference (the left parent ties) or c from a family and the breakpoint
    behind it (the right one ties); a haplotype itself; T at every own column; a | c | a2 (two breakpoints); a | c with scattered
    '-', N and uncovered cells; a | c with the codons around the breakpoint opened; a | c with ragged code-6 ends; code 6 throughout;
    seeded bases A .. T at the own columns.  Returns (rows, pos_cols, pattern)."""
    rng = np.random.default_rng(seed)
    pos_cols, n_cols = positions(vp)
    own = np.array([own_column(pos_cols, p) for p in range(vp)])
    backbone = rng.integers(0, 4, size=n_cols, dtype=np.uint8)
    if vp <= 3:
        words = np.array([[(h + (h // 3) * p) % 3 for p in range(vp)] for h in range(n_hap)], dtype=np.uint8)
    else:
        words = rng.integers(0, 3, size=(n_hap, vp), dtype=np.uint8)
    families = []
    if vp >= 3 and n_hap >= 3:
        for base, copy in FAMILIES:
            if base < n_hap and copy < n_hap:
                lo = int(rng.integers(1, vp - 1))
                hi = int(rng.integers(lo, vp - 1))                          # the copy differs at lo .. hi: 1 <= lo <= hi <= vp - 2
                words[copy] = words[base]
                words[copy, lo:hi + 1] = (words[base, lo:hi + 1] + 1) % 3
                families.append((base, copy, lo, hi))
    haps = np.repeat(backbone[None, :], n_hap, axis=0)
    haps[:, own] = words
    turns = ["rec", "left", "right", "whole", "far", "two", "scattered", "junction", "ragged", "out", "random"]
    rows = np.repeat(backbone[None, :], n, axis=0)
    for i in range(n):
        kind = turns[i % len(turns)]
        a, c = (int(x) for x in rng.integers(0, n_hap, size=2))
        b = int(rng.integers(1, vp)) if vp > 1 else 0
        if kind in ("left", "right") and families:
            base, copy, lo, hi = families[(i // len(turns)) % len(families)]
            member = int(base if rng.random() < 0.5 else copy)
            if kind == "left":
                a, b = member, int(rng.integers(1, lo + 1))
            else:
                c, b = member, int(rng.integers(hi + 1, vp))
        w = np.concatenate([words[a, :b], words[c, b:]])
        if kind == "whole":
            w = words[a].copy()
        elif kind == "far":
            w[:] = 3
        elif kind == "two" and vp >= 3:
            b2 = int(rng.integers(b, vp))
            w[b2:] = words[int(rng.integers(0, n_hap)), b2:]
        elif kind == "random":
            w = rng.integers(0, 4, size=vp, dtype=np.uint8)
        rows[i, own] = w
        if kind == "scattered":
            cell = rng.random(size=n_cols)
            rows[i, cell < 1.5 / n_cols] = 4
            rows[i, cell > 1.0 - 1.5 / n_cols] = 5
            rows[i, (cell > 0.5) & (cell < 0.5 + 1.0 / n_cols)] = 6
        elif kind == "junction":
            for p in range(max(0, b - int(rng.integers(0, 3))), min(vp, b + int(rng.integers(0, 3)))):
                rows[i, own[p]] = 4 + int(rng.integers(0, 3))
        elif kind == "ragged":
            lo, hi = int(rng.integers(0, n_cols // 3 + 1)), n_cols - int(rng.integers(0, n_cols // 3 + 1))
            rows[i, :lo] = 6
            rows[i, hi:] = 6
        elif kind == "out":
            rows[i] = 6
    return rows, pos_cols, codons_at(haps, pos_cols)


def outcomes(exp, n_hap):
    """Which of the six outcomes the mirror's answers hold: B both parents unique, L the left parent alone ambiguous, R the right one
    alone, W whole, N none, U uninformative."""
    left, right = exp["left"], exp["right"]
    held = ""
    held += "B" if ((left < n_hap) & (right < n_hap)).any() else ""
    held += "L" if ((left == AMB) & (right < n_hap)).any() else ""
    held += "R" if ((left < n_hap) & (right == AMB)).any() else ""
    held += "W" if (left == WHOLE).any() else ""
    held += "N" if (left == NONE).any() else ""
    held += "U" if (left == U).any() else ""
    return held


def check(j, rows, pos_cols, pattern, min_positions, expected=None):
    exp = expected or rm.recombinants(rows, pos_cols, pattern, min_positions)
    out = j.phase_recombinants(pos_cols, pattern, min_positions)
    for key in ("left", "right", "prefix", "suffix"):
        assert out[key].dtype == np.uint16 and out[key].shape == (len(rows),)
    assert out["parent_reads"].shape == (len(pattern), 2) and out["tally"].shape == (5,)
    for key in KEYS:
        assert (out[key] == exp[key]).all(), (key, np.flatnonzero(np.asarray(out[key] != exp[key]).reshape(len(out[key]), -1).any(axis=1))[:8])
    assert int(out["tally"].sum()) == len(rows)
    return out


# (reads, positions, haplotypes, min_positions or "vp", the outcomes the case is designed to hold): the word / run of 64 /
# two-workgroup edges of the reads, the dword of four and the tile of 64 positions, the chunk of 64 haplotypes (ids with bit 9 at
# 702), every value once and the corners together.  Not asked: a recombinant of one position (consequence (e)) or of one haplotype
# (its prefix and suffix cannot meet); an ambiguous side with two haplotypes (the third would be the other parent) or without a
# family (three positions at least); more than the one read's outcome of one read.
CASES = [
    (2049, 65, 129, 1, "BLRWNU"), (1, 64, 2, 1, ""), (31, 2, 2, 1, "BWNU"), (32, 3, 2, 2, "BWNU"), (33, 63, 63, "vp", "BLRWNU"),
    (63, 64, 64, 1, "BLRWNU"), (64, 65, 65, 2, "BLRWNU"), (65, 130, 702, 1, "BLRWNU"), (1023, 1, 1, 1, "WNU"), (1025, 130, 129, 2, "BLRWNU"),
    (2049, 3, 2, "vp", "BWNU"), (1023, 65, 702, 2, "BLRWNU"), (1025, 2, 1, 2, "WNU"), (64, 1, 64, 1, "WNU"), (33, 130, 702, "vp", "BLRWNU"),
    (1023, 63, 2, 1, "BWNU"), (65, 64, 1, 2, "WNU"),
]


@pytest.mark.parametrize("n,vp,n_hap,min_positions,held", CASES)
def test_recombinants_equal_mirror(ctx, n, vp, n_hap, min_positions, held):
    rows, pos_cols, pattern = make_case(n, vp, n_hap, 1000 * n + 7 * vp + n_hap)
    assert pos_cols[0] == 0 and pos_cols[-1] == rows.shape[1] - 3 and (vp < 2 or pos_cols[1] == 1)
    k = vp if min_positions == "vp" else min_positions
    exp = rm.recombinants(rows, pos_cols, pattern, k)
    got = outcomes(exp, n_hap)
    assert all(o in got for o in held), (held, got)                         # from the mirror: the case cannot pass empty
    ctx.upload_rows(rows, win_begin=3)
    check(ctx, rows, pos_cols, pattern, k, exp)
    assert (msa.unpack_columns(ctx.download_columns(), n) == rows).all()     # the matrix is untouched


# (positions, haplotypes): two chunks of haplotypes at few positions, two tiles of positions at few haplotypes
SECOND_TURN_SHAPES = [(5, 65), (65, 2)]


def second_turn_block(vp, n_hap):
    """The 2049-read case of this file's builder at the shape, cut to the block of st.BLOCK reads; (block, pos_cols, pattern)."""
    rows, pos_cols, pattern = make_case(2049, vp, n_hap, 1000 * 2049 + 7 * vp + n_hap)
    return rows[:st.BLOCK], pos_cols, pattern


def second_turn_expectation(block, pos_cols, pattern, n):
    """The dict of the n tiled reads from the mirror over the block and over the tail."""
    whole = rm.recombinants(block, pos_cols, pattern, 1)
    tail = rm.recombinants(block[:st.split(n)[1]], pos_cols, pattern, 1)
    exp = {key: st.tiled(whole[key], n) for key in ("left", "right", "prefix", "suffix")}
    exp.update({key: st.summed(whole[key], tail[key], n, st.BLOCK) for key in ("parent_reads", "tally")})
    return exp


@pytest.mark.parametrize("vp,n_hap", SECOND_TURN_SHAPES)
@pytest.mark.parametrize("n,what", st.COUNTS)
def test_a_workgroups_second_turn(n, what, vp, n_hap):
    """More than 4096 runs: a workgroup walks a second run — both walks' verdicts and `informative` start again, its parent counts and
    tallies are carried into one flush.  The rows are the block repeated (tests/second_turn.py)."""
    block, pos_cols, pattern = second_turn_block(vp, n_hap)
    exp = second_turn_expectation(block, pos_cols, pattern, n)
    assert int(exp["tally"].sum()) == n
    if n - st.ONE_TURN > 1:                                 # every outcome the shape can hold among the reads of the second turns
        late = {key: exp[key][st.second_turn_reads(n)] for key in ("left", "right")}
        assert all(o in outcomes(late, n_hap) for o in "BWNU"), outcomes(late, n_hap)
    j = capi.Juliet(0)
    try:
        st.adopt_tiled(j, block, n)
        out = j.phase_recombinants(pos_cols, pattern, 1)
        for key in KEYS:
            assert out[key].shape == exp[key].shape and (out[key] == exp[key]).all(), key
        assert int(out["tally"].sum()) == n
    finally:
        j.close()


def test_the_index_does_not_wrap_or_truncate(ctx):
    """4096 positions on 4098 columns, every codon overlapping its neighbours, 70 reads.  Haplotype A and three others that differ from
    it at the columns = 0, 1 and 2 (mod 3): every codon holds one such column, so A[:c] + B_r[c:] with c = r (mod 3) is A up to
    position c - 3 and B_r from c - 2 on — breakpoints at 1, 2047, 2048 and 4095, both ways round; a read that never disagrees; first
    mismatches at 0 and at 4095 from both ends.  An index kept in 12 bits would read 4096 as 0."""
    n, n_cols, vp = 70, 4098, 4096
    rng = np.random.default_rng(8)
    ha = rng.integers(0, 4, size=n_cols, dtype=np.uint8)
    haps = np.stack([ha] * 4)
    for r in range(3):
        haps[1 + r, r::3] = (ha[r::3] + 1) % 4
    pos_cols = np.arange(vp, dtype=np.uint32)
    pattern = codons_at(haps, pos_cols)
    rows = np.repeat(ha[None, :], n, axis=0)
    cuts = (3, 2049, 2050, 4097)
    for i, c in enumerate(cuts):
        rows[i] = np.concatenate([ha[:c], haps[1 + c % 3, c:]])
        rows[4 + i] = np.concatenate([haps[1 + c % 3, :c], ha[c:]])
    rows[9, 0] = (ha[0] + 2) % 4                              # a codon of nobody at position 0: first mismatch at 0, and at 4095 from the end
    rows[10, n_cols - 1] = (ha[n_cols - 1] + 2) % 4           # ... at position 4095: at 4095, and at 0 from the end
    rows[11:] = haps[rng.integers(0, 4, size=n - 11)]
    rows[13] = 6
    cell = rng.random(size=rows.shape)
    cell[:11] = 1.0
    rows[cell < 1e-4] = 4
    exp = rm.recombinants(rows, pos_cols, pattern, 1)
    assert exp["prefix"][:4].tolist() == [1, 2047, 2048, 4095] == (vp - exp["suffix"][:4].astype(np.int64)).tolist() == exp["prefix"][4:8].tolist()
    assert exp["left"][:8].tolist() == [0, 0, 0, 0, 1, 1, 2, 3] and exp["right"][:8].tolist() == [1, 1, 2, 3, 0, 0, 0, 0]
    assert (exp["left"][8], exp["prefix"][8], exp["suffix"][8]) == (WHOLE, 4096, 4096)
    assert (exp["prefix"][9], exp["suffix"][9], exp["prefix"][10], exp["suffix"][10]) == (0, 4095, 4095, 0)
    assert exp["left"][9] == exp["left"][10] == NONE and exp["left"][13] == U
    ctx.upload_rows(rows)
    check(ctx, rows, pos_cols, pattern, 1, exp)
    check(ctx, rows, pos_cols, pattern, 4000)


def test_order_matters(ctx):
    """Two haplotypes that differ at every one of 9 positions.  A read taking A at the even and B at the odd positions is four codons
    from A for the nearest call and explained by no breakpoint here; A[:4] + B[4:] is the recombinant (A, B); swapping the rows
    swaps the parents."""
    vp = 9
    pos_cols, n_cols = positions(vp)
    own = np.array([own_column(pos_cols, p) for p in range(vp)])
    haps = np.zeros((2, n_cols), dtype=np.uint8)
    haps[1, own] = 1
    rows = np.zeros((2, n_cols), dtype=np.uint8)
    rows[0, own[1::2]] = 1
    rows[1, own[4:]] = 1
    pattern = codons_at(haps, pos_cols)
    ctx.upload_rows(rows)
    out = check(ctx, rows, pos_cols, pattern, 1)
    assert (out["left"][0], out["right"][0]) == (NONE, NONE)
    near = ctx.phase_nearest(pos_cols, pattern, 1, 7)
    assert near["nearest"][0] == 0 and near["dist"][0] == 4 == nearest_mirror.nearest(rows, pos_cols, pattern, 1, 7)[1][0]
    assert (out["left"][1], out["right"][1], out["prefix"][1], out["suffix"][1]) == (0, 1, 4, 5)
    swapped = check(ctx, rows, pos_cols, pattern[::-1].copy(), 1)
    assert (swapped["left"][1], swapped["right"][1], swapped["prefix"][1], swapped["suffix"][1]) == (1, 0, 4, 5)
    assert swapped["parent_reads"].tolist() == [[0, 1], [1, 0]] and out["parent_reads"].tolist() == [[1, 0], [0, 1]]


def test_equal_rows_tie_and_open_junctions_widen(ctx):
    vp = 7
    pos_cols, n_cols = positions(vp)
    own = np.array([own_column(pos_cols, p) for p in range(vp)])
    haps = np.zeros((4, n_cols), dtype=np.uint8)
    haps[1, own] = 1
    haps[2], haps[3] = haps[0], haps[1]                     # rows 0 = 2 and 1 = 3
    rows = np.zeros((4, n_cols), dtype=np.uint8)
    rows[:, own[3:]] = 1                                    # A[:3] + B[3:]
    rows[1, own[3]] = 4                                     # position 3 open: breakpoints 3 and 4
    rows[2, own[2]], rows[2, own[3]] = 5, 6                 # 2 and 3 open: 2, 3, 4
    rows[3, own[:3]] = 6                                    # everything in front of the breakpoint open: B agrees throughout
    pattern = codons_at(haps, pos_cols)
    ctx.upload_rows(rows)
    out = check(ctx, rows, pos_cols, pattern, 1)
    assert out["left"].tolist() == [AMB, AMB, AMB, WHOLE] and out["right"].tolist() == [AMB, AMB, AMB, WHOLE]
    assert (vp - out["suffix"]).tolist() == [3, 3, 2, 0] and out["prefix"].tolist() == [3, 4, 4, 7]
    assert out["tally"].tolist() == [0, 3, 1, 0, 0] and not out["parent_reads"].any()
    out = check(ctx, rows, pos_cols, pattern[:2].copy(), 1)           # without the copies both parents are unique
    assert out["left"].tolist() == [0, 0, 0, WHOLE] and out["right"].tolist() == [1, 1, 1, WHOLE]
    assert out["parent_reads"].tolist() == [[3, 0], [0, 3]]


def fetch_copy(j):
    out = j.run_fetch(True, True, cap_var=64)
    return dict(variants=out["variants"].copy(), phase={k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in out["phase"].items()})


def assert_same_run(a, b):
    assert (a["variants"] == b["variants"]).all()
    pa, pb = a["phase"], b["phase"]
    assert pa["summary"] == pb["summary"]
    for key in ("pos_cols", "hap_count", "hap_pattern", "hit", "read_hap", "cooc"):
        assert (pa[key] == pb[key]).all(), key


def test_consequences_after_a_real_run(ctx):
    """A run with phasing over reads with a raised substitution rate, deletions, masked bases and partial reads; then the rule with the
    run's own positions and haplotypes over all reads: consequences (a), (b) and (d) of §23 hold, the run's results and the matrix
    are what they were.  Consequence (e) on the same upload: one position never yields a recombinant."""
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
    assert n_hap >= 2 and vp >= 2
    for k in (1, 2, vp):
        out = check(ctx, rows, pos_cols, pattern, k)
        res = rescue_mirror.rescue(rows, pos_cols, pattern, k)[0]
        assert ((out["left"] == WHOLE) == ((res < n_hap) | (res == AMB))).all() and ((out["left"] == U) == (res == U)).all()      # (a)
        assert ((out["prefix"] == vp) == (out["suffix"] == vp)).all()                                                            # (b)
        assert (out["left"][read_hap < n_hap] == WHOLE).all() and (read_hap < n_hap).sum() > 0                                   # (d)
    one = check(ctx, rows, pos_cols[:1], pattern[:, :1].copy(), 1)                                                               # (e)
    assert one["tally"][0] == one["tally"][1] == 0 and one["tally"][2] > 0 and one["tally"][3] > 0
    assert_same_run(first, fetch_copy(ctx))
    assert (msa.unpack_columns(ctx.download_columns(), n) == rows).all()
    ctx.run_async(genes, ref, capi.default_params(), None, True, 10, True)
    assert_same_run(first, fetch_copy(ctx))


def test_adopted_matrix_with_its_own_stride():
    """A torch tensor as the matrix: 2049 reads in planes of 272 bytes (the library's own stride is 384), garbage in the bytes
    past ceil(n / 8) of every plane row.  None of it may show in any read's answer or in a count."""
    import torch
    n, vp, n_hap, stride = 2049, 65, 129, 272
    assert stride != msa.plane_stride(n) and stride % 16 == 0
    rows, pos_cols, pattern = make_case(n, vp, n_hap, 99)
    planes = msa.pack_planes(rows, stride)
    planes[:, :, (n + 7) // 8:] = np.random.default_rng(1).integers(0, 256, size=(rows.shape[1], 3, stride - (n + 7) // 8), dtype=np.uint8)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t = torch.from_numpy(planes).cuda(non_blocking=False)
    stream.synchronize()
    j = capi.Juliet(0, stream=stream.cuda_stream)
    j.adopt(t.data_ptr(), n, rows.shape[1], stride, keep_alive=t)
    out = check(j, rows, pos_cols, pattern, 1)
    assert (out["tally"] > 0).all()
    check(j, rows, pos_cols[:3], pattern[:2, :3].copy(), 3)
    j.close()


def test_repeat_calls_and_staging_that_grows(ctx):
    """(130, 702), then (2, 2), then (65, 129) on one matrix: no stale pattern, position, id, length or count shows.  Then a call
    that only enqueues, its inputs overwritten at once: they were copied before it returned.  Then a larger matrix and a smaller
    one again: the buffers grow and are reused."""
    rows, pos_cols, pattern = make_case(1025, 130, 702, 12)
    ctx.upload_rows(rows)
    check(ctx, rows, pos_cols, pattern, 1)
    check(ctx, rows, pos_cols[:2], pattern[:2, :2].copy(), 2)
    check(ctx, rows, pos_cols[:65], pattern[:129, :65].copy(), 1)
    cols, pat = pos_cols[:64].copy(), pattern[:65, :64].copy()
    exp = rm.recombinants(rows, cols, pat, 2)
    assert ctx.phase_recombinants(cols, pat, 2, wait=False) is None
    cols[:] = 0
    pat[:] = 63
    out = ctx.phase_recombinants_fetch()
    for key in KEYS:
        assert (out[key] == exp[key]).all(), key
    for seed, (n, vp, n_hap) in enumerate(((1500, 3, 9), (5000, 40, 70), (1500, 3, 9))):
        rows, pos_cols, pattern = make_case(n, vp, n_hap, 70 + seed)
        ctx.upload_rows(rows)
        out = check(ctx, rows, pos_cols, pattern, 1 if vp == 3 else 2)
        assert out["tally"][0] > 0


def test_refusals_change_nothing():
    lib = capi.load_library()
    j = capi.Juliet(0)
    rows, pos_cols, pattern = make_case(40, 3, 4, 1)           # 8 columns: codons at 0, 1, 4
    n_cols = rows.shape[1]

    def refused(status, word, cols=pos_cols, n_pos=3, pat=pattern, stride=3, n_hap=4, min_positions=1):
        rc = lib.jl_phase_recombinants_async(j.h, None if cols is None else cols.ctypes.data, n_pos, None if pat is None else pat.ctypes.data,
                                             stride, n_hap, min_positions)
        assert rc == status
        assert word in lib.jl_last_error(j.h).decode(), lib.jl_last_error(j.h)

    refused(-4, "no resident matrix")
    j.upload_rows(rows)
    res = np.zeros(40, dtype=np.uint16)
    assert lib.jl_phase_recombinants_fetch(j.h, res.ctypes.data, None, None, None, None, None) == -4     # a fetch before any call
    assert "before jl_phase_recombinants_async" in lib.jl_last_error(j.h).decode()
    good = j.phase_recombinants(pos_cols, pattern, 2)
    exp = rm.recombinants(rows, pos_cols, pattern, 2)
    assert all((good[key] == exp[key]).all() for key in KEYS)
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
    refused(-1, "ends beyond the window", cols=np.array([0, 1, n_cols - 2], dtype=np.uint32))
    refused(-1, "not strictly ascending", cols=np.array([0, 4, 4], dtype=np.uint32))
    refused(-1, "not strictly ascending", cols=np.array([1, 0, 4], dtype=np.uint32))
    bad = pattern.copy()
    bad[3, 2] = 64
    refused(-1, "is no codon", pat=bad)
    again = j.phase_recombinants_fetch()                                              # what was enqueued before is still there
    for key in KEYS:
        assert (again[key] == good[key]).all(), key
    # any pointer of the fetch may be NULL
    tally = np.zeros(5, dtype=np.uint64)
    suffix = np.zeros(40, dtype=np.uint16)
    assert lib.jl_phase_recombinants_fetch(j.h, None, None, None, None, None, tally.ctypes.data) == 0 and (tally == exp["tally"]).all()
    assert lib.jl_phase_recombinants_fetch(j.h, None, None, None, suffix.ctypes.data, None, None) == 0 and (suffix == exp["suffix"]).all()
    assert lib.jl_phase_recombinants_fetch(j.h, None, None, None, None, None, None) == 0
    assert (msa.unpack_columns(j.download_columns(), 40) == rows).all()
    j.close()


def test_the_three_calls_keep_their_own_results(ctx):
    """Rescue, nearest and recombinant results each survive the other two calls."""
    rows, pos_cols, pattern = make_case(1025, 17, 65, 5)
    ctx.upload_rows(rows)
    res = ctx.phase_rescue(pos_cols, pattern, 1)
    near = ctx.phase_nearest(pos_cols[:5], pattern[:9, :5].copy(), 2, 3)
    rec = check(ctx, rows, pos_cols[:9], pattern[:33, :9].copy(), 2)
    again_res, again_near = ctx.phase_rescue_fetch(), ctx.phase_nearest_fetch()
    assert all((again_res[key] == res[key]).all() for key in res) and all((again_near[key] == near[key]).all() for key in near)
    exp = rescue_mirror.rescue(rows, pos_cols, pattern, 1)
    assert (again_res["rescue"] == exp[0]).all() and (again_res["hap_reads"] == exp[1]).all() and (again_res["tally"] == exp[2]).all()
    exp = nearest_mirror.nearest(rows, pos_cols[:5], pattern[:9, :5], 2, 3)
    assert (again_near["nearest"] == exp[0]).all() and (again_near["dist"] == exp[1]).all()
    ctx.phase_rescue(pos_cols[:4], pattern[:3, :4].copy(), 1)
    ctx.phase_nearest(pos_cols[:3], pattern[:7, :3].copy(), 1, 1)
    after = ctx.phase_recombinants_fetch()
    assert all((after[key] == rec[key]).all() for key in KEYS)


# ---------------------------------------------------------------------------------------------- the command line
N_CLI, L_CLI = 600, 60
VAR_CODONS = (2, 6, 10, 14, 18)          # the five codons at which clone B differs from clone A (= the reference)
CATEGORIES = ("recombinant_reads", "ambiguous_parent_reads", "whole_reads", "unexplained_reads", "uninformative_reads")
NEW_HAP_KEYS = ("putative_recombinant", "recombinant_of")


def to_bam(tmp, rows, ref, name):
    mpath, bam, cfg = (str(tmp / f"{name}.{x}") for x in ("msa", "bam", "json"))
    with open(mpath, "wb") as f:
        f.write(np.array([rows.shape[0], rows.shape[1], 0], dtype=np.uint64).tobytes())
        f.write(np.ascontiguousarray(rows, dtype=np.uint8).tobytes())
    refs = "".join("ACGT"[b] for b in ref)
    subprocess.check_call([SYNTH, "--from-rows", mpath, "--ref", refs, "-o", bam])
    json.dump({"genes": [dict(name="G", begin=1, end=len(ref) + 1, drms=[])], "referenceName": "printed", "referenceSequence": refs,
               "version": "tests/test_gpu_recombinant.py", "databaseVersion": "none"}, open(cfg, "w"))


def juliet(d, *args):
    return subprocess.run([JULIET, *args], cwd=d, capture_output=True, text=True, timeout=120)


def cli_rows():
    """Clones A (the reference) and B at 45 % each; A | B in front of position 2 at 6 %, which phasing reports as a haplotype; B | A
    in front of position 3 at 1 %, which stays insufficient; damaged recombinants — B | A with the last codon, or the codon at the
    junction, deleted, and A | B with the first one filtered; A with a codon of its own at position 2 (explained by no breakpoint);
    reads uncovered from column 6 on."""
    rng = np.random.default_rng(23)
    ref = rng.integers(0, 4, size=L_CLI, dtype=np.uint8)
    a, b = ref.copy(), ref.copy()
    for c in VAR_CODONS:
        b[3 * c + 1] = (ref[3 * c + 1] + 1) % 4
    cut = lambda x, y, p: np.concatenate([x[:3 * VAR_CODONS[p]], y[3 * VAR_CODONS[p]:]])      # noqa: E731
    ab, ba = cut(a, b, 2), cut(b, a, 3)
    rows = np.concatenate([np.repeat(a[None], 270, 0), np.repeat(b[None], 270, 0), np.repeat(ab[None], 36, 0), np.repeat(ba[None], 6, 0),
                           np.repeat(ba[None], 6, 0), np.repeat(ab[None], 3, 0), np.repeat(a[None], 6, 0), np.repeat(a[None], 3, 0)])
    assert len(rows) == N_CLI
    col = lambda p: 3 * VAR_CODONS[p]      # noqa: E731
    rows[582:585, col(4):col(4) + 3] = 4
    rows[585:588, col(3):col(3) + 3] = 4
    rows[588:591, col(0) + 1] = 5
    for i in range(591, 597):
        rows[i, col(2) + 2] = (ref[col(2) + 2] + 1 + (i % 3)) % 4
        rows[i, col(2)] = (ref[col(2)] + 1 + (i // 3) % 2) % 4
    rows[597:600, 6:] = 6
    return rows[rng.permutation(N_CLI)], ref


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    d = tmp_path_factory.mktemp("recombinant_cli")
    rows, ref = cli_rows()
    to_bam(d, rows, ref, "in")
    for name, flags in (("f", ["--flag-recombinants", "--timing"]), ("fa", ["--flag-recombinants", "--rescue-damaged", "--absorb-distance", "1"]),
                        ("a", ["--rescue-damaged", "--absorb-distance", "1"]), ("plain", []),
                        ("k", ["--flag-recombinants", "--recombinant-min-positions", "4000", "--recombinant-parent-ratio", "50"])):
        r = juliet(d, "-c", "in.json", "--mode-phasing", *flags, "in.bam", name + ".json", name + ".html")
        assert r.returncode == 0, r.stderr
        if "--timing" in flags:
            assert re.search(r"timing recombinants\b", r.stderr), r.stderr             # the stage line of --timing
    return d, rows


def index_of(name):
    return int(name.split("/")[1])


def categories_of_json(j, rows):
    """From the JSON's own positions, codons and read names: (pos_cols, pattern, insufficient per read, damaged per read)."""
    hb = j["haplotype"]
    pos_cols = np.array([p - 1 for p in hb["variant_positions_abs"]], dtype=np.uint32)
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


def expected_block(j, rows, min_positions, ratio):
    hb = j["haplotype"]
    names = [h["name"] for h in hb["haplotypes"]]
    pos_cols, pattern, insufficient, damaged = categories_of_json(j, rows)
    vp, n_hap = len(pos_cols), len(names)
    exp = rm.recombinants(rows, pos_cols, pattern, min_positions)
    left, right = exp["left"].astype(np.int64), exp["right"].astype(np.int64)
    both = (left < n_hap) & (right < n_hap)
    block = dict(min_positions=min_positions, parent_ratio=ratio)
    for key, kind in (("insufficient", insufficient), ("damaged", damaged)):
        block[key] = dict(recombinant_reads=int((kind & both).sum()), ambiguous_parent_reads=int((kind & ~both & ((left < n_hap) | (left == AMB))).sum()),
                          whole_reads=int((kind & (left == WHOLE)).sum()), unexplained_reads=int((kind & (left == NONE)).sum()),
                          uninformative_reads=int((kind & (left == U)).sum()))
    pairs = []
    for lft, rgt in sorted({(int(x), int(y)) for x, y in zip(left[both], right[both])}):
        of = both & (left == lft) & (right == rgt) & (insufficient | damaged)
        pairs.append(dict(left=names[lft], right=names[rgt], reads=int(of.sum()), insufficient_reads=int((of & insufficient).sum()),
                          damaged_reads=int((of & damaged).sum()), breakpoint_min=int((vp - exp["suffix"][of].astype(np.int64)).min()),
                          breakpoint_max=int(exp["prefix"][of].max())))
    pairs.sort(key=lambda p: (-p["reads"], names.index(p["left"]), names.index(p["right"])))
    block["pairs"] = pairs
    haps = rm.haplotype_recombinants(pattern.tolist(), [h["reads"] for h in hb["haplotypes"]], ratio)
    return block, haps, names


def test_cli_json_equals_the_mirror(cli):
    d, rows = cli
    for name in ("f", "fa"):
        j = json.load(open(d / (name + ".json")))
        hb = j["haplotype"]
        block, haps, names = expected_block(j, rows, 2, 2.0)
        assert hb["recombinants"] == block
        for kind, total in (("insufficient", hb["insufficient_coverage_reads"]), ("damaged", hb["damaged_reads"])):
            assert sum(block[kind][c] for c in CATEGORIES) == total
        assert block["insufficient"]["recombinant_reads"] >= 6 and block["damaged"]["recombinant_reads"] >= 6       # nothing passes vacuously
        assert block["insufficient"]["unexplained_reads"] >= 1 and block["damaged"]["uninformative_reads"] >= 1 and block["damaged"]["whole_reads"] >= 1
        assert sorted(h["reads"] for h in hb["haplotypes"]) == [36, 270, 270]
        chimera = next(h for h in hb["haplotypes"] if h["reads"] == 36)
        a_name = next(h["name"] for h in hb["haplotypes"] if h["reads"] == 270 and h["codons"][0] == chimera["codons"][0])
        b_name = next(h["name"] for h in hb["haplotypes"] if h["reads"] == 270 and h["name"] != a_name)
        assert chimera["putative_recombinant"] is True and chimera["recombinant_of"] == dict(left=a_name, right=b_name, prefix=2, suffix=3)
        assert block["pairs"][0]["left"] == b_name and block["pairs"][0]["right"] == a_name and block["pairs"][0]["reads"] == 12
        assert (block["pairs"][0]["breakpoint_min"], block["pairs"][0]["breakpoint_max"]) == (3, 4)
        for h, e in zip(hb["haplotypes"], haps):
            assert h["putative_recombinant"] is e["flagged"]
            assert ("recombinant_of" in h) == e["flagged"]
            if e["flagged"]:
                assert h["recombinant_of"] == dict(left=names[e["left"]], right=names[e["right"]], prefix=e["prefix"], suffix=e["suffix"])
            elif h["reads"] == 270:
                assert h["putative_recombinant"] is False                    # the clones are none


def strip(j):
    j["input"].pop("timestamp")
    j["input"].pop("command_line")
    j["haplotype"].pop("recombinants", None)
    for h in j["haplotype"]["haplotypes"]:
        for key in NEW_HAP_KEYS:
            h.pop(key, None)
    return j


def test_cli_without_the_new_keys_the_json_is_the_plain_run(cli):
    d, rows = cli
    for flagged, base in (("f", "plain"), ("fa", "a"), ("k", "plain")):
        with_flag, plain = json.load(open(d / (flagged + ".json"))), json.load(open(d / (base + ".json")))
        assert "recombinants" in with_flag["haplotype"] and "recombinants" not in plain["haplotype"]
        assert all("putative_recombinant" in h for h in with_flag["haplotype"]["haplotypes"])
        assert not any(key in h for h in plain["haplotype"]["haplotypes"] for key in NEW_HAP_KEYS)
        assert strip(with_flag) == strip(plain)


TABLES = re.compile(r'\n<table id="hap-recombinants".*?</table>\n<table id="hap-recombinant-pairs">.*?</table>\n<table id="hap-putative-recombinants">.*?</table>\n',
                    flags=re.S)
RUN_ROWS = re.compile(r"<tr><th>(timestamp|command_line)</th>.*?</tr>\n")


def test_cli_html_tables_parse_back_to_the_json(cli):
    d, rows = cli
    for name, base in (("f", "plain"), ("fa", "a")):
        hb = json.load(open(d / (name + ".json")))["haplotype"]
        rc = hb["recombinants"]
        page, plain = open(d / (name + ".html")).read(), open(d / (base + ".html")).read()
        assert len(TABLES.findall(page)) == 1 and "hap-recombinants" not in plain
        assert RUN_ROWS.sub("", TABLES.sub("", page, count=1)) == RUN_ROWS.sub("", plain)          # outside the tables: the page it was
        html = TABLES.search(page).group(0)
        head = re.search(r'<table id="hap-recombinants" data-min-positions="(\d+)" data-parent-ratio="([^"]+)">', html)
        assert (int(head.group(1)), float(head.group(2))) == (rc["min_positions"], rc["parent_ratio"])
        for key in CATEGORIES:
            m = re.search(r'<tr data-key="%s"><th>[^<]*</th><td>(\d+)</td><td>(\d+)</td></tr>' % key, html)
            assert (int(m.group(1)), int(m.group(2))) == (rc["insufficient"][key], rc["damaged"][key])
        pairs = re.findall(r"<tr><td>([A-Z][a-z]?)</td><td>([A-Z][a-z]?)</td><td>(\d+)</td><td>(\d+)</td><td>(\d+)</td><td>(\d+)</td><td>(\d+)</td></tr>",
                           html.split('<table id="hap-recombinant-pairs">')[1].split("</table>")[0])
        assert [dict(left=p[0], right=p[1], reads=int(p[2]), insufficient_reads=int(p[3]), damaged_reads=int(p[4]), breakpoint_min=int(p[5]),
                     breakpoint_max=int(p[6])) for p in pairs] == rc["pairs"] and pairs
        per_hap = re.findall(r"<tr><td>([A-Z][a-z]?)</td><td>(yes|no)</td><td>([^<]*)</td><td>([^<]*)</td><td>(\d*)</td><td>(\d*)</td></tr>",
                             html.split('<table id="hap-putative-recombinants">')[1])
        assert len(per_hap) == len(hb["haplotypes"])
        for row, h in zip(per_hap, hb["haplotypes"]):
            assert row[0] == h["name"] and (row[1] == "yes") is h["putative_recombinant"]
            if h["putative_recombinant"]:
                assert dict(left=row[2], right=row[3], prefix=int(row[4]), suffix=int(row[5])) == h["recombinant_of"]
            else:
                assert row[2:] == ("", "", "", "")


def test_cli_follows_the_taken_window_and_the_zero_blocks(cli, tmp_path):
    d, rows = cli
    r = juliet(d, "-c", "in.json", "--mode-phasing", "--downsample", "300", "--flag-recombinants", "--recombinant-min-positions", "3", "in.bam", "ds.json")
    assert r.returncode == 0, r.stderr
    j = json.load(open(d / "ds.json"))
    hb = j["haplotype"]
    rc = hb["recombinants"]
    assert j["target_config"]["n_reads"] == 300 and len(hb["haplotypes"]) >= 2 and rc["min_positions"] == 3 and rc["parent_ratio"] == 2.0
    for kind, total in (("insufficient", hb["insufficient_coverage_reads"]), ("damaged", hb["damaged_reads"])):
        assert sum(rc[kind][c] for c in CATEGORIES) == total                     # the taken reads, no others
    assert sum(p["reads"] for p in rc["pairs"]) == rc["insufficient"]["recombinant_reads"] + rc["damaged"]["recombinant_reads"]
    assert all(p["reads"] == p["insufficient_reads"] + p["damaged_reads"] for p in rc["pairs"])
    # more informative positions asked for than the run has: no device call is made, nobody can be judged; the haplotype level stands
    hb = json.load(open(d / "k.json"))["haplotype"]
    zero = dict(recombinant_reads=0, ambiguous_parent_reads=0, whole_reads=0, unexplained_reads=0)
    assert hb["recombinants"] == dict(min_positions=4000, parent_ratio=50.0, insufficient=dict(zero, uninformative_reads=hb["insufficient_coverage_reads"]),
                                      damaged=dict(zero, uninformative_reads=hb["damaged_reads"]), pairs=[])
    assert all(h["putative_recombinant"] is False and "recombinant_of" not in h for h in hb["haplotypes"])      # nobody has 50 times the reads
    # reads without a minor clone: nothing is called, nothing is phased, no call is made; the block has zeros and exit status 0
    subprocess.check_call([SYNTH, "--reads", "400", "--cols", "90", "--seed", "3", "--minor-permille", "0", "0", "0", "0",
                           "-o", str(tmp_path / "in.bam"), "--config-out", str(tmp_path / "cfg.json")])
    r = juliet(tmp_path, "-c", "cfg.json", "--mode-phasing", "--flag-recombinants", "in.bam", "out.json")
    assert r.returncode == 0, r.stderr
    hb = json.load(open(tmp_path / "out.json"))["haplotype"]
    assert hb["haplotypes"] == []
    assert hb["recombinants"] == dict(min_positions=2, parent_ratio=2.0, insufficient=dict(zero, uninformative_reads=hb["insufficient_coverage_reads"]),
                                      damaged=dict(zero, uninformative_reads=hb["damaged_reads"]), pairs=[])
