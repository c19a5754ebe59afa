"""The in-frame insertion alleles of a record build on the device (docs/SPEC.md §17): jl_msa_track_insertion_alleles,
jl_insertion_alleles_fetch, and `juliet --call-insertions` on top of them.  Every expectation is tests/insertion_mirror.py — the
rule as plain loops over the record arrays, the test in exact arithmetic — compared for equality on every entry; never another
device result."""
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import bam_py
import insertion_mirror as im
import records_expand
from minorseq_amd import capi, msa, synth
from test_insertion_host import HAND_ALLELES, HAND_FRAMESHIFT, HAND_READS, HAND_UNREAD

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JULIET = os.path.join(ROOT, "minorseq_amd", "bin", "juliet")
SYNTH = os.path.join(ROOT, "minorseq_amd", "bin", "juliet-synth")
WB = 7          # win_begin of the generated cases: reads begin up to three bases before the window


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
    j.track_insertion_alleles()
    yield j
    j.close()


# ---------------------------------------------------------------------------------------------- generated reads
POOL = ["AAA", "AAAAAA", "ACG", "ACT", "CCGTTA", "GATTACAGA", "T" * 29 + "G", "ACGT" * 7 + "AC", "ACGT" * 7 + "AG"]   # the alleles that repeat


def insertion(rng, k):
    """Kind k of 16 -> (ops, bases, index of a base to give a low quality or None).  Total lengths 1, 2, 3, 4, 29, 30, 31, 33 occur,
    two 'I' ops at one junction with a 'P', an empty op, an 'S' or nothing between them, a base that is no A C G T."""
    rnd = lambda n: "".join("ACGT"[b] for b in rng.integers(0, 4, size=n))     # noqa: E731
    if k == 0:
        return [("I", 1)], rnd(1), None
    if k == 1:
        return [("I", 2)], rnd(2), None
    if k == 2:
        return [("I", 4)], rnd(4), None
    if k == 3:
        return [("I", 29)], rnd(29), None
    if k == 4:
        return [("I", 31)], rnd(31), None
    if k == 5:
        return [("I", 33)], rnd(33), None                    # in frame, too long
    if k == 6:
        return [("I", 1), ("P", 1), ("I", 2)], "ACG", None   # two ops summing to in-frame: the allele ACG
    if k == 7:
        return [("I", 2), ("I", 2)], rnd(4), None            # ... to out-of-frame
    if k == 8:
        return [("I", 3), ("D", 0), ("I", 3)], "CCGTTA", None
    if k == 9:
        return [("I", 3)], "ANG" if rng.integers(0, 2) else "RCG", None          # a base that is not exactly A C G T
    if k == 10:
        s = POOL[int(rng.integers(0, len(POOL)))]
        return [("I", len(s))], s, int(rng.integers(0, len(s)))                  # one low quality among the inserted bases
    if k == 11:
        return [("I", 3), ("S", 2), ("I", 3)], "CCG" + "TT" + "TTA", None        # the clipped bases are not the insertion's
    if k == 12:
        return [("I", 6)], rnd(6), None
    s = POOL[int(rng.integers(0, len(POOL)))]
    return [("I", len(s))], s, None


def one_read(rng, n_cols, events=None):
    """A read over window columns [s, e), s in -3 .. 1 and e within three of the window's end, cut at up to four junctions into runs
    of '=' mostly, some 'X', 'D' (an insertion beside it still spans) and 'N' (beside it: counts nowhere); an insertion at every
    cut — at c = 0, n_cols - 1, n_cols and beyond when the cut falls there — and now and then one in front of the first and behind
    the last reference op, next to a clip.  `events`: [(junction, kind)] instead of the random cuts, between '=' runs."""
    s = int(rng.integers(-3, 2))
    e = int(rng.integers(max(s + 2, n_cols - 2), n_cols + 4))
    if events is None:
        cand = np.arange(s + 1, e)
        cuts = sorted(rng.choice(cand, size=min(len(cand), int(rng.integers(0, 5))), replace=False).tolist())
        events = [(c, int(rng.integers(0, 16))) for c in cuts]
        plain = False
    else:
        s, e, plain = min(s, 0), max(e, n_cols), True
    ops, bases, quals = [], "", []

    def add(op, ln, text=None, low=None):
        nonlocal bases
        ops.append((op, ln))
        if op in "IS=X":
            text = text if text is not None else "".join("ACGT"[b] for b in rng.integers(0, 4, size=ln))
            bases += text
            quals.extend(5 if low is not None and j == low else 40 for j in range(ln))

    if not plain and rng.random() < 0.2:
        add("S", 2)
    if not plain and rng.random() < 0.2:
        add("I", 3)                                          # before the first reference op: spans nothing
    at = s
    for c, k in list(events) + [(e, None)]:
        kind = "=" if plain or not events else "==X=D=N="[int(rng.integers(0, 8))]
        add(kind, c - at)
        at = c
        if k is None:
            break
        iops, text, low = insertion(rng, k)
        used = 0
        for op, ln in iops:
            if op in "IS":
                piece = text[used:used + ln]
                add(op, ln, piece, None if low is None else low - used)
                used += ln
            else:
                add(op, ln)
    if not plain and rng.random() < 0.2:
        add("I", 3)                                          # behind the last one
    if not plain and rng.random() < 0.1:
        add("H", 4)
    return (WB + s, ops, bases, quals)


def make_reads(n, n_cols, seed):
    """n generated reads.  The first ones are anchors, so that the smallest case holds all three classes and two alleles: the
    alleles AAA and ACG, a two-base and a 33-base insertion at junctions 1 .. 4 of read 0, or — when the window has fewer than five
    columns — at junction 1 of reads 0 .. 3."""
    rng = np.random.default_rng(seed)
    anchor = [13, 6, 1, 5]

    def fixed(c, k):
        rd = None
        while rd is None or (k == 13 and "AAA" not in rd[2]):
            rd = one_read(rng, n_cols, [(c, k)] if not isinstance(c, list) else [(cc, kk) for cc, kk in zip(c, k)])
        return rd
    if n_cols >= 5:
        reads = [fixed([1, 2, 3, 4], anchor)]
    else:
        assert n >= 4
        reads = [fixed(1, k) for k in anchor]
    while len(reads) < n:
        reads.append(one_read(rng, n_cols))
    return reads[:n]


def upload(j, rec, n_cols, form, min_qv, wb=WB):
    """form: 'bytes' (qualities), 'mask' (a bit per base, derived from them by the library's own host rule at threshold 20),
    'chunks' (three appends), 'window' (records on another context)."""
    a = (rec["pos"], rec["cigar"], rec["cig_off"], rec["seq4"], rec["seq_off"])
    if form == "bytes":
        j.ingest_records(n_cols, wb, *a, rec["qual"], rec["qual_off"], min_qv=min_qv)
    elif form == "mask":
        j.ingest_records(n_cols, wb, *a, min_qv=min_qv, qmask=QMASK(rec))
    elif form == "chunks":
        j.ingest_records_chunked(n_cols, wb, *a, rec["qual"], rec["qual_off"], min_qv=min_qv, chunk_reads=max(1, len(rec["pos"]) // 3))
    else:
        raise AssertionError(form)


def QMASK(rec):
    return capi.qmask_from_quals(rec["seq_off"], rec["qual"], rec["qual_off"], 20)


def rows_of(alleles):
    out = np.zeros(len(alleles), dtype=capi.INSERTION_ALLELE)
    for i, (c, l, s, n) in enumerate(alleles):
        out[i] = (c, l, s, n, 0)
    return out


def check(j, rec, n_cols, form="bytes", min_qv=20, wb=WB, need_all=True):
    """Build with tracking on, then every entry of jcnt and of the table against the mirror."""
    upload(j, rec, n_cols, form, min_qv, wb)
    exp_cnt, exp_alleles = im.walk(rec, n_cols, wb, min_qv, QMASK(rec) if form == "mask" else None)
    if need_all:                                             # nothing passes vacuously
        assert exp_cnt[:, im.INFRAME].any() and exp_cnt[:, im.FRAMESHIFT].any() and exp_cnt[:, im.UNREAD].any() and len(exp_alleles) >= 2
    jcnt, rows = j.insertion_alleles()
    assert jcnt.dtype == np.uint32 and jcnt.shape == (n_cols, 4) and not jcnt[0].any()
    assert (jcnt == exp_cnt).all(), np.argwhere(jcnt != exp_cnt)[:8]
    exp_rows = rows_of(exp_alleles)
    assert len(rows) == len(exp_rows) and (rows == exp_rows).all(), (rows[:8], exp_rows[:8])
    # the consequences of §17: the alleles of a junction add up to its inframe count
    total = np.zeros(n_cols, dtype=np.int64)
    np.add.at(total, rows["col"], rows["count"])
    assert (total == jcnt[:, im.INFRAME]).all()
    assert (jcnt[:, 1:].astype(np.int64).sum(axis=1) <= jcnt[:, im.SPAN]).all()
    return jcnt, rows


# (reads, columns).  The sizes of the kernels (kernels_ins.hip).  The record walk: a lane a read, a wave of 64 groups its events, a
# workgroup is 256 reads: 63 / 64 / 65 and 255 / 256 / 257.  The span pass: a word is 32 reads, a tile 512 reads (16 words), a plane
# row whole 128-byte lines (1024 reads); a lane owns a junction, a workgroup 64 of them and stages their 65 columns: n_cols = 65 is
# one full group, 66 the first junction of a second one, 129 / 130 end the second group at and one past its last junction, 2 and 3
# are one and two junctions.  The reads are split over workgroups in segments of an even number of tiles once there are more than
# two: 1025 reads are segments of 2 + 1 tiles, 2049 reads 2 + 2 + 1.  A single read needs five columns to show all three classes.
CASES = [
    (1, 130), (31, 2), (32, 3), (33, 64), (63, 65), (64, 66), (65, 129), (255, 130), (256, 2), (257, 3), (511, 66), (512, 65),
    (513, 64), (1023, 66), (1024, 65), (1025, 130), (2049, 64), (2049, 3),
]


@pytest.mark.parametrize("n,n_cols", CASES)
def test_counts_and_table_equal_mirror(ctx, n, n_cols):
    rec = im.records(make_reads(n, n_cols, 1000 * n + n_cols), with_qual=True)
    check(ctx, rec, n_cols)
    # the matrix is what a build without tracking makes
    assert (msa.unpack_columns(ctx.download_columns(), n) == records_expand.expand_reference(rec, n_cols, WB, 20)).all()


def test_span_with_segments_of_four_tiles():
    """The smallest read count at 3000 columns at which a workgroup of the span pass walks four tiles (jl_walk_shape_for with 47 groups
    of 64 junctions: more than 174 tiles), so that its prefetching schedule has an iteration with a tile before and a tile after:
    the last segment is shorter than the others and its last tile ragged.  Generated records with insertions, one read in three
    partial; SPAN is the reads covered at c - 1 and at c, counted from the cigars (records_expand.covered_pairs, pinned against the
    mirror's own statement of it in tests/test_insertion_host.py), compared for equality at every junction."""
    import walk_shape
    l = 3000
    n_groups = (l - 1 + 63) // 64
    n, seg_tiles, n_segs = walk_shape.deep_case(lambda n: walk_shape.walk(n, n_groups))
    n_tiles = -(-n // 512)
    assert n_groups == 47 and seg_tiles >= 4 and n_segs >= 2 and n_tiles % seg_tiles != 0 and n % 512 == 300
    assert walk_shape.walk(n - 512, n_groups)[0] < 4                      # ... and one tile fewer has shorter segments
    rec = synth.raw_records(9, n, l, extra=("--ins-ppm", "2500", "--partial", "0.3"))
    exp_span = records_expand.covered_pairs(rec, l)                      # (from the cigars: the expected matrix never exists)
    r0 = n - 600                                                          # ... and over the last two tiles from the matrix itself
    cov = records_expand.expand(rec, l, 0, 0, read_begin=r0, read_end=n) != 6
    tail = {k: rec[k] for k in ("seq4", "seq_off")}
    tail.update(pos=rec["pos"][r0:], cig_off=rec["cig_off"][r0:] - rec["cig_off"][r0], cigar=rec["cigar"][int(rec["cig_off"][r0]):])
    assert (records_expand.covered_pairs(tail, l)[1:] == (cov[:, :-1] & cov[:, 1:]).sum(axis=0)).all()
    assert exp_span[0] == 0 and exp_span[1:].min() > 0 and len(np.unique(exp_span[1:])) > 100      # partial reads: the junctions differ
    j = capi.Juliet(0)
    try:
        j.track_insertion_alleles()
        j.ingest_records(l, 0, rec["pos"], rec["cigar"], rec["cig_off"], rec["seq4"], rec["seq_off"])
        jcnt, rows = j.insertion_alleles()
        assert jcnt.shape == (l, 4) and (jcnt[:, im.SPAN] == exp_span).all(), np.flatnonzero(jcnt[:, im.SPAN] != exp_span)[:8]
        assert jcnt[:, im.INFRAME].any() and jcnt[:, im.FRAMESHIFT].any()
        assert (jcnt[:, 1:].astype(np.int64).sum(axis=1) <= jcnt[:, im.SPAN]).all()
    finally:
        j.close()


@pytest.mark.parametrize("form,min_qv", [("bytes", 0), ("bytes", 20), ("mask", 0), ("mask", 20), ("chunks", 20)])
def test_filter_forms(ctx, form, min_qv):
    """A low quality on ONE inserted base: with the filter on the read moves from inframe to unread, in the byte form and in the mask
    form alike; at min_qv 0 either form applies no filter."""
    reads = make_reads(300, 40, 5)
    reads += [(WB, [("=", 5), ("I", 3), ("=", 5)], "ACGTA" + "GGG" + "ACGTA", [40] * 5 + [40, 19, 40] + [40] * 5),
              (WB, [("=", 5), ("I", 3), ("=", 5)], "ACGTA" + "GGG" + "ACGTA", [40] * 5 + [20, 0xFF, 93] + [40] * 5)]
    rec = im.records(reads, with_qual=True)
    jcnt, rows = check(ctx, rec, 40, form, min_qv)
    ggg = [r for r in rows if r["col"] == 5 and r["len"] == 3 and im.seq_of(r["seq"], 3) == "GGG"]
    assert len(ggg) == 1 and ggg[0]["count"] >= (2 if min_qv == 0 else 1)
    off = im.walk(rec, 40, WB, 0)[0]
    assert (jcnt == off).all() if min_qv == 0 else (jcnt[:, im.UNREAD].sum() > off[:, im.UNREAD].sum())


def hand(ctx, reads, n_cols, wb=0, min_qv=0):
    rec = im.records(reads, with_qual=True)
    return check(ctx, rec, n_cols, "bytes", min_qv, wb, need_all=False)


def test_hand_written_junction_rules(ctx):
    """What counts nowhere, what still spans, what is one insertion: the reads of tests/test_insertion_host.py, whose expectations
    are spelled out there beside the mirror."""
    jcnt, rows = hand(ctx, HAND_READS, 8)
    assert [(int(r["col"]), int(r["len"]), im.seq_of(r["seq"], r["len"]), int(r["count"])) for r in rows] == HAND_ALLELES
    assert jcnt[:, im.FRAMESHIFT].tolist() == HAND_FRAMESHIFT and jcnt[:, im.UNREAD].tolist() == HAND_UNREAD
    # a window beginning inside the reads: junction 0 of the window is never reported, the one at its first column pair is
    jcnt, rows = hand(ctx, HAND_READS, 4, wb=4)
    assert [(int(r["col"]), int(r["len"])) for r in rows] == [(1, 3), (1, 30), (3, 3)] and not jcnt[0].any()
    # ... and a one-column window has no junction at all
    jcnt, rows = hand(ctx, HAND_READS, 1, wb=4)
    assert jcnt.tolist() == [[0, 0, 0, 0]] and len(rows) == 0


def with_anchors(reads):
    """+ four reads that bring the classes a check asks for."""
    s = "ACGTACGTAC"
    return reads + [(0, [("=", 5), ("I", ln), ("=", 5)], s[:5] + text + s[5:]) for ln, text in ((3, "TTT"), (3, "TNT"), (2, "TT"), (6, "TTTTTT"))]


def test_contention_one_allele_in_every_read(ctx):
    """1025 reads with the same insertion: one counter, one slot — the waves add their sums."""
    s = "ACGTACGTAC"
    reads = with_anchors([(0, [("=", 5), ("I", 6), ("=", 5)], s[:5] + "GATTAC" + s[5:])] * 1025)
    rec = im.records(reads, with_qual=True)
    jcnt, rows = check(ctx, rec, 10, wb=0)
    assert jcnt[5].tolist() == [1029, 1027, 1, 1] and (5, 6, 1025) in [(r["col"], r["len"], r["count"]) for r in rows]


def test_table_load_every_read_its_own_allele(ctx):
    """1025 reads, 1025 alleles of six bases at one junction (every pair of neighbours differs in the last base only), and the same
    1025 once more at another junction: keys that differ in their high word only.  The table holds as many slots as the sizing rule gives."""
    s = "ACGTACGTAC"
    word = lambda i: "".join("ACGT"[(i >> (2 * (5 - j))) & 3] for j in range(6))     # noqa: E731
    reads = [(0, [("=", 5), ("I", 6), ("=", 5)], s[:5] + word(i) + s[5:]) for i in range(1025)]
    reads += [(0, [("=", 6), ("I", 6), ("=", 4)], s[:6] + word(i) + s[6:]) for i in range(1025)]
    rec = im.records(with_anchors(reads), with_qual=True)
    jcnt, rows = check(ctx, rec, 10, wb=0)
    assert len(rows) == 2 * 1025 + 2 and (rows["count"] == 1).all()


def test_tracking_off_and_on():
    """Off: the fetch is a state error and the §11 counters are what they are.  On: the matrix and the §11 counters equal the
    untracked build's; a matrix made by anything else afterwards takes the table with it."""
    rec = im.records(make_reads(700, 70, 3), with_qual=True)
    a = (rec["pos"], rec["cigar"], rec["cig_off"], rec["seq4"], rec["seq_off"], rec["qual"], rec["qual_off"])
    j = capi.Juliet(0)
    j.track_insertions()
    j.ingest_records(70, WB, *a, min_qv=20)
    with pytest.raises(capi.JulietError) as e:
        j.insertion_alleles()
    assert e.value.status == -4 and "jl_msa_track_insertion_alleles" in str(e.value)
    plain_cols, (plain_lh, plain_bc) = j.download_columns().copy(), j.insertions_fetch()
    assert plain_lh.any() and plain_bc.any()
    j.track_insertion_alleles()
    check(j, rec, 70)
    assert (j.download_columns() == plain_cols).all()
    lh, bc = j.insertions_fetch()
    assert (lh == plain_lh).all() and (bc == plain_bc).all()
    n = np.zeros(1, dtype=np.uint32)
    lib = capi.load_library()
    assert lib.jl_insertion_alleles_fetch(j.h, None, None, 0, n.ctypes.data) == 0 and n[0] >= 2      # rows == NULL: only the count
    small = np.zeros(1, dtype=capi.INSERTION_ALLELE)
    assert lib.jl_insertion_alleles_fetch(j.h, None, small.ctypes.data, 1, None) == -1               # too little room
    assert "room for 1 rows" in lib.jl_last_error(j.h).decode()
    # records on another context, the window only enqueued: the same table
    src, win = capi.Juliet(0), capi.Juliet(0)
    src.records_upload(*a)
    win.track_insertion_alleles()
    win.records_window(src, 70, WB, 20, wait=False)
    exp_cnt, exp_alleles = im.walk(rec, 70, WB, 20)
    jcnt, rows = win.insertion_alleles()
    assert (jcnt == exp_cnt).all() and (rows == rows_of(exp_alleles)).all()
    # the switch off again: the next build leaves nothing to fetch
    j.track_insertion_alleles(False)
    j.ingest_records(70, WB, *a, min_qv=20)
    with pytest.raises(capi.JulietError):
        j.insertion_alleles()
    # another producer replaces the matrix
    win.upload_rows(records_expand.expand_reference(rec, 70, WB, 20))
    with pytest.raises(capi.JulietError) as e:
        win.insertion_alleles()
    assert e.value.status == -4
    taken = capi.Juliet(0)
    taken.track_insertion_alleles()
    taken.ingest_records(70, WB, *a, min_qv=20)
    taken.insertion_alleles()
    taken.take([(win, np.arange(100, dtype=np.uint32))])
    with pytest.raises(capi.JulietError):
        taken.insertion_alleles()
    for c in (j, src, win, taken):
        c.close()


def test_span_against_the_pileup(ctx):
    """span[c] is at most the reads covering c - 1 and those covering c, from the column pileup of the same matrix."""
    n, n_cols = 1500, 90
    rec = im.records(make_reads(n, n_cols, 11), with_qual=True)
    jcnt, rows = check(ctx, rec, n_cols)
    ctx.pileup_async(np.array([(WB + 1, WB + n_cols + 1)], dtype=capi.GENE))
    cov = ctx.pileup_fetch()["col_counts"].astype(np.int64)[:, :6].sum(axis=1)
    assert len(cov) == n_cols and cov.max() <= n
    assert (jcnt[1:, im.SPAN] <= np.minimum(cov[:-1], cov[1:])).all()
    assert (jcnt[:, 1:].astype(np.int64).sum(axis=1) <= jcnt[:, im.SPAN]).all()


# ---------------------------------------------------------------------------------------------- the command line
N_CLI, L_CLI = 3000, 300
PLANT_COL, SPLIT_COL, PLANT_LEN, PLANT_PERMILLE = 30, 46, 6, 20      # before gene codon 11 (a boundary); inside codon 16


def read_bam(path):
    """The records of a BAM as the arrays the library takes, through the suite's independent reader (tests/bam_py.py)."""
    return bam_py.record_arrays(bam_py.read_bam(str(path))[2])


def juliet(d, *args):
    return subprocess.run([JULIET, *args], cwd=d, capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    d = tmp_path_factory.mktemp("insertions_cli")
    subprocess.check_call([SYNTH, "--reads", str(N_CLI), "--cols", str(L_CLI), "--seed", "23", "--insert", f"{PLANT_COL}:{PLANT_LEN}:{PLANT_PERMILLE}",
                           "--insert", f"{SPLIT_COL}:{PLANT_LEN}:{PLANT_PERMILLE}", "-o", "in.bam", "--config-out", "in.json"], cwd=d)
    r = juliet(d, "-c", "in.json", "--mode-phasing", "--call-insertions", "--timing", "in.bam", "i.json", "i.html")
    assert r.returncode == 0, r.stderr
    assert re.search(r"timing insertions\s", r.stderr)              # the stage line of --timing
    for args in (("--mode-phasing", "in.bam", "plain.json", "plain.html"), ("--call-insertions", "in.bam", "i0.json", "i0.html"),
                 ("in.bam", "plain0.json", "plain0.html"), ("--call-insertions", "--insertion-rate", "0.004", "in.bam", "r.json")):
        p = juliet(d, "-c", "in.json", *args)
        assert p.returncode == 0, p.stderr
    rec = read_bam(d / "in.bam")
    assert len(rec["pos"]) == N_CLI
    return d, im.walk(rec, L_CLI)


CODONS = [a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT"]


def expected_entries(walked, n_tests, rate):
    """insertion_positions of the one gene (columns 0 .. L_CLI): the mirror's alleles at codon starts and the exact test."""
    jcnt, alleles = walked
    out = []
    for c, l, s, n in alleles:
        if c % 3 or c == 0:
            continue
        t = im.test(n, jcnt[c], rate, n_tests)
        if t["called"]:
            text = im.seq_of(s, l)
            out.append((c // 3, [text[k:k + 3] for k in range(0, l, 3)], t))
    return out


@pytest.mark.parametrize("name,rate", [("i.json", 1.0e-3), ("i0.json", 1.0e-3), ("r.json", 4.0e-3)])
def test_cli_block_equals_the_mirror_and_the_exact_test(cli, name, rate):
    d, walked = cli
    jcnt, alleles = walked
    assert {c for c, _, _, _ in alleles} >= {PLANT_COL, SPLIT_COL}        # both plants are in the records
    exp = expected_entries(walked, L_CLI // 3, rate)                     # (the BAM says SEQUEL: its deletion rate is the default)
    assert [e[0] for e in exp] == [PLANT_COL // 3]                       # the plant at the codon boundary and nothing else
    genes = json.load(open(d / name))["genes"]
    assert len(genes) == 1
    got = genes[0]["insertion_positions"]
    assert len(got) == len(exp)
    for g, (after, codons, t) in zip(got, exp):
        assert list(g) == ["after_position", "inserted_codons", "inserted_amino_acids", "count", "coverage", "frequency", "expected", "pValue",
                           "log_pValue", "frameshift_reads", "unread_reads"]
        assert (g["after_position"], g["inserted_codons"], g["count"], g["coverage"], g["expected"], g["frameshift_reads"], g["unread_reads"]) == \
            (after, codons, t["count"], t["coverage"], t["expected"], t["frameshift"], t["unread"])
        assert len(g["inserted_amino_acids"]) == len(codons) and g["frequency"] == t["count"] / t["coverage"]
        p_adj, lp = float(t["p_adj"]), math.log(float(t["p"]))
        assert abs(g["pValue"] - p_adj) <= 5e-12 * p_adj and abs(g["log_pValue"] - lp) <= 1e-12 * max(1.0, abs(lp)) + 1e-13
    # the plant that splits codon 16 is in nobody's list
    assert all(3 * g["after_position"] != SPLIT_COL - SPLIT_COL % 3 for g in got)
    assert 40 <= got[0]["count"] <= 80 and got[0]["coverage"] > 2000


def json_number(v):
    """A number as the JSON writer prints it."""
    return "%.0f" % v if v == int(v) else "%.17g" % v


def test_cli_html_holds_one_row_per_entry(cli):
    d, _ = cli
    got = json.load(open(d / "i.json"))["genes"][0]["insertion_positions"]
    html = open(d / "i.html").read()
    block = re.search(r'<details open id="insertions">.*?</details>', html, flags=re.S).group(0)
    trs = [re.findall(r"<td>(.*?)</td>", tr) for tr in re.findall(r'<tr class="insertion">.*?</tr>', block)]
    assert len(trs) == len(got) == 1
    for cells, g in zip(trs, got):
        assert cells == [str(g["after_position"]), " ".join(g["inserted_codons"]), g["inserted_amino_acids"]] + \
            [json_number(g[k]) for k in ("count", "coverage", "frequency", "expected", "pValue", "log_pValue", "frameshift_reads", "unread_reads")]


def strip_json(text):
    j = json.loads(text)
    j["input"].pop("timestamp")
    j["input"].pop("command_line")
    for g in j["genes"]:
        g.pop("insertion_positions", None)
    return json.dumps(j, indent=1)


def strip_html(text):
    text = re.sub(r'<details open id="insertions">.*?</table>\n</details>\n', "", text, flags=re.S)
    return re.sub(r"<tr><th>(timestamp|command_line)</th>.*?</tr>\n", "", text)


def test_cli_without_the_flag_the_outputs_are_the_plain_run(cli):
    d, _ = cli
    for with_flag, plain in (("i", "plain"), ("i0", "plain0")):
        assert "insertion_positions" in open(d / (with_flag + ".json")).read() and "insertion" not in open(d / (plain + ".json")).read()
        assert strip_json(open(d / (with_flag + ".json")).read()) == strip_json(open(d / (plain + ".json")).read())
        html, plain_html = open(d / (with_flag + ".html")).read(), open(d / (plain + ".html")).read()
        assert 'id="insertions"' in html and "insertion" not in plain_html
        assert strip_html(html) == strip_html(plain_html)


def test_cli_drm_only_is_empty(cli):
    d, _ = cli
    r = juliet(d, "-c", "in.json", "--call-insertions", "--drm-only", "in.bam", "drm.json")
    assert r.returncode == 0, r.stderr
    assert json.load(open(d / "drm.json"))["genes"][0]["insertion_positions"] == []
