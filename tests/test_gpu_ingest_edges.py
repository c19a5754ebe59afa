"""The record ingest (csrc/kernels_ingest.hip) at the edges its constants draw, each from explicit cigars: a case says in its docstring
why its reads land where they do.  Every cell against records_expand.expand, in the three filter modes: none, quality bytes with
min_qv 20 and qualities on both sides of it, and the same filter as a bit mask.  (The counters of a build are not exported: that a
case takes the path it is built for follows from the constants, not from an assertion.)

The constants: a sweep is kSweep = 256 columns, a tile kTileReads = 128 reads in two read waves of 64; the planes kernel's first
size has room for kEntPerRead = 4 entries a read — kEntCapWave = 4 x 64 = 256 a read wave — the second for 16: 1024 a wave.
The entries of a (read, sweep): from the one that holds the sweep's first column to the first that begins behind its last one, both
counted — k deletions inside a sweep that the read covers whole are k + 1 aligned runs, k deletions and the closing entry: 2 k + 2;
a read that ends inside the sweep closes with its end AND the 'never' entry: one more."""
import numpy as np
import pytest

import records_expand
from minorseq_amd import capi
from test_gpu_parity import _records_from_cigars
from test_gpu_qmask import MIN_QV, five, matrix, np_mask

pytestmark = pytest.mark.gpu

MODES = ("none", "bytes", "mask")


@pytest.fixture(scope="module")
def ctxs():
    rec, win = capi.Juliet(0), capi.Juliet(0)
    yield rec, win
    win.close()
    rec.close()


def records_of(cigars, seed, pos=None):
    """the records of the cigars, qualities on both sides of MIN_QV and a few absent ones"""
    rng = np.random.default_rng(seed)
    rec = _records_from_cigars(cigars, rng, pos)
    rec["qual"] = rng.integers(0, 41, len(rec["qual"])).astype(np.uint8)
    rec["qual"][::97] = 0xFF
    return rec


def check(ctxs, rec, windows, modes=MODES):
    """every cell of every window (first column, columns) in every mode; the expected matrices are made once"""
    jl, w = ctxs
    n = len(rec["pos"])
    exp = {}
    for mode in modes:
        more = {"none": {}, "bytes": {"qual": rec["qual"], "qual_off": rec["qual_off"]}, "mask": {"qmask": np_mask(rec, MIN_QV)}}[mode]
        jl.records_upload(*five(rec), **more)
        try:
            for b, cols in windows:
                qv = 0 if mode == "none" else MIN_QV          # (a stream without qualities is never filtered)
                if (b, cols, qv) not in exp:
                    exp[b, cols, qv] = records_expand.expand(rec, cols, b, qv)
                w.records_window(jl, cols, b, MIN_QV)
                got = matrix(w, n)
                diff = np.argwhere(got != exp[b, cols, qv])
                assert len(diff) == 0, (mode, b, cols, "read %d column %d" % tuple(diff[0]), len(diff))
        finally:
            jl.records_drop()
    if "bytes" in modes:
        assert any((exp[b, c, MIN_QV] != exp[b, c, 0]).any() for b, c in windows if (b, c, 0) in exp)


def with_deletions(k, tail, every=20):
    """k deletions of one column, `every` aligned columns before each, `tail` aligned columns behind the last"""
    return [("=", every), ("D", 1)] * k + [("=", tail)]


PLAIN = [("=", 300)]                  # one entry covers each of the two sweeps of a 300-column window
COLS = 300


@pytest.mark.parametrize("busy_tile", [1, 0])
def test_sibling_tiles_one_stays_one_is_handed_on(ctxs, busy_tile):
    """256 reads = tiles 0 and 1 of group 0, the two units a workgroup of the first size takes one after the other where it takes two
    (the byte and the mask mode).  The reads of one tile have two deletions in sweep 0: 2 x 2 + 2 = 6 entries each, 64 x 6 = 384 a
    read wave > kEntCapWave = 256 — the unit goes to the second size and the workgroup stores the OTHER tile's words alone (its
    bit of `ok`); the other tile's reads have one entry a sweep.  Both ways round.  Sweep 1 (44 columns) is plain in both."""
    busy = with_deletions(2, COLS - 2 * 21)
    cigars = [busy if i // 128 == busy_tile else PLAIN for i in range(256)]
    check(ctxs, records_of(cigars, 1 + busy_tile), [(0, COLS)])


@pytest.mark.parametrize("wave", [0, 1])
@pytest.mark.parametrize("extra", [0, 1])
def test_read_wave_entries_first_size(ctxs, wave, extra):
    """One deletion a read in sweep 0 = 4 entries: the 64 reads of a read wave fill its part of the entry area exactly (64 x 4 =
    kEntCapWave = 256: `off_e + n_ent > kEntCapWave` is false for the last of them) and the unit stays in the first size.  extra: the
    wave's LAST read also ends inside the sweep — 5 entries, 257 — and the unit is handed on.  The other wave's reads have one entry."""
    four, five_ = with_deletions(1, COLS - 21, 100), with_deletions(1, 50, 100)
    cigars = [four if i // 64 == wave else PLAIN for i in range(128)]
    if extra:
        cigars[64 * wave + 63] = five_
    check(ctxs, records_of(cigars, 10 + 2 * wave + extra), [(0, COLS)])


@pytest.mark.parametrize("extra", [0, 1])
def test_read_wave_entries_second_size(ctxs, extra):
    """Seven deletions a read in sweep 0 = 16 entries: 64 x 16 = 1024 = the second size's kEntCapWave, to which the first size hands
    the unit on (1024 > 256) and where it fits exactly.  extra: the wave's last read ends inside the sweep as well — 17 entries, 1025 —
    and is left to the column-by-column path behind the workgroup's stores (slow_pair), the other 63 are not.  The reads of the
    other read wave have one entry; sixteen entries are also two trips for the entries beyond the eighth."""
    cigars = [with_deletions(7, COLS - 7 * 21) if i < 64 else PLAIN for i in range(128)]
    if extra:
        cigars[63] = with_deletions(7, 50)
    check(ctxs, records_of(cigars, 20 + extra), [(0, COLS)])


def test_eight_and_nine_entries_in_a_sweep(ctxs):
    """A read thread asks for a sweep's first eight entries in four 16-byte requests; a ninth is another trip (`for i = 8 ..`).  Three
    deletions = 8 entries; three deletions and the read's end inside the sweep = 9; 7 and 10 on either side."""
    kinds = [with_deletions(3, COLS - 3 * 21), with_deletions(3, 50), with_deletions(2, 50), with_deletions(4, COLS - 4 * 21), PLAIN]
    cigars = [kinds[i % len(kinds)] for i in range(40)]
    check(ctxs, records_of(cigars, 30), [(0, COLS)])


def test_inserted_bases_a_row_takes_and_one_more(ctxs):
    """A staging row is kRowPieces = 9 pieces = 288 bases for a sweep's 256; its first piece begins on the DWORD of the sweep's first
    base, up to seven bases before it: 7 + 256 + 25 = 288 — 25 inserted bases in a sweep fit whatever the alignment, the 26th
    asks for a tenth piece when the first base is the last of its dword (np > kRowPieces: slow_pair).  Where the first base lies
    follows from the read's first byte in the resident bases (mod 4) and from its soft clip (0..7 bases): all 32 combinations,
    with 25 and with 26 inserted bases — a short read in front of each puts its first byte where the case wants it."""
    cigars, at, want = [], 0, []
    for ins in (25, 26):
        for clip in range(8):
            for first in range(4):
                fill = 20 + (first - at - 20) % 4                     # bytes of the read in front
                cigars.append([("=", 2 * fill)])
                bases = clip + 300 + ins
                cigars.append(([("S", clip)] if clip else []) + [("=", 100), ("I", ins), ("=", 200)])
                want.append(first)
                at += fill + (bases + 1) // 2
    rec = records_of(cigars, 40)
    assert (rec["seq_off"][1:-1:2].astype(np.int64) % 4 == np.array(want)).all()
    check(ctxs, rec, [(0, COLS)])


@pytest.mark.parametrize("last", [1, 7, 8, 9])
def test_last_sweep_width(ctxs, last):
    """The window's last sweep is 1, 7, 8 or 9 columns wide: one ragged block of eight columns, one whole block (the store without
    a question per column), a whole block and a ragged one — for one tile a workgroup (no filter) and two (bytes, mask): 200
    reads, tile 1 partial.  Every third read has a deletion across the last sweep's first column, every third ends in it."""
    cols = 256 + last
    kinds = [[("=", 320)], [("=", 250), ("D", 8), ("=", 62)], [("=", 257)], [("=", 254), ("D", 1), ("X", 3)]]
    cigars = [kinds[i % len(kinds)] for i in range(200)]
    check(ctxs, records_of(cigars, 50 + last), [(0, cols), (3, cols)])


def test_window_begins_inside_a_deletion_and_at_an_insertion(ctxs):
    """Runs that begin before the window begin at its column 0 with their query offset moved along (window_col's `before`).  The
    reads: 50 aligned columns, a deletion over 50..59, aligned 60..109, five inserted bases, aligned 110..309.  Windows that begin
    at the deletion's first, a middle and its last column and just behind it; at the last column before the insertion and at
    the first behind it (the inserted bases are skipped in the query, not in the columns)."""
    cig = [("=", 50), ("D", 10), ("=", 50), ("I", 5), ("=", 200)]
    cigars = [([("S", i % 3)] if i % 3 else []) + cig for i in range(70)]
    pos = [i % 2 for i in range(70)]
    check(ctxs, records_of(cigars, 60, pos), [(b, 270 - b) for b in (50, 55, 59, 60, 61, 109, 110, 111)])


def alternating(n_runs, aligned, gap="D"):
    return [("=", aligned) if k % 2 == 0 else (gap, 1) for k in range(n_runs)]


def test_long_read_over_sixteen_sweeps(ctxs):
    """cigar_runs_kernel writes the descriptors of a long read a lane per sweep, kDescSweeps = 15 sweeps a pass: a window of 3900
    columns has 16 sweeps, so a second pass writes the last one's.  (Wider than the other cases by need; seven reads.)  The long
    reads — 41, 61 and 199 runs (more than the 37 cigar_walk_kernel keeps), and 193 ops of one run — cover all sixteen sweeps or begin
    in the second; short reads among them, one with a reference skip over eight sweeps."""
    cols = 3900
    cigars = [alternating(41, 190), [("=", 3900)], alternating(199, 38), [("=", 20) if k % 2 == 0 else ("X", 1) for k in range(193)],
              alternating(41, 170), [("=", 1000), ("N", 2000), ("=", 900)], alternating(61, 110, "N")]
    pos = [0, 0, 0, 300, 300, 0, 0]
    assert 15 * 256 < cols <= 16 * 256
    check(ctxs, records_of(cigars, 70, pos), [(0, cols), (5, cols - 5)], modes=("none", "bytes"))


@pytest.mark.parametrize("n_runs", [509, 510])
def test_long_read_entries_in_lds_and_read_back(ctxs, n_runs):
    """A wave of cigar_runs_kernel keeps kRunsLds = 512 entries of each of its four reads in LDS: 509 runs and the three sentinel
    entries fill them exactly (`n_max + 3 <= kRunsLds`), 510 runs make the wave read entry 512 back from HBM behind its release
    fence.  The longest of the wave's reads decides, so the 510-run case has shorter long reads next to it and the 509-run case
    nothing longer.  Two aligned columns and a deletion in turns: 764 columns, ~170 entries a sweep — the second size of the planes kernel."""
    cigars = [[("=", 800)], alternating(n_runs, 2), alternating(39, 20), [("=", 700)], alternating(n_runs - 2, 2, "N"), alternating(509, 2)]
    check(ctxs, records_of(cigars, 80 + n_runs), [(0, 800), (100, 500)], modes=("none", "mask"))
