"""The record ingest with the QV filter as one bit per base (jl_records_append_masked, include/juliet_hip.h) instead of one quality
byte per base and a threshold.  The device gets the records' bases and a mask made HERE with numpy (not by
jl_qmask_from_quals); the reference of every cell is records_expand.expand on the records WITH their quality bytes."""
import json
import os
import subprocess

import numpy as np
import pytest

import records_expand
from minorseq_amd import capi, msa, synth
from test_gpu_parity import _records_from_cigars, rows_to_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JULIET = os.path.join(ROOT, "minorseq_amd", "bin", "juliet")
SYNTH = os.path.join(ROOT, "minorseq_amd", "bin", "juliet-synth")
MIN_QV = 20
JL_ERR_ARG = -1
FIVE = ("pos", "cigar", "cig_off", "seq4", "seq_off")


def np_mask(rec, min_qv):
    """bit 2 * (seq_off[r] - seq_off[0]) + q of base q of read r: qual < min(min_qv, 127) and qual != 0xFF"""
    so, qo = rec["seq_off"].astype(np.int64), rec["qual_off"].astype(np.int64)
    lens = np.diff(qo)
    q = np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(qo[:-1] - qo[0], lens)
    i = np.repeat(2 * (so[:-1] - so[0]), lens) + q
    qual = rec["qual"][int(qo[0]):int(qo[-1])]
    flag = (qual < min(min_qv, 127)) & (qual != 0xFF)
    bits = np.zeros(8 * ((int(so[-1] - so[0]) + 3) // 4), dtype=np.uint8)
    bits[i[flag]] = 1
    return np.packbits(bits, bitorder="little")


def five(rec):
    return [rec[k] for k in FIVE]


def matrix(ctx, n):
    return msa.unpack_columns(ctx.download_columns(), n)


@pytest.fixture(scope="module")
def ctxs():
    rec, win = capi.Juliet(0), capi.Juliet(0)
    yield rec, win
    win.close()
    rec.close()


RICH = ("--rich-qv",)
NOISY = ("--ins-ppm", "2500", "--clips", "--low-qv-ppm", "20000", "--partial", "0.3")
_sets = {}


def records(n, l, extra):
    key = (n, l, extra)
    if key not in _sets:
        rec = synth.raw_records(11 + n, n, l, extra=extra)
        assert ((rec["qual"] < MIN_QV).sum() > 0) and ((rec["qual"] >= MIN_QV).sum() > 0)
        _sets[key] = (rec, np_mask(rec, MIN_QV))
    return _sets[key]


WINDOWS = ((0, 600), (37, 560), (150, 333))     # the whole reference; begins inside the reads, 560 % 256 != 0; ends mid-read


@pytest.mark.parametrize("n", [300, 1100])      # three tiles of 128 reads, the last partial; across the 1024-read group line
@pytest.mark.parametrize("extra", [RICH, NOISY], ids=["rich", "noisy"])
def test_masked_windows_match_every_cell(ctxs, n, extra):
    jl, w = ctxs
    rec, mask = records(n, 600, extra)
    got = {}
    jl.records_upload(*five(rec), qmask=mask)
    try:
        for b, cols in WINDOWS:
            w.records_window(jl, cols, b, MIN_QV)
            got[b, cols] = matrix(w, n)
            assert (got[b, cols] == records_expand.expand(rec, cols, b, MIN_QV)).all(), (b, cols)
            w.records_window(jl, cols, b, 0)          # min_qv 0: the same upload, the letters kept
            assert (matrix(w, n) == records_expand.expand(rec, cols, b, 0)).all(), (b, cols)
    finally:
        jl.records_drop()
    # the byte form of the same records: the same resident matrix
    jl.records_upload(*five(rec), rec["qual"], rec["qual_off"])
    try:
        for b, cols in WINDOWS:
            w.records_window(jl, cols, b, MIN_QV)
            assert (matrix(w, n) == got[b, cols]).all(), (b, cols)
    finally:
        jl.records_drop()


def test_masked_dense_runs_take_the_slow_path(ctxs):
    """A deletion at every other column (test_device_ingest_dense_runs_take_the_slow_path's construction), random qualities: most
    (read, sweep) pairs go column by column (slow_pair), which takes one bit per base."""
    jl, _ = ctxs
    n, l = 700, 1000
    rng = np.random.default_rng(5)
    sp = synth.SynthParams(seed=41, partial_rate=0.2, mask_rate=0.02, sub_rate=0.01)
    ref = synth.reference(sp.seed, l)
    rows = synth.rows(sp, l, 0, n, ref)
    dense = rows[:, 1::2]
    dense[dense < 6] = 4
    rows[3] = 6
    names = FIVE + ("qual", "qual_off")
    rec = dict(zip(names, rows_to_records(rows, ref, rng)))
    assert np.diff(rec["cig_off"]).max() > 600
    rec["qual"] = rng.integers(0, 41, len(rec["qual"])).astype(np.uint8)      # about half below 20
    rec["qual"][::97] = 0xFF
    mask = np_mask(rec, MIN_QV)
    for b, cols in ((0, l), (77, l - 133)):
        jl.ingest_records(cols, b, *five(rec), min_qv=MIN_QV, qmask=mask)
        exp = records_expand.expand(rec, cols, b, MIN_QV)
        assert (exp == 5).sum() > exp.size // 8
        assert (matrix(jl, n) == exp).all(), (b, cols)


def test_masked_indel_rich_second_size(ctxs):
    """An indel every 50 columns: units the first size hands on to the second (BIG) instantiation."""
    jl, _ = ctxs
    n, l = 400, 1500
    rec = synth.raw_records(77, n, l, extra=("--rich-qv", "--ins-ppm", "20000", "--del", "0.02", "--low-qv-ppm", "20000"))
    mask = np_mask(rec, MIN_QV)
    for b, cols in ((0, l), (301, 1111)):
        jl.ingest_records(cols, b, *five(rec), min_qv=MIN_QV, qmask=mask)
        assert (matrix(jl, n) == records_expand.expand(rec, cols, b, MIN_QV)).all(), (b, cols)


@pytest.mark.parametrize("with_long", [False, True])
def test_masked_reads_at_the_long_read_boundary(ctxs, with_long):
    """Reads of 35..37 runs and 192 ops (cigar_walk_kernel), and with 38, 39, 60 runs and 193 ops among them (cigar_runs_kernel),
    built as in test_device_ingest_reads_at_the_long_read_boundary: both kernels without qual_off."""
    jl, w = ctxs
    rng = np.random.default_rng(31 + with_long)
    l = 700

    def alternating(n_runs, gap="D"):
        return [("=", 600 // n_runs) if k % 2 == 0 else (gap, 1 + k % 3) for k in range(n_runs)]

    cigars = []
    for n_runs in (1, 5, 35, 36, 37):
        cigars += [alternating(n_runs), alternating(n_runs, "N"), [("S", 3)] + alternating(n_runs) + [("H", 2)]]
    cigars.append([("=", 2) if k % 2 == 0 else ("X", 1) for k in range(192)])
    cigars.append(sum(([("=", 20), ("I", 2)] for _ in range(14)), []) + [("=", 20)])
    if with_long:
        for n_runs in (38, 39, 60):
            cigars += [alternating(n_runs), alternating(n_runs, "N")]
        cigars.append([("=", 2) if k % 2 == 0 else ("X", 1) for k in range(193)])
    cigars = [cigars[i] for i in rng.permutation(len(cigars))] * 3
    rec = _records_from_cigars(cigars, rng, [int(p) for p in rng.integers(0, 60, len(cigars))])
    rec["qual"] = rng.integers(0, 41, len(rec["qual"])).astype(np.uint8)
    n = len(cigars)
    jl.records_upload(*five(rec), qmask=np_mask(rec, MIN_QV))
    try:
        for b, cols, min_qv in ((0, l, 0), (17, 623, MIN_QV), (300, 1, MIN_QV)):
            w.records_window(jl, cols, b, min_qv)
            assert (matrix(w, n) == records_expand.expand(rec, cols, b, min_qv)).all(), (b, cols, min_qv)
    finally:
        jl.records_drop()


@pytest.mark.parametrize("chunk", [1, 7, 133])
def test_masked_chunks_equal_one_append(ctxs, chunk):
    """Chunks whose base-byte counts are no multiples of 4 or 16: the library starts each on a 16-byte boundary of its arrays and
    puts the chunk's mask at the matching dword."""
    jl, _ = ctxs
    n, l = 300, 600
    rec, mask = records(n, l, NOISY)
    assert (np.diff(rec["qual_off"].astype(np.int64)) % 2 == 1).sum() > n // 4          # odd-length reads: spare nibbles
    nbytes = np.diff(rec["seq_off"].astype(np.int64)[::chunk])
    assert (nbytes % 4 != 0).any() and (nbytes % 16 != 0).any()
    exp = records_expand.expand(rec, 560, 37, MIN_QV)
    jl.ingest_records(560, 37, *five(rec), min_qv=MIN_QV, qmask=mask)
    one = matrix(jl, n)
    assert (one == exp).all()
    jl.ingest_records_chunked(560, 37, *five(rec), min_qv=MIN_QV, chunk_reads=chunk, qmask=mask)
    assert (matrix(jl, n) == one).all()


def test_masked_chunk_from_the_middle_of_larger_arrays(ctxs):
    """seq_off[0] != 0: the mask begins at the chunk's first base all the same."""
    jl, _ = ctxs
    n, l = 300, 600
    rec, _ = records(n, l, NOISY)
    a, b = 41, 263
    sub = {"pos": rec["pos"][a:b], "cigar": rec["cigar"], "seq4": rec["seq4"], "qual": rec["qual"],
           "cig_off": rec["cig_off"][a:b + 1], "seq_off": rec["seq_off"][a:b + 1], "qual_off": rec["qual_off"][a:b + 1]}
    assert sub["seq_off"][0] % 16 != 0
    jl.ingest_records(l, 0, *five(sub), min_qv=MIN_QV, qmask=np_mask(sub, MIN_QV))
    assert (matrix(jl, b - a) == records_expand.expand(rec, l, 0, MIN_QV)[a:b]).all()


def test_mixed_forms_are_refused(ctxs):
    jl, _ = ctxs
    rec, mask = records(300, 600, RICH)
    lib, p = jl.lib, capi._p
    args = [300] + [p(np.ascontiguousarray(x)) for x in five(rec)]
    qual, qo = p(rec["qual"]), p(rec["qual_off"])

    def begin():
        assert lib.jl_records_begin(jl.h, 300, 0, 0, 0) == 0

    def refused(rc, word):
        assert rc == JL_ERR_ARG
        assert word in lib.jl_last_error(jl.h).decode(), lib.jl_last_error(jl.h)
        begin()                                                             # the stream is dropped; a new one begins
        assert lib.jl_records_append_masked(jl.h, *args, p(mask)) == 0
        jl.records_drop()

    begin()
    assert lib.jl_records_append(jl.h, *args, None, None) == 0
    refused(lib.jl_records_append_masked(jl.h, *args, p(mask)), "mask")     # masked after unmasked
    begin()
    assert lib.jl_records_append_masked(jl.h, *args, p(mask)) == 0
    refused(lib.jl_records_append(jl.h, *args, None, None), "mask")         # unmasked after masked
    begin()
    assert lib.jl_records_append(jl.h, *args, qual, qo) == 0
    refused(lib.jl_records_append_masked(jl.h, *args, p(mask)), "mask")     # masked after qualities
    begin()
    assert lib.jl_records_append_masked(jl.h, *args, p(mask)) == 0
    refused(lib.jl_records_append(jl.h, *args, qual, qo), "mask")           # qualities after masked
    begin()
    refused(lib.jl_records_append_masked(jl.h, *args, None), "no mask")     # a NULL mask


def test_insertion_counters_do_not_depend_on_the_form(ctxs):
    jl, _ = ctxs
    rec, mask = records(300, 600, NOISY)
    jl.track_insertions(True)
    try:
        jl.ingest_records(600, 0, *five(rec), min_qv=MIN_QV, qmask=mask)
        lh_m, bc_m = jl.insertions_fetch()
        jl.ingest_records(600, 0, *five(rec), rec["qual"], rec["qual_off"], min_qv=MIN_QV)
        lh_b, bc_b = jl.insertions_fetch()
    finally:
        jl.track_insertions(False)
    assert lh_m.sum() > 0 and (lh_m == lh_b).all() and (bc_m == bc_b).all()


def test_empty_stream_is_refused_and_the_contexts_go_on(ctxs):
    """A stream nothing was appended to builds no matrix: jl_records_finish, jl_records_window and jl_records_window_async refuse
    it as an "empty matrix" (the matrix is allocated first, so the ingest's launches never see zero reads).  The contexts take a
    plain ingest afterwards — 300 reads: three tiles, the last one partial."""
    jl, w = ctxs
    lib = jl.lib
    rec, _ = records(300, 600, RICH)
    exp = records_expand.expand(rec, 600, 0, 0)

    def refused(ctx, rc):
        assert rc == JL_ERR_ARG
        assert "empty matrix" in lib.jl_last_error(ctx.h).decode(), lib.jl_last_error(ctx.h)

    def plain(ctx):
        ctx.ingest_records(600, 0, *five(rec))
        assert (matrix(ctx, 300) == exp).all()

    assert lib.jl_records_begin(jl.h, 0, 0, 0, 0) == 0
    refused(jl, lib.jl_records_finish(jl.h, 600, 0, MIN_QV))
    plain(jl)
    for window in (lib.jl_records_window, lib.jl_records_window_async):
        assert lib.jl_records_begin(jl.h, 0, 0, 0, 0) == 0
        refused(w, window(jl.h, w.h, 600, 0, MIN_QV))
        plain(jl)
        plain(w)


_noisy_window = {}


def noisy_window(min_qv):
    """records(300, 600, NOISY) in the window (37, 560)"""
    if min_qv not in _noisy_window:
        _noisy_window[min_qv] = records_expand.expand(records(300, 600, NOISY)[0], 560, 37, min_qv)
    return _noisy_window[min_qv]


@pytest.mark.parametrize("kind", ["none", "bytes", "mask"])
def test_one_resident_stream_mode_chosen_per_build(ctxs, kind):
    """One upload, the window built with min_qv 0, 20 and 0 again: the filter is on or off per build, whatever form the stream
    carries it in; a stream without qualities is never filtered.  The quality COUNT of a stream with quality bytes is checked
    at min_qv 0 too (the cigar kernels get the quality offsets whenever the stream has qualities)."""
    jl, w = ctxs
    rec, mask = records(300, 600, NOISY)
    more = {"none": {}, "bytes": {"qual": rec["qual"], "qual_off": rec["qual_off"]}, "mask": {"qmask": mask}}[kind]
    jl.records_upload(*five(rec), **more)
    try:
        for min_qv in (0, MIN_QV, 0):
            w.records_window(jl, 560, 37, min_qv)
            assert (matrix(w, 300) == noisy_window(0 if kind == "none" else min_qv)).all(), min_qv
    finally:
        jl.records_drop()
    if kind != "bytes":
        return
    short = rec["qual_off"].copy()       # read 7: one quality fewer than its cigar consumes
    assert short[8] - short[7] > 1
    short[8:] -= 1
    jl.records_upload(*five(rec), rec["qual"], short)
    try:
        with pytest.raises(capi.JulietError) as err:
            w.records_window(jl, 560, 37, 0)
        assert "record 7: its cigar consumes more qualities than the record holds" in str(err.value)
    finally:
        jl.records_drop()


# --------------------------------------------------------------------------------------------- the command line
def _norm(path):
    j = json.load(open(path))
    j["input"].pop("timestamp")
    j["input"].pop("command_line")
    j["input"].pop("input_file", None)
    return j


def test_cli_mask_upload_equals_byte_upload(tmp_path):
    """`juliet --min-qv 20 --qv-upload mask` uploads the filter as a mask, `--qv-upload bytes` the quality bytes, and without the
    option one of the two: the same JSON — plain, with --windows 3, and as two lines of a --batch list."""
    d = tmp_path
    subprocess.check_call([SYNTH, "--reads", "3000", "--cols", "900", "--seed", "5", "--rich-qv", "-o", str(d / "a.bam"),
                           "--config-out", str(d / "cfg.json")])
    opts = ["-c", "cfg.json", "--mode-phasing", "--min-qv", "20"]

    def run(*more):
        r = subprocess.run([JULIET, *opts, *more], cwd=d, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr

    run("--qv-upload", "bytes", "a.bam", "bytes.json")
    run("a.bam", "mask.json")
    run("--qv-upload", "mask", "a.bam", "mask2.json")
    ref = _norm(d / "bytes.json")
    assert ref["genes"][0]["variant_positions"]
    assert _norm(d / "mask.json") == ref and _norm(d / "mask2.json") == ref
    run("--windows", "3", "--qv-upload", "bytes", "a.bam", "w_bytes.json")
    run("--windows", "3", "--qv-upload", "mask", "a.bam", "w_mask.json")
    run("--windows", "3", "a.bam", "w_default.json")
    assert _norm(d / "w_mask.json") == _norm(d / "w_bytes.json") == _norm(d / "w_default.json")
    for form in ("mask", "bytes"):
        (d / "list.tsv").write_text(f"a.bam\t{form}0.json\na.bam\t{form}1.json\n")
        run("--qv-upload", form, "--batch", "list.tsv")
        assert _norm(d / f"{form}0.json") == ref and _norm(d / f"{form}1.json") == ref
