"""The host-only half of the reading-frame screen (docs/SPEC.md §27): the by-row mirror on rows small enough to count by hand,
jl_orf_classify and jl_orf_filter against it over every flag combination, at the tail and deletion bounds and at every refusal, the
invariants of the launch shape, what the library exports, and the command lines the front end refuses before it reads a file.  No
GPU: the library only has to load."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import orf_mirror as om
import orf_shape
from minorseq_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JULIET = os.path.join(ROOT, "minorseq_amd", "bin", "juliet")
NAMES = ("jl_read_orf_async", "jl_read_orf_fetch", "jl_orf_classify", "jl_orf_filter")
A, Cc, G, T = om.A, om.C, om.G, om.T


# ---------------------------------------------------------------------------------------------- the mirror, counted by hand
def test_mirror_on_hand_counted_rows():
    ref = np.array([Cc, T, A, A, Cc, Cc, Cc, T, G, A, 5], dtype=np.uint8)      # frame 1: TAA CCC TGA; frame 0: CTA ACC CTG
    rows = np.array([
        [Cc, T, A, G, T, G, A, T, A, A, Cc],     # frame 1: TAG (ref stop: masked) TGA (counted, k = 1) TAA (masked); frame 0: CTA GTG ATA
        [6, 6, 6, 6, T, A, A, 4, 4, 4, Cc],      # frame 1: uncovered codon, TAA at k = 1, a gap codon
        [Cc, Cc, 5, Cc, T, 4, A, Cc, Cc, Cc, 6], # N makes codon 0 unread (covered, no gap); T-A is no codon: a gap cell inside
        [T, A, A, T, A, G, T, G, A, Cc, Cc],     # frame 0: TAA TAG TGA, all counted (ref frame 0 has no stop)
    ], dtype=np.uint8)
    spans = [(1, 3), (0, 3)]
    cnt, first = om.counters(rows, spans, ref)
    assert cnt.dtype == np.uint32 and cnt.shape == (4, 2, 4) and first.shape == (2, 4)
    assert cnt[om.COVERED, 0].tolist() == [9, 6, 9, 9] and cnt[om.COVERED, 1].tolist() == [9, 5, 9, 9]
    assert cnt[om.GAP_CELLS, 0].tolist() == [0, 3, 1, 0] and cnt[om.GAP_CELLS, 1].tolist() == [0, 2, 1, 0]
    assert cnt[om.CODONS_READ, 0].tolist() == [3, 1, 1, 3] and cnt[om.CODONS_READ, 1].tolist() == [3, 0, 1, 3]
    assert cnt[om.STOPS, 0].tolist() == [1, 1, 0, 0] and first[0].tolist() == [1, 1, om.NO_STOP, om.NO_STOP]
    assert cnt[om.STOPS, 1].tolist() == [0, 0, 0, 3] and first[1].tolist() == [om.NO_STOP, om.NO_STOP, om.NO_STOP, 0]
    flags = om.classify(cnt, first, spans)
    assert flags[0].tolist() == [om.STOP, om.PARTIAL | om.STOP, om.FRAMESHIFT, 0]
    assert flags[1].tolist() == [0, om.PARTIAL | om.FRAMESHIFT, om.FRAMESHIFT, om.STOP]
    assert om.classify(cnt, first, spans, max_gap_cells=3)[0].tolist() == [om.STOP, om.PARTIAL | om.STOP | om.DELETION, om.FRAMESHIFT, 0]
    assert om.classify(cnt, first, spans, tail_codons=2)[0].tolist() == [0, om.PARTIAL, om.FRAMESHIFT, 0]      # codon 1 of 3 is in a tail of two
    assert om.classify(cnt, first, spans, tail_codons=1)[0].tolist() == [om.STOP, om.PARTIAL | om.STOP, om.FRAMESHIFT, 0]
    idx, flagged = om.keep(flags, om.STOP)
    assert idx.tolist() == [2] and flagged == 3
    idx, flagged = om.keep(flags, om.FRAMESHIFT)
    assert idx.tolist() == [0, 3] and flagged == 2
    assert [om.letters(f) for f in (0, 1, 2, 4, 8, 15, 6)] == ["-", "P", "S", "F", "D", "PSFD", "SF"]
    # a -1 and a -2 deletion in one span cancel: the NET frame
    row = np.full((1, 12), Cc, dtype=np.uint8)
    row[0, 2] = row[0, 6] = row[0, 7] = om.GAP
    c1, f1 = om.counters(row, [(0, 4)], np.full(12, Cc, dtype=np.uint8))
    assert c1[om.GAP_CELLS, 0, 0] == 3 and om.classify(c1, f1, [(0, 4)])[0, 0] == 0


# ---------------------------------------------------------------------------------------------- exports
def test_exports_and_layout():
    lib = capi.load_library()
    header = open(os.path.join(ROOT, "include", "juliet_hip.h")).read()
    declared = set(re.findall(r"\b(jl_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in NAMES:
        assert name in declared and name in capi.EXPORTS and name in exported and hasattr(lib, name), name
    assert exported == declared                # the library's dynamic symbols are exactly the header's
    assert lib.jl_abi_version() == 5           # additive: the ABI version stays
    assert re.search(r"enum \{ JL_ORF_COVERED = 0, JL_ORF_GAP_CELLS = 1, JL_ORF_CODONS_READ = 2, JL_ORF_STOPS = 3, JL_ORF_COUNTERS = 4 \};", header)
    assert re.search(r"enum \{ JL_ORF_PARTIAL = 1, JL_ORF_STOP = 2, JL_ORF_FRAMESHIFT = 4, JL_ORF_DELETION = 8 \};", header)
    assert "enum { JL_ORF_MAX_SPANS = 64 };" in header and "#define JL_ORF_NO_STOP 0xFFFFFFFFu" in header
    assert (capi.ORF_COVERED, capi.ORF_GAP_CELLS, capi.ORF_CODONS_READ, capi.ORF_STOPS, capi.ORF_COUNTERS) == (0, 1, 2, 3, 4)
    assert (om.COVERED, om.GAP_CELLS, om.CODONS_READ, om.STOPS) == (0, 1, 2, 3)
    assert (capi.ORF_PARTIAL, capi.ORF_STOP, capi.ORF_FRAMESHIFT, capi.ORF_DELETION) == (om.PARTIAL, om.STOP, om.FRAMESHIFT, om.DELETION) == (1, 2, 4, 8)
    assert capi.ORF_NO_STOP == om.NO_STOP and capi.ORF_MAX_SPANS == orf_shape.constants()["max_spans"] == 64
    assert capi.ORF_SPAN.itemsize == 8 and C.sizeof(capi.OrfRule) == 8
    assert hasattr(capi.Juliet, "read_orf") and hasattr(capi.Juliet, "read_orf_fetch")


# ---------------------------------------------------------------------------------------------- jl_orf_classify
def table(entries, n_spans=1):
    """counts[4, n_spans, n] and first[n_spans, n] from (covered, gaps, read, stops, first) tuples, the same in every span."""
    e = np.array(entries, dtype=np.uint64).T
    return np.repeat(e[:4, None, :], n_spans, axis=1).astype(np.uint32), np.repeat(e[4][None, :], n_spans, axis=0).astype(np.uint32)


def test_classify_every_flag_combination():
    """A span of 10 codons; one read for every combination of the four flags, under a rule with both bounds on."""
    n, K, tail = 10, 6, 2
    entries = []
    for partial, stop, shift, deletion in itertools.product((0, 1), repeat=4):
        gaps = (K if shift == 0 else K + 1) if deletion else (3 if shift == 0 else 2)
        covered = 3 * n - (5 if partial else 0)
        first = 4 if stop else om.NO_STOP
        entries.append((covered, gaps, 3, 1 if stop else 0, first))
    cnt, first = table(entries)
    spans = [(7, n)]
    flags = capi.orf_classify(cnt, first, spans, max_gap_cells=K, tail_codons=tail)
    assert flags.dtype == np.uint8 and flags.shape == (1, 16)
    assert (flags == om.classify(cnt, first, spans, K, tail)).all()
    assert flags[0].tolist() == [8 * d + 4 * s + 2 * st + p for p, st, s, d in itertools.product((0, 1), repeat=4)]
    assert sorted(flags[0].tolist()) == list(range(16))
    # the rule {0, 0}: no DELETION, no tail
    off = capi.orf_classify(cnt, first, spans)
    assert (off == om.classify(cnt, first, spans)).all() and not (off & om.DELETION).any() and ((off & 7) == (flags & 7)).all()


def test_classify_tail_rule_at_its_bound():
    n = 12
    for tail in (0, 1, 3, n - 1, n, n + 1, 2**32 - 1):
        body = n - min(tail, n)
        firsts = sorted({0, max(body - 1, 0), min(body, n - 1), n - 1})
        cnt, first = table([(3 * n, 0, n, 1, f) for f in firsts] + [(3 * n, 0, n, 0, om.NO_STOP)])
        flags = capi.orf_classify(cnt, first, [(0, n)], tail_codons=tail)
        assert (flags == om.classify(cnt, first, [(0, n)], tail_codons=tail)).all(), tail
        assert flags[0].tolist() == [om.STOP if f < body else 0 for f in firsts] + [0], tail
        if 0 < tail < n:      # first_stop = n - T - 1 is a stop, n - T is in the tail
            assert flags[0][firsts.index(n - tail - 1)] == om.STOP and flags[0][firsts.index(n - tail)] == 0
        if tail >= n:         # the whole span is tail
            assert not flags.any()


def test_classify_deletion_bound_and_net_frame():
    n, K = 20, 7
    cnt, first = table([(3 * n, g, 0, 0, om.NO_STOP) for g in (0, 1, 2, 3, K - 1, K, K + 1, 3 * n)])
    flags = capi.orf_classify(cnt, first, [(0, n)], max_gap_cells=K)
    assert (flags == om.classify(cnt, first, [(0, n)], max_gap_cells=K)).all()
    assert flags[0].tolist() == [0, 4, 4, 0, 0, 4 | 8, 4 | 8, 8]      # K - 1 = 6 gap cells: in frame, below the bound; K = 7: both
    several = capi.orf_classify(*table([(30, 2, 0, 0, om.NO_STOP), (29, 3, 1, 1, 9)], n_spans=3), [(0, 10), (5, 10), (1, 10)], tail_codons=1)
    assert several.tolist() == [[4, 1]] * 3                          # (a stop in the last codon with a tail of one: no STOP)


def test_classify_refusals():
    lib = capi.load_library()
    spans = capi.orf_spans([(0, 10)])
    cnt, first = table([(30, 3, 9, 1, 4), (12, 0, 4, 0, om.NO_STOP)])
    flags = np.full((1, 2), 77, dtype=np.uint8)
    rule = capi.OrfRule(0, 0)

    def call(c=cnt, f=first, s=spans, ns=1, n=2, r=C.byref(rule), out=flags):
        return lib.jl_orf_classify(*(x.ctypes.data if x is not None else None for x in (c, f, s)), ns, n, r, out.ctypes.data if out is not None else None)

    def refused(word, **kw):
        assert call(**kw) == -1
        assert word in lib.jl_last_error(None).decode(), lib.jl_last_error(None)
        assert flags.tolist() == [[77, 77]]                          # a refused call writes nothing

    for kw in (dict(c=None), dict(f=None), dict(s=None), dict(r=None), dict(out=None)):
        refused("NULL", **kw)
    refused("32 bits", n=2**32)
    refused("1 .. 64", ns=0)
    refused("1 .. 64", ns=65)
    for bad, word in (((31, 3, 9, 1, 4), "more covered cells"), ((30, 31, 9, 1, 4), "more gap cells"), ((30, 3, 1, 2, 4), "more stops"),
                      ((30, 3, 9, 1, 10), "first stop outside"), ((30, 3, 9, 1, 2**32 - 2), "first stop outside")):
        c2, f2 = table([(12, 0, 4, 0, om.NO_STOP), bad])             # the SECOND read contradicts its span: the first's flag is not written either
        refused(word, c=c2, f=f2)
    assert call() == 0 and flags.tolist() == [[om.STOP, om.PARTIAL]]
    with pytest.raises(capi.JulietError) as e:
        capi.orf_classify(*table([(31, 0, 0, 0, om.NO_STOP)]), [(0, 10)])
    assert e.value.status == -1


# ---------------------------------------------------------------------------------------------- jl_orf_filter
def test_filter_follows_the_mirror_for_every_mask():
    rng = np.random.default_rng(27)
    flags = rng.integers(0, 16, size=(5, 400), dtype=np.uint8)
    flags[:, rng.random(400) < 0.5] = 0
    flags[:, 7] = om.PARTIAL                                         # partial alone is no defect
    for mask in range(1, 16):
        if mask & om.PARTIAL:
            continue
        idx, flagged = capi.orf_filter(flags, mask)
        exp_idx, exp_flagged = om.keep(flags, mask)
        assert idx.dtype == np.uint32 and idx.tolist() == exp_idx.tolist() and flagged == exp_flagged and 7 in idx
        assert 0 < flagged < 400
    assert capi.orf_filter(np.zeros((3, 0), dtype=np.uint8))[0].tolist() == []
    idx, flagged = capi.orf_filter(np.array([[0, 2, 0], [4, 0, 0]], dtype=np.uint8))      # the default mask: stop, frameshift; any span
    assert idx.tolist() == [2] and flagged == 2


def test_filter_refusals():
    lib = capi.load_library()
    flags = np.array([[0, 2]], dtype=np.uint8)
    idx, kept, flagged = np.full(2, 77, dtype=np.uint32), C.c_uint64(99), C.c_uint64(98)

    def call(f=flags.ctypes.data, ns=1, n=2, mask=2, i=idx.ctypes.data, k=C.byref(kept), fl=C.byref(flagged)):
        return lib.jl_orf_filter(f, ns, n, mask, i, k, fl)

    def refused(word, **kw):
        assert call(**kw) == -1
        assert word in lib.jl_last_error(None).decode(), lib.jl_last_error(None)
        assert idx.tolist() == [77, 77] and kept.value == 99 and flagged.value == 98      # a refused call writes nothing

    for kw in (dict(f=None), dict(i=None), dict(k=None), dict(fl=None)):
        refused("NULL", **kw)
    for mask in (0, 1, 3, 16, 15, 2**31):
        refused("subset", mask=mask)
    refused("32 bits", n=2**32)
    refused("1 .. 64", ns=0)
    assert call() == 0 and kept.value == 1 and flagged.value == 1 and idx[0] == 0


# ---------------------------------------------------------------------------------------------- the launch shape
def test_shape_invariants():
    c = orf_shape.constants()
    assert c["seg_codons_max"] == 85 and 3 * c["seg_codons_max"] <= 255 and c["k"] in (4, 5, 6)
    rng = np.random.default_rng(3)
    cases = [([1], 1), ([85], 1), ([86], 5000), ([1000], 100000), ([333] * 15, 100000), ([1] * 64, 3), ([10**6], 2048 * 1025), ([7, 4000, 85, 86], 2048 * 40)]
    cases += [(rng.integers(1, 3000, size=int(rng.integers(1, 65))).tolist(), int(rng.integers(1, 3 * 10**6))) for _ in range(40)]
    for n_codons, n_reads in cases:
        for k in (0, 4, 5, 6):
            s = orf_shape.shape(n_codons, n_reads, k)
            assert s["wg_reads"] == 2048 and s["n_chunks"] == -(-n_reads // 2048)
            assert 1 <= s["seg_codons"] <= c["seg_codons_max"]
            assert s["k"] == (k or c["k"]) and 1 <= s["flush_codons"] and 3 * s["flush_codons"] <= 2 ** s["k"] - 1 < 3 * (s["flush_codons"] + 1)
            # the segments tile every span exactly: segment s of a span is the codons [s seg, min((s + 1) seg, n))
            for n, segs in zip(n_codons, s["span_segs"]):
                assert segs >= 1 and (segs - 1) * s["seg_codons"] < n <= segs * s["seg_codons"]
            assert s["n_segs"] == sum(s["span_segs"]) and s["grid"] == s["n_segs"] * s["n_chunks"]
    # a long span of few reads is cut into segments no shorter than the minimum; of many reads, into the longest
    assert orf_shape.shape([1000], 97)["seg_codons"] == c["seg_codons_min"]
    assert orf_shape.shape([1000], 2048 * 1025)["seg_codons"] == c["seg_codons_max"]


# ---------------------------------------------------------------------------------------------- the command line
def juliet(d, *args):
    return subprocess.run([JULIET, *args], cwd=d, capture_output=True, text=True, timeout=60)


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(JULIET):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "host")])


@pytest.mark.parametrize("args", [["--windows", "2"], ["--mix", "b.bam"], ["--devices", "0,0"], ["--consensus", "c.fasta"], ["--call-insertions"]])
def test_cli_refuses_what_the_hypermutation_filter_refuses(built, tmp_path, args):
    for flags in (["--drop-defective"], ["--orf-report", "r.tsv"], ["--drop-defective", "--defect-tail-codons", "2"]):
        r = juliet(tmp_path, *flags, *args, "no_such.bam", "o.json")
        assert r.returncode == 1 and ("--drop-defective" in r.stderr or "--orf-report" in r.stderr), (r.returncode, r.stderr)
        assert not list(tmp_path.iterdir())


def test_cli_refuses_bad_defect_options(built, tmp_path):
    (tmp_path / "l.tsv").write_text("no_such.bam\ta.json\n")
    r = juliet(tmp_path, "--orf-report", "r.tsv", "--batch", "l.tsv")
    assert r.returncode == 1 and "--batch" in r.stderr
    r = subprocess.run([os.path.join(ROOT, "minorseq_amd", "bin", "fuse"), "--drop-defective", "no_such.bam", "o.fasta"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "fuse" in r.stderr
    for opt in (["--defect-kinds", "stop"], ["--defect-max-deletion", "9"], ["--defect-tail-codons", "1"]):
        r = juliet(tmp_path, *opt, "no_such.bam", "o.json")          # a --defect-* option without --drop-defective
        assert r.returncode == 1 and "--drop-defective" in r.stderr, (opt, r.stderr)
        r = juliet(tmp_path, "--orf-report", "r.tsv", *opt, "no_such.bam", "o.json")
        assert r.returncode == 1 and "--drop-defective" in r.stderr, (opt, r.stderr)
    for kinds in ("stops", "stop,,frameshift", "", "stop,partial", "STOP"):
        r = juliet(tmp_path, "--drop-defective", "--defect-kinds", kinds, "no_such.bam", "o.json")
        assert r.returncode == 1 and "--defect-kinds" in r.stderr, (kinds, r.stderr)
    r = juliet(tmp_path, "--drop-defective", "--defect-kinds", "stop,deletion", "no_such.bam", "o.json")
    assert r.returncode == 1 and "--defect-max-deletion" in r.stderr
    for opt, bad in (("--defect-max-deletion", "0"), ("--defect-max-deletion", "-3"), ("--defect-max-deletion", "x"), ("--defect-tail-codons", "-1"), ("--defect-tail-codons", "1.5")):
        r = juliet(tmp_path, "--drop-defective", opt, bad, "no_such.bam", "o.json")
        assert r.returncode == 1 and opt in r.stderr, (opt, bad, r.stderr)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["l.tsv"]


def test_cli_accepted_options_reach_the_input(built, tmp_path):
    """Every well-formed choice of kinds passes the option check: the run ends at the missing input file (2), not at a refusal (1)."""
    for opt in (["--drop-defective"], ["--orf-report", "r.tsv"], ["--drop-defective", "--defect-kinds", "frameshift"],
                ["--drop-defective", "--defect-kinds", "deletion,stop", "--defect-max-deletion", "30", "--defect-tail-codons", "3"],
                ["--drop-defective", "--defect-max-deletion", "30"]):
        r = juliet(tmp_path, *opt, "no_such.bam", "o.json")
        assert r.returncode == 2, (opt, r.returncode, r.stderr)
    assert not list(tmp_path.iterdir())
