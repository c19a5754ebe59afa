"""The BAM front end (minorseq_amd/host/bam.hpp, bgzf.hpp, decode.hpp, msa_builder.hpp) against files that its own writer never
touched: every case is written by tests/bam_py.py (plain Python, from the SAM specification), read by both readers through
tests/cpp/records_dump.cpp — which also checks on every record what the device takes on trust — and compared for equality with arrays
computed in Python from the record list (tests/bam_diff.py).  Then `juliet --dump-msa` of the same file against
tests/records_expand.py on those arrays, cell by cell.  CPU only."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bam_diff
import bam_py
import records_expand

ROOT = bam_diff.ROOT
JULIET = os.path.join(ROOT, "minorseq_amd", "bin", "juliet")
REFS = [("ref one", 2000), ("ref two", 3000), ("ref three", 4000)]
TEXT = "@HD\tVN:1.5\tSO:coordinate\n@SQ\tSN:ref one\tLN:2000\n"
READERS = (("seq", 1, 8192), ("seq", 1, 3), ("pipe", 1, 8192), ("pipe", 4, 8192))


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "csrc")])
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "host")])
    return bam_diff.build_records_dump(tmp_path_factory.mktemp("records_dump"))


def rec(pos=10, cigar=(("=", 4),), seq="ACGT", qual=None, tags=(), name="r", flag=0, ref_id=0, mapq=30):
    return dict(ref_id=ref_id, pos=pos, flag=flag, mapq=mapq, name=name, cigar=list(cigar), seq=seq, qual=qual, tags=list(tags))


def both(dump, path, **kw):
    """[(status, message, sections)] of the two readers: sequential (whole and in chunks of 3), pipelined on 1 and 4 threads."""
    out = [bam_diff.run_dump(dump, path, path + ".bin", reader=r, threads=t, chunk_reads=c, **kw) for r, t, c in READERS]
    assert len({o[0] for o in out}) == 1 and len({o[1] for o in out}) == 1, [o[:2] for o in out]
    return out


def msa_of(path, *flags):
    r = subprocess.run([JULIET, *flags, "--dump-msa", path + ".msa", path], capture_output=True, text=True, timeout=120)
    if r.returncode != 0:
        return r, None, None
    raw = open(path + ".msa", "rb").read()
    n, l, wb = (int(x) for x in np.frombuffer(raw[:24], dtype=np.uint64))
    return r, np.frombuffer(raw[24:], dtype=np.uint8).reshape(n, l), wb


def check(dump, tmp_path, records, refs=REFS, text=TEXT, min_qv=0, min_rq=0.0, ref=-1, msa=True, name="c.bam", region="1-700", **bgzf):
    """Writes `records`, requires both readers to hand over exactly the expected arrays in every form, then the host expansion."""
    path = str(tmp_path / name)
    bam_py.write_bam(path, text, refs, records, **bgzf)
    for form in ("none", "bytes", "mask"):
        exp = bam_diff.expected(records, ref, min_qv, min_rq, form)
        for status, msg, got in both(dump, path, min_qv=min_qv, min_rq=min_rq, form=form, ref=ref):
            assert status == 0, msg
            bam_diff.assert_same(got, exp, form)
            assert got["refs"] == [(n, l) for n, l in refs] and got["text"] == text
    if msa and ref < 0:
        exp = bam_diff.expected(records, ref, min_qv, min_rq, "bytes")
        flags = ["-r", region] + (["--min-qv", str(min_qv)] if min_qv else []) + (["--min-rq", repr(min_rq)] if min_rq else [])
        r, rows, wb = msa_of(path, *flags)
        assert r.returncode == 0, r.stderr
        want = records_expand.expand(exp, rows.shape[1], wb, min_qv)
        assert rows.shape == want.shape and (rows == want).all(), np.argwhere(rows != want)[:8]
        assert (want != 6).any()
    return path


def refused(dump, tmp_path, raw=None, records=None, refs=REFS, text=TEXT, expect="", cli=True, name="bad.bam", data=None, **kw):
    """Both readers end with exit 2 and the same message (which holds `expect`); so does the command line."""
    path = str(tmp_path / name)
    if data is None:
        if raw is None:
            raw = bam_py.bam_stream(text, refs, records)[0]
        data = bam_py.bgzf_wrap(raw)
    open(path, "wb").write(data)
    out = both(dump, path, **kw)
    assert out[0][0] == 2 and expect in out[0][1], out[0][:2]
    if cli:
        r, _, _ = msa_of(path)
        assert r.returncode == 2 and expect in r.stderr, r.stderr
    return out[0][1]


# ---------------------------------------------------------------------------------------------- sequence and name lengths
def test_sequence_and_name_lengths(dump, tmp_path):
    """l_seq 1, 2, odd, even (the last nibble of an odd read is the HIGH one of its byte), a mapped record with `*` and no cigar, a name
    that is the NUL alone and one of 254 characters: the packed bases, offsets and names of both readers, and the expanded rows."""
    records = [rec(5, [("=", 1)], "G", bytes([9])), rec(6, [("X", 2)], "TC"), rec(7, [("=", 7)], "ACGTTGC", bytes(range(7))),
               rec(8, [("=", 8)], "TGCATGCA"), rec(9, [], "*"), rec(11, [("=", 3)], "CAT", name=""), rec(12, [("=", 5)], "GATTA", name="x" * 254)]
    check(dump, tmp_path, records, min_qv=5)
    got = bam_diff.run_dump(dump, str(tmp_path / "c.bam"), str(tmp_path / "o.bin"))[2]
    assert list(np.diff(got["seq_off"])) == [1, 1, 4, 4, 0, 2, 3] and got["names"][5] == "" and len(got["names"][6]) == 254
    assert got["seq4"][0] == 0x40 and got["seq4"][5] == 0x20        # G- ; the seventh base C in the high nibble


# ---------------------------------------------------------------------------------------------- flags and references
def test_flags_and_references(dump, tmp_path):
    """0x4 and 0x100 are dropped, 0x800, 0x10 and 0x400 kept; ref_id -1 and pos -1 dropped; of three interleaved references the first
    KEPT record decides (the file begins with dropped records of the others), and asking for another reference reads that one."""
    records = [rec(1, ref_id=2, flag=0x4), rec(2, ref_id=1, flag=0x100), rec(3, ref_id=-1), rec(-1, ref_id=2),
               rec(20, ref_id=1, name="first kept"), rec(21, ref_id=0), rec(22, ref_id=1, flag=0x800), rec(23, ref_id=2),
               rec(24, ref_id=1, flag=0x10), rec(25, ref_id=1, flag=0x400), rec(26, ref_id=1, flag=0x900), rec(27, ref_id=1, flag=0x14),
               rec(28, ref_id=0, flag=0x800), rec(29, ref_id=2, flag=0x10)]
    check(dump, tmp_path, records)
    exp = bam_diff.expected(records)
    assert exp["extent"][3] == 1 and list(exp["pos"]) == [20, 22, 24, 25]
    for ref, want in ((0, [21, 28]), (2, [23, 29])):
        check(dump, tmp_path, records, ref=ref)
        assert list(bam_diff.expected(records, ref)["pos"]) == want


def test_every_record_dropped_is_no_alignments(dump, tmp_path):
    """A file whose every record is dropped: both readers hand over nothing, the command line says so and exits 2."""
    records = [rec(1, flag=0x4), rec(2, flag=0x100), rec(3, ref_id=-1), rec(-1)]
    path = str(tmp_path / "none.bam")
    bam_py.write_bam(path, TEXT, REFS, records)
    for status, msg, got in both(dump, path):
        assert status == 0 and len(got["pos"]) == 0 and list(got["extent"][[0, 2, 3]]) == [0, 0, -1]
    r, _, _ = msa_of(path)
    assert r.returncode == 2 and "no primary or supplementary alignments" in r.stderr
    bam_py.write_bam(path, TEXT, REFS, [])                        # and a file of the header alone
    for status, msg, got in both(dump, path):
        assert status == 0 and len(got["pos"]) == 0
    assert msa_of(path)[0].returncode == 2


def test_rq_filter(dump, tmp_path):
    """--min-rq drops a read whose rq (type f) is below it; a read without rq, with a negative rq, or whose rq has another type (here
    an integer and a string) is kept; the first record the filter keeps decides the reference."""
    records = [rec(5, ref_id=1, tags=[("rq", "f", 0.5)]), rec(6, tags=[("rq", "f", 0.999)]), rec(7, tags=[("rq", "f", 0.98)]), rec(8),
               rec(9, tags=[("rq", "f", -1.0)]), rec(10, tags=[("rq", "i", 0)]), rec(11, tags=[("rq", "Z", "0.1")]),
               rec(12, tags=[("XX", "i", 5), ("rq", "f", 0.9899), ("YY", "Z", "t")]), rec(13, tags=[("rq", "f", 0.99)])]
    check(dump, tmp_path, records, min_rq=0.99)
    assert list(bam_diff.expected(records, min_rq=0.99)["pos"]) == [6, 8, 9, 10, 11, 13]
    check(dump, tmp_path, records)                                 # without the filter the first record's reference is read
    assert list(bam_diff.expected(records)["pos"]) == [5]


# ---------------------------------------------------------------------------------------------- cigars
def test_every_cigar_op(dump, tmp_path):
    """= X I D S H N P, zero-length ops between and at the ends, H then S in front, P in the middle, N over many columns, and the
    undefined op codes 9..15, which consume neither bases nor columns in the host expansion, in records_expand and (section 5 of the
    GPU suite) on the device: pinned as accepted."""
    records = [
        rec(10, [("H", 3), ("S", 2), ("=", 3), ("X", 1), ("I", 2), ("=", 2), ("D", 3), ("=", 1), ("P", 2), ("=", 2), ("N", 400), ("X", 2), ("S", 1), ("H", 9)],
            "AACGTTTGCAGTCAT"[:16] + "A", bytes(range(16))),
        rec(20, [("=", 0), ("S", 0), ("=", 3), ("D", 0), ("I", 0), ("N", 0), ("X", 2), ("P", 0), ("H", 0), ("X", 0)], "ACGTA"),
        rec(30, [(9, 7), ("=", 2), (10, 0), (11, 1), (12, 100000), ("D", 1), (13, 5), (14, 5), ("=", 2), (15, 0xFFFFFFF)], "ACGT"),
        rec(0, [("N", 1500), ("=", 4)], "TTGA"),
        rec(40, [("D", 2), ("=", 3), ("D", 2)], "CCC"),
    ]
    assert sum(ln for op, ln in records[0]["cigar"] if op in "=XIS") == 16
    check(dump, tmp_path, records, min_qv=8, region="1-1600")


def test_cigar_of_65535_ops(dump, tmp_path):
    """n_cigar is a 16-bit field: its largest value, alternating = and D of one base."""
    ops = [("=", 1) if k % 2 == 0 else ("D", 1) for k in range(65535)]
    r = rec(0, ops, "ACGT" * 8192)
    check(dump, tmp_path, [r, rec(5)], refs=[("long", 70000)], region="1-66000")


def test_reference_span_limit(dump, tmp_path):
    """A read may span 2^30 - 1 reference bases (the device keeps a window column in 30 bits: cigar_rules.h).  One base more, and a
    cigar whose 32-bit sum of spans wraps to a small number, end in exit 2 with a message from both readers before any extent is
    formed; the largest span that is allowed comes through with its true extent.  (Before the fix the sum was 32 bits wide: the wrapped
    cigar was accepted with max_end = pos + 4.)"""
    m = (1 << 28) - 1
    ok = rec(7, [("=", 2), ("N", m), ("N", m), ("N", m), ("N", m), ("=", 1)], "ACG")          # 2^30 - 1
    path = str(tmp_path / "ok.bam")
    bam_py.write_bam(path, TEXT, REFS, [ok])
    for status, msg, got in both(dump, path):
        assert status == 0 and list(got["extent"]) == [1, 7, 7 + (1 << 30) - 1, 0]
    at = rec(7, [("=", 2), ("N", m), ("N", m), ("N", m), ("N", m), ("=", 2)], "ACGT", name="reaches")
    msg = refused(dump, tmp_path, records=[rec(1), at], expect="cigar spans 1073741824 reference bases")
    assert "read reaches" in msg
    wraps = rec(7, [("N", m)] * 16 + [("N", 16), ("=", 4)], "ACGT", name="wraps")               # 2^32 + 4
    msg = refused(dump, tmp_path, records=[rec(1), wraps], expect="cigar spans 4294967300 reference bases")
    assert "read wraps" in msg


def test_m_and_query_length_are_refused(dump, tmp_path):
    """An M op; a cigar that consumes more bases than l_seq, and fewer: each exit 2, the same message from both readers, naming the read."""
    assert "read em" in refused(dump, tmp_path, records=[rec(), rec(5, [("=", 2), ("M", 2)], name="em")], expect="cigar M is forbidden")
    refused(dump, tmp_path, records=[rec(5, [("=", 5)], "ACGT", name="more")], expect="read more: cigar consumes 5 bases, the record holds 4")
    refused(dump, tmp_path, records=[rec(5, [("=", 2), ("S", 1)], "ACGT", name="fewer")], expect="read fewer: cigar consumes 3 bases, the record holds 4")
    refused(dump, tmp_path, records=[rec(5, [], "ACGT", name="nocigar")], expect="cigar consumes 0 bases, the record holds 4")
    # a dropped record is not looked at that far: M in an unmapped read passes
    check(dump, tmp_path, [rec(), rec(5, [("M", 4)], flag=0x4)])


# ---------------------------------------------------------------------------------------------- aux
def test_aux_types_and_tracks(dump, tmp_path):
    """Every aux type (B arrays of every subtype, one of them empty) before, between and after rq / dq / iq / sq; a Z tag named xq that is
    no track; tracks shorter and longer than l_seq, and absent; QUAL all 0xFF with tracks present; characters below '!' (they wrap to
    large values); a track tag of type H or B, which is no track."""
    e = bam_diff._EVERY_TAG
    t8 = "".join(chr(33 + v) for v in (30, 5, 19, 20, 21, 60, 0, 93))
    records = [
        rec(10, [("=", 8)], "ACGTACGT", bytes([40] * 8), e[:6] + [("rq", "f", 0.999)] + e[6:11] + [("dq", "Z", t8)] + e[11:14] + [("iq", "Z", t8[::-1]), ("sq", "Z", "I" * 8)] + e[14:]),
        rec(11, [("=", 8)], "ACGTACGT", None, [("xq", "Z", "!!!!!!!!"), ("sq", "Z", t8)]),
        rec(12, [("=", 8)], "ACGTACGT", bytes([25] * 8), [("dq", "Z", "+++"), ("iq", "Z", "4" * 30), ("sq", "Z", "")]),
        rec(13, [("=", 8)], "ACGTACGT", bytes([25, 10] * 4), []),
        rec(14, [("=", 8)], "ACGTACGT", bytes([25] * 8), [("dq", "Z", " \x1f" + "5" * 6)]),
        rec(15, [("=", 8)], "ACGTACGT", bytes([25] * 8), [("dq", "H", "00"), ("iq", "B", ("C", [1] * 8)), ("sq", "A", "!")]),
        rec(16, [("=", 3)], "ACG", bytes([25] * 3), [("sq", "Z", "5!5")]),
    ]
    check(dump, tmp_path, records, min_qv=20, min_rq=0.5)
    q = bam_diff.expected(records, min_qv=20, form="bytes")["qual"]
    assert list(q[:8]) == [30, 0, 19, 20, 20, 19, 0, 30] and list(q[8:16]) == [30, 5, 19, 20, 21, 60, 0, 93] and list(q[16:24]) == [10, 10, 10] + [19] * 5


def test_aux_that_ends_at_or_beyond_the_record(dump, tmp_path):
    """With a filter that reads tags: a Z without its NUL at the record's end is refused (pinned); a B array whose count ends exactly
    at the record's end is fine, one byte beyond is refused; so are a B without its count and an unknown type; fewer than three stray
    bytes are ignored.  Both readers, the same message.  Without a filter nobody reads the tags and the same records pass."""
    base = rec(10, [("=", 4)], "ACGT", bytes([30] * 4), [("rq", "f", 0.9)])

    def with_tail(tail):
        body = bam_py.pack_record(base, with_size=False) + tail
        return struct.pack("<i", len(body)) + body

    head = bam_py.pack_header(TEXT, REFS)
    exp = bam_diff.expected([base], min_qv=20, form="bytes")
    for tail, ok in ((b"XZZno nul", False), (b"sqZ5!5", False), (b"XZZnul\0", True), (b"XBBs" + struct.pack("<Ihh", 2, 1, 2), True), (b"XBBs" + struct.pack("<Ih", 2, 1) + b"\1", False),
                     (b"XBB", False), (b"XYq", False), (b"XY", True)):
        path = str(tmp_path / "tail.bam")
        open(path, "wb").write(bam_py.bgzf_wrap(head + with_tail(tail)))
        out = both(dump, path, min_qv=20, form="bytes")
        assert (out[0][0] == 0) == ok and out[0][0] in (0, 2), (tail, out[0][:2])
        if ok:
            bam_diff.assert_same(out[0][2], exp)
        if not ok:
            assert "BAM aux" in out[0][1]
            assert msa_of(path, "--min-qv", "20")[0].returncode == 2
        assert both(dump, path)[0][0] == 0

# ---------------------------------------------------------------------------------------------- BGZF
def _variety():
    return bam_diff.variety_records(120, seed=5)


@pytest.mark.parametrize("split", [1, 2, 3])
def test_block_size_word_straddles_two_blocks(dump, tmp_path, split):
    """The four bytes of a record's block_size word split 1+3, 2+2 and 3+1 over two BGZF blocks — at the first record (the header's
    last block) and at every fifth one."""
    records = _variety()
    raw, at = bam_py.bam_stream(TEXT, bam_diff.VARIETY_REFS, records)
    check(dump, tmp_path, records, refs=bam_diff.VARIETY_REFS, min_qv=20, cuts=[a + split for a in at[::5]])


@pytest.mark.parametrize("knobs", [dict(block=1, level=1), dict(block=7, level=0), dict(block=300, empty_at=(0, 1, 5, 6, 40)),
                                   dict(block=65536, level=9), dict(block=0xff00, level=0), dict(eof=False), dict(block=97, eof=False, level=0)],
                         ids=["one-byte", "stored-7", "empty-blocks", "65536", "stored-max", "no-eof", "no-eof-97"])
def test_bgzf_shapes(dump, tmp_path, knobs):
    """One-byte blocks, stored blocks (level 0), empty blocks at the start, in the middle and next to each other, a block of 65536 bytes
    (the largest ISIZE), and a file without the EOF block, which the specification asks writers for but both readers accept (pinned)."""
    if knobs.get("block") == 65536:
        records = [rec(k, [("=", 3000)], "ACGT" * 750, bytes([40]) * 3000, name="r%d" % k) for k in range(60)]
        raw = bam_py.bam_stream(TEXT, REFS, records)[0]
        assert len(raw) > 2 * 65536
        check(dump, tmp_path, records, region="1-1500", **knobs)
    else:
        n = 12 if knobs.get("block") == 1 else 120
        check(dump, tmp_path, _variety()[:n], refs=bam_diff.VARIETY_REFS, min_qv=20, **knobs)


def test_bgzf_extra_subfield(dump, tmp_path):
    """Another subfield beside BC in a member's extra field, which the specification allows.  Pinned (docs/SPEC.md, input): when the
    FIRST member carries one, the file is not taken for BGZF and is read correctly as a plain series of gzip members, by the sequential
    reader, which the product then uses on every path; when only a LATER member carries one, both readers refuse the file with the same
    message."""
    records = _variety()[:40]
    extra = struct.pack("<BBH", ord("X"), ord("Y"), 3) + b"abc"
    check(dump, tmp_path, records, refs=bam_diff.VARIETY_REFS, min_qv=20, block=500, extra=extra)
    raw = bam_py.bam_stream(TEXT, bam_diff.VARIETY_REFS, records)[0]
    refused(dump, tmp_path, data=bam_py.bgzf_wrap(raw, block=500, extra=extra, extra_on=(3,)), expect="corrupt BGZF block header")


# ---------------------------------------------------------------------------------------------- header
def test_header_shapes(dump, tmp_path):
    """l_text 0; text without a NUL and with one (handed on as stored); n_ref 0 (every record is then without a reference the window
    could be clipped to, and still read); a reference name of 200 bytes."""
    check(dump, tmp_path, [rec()], text="")
    check(dump, tmp_path, [rec()], text="@CO\tno nul")
    path = str(tmp_path / "nul.bam")
    bam_py.write_bam(path, "@CO\tnul", REFS, [rec()], text_nul=True)
    assert all(o[2]["text"] == "@CO\tnul\0" for o in both(dump, path))
    check(dump, tmp_path, [rec()], refs=[], msa=False)
    check(dump, tmp_path, [rec(ref_id=1)], refs=[("a", 10), ("n" * 199, 900)])


def test_negative_header_lengths_are_refused(dump, tmp_path):
    """l_text, n_ref and l_name below zero: exit 2 with the same message from both readers (before the fix the sequential reader sized a
    string by the negative length, and ignored whether the bytes of the text and of the names arrived at all).  And a header cut short
    at every field: 'truncated BAM header' from both."""
    raw = bam_py.bam_stream(TEXT, REFS, [rec()])[0]
    o_nref = 8 + len(TEXT)
    for at in (4, o_nref, o_nref + 4):
        for v in (-1, -(1 << 31), -70000):
            m = bytearray(raw)
            struct.pack_into("<i", m, at, v)
            assert refused(dump, tmp_path, raw=bytes(m), expect="corrupt BAM header") == "records_dump: corrupt BAM header"
    for at, v in ((4, 1 << 30), (o_nref, 1 << 30), (o_nref + 4, 0x7FFFFFFF)):      # lengths far beyond the file
        m = bytearray(raw)
        struct.pack_into("<i", m, at, v)
        refused(dump, tmp_path, raw=bytes(m), expect="truncated BAM header")
    hdr = len(bam_py.pack_header(TEXT, REFS))
    for cut in (1, 3, 4, 6, 8, 20, o_nref + 2, o_nref + 6, o_nref + 12, hdr - 1):
        refused(dump, tmp_path, raw=raw[:cut], expect="truncated BAM header")
    refused(dump, tmp_path, raw=b"BAM\2" + raw[4:], expect="not a BAM file")
    refused(dump, tmp_path, raw=b"BAX", expect="truncated BAM header")
    for cut in (hdr + 1, hdr + 3, hdr + 4, hdr + 20, len(raw) - 1):             # and inside the record
        refused(dump, tmp_path, raw=raw[:cut], expect="truncated BAM record")
    for v in (-1, 0, 31, -(1 << 31)):                                            # block_size is a signed word
        m = bytearray(raw)
        struct.pack_into("<i", m, hdr, v)
        refused(dump, tmp_path, raw=bytes(m), expect="corrupt BAM record")
    m = bytearray(raw)
    struct.pack_into("<i", m, hdr, 0x7FFFFFFF)
    refused(dump, tmp_path, raw=bytes(m), expect="truncated BAM record")


def test_dropped_records_are_checked_alike(dump, tmp_path):
    """A record that overruns its block in front of the first kept record: the sequential reader checks every record's layout before
    it looks at the flags; the pipelined one skipped the records of a segment without a kept record (fixed: both refuse)."""
    raw, at = bam_py.bam_stream(TEXT, REFS, [rec(flag=0x4), rec()])
    m = bytearray(raw)
    struct.pack_into("<I", m, at[0] + 4 + 16, 100000)       # l_seq of the dropped record
    for block in (0xff00, at[1] - 1, at[1]):
        refused(dump, tmp_path, data=bam_py.bgzf_wrap(bytes(m), cuts=[block]), expect="corrupt BAM record")


# ---------------------------------------------------------------------------------------------- the variety sample
def test_variety_sample(dump, tmp_path):
    """The sample of the GPU ingest test (tests/test_gpu_bam_independent.py), on the CPU: both readers, every form, the host expansion."""
    records = bam_diff.variety_records()
    assert len(records) <= 300
    check(dump, tmp_path, records, refs=bam_diff.VARIETY_REFS, min_qv=bam_diff.VARIETY_MIN_QV, min_rq=0.95, block=4000)
    exp = bam_diff.expected(records, min_qv=20, min_rq=0.95, form="bytes")
    assert exp["extent"][3] == 0 and exp["extent"][0] > 150 and ((exp["cigar"] & 15) >= 9).any()
    assert (exp["qual"] < 20).any() and (exp["qual"] == 0xFF).any() and (np.diff(exp["seq_off"]) == 0).any()
