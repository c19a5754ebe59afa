"""Seeded mutation fuzz of the BAM front end's record parser under AddressSanitizer + UBSan (tests/cpp/bam_fuzz.cpp): a stand-alone
program, built with g++, that links nothing of HIP.  Four seed files — a plain and a rich-QV one from juliet-synth, the variety sample
and a small file of cigar shapes and 'traps' from tests/bam_py.py — are mutated field by field in the inflated stream (wrapped into
BGZF again with correct CRCs, so that the record parser is reached) and in the compressed bytes; both readers run on every case in one
process.  A signal or a sanitizer report aborts the program; it fails a case itself when one reader accepts what the other refuses,
when the hand-overs differ, when a record is handed over that the device would have to refuse, or (stream mutations) when the refusal
messages differ.  CPU only."""
import os
import subprocess

import pytest

import bam_diff
import bam_py

ROOT = bam_diff.ROOT
SYNTH = os.path.join(ROOT, "minorseq_amd", "bin", "juliet-synth")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g"]
SEED, CASES = 20261020, 2000
CLASSES = ["block_size", "l_read_name", "n_cigar", "l_seq", "cigar_word", "aux_type", "b_count", "ref_id", "pos", "flag", "hdr_l_text",
           "hdr_n_ref", "hdr_l_name", "truncation", "byte_flip", "bgzf_header", "bgzf_bsize", "bgzf_isize", "bgzf_crc", "bgzf_payload"]
# classes for which a mutated file can still be a valid one: another flag, position or reference, a cigar word that keeps the query
# length, a flipped bit in a name or a quality, a cut at a record boundary, a gzip header field nobody reads, an aux type of the
# same size.  The list stops at the classes whose mutation ranges AIM at a valid outcome.  Other classes accept now and then by luck —
# a length nudged by 0, a record that is dropped anyway, a flipped payload bit that moves a byte nobody reads (bgzf_payload: 16 of 1000
# in the long pass) — and a count that depends on luck is not required.
MUST_ACCEPT = ["ref_id", "pos", "flag", "cigar_word", "byte_flip", "truncation", "aux_type", "bgzf_header"]


def trap_records():
    """Cigar shapes on two references, and 'traps': records that are dropped as they stand (unmapped, no position, no reference) and
    carry an M op or the wrong number of bases, so that a mutation of flag, pos or ref_id that makes them kept must end in a refusal."""
    def r(name, pos=5, cigar=(("=", 6),), seq="ACGTAC", flag=0, ref_id=0, tags=(("rq", "f", 0.99),)):
        return dict(ref_id=ref_id, pos=pos, flag=flag, mapq=9, name=name, cigar=list(cigar), seq=seq, qual=bytes([30, 10, 25, 19, 20, 40][:len(seq)]),
                    tags=list(tags))
    m = (("=", 2), ("M", 4))
    return [r("trap ref a", ref_id=-1, cigar=m), r("ok 1", tags=[("rq", "f", 0.99), ("XB", "B", ("s", [1, -2, 3])), ("sq", "Z", "5I!5I5")]),
            r("trap flag a", flag=0x4, cigar=m), r("trap pos a", pos=-1, cigar=m), r("other", ref_id=1),
            r("ok 2", 7, [("H", 2), ("S", 1), ("=", 2), ("I", 1), ("D", 2), ("X", 1), ("N", 30), ("P", 1), ("=", 1)], "ACGTAC"),
            r("trap flag b", flag=0x100, cigar=[("=", 9)]), r("trap pos b", pos=-1, cigar=[("=", 2)]), r("trap ref b", ref_id=-1, cigar=m),
            r("ok 3", 0, [("=", 1), (11, 7), ("X", 1)], "AC", tags=[("Xi", "i", -5), ("rq", "f", 0.999), ("XC", "B", ("C", [7] * 5)), ("dq", "Z", "II")]),
            r("trap flag c", flag=0x904, cigar=m), r("trap ref c", ref_id=-1, cigar=[("I", 1)])]


@pytest.fixture(scope="module")
def fuzz(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_fuzz")
    if not os.path.exists(SYNTH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "csrc")])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "host")])
    exe = str(d / "bam_fuzz")
    subprocess.check_call(["g++", "-std=c++17", *SAN, *bam_diff.INCLUDES, "-o", exe, os.path.join(ROOT, "tests", "cpp", "bam_fuzz.cpp"), "-lz", "-lpthread"])
    seeds = [str(d / x) for x in ("plain.bam", "rich.bam", "variety.bam", "traps.bam")]
    subprocess.check_call([SYNTH, "--reads", "30", "--cols", "150", "--seed", "7", "--partial", "0.3", "-o", seeds[0]])
    subprocess.check_call([SYNTH, "--reads", "30", "--cols", "150", "--seed", "8", "--rich-qv", "-o", seeds[1]])
    bam_py.write_bam(seeds[2], "@HD\tVN:1.5\n", bam_diff.VARIETY_REFS, bam_diff.variety_records(40, seed=3))
    bam_py.write_bam(seeds[3], "", [("a", 700), ("b", 800)], trap_records())
    return exe, seeds, d


def run_fuzz(fuzz, seed, cases):
    exe, seeds, d = fuzz
    env = {k: v for k, v in os.environ.items() if k not in ("JL_BGZF_THREADS", "JL_DECODE_THREADS")}
    r = subprocess.run([exe, str(seed), str(cases), str(d), *seeds], capture_output=True, text=True, timeout=1500, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    table = {w[0]: (int(w[1]), int(w[2])) for w in (line.split() for line in r.stdout.strip().splitlines())}
    return table, r.stdout


def test_mutated_files_never_split_the_readers(fuzz):
    """2000 cases, fixed seed, every class in turn.  Every class has at least one refused case, and every class for which a valid
    outcome exists at least one accepted case: a fuzz that bounces off the magic check cannot pass."""
    table, text = run_fuzz(fuzz, SEED, CASES)
    assert sorted(table) == sorted(CLASSES), text
    assert sum(a + r for a, r in table.values()) == CASES, text
    for c in CLASSES:
        assert table[c][1] >= 1, "no refused case of class %s\n%s" % (c, text)
    for c in MUST_ACCEPT:
        assert table[c][0] >= 1, "no accepted case of class %s\n%s" % (c, text)
