"""The host-only half of taking reads (docs/SPEC.md §12): which reads a downsample keeps (jl_sample_reads), how many reads
each clone gives to a mixture (jl_mix_counts, doc/MIXDATA.md:10-22), and what the command line refuses before any device call.
No GPU: the library only has to load."""
import os
import subprocess

import numpy as np
import pytest

from minorseq_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JULIET = os.path.join(ROOT, "minorseq_amd", "bin", "juliet")


@pytest.fixture(scope="module", autouse=True)
def built():
    """The front end links the library: build both only if they are missing."""
    if not os.path.exists(os.path.join(ROOT, "minorseq_amd", "libjuliet_hip.so")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "csrc")])
    if not os.path.exists(JULIET):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "host")])


def mirror_sample(n, k, seed):
    """The rule in numpy: key(i) = splitmix64(seed + i); the k smallest (key, i) — a stable argsort of the keys — in ascending i."""
    with np.errstate(over="ignore"):
        keys = synth.splitmix64(np.uint64(seed) + np.arange(n, dtype=np.uint64))
    return np.sort(np.argsort(keys, kind="stable")[:k]).astype(np.uint32)


@pytest.mark.parametrize("seed", [0, 7, 0xFFFFFFFFFFFFFFF0])   # (the last: seed + i wraps around 2^64)
@pytest.mark.parametrize("n,k", [(1, 1), (10, 3), (1000, 1000), (1000, 2000), (100003, 6000)])
def test_sample_reads_equals_the_numpy_mirror(n, k, seed):
    got = capi.sample_reads(n, k, seed)
    exp = mirror_sample(n, k, seed)
    assert got.dtype == np.uint32 and len(got) == min(n, k)
    assert (got == exp).all()
    assert (np.diff(got.astype(np.int64)) > 0).all()       # ascending, no read twice


def test_samples_of_one_seed_are_nested():
    small, large = capi.sample_reads(100003, 100, 5), capi.sample_reads(100003, 1000, 5)
    assert len(small) == 100 and len(large) == 1000
    assert np.isin(small, large).all()
    assert not np.isin(capi.sample_reads(100003, 100, 6), large).all()    # another seed, another sample


def test_sample_of_nothing():
    assert len(capi.sample_reads(1000, 0, 3)) == 0
    assert len(capi.sample_reads(0, 10, 3)) == 0
    with pytest.raises(capi.JulietError) as e:     # an index is 32 bits
        capi.sample_reads(1 << 32, 1, 0)
    assert e.value.status == -1


def test_mix_counts_of_the_documented_examples():
    # doc/MIXDATA.md: three clones at 3000x and 1 %, five clones at 6000x and 10 %
    assert capi.mix_counts(3, 3000, 1).tolist() == [2940, 30, 30]
    assert capi.mix_counts(5, 6000, 10).tolist() == [3600, 600, 600, 600, 600]
    assert capi.mix_counts(1, 500, 10).tolist() == [500]
    assert capi.mix_counts(2, 999, 0.15).tolist() == [998, 1]          # floor(1.4985), the rest to the major clone
    assert int(capi.mix_counts(16, 100000, 3.3).sum()) == 100000       # the total is the coverage exactly


@pytest.mark.parametrize("n_sources,coverage,perc", [
    (4, 3000, 40),           # three minors of 1200 reads exceed 3000
    (3, 3000, 0), (3, 3000, 100), (3, 3000, -1), (3, 3000, 150), (3, 3000, float("nan")),   # outside (0, 100)
    (0, 3000, 1),
])
def test_mix_counts_errors(n_sources, coverage, perc):
    with pytest.raises(capi.JulietError) as e:
        capi.mix_counts(n_sources, coverage, perc)
    assert e.value.status == -1


def juliet(cwd, *args):
    return subprocess.run([JULIET, *args], cwd=cwd, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args, words", [
    (["--downsample", "100", "--windows", "2"], ["--downsample", "--windows"]),
    (["--downsample", "100", "--consensus", "c.fasta"], ["--downsample", "--consensus"]),
    (["--downsample", "0"], ["--downsample", "at least one read"]),
    (["--mix", "b.bam", "--windows", "2"], ["--mix", "--windows"]),
    (["--mix", "b.bam", "--consensus", "c.fasta"], ["--mix", "--consensus"]),
    (["--mix", "b.bam", "--downsample", "0"], ["at least one read"]),
    (["--mix", "b.bam,c.bam", "--mix-perc", "60"], ["--mix-perc"]),
    (["--mix", "b.bam", "--mix-perc", "0"], ["--mix-perc"]),
])
def test_flag_combinations_the_command_line_refuses(tmp_path, args, words):
    """Exit 1 with a message, decided before any file is read or any device call is made: the BAMs need not exist."""
    r = juliet(tmp_path, *args, "a.bam", "o.json")
    assert r.returncode == 1, (r.returncode, r.stderr)
    for w in words:
        assert w in r.stderr, (w, r.stderr)
    assert not list(tmp_path.iterdir())


def test_mix_is_refused_with_batch(tmp_path):
    (tmp_path / "l.tsv").write_text("a.bam\ta.json\n")
    r = juliet(tmp_path, "--mix", "b.bam", "--batch", "l.tsv")
    assert r.returncode == 1 and "--mix" in r.stderr and "--batch" in r.stderr


def test_help_mentions_the_flags():
    r = subprocess.run([JULIET, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for w in ("--downsample", "--sample-seed", "--mix", "--mix-perc"):
        assert w in r.stderr
