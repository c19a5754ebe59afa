"""The host side of the mask form of the record ingest (include/juliet_hip.h): jl_qmask_from_quals against its numpy statement,
and the front end's decoder, which emits a chunk's mask from the folded effective qualities (tests/cpp/qmask_decode_check.cpp)."""
import os
import subprocess

import numpy as np
import pytest

from minorseq_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYNTH = os.path.join(ROOT, "minorseq_amd", "bin", "juliet-synth")


def np_mask(seq_off, qual, qual_off, min_qv):
    so, qo = seq_off.astype(np.int64), qual_off.astype(np.int64)
    bits = np.zeros(8 * ((int(so[-1] - so[0]) + 3) // 4), dtype=np.uint8)
    t = min(min_qv, 127)
    for r in range(len(so) - 1):
        for q in range(int(qo[r + 1] - qo[r])):
            v = int(qual[qo[r] + q])
            if v < t and v != 0xFF:
                bits[2 * (so[r] - so[0]) + q] = 1
    return np.packbits(bits, bitorder="little")


def random_reads(rng, min_qv, first_seq=0, first_qual=0):
    lens = [0, 1, 3, 2, 17, 0, 33, 64, 5] + [int(x) for x in rng.integers(0, 70, 40)]
    values = np.array([0, max(min_qv, 1) - 1, min(min_qv, 254), 93, 0xFF, 19, 20, 126, 127, 128, 200], dtype=np.uint8)
    seq_off, qual_off = [first_seq], [first_qual]
    for n in lens:
        seq_off.append(seq_off[-1] + (n + 1) // 2)
        qual_off.append(qual_off[-1] + n)
    qual = values[rng.integers(0, len(values), qual_off[-1])]
    return np.array(seq_off, dtype=np.uint64), qual, np.array(qual_off, dtype=np.uint64)


@pytest.mark.parametrize("min_qv", [0, 20, 127, 200])
@pytest.mark.parametrize("first", [(0, 0), (13, 29)])
def test_qmask_from_quals_equals_numpy(min_qv, first):
    rng = np.random.default_rng(min_qv + first[0])
    seq_off, qual, qual_off = random_reads(rng, min_qv, *first)
    got = capi.qmask_from_quals(seq_off, qual, qual_off, min_qv)
    exp = np_mask(seq_off, qual, qual_off, min_qv)
    lib = capi.load_library()
    assert len(got) == lib.jl_qmask_bytes(int(seq_off[-1] - seq_off[0])) == (int(seq_off[-1] - seq_off[0]) + 3) // 4
    assert (got == exp).all()                  # every bit: the spare bits of odd reads and behind the last read are clear
    if min_qv == 0:
        assert not got.any()
    else:
        assert got.any()
        clamped = capi.qmask_from_quals(seq_off, qual, qual_off, min(min_qv, 127))
        assert (clamped == got).all()          # 200 is taken as 127
    # a buffer that is too small is refused, a larger one is cleared to its end
    small = np.zeros(max(len(got) - 1, 0), dtype=np.uint8)
    assert lib.jl_qmask_from_quals(len(seq_off) - 1, capi._p(seq_off), capi._p(qual), capi._p(qual_off), min_qv, capi._p(small), len(small)) == -1
    big = np.full(len(got) + 5, 0xFF, dtype=np.uint8)
    assert lib.jl_qmask_from_quals(len(seq_off) - 1, capi._p(seq_off), capi._p(qual), capi._p(qual_off), min_qv, capi._p(big), len(big)) == 0
    assert (big[:len(got)] == exp).all() and not big[len(got):].any()


def test_qmask_slice_rebases_a_chunk():
    rng = np.random.default_rng(3)
    seq_off, qual, qual_off = random_reads(rng, 20)
    whole = capi.qmask_from_quals(seq_off, qual, qual_off, 20)
    a, b = 7, 31
    part = capi.qmask_from_quals(seq_off[a:b + 1], qual, qual_off[a:b + 1], 20)
    cut = capi.qmask_slice(whole, int(seq_off[a] - seq_off[0]), int(seq_off[b] - seq_off[a]))
    assert (cut == part).all()


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_decoder_mask_equals_threshold_of_effective_quals(tmp_path, sanitize):
    """tests/cpp/qmask_decode_check.cpp: a rich-QV BAM of a few hundred reads through the front end's decoder in both forms, the
    sequential and the pipelined reader; a stand-alone program, built once more with AddressSanitizer + UBSan."""
    host = os.path.join(ROOT, "minorseq_amd", "host")
    exe = str(tmp_path / "qmask_decode_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", *flags, "-I" + host, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "qmask_decode_check.cpp"), "-lz", "-lpthread", "-o", exe])
    bam = str(tmp_path / "q.bam")
    subprocess.check_call([SYNTH, "--reads", "700", "--cols", "901", "--seed", "8", "--partial", "0.3", "--rich-qv", "--low-qv-ppm", "20000",
                           "--mask", "0.03", "-o", bam])
    for min_qv in ("20", "200"):
        out = subprocess.run([exe, bam, min_qv], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
