"""The pure helpers of the plane-row tile walk (csrc/planes.h, the host half of csrc/plane_walk.h), compiled for the host:
the valid mask of a 32-read word and the launch shape of the three counting kernels, at their edges.  The kernels on them:
test_gpu_class.py, test_gpu_deletions.py, test_gpu_insertions.py, test_gpu_sites.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import class_codons_mirror
import walk_shape

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("shim") / "libwalk_shim.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "csrc", "walk_shim.cpp")])
    lib = C.CDLL(out)
    lib.shim_valid_bits.restype = C.c_uint32
    lib.shim_valid_bits.argtypes = [C.c_uint64, C.c_uint64]
    lib.shim_walk_tiles.restype = C.c_uint32
    lib.shim_walk_tiles.argtypes = [C.c_uint64]
    lib.shim_walk_shape.restype = None
    lib.shim_walk_shape.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    return lib


READS = (1, 31, 32, 33, 511, 512, 513, 2**31 - 1)


def test_valid_bits_are_the_reads_of_the_word(shim):
    for n in READS:
        last = (n - 1) // 32                    # the word of the last read
        words = {0, 1, last + 2, last + 16, 2**27} | {w for w in range(last - 2, last + 3) if w >= 0}
        for w in sorted(words):
            bits = min(32, max(0, n - 32 * w))
            assert shim.shim_valid_bits(n, w) == (1 << bits) - 1, (n, w)


def test_tiles_hold_512_reads(shim):
    for n in READS + (1023, 1024, 1025, 2049, 100000):
        assert shim.shim_walk_tiles(n) == -(-n // 512), n


def present_rule(n_reads, n_groups):
    """The launch shape as the three launchers had it, each for itself."""
    n_words = (n_reads + 31) // 32
    n_tiles = (n_words + 15) // 16
    segs = max(1, min(n_tiles, 4096 // max(1, n_groups)))
    tiles = (n_tiles + segs - 1) // segs
    seg_tiles = (tiles + 1) & ~1
    return seg_tiles, (n_tiles + seg_tiles - 1) // seg_tiles


def test_walk_shape(shim):
    for n_reads in (1, 512, 513, 2049, 100000, 2**31 - 1):
        n_tiles = -(-n_reads // 512)
        for n_groups in (1, 2, 47, 4096, 5000):
            seg_tiles, n_segs = C.c_uint32(), C.c_uint32()
            shim.shim_walk_shape(n_reads, n_groups, C.byref(seg_tiles), C.byref(n_segs))
            st, ns = seg_tiles.value, n_segs.value
            case = (n_reads, n_groups, st, ns)
            assert st % 2 == 0 and st >= 2, case
            assert ns * st >= n_tiles, case              # every tile is walked
            assert (ns - 1) * st < n_tiles, case         # ... and no segment is empty
            assert (st, ns) == present_rule(n_reads, n_groups), case
    # 2049 reads are five tiles in three segments
    shim.shim_walk_shape(2049, 1, C.byref(seg_tiles), C.byref(n_segs))
    assert (seg_tiles.value, n_segs.value) == (2, 3)


# ---------------------------------------------------------------------------------------------- segments of four tiles and more
def class_codons_rule(n_reads, n_pos, n_classes):
    """The shape as kernels_class_codons.hip had it inline."""
    n_tiles = -(-n_reads // 512)
    n_groups, full = (n_pos + 63) // 64, n_classes // 16
    segs = max(1, min(n_tiles, 1536 // max(1, n_groups * max(1, full))))
    seg_tiles = (n_tiles + segs - 1) // segs
    return seg_tiles, (n_tiles + seg_tiles - 1) // seg_tiles


def test_class_codons_shape():
    for n_reads in (1, 512, 513, 2049, 100000, 2359596, 2**31 - 1):
        for n_pos, n_classes in ((1, 1), (10, 3), (64, 15), (65, 16), (130, 704), (4096, 33)):
            st, ns = walk_shape.class_codons(n_reads, n_pos, n_classes)
            n_tiles = -(-n_reads // 512)
            assert st >= 1 and ns * st >= n_tiles and (ns - 1) * st < n_tiles
            assert (st, ns) == class_codons_rule(n_reads, n_pos, n_classes)


def test_the_deep_cases_are_the_smallest_with_segments_of_four_tiles():
    """What tests/test_gpu_class.py and tests/test_gpu_class_codons.py run: n_tiles * n_groups > 8192 for the shared shape, n_tiles >
    3 * 1536 for the class codons' own; the last segment shorter than the others, the last tile ragged."""
    n, st, ns = walk_shape.deep_case(lambda n: walk_shape.walk(n, 2))
    n_tiles = -(-n // 512)
    assert (st, ns) == (4, 1025) and n_tiles == 4097 and n_tiles * 2 > 8192 and n % 512 == 300 and n_tiles % st == 1
    assert walk_shape.walk(n - 512, 2)[0] == 2                                   # one tile fewer: segments of two
    n, st, ns = walk_shape.deep_case(lambda n: walk_shape.class_codons(n, 10, 3))
    n_tiles = -(-n // 512)
    assert (st, ns) == (4, 1153) and n_tiles == 4609 and n % 512 == 300 and n_tiles % st == 1
    assert walk_shape.class_codons(n - 512, 10, 3)[0] == 3


def test_counts_are_additive_over_reads():
    """The expectation of the deep cases: for rows that are a block repeated with a tail, and labels repeated the same way, the class
    pileup and the class codons are the block's counts times the repeats plus the tail's — against the numpy rules run in full."""
    from test_gpu_class import code_rows, expected, labels
    import second_turn
    block, lab = code_rows(1536, 65, 11), labels("mixed", 1536, 3, 5)
    n = 3 * 1536 + 300
    rows, labs = second_turn.tiled_rows(block, n), second_turn.tiled(lab, n)
    full_c, full_r = expected(rows, labs, 3)
    c, r = expected(block, lab, 3)
    tc, tr = expected(block[:300], lab[:300], 3)
    assert (full_c == 3 * c + tc).all() and (full_r == 3 * r + tr).all() and full_c.any()
    cols = np.arange(63, dtype=np.uint32)
    full_h, full_r = class_codons_mirror.class_codons(rows, labs, 3, cols)
    h, r = class_codons_mirror.class_codons(block, lab, 3, cols)
    th, tr = class_codons_mirror.class_codons(block[:300], lab[:300], 3, cols)
    assert (full_h == 3 * h + th).all() and (full_r == 3 * r + tr).all() and full_h.any()
