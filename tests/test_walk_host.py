"""The pure helpers of the plane-row tile walk (csrc/planes.h, the host half of csrc/plane_walk.h), compiled for the host:
the valid mask of a 32-read word and the launch shape of the three counting kernels, at their edges.  The kernels on them:
test_gpu_class.py, test_gpu_deletions.py, test_gpu_insertions.py, test_gpu_sites.py."""
import ctypes as C
import os
import subprocess

import pytest

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
