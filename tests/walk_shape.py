"""The launch shapes of the plane-row tile walk (minorseq_amd/csrc/plane_walk.h) for the tests: the header compiled for the host
(tests/csrc/walk_shim.cpp), so that a deep case is named by the function the launcher calls, not by copied numbers."""
import ctypes as C
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TILE_READS = 512
_lib = None
_dir = None


def _shim():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.TemporaryDirectory(prefix="walk_shim_")
        out = os.path.join(_dir.name, "libwalk_shim.so")
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "csrc", "walk_shim.cpp")])
        _lib = C.CDLL(out)
    return _lib


def walk(n_reads, n_groups):
    """(seg_tiles, n_segs) of jl_walk_shape_for: class pileup (groups of 64 columns), codon deletions, junction span."""
    a, b = C.c_uint32(), C.c_uint32()
    _shim().shim_walk_shape(C.c_uint64(n_reads), C.c_uint32(n_groups), C.byref(a), C.byref(b))
    return a.value, b.value


def class_codons(n_reads, n_pos, n_classes):
    """(seg_tiles, n_segs) of jl_class_codons_shape_for."""
    a, b = C.c_uint32(), C.c_uint32()
    _shim().shim_class_codons_shape(C.c_uint64(n_reads), C.c_uint32(n_pos), C.c_uint32(n_classes), C.byref(a), C.byref(b))
    return a.value, b.value


def deep_case(shape_of):
    """The smallest read count n = 512 t + 300 (the last tile ragged) at which shape_of(n) has seg_tiles >= 4 and n_segs >= 2 and
    the last segment is shorter than the others; (n, seg_tiles, n_segs)."""
    t = 1
    while True:                       # (seg_tiles does not fall as the reads grow: double, then bisect)
        st, ns = shape_of(TILE_READS * t + 300)
        if st >= 4 and ns >= 2:
            break
        t *= 2
    lo, hi = t // 2, t
    while hi - lo > 1:
        mid = (lo + hi) // 2
        st, ns = shape_of(TILE_READS * mid + 300)
        lo, hi = (lo, mid) if st >= 4 and ns >= 2 else (mid, hi)
    for t in range(hi, hi + 8):
        n = TILE_READS * t + 300
        st, ns = shape_of(n)
        if st >= 4 and ns >= 2 and (t + 1) % st != 0:
            return n, st, ns
    raise AssertionError("no deep case near %d tiles" % hi)
