"""The launch shape of the per-read counters (minorseq_amd/csrc/readstats_shape.h) for the tests: the header compiled for the host
(tests/csrc/readstats_shape_shim.cpp), so that the edge cases are named by the function the launcher calls, not by copied numbers."""
import ctypes as C
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("wg_reads", "n_chunks", "seg_cols", "n_segs", "k", "flush", "combine")
SEG_COLS_MIN, SEG_COLS_MAX = 64, 255          # JL_RS_SEG_COLS_MIN / _MAX: asserted against the function by test_readstats_host.py
_lib = None
_dir = None


def shape(n_reads, n_cols):
    """dict of FIELDS for a window of n_reads x n_cols."""
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.TemporaryDirectory(prefix="readstats_shim_")
        out = os.path.join(_dir.name, "libreadstats_shape_shim.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "csrc", "readstats_shape_shim.cpp")])
        _lib = C.CDLL(out)
        _lib.shim_readstats_shape.restype = None
        _lib.shim_readstats_shape.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32)]
    v = (C.c_uint32 * 7)()
    _lib.shim_readstats_shape(n_reads, n_cols, v)
    return dict(zip(FIELDS, (int(x) for x in v)))
