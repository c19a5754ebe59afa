"""The launch shape of the per-read reading-frame counters (minorseq_amd/csrc/orf_shape.h) for the tests: the header compiled for
the host (tests/csrc/orf_shape_shim.cpp), so that the edge cases are named by the function the launcher calls, not by copied
numbers."""
import ctypes as C
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("wg_reads", "n_chunks", "seg_codons", "k", "flush_codons", "n_segs", "grid")
_lib = None
_dir = None


def _load():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.TemporaryDirectory(prefix="orf_shim_")
        out = os.path.join(_dir.name, "liborf_shape_shim.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "csrc", "orf_shape_shim.cpp")])
        _lib = C.CDLL(out)
        _lib.shim_orf_shape.restype = None
        _lib.shim_orf_shape.argtypes = [C.POINTER(C.c_uint32), C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        _lib.shim_orf_constants.restype = None
        _lib.shim_orf_constants.argtypes = [C.POINTER(C.c_uint32)]
    return _lib


def constants():
    """dict of max_spans, seg_codons_max, seg_codons_min, k (the library's own slice count)."""
    v = (C.c_uint32 * 4)()
    _load().shim_orf_constants(v)
    return dict(zip(("max_spans", "seg_codons_max", "seg_codons_min", "k"), (int(x) for x in v)))


def shape(n_codons, n_reads, k=0):
    """dict of FIELDS, and span_segs (a list), for spans of n_codons[g] codons over n_reads reads; k = 0: the library's own."""
    n_codons = [int(x) for x in n_codons]
    arr = (C.c_uint32 * len(n_codons))(*n_codons)
    v = (C.c_uint32 * 7)()
    segs = (C.c_uint32 * len(n_codons))()
    _load().shim_orf_shape(arr, len(n_codons), n_reads, k, v, segs)
    d = dict(zip(FIELDS, (int(x) for x in v)))
    d["span_segs"] = [int(x) for x in segs]
    return d
