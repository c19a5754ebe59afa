"""The resident format without a GPU: the bit helpers of csrc/planes.h (compiled for the host) against per-bit loops, the numpy
layouts of minorseq_amd/msa.py against per-cell loops, and the shapes of test_gpu_planes.py against ten wrong producers — a
shape list that cannot tell one of them from the right image is a failed test.  The producers themselves: test_gpu_planes.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import planes_cases as pc
from minorseq_amd import msa

HERE = os.path.dirname(os.path.abspath(__file__))
U32P = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("shim") / "libplanes_shim.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "csrc", "planes_shim.cpp")])
    lib = C.CDLL(out)
    lib.shim_plane_bits8.argtypes = [U32P, C.c_uint32, U32P, C.c_uint64]
    lib.shim_spread8.argtypes = [U32P, U32P, C.c_uint64]
    lib.shim_planes_to_nibbles8.argtypes = [U32P, U32P, U32P, U32P, C.c_uint64]
    for f in (lib.shim_plane_bits8, lib.shim_spread8, lib.shim_planes_to_nibbles8):
        f.restype = None
    return lib


def ptr(a):
    return a.ctypes.data_as(U32P)


# ------------------------------------------------------------------------------------------------ bit helpers
def loop_plane_bits8(w, k):
    """bit k of nibble j of w -> bit j"""
    return sum(((w >> (4 * j + k)) & 1) << j for j in range(8))


def loop_spread8(b):
    """bit j of b -> bit 0 of nibble j"""
    return sum(((b >> j) & 1) << (4 * j) for j in range(8))


def test_spread8_every_byte(shim):
    b = np.arange(256, dtype=np.uint32)
    out = np.zeros_like(b)
    shim.shim_spread8(ptr(b), ptr(out), len(b))
    assert out.tolist() == [loop_spread8(int(x)) for x in b]


@pytest.mark.parametrize("others", [0x00, 0xFF])
def test_planes_to_nibbles8_every_byte_of_every_plane(shim, others):
    for plane in range(3):
        b = [np.full(256, others, dtype=np.uint32) for _ in range(3)]
        b[plane] = np.arange(256, dtype=np.uint32)
        out = np.zeros(256, dtype=np.uint32)
        shim.shim_planes_to_nibbles8(ptr(b[0]), ptr(b[1]), ptr(b[2]), ptr(out), 256)
        exp = [sum(loop_spread8(int(b[k][i])) << k for k in range(3)) for i in range(256)]
        assert out.tolist() == exp, plane


def test_plane_bits8_random_dwords(shim):
    """10^5 dwords, a third of them codes 0..7 only, the rest any nibble (bit 3 set in half of them: it must not leak into a plane);
    the edges by hand."""
    rng = np.random.default_rng(8)
    w = rng.integers(0, 1 << 32, size=100000, dtype=np.uint64).astype(np.uint32)
    w[::3] &= 0x77777777
    w[:6] = (0, 0xFFFFFFFF, 0x88888888, 0x66666666, 0x00000008, 0x80000000)
    assert (w & 0x88888888).astype(bool).mean() > 0.5
    for k in range(3):
        out = np.zeros_like(w)
        shim.shim_plane_bits8(ptr(w), k, ptr(out), len(w))
        exp = np.zeros_like(w)
        for j in range(8):                                  # per bit, vectorised over the dwords only
            exp |= ((w >> np.uint32(4 * j + k)) & np.uint32(1)) << np.uint32(j)
        assert (out == exp).all(), k
        assert out[:2000].tolist() == [loop_plane_bits8(int(x), k) for x in w[:2000]]
    # the two are inverse on codes
    codes = w & 0x77777777
    b = [np.zeros_like(w) for _ in range(3)]
    for k in range(3):
        shim.shim_plane_bits8(ptr(codes), k, ptr(b[k]), len(w))
    back = np.zeros_like(w)
    shim.shim_planes_to_nibbles8(ptr(b[0]), ptr(b[1]), ptr(b[2]), ptr(back), len(w))
    assert (back == codes).all()


# ------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize("n", pc.READS)
def test_layouts_equal_per_cell_loops(n):
    l = pc.cols_for(n)
    rows = pc.code_rows(n, l)
    assert rows.shape == (n, l) and rows.max() <= 6
    for stride in pc.strides(n) if n <= 1025 else [msa.plane_stride(n)]:
        planes = msa.pack_planes(rows, stride)
        assert planes.shape == (l, 3, stride) and planes.dtype == np.uint8
        assert (planes == pc.loop_pack_planes(rows, stride)).all(), stride
        assert (msa.unpack_planes(planes, n) == rows).all()
        assert (pc.from_planes(planes)[:, n:] == 6).all()                       # the padding, to the end of the row
    assert (msa.pack_planes(rows) == msa.pack_planes(rows, msa.plane_stride(n))).all()
    packed = msa.pack_columns(rows)
    assert packed.shape == (l, msa.col_stride(n))
    assert (packed == pc.loop_pack_columns(rows)).all()
    assert (msa.unpack_columns(packed, n) == rows).all()
    assert (packed == pc.nibble_buffer(rows, msa.col_stride(n))).all()
    assert (pc.download_of_planes(msa.pack_planes(rows), n) == packed).all()


def test_strides_are_the_headers():
    assert [msa.plane_stride(n) for n in (1, 1024, 1025, 2049)] == [128, 128, 256, 384]
    assert [msa.col_stride(n) for n in (1, 256, 257, 2049)] == [128, 128, 256, 1152]
    assert [pc.stride16(n) for n in (1, 128, 129, 1025)] == [16, 16, 32, 144]
    sh = pc.staging_shape()
    per = pc.stage_per(sh.l, sh.col_stride)
    assert (sh.col_stride, per, sh.l) == (524416, 127, 129)
    assert per * sh.col_stride <= pc.STAGE_BYTES < (per + 1) * sh.col_stride     # two chunks: 127 columns and 2
    assert pc.staging_columns(sh) == [0, 126, 127, 128]


# ------------------------------------------------------------------------------------------------ sensitivity
# the shapes that must catch each wrong producer (more may): a change of the shape list that loses one of these fails here
CAUGHT_AT = {
    "pad_ends_at_col_stride": "n1 stride128",                 # 256 read positions shown, 1024 in the row
    "pad_code_0": "n1 stride16",
    "pad_code_7": "n1 stride16",
    "last_byte_not_padded": "n7 stride16",
    "last_word_not_padded": "n8 stride16",                    # ... which the byte rule cannot see
    "last_unit_not_padded": "n33 stride16",
    "planes_1_2_swapped": "n64 stride16",
    "bit_order_reversed": "n64 stride16",
    "second_chunk_at_column_0": "staging",
    "col_stride_is_the_read_bound": "n257 col_stride+128 behind8",
}


def test_every_wrong_producer_is_caught_by_a_named_shape():
    shapes = pc.named_shapes()
    caught = {name: [] for name in pc.WRONG}
    for sname, sh in shapes.items():
        cols = pc.columns_of(sname, sh)
        exp = pc.expected_image(sh, cols)
        assert exp.shape == (len(cols), 3, sh.stride)
        for name, fn in pc.WRONG.items():
            if sname == "staging" and name != "second_chunk_at_column_0":
                continue                                    # (a megaread shape: only the chunk rule needs it)
            got = fn(sh, cols)
            assert got.shape == exp.shape and got.dtype == exp.dtype, (name, sname)
            if (got != exp).any():
                caught[name].append(sname)
    for name in pc.WRONG:
        print("%-30s caught at %3d shapes, first: %s" % (name, len(caught[name]), ", ".join(caught[name][:4])))
    for name in pc.WRONG:
        assert caught[name], name
        assert CAUGHT_AT[name] in caught[name], (name, caught[name][:8])
    # what only ONE kind of shape can see
    assert caught["second_chunk_at_column_0"] == ["staging"]
    assert all("behind" in s and "behind6" not in s for s in caught["col_stride_is_the_read_bound"])
    assert all(shapes[s].n % 8 for s in caught["last_byte_not_padded"])
    assert all(8 * shapes[s].stride > 2 * msa.col_stride(shapes[s].n) for s in caught["pad_ends_at_col_stride"])
