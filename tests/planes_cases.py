"""The shapes, the plain statements and the wrong producers of the resident-format tests (test_planes_host.py without a GPU,
test_gpu_planes.py on one).  The format (include/juliet_hip.h "THE resident format", docs/SPEC.md §1): [n_cols][3][plane_stride]
bytes, plane k = bit k of every read's code, read i in bit i & 7 of byte i >> 3, every read past n_reads code 6 to the END of
the plane row.  Test infrastructure; nothing of the product imports it."""
from collections import namedtuple

import numpy as np

from minorseq_amd import msa

# read counts on both sides of the units the producers work in: the byte (8 reads), the 32-read word, the 64-read unit of the
# upload kernel, the 128-byte line of nibbles a download shows (256), the walk tile (512), the 128-byte line of a plane (1024)
READS = (1, 7, 8, 9, 31, 33, 63, 64, 65, 255, 256, 257, 511, 513, 1023, 1024, 1025, 2049)
COLS = (1, 2, 3, 5)
STAGE_BYTES = 64 << 20              # capi.hip jl_msa_upload / jl_msa_download: ((uint64_t)64 << 20) / col_stride columns a chunk
PAD = 6

# n reads x l columns resident at `stride` bytes a plane row; `col_stride`, `behind`: the interchange buffer an upload is given
# (bytes per column, and the nibble it holds wherever no read is)
Shape = namedtuple("Shape", "n l stride col_stride behind")


def cols_for(n):
    return COLS[READS.index(n) % len(COLS)]


def stride16(n):
    """The smallest plane stride jl_msa_adopt takes: a multiple of 16 bytes that holds the reads."""
    return ((n + 7) // 8 + 15) // 16 * 16


def strides(n):
    return sorted({msa.plane_stride(n), stride16(n), stride16(n) + 16})


def stage_per(n_cols, col_stride):
    """Columns per staging chunk, the code's own rule."""
    return min(n_cols, max(1, STAGE_BYTES // col_stride))


def column(n, l, c):
    """Column c of the n x l matrix of a shape: codes uniform over 0..6 (every code next to every padding boundary)."""
    return np.random.default_rng([n, l, c]).integers(0, 7, size=n, dtype=np.uint8)


def code_rows(n, l):
    return np.stack([column(n, l, c) for c in range(l)], axis=1)


def shape_of(n, l=None, stride=None, wider=0, behind=PAD):
    return Shape(n, cols_for(n) if l is None else l, msa.plane_stride(n) if stride is None else stride, msa.col_stride(n) + wider, behind)


def staging_shape():
    """The smallest matrix whose interchange form is two staging chunks: 2^20 + 1 reads are 524416 bytes a column, 127 of them fit
    64 MiB, two more make the second chunk."""
    n = (1 << 20) + 1
    cs = msa.col_stride(n)
    per = STAGE_BYTES // cs
    return Shape(n, per + 2, msa.plane_stride(n), cs, PAD)


def staging_columns(sh):
    """The columns compared of the staging shape: the first, both sides of the chunk boundary, the last."""
    per = stage_per(sh.l, sh.col_stride)
    return [0, per - 1, per, sh.l - 1]


def named_shapes():
    """Every shape test_gpu_planes.py drives a producer at, by name."""
    out = {}
    for n in READS:
        for s in strides(n):
            out["n%d stride%d" % (n, s)] = shape_of(n, stride=s)
        for wider in (128, 384):
            for behind in (PAD, 7, 8, 15):
                out["n%d col_stride+%d behind%X" % (n, wider, behind)] = shape_of(n, wider=wider, behind=behind)
    out["staging"] = staging_shape()
    return out


def columns_of(name, sh):
    return staging_columns(sh) if name == "staging" else list(range(sh.l))


# ------------------------------------------------------------------------------------------------ plain statements
def cells_of(sh, cols):
    """uint8[len(cols)][8 stride]: the codes of a plane row, read by read, code 6 past the reads."""
    out = np.full((len(cols), 8 * sh.stride), PAD, dtype=np.uint8)
    for k, c in enumerate(cols):
        out[k, :sh.n] = column(sh.n, sh.l, c)
    return out


def to_planes(cells):
    """uint8[k][reads] codes 0..7 -> uint8[k][3][reads / 8]"""
    return np.stack([np.packbits((cells >> k) & 1, axis=1, bitorder="little") for k in range(3)], axis=1)


def from_planes(planes):
    """uint8[k][3][stride] -> uint8[k][8 stride] codes 0..7"""
    out = np.zeros((planes.shape[0], 8 * planes.shape[2]), dtype=np.uint8)
    for k in range(3):
        out |= np.unpackbits(planes[:, k, :], axis=1, bitorder="little") << k
    return out


def expected_image(sh, cols):
    rows = np.stack([column(sh.n, sh.l, c) for c in cols], axis=1)
    return msa.pack_planes(rows, sh.stride)


def to_nibbles(cells):
    """uint8[k][reads] codes 0..15 (reads even) -> uint8[k][reads / 2]: read i in byte i / 2, low nibble for even i"""
    return (cells[:, 0::2] | (cells[:, 1::2] << 4)).astype(np.uint8)


def from_nibbles(packed):
    out = np.empty((packed.shape[0], 2 * packed.shape[1]), dtype=np.uint8)
    out[:, 0::2] = packed & 15
    out[:, 1::2] = packed >> 4
    return out


def nibble_buffer(rows, col_stride, behind=PAD):
    """What a caller may hand jl_msa_upload: [l][col_stride] nibbles, `behind` in every nibble past read n - 1."""
    n, l = rows.shape
    cells = np.full((l, 2 * col_stride), behind, dtype=np.uint8)
    cells[:, :n] = rows.T
    return to_nibbles(cells)


def download_of_planes(planes, n):
    """What jl_msa_download returns of resident planes uint8[l][3][stride], as kernels_util.hip documents it: the stored bits of
    every read position the planes hold (codes 0..7, whatever they are), padding (6) past the planes' end; 2 jl_col_stride(n)
    read positions a column."""
    shown = 2 * msa.col_stride(n)
    cells = from_planes(planes)
    out = np.full((planes.shape[0], shown), PAD, dtype=np.uint8)
    m = min(shown, cells.shape[1])
    out[:, :m] = cells[:, :m]
    return to_nibbles(out)


def tail_filled(planes, n, fill):
    """The planes with every byte past the smallest stride that holds the reads (stride16) set to `fill`: stored bits behind the
    padding reads that are no padding."""
    out = planes.copy()
    out[:, :, stride16(n):] = fill
    return out


# ------------------------------------------------------------------------------------------------ per-cell loops (small shapes)
def loop_pack_planes(rows, stride):
    n, l = rows.shape
    out = np.zeros((l, 3, stride), dtype=np.uint8)
    for c in range(l):
        for i in range(8 * stride):
            code = int(rows[i, c]) if i < n else PAD
            for k in range(3):
                if (code >> k) & 1:
                    out[c, k, i >> 3] |= 1 << (i & 7)
    return out


def loop_pack_columns(rows):
    n, l = rows.shape
    stride = ((n + 1) // 2 + 127) // 128 * 128
    out = np.zeros((l, stride), dtype=np.uint8)
    for c in range(l):
        for i in range(2 * stride):
            code = int(rows[i, c]) if i < n else PAD
            out[c, i >> 1] |= code << (4 * (i & 1))
    return out


# ------------------------------------------------------------------------------------------------ wrong producers
UNWRITTEN = 0     # what a producer that stores nothing somewhere leaves there: the zeroes of fresh memory


def _pad_from(sh, cols, first_pad, code=PAD, last_pad=None):
    """reads, then UNWRITTEN up to read position first_pad, then `code` up to last_pad (the row's end), UNWRITTEN behind"""
    cells = cells_of(sh, cols)
    end = cells.shape[1]
    cells[:, sh.n:] = UNWRITTEN
    lo = max(sh.n, min(first_pad, end))
    hi = end if last_pad is None else max(sh.n, min(last_pad, end))
    cells[:, lo:hi] = code
    return to_planes(cells)


def _up(n, unit):
    return -(-n // unit) * unit


def wrong_pad_ends_at_col_stride(sh, cols):
    return _pad_from(sh, cols, sh.n, last_pad=2 * msa.col_stride(sh.n))


def wrong_pad_code_0(sh, cols):
    return _pad_from(sh, cols, sh.n, code=0)


def wrong_pad_code_7(sh, cols):
    return _pad_from(sh, cols, sh.n, code=7)


def wrong_last_byte_not_padded(sh, cols):
    return _pad_from(sh, cols, _up(sh.n, 8))


def wrong_last_word_not_padded(sh, cols):
    return _pad_from(sh, cols, _up(sh.n, 32))


def wrong_last_unit_not_padded(sh, cols):
    return _pad_from(sh, cols, _up(sh.n, 64))


def wrong_planes_1_2_swapped(sh, cols):
    return expected_image(sh, cols)[:, [0, 2, 1], :]


def wrong_bit_order_reversed(sh, cols):
    cells = cells_of(sh, cols)
    return to_planes(cells.reshape(len(cols), -1, 8)[:, :, ::-1].reshape(len(cols), -1))


def wrong_second_chunk_at_column_0(sh, cols):
    """every staging chunk's columns land from column 0 on: a later chunk overwrites the first, the columns behind stay unwritten"""
    per = stage_per(sh.l, sh.col_stride)
    out = np.zeros((len(cols), 3, sh.stride), dtype=np.uint8)
    for k, d in enumerate(cols):
        src = [s for s in range(d, sh.l, per)] if d < per else []
        if src:
            out[k] = expected_image(sh, [src[-1]])[0]
    return out


def wrong_col_stride_is_the_read_bound(sh, cols):
    """whatever the caller's buffer holds up to its column stride is taken for reads (its low three bits stored)"""
    cells = cells_of(sh, cols)
    cells[:, sh.n:min(2 * sh.col_stride, cells.shape[1])] = sh.behind & 7
    return to_planes(cells)


WRONG = {
    "pad_ends_at_col_stride": wrong_pad_ends_at_col_stride,
    "pad_code_0": wrong_pad_code_0,
    "pad_code_7": wrong_pad_code_7,
    "last_byte_not_padded": wrong_last_byte_not_padded,
    "last_word_not_padded": wrong_last_word_not_padded,
    "last_unit_not_padded": wrong_last_unit_not_padded,
    "planes_1_2_swapped": wrong_planes_1_2_swapped,
    "bit_order_reversed": wrong_bit_order_reversed,
    "second_chunk_at_column_0": wrong_second_chunk_at_column_0,
    "col_stride_is_the_read_bound": wrong_col_stride_is_the_read_bound,
}
