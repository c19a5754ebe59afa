"""The matrix of tests/test_gpu_high_rows.py and the numbers that make it the edge it claims to be.  numpy only: nothing of the
library is loaded, and importing it asserts the numbers.

2049 reads x 1150 columns at configs[4]'s own plane stride of 1 250 048 bytes: 3450 plane rows, 4.31 GB, the last 14 of them start
above 2^32.  Column 1145 has plane 0 below the line and planes 1 and 2 above it.  Everything a stage can be asked about lies in three
bands of columns: 0 .. 20, the columns whose codon straddles the line (codon starts 1143 .. 1145, all three frames) and the columns
above it (codon starts 1146 and 1147 = n_cols - 3)."""
import numpy as np

N, L, STRIDE, PREFIX = 2049, 1150, 1_250_048, 272
NB = (N + 7) // 8                                    # bytes of a plane row that hold reads
LINE = 1 << 32
FIRST_HIGH_ROW = -(-LINE // STRIDE)                  # the first plane row that starts at or above 2^32
STRADDLE_COL = FIRST_HIGH_ROW // 3                   # the column whose three plane rows lie on both sides

# the claims of the module text, from the numbers
assert STRIDE == (10_000_000 + 1023) // 1024 * 128 and STRIDE % 16 == 0 and PREFIX % 16 == 0 and NB == 257 <= PREFIX
assert 3 * L == 3450 and 3 * L * STRIDE == 4_312_665_600 > LINE
assert FIRST_HIGH_ROW == 3436 and (FIRST_HIGH_ROW - 1) * STRIDE < LINE <= FIRST_HIGH_ROW * STRIDE
assert STRADDLE_COL == 1145 and FIRST_HIGH_ROW % 3 == 1          # plane 0 of column 1145 below, planes 1 and 2 above
assert 3 * L - FIRST_HIGH_ROW == 14

LOW_STARTS = [0, 1, 3, 6, 9, 12, 15, 18]             # codon starts of the low band (0 and 1 overlap: two frames)
MID_STARTS = [1143, 1144, 1145]                      # codons that hold column 1145: rows on both sides of the line
HIGH_STARTS = [1146, 1147]                           # codons wholly above the line; 1147 = n_cols - 3
POS_COLS = np.array(LOW_STARTS + [1140] + MID_STARTS + HIGH_STARTS, dtype=np.uint32)
HIGH_POS = np.array(MID_STARTS + HIGH_STARTS, dtype=np.uint32)
VAR_COLS = [2, 5, 8, 11, 14, 17, 20, 1142, 1145, 1148, 1149]     # the columns at which the haplotypes differ
DAMAGE_STARTS = [0, 1, 2, 3, 9, 16, 17, 18, 1141, 1142, 1143, 1144, 1145, 1146, 1147]
GENES = [(1, 1150), (2, 1151), (3, 1149)]            # three frames: codon starts 0 .. 1146, 1 .. 1147, 2 .. 1145
CONTROL_GENES = [(1, 10), (1141, 1150), (1142, 1151), (1143, 1149)]     # the bands only: the exact mirror is slow
N_HAP = 8
STOPS = ((3, 0, 0), (3, 0, 2), (3, 2, 0))
assert HIGH_STARTS[-1] == L - 3 and all(3 * (c + 2) + 2 >= FIRST_HIGH_ROW > 3 * c for c in MID_STARTS)
assert all(3 * c >= FIRST_HIGH_ROW for c in HIGH_STARTS) and 3 * (LOW_STARTS[-1] + 2) + 2 < FIRST_HIGH_ROW


def codons_at(base_rows, pos_cols):
    c = np.asarray(pos_cols).astype(np.int64)
    return (16 * base_rows[:, c] + 4 * base_rows[:, c + 1] + base_rows[:, c + 2]).astype(np.uint8)


def build(seed=4):
    """(rows, ref, haps).  Eight haplotype rows — the reference with seeded changes at VAR_COLS; 1 is 0 but for column 1148 and 3 is 2
    but for column 5, so a read opened there agrees with both — and reads that are copies of them, 44 % of haplotype 0 and 8 % of
    each other, with seeded damage by kind of read as the stages' own case builders plant it: scattered '-' and N, ragged code-6 ends
    inside the bands, code 6 throughout, a substitution at a variant column, the twins' column opened, a codon deletion and deletions
    of 1, 2 and 6 bases at the bands' starts, a stop codon there, a recombinant of two haplotypes with the breakpoint in a band, a
    G -> A hypermutated read; five kinds in sixteen stay clean.  A little N noise lies over everything."""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, size=L, dtype=np.uint8)
    ref[[0, 9, 18, 1143, 1146]] = 2                                    # G: hypermutation sites in every band
    haps = np.repeat(ref[None, :], N_HAP, axis=0)
    var = np.array(VAR_COLS)
    flip = rng.random(size=(N_HAP, len(var))) < 0.5
    flip[0] = False
    alt = rng.integers(1, 4, size=(1, len(var)))
    alt[0, [VAR_COLS.index(1145), VAR_COLS.index(1148)]] = 1
    haps[:, var] = ((haps[:, var] + flip * alt) % 4).astype(np.uint8)
    haps[1] = haps[0]
    haps[1, 1148] = (haps[0, 1148] + 1) % 4
    haps[3] = haps[2]
    haps[3, 5] = (haps[2, 5] + 2) % 4
    haps[6, 1145], haps[7, 1145] = (ref[1145] + 2) % 4, ref[1145]       # 6 alone has its base at 1145, 7 and 6 theirs at 1148:
    haps[6, 1148], haps[7, 1148] = (ref[1148] + 3) % 4, (ref[1148] + 2) % 4   # 6 | 7 cut at 1146 has both parents unique above the line
    of = rng.choice(N_HAP, size=N, p=[0.44] + [0.08] * 7)
    rows = haps[of].copy()
    noise = rng.random(size=rows.shape)
    rows[noise < 0.002] = 5
    kind = rng.integers(0, 16, size=N)
    cell = rng.random(size=rows.shape)
    some = (kind == 0) | (kind == 1)
    rows[some[:, None] & (cell < 0.004)] = 4
    rows[some[:, None] & (cell > 0.996)] = 5
    lo, hi = rng.integers(0, 25, size=N), L - rng.integers(0, 25, size=N)
    ci = np.arange(L)[None, :]
    rows[(kind == 2)[:, None] & ((ci < lo[:, None]) | (ci >= hi[:, None]))] = 6
    rows[kind == 3] = 6
    for i in np.flatnonzero(kind == 4):
        c = int(var[rng.integers(0, len(var))])
        rows[i, c] = (rows[i, c] + 1 + rng.integers(0, 3)) % 4
    for i in np.flatnonzero(kind == 5):
        c = 1148 if of[i] in (0, 1) else 5 if of[i] in (2, 3) else int(var[rng.integers(0, len(var))])
        rows[i, c] = 4 + int(rng.integers(0, 3))
    for i in np.flatnonzero(kind == 6):
        c = DAMAGE_STARTS[rng.integers(0, len(DAMAGE_STARTS))]
        rows[i, c:c + 3] = 4
    for i in np.flatnonzero(kind == 7):
        c = DAMAGE_STARTS[rng.integers(0, len(DAMAGE_STARTS))]
        rows[i, c:c + (1, 2, 6)[rng.integers(0, 3)]] = 4
    for i in np.flatnonzero(kind == 8):
        c = DAMAGE_STARTS[rng.integers(0, len(DAMAGE_STARTS))]
        rows[i, c:c + 3] = STOPS[rng.integers(0, 3)]
    for i in np.flatnonzero(kind == 9):
        b = (4, 10, 600, 1144, 1146, 1148)[rng.integers(0, 6)]
        rows[i, b:] = haps[rng.integers(0, N_HAP), b:]
        if i % 3 == 0:
            rows[i] = np.concatenate([haps[6, :1146], haps[7, 1146:]])
    for i in np.flatnonzero(kind == 10):
        g = (ref == 2) & (rng.random(L) < 0.7) & ((np.arange(L) < 60) | (np.arange(L) >= 1090))      # (the bands and a little more)
        g[[0, 9, 18, 1143, 1146]] = True
        rows[i, g & (rows[i] == 2)] = 0
    return rows, ref, haps


def pack_prefix(rows, seed=1):
    """uint8[3 L][PREFIX]: the first PREFIX bytes of every plane row — the packed planes, and seeded random bytes in NB .. PREFIX - 1."""
    n, l = rows.shape
    cols = np.full((l, PREFIX * 8), 6, dtype=np.uint8)
    cols[:, :n] = rows.T
    out = np.empty((l, 3, PREFIX), dtype=np.uint8)
    for k in range(3):
        out[:, k, :] = np.packbits((cols >> k) & 1, axis=1, bitorder="little")
    clean = out.reshape(3 * l, PREFIX).copy()
    out[:, :, NB:] = np.random.default_rng(seed).integers(0, 256, size=(l, 3, PREFIX - NB), dtype=np.uint8)
    return out.reshape(3 * l, PREFIX), clean


def in_high(cols):
    """Which of the columns (codon starts) have a plane row at or above 2^32 under their three columns."""
    return 3 * (np.asarray(cols).astype(np.int64) + 2) + 2 >= FIRST_HIGH_ROW
