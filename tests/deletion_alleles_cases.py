"""The matrices of tests/test_gpu_deletion_alleles.py and the conditions that keep its cases from passing vacuously
(tests/test_deletion_alleles_host.py runs the mirror over them without a GPU).  numpy only: nothing of the library is loaded."""
import numpy as np

GAP = 4

# (reads, columns).  The sizes the issue names — a word is 32 reads, a tile 512, a plane row whole 128-byte lines (1024 reads), a
# column group 64 — and the sizes of this kernel (kernels_del_alleles.hip): a lane owns a word, a workgroup a WORD GROUP of 64
# words (2048 reads) and a COLUMN SEGMENT of at least 8 columns, walked in batches of 4.  2047 / 2048 / 2049 reads end a word
# group one short of, at and one past its last read, 4097 reads are three groups, the last of one read; 8 / 9 columns are one
# segment and the first column of a second, 16 / 17 two segments and one more, 7 columns a segment with a batch cut short, 11 a
# second segment of three.  Below 3 columns no run is bounded.
CASES = [
    (1, 1), (1, 2), (1, 3), (1, 7), (31, 3), (32, 4), (33, 5), (1023, 64), (1024, 65), (1025, 66), (2049, 67), (33, 130),
    (1025, 131), (5000, 200),
    (2047, 8), (2048, 9), (2049, 16), (4097, 17), (40, 11), (65, 33),
]


def make_case(n, n_cols, seed, n_hap=4):
    """Reads that are copies of a few haplotype rows of bases with seeded damage by kind of read (deletions of 1, 2, 3, 6 bases at
    a seeded start, scattered N cells, ragged code-6 ends, code 6 throughout, some clean), as test_gpu_deletions.make_case has it,
    one-base deletions at a seeded cell in a hundred, and planted on top, where the shape has room:
      runs of four columns across every multiple of 8 (this kernel's segments) and of 64 (a column group), in reads 0, 1, 2, ...;
      the same run in the last read of every 512-read tile and in the first of the next;
      the longest bounded run (s = 1, len = n_cols - 2), a run open at column 0, one open at the last column, a read that is '-'
      throughout, and an N flank and a code-6 flank."""
    rng = np.random.default_rng(seed)
    haps = rng.integers(0, 4, size=(n_hap, n_cols), dtype=np.uint8)
    rows = haps[rng.integers(0, n_hap, size=n)].copy()
    kind = rng.integers(0, 10, size=n)
    ci = np.arange(n_cols)[None, :]
    for k, length in ((0, 3), (1, 1), (2, 2), (3, 6)):
        if n_cols < length:
            continue
        start = rng.integers(0, n_cols - length + 1, size=n)[:, None]
        rows[(kind == k)[:, None] & (ci >= start) & (ci < start + length)] = GAP
    rows[rng.random(size=rows.shape) < 0.01] = GAP
    rows[(kind == 4)[:, None] & (rng.random(size=rows.shape) < 2.0 / n_cols)] = 5
    lo, hi = rng.integers(0, n_cols // 3 + 1, size=n), n_cols - rng.integers(0, n_cols // 3 + 1, size=n)
    rows[(kind == 5)[:, None] & ((ci < lo[:, None]) | (ci >= hi[:, None]))] = 6
    rows[kind == 6] = 6
    r = 0
    for edge in range(8, n_cols - 3, 8):                   # [edge - 2, edge + 2): across a segment (and every 64: a group) boundary
        row = r % n
        rows[row, max(0, edge - 4):edge + 4] = haps[0, max(0, edge - 4):edge + 4]
        rows[row, edge - 2:edge + 2] = GAP
        r += 1
    if n_cols >= 6:
        for t in range(512, n, 512):
            for row in (t - 1, t):
                rows[row] = haps[1]
                rows[row, 2:5] = GAP
    special = [i for i in range(n - 1, max(-1, n - 7), -1)]
    if n_cols >= 3 and special:
        i = special.pop(0)
        rows[i] = haps[0]
        rows[i, 1:n_cols - 1] = GAP                        # the longest bounded run
    if n_cols >= 2 and special:
        i = special.pop(0)
        rows[i] = haps[0]
        rows[i, 0] = GAP                                   # open at the left edge
    if n_cols >= 2 and special:
        i = special.pop(0)
        rows[i] = haps[0]
        rows[i, n_cols - 1] = GAP                          # open at the right edge
    if n_cols >= 5 and special:
        i = special.pop(0)
        rows[i] = haps[0]
        rows[i, 0], rows[i, 1:3], rows[i, 3] = 5, GAP, haps[0, 3]      # an N flank: bounded
    if n_cols >= 5 and special:
        i = special.pop(0)
        rows[i] = haps[0]
        rows[i, 0], rows[i, 1:3] = 6, GAP                              # a code-6 flank: open
    if special:
        rows[special.pop(0)] = GAP                         # '-' throughout
    if n == 1 and n_cols >= 7:
        rows[0] = haps[0]
        rows[0, 0], rows[0, 2:4], rows[0, 6] = GAP, GAP, GAP   # the only read: an open run at each edge and a bounded one
    elif n == 1 and n_cols >= 3:
        rows[0] = haps[0]
        rows[0, 1:n_cols - 1] = GAP
    elif n == 1:
        rows[0] = GAP
    return rows


def assert_not_vacuous(rows, res):
    """At least one bounded and, where the shape allows one, one open run."""
    n, n_cols = rows.shape
    if n_cols >= 3:
        assert res["runs"][0] >= 1 and len(res["alleles"]) >= 1
    else:
        assert res["runs"][0] == 0 and len(res["alleles"]) == 0 and res["runs"][1] >= 1
    if n > 1 or n_cols >= 7:
        assert res["runs"][1] >= 1 and res["open"].any()


def distinct_alleles(n, n_cols):
    """A different bounded (s, len) in every read: read i has the i-th of the (s, len) with 1 <= s, s + len <= n_cols - 1."""
    keys = [(s, length) for s in range(1, n_cols - 1) for length in range(1, n_cols - s)]
    assert len(keys) >= n
    rng = np.random.default_rng(n + n_cols)
    rows = np.repeat(rng.integers(0, 4, size=(1, n_cols), dtype=np.uint8), n, axis=0)
    for i in range(n):
        s, length = keys[(i * 2) % len(keys)] if len(keys) >= 2 * n else keys[i]
        rows[i, s:s + length] = GAP
    return rows


def one_allele_everywhere(n, n_cols):
    """One allele (5, 9) in every read plus a second, distinct run per read behind it."""
    rng = np.random.default_rng(7)
    rows = np.repeat(rng.integers(0, 4, size=(1, n_cols), dtype=np.uint8), n, axis=0)
    rows[:, 5:14] = GAP
    for i in range(n):
        s = 16 + i % (n_cols - 16 - 34)
        rows[i, s:s + 1 + (i // (n_cols - 50)) % 32] = GAP
    return rows


def every_allele(n, n_cols):
    """Every possible bounded (s, len) of n_cols columns occurs: (n_cols - 1)(n_cols - 2) / 2 of them, one a read, the rest of the
    reads repeat them."""
    keys = [(s, length) for s in range(1, n_cols - 1) for length in range(1, n_cols - s)]
    assert len(keys) == (n_cols - 1) * (n_cols - 2) // 2 <= n
    rng = np.random.default_rng(n_cols)
    rows = np.repeat(rng.integers(0, 4, size=(1, n_cols), dtype=np.uint8), n, axis=0)
    for i in range(n):
        s, length = keys[i % len(keys)]
        rows[i, s:s + length] = GAP
    return rows
