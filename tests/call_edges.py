"""Designed codon histograms for the call stage (test infrastructure, like records_expand.py; nothing of the product imports it).

`rows_from_hists` turns chosen histograms into a by-row symbol matrix, so that every codon position of a window is one chosen
set of 2x2 tables; the rest lays the cases of tests/golden/call_edges.json out as windows (one position per case, cases that
share launch parameters side by side) and states the rows the call stage must produce for them.

Symbols as everywhere: A C G T = 0..3, '-' = 4, N = 5, not covered = 6; codon index = 16 b0 + 4 b1 + b2."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "call_edges.json")

ERROR_MODELS = {"sequel": (0.998826, 5.8e-5, 1.0e-3), "permissive": (0.99764, 1.2e-4, 2.0e-3)}   # docs/SPEC.md §5
NOT_SIGNIFICANT, CALLED, FILTERED = 0, 1, 2   # a fixture codon's decision; FILTERED: significant, dropped by min/max-perc or the DRM mask


def rows_from_hists(hists, extra=None, seed=0):
    """uint8[max reads][3 * len(hists)] whose codon histogram at position p (columns 3p..3p+2) is exactly hists[p].

    hists: one mapping codon index -> count per position.  extra: per position, the number of further reads that carry a
    deletion, an N or nothing in one of the three columns (they are skipped there: coverage < number of reads).  Reads a
    position does not need carry code 6 in its columns.  The reads of every position are spread over the rows by a seeded
    permutation of its own, so counts do not line up with the tiles of the counting kernels."""
    n_pos = len(hists)
    extra = [0] * n_pos if extra is None else [int(x) for x in extra]
    need = [sum(int(v) for v in h.values()) + x for h, x in zip(hists, extra)]
    n_rows = max(need, default=0)
    rows = np.full((n_rows, 3 * n_pos), 6, dtype=np.uint8)
    rng = np.random.default_rng(seed)
    for p, (h, x) in enumerate(zip(hists, extra)):
        if need[p] == 0:
            continue
        codons = np.repeat(np.array([int(j) for j in h], dtype=np.int64), [int(v) for v in h.values()])
        blk = np.stack([(codons >> 4) & 3, (codons >> 2) & 3, codons & 3], axis=1).astype(np.uint8)
        if x:
            i = np.arange(x)
            bad = np.stack([(i + 1) & 3, (i >> 1) & 3, (i >> 2) & 3], axis=1).astype(np.uint8)   # bases that would count ...
            bad[i, i % 3] = np.array([4, 5, 6], dtype=np.uint8)[(i // 3) % 3]                    # ... but for this column
            blk = np.concatenate([blk, bad])
        at = rng.permutation(n_rows)[: need[p]]
        rows[at, 3 * p: 3 * p + 3] = blk
    return rows


def n_substituted(ref, j):
    return sum(((ref >> s) & 3) != ((j >> s) & 3) for s in (4, 2, 0))


def load_fixture():
    with open(FIXTURE) as f:
        fx = json.load(f)
    for c in fx["cases"]:
        c["hist"] = {int(j): int(v) for j, v in c["hist"].items()}
        c["codons"] = {int(j): v for j, v in c["codons"].items()}
        c["prm"] = fx["params"][c["params"]]
        c.setdefault("ref_codon", c["ref"])   # written only for majority-mode cases
        c.setdefault("drm", None)
        c.setdefault("extra", 0)
    return fx


def error_row(prm):
    e = prm["err"]
    return ERROR_MODELS[e] if isinstance(e, str) else tuple(e)


def batch_key(case):
    """Cases with the same key can be positions of one launch: parameters, reference or majority mode, DRM masks or none."""
    return (case["params"], case["ref"] is None, case["drm"] is not None)


def batches(cases):
    """[(key, [cases])] in fixture order."""
    out = {}
    for c in cases:
        out.setdefault(batch_key(c), []).append(c)
    return list(out.items())


class Window:
    """Cases laid out as the positions of one window, `lead` empty positions (no read at all) first: one gene (1, 3P + 1) in
    frame 0, position p at column 3p."""

    def __init__(self, cases, lead=0, seed=0):
        self.cases, self.lead = list(cases), lead
        self.P = lead + len(self.cases)
        self.genes = np.array([(1, 3 * self.P + 1)], dtype=[("begin", "<u4"), ("end", "<u4")])
        self.hists = [{}] * lead + [c["hist"] for c in self.cases]
        self.extra = [0] * lead + [c.get("extra", 0) for c in self.cases]
        self.seed = seed
        self._rows = None
        c0 = self.cases[0]
        self.prm = c0["prm"]
        self.refseq = None
        if c0["ref"] is not None:
            codons = [0] * lead + [c["ref"] for c in self.cases]
            self.refseq = np.array([[(r >> 4) & 3, (r >> 2) & 3, r & 3] for r in codons], dtype=np.uint8).reshape(-1)
        self.drm = None
        if c0["drm"] is not None:
            self.drm = np.array([2 ** 64 - 1] * lead + [c["drm"] for c in self.cases], dtype=np.uint64)

    @property
    def rows(self):
        if self._rows is None:
            self._rows = rows_from_hists(self.hists, self.extra, seed=self.seed)
            if self._rows.shape[0] == 0:   # only empty positions: one read that covers nothing
                self._rows = np.full((1, 3 * self.P), 6, dtype=np.uint8)
        return self._rows

    def expected_rows(self, keep=(CALLED,)):
        """The variant rows of the window in table order (SPEC §6) as tuples
        (codon_pos, col, ref_codon, codon, count, coverage, expected, p_adj string, log_p string)."""
        out = []
        for k, c in enumerate(self.cases):
            p = self.lead + k
            for j in sorted(c["codons"]):
                v = c["codons"][j]
                if v[1] in keep:
                    out.append((p + 1, 3 * p, c["ref_codon"], j, c["hist"][j], c["cov"], v[0], v[2], v[3]))
        return out
