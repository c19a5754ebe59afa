#!/usr/bin/env python3
"""Generates tests/golden/linkage_tails.json — run in the dev container only (needs mpmath).

The exact values of p_positive = P(X >= n11) and p_negative = P(X <= n11) of jl_linkage_stats (docs/SPEC.md §15) for the designed
2 x 2 tables of tests/linkage_mirror.py (`tail_design`), X = the reads with both variants when the margins are fixed, to 25
significant digits.  Both are upper tails of a 2 x 2 table, evaluated by make_fisher_general_domain_golden.py's `evaluate`
(rationals up to 400 marked reads, beyond that one point mass from mpmath at 120 digits and the ratio recurrence):
    P(X >= x) of [[x, row1 - x], [col1 - x, n - row1 - col1 + x]],
    P(X <= x) = P(col1 - X >= col1 - x) of the table with its rows exchanged.
A margin of 0 leaves one table: both are 1.  A re-run reproduces the file byte for byte."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from make_fisher_general_domain_golden import DPS, K_EXACT, evaluate   # noqa: E402


def main():
    import linkage_mirror
    tabs = linkage_mirror.tail_design()
    assert len(tabs) <= linkage_mirror.MAX_TAIL_TABLES, len(tabs)
    out = []
    for n11, n10, n01, n00 in tabs:
        row1, row0, col1 = n11 + n10, n01 + n00, n11 + n01
        if 0 in (row1, row0, col1, n10 + n00):
            pos = neg = "1.0"
        else:
            pos = evaluate(n11, row1, n01, row0)[0]
            neg = evaluate(n01, row0, n11, row1)[0]
        out.append({"n11": n11, "n10": n10, "n01": n01, "n00": n00, "p_positive": pos, "p_negative": neg})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "linkage_tails.json")
    with open(path, "w") as f:
        json.dump({"generator": "tests/golden/make_linkage_tails_golden.py", "dps": DPS, "k_exact": K_EXACT, "tables": out}, f, indent=0)
        f.write("\n")
    print(len(out), "tables")


if __name__ == "__main__":
    main()
