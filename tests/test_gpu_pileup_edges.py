"""Every form of the pileup kernels at its tile, flush-batch and load-width edges (tests/pileup_edges.py: read counts on the
edges x column layouts x contents, 76 narrow windows and 4 wide ones), bit for bit against a plain numpy reference.

Each case goes through the stage API (twice in a row; with the reference, with a reference that differs in every base, in
majority mode), a single run and a group run beside a shallower window, folded and unfolded; which kernel form a launch took —
chunk width, load width, tiles, read splits, fast or general stream, flush batches — is read from the -DJL_TUNING build of the
library (jl_tuning_pileup_shape) and asserted against what the case was designed for, so a case that lands on another path fails.
A process loads one library and has one JL_NO_FOLD_CALL, so the parts run in child processes (tests/pileup_edges_child.py).
Runs only on a real MI355X: `pytest -m gpu`.
"""
import os
import subprocess
import sys

import pytest

import pileup_edges as pe

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TUNING_LIB = os.path.join(ROOT, "tools_tuning", "lib_exp", "libjuliet_hip.so")


def run_child(part, form):
    assert os.path.exists(TUNING_LIB), "no tuning build of the library: tools_tuning/build_tuning_lib.sh (build() runs it)"
    env = dict(os.environ, JL_LIB=TUNING_LIB, JL_EXPECT_FORM=form)
    for k in ("JL_NO_GRAPH", "JL_NO_FOLD_CALL", "JL_EDGES_KEEP_GOING"):
        env.pop(k, None)
    if form == "unfolded":
        env["JL_NO_FOLD_CALL"] = "1"
    out = subprocess.run([sys.executable, os.path.join(HERE, "pileup_edges_child.py"), part], env=env, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    assert "EDGES-OK %s %s" % (part, form) in out.stdout
    print(out.stdout)
    taken = set()
    for line in out.stdout.splitlines():
        if line.startswith("TAKEN "):
            k, w, nq, s, m = line.split()[1:]
            taken.add((k, int(w), int(nq), s, bool(int(m))))
    return taken


@pytest.mark.parametrize("form", ["folded", "unfolded"])
@pytest.mark.parametrize("part", sorted(pe.PARTS))
def test_designed_windows_through_every_form(part, form):
    """col_counts, hist and coverage of every case of the part, on every path, equal the numpy reference; the forms the launches
    took (the child reads them from the library) are the ones the cases were designed for."""
    exp = set()
    for c in pe.PARTS[part]:
        exp |= pe.case_forms(c, form == "folded")
    assert run_child(part, form) == exp


def test_single_runs_with_one_workgroup_over_more_tiles_than_a_batch():
    """Windows wide enough (the column count comes from the device's occupancy) that jl_pileup_rsplit gives 1: 16 tiles of <3,2>
    and of <6,2> and 8 tiles of <3,4> in ONE workgroup, plain and folded — and 7 tiles over 2 workgroups, a split of the atomic
    path that does not divide the tile count.  The window is a 24-column block repeated; the reference is computed on the block."""
    exp = set()
    for layout, n, rsplit in pe.WIDE:
        exp |= pe.wide_forms(layout, n, rsplit)
    assert run_child("wide", "folded") == exp
