"""The folded index kernels under their register budget, and the call evaluation in stages (csrc/call_eval.h: screen, Fisher,
store; DESIGN.md "With the deviation index").  Nothing that is computed may change: every comparison is exact equality between a
window's run 1 (planes, folded), its run 3 (index form, folded: pileup_index_fold_kernel, or pileup_index_fold_group_kernel in a
group) and, for the integer fields and the haplotypes, the oracle; p-values against the oracle within the tolerances of
tests/test_gpu_parity.py.  Runs only on a real MI355X: `pytest -m gpu`.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib
from group_forms_child import variants_equal
from minorseq_amd import capi
from test_gpu_deviation_index import ONE_FRAME, assert_oracle, assert_same, make_rows

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TUNING_LIB = os.path.join(ROOT, "tools_tuning", "lib_exp", "libjuliet_hip.so")


@pytest.fixture(scope="module")
def orc():
    return oracle_lib.load()


def three_single_runs(jl, genes, refseq, prm=None, masks=None):
    """jl_run_async three times, each collected: run 1 and 2 from the planes, the build waited for, run 3 from the index.
    Returns the (result, pileup) of run 1 and of run 3."""
    snaps = []
    for run in (1, 2, 3):
        out = jl.run(genes, refseq, prm or capi.default_params(), masks, True)
        snaps.append((out, jl.pileup_fetch()))
        info = jl.index_info(wait=True)
        assert info["runs"] == run and info["last_form"] == (1 if run == 3 else 0), (run, info)
        if run == 2:
            assert info["state"] == capi.INDEX_BUILT and info["indexed_chunks"] > 0, info
    return snaps[0], snaps[2]


def test_group_of_three_third_launch_index_form_and_folded():
    """tests/fold_budget_child.py on the tuning build: three windows, three launches, the third index-form and folded by
    jl_msa_index_info and by the library's form counter."""
    assert os.path.exists(TUNING_LIB), "no tuning build of the library: tools_tuning/build_tuning_lib.sh (build() runs it)"
    env = dict(os.environ, JL_LIB=TUNING_LIB)
    for k in ("JL_NO_GRAPH", "JL_NO_FOLD_CALL"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(HERE, "fold_budget_child.py")], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "FOLD-BUDGET-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


@pytest.mark.parametrize("n", [5000])
def test_single_window_index_form(orc, n):
    """One 240-column window through jl_run_async: run 3 is pileup_index_fold_kernel."""
    l = 240
    rows, ref = make_rows(n, l, seed=77)
    genes = ONE_FRAME(l)
    jl = capi.Juliet(0)
    try:
        jl.upload_rows(rows)
        s1, s3 = three_single_runs(jl, genes, ref)
        assert_same(s1, s3, "single")
        assert_oracle(orc, rows, genes, ref, s3, "single")
        variants_equal(s3[0]["variants"], orc.call(rows, genes, refseq=ref))
        assert len(s3[0]["variants"]) >= 4
    finally:
        jl.close()


# The walk takes a chunk's list in batches of DEPTH rounds of 256 lanes x 4 entries: the batch edges are at 1024 x DEPTH entries.
# The register budget left the depth of the folded kernels at 8 (csrc/kernels_pileup.hip: JL_IX_FOLD_DEPTH), so these edges did
# not move; the edges of the two depths that were swept against it (2, 4) ride along, and the empty list and the list of one entry.
WALK_EDGES = [0, 1] + [1024 * d + k for d in (2, 4, 8) for k in (-1, 0, 1)]


def test_walk_batch_edges(orc):
    """One window, one plain chunk per length in WALK_EDGES: exactly that many reads deviate in the chunk's middle column.  60 000
    reads keep the longest list (8 193) under the density bound (9 plane_stride / 8 = 8 496 entries)."""
    n, l = 60000, 3 * len(WALK_EDGES)
    assert max(WALK_EDGES) <= 9 * ((n + 1023) // 1024 * 128) // 8
    rng = np.random.default_rng(5)
    ref = rng.integers(0, 4, l).astype(np.uint8)
    rows = np.tile(ref, (n, 1))
    for c, e in enumerate(WALK_EDGES):
        who = rng.choice(n, e, replace=False)
        rows[who, 3 * c + 1] = (ref[3 * c + 1] + 1 + (who % 3)) % 4   # three other codons, so the histogram atomics spread
    genes = ONE_FRAME(l)
    jl = capi.Juliet(0)
    try:
        jl.upload_rows(rows)
        s1, s3 = three_single_runs(jl, genes, ref)
        info = jl.index_info()
        assert info["indexed_chunks"] == len(WALK_EDGES) and info["entries"] == sum(WALK_EDGES), info
        assert_same(s1, s3, "walk edges")
        assert_oracle(orc, rows, genes, ref, s3, "walk edges")
    finally:
        jl.close()


@pytest.mark.parametrize("given_reference", [True, False])
def test_screen_none_and_exactly_one_lane(orc, given_reference):
    """Codon 0: every read carries the reference codon — no lane passes the screen, the wave writes an empty mask and leaves.
    Codon 1: 150 of 3 000 reads carry ONE other codon — exactly one lane passes, and is called.  Codon 2: one other codon seen
    once — one lane enters the Fisher stage and is not called.  With the reference given and with the majority codon as reference."""
    n, l = 3000, 9
    ref = np.array([0, 1, 2, 3, 2, 1, 1, 0, 3], dtype=np.uint8)
    rows = np.tile(ref, (n, 1))
    rows[:150, 4] = 0
    rows[200, 7] = 2
    genes = ONE_FRAME(l)
    refseq = ref if given_reference else None
    jl = capi.Juliet(0)
    try:
        jl.upload_rows(rows)
        s1, s3 = three_single_runs(jl, genes, refseq)
        assert_same(s1, s3, given_reference)
        exp_v = orc.call(rows, genes, refseq=refseq)
        assert len(exp_v) == 1 and exp_v[0]["codon_pos"] == 2 and exp_v[0]["count"] == 150
        for s in (s1, s3):
            variants_equal(s[0]["variants"], exp_v)
            assert (s[1]["hist"].sum(axis=1) == n).all() and [(h > 0).sum() for h in s[1]["hist"]] == [1, 2, 2]
    finally:
        jl.close()


def test_two_sided_tail(orc):
    """tail = 1: the two-sided test, the other branch of the Fisher stage — and of the screen, which lets h <= e through."""
    n, l = 5000, 60
    rows, ref = make_rows(n, l, seed=31)
    genes = ONE_FRAME(l)
    jl = capi.Juliet(0)
    try:
        jl.upload_rows(rows)
        s1, s3 = three_single_runs(jl, genes, ref, prm=capi.default_params(tail=1))
        assert_same(s1, s3, "tail")
        exp_v = orc.call(rows, genes, refseq=ref, params=oracle_lib.default_params(tail=1))
        assert len(exp_v) >= 4
        variants_equal(s3[0]["variants"], exp_v)
    finally:
        jl.close()


def test_drm_mask(orc):
    """A DRM mask: the screen drops the lanes the mask does not name before their p-value is asked for.  The mask keeps the first
    and the third of the window's variants."""
    n, l = 5000, 60
    rows, ref = make_rows(n, l, seed=32)
    genes = ONE_FRAME(l)
    all_v = orc.call(rows, genes, refseq=ref)
    assert len(all_v) >= 4
    mask = np.zeros(l // 3, dtype=np.uint64)
    for r in (all_v[0], all_v[2]):
        mask[r["codon_pos"] - 1] |= np.uint64(1) << np.uint64(r["codon"])
    keep = np.array([bool((mask[r["codon_pos"] - 1] >> np.uint64(r["codon"])) & np.uint64(1)) for r in all_v], dtype=bool)
    exp_v = all_v[keep]
    assert len(exp_v) == 2
    jl = capi.Juliet(0)
    try:
        jl.upload_rows(rows)
        s1, s3 = three_single_runs(jl, genes, ref, masks=mask)
        assert_same(s1, s3, "drm")
        variants_equal(s3[0]["variants"], exp_v)
        exp_p = orc.phase(rows, exp_v)
        assert s3[0]["phase"]["summary"] == exp_p["summary"] and (s3[0]["phase"]["read_hap"] == exp_p["read_hap"]).all()
    finally:
        jl.close()
