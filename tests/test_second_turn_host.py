"""The property tests/second_turn.py rests on, against the mirrors run in full: for rows that are a block repeated with a tail, the
per-read outputs of the three hap-walk stages are the block's, tiled, and every count is the block's times the repeats plus the
tail's — at 3 x 2049 + 1 reads, for the shapes of the second-turn cases.  And the second-turn cases hold what they claim."""
import numpy as np
import pytest

import nearest_mirror
import recombinant_mirror
import rescue_mirror
import second_turn as st
import test_gpu_nearest as tn
import test_gpu_recombinant as tr
import test_gpu_rescue as ts

N = 3 * 2049 + 1


def block_of(module, vp, n_hap):
    """The module's 2049-read case, whole: the block of the property (any length tiles; only the planes need a multiple of 8)."""
    if module is tn:
        return module.make_case(2049, vp, n_hap, tn.SECOND_TURN_D, tn.seed_of(2049, vp, n_hap, tn.SECOND_TURN_D))
    return module.make_case(2049, vp, n_hap, 1000 * 2049 + 7 * vp + n_hap)


@pytest.mark.parametrize("vp,n_hap", ts.SECOND_TURN_SHAPES)
def test_rescue_of_tiled_rows_is_the_tiled_rescue(vp, n_hap):
    block, pos_cols, pattern = block_of(ts, vp, n_hap)
    full = rescue_mirror.rescue(st.tiled_rows(block, N), pos_cols, pattern, 1)
    whole, tail = rescue_mirror.rescue(block, pos_cols, pattern, 1), rescue_mirror.rescue(block[:1], pos_cols, pattern, 1)
    assert st.split(N, 2049) == (3, 1)
    assert (full[0] == st.tiled(whole[0], N)).all()
    for k in (1, 2):
        assert (full[k] == st.summed(whole[k], tail[k], N, 2049)).all()


@pytest.mark.parametrize("vp,n_hap", tn.SECOND_TURN_SHAPES)
def test_nearest_of_tiled_rows_is_the_tiled_nearest(vp, n_hap):
    block, pos_cols, pattern = block_of(tn, vp, n_hap)
    d = tn.SECOND_TURN_D
    full = nearest_mirror.nearest(st.tiled_rows(block, N), pos_cols, pattern, 1, d)
    whole, tail = nearest_mirror.nearest(block, pos_cols, pattern, 1, d), nearest_mirror.nearest(block[:1], pos_cols, pattern, 1, d)
    for k in (0, 1):
        assert (full[k] == st.tiled(whole[k], N)).all()
    for k in (2, 3):
        assert (full[k] == st.summed(whole[k], tail[k], N, 2049)).all()


@pytest.mark.parametrize("vp,n_hap", tr.SECOND_TURN_SHAPES)
def test_recombinants_of_tiled_rows_are_the_tiled_recombinants(vp, n_hap):
    block, pos_cols, pattern = block_of(tr, vp, n_hap)
    full = recombinant_mirror.recombinants(st.tiled_rows(block, N), pos_cols, pattern, 1)
    whole, tail = recombinant_mirror.recombinants(block, pos_cols, pattern, 1), recombinant_mirror.recombinants(block[:1], pos_cols, pattern, 1)
    for key in ("left", "right", "prefix", "suffix"):
        assert (full[key] == st.tiled(whole[key], N)).all(), key
    for key in ("parent_reads", "tally"):
        assert (full[key] == st.summed(whole[key], tail[key], N, 2049)).all(), key


def test_the_counts_are_the_turns_they_claim():
    runs = [-(-n // st.RUN) for n, _ in st.COUNTS]
    assert runs == [4096, 4097, 4160] and st.GRID_CAP == 4096
    n = st.COUNTS[2][0]
    assert runs[2] - st.GRID_CAP == 64 and n % st.RUN == 1                 # workgroups 0 .. 63 walk twice, 64 once; the last run holds one read
    assert n - st.ONE_TURN == 4033 and st.split(n) == (130, 977)
    # a lane's second turn holds other rows than its first
    assert all((st.ONE_TURN + i) % st.BLOCK != i % st.BLOCK for i in (0, 63, 4032))


@pytest.mark.parametrize("vp,n_hap", ts.SECOND_TURN_SHAPES)
def test_second_turn_reads_hold_every_category(vp, n_hap):
    """What the GPU cases assert of the mirror before they look at the device, without one."""
    n = st.COUNTS[2][0]
    late = st.second_turn_reads(n)
    r = ts.second_turn_expectation(*ts.second_turn_block(vp, n_hap), n)[0][late]
    assert (r < n_hap).any() and (r == rescue_mirror.AMBIGUOUS).any() and (r == rescue_mirror.NONE).any() and (r == rescue_mirror.UNINFORMATIVE).any()
    e = tn.second_turn_expectation(*tn.second_turn_block(vp, n_hap), n)
    near, dist = e[0][late], e[1][late]
    assert (near < n_hap).any() and (near == tn.AMB).any() and (near == tn.NONE).any() and (near == tn.U).any()
    assert set(dist[near < n_hap].tolist()) == set(range(tn.SECOND_TURN_D + 1))
    e = tr.second_turn_expectation(*tr.second_turn_block(vp, n_hap), n)
    got = tr.outcomes({key: e[key][late] for key in ("left", "right")}, n_hap)
    assert all(o in got for o in "BWNU"), got
