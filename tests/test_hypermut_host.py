"""The host-only half of the hypermutation screen (docs/SPEC.md §26): the numpy mirror on a matrix small enough to count by hand,
jl_hypermut_test against exact rational arithmetic over every small table and a designed family up to 3000 sites, jl_hypermut_filter
at its bound, and what the library exports and refuses.  No GPU: the library only has to load."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import hypermut_mirror as hm
from hypermut_tables import P_FLOOR, assert_p_close, designed_tables, exhaustive_tables, to_counts
from minorseq_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("jl_read_hypermut_async", "jl_read_hypermut_fetch", "jl_hypermut_eval", "jl_hypermut_test", "jl_hypermut_filter")


def host_eval(cnt):
    vals = [capi.hypermut_test(cnt[hm.TARGET_MUT, i], cnt[hm.TARGET_SITES, i], cnt[hm.CONTROL_MUT, i], cnt[hm.CONTROL_SITES, i]) for i in range(cnt.shape[1])]
    return np.array([v[0] for v in vals]), np.array([v[1] for v in vals])


# ---------------------------------------------------------------------------------------------- the mirror, counted by hand
def test_mirror_on_the_hand_counted_matrix():
    A, Cc, G, T = hm.A, hm.C, hm.G, hm.T
    ref = np.array([G, G, G, 0, G, 4, G, G], dtype=np.uint8)
    rows = np.array([
        [G, G, A, T, A, A, G, G],      # sites 0 (GGA target), 1 (GAT target), 2 (A,T,A control mut), 4 (AAG target mut); 6, 7: the last two
        [A, G, Cc, G, 4, A, A, A],     # 0: A G C -> control, mutated; 1: G C G control; 2: x = C no site; 4: gap
        [G, A, 5, G, G, 6, G, G],      # 0: z = N no site; 1: x = A, y = N no; 2: N; 4: y uncovered no site
        [A, A, A, A, A, A, A, A],      # 0, 1, 2, 4 target, all mutated; column 3 and 5: ref is no G
        [T, T, T, T, T, T, T, T],      # no purine anywhere
    ], dtype=np.uint8)
    got = hm.counts(rows, ref)
    assert got.dtype == np.uint32 and got.shape == (4, 5)
    assert got[hm.TARGET_SITES].tolist() == [3, 0, 0, 4, 0]
    assert got[hm.TARGET_MUT].tolist() == [1, 0, 0, 4, 0]
    assert got[hm.CONTROL_SITES].tolist() == [1, 2, 0, 0, 0]
    assert got[hm.CONTROL_MUT].tolist() == [1, 1, 0, 0, 0]
    assert not hm.counts(rows[:, :2], ref[:2]).any() and not hm.counts(rows[:, :1], ref[:1]).any()
    # the exact p of a table small enough to do by hand: [[2, 0], [0, 2]] -> 1 / C(4, 2)
    assert hm.exact_p(2, 2, 0, 2) == hm.Fraction(1, 6) and hm.exact_p(1, 2, 1, 2) == hm.Fraction(5, 6)
    assert hm.exact_p(0, 5, 3, 4) == 1 and hm.exact_p(0, 0, 2, 3) == 1 and hm.exact_p(2, 3, 0, 0) == 1
    idx, flagged = hm.keep([0.05, 0.049, 1.0, 0.0], 0.05)
    assert idx.tolist() == [0, 2] and flagged == 2


# ---------------------------------------------------------------------------------------------- jl_hypermut_test
def test_exports_and_layout():
    lib = capi.load_library()
    header = open(os.path.join(ROOT, "include", "juliet_hip.h")).read()
    declared = set(re.findall(r"\b(jl_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in NAMES:
        assert name in declared and name in capi.EXPORTS and name in exported and hasattr(lib, name), name
    assert "global: jl_*;" in open(os.path.join(ROOT, "minorseq_amd", "csrc", "exports.map")).read()
    assert lib.jl_abi_version() == 5          # additive: the ABI version stays
    m = re.search(r"enum \{ JL_HM_TARGET_SITES = (\d), JL_HM_TARGET_MUT = (\d), JL_HM_CONTROL_SITES = (\d), JL_HM_CONTROL_MUT = (\d), JL_HM_COUNTERS = (\d) \};", header)
    assert m and [int(x) for x in m.groups()] == [0, 1, 2, 3, 4]
    assert (capi.HM_TARGET_SITES, capi.HM_TARGET_MUT, capi.HM_CONTROL_SITES, capi.HM_CONTROL_MUT, capi.HM_COUNTERS) == (0, 1, 2, 3, 4)
    assert (hm.TARGET_SITES, hm.TARGET_MUT, hm.CONTROL_SITES, hm.CONTROL_MUT) == (0, 1, 2, 3)
    assert hasattr(capi.Juliet, "read_hypermut") and hasattr(capi.Juliet, "hypermut_eval") and callable(capi.hypermut_filter)


def test_every_small_table_against_exact_rationals():
    cnt = to_counts(exhaustive_tables())
    assert cnt.shape[1] == 91 * 91
    p, lp = host_eval(cnt)
    assert_p_close(p, lp, cnt)
    nothing = (cnt[hm.TARGET_SITES] == 0) | (cnt[hm.CONTROL_SITES] == 0) | (cnt[hm.TARGET_MUT] == 0)
    assert nothing.sum() > 1000 and (p[nothing] == 1.0).all() and (lp[nothing] == 0.0).all()      # exactly 1 and 0


def test_designed_tables_up_to_3000_sites():
    tables = designed_tables()
    assert max(t[1] for t in tables) == 3000 and max(t[3] for t in tables) == 3000
    cnt = to_counts(tables)
    p, lp = host_eval(cnt)
    exp_p = assert_p_close(p, lp, cnt)
    assert (exp_p < P_FLOOR).any() and (exp_p == 1.0).any() and ((exp_p > 1e-12) & (exp_p < 0.05)).any()      # both tails and the far end


def test_no_sites_and_no_mutations_are_exactly_one():
    for t in ((0, 0, 0, 0), (0, 0, 5, 9), (3, 7, 0, 0), (0, 7, 4, 4), (0, 3000, 3000, 3000), (0, 1, 0, 1)):
        assert capi.hypermut_test(*t) == (1.0, 0.0), t


def test_test_refusals():
    lib = capi.load_library()
    p, lp = C.c_double(7.0), C.c_double(7.0)
    assert lib.jl_hypermut_test(3, 2, 0, 5, C.byref(p), C.byref(lp)) == -1 and "more mutations than sites" in lib.jl_last_error(None).decode()
    assert lib.jl_hypermut_test(1, 2, 6, 5, C.byref(p), C.byref(lp)) == -1
    assert lib.jl_hypermut_test(1, 2, 1, 5, None, C.byref(lp)) == -1 and "NULL" in lib.jl_last_error(None).decode()
    assert lib.jl_hypermut_test(1, 2, 1, 5, C.byref(p), None) == -1
    assert (p.value, lp.value) == (7.0, 7.0)                                        # a refused call writes nothing
    with pytest.raises(capi.JulietError) as e:
        capi.hypermut_test(4, 3, 0, 1)
    assert e.value.status == -1


# ---------------------------------------------------------------------------------------------- jl_hypermut_filter
ALPHAS = (0.05, 0.01, 1e-6)


def test_filter_on_designed_tables_follows_the_exact_rule():
    """The p-values of the library's own test, the rule of the exact ones: no exact p is close enough to an alpha for the two to
    differ, which the test asserts rather than assumes."""
    tables = [t for t in exhaustive_tables() if t[1] >= 6 and t[3] >= 6] + designed_tables()
    cnt = to_counts(tables)
    p, _ = host_eval(cnt)
    exp_p, _, frs = hm.p_values(cnt)
    for alpha in ALPHAS:
        fa = hm.Fraction(alpha)
        assert all(abs(f - fa) > fa / 10**9 for f in frs), alpha
        idx, flagged = capi.hypermut_filter(p, alpha)
        exp_idx, exp_flagged = hm.keep(frs, fa)
        assert idx.dtype == np.uint32 and idx.tolist() == exp_idx.tolist() and flagged == exp_flagged, alpha
        assert 0 < flagged < len(tables)


def test_filter_is_strict_at_alpha():
    up, down = np.nextafter(0.05, 1.0), np.nextafter(0.05, 0.0)
    p = np.array([0.05, down, up, 0.0, 1.0, 0.05], dtype=np.float64)
    idx, flagged = capi.hypermut_filter(p, 0.05)
    assert idx.tolist() == [0, 2, 4, 5] and flagged == 2                            # p == alpha is kept
    assert (idx.tolist(), flagged) == (hm.keep(p, 0.05)[0].tolist(), hm.keep(p, 0.05)[1])
    # alpha = 1: only p = 1 is kept
    p = np.array([1.0, np.nextafter(1.0, 0.0), 0.5, 1.0, 0.0], dtype=np.float64)
    idx, flagged = capi.hypermut_filter(p, 1.0)
    assert idx.tolist() == [0, 3] and flagged == 3
    # all flagged, none flagged, no read
    idx, flagged = capi.hypermut_filter(np.full(9, 1e-9), 0.05)
    assert idx.tolist() == [] and flagged == 9
    idx, flagged = capi.hypermut_filter(np.full(9, 0.5), 0.05)
    assert idx.tolist() == list(range(9)) and flagged == 0
    idx, flagged = capi.hypermut_filter(np.zeros(0), 0.05)
    assert idx.tolist() == [] and flagged == 0


def test_filter_refusals():
    lib = capi.load_library()
    p = np.array([0.5, 0.001], dtype=np.float64)
    idx, kept, flagged = np.full(2, 77, dtype=np.uint32), C.c_uint64(99), C.c_uint64(98)

    def call(pp=p.ctypes.data, n=2, alpha=0.05, i=idx.ctypes.data, k=C.byref(kept), f=C.byref(flagged)):
        return lib.jl_hypermut_filter(pp, n, alpha, i, k, f)

    def refused(word, **kw):
        assert call(**kw) == -1
        assert word in lib.jl_last_error(None).decode(), lib.jl_last_error(None)
        assert idx.tolist() == [77, 77] and kept.value == 99 and flagged.value == 98      # a refused call writes nothing

    refused("NULL", pp=None)
    refused("NULL", i=None)
    refused("NULL", k=None)
    refused("NULL", f=None)
    for alpha in (0.0, -0.05, 1.0000001, float("nan"), float("inf")):
        refused("(0, 1]", alpha=alpha)
    refused("32 bits", n=2**32)
    assert call() == 0 and kept.value == 1 and flagged.value == 1 and idx[0] == 0
    with pytest.raises(capi.JulietError) as e:
        capi.hypermut_filter(p, 2.0)
    assert e.value.status == -1


def test_stage_refused_without_a_matrix():
    """With a device: a context without a matrix is a state error, and so is a fetch.  Without one no context exists, and the entry
    points refuse the NULL context."""
    lib = capi.load_library()
    ref = np.zeros(4, dtype=np.uint8)
    if lib.jl_device_count() > 0:
        j = capi.Juliet(0)
        assert lib.jl_read_hypermut_async(j.h, ref.ctypes.data) == -4 and "no resident matrix" in lib.jl_last_error(j.h).decode()
        assert lib.jl_read_hypermut_fetch(j.h, None, None, None) == -4
        j.close()
    else:
        with pytest.raises(capi.JulietError) as e:
            capi.Juliet(0)
        assert e.value.status == -2
        assert lib.jl_read_hypermut_async(None, ref.ctypes.data) == -1 and lib.jl_read_hypermut_fetch(None, None, None, None) == -1
        assert lib.jl_hypermut_eval(None, None, 0, None, None) == -1
