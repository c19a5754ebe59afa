"""The count tables of the hypermutation test's domain checks (docs/SPEC.md §26) and their comparison with exact rational
arithmetic (tests/hypermut_mirror.py), shared by the host routine's test (tests/test_hypermut_host.py) and the device kernel's
(tests/test_gpu_hypermut.py)."""
import numpy as np

import hypermut_mirror as hm

# the project's own bounds for jl_fisher_greater_general (tests/test_gpu_control.py)
P_REL_TOL, P_FLOOR = 5e-12, 1e-300


def exhaustive_tables():
    """Every table with n, m <= 12: (a, n, c, m)."""
    return [(a, n, c, m) for n in range(13) for m in range(13) for a in range(n + 1) for c in range(m + 1)]


def designed_tables():
    """Sites up to 3000: the mutation fraction equal in both rows, all mutations in the target, all in the control, a at both ends."""
    out = []
    sizes = (13, 100, 640, 3000)
    for n in sizes:
        for m in sizes:
            for num, den in ((1, 100), (1, 10), (1, 2), (9, 10)):
                out.append((n * num // den, n, m * num // den, m))            # the same fraction in both rows
            for k in (1, 7, min(n, m) // 2, min(n, m)):
                out.append((k, n, 0, m))                                     # all in the target
                out.append((0, n, k, m))                                     # all in the control
            for c in (0, m // 3, m):
                out.append((0, n, c, m))                                     # a at both ends
                out.append((n, n, c, m))
            out.append((n // 2 + 1, n, m // 2, m))                           # just above and just below the mean
            out.append((max(n // 2 - 1, 0), n, m // 2, m))
    return sorted(set(out))


def to_counts(tables):
    t = np.array(tables, dtype=np.uint32).reshape(-1, 4)
    return np.ascontiguousarray(np.stack([t[:, 1], t[:, 0], t[:, 3], t[:, 2]]))      # sites, mut, sites, mut


def assert_p_close(got_p, got_lp, cnt):
    """(p, log_p) of counts[4, n] against the exact rationals; prints the largest deviations before it asserts."""
    exp_p, exp_lp, _ = hm.p_values(cnt)
    got_p, got_lp = np.asarray(got_p), np.asarray(got_lp)
    big = exp_p >= P_FLOOR
    rel = np.abs(got_p[big] - exp_p[big]) / exp_p[big]
    dl = np.abs(got_lp - exp_lp) - (1e-12 * np.maximum(1.0, np.abs(exp_lp)) + 1e-13)
    print("tables %d  max rel dp %.3g  max (|d log_p| - bound) %.3g" % (cnt.shape[1], rel.max() if rel.size else 0.0, dl.max()))
    assert (rel <= P_REL_TOL).all(), np.argwhere(rel > P_REL_TOL)[:4]
    assert (np.abs(got_p[~big] - exp_p[~big]) <= P_FLOOR).all()
    assert (dl <= 0.0).all(), np.argwhere(dl > 0.0)[:4]
    return exp_p
