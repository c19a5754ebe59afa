"""The cigar rules of the record ingest (csrc/cigar_rules.h), compiled for the host: what an op consumes and shows, where an entry
begins, window columns, the verdict on a record and the long-read rule, at their edges — the functions cigar_walk_kernel,
cigar_runs_kernel and the upload's jl_ingest_read_is_long share.  The kernels on them: test_gpu_ingest_edges.py, test_gpu_parity.py
(test_device_ingest_*), test_gpu_qmask.py."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "cigar_rules_shim.cpp")
OPS = {"M": 0, "I": 1, "D": 2, "N": 3, "S": 4, "H": 5, "P": 6, "=": 7, "X": 8}
RUN_MASK = 2**30 - 1


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("shim") / "libcigar_rules_shim.so")
    subprocess.check_call(["g++", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-o", out, SRC])
    lib = C.CDLL(out)
    u32, u64, p32 = C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32)
    for name, args in (("shim_decode", [u32, u32]), ("shim_begins_entry", [u32, u32]), ("shim_verdict", [u32, u64, u64, u64, u64]),
                       ("shim_read_is_long", [p32, u64])):
        getattr(lib, name).restype = u32
        getattr(lib, name).argtypes = args
    lib.shim_window_col.restype = None
    lib.shim_window_col.argtypes = [C.c_int64, u64, u32, p32, p32]
    for name, args in (("shim_sentinels", [u32, u32, p32]), ("shim_entry_run", [u32, u32, u32, p32]), ("shim_limits", [p32, p32, p32])):
        getattr(lib, name).restype = None
        getattr(lib, name).argtypes = args
    return lib


def test_decode_of_all_sixteen_op_codes(shim):
    """D N = X consume the reference, I S = X the query; = X show aligned bases (kind 1), D a deletion (2), N nothing (3), the other
    twelve codes — M, the clips, the pad and the nine BAM does not define — no columns; zero length: no kind, the same consumption."""
    ref, qry, kind = {2, 3, 7, 8}, {1, 4, 7, 8}, {7: 1, 8: 1, 2: 2, 3: 3}
    for op in range(16):
        for ln in (0, 1, 2**28 - 1):
            exp = (op in ref) | (op in qry) << 1 | (kind.get(op, 0) if ln else 0) << 2
            assert shim.shim_decode(op, ln) == exp, (op, ln)


def test_begins_entry_over_all_pairs(shim):
    for kind in range(4):
        for prev in range(4):
            assert shim.shim_begins_entry(kind, prev) == (kind != 0 and not (kind == 1 and prev == 1)), (kind, prev)


def test_window_col_clamps_and_counts_what_lies_before(shim):
    n_cols = 1000
    col, before = C.c_uint32(), C.c_uint32()
    for w, exp in ((-2**32 - 1, (0, 2**32 - 1)), (-2**32, (0, 2**32 - 1)), (-2**32 + 1, (0, 2**32 - 1)), (-2**32 + 2, (0, 2**32 - 2)),
                   (-1, (0, 1)), (0, (0, 0)), (1, (1, 0)), (n_cols - 1, (n_cols - 1, 0)), (n_cols, (n_cols, 0)), (n_cols + 1, (n_cols, 0)),
                   (2**59, (n_cols, 0))):
        for ref in (0, 5, 2**31 + 3):               # base + ref = w, split three ways
            shim.shim_window_col(w - ref, ref, n_cols, C.byref(col), C.byref(before))
            assert (col.value, before.value) == exp, (w, ref)


def test_verdict_thresholds_and_precedence(shim):
    none = 2**64 - 1                                 # the quality length of a stream without qualities
    v = shim.shim_verdict
    assert v(0, 0, 0, 0, 0) == 0 and v(0, 0, 0, none, 0) == 0
    # 2: more bases than 2 x bytes hold, or 2^31 and more
    assert v(0, 200, 100, none, 5) == 0 and v(0, 201, 100, none, 5) == 2
    assert v(0, 2**31 - 1, 2**40, none, 5) == 0 and v(0, 2**31, 2**40, none, 5) == 2
    # 3: more qualities than the record holds
    assert v(0, 150, 100, 150, 5) == 0 and v(0, 151, 100, 150, 5) == 3
    # 4: a span of 2^30 reference bases or more
    assert v(0, 150, 100, 150, RUN_MASK) == 0 and v(0, 150, 100, 150, RUN_MASK + 1) == 4
    # the first that applies: M, bases, qualities, span
    assert v(1, 201, 100, 150, RUN_MASK + 1) == 1 and v(1, 0, 0, none, 0) == 1
    assert v(0, 201, 100, 150, RUN_MASK + 1) == 2
    assert v(0, 151, 100, 150, RUN_MASK + 1) == 3


def test_sentinel_entries_and_fields(shim):
    six, four = (C.c_uint32 * 6)(), (C.c_uint32 * 4)()
    shim.shim_sentinels(777, 4321, six)
    assert list(six) == [3 << 30, 0, 777 | 3 << 30, 4321, RUN_MASK | 3 << 30, 0]
    for col, kind, q in ((0, 1, 0), (RUN_MASK, 3, 2**32 - 1), (256, 2, 99)):
        shim.shim_entry_run(col, kind, q, four)
        assert list(four) == [col | kind << 30, q, col, kind]


def is_long(ops, walk_ops, walk_ent):
    """The rule in plain words: more than walk_ops ops, or runs + 3 more than walk_ent entries — a run: a stretch of = / X of
    length > 0 with nothing in between, or a D or an N of length > 0."""
    if len(ops) > walk_ops:
        return True
    runs, in_aligned = 0, False
    for op, ln in ops:
        if ln and op in "=X":
            runs += not in_aligned
            in_aligned = True
        else:
            runs += bool(ln and op in "DN")
            in_aligned = False
    return runs + 3 > walk_ent


def test_read_is_long_at_192_ops_and_37_runs(shim):
    a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    shim.shim_limits(C.byref(a), C.byref(b), C.byref(c))
    walk_ops, walk_ent = a.value, b.value
    assert (walk_ops, walk_ent, c.value) == (192, 40, RUN_MASK)

    def runs_ended_by(gap, n_runs):                  # n_runs aligned runs with `gap` between them
        return sum(([("=", 9), gap, ("X", 1)] for _ in range(n_runs - 1)), []) + [("=", 5)]

    cases = []
    for n_ops in (191, 192, 193):
        cases.append([("=", 2) if k % 2 == 0 else ("X", 1) for k in range(n_ops)])             # one run, whatever its ops
    for n_runs in (36, 37, 38):
        cases.append([("=", 10) if k % 2 == 0 else ("D", 1) for k in range(n_runs)])           # D and N are runs of their own
        cases.append([("=", 10) if k % 2 == 0 else ("N", 4) for k in range(n_runs)])
        for gap in (("I", 2), ("S", 1), ("H", 3), ("P", 1), ("D", 0), ("M", 1)):               # ... these only end one
            cases.append(runs_ended_by(gap, n_runs))
        cases.append([("=", 0), ("D", 0)] + runs_ended_by(("I", 1), n_runs) + [("N", 0)])      # zero-length ops begin nothing
    cases += [[], [("S", 5)], [("D", 1)] * 37, [("D", 1)] * 38, [("=", 1), ("I", 0)] * 37, [("=", 1), ("I", 0)] * 38]
    seen = set()
    for ops in cases:
        words = (C.c_uint32 * max(1, len(ops)))(*[(ln << 4) | OPS[op] for op, ln in ops])
        exp = is_long(ops, walk_ops, walk_ent)
        seen.add((len(ops) > walk_ops, exp))
        assert shim.shim_read_is_long(words, len(ops)) == exp, ops[:8]
    assert seen == {(False, False), (False, True), (True, True)}


def test_stand_alone_walk_under_sanitizers(tmp_path):
    """The same functions in a program of their own under AddressSanitizer and UndefinedBehaviorSanitizer: every op code, the shifts
    of the tables, the 64-bit sums at their ends, cigar lists read to exactly their last word."""
    exe = str(tmp_path / "cigar_rules_walk")
    subprocess.check_call(["g++", "-O1", "-g", "-DSHIM_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "cigar rules walked" in r.stdout, r.stderr
