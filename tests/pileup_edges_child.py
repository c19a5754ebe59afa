"""Child process of tests/test_gpu_pileup_edges.py (not a test module: the read-out of the launch shape is in the -DJL_TUNING
build of the library, and the form of a group launch depends on the process's environment).

    python pileup_edges_child.py PART        PART: a key of pileup_edges.PARTS, or `wide`
    JL_LIB: the library to load (the -DJL_TUNING build: jl_tuning_pileup_shape, jl_tuning_group_forms)
    JL_EXPECT_FORM: folded | unfolded — the form the group launches must take (unfolded: the parent sets JL_NO_FOLD_CALL=1)
    JL_EDGES_KEEP_GOING=1: report every failing case instead of stopping at the first

folded: every case through the stage API (twice in a row, with the reference, with a reference that differs in every base and in
majority mode), through a single run, and through a group run beside a shallower window.  unfolded: the group run only (the
single launches do not depend on the form).  One context is reused by all cases of a part, depths shrinking and growing.
Prints `TAKEN kernel W NQ stream multi` for every form a launch took, then EDGES-OK as its last line."""
import ctypes as C
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

if len(sys.argv) > 1 and sys.argv[1] == "wide":
    import torch  # noqa: F401, E402  (before the library: tests/conftest.py)

import pileup_edges as pe  # noqa: E402
from minorseq_amd import capi, msa  # noqa: E402

FIELDS = ("w", "nq", "tiles", "nq_group", "tiles_group", "n_chunks", "rsplit", "can_fold", "blocks_per_cu", "n_fast", "n_halo",
          "flush")
FOLDED = os.environ.get("JL_EXPECT_FORM", "folded") == "folded"
KEEP_GOING = os.environ.get("JL_EDGES_KEEP_GOING") == "1"
failures = []


def shape_of(lib, j):
    out = (C.c_uint32 * len(FIELDS))()
    rc = lib.jl_tuning_pileup_shape(j.h, out)
    assert rc == 0, rc
    return dict(zip(FIELDS, (int(x) for x in out)))


def group_forms(lib):
    f, u = C.c_uint64(), C.c_uint64()
    lib.jl_tuning_group_forms(C.byref(f), C.byref(u))
    return int(f.value), int(u.value)


def check(what, got, exp):
    """col_counts, hist and coverage bit for bit; a mismatch names the first columns and symbols that differ."""
    for k in ("col_counts", "hist", "coverage"):
        if got[k].shape != exp[k].shape or not (got[k] == exp[k]).all():
            at = np.argwhere(got[k] != exp[k])[:4].tolist() if got[k].shape == exp[k].shape else "shape"
            msg = "%s: %s differs at %s: got %s, expected %s" % (what, k, at, [int(got[k][tuple(a)]) for a in at] if at != "shape" else got[k].shape,
                                                                 [int(exp[k][tuple(a)]) for a in at] if at != "shape" else exp[k].shape)
            if not KEEP_GOING:
                raise AssertionError(msg)
            failures.append(msg)
            print("FAIL", msg, flush=True)
            return


def streams_of(s):
    return (["fast"] if s["n_fast"] else []) + (["general"] if s["n_fast"] < s["n_chunks"] else [])


def batches(tiles, split, flush):
    per_block = -(-tiles // split)
    return -(-per_block // flush)


def run_window(lib, j, comp, genes, ref, exp, exp_comp, name, intent, taken):
    """One resident window (and its resident companion) through every path; `intent`: the read-out fields the case was designed
    for."""
    prm = capi.default_params(max_perc=0.0)    # the call stage is not under test: nothing is called, its tables stay empty
    if FOLDED:
        for label, refseq in pe.reference_modes(ref):
            for rep in range(2):           # twice in a row: an added total that is not zeroed again would double
                j.pileup_async(genes, refseq)
                check("%s stage %s #%d" % (name, label, rep), j.pileup_fetch(), exp)
        s = shape_of(lib, j)
        for k, v in intent.items():
            assert s[k] == v, (name, k, s[k], v, s)
        assert 1 <= s["rsplit"] <= s["tiles"] and s["can_fold"] == (s["rsplit"] == 1), (name, s)
        taken |= pe.taken("plain", s["w"], s["nq"], streams_of(s), batches(s["tiles"], s["rsplit"], s["flush"]))
        j.run_async(genes, ref, prm, None, False, 10, False)
        j.run_wait()
        check(name + " run", j.pileup_fetch(), exp)
        if s["can_fold"]:
            taken |= pe.taken("fold", s["w"], s["nq"], streams_of(s), batches(s["tiles"], 1, s["flush"]))
    if comp is None:
        return
    before = group_forms(lib)
    grp = capi.Group([j, comp])
    for rep in range(2):                   # (the second launch replays the captured graph)
        grp.run_async(genes, ref, prm, False, 10, False)
        for c, e, who in ((j, exp, "window"), (comp, exp_comp, "companion")):
            c.run_wait()
            check("%s group %s #%d" % (name, who, rep), c.pileup_fetch(), e)
    grp.close()
    after = group_forms(lib)
    assert (after[0] - before[0], after[1] - before[1]) == ((2, 0) if FOLDED else (0, 2)), (name, before, after)
    s = shape_of(lib, j)
    taken |= pe.taken("fold_group" if FOLDED else "group", s["w"], s["nq_group"], streams_of(s),
                      batches(s["tiles_group"], 1, pe.flush_tiles(s["nq_group"])))


def run_part(lib, part):
    cases = sorted(pe.PARTS[part], key=lambda c: c.n)
    order = [cases[i // 2] if i % 2 == 0 else cases[-1 - i // 2] for i in range(len(cases))]   # depths shrink and grow
    j, comp = capi.Juliet(0), capi.Juliet(0)
    taken, expect = set(), set()
    for c in order:
        t0 = time.time()
        rows, ref = c.build()
        comp_rows = c.companion(ref)
        j.upload_rows(rows)
        comp.upload_rows(comp_rows)
        nq = pe.single_nq(c.w, c.n)
        tiles = pe.tiling(c.n, nq)[0]
        chunks = c.plan["chunks"]
        intent = dict(w=c.w, nq=nq, tiles=tiles, nq_group=pe.group_nq(c.w), tiles_group=pe.tiling(c.n, pe.group_nq(c.w))[0],
                      n_chunks=len(chunks), n_fast=sum(ch[4] for ch in chunks), n_halo=sum(ch[3] for ch in chunks),
                      rsplit=tiles)       # so few chunks that a single run gives every tile a workgroup of its own
        run_window(lib, j, comp, c.genes, ref, c.expected(rows), window_expected(comp_rows, c), c.name, intent, taken)
        expect |= pe.case_forms(c, FOLDED)
        print("case %s %.2f s" % (c.name, time.time() - t0), flush=True)
    j.close()
    comp.close()
    assert KEEP_GOING or taken == expect, (sorted(taken - expect), sorted(expect - taken))
    return taken


def window_expected(rows, c):
    return pe.window_counts(rows, c.plan["pos_col"])


def run_wide(lib):
    """Single runs that count a chunk with one workgroup (or two) over more tiles than a flush batch holds."""
    import torch
    taken, expect = set(), set()
    for layout, n, rsplit in pe.WIDE:
        t0 = time.time()
        block, ref_block = pe.contents("mixture", n, pe.WIDE_BLOCK, 1000 + n % 997 + rsplit)
        # the occupancy of this depth's kernel, from a window of the block alone
        probe = capi.Juliet(0)
        probe.upload_rows(block)
        probe.pileup_async(pe.wide_genes(layout, pe.WIDE_BLOCK), ref_block)
        s0 = shape_of(lib, probe)
        probe.close()
        l = pe.wide_columns(layout, s0["blocks_per_cu"], s0["tiles"], rsplit)
        reps = -(-l // pe.WIDE_BLOCK)
        genes = pe.wide_genes(layout, l)
        plan = pe.plan(genes, l)
        ref = np.tile(ref_block, reps)[:l]
        t = torch.from_numpy(msa.pack_planes(block)).cuda().repeat(reps, 1, 1)[:l].contiguous()
        torch.cuda.synchronize()
        j = capi.Juliet(0)
        j.adopt(t.data_ptr(), n, l, msa.plane_stride(n), keep_alive=t)
        w = 6 if layout == "six" else 3
        nq = pe.single_nq(w, n)
        intent = dict(w=w, nq=nq, tiles=pe.tiling(n, nq)[0], n_chunks=len(plan["chunks"]), rsplit=rsplit,
                      n_fast=sum(ch[4] for ch in plan["chunks"]), n_halo=sum(ch[3] for ch in plan["chunks"]))
        name = "wide-%s-%dx%d-split%d" % (layout, n, l, rsplit)
        run_window(lib, j, None, genes, ref, pe.window_counts(block, plan["pos_col"], l), None, name, intent, taken)
        expect |= pe.wide_forms(layout, n, rsplit, FOLDED)
        j.close()
        del t
        print("case %s %.2f s" % (name, time.time() - t0), flush=True)
    assert KEEP_GOING or taken == expect, (sorted(taken - expect), sorted(expect - taken))
    return taken


def main():
    lib = capi.load_library(os.environ["JL_LIB"])
    lib.jl_tuning_group_forms.restype = None
    lib.jl_tuning_pileup_shape.restype = C.c_int
    lib.jl_tuning_pileup_shape.argtypes = [C.c_void_p, C.c_void_p]
    t0 = time.time()
    part = sys.argv[1]
    taken = run_wide(lib) if part == "wide" else run_part(lib, part)
    for k in sorted(taken):
        print("TAKEN %s %d %d %s %d" % k)
    print("part %s %.2f s" % (part, time.time() - t0))
    if failures:
        print("EDGES-FAILED", len(failures))
        sys.exit(1)
    print("EDGES-OK", part, "folded" if FOLDED else "unfolded")


if __name__ == "__main__":
    main()
