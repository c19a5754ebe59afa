"""Child process of tests/test_gpu_group_forms.py (not a test module: the form of a group launch depends on the
process's environment and on the library build, so each scenario runs in a process of its own).

    python group_forms_child.py SCENARIO       SCENARIO: forms | switch | hook
    JL_LIB: the library to load (the -DJL_TUNING build, whose jl_tuning_group_forms counts the forms taken)
    JL_EXPECT_FORM: folded | unfolded — the form every launch of `forms` must take

Prints FORMS-OK / SWITCH-OK / HOOK-OK as its last line.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import oracle_lib  # noqa: E402
from minorseq_amd import capi, msa, synth  # noqa: E402

P_ABS_TOL = 1e-10     # as tests/test_gpu_parity.py
LOGP_REL_TOL = 1e-9


def variants_equal(got, exp, exact_p=False):
    assert len(got) == len(exp), (len(got), len(exp))
    for k in ("gene", "codon_pos", "col", "ref_codon", "codon", "count", "coverage", "expected"):
        assert (got[k] == exp[k]).all(), k
    if exact_p:   # against a single run of the same library: the same bits
        assert (got["p_value"] == exp["p_value"]).all() and (got["log_p"] == exp["log_p"]).all()
        return
    assert np.abs(got["p_value"] - exp["p_value"]).max(initial=0.0) <= P_ABS_TOL
    fin = np.isfinite(exp["log_p"])
    assert (np.isfinite(got["log_p"]) == fin).all()
    if fin.any():
        rel = np.abs(got["log_p"][fin] - exp["log_p"][fin]) / np.maximum(1.0, np.abs(exp["log_p"][fin]))
        assert rel.max() <= LOGP_REL_TOL


def phase_equal(got, exp, n_var):
    assert got["summary"] == exp["summary"], (got["summary"], exp["summary"])
    h = exp["summary"]["n_haplotypes"]
    assert (np.asarray(got["pos_cols"]) == exp["pos_cols"]).all()
    assert (np.asarray(got["hap_count"]) == exp["hap_count"]).all()
    assert (np.asarray(got["hap_pattern"]) == exp["hap_pattern"]).all()
    assert (np.asarray(got["hit"])[:n_var, :h] == np.asarray(exp["hit"])[:n_var, :h]).all()
    assert (np.asarray(got["read_hap"]) == np.asarray(exp["read_hap"])).all()


def forms_taken(lib):
    f, u = C.c_uint64(), C.c_uint64()
    lib.jl_tuning_group_forms(C.byref(f), C.byref(u))
    return int(f.value), int(u.value)


def make_windows(n_win, l, seed0, with_plain=True, n0=2500):
    """n_win windows of different depth over one reference; window 1 (if any) holds the reference only: no variant."""
    ref = synth.reference(seed0, l)
    wins = []
    for k in range(n_win):
        n = n0 + 1111 * k
        j = capi.Juliet(0)
        if with_plain and k == 1:
            rows = np.tile(ref, (n, 1)).astype(np.uint8)
            j.upload_columns(msa.pack_columns(rows), n)
            j.sync()
        else:   # generated on the device (the numpy mirror of the generator is slow at the sizes of `switch`)
            j.alloc(n, l)
            j.synth_fill(synth.SynthParams(seed=seed0 + k, minor_permille=(70, 50, 40, 30), partial_rate=0.03 * (k % 4)), ref)
            j.sync()
            rows = msa.unpack_columns(j.download_columns(), n)
        wins.append((j, rows))
    return ref, wins


def check_window(j, exp_v, exp_p, single, phasing):
    """The window's results of the group run: run view and copying fetch, against the oracle and the single run."""
    v = j.run_view()
    assert v is not None
    f = j.run_fetch(phasing, True, cap_var=64)
    for got in (v, f):
        variants_equal(got["variants"], exp_v)
        variants_equal(got["variants"], single["variants"], exact_p=True)
        if phasing:
            phase_equal(got["phase"], exp_p, len(exp_v))
            phase_equal(got["phase"], single["phase"], len(exp_v))


def scenario_forms(lib, orc):
    expect = os.environ["JL_EXPECT_FORM"]
    l = 240
    genes = np.array([(1, l + 1)], dtype=capi.GENE)
    prm = capi.default_params()
    launches = 0
    for n_win in (1, 3, 8):
        ref, wins = make_windows(n_win, l, 700 + 10 * n_win)
        exp = []
        for j, rows in wins:
            ev = orc.call(rows, genes, refseq=ref)
            exp.append((ev, orc.phase(rows, ev)))
        if n_win > 1:
            assert len(exp[1][0]) == 0      # the window without any variant
        for phasing in (True, False):
            single = [j.run(genes, ref, prm, None, phasing) for j, _ in wins]   # jl_run_async on each window alone
            grp = capi.Group([j for j, _ in wins])
            for rep in range(3):            # the second and third launch replay the form's captured graph
                grp.run_async(genes, ref, prm, phasing, 10, True)
                launches += 1
                for (j, _), (ev, ep), s in zip(wins, exp, single):
                    check_window(j, ev, ep, s, phasing)
            grp.close()
        if n_win == 3:
            # per-window DRM masks (--drm-only): window 0 keeps its first two variants, window 1 has no mask, window 2 keeps one
            masks = [None] * n_win
            kept = []
            for k in (0, 2):
                ev = exp[k][0]
                m = np.zeros(l // 3, dtype=np.uint64)
                for r in ev[:2 if k == 0 else 1]:
                    m[r["codon_pos"] - 1] |= np.uint64(1) << np.uint64(r["codon"])
                masks[k] = m
            for k, (j, rows) in enumerate(wins):
                ev = exp[k][0]
                if masks[k] is not None:
                    keep = np.array([bool((masks[k][r["codon_pos"] - 1] >> np.uint64(r["codon"])) & np.uint64(1)) for r in ev], dtype=bool)
                    ev = ev[keep]
                    assert 0 < len(ev) < len(exp[k][0])
                kept.append((ev, orc.phase(rows, ev)))
            single = [j.run(genes, ref, prm, masks[k], True) for k, (j, _) in enumerate(wins)]
            grp = capi.Group([j for j, _ in wins])
            for rep in range(2):
                grp.run_masked_async(genes, ref, prm, masks, True, 10, True)
                launches += 1
                for (j, _), (ev, ep), s in zip(wins, kept, single):
                    check_window(j, ev, ep, s, True)
            grp.close()
        for j, _ in wins:
            j.close()
    folded, unfolded = forms_taken(lib)
    assert (folded, unfolded) == ((launches, 0) if expect == "folded" else (0, launches)), (expect, launches, folded, unfolded)
    print("FORMS-OK", expect, launches)


def scenario_switch(lib, orc):
    """Five groups of different reads (two windows of 300k reads x 1200 columns each) launched back to back without
    collecting, collected in launch order; then the same five one at a time, each collected before the next is launched."""
    l = 1200
    genes = np.array([(1, l + 1)], dtype=capi.GENE)
    prm = capi.default_params()
    groups = []
    for g in range(5):
        ref, wins = make_windows(2, l, 900 + 17 * g, with_plain=(g == 2), n0=300_000)
        exp, single = [], []
        for j, rows in wins:
            ev = orc.call(rows, genes, refseq=ref)
            exp.append((ev, orc.phase(rows, ev)))
            single.append(j.run(genes, ref, prm, None, True))
        groups.append((capi.Group([j for j, _ in wins]), ref, wins, exp, single))
    assert forms_taken(lib) == (0, 0)

    def collect(g):
        grp, ref, wins, exp, single = g
        vw = grp.views()
        assert vw["complete"].all()
        for (j, _), (ev, ep), s in zip(wins, exp, single):
            check_window(j, ev, ep, s, True)

    for rnd in range(3):      # (a form's first launch captures its graph; later rounds replay it)
        # back to back: what a launch finds in flight depends on the device's speed, so the forms of this part are not
        # asserted one by one — only that every result is right whatever was taken
        for g in groups:
            g[0].run_async(genes, g[1], prm, True, 10, True)
        for g in groups:
            collect(g)
        f0, u0 = forms_taken(lib)
        assert f0 + u0 == 10 * rnd + 5
        # one at a time: nothing of the device's other groups is in flight at any enqueue, so every launch is folded
        for g in groups:
            g[0].run_async(genes, g[1], prm, True, 10, True)
            collect(g)
        f1, u1 = forms_taken(lib)
        assert (f1 - f0, u1 - u0) == (5, 0), (f0, u0, f1, u1)
    folded, unfolded = forms_taken(lib)
    # Both forms were in fact taken.  Folded: shown above, launch by launch.  Unfolded: the fourth and fifth launch of a back-to-back
    # round find three launches incomplete unless the device finishes a launch over 270 MB of planes (43 us at the HBM peak, plus
    # its latency-bound tail) sooner than the host enqueues three more (about 10 us each).  That is the one thing here that
    # leans on the device at all — it asks for one such launch among the four of rounds two and three (the first round's launches
    # capture their graphs, milliseconds each, and find nothing in flight), and no result depends on it.
    print("forms taken: folded %d, unfolded %d" % (folded, unfolded))
    assert folded >= 15 and unfolded >= 1, (folded, unfolded)
    for grp, ref, wins, exp, single in groups:
        grp.close()
        for j, _ in wins:
            j.close()
    print("SWITCH-OK", folded, unfolded)


def ctx_meta(lib, j):
    buf = (C.c_uint8 * 256)()
    n = lib.jl_tuning_ctx_meta(j.h, buf, 256)
    assert n > 0, n
    return bytes(buf[:n])


def scenario_hook(lib, orc):
    """jl_group_time_pileup between a group run and the reading of its results: it must not touch anything of the run — the
    device's run counters (n_occupied, the overflow bits, the summary: what a relaunch of the folded kernel would zero), the
    tables behind jl_call_fetch / jl_phase_fetch, the result blocks behind jl_group_views and the run views."""
    l = 300
    genes = np.array([(1, l + 1)], dtype=capi.GENE)
    prm = capi.default_params()
    ref, wins = make_windows(3, l, 611)
    exp, single = [], []
    for j, rows in wins:
        ev = orc.call(rows, genes, refseq=ref)
        exp.append((ev, orc.phase(rows, ev)))
        single.append(j.run(genes, ref, prm, None, True))
    grp = capi.Group([j for j, _ in wins])
    for rep in range(2):
        grp.run_async(genes, ref, prm, True, 10, True)
        vw = grp.views()
        before = [int(x) for x in vw["n_variants"]]
        meta = [ctx_meta(lib, j) for j, _ in wins]
        assert any(any(m) for m in meta)      # (a run leaves a summary: the words are not all zero)
        ms, nbytes = capi.time_pileup_groups([grp], reps=5)
        assert ms > 0.0 and nbytes == sum(len(rows) * l * 3 // 8 for _, rows in wins)
        assert [ctx_meta(lib, j) for j, _ in wins] == meta
        vw = grp.views()
        assert vw["complete"].all() and vw["phased"].all() and [int(x) for x in vw["n_variants"]] == before
        for (j, _), (ev, ep), s in zip(wins, exp, single):
            check_window(j, ev, ep, s, True)
    grp.close()
    for j, _ in wins:
        j.close()
    print("HOOK-OK")


def main():
    lib = capi.load_library(os.environ["JL_LIB"])
    lib.jl_tuning_group_forms.restype = None
    lib.jl_tuning_ctx_meta.restype = C.c_int
    lib.jl_tuning_ctx_meta.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    orc = oracle_lib.load()
    {"forms": scenario_forms, "switch": scenario_switch, "hook": scenario_hook}[sys.argv[1]](lib, orc)


if __name__ == "__main__":
    main()
