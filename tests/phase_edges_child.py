"""Child process of tests/test_gpu_phase_edges.py (not a test module: which pipeline phased a context is read from the
-DJL_TUNING build of the library, and a process loads one library).

    python phase_edges_child.py PART        PART: a key of phase_edges.PARTS, or `growth`
    JL_LIB: the library to load (the -DJL_TUNING build: jl_tuning_ctx_meta, jl_tuning_phase_form, jl_tuning_group_ids_inline)

Every case of the part goes through the stage API on a fresh context (phase_async with its host table, phase_fetch) and, with the
table the call stage gives for its matrix, through the whole-path run and through group runs of three windows — a window without
variants, the case, a different window — once with a launch that writes the per-read ids itself and once with one that leaves
them to the separate launch (phase_edges.NO_WHOLE_PATH and NO_GROUP name the few cases that cannot, and why).  Every field and every read's id is compared with the numpy statement by ==; the pipeline that ran, its key
words, the positions it found, its overflow bits and the width of its ids are read from the library and asserted.
Prints `COMPARED name entries` per case, then PHASE-EDGES-OK as its last line."""
import ctypes as C
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import phase_edges as pe  # noqa: E402
from minorseq_amd import capi, msa  # noqa: E402

META = ("n_var", "vp", "kwords", "n_occupied", "overflow", "vp_true", "id_bits")
OVF_CANDIDATES, OVF_HAPLOTYPES = 1, 2     # jl_internal.h: JL_PHASE_OVF_CANDIDATES, JL_PHASE_OVF_HAPLOTYPES
LOOSE = capi.default_params(alpha=0.9, n_tests=1.0)


def ctx_meta(lib, j):
    buf = (C.c_uint8 * 256)()
    n = lib.jl_tuning_ctx_meta(j.h, buf, 256)
    assert n >= 4 * len(META), n
    return dict(zip(META, (int(x) for x in np.frombuffer(bytes(buf[:4 * len(META)]), dtype=np.uint32))))


def phase_form(lib, j):
    out = (C.c_uint32 * 4)()
    assert lib.jl_tuning_phase_form(j.h, out) == 0
    return dict(form=int(out[0]), keys_words=int(out[1]), blocks=int(out[2]), inline=int(out[3]))


def fetch(j, nv):
    """jl_phase_fetch with its status: (rc, results as capi.Juliet.phase_fetch gives them)."""
    cap = max(1, nv)
    summ = np.zeros(1, dtype=capi.SUMMARY)
    pos_cols = np.zeros(cap, dtype=np.uint32)
    hap_count = np.zeros(capi.MAX_HAPLOTYPES, dtype=np.uint32)
    hap_pattern = np.zeros((capi.MAX_HAPLOTYPES, cap), dtype=np.uint8)
    hit = np.zeros((cap, capi.MAX_HAPLOTYPES), dtype=np.uint8)
    read_hap = np.zeros(j.n_reads, dtype=np.uint16)
    cooc = np.zeros((cap, cap), dtype=np.uint32)
    p = capi._p
    rc = j.lib.jl_phase_fetch(j.h, p(summ), p(pos_cols), p(hap_count), p(hap_pattern), p(hit), p(read_hap), p(cooc), cap)
    s = {k: int(summ[0][k]) for k in capi.SUMMARY_FIELDS}
    h, vp = s["n_haplotypes"], s["n_positions"]
    return rc, dict(summary=s, pos_cols=pos_cols[:vp].copy(), hap_count=hap_count[:h].copy(), hap_pattern=hap_pattern[:h, :vp].copy(),
                    hit=hit[:nv, :h].copy(), read_hap=read_hap, cooc=cooc[:nv, :nv].copy())


def same(what, got, exp, nv):
    """Every field and every read's id, by ==."""
    assert got["summary"] == exp["summary"], (what, got["summary"], exp["summary"])
    h = exp["summary"]["n_haplotypes"]
    for k in ("pos_cols", "hap_count", "hap_pattern"):
        g = np.asarray(got[k])
        assert g.shape == exp[k].shape and (g == exp[k]).all(), (what, k)
    assert (np.asarray(got["hit"])[:nv, :h] == exp["hit"]).all(), (what, "hit")
    ids = np.asarray(got["read_hap"])
    assert ids.shape == exp["read_hap"].shape and (ids == exp["read_hap"]).all(), (what, "read_hap", np.flatnonzero(ids != exp["read_hap"])[:8].tolist())
    if got.get("cooc") is not None:
        assert (np.asarray(got["cooc"])[:nv, :nv] == exp["cooc"]).all(), (what, "cooc")


def ran(what, lib, j, exp, n_cand, form, n_reads, n_groups=None):
    """What the library says of the run: the pipeline, its key words, the positions, the overflow bits, the ids' width (and, where
    asked, the groups its table took)."""
    vp, h = exp["summary"]["n_positions"], exp["summary"]["n_haplotypes"]
    f, m = phase_form(lib, j), ctx_meta(lib, j)
    assert f["form"] == form, (what, f, m)
    assert f["blocks"] == pe.grid_blocks(n_reads) and f["inline"] == (f["blocks"] <= pe.INLINE_IDS_MAX_BLOCKS and form != pe.FORM_MULTI), (what, f)
    ovf = (OVF_CANDIDATES if n_cand > pe.CAND_CAP else 0) | (OVF_HAPLOTYPES if n_cand > pe.MAX_HAPLOTYPES else 0)
    assert (m["vp"], m["vp_true"], m["overflow"]) == (vp, vp, ovf), (what, m)
    if vp:
        # Every run here ends in a launch whose key words are the words its positions need: the plan kernel's (stage API, re-runs)
        # or, planned from the call masks on a fresh context, the one word of the one-word launch for up to 10 positions.
        assert m["kwords"] == pe.key_words(vp), (what, m)
        assert m["id_bits"] == pe.id_bits(h, vp), (what, m, h)
    if n_groups is not None:
        assert m["n_occupied"] == n_groups, (what, m, n_groups)
    return f, m


def check_capacity(what, rc, got, exp, c, table, n_cols):
    """More candidates than the selector ranks: the documented status.  Which candidate is not ranked follows the order of an
    atomic, so at most one of the statement's haplotypes may be missing; everything returned must be right for what was ranked:
    the positions, the damaged reads and their marginals, haplotypes that are groups of the statement in the documented order,
    every read's id against its own pattern, hit against the returned patterns, the balance of the reads."""
    assert rc == c.capacity, (what, rc)
    s, e = got["summary"], exp["summary"]
    for k in ("damaged_reads", "marginal_gap", "marginal_heteroduplex", "marginal_partial", "n_positions", "n_haplotypes"):
        assert s[k] == e[k], (what, k)
    assert (got["pos_cols"] == exp["pos_cols"]).all()
    mine = [(int(n), tuple(p)) for n, p in zip(got["hap_count"], got["hap_pattern"].tolist())]
    theirs = [(int(n), tuple(p)) for n, p in zip(exp["hap_count"], exp["hap_pattern"].tolist())]
    assert mine == sorted(mine, key=lambda x: (-x[0], x[1])) and len(set(mine)) == len(mine)
    assert len(set(mine) & set(theirs)) >= len(theirs) - 1, what
    ids, pats, h = got["read_hap"], exp["patterns"], len(mine)
    clean = pats[:, 0] >= 0
    assert ((ids == pe.HAP_DAMAGED) == ~clean).all()
    named = ids < h
    assert (named <= clean).all() and (ids[clean & ~named] == pe.HAP_INSUFFICIENT).all()
    assert (pats[named] == got["hap_pattern"][ids[named]]).all(), what                    # every read of a haplotype carries its pattern ...
    assert (np.bincount(ids[named], minlength=h) == got["hap_count"]).all(), what         # ... and every read that carries it has the id
    for n, p in mine:
        assert n == int((pats == np.array(p)).all(axis=1).sum())
    assert s["reported_reads"] == int(got["hap_count"].sum()) and s["insufficient_reads"] == int(clean.sum()) - s["reported_reads"], (what, s)
    inside = table["col"].astype(np.int64) + 2 < n_cols
    for v, r in enumerate(table):
        p = np.flatnonzero(exp["pos_cols"] == r["col"])
        want = got["hap_pattern"][:, p[0]] == r["codon"] if len(p) and inside[v] else np.zeros(h, bool)
        assert (got["hit"][v] == want).all(), (what, "hit", v)
    hit = got["hit"].astype(np.int64)
    assert (got["cooc"] == (hit * got["hap_count"].astype(np.int64)) @ hit.T).all(), (what, "cooc")


def upload(j, rows):
    n = rows.shape[0]
    if rows.shape[1] > 4096:
        j.upload_columns(msa.pack_columns(rows), n)     # a wide window goes up as packed columns
    else:
        j.upload_rows(rows)
    j.sync()


def stage(lib, c, exp):
    rows, table = c.build()
    j = capi.Juliet(0)
    upload(j, rows)
    j.phase_async(table, min_reads=c.min_reads)
    rc, got = fetch(j, len(table))
    what = c.name + " stage"
    if c.capacity is not None:
        check_capacity(what, rc, got, exp, c, table, rows.shape[1])
    else:
        assert rc == 0, (what, rc)
        same(what, got, exp, len(table))
    # (a block that fills its LDS table: every distinct pattern is one group of the global table, spilled or not)
    ran(what, lib, j, exp, exp["n_candidates"], pe.form_of_run(exp["summary"]["n_positions"], len(table), exp["n_candidates"]), rows.shape[0],
        len(exp["group_counts"]) if "distinct0" in c.want else None)
    # once more on the same context (the tables a run empties behind itself, the form it has taken)
    if c.capacity is None:
        j.phase_async(table, min_reads=c.min_reads)
        rc, got = fetch(j, len(table))
        assert rc == 0
        same(what + " #2", got, exp, len(table))
    j.close()


def table_is(what, variants, table):
    assert [(int(r["col"]), int(r["codon"])) for r in variants] == [(int(r["col"]), int(r["codon"])) for r in table], what


def whole_path(lib, c, table, exp):
    """jl.run on a fresh context: the called table is the case's, phasing equals the statement on it."""
    rows = c.build()[0]
    j = capi.Juliet(0)
    upload(j, rows)
    what = c.name + " run"
    form = pe.form_of_run(exp["summary"]["n_positions"], len(table), exp["n_candidates"])
    if c.capacity is not None:
        try:
            j.run(c.genes(), c.refseq(), LOOSE, None, True, c.min_reads)
            raise AssertionError(what + ": no overflow status")
        except capi.JulietError as e:
            assert e.status == c.capacity, (what, e.status)
    else:
        out = j.run(c.genes(), c.refseq(), LOOSE, None, True, c.min_reads)
        table_is(what, out["variants"], table)
        same(what, out["phase"], exp, len(table))
    f, _ = ran(what, lib, j, exp, exp["n_candidates"], form, rows.shape[0])
    if exp["summary"]["n_positions"] > 4 * pe.POS_PER_WORD:
        assert f["keys_words"] >= pe.key_words(exp["summary"]["n_positions"]) > 4, (what, f)   # the key buffer grew in the re-run
    j.close()


_beside = {}


def beside(l, deep, min_reads):
    """The resident windows that share a case's group runs: (context, table, expected phasing, reads) of the window without
    variants and of the different window.  Kept while the width stays the same."""
    for key in [k for k in _beside if k[0] != l]:
        for j in _beside.pop(key)["ctx"]:
            j.close()
    b = _beside.get((l, deep))
    if b is None:
        b = _beside[(l, deep)] = dict(ctx=[], rows=[], table=[], exp={})
        for rows, table in ((pe.plain(l), pe.table_of([])), pe.companion(l, pe.COMPANION_DEEP if deep else pe.COMPANION_READS)):
            j = capi.Juliet(0)
            upload(j, rows)
            b["ctx"].append(j), b["rows"].append(rows), b["table"].append(table)
    if min_reads not in b["exp"]:
        b["exp"][min_reads] = [pe.phase(r, t, min_reads) for r, t in zip(b["rows"], b["table"])]
    return [(j, t, e, len(r)) for j, t, e, r in zip(b["ctx"], b["table"], b["exp"][min_reads], b["rows"])]


def group_ids_inline(lib, grp):
    out = (C.c_uint32 * 8)()
    assert lib.jl_tuning_group_ids_inline(grp.h, out, 8) == 1      # three windows: one chunk
    return bool(out[0])


def group_runs(lib, c, table, exp, seen):
    """The case as the middle window of group runs of three windows, between a window without variants and a different one:
    beside a shallow one (the phasing launch writes the ids) and beside a deep one (the separate launch does).  seen: (ids inline
    as the library says, id width of the case) of every one-word case."""
    rows = c.build()[0]
    n, l = rows.shape
    vp = exp["summary"]["n_positions"]
    for deep in (False, True):
        (jp, tp, exp_plain, n_plain), (jo, to, exp_other, n_other) = beside(l, deep, c.min_reads)
        j = capi.Juliet(0)
        upload(j, rows)
        grp = capi.Group([jp, j, jo])
        blocks = sum(pe.grid_blocks(k) for k in (n_plain, n, n_other))
        for rep in range(2):                   # (the second launch replays the captured graph)
            grp.run_async(c.genes(), c.refseq(), LOOSE, True, c.min_reads, True)
            inline = group_ids_inline(lib, grp)
            assert inline == (blocks <= pe.INLINE_IDS_MAX_BLOCKS), (c.name, deep, blocks, inline)
            for ctx, t, e, who in ((jp, tp, exp_plain, "plain"), (j, table, exp, "case"), (jo, to, exp_other, "other")):
                what = "%s group deep=%d #%d %s" % (c.name, deep, rep, who)
                ctx.run_wait()
                v = ctx.run_view()
                over = e["summary"]["n_positions"] > pe.FORM_ONE_WORD_MAX      # more positions than the group launch covers: no view
                assert v is None or not over, what
                if v is not None:
                    table_is(what + " view", v["variants"], t)
                    same(what + " view", dict(v["phase"], cooc=None), e, len(t))
                f = ctx.run_fetch(True, True, cap_var=max(128, len(t)))
                table_is(what, f["variants"], t)
                same(what, f["phase"], e, len(t))
            if vp > pe.FORM_ONE_WORD_MAX:
                break                          # that context has left the one-word form: group runs refuse it from now on
        if 0 < vp <= pe.FORM_ONE_WORD_MAX:
            seen.add((inline, pe.id_bits(exp["summary"]["n_haplotypes"], vp)))
        ran(c.name + " group", lib, j, exp, exp["n_candidates"], pe.form_of_run(vp, len(table), exp["n_candidates"]), n)
        grp.close()
        j.close()


# what the group runs of a part must have met: ids written by the phasing launch and by the separate launch, at these widths
GROUP_MUST_SEE = {"positions": {(True, 4), (False, 4)}, "reads": {(True, 4), (False, 4)},
                  "selection": {(m, b) for m in (True, False) for b in (4, 8, 16)}, "table": {(True, 16), (False, 16)}}


def run_part(lib, part):
    seen = set()
    for name in pe.PARTS[part]:
        c = pe.CASES[name]
        t0 = time.time()
        exp = c.expected()
        entries = ["stage"]
        stage(lib, c, exp)
        if c.whole_path:
            table = c.called()
            exp_run = c.expected_run()
            whole_path(lib, c, table, exp_run)
            entries.append("run")
            if name not in pe.NO_GROUP:
                group_runs(lib, c, table, exp_run, seen)
                entries.append("group")
        c.drop()
        print("COMPARED %s %s  (%.2f s)" % (name, "+".join(entries), time.time() - t0), flush=True)
    assert GROUP_MUST_SEE.get(part, set()) <= seen, (part, sorted(seen))
    for b in _beside.values():
        for j in b["ctx"]:
            j.close()


def run_growth(lib):
    """One context asked for 10, 11, 21, then 10 positions again: the form only grows, the key buffer grows with it, every result
    is exact.  A fresh context asked for 21 positions first.  (With a host table the key buffer is sized from the table before the
    launch, so this sequence meets JL_PHASE_OVF_FORM only; JL_PHASE_OVF_KEY_WORDS needs a run that cannot know its positions
    beforehand and finds more than 40: the whole-path run of the case vp41.)"""
    def ask(j, name, form):
        c = pe.CASES[name]
        rows, table = c.build()
        exp = c.expected()
        upload(j, rows)
        j.phase_async(table, min_reads=c.min_reads)
        rc, got = fetch(j, len(table))
        assert rc == 0
        same("growth " + name, got, exp, len(table))
        f, m = ran("growth " + name, lib, j, exp, exp["n_candidates"], form, rows.shape[0])
        assert f["keys_words"] >= pe.key_words(exp["summary"]["n_positions"])
        print("COMPARED %s stage form %d kwords %d" % (name, f["form"], m["kwords"]), flush=True)
        return f
    j = capi.Juliet(0)
    words = [ask(j, name, form)["keys_words"] for name, form in zip(pe.GROWTH, pe.GROWTH_FORMS)]
    assert words == sorted(words) and words[2] >= 3, words
    j.close()
    j = capi.Juliet(0)
    ask(j, pe.GROWTH_FRESH, pe.FORM_MULTI)
    ask(j, pe.GROWTH[0], pe.FORM_MULTI)
    j.close()


def main():
    lib = capi.load_library(os.environ["JL_LIB"])
    lib.jl_tuning_ctx_meta.restype = C.c_int
    lib.jl_tuning_ctx_meta.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    lib.jl_tuning_phase_form.restype = C.c_int
    lib.jl_tuning_phase_form.argtypes = [C.c_void_p, C.c_void_p]
    lib.jl_tuning_group_ids_inline.restype = C.c_int
    lib.jl_tuning_group_ids_inline.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    part = sys.argv[1]
    t0 = time.time()
    run_growth(lib) if part == "growth" else run_part(lib, part)
    print("part %s %.2f s" % (part, time.time() - t0))
    print("PHASE-EDGES-OK", part)


if __name__ == "__main__":
    main()
