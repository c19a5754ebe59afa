"""The designed phasing windows of tests/phase_edges.py, without a GPU: every case sits on the edge it is named for (computed from
its matrix), the plain numpy statement of SPEC §8 equals the oracle on every case, the mirrored constants are the library's, and
the cases tell five wrong kernels from the right one.  tests/test_gpu_phase_edges.py sends the same cases through the kernels."""
import os
import re

import numpy as np
import pytest

import phase_edges as pe
from minorseq_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minorseq_amd", "csrc")
SMALL = [n for n in pe.CASES if n not in pe.WIDE]


def source(name):
    with open(os.path.join(CSRC, name) if not name.startswith("include") else os.path.join(ROOT, name)) as f:
        return f.read()


def define(text, name):
    m = re.search(r"^\s*#\s*define\s+%s\s+(\d+)u?\b" % name, text, re.M)
    assert m, name
    return int(m.group(1))


def test_mirrored_constants_are_the_librarys():
    internal, phase, plan, api, host = (source(f) for f in ("jl_internal.h", "kernels_phase.hip", "phase_plan.h", "include/juliet_hip.h", "capi.hip"))
    assert pe.POS_PER_WORD == define(internal, "JL_POS_PER_WORD")
    assert pe.CAND_CAP == define(internal, "JL_CAND_CAP")
    assert pe.PACK_MAX_HAP == define(internal, "JL_PACK_MAX_HAP")
    assert pe.PACK_MAX_VAR == define(internal, "JL_PACK_MAX_VAR") and pe.SEL_HIT_BYTES == define(internal, "JL_SEL_HIT_BYTES")
    assert "if (T.bail || nv * H > JL_SEL_HIT_BYTES) return false;" in phase and "nv > JL_PACK_MAX_VAR || n_rows > JL_PACK_MAX_VAR" in phase
    assert pe.ID4_MAX_H == define(internal, "JL_ID4_MAX_H") and pe.ID8_MAX_H == define(internal, "JL_ID8_MAX_H")
    assert pe.INLINE_IDS_MAX_BLOCKS == define(internal, "JL_INLINE_IDS_MAX_BLOCKS")
    assert pe.PLAN_LDS_COLS == define(plan, "JL_PLAN_LDS_WORDS") * 32 and "n_cols <= JL_PLAN_LDS_WORDS * 32u" in plan
    assert pe.LDS_SLOTS == int(re.search(r"constexpr uint32_t kLdsSlots = (\d+);", phase).group(1))
    assert "constexpr uint32_t kSelCand = JL_PACK_MAX_HAP;" in phase
    assert pe.MAX_HAPLOTYPES == int(re.search(r"JL_MAX_HAPLOTYPES = (\d+)", api).group(1)) == capi.MAX_HAPLOTYPES
    assert (pe.HAP_INSUFFICIENT, pe.HAP_DAMAGED) == (capi.HAP_INSUFFICIENT, capi.HAP_DAMAGED)
    assert pe.ERR_OVERFLOW == int(re.search(r"JL_ERR_OVERFLOW = (-\d+)", api).group(1))
    assert pe.SUMMARY_FIELDS == tuple(capi.SUMMARY_FIELDS)
    # a workgroup of the fused launch: 256 lanes, a lane the dword of eight codes that one byte of each plane gives
    assert re.search(r"jl_phase_grid_blocks\(const jl_ctx \*ctx\) \{ return \(uint32_t\)\(\(ctx->col_stride / 4u \+ 255u\) / 256u\) \+ 1u; \}", phase)
    assert "const uint64_t t = (uint64_t)blockIdx.x * 256u + tid;" in phase and "if (t * 8u + r < n_reads)" in phase
    assert pe.BLOCK_READS == 256 * 8
    assert "return total_blocks <= JL_INLINE_IDS_MAX_BLOCKS" in phase
    lib = capi.load_library()
    for n in pe.READ_COUNTS:
        assert lib.jl_plane_stride(n) * 8 == -(-n // pe.LINE_READS) * pe.LINE_READS
    # the forms: the limits of phase_form_for and the enum's values
    assert "if (vp <= JL_POS_PER_WORD) return from;" in host
    assert "if (vp <= 2u * JL_POS_PER_WORD && from == jl_phase_form::one_word && two_word_ok) return jl_phase_form::two_word;" in host
    assert (pe.FORM_ONE_WORD_MAX, pe.FORM_TWO_WORD_MAX) == (pe.POS_PER_WORD, 2 * pe.POS_PER_WORD)
    for name, v in (("multi_word", pe.FORM_MULTI), ("one_word", pe.FORM_ONE), ("two_word", pe.FORM_TWO)):
        assert re.search(r"^\s*%s = %d," % (name, v), internal, re.M)
    assert [pe.form_for(vp) for vp in (0, 10, 11, 20, 21)] == [1, 1, 2, 2, 0] and pe.form_for(10, pe.FORM_TWO) == 2 and pe.form_for(11, pe.FORM_TWO) == 0
    assert [pe.id_bits(h, 2) for h in (0, 14, 15, 254, 255, 702)] == [4, 4, 8, 8, 16, 16]
    assert pe.READ_COUNTS == (1, 63, 64, 65, 2047, 2048, 2049, 4097, 260096, 260097)
    assert [pe.grid_blocks(n) for n in (1, 2048, 2049, 4097, 260096, 260097)] == [2, 2, 3, 4, 128, 129]


@pytest.fixture(scope="module")
def expected():
    """The numpy statement of every small case, computed once."""
    return {n: pe.CASES[n].expected() for n in SMALL}


def test_cases_sit_on_the_edges_their_names_say(expected):
    assert len(pe.CASES) == 46
    seen_vp = set()
    for name in SMALL:
        c, e = pe.CASES[name], expected[name]
        rows, table = c.build()
        w, s = c.want, e["summary"]
        n, l = rows.shape
        assert w, name
        if "vp" in w:
            assert s["n_positions"] == w["vp"], name
            seen_vp.add(w["vp"])
        if "ignored_rows" in w:
            assert int((table["col"].astype(np.int64) + 2 >= l).sum()) == w["ignored_rows"] and (l - 2) in table["col"] and (l - 3) in table["col"], name
        if "blocks" in w:
            assert pe.grid_blocks(n) == w["blocks"] and (w["blocks"] <= pe.INLINE_IDS_MAX_BLOCKS) == (n <= pe.INLINE_MAX_READS), name
        if "distinct0" in w:
            per_block = pe.distinct_patterns_per_block(e["patterns"])
            assert per_block[0] == w["distinct0"] and len(per_block) == 2 and (e["patterns"][:pe.BLOCK_READS] >= 0).all(), name
            # the dominant pattern (the first clean read's) is one of the three large groups: the other distinct0 - 1 go to the table;
            # more than half of the small groups are reported, so a read that went round a full table shows in its id
            assert e["read_hap"][0] < 3 and c.min_reads == 2 and len(e["group_counts"]) == w["distinct0"], name
            # (the two-word launch selects at most 128 candidates itself: there 120 of the small groups are reported)
            lo, hi = (w["distinct0"] // 2, pe.MAX_HAPLOTYPES) if w["vp"] == 2 else (100, pe.PACK_MAX_HAP)
            assert lo < s["n_haplotypes"] <= hi and sorted(e["group_counts"])[-4] == 2, (name, s)
        if "vary" in w:
            differ = np.flatnonzero((e["patterns"][e["patterns"][:, 0] >= 0] != e["patterns"][e["patterns"][:, 0] >= 0][0]).any(axis=0))
            assert set(differ) <= set(w["vary"]) and len(differ) >= 1, (name, differ)
        if "at_threshold" in w:
            m = w["at_threshold"]
            assert c.min_reads == m and m in e["group_counts"] and (m == 1 or m - 1 in e["group_counts"]) and m + 1 in e["group_counts"], name
            assert s["insufficient_reads"] == (m - 1 if m > 1 else 0), name
        if "ties" in w:
            assert e["hap_count"].tolist() == [7, 7, 5, 5, 5, 5, 5, 5], name
        if "haplotypes" in w:
            assert (s["n_haplotypes"], e["n_candidates"]) == (w["haplotypes"], w["candidates"]), name
        assert s["reported_reads"] + s["insufficient_reads"] + s["damaged_reads"] == (n if s["n_positions"] else 0), name
    assert seen_vp >= {0, 1, 10, 11, 20, 21, 30, 31, 41}
    # two variants at one column; overlapping codons; column 0; codons AAA and TTT at the first and last position of a key word
    t10 = pe.CASES["vp10"].build()[1]
    assert len(t10) == 11 and len(np.unique(t10["col"])) == 10
    p = expected["vp11-overlap"]["pos_cols"].tolist()
    assert 24 in p and 25 in p
    for name in ("vp10", "vp20", "vp21", "vp31"):
        e, t = expected[name], pe.CASES[name].build()[1]
        assert e["pos_cols"][0] == 0
        codon_at = {int(np.searchsorted(e["pos_cols"], r["col"])): int(r["codon"]) for r in t if r["codon"] in (0, 63)}
        for word in range(pe.key_words(len(e["pos_cols"]))):
            assert codon_at.get(10 * word) == 0, (name, word)
            if 10 * word + 9 < len(e["pos_cols"]):
                assert codon_at[10 * word + 9] == 63, (name, word)
    # every damage branch, in each codon column, and a third codon that is no variant
    rows, table = pe.CASES["vp20-last"].build()
    e = expected["vp20-last"]
    for p in (0, 9, 10, 19):
        c = int(e["pos_cols"][p])
        for k in range(3):
            assert {4, 5, 6} <= set(rows[:, c + k].tolist()), (p, k)
    s = e["summary"]
    assert s["marginal_gap"] == s["marginal_heteroduplex"] == s["marginal_partial"] == 12 and s["damaged_reads"] == 36
    clean = e["patterns"][e["patterns"][:, 0] >= 0]
    assert 38 in clean[:, 0] and 38 not in table["codon"][table["col"] == 0]
    # the id-width steps and the selection's capacities, on both sides
    assert {pe.CASES[n].want["haplotypes"] for n in pe.CASES if n.startswith("haps-")} == {14, 15, 128, 129, 254, 255, 702}
    assert [(pe.CASES[n].want["candidates"], pe.CASES[n].want["form"]) for n in ("haps2w-128", "haps2w-129")] == [(128, pe.FORM_TWO), (129, pe.FORM_MULTI)]
    for n in ("haps2w-128", "haps2w-129", "lds-1026-w0", "lds-1026-w1", "w1-last", "ties", "vp11", "vp20"):      # through the stage API: the host table
        e, t = expected[n], pe.CASES[n].build()[1]
        assert pe.form_of_run(e["summary"]["n_positions"], len(t), e["n_candidates"]) == pe.CASES[n].want.get("form", pe.FORM_TWO), n
    assert [pe.CASES[n].want["candidates"] for n in ("haps-703", "cand-4096", "cand-4097")] == [703, 4096, 4097]
    assert [n for n in pe.CASES if pe.CASES[n].capacity is not None] == ["cand-4097"]


def test_wide_cases_sit_on_the_plans_two_paths():
    for name, vp in zip(pe.WIDE, (3, 4)):
        c = pe.CASES[name]
        rows, table = c.build()
        e = c.expected()
        n, l = rows.shape
        assert (n, l) == (64, c.want["cols"]) and (l <= pe.PLAN_LDS_COLS) == (name == pe.WIDE[0])
        p = e["pos_cols"].tolist()
        assert len(p) == vp == c.want["vp"] and p[0] == 0 and p[-1] == l - 3 and 131069 in p and (l - 2) in table["col"]
        s = e["summary"]
        assert (s["marginal_gap"], s["marginal_heteroduplex"], s["marginal_partial"]) == (1, 1, 1) and s["n_haplotypes"] >= 3
        c.drop()


def oracle_fields_equal(got, exp, n_var):
    """The fields assert_phase_equal of tests/test_gpu_parity.py compares."""
    return (got["summary"] == exp["summary"] and got["pos_cols"].shape == exp["pos_cols"].shape and (got["pos_cols"] == exp["pos_cols"]).all()
            and got["hap_count"].shape == exp["hap_count"].shape and (got["hap_count"] == exp["hap_count"]).all()
            and got["hap_pattern"].shape == exp["hap_pattern"].shape and (got["hap_pattern"] == exp["hap_pattern"]).all()
            and (got["hit"] == exp["hit"]).all() and (got["read_hap"] == exp["read_hap"]).all() and (got["cooc"][:n_var, :n_var] == exp["cooc"]).all())


def oracle_phase(oracle, c):
    """The oracle knows no row outside the window (it would read the codon beyond the last column as not covered): it is given
    the rows inside, and the rows outside are those the statement gives no hit at all."""
    rows, table = c.build()
    inside = table["col"].astype(np.int64) + 2 < rows.shape[1]
    return oracle.phase(rows, table[inside], min_reads=c.min_reads), inside


@pytest.mark.parametrize("part", sorted(pe.PARTS))
def test_numpy_statement_equals_oracle(oracle, part):
    for name in pe.PARTS[part]:
        c = pe.CASES[name]
        rows, table = c.build()
        e = c.expected()
        exp, inside = oracle_phase(oracle, c)
        assert not e["hit"][~inside].any() and not e["cooc"][~inside].any() and not e["cooc"][:, ~inside].any(), name
        got = dict(e, hit=e["hit"][inside], cooc=e["cooc"][np.ix_(inside, inside)])
        for k in ("summary", "pos_cols", "hap_count", "hap_pattern", "hit", "read_hap", "cooc"):
            same = got[k] == exp[k] if k == "summary" else (got[k].shape == exp[k].shape and (got[k] == exp[k]).all())
            assert same, (name, k)
        assert oracle_fields_equal(got, exp, int(inside.sum())), name
        c.drop() if name in pe.WIDE else None


def test_whole_path_cases_have_the_table_the_call_stage_gives(oracle):
    """called() of every case that goes through the whole path is what the call stage makes of its matrix (one gene in frame, the
    background as reference, alpha 0.9, n_tests 1): same rows in the same order, by column and codon — and it gives the positions
    the case is named for.  The statement on that table equals the oracle too.  Only the cases named in NO_WHOLE_PATH stay out."""
    import oracle_lib
    loose = oracle_lib.default_params(alpha=0.9, n_tests=1.0)
    assert sorted(pe.NO_WHOLE_PATH) == ["reads-1", "vp11-overlap"] + pe.WIDE and set(pe.NO_GROUP) <= set(pe.CASES)
    for name, c in pe.CASES.items():
        rows, table = c.build()
        if name in pe.WIDE:
            continue
        if not c.whole_path:
            called = oracle.call(rows, c.genes(), refseq=c.refseq(), params=loose)
            assert [(int(r["col"]), int(r["codon"])) for r in called] != [(int(r["col"]), int(r["codon"])) for r in table], name
            continue
        mine = c.called()
        called = oracle.call(rows, c.genes(), refseq=c.refseq(), params=loose)
        assert [(int(r["col"]), int(r["codon"])) for r in called] == [(int(r["col"]), int(r["codon"])) for r in mine], name
        assert (called["codon_pos"] == mine["codon_pos"]).all() and (called["ref_codon"] == mine["ref_codon"]).all(), name
        e = c.expected_run()
        assert e["summary"]["n_positions"] == c.want.get("vp", e["summary"]["n_positions"]), name
        assert e["summary"]["n_haplotypes"] == c.want.get("haplotypes", e["summary"]["n_haplotypes"]), name
        assert oracle_fields_equal(e, oracle.phase(rows, mine, min_reads=c.min_reads), len(mine)), name
    # the windows that share a case's group runs: one without variants, one with a table of its own
    for l, n in ((8, pe.COMPANION_READS), (190, pe.COMPANION_READS), (16, pe.COMPANION_DEEP)):
        genes = np.array([(1, l + 1)], dtype=pe.GENE)
        assert len(oracle.call(pe.plain(l), genes, refseq=pe.background(l), params=loose)) == 0
        rows, table = pe.companion(l, n)
        called = oracle.call(rows, genes, refseq=pe.background(l), params=loose)
        assert [(int(r["col"]), int(r["codon"])) for r in called] == [(int(r["col"]), int(r["codon"])) for r in table] and len(table) == 3
        e = pe.phase(rows, table, 2)
        exp = oracle.phase(rows, table, min_reads=2)
        assert oracle_fields_equal(e, exp, 3) and e["summary"]["n_haplotypes"] >= 4 and e["summary"]["damaged_reads"] > 0
    assert pe.grid_blocks(pe.COMPANION_DEEP) > pe.INLINE_IDS_MAX_BLOCKS and 3 * pe.grid_blocks(pe.COMPANION_READS) <= pe.INLINE_IDS_MAX_BLOCKS


WRONG = ("gt", "last_col", "drop10th", "no_word1", "ties_reversed")
# which cases tell each wrong kernel from the right one (at least these; the test prints the whole table)
CATCHES = {
    "gt": ("minreads-1", "minreads-2", "minreads-10"),
    "last_col": ("vp20-last", "vp21-last"),
    "drop10th": ("vp10", "vp20", "w1-last", "lds-1026-w1", "lds-1026-w0", "ties"),
    "no_word1": ("vp11", "vp20", "w1-last", "lds-1026-w1", "ties"),
    "ties_reversed": ("ties", "vp10", "vp31"),
}


def test_cases_tell_wrong_kernels_from_the_right_one(oracle):
    caught = {w: [] for w in WRONG}
    for name in SMALL:
        c = pe.CASES[name]
        rows, table = c.build()
        exp, inside = oracle_phase(oracle, c)
        for w in WRONG:
            e = pe.phase(rows, table, c.min_reads, wrong=w)
            if w == "last_col":       # this wrong kernel takes more rows for inside the window: compare what the oracle has
                ok = e["hit"].shape[1] == exp["hit"].shape[1] and oracle_fields_equal(dict(e, hit=e["hit"][inside], cooc=e["cooc"][np.ix_(inside, inside)]),
                                                                                      exp, int(inside.sum()))
            else:
                ok = oracle_fields_equal(dict(e, hit=e["hit"][inside], cooc=e["cooc"][np.ix_(inside, inside)]), exp, int(inside.sum()))
            if not ok:
                caught[w].append(name)
    for w in WRONG:
        print("%-14s caught by %d cases: %s" % (w, len(caught[w]), " ".join(caught[w])))
        assert set(CATCHES[w]) <= set(caught[w]), (w, caught[w])
