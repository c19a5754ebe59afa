"""The eight stage calls of a context — class_pileup, class_codons, phase_rescue, phase_nearest, phase_recombinants,
variant_linkage, codon_deletions, read_stats — and the run, in sequences (docs/SPEC.md §13 – §24: a stage "changes nothing else of
the context ... and the other way round"): several stages enqueued on one context with no wait in between and fetched in another
order, every stage in front of every other, results fetched after the matrix they were computed from was replaced by each producer,
stages in front of and behind a run and its captured graph, a refused call between the enqueues and the fetches, and one context
taken through matrices that grow and shrink.  Matrices, parameters and expected values are tests/stage_sequences.py's: every
expected value is a mirror (or the oracle, for the run) applied to the rows that were uploaded, never another device result —
except where the claim is "identical to the same run alone".  Runs only on a real MI355X: `pytest -m gpu`."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import stage_sequences as ss
from minorseq_amd import capi, msa, synth
from stage_sequences import LARGE, SMALL, STAGES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def built():
    """The library normally travels with the tree; build it only if it is missing (never under a loaded .so)."""
    if not os.path.exists(os.path.join(ROOT, "minorseq_amd", "libjuliet_hip.so")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "csrc")])


@pytest.fixture(scope="module")
def cases(built):
    return ss.check_not_vacuous()


@pytest.fixture
def ctx():
    j = capi.Juliet(0)
    yield j
    j.close()


@pytest.fixture
def second():
    j = capi.Juliet(0)
    yield j
    j.close()


# ------------------------------------------------------------------------------------------------ enqueue, fetch, compare
def enqueue(j, stage, prm):
    """The stage on the context's stream, nothing waited for."""
    if stage == "class_pileup":
        r = j.class_pileup(prm["label"], prm["n_classes"], wait=False)
    elif stage == "class_codons":
        r = j.class_codons(prm["label"], prm["n_classes"], prm["pos_cols"], wait=False)
    elif stage == "phase_rescue":
        r = j.phase_rescue(prm["pos_cols"], prm["pattern"], prm["min_positions"], wait=False)
    elif stage == "phase_nearest":
        r = j.phase_nearest(prm["pos_cols"], prm["pattern"], prm["min_positions"], prm["max_distance"], wait=False)
    elif stage == "phase_recombinants":
        r = j.phase_recombinants(prm["pos_cols"], prm["pattern"], prm["min_positions"], wait=False)
    elif stage == "variant_linkage":
        r = j.variant_linkage(prm["link_pos"], prm["var_pos"], prm["var_codon"], wait=False)
    elif stage == "codon_deletions":
        r = j.codon_deletions(wait=False)
    elif stage == "read_stats":
        r = j.read_stats(prm["compare"], wait=False)
    else:
        raise ValueError(stage)
    assert r is None


def fetch(j, stage):
    """{array name: array} of the stage's last enqueue, named as stage_sequences.expected names them."""
    r = getattr(j, stage + "_fetch")()
    if stage == "class_pileup":
        return dict(counts=r[0], class_reads=r[1])
    if stage == "class_codons":
        return dict(hist=r[0], class_reads=r[1])
    if stage == "codon_deletions":
        return dict(cnt=r)
    if stage == "read_stats":
        return dict(stats=r)
    return r


SENTINEL = 0xA5


def raw_fetch(j, stage, exp):
    """The same through the raw entry point, into arrays of the shapes of `exp` with a guard band behind each: room for what a
    fetch sized by any other matrix of this module would write, filled with a sentinel that must come back untouched — so a fetch
    of the wrong size is a failed assertion, never a host overrun."""
    bufs = {}
    for key, want in exp.items():
        buf = np.empty(want.size + max(4096, 2 * want.size), dtype=want.dtype)
        buf.view(np.uint8)[:] = SENTINEL
        bufs[key] = buf
    fn = getattr(j.lib, {"class_pileup": "jl_class_pileup_fetch", "class_codons": "jl_class_codons_fetch", "phase_rescue": "jl_phase_rescue_fetch",
                         "phase_nearest": "jl_phase_nearest_fetch", "phase_recombinants": "jl_phase_recombinants_fetch",
                         "variant_linkage": "jl_variant_linkage_fetch", "codon_deletions": "jl_codon_deletions_fetch",
                         "read_stats": "jl_read_stats_fetch"}[stage])
    rc = fn(j.h, *(bufs[key].ctypes.data_as(C.c_void_p) for key in exp))      # (the dict's order is the entry point's)
    assert rc == 0, (stage, j.lib.jl_last_error(j.h).decode())
    out = {}
    for key, want in exp.items():
        guard = bufs[key][want.size:].view(np.uint8)
        assert (guard == SENTINEL).all(), (stage, key, "the fetch wrote %d bytes past the recorded shape" % (int(np.flatnonzero(guard != SENTINEL)[-1]) + 1))
        out[key] = bufs[key][:want.size].reshape(want.shape)
    return out


def assert_stage(got, exp, where):
    assert list(got) == list(exp), where
    for key, want in exp.items():
        assert got[key].shape == want.shape and got[key].dtype == want.dtype, (where, key, got[key].shape, want.shape)
        bad = np.argwhere(got[key] != want)
        assert len(bad) == 0, (where, key, "%d cells differ, the first at %s: %s for %s" % (len(bad), tuple(bad[0]), got[key][tuple(bad[0])], want[tuple(bad[0])]))


def matrix_is(j, rows):
    assert (msa.unpack_columns(j.download_columns(), len(rows)) == rows).all()


def enqueue_all(j, case, setting_of, order=STAGES):
    for stage in order:
        enqueue(j, stage, case.prm[setting_of(stage)])


def fetch_all(j, case, setting_of, order=STAGES, raw=False, where=()):
    for stage in order:
        exp = case.exp[setting_of(stage)][stage]
        got = raw_fetch(j, stage, exp) if raw else fetch(j, stage)
        assert_stage(got, exp, (*where, case.name, stage, setting_of(stage)))


def every(setting):
    return lambda stage: setting


# ------------------------------------------------------------------------------------------------ 1. interleaved enqueue, permuted fetch
FORWARD = STAGES
REVERSE = STAGES[::-1]
# two pairs of fixed permutations (numpy.random.default_rng(1).permutation(8) four times over, written out)
PERM_A = tuple(STAGES[k] for k in (6, 5, 0, 3, 7, 2, 4, 1))
PERM_B = tuple(STAGES[k] for k in (2, 7, 4, 1, 6, 0, 5, 3))
PERM_C = tuple(STAGES[k] for k in (3, 0, 6, 4, 1, 7, 5, 2))
PERM_D = tuple(STAGES[k] for k in (7, 1, 5, 2, 0, 4, 3, 6))
ORDER_PAIRS = {"forward-forward": (FORWARD, FORWARD), "forward-reverse": (FORWARD, REVERSE), "perm-a-b": (PERM_A, PERM_B), "perm-c-d": (PERM_C, PERM_D)}


@pytest.mark.parametrize("name", list(ORDER_PAIRS))
def test_interleaved_enqueue_permuted_fetch(ctx, cases, name):
    """All eight enqueued on A with no fetch in between, all eight fetched in another order; in the permuted cases the stages take
    the large and the small setting by turns."""
    first, then = ORDER_PAIRS[name]
    assert sorted(first) == sorted(then) == sorted(STAGES)
    a = cases["A"]
    mixed = name.startswith("perm")
    setting_of = (lambda stage: (LARGE, SMALL)[(STAGES.index(stage) + (name == "perm-c-d")) % 2]) if mixed else every(LARGE)
    ctx.upload_rows(a.rows, win_begin=3)
    enqueue_all(ctx, a, setting_of, first)
    fetch_all(ctx, a, setting_of, then, where=(name,))
    matrix_is(ctx, a.rows)
    fetch_all(ctx, a, setting_of, first, raw=True, where=(name, "again"))        # ... and a second fetch is the first


# ------------------------------------------------------------------------------------------------ 2. each stage in front of each other
PAIRS = [(x, y) for x in STAGES for y in STAGES if x != y]
PAIR_SETTING = {pair: (LARGE, SMALL)[k % 2] for k, pair in enumerate(PAIRS)}


def test_pair_settings_alternate():
    """Over the 56 pairs in their order every stage is called large after small and small after large on the shared context."""
    assert len(PAIRS) == 56
    for stage in STAGES:
        calls = [PAIR_SETTING[pair] for pair in PAIRS if stage in pair]
        steps = set(zip(calls, calls[1:]))
        assert (LARGE, SMALL) in steps and (SMALL, LARGE) in steps, (stage, steps)


@pytest.fixture(scope="module")
def pair_ctx(cases):
    j = capi.Juliet(0)
    j.upload_rows(cases["A"].rows)
    yield j
    matrix_is(j, cases["A"].rows)              # after all the pairs the matrix is what was uploaded once
    j.close()


@pytest.mark.parametrize("x,y", PAIRS, ids=["%s-then-%s" % pair for pair in PAIRS])
def test_stage_in_front_of_stage(pair_ctx, cases, x, y):
    a, setting = cases["A"], PAIR_SETTING[x, y]
    enqueue(pair_ctx, x, a.prm[setting])
    enqueue(pair_ctx, y, a.prm[setting])
    assert_stage(fetch(pair_ctx, y), a.exp[setting][y], (x, y, setting, "the second"))
    assert_stage(fetch(pair_ctx, x), a.exp[setting][x], (x, y, setting, "the first"))


# ------------------------------------------------------------------------------------------------ 3. results outlive their matrix
def records_1025():
    """1025 aligned records over about 40 columns (test_gpu_planes.records) and their rows in a 66-column window."""
    import records_expand
    from test_gpu_planes import records
    rec = records(1025)
    return rec, records_expand.expand(rec, 66, 0, 0)


def replace(j, how, cases, other):
    """The resident matrix of `j` replaced by producer `how`; `other` is a second context where the producer reads one.  Returns the
    Case of the new matrix (rows as numpy says the producer makes them) and what must stay alive."""
    if how in ("upload_B", "upload_C", "upload_A2", "upload_A"):
        new = cases[how.split("_")[1]]
        j.upload_rows(new.rows, win_begin=5)
        return new, None
    b = cases["B"]
    if how == "take":
        other.upload_rows(b.rows)
        idx = np.random.default_rng(11).integers(0, len(b.rows), size=700).astype(np.uint32)       # any order, repeats
        j.take([(other, idx)])
        return ss.Case(how, b.rows[idx], 12, b.haps), None
    if how == "alloc_synth_fill":
        n, l = 1500, 70
        sp = synth.SynthParams(seed=7, minor_permille=(150, 120, 100, 80))
        ref = synth.reference(sp.seed, l)
        j.alloc(n, l)
        j.synth_fill(sp, ref)
        return ss.Case(how, synth.rows(sp, l, 0, n, ref), 13), None
    if how == "records_window":
        from test_gpu_qmask import five
        rec, rows = records_1025()
        other.records_upload(*five(rec))
        j.records_window(other, 66, 0, 0)
        other.records_drop()
        return ss.Case(how, rows, 14), None
    if how == "adopt":
        # a torch tensor with its own stride (272; the library's is 384), garbage past byte ceil(n / 8) of every plane row
        import torch
        n, l, stride = 2049, 67, 272
        rows = b.rows[:, :l]
        planes = msa.pack_planes(rows, stride)
        planes[:, :, (n + 7) // 8:] = np.random.default_rng(1).integers(0, 256, size=(l, 3, stride - (n + 7) // 8), dtype=np.uint8)
        t = torch.from_numpy(planes).cuda()
        torch.cuda.synchronize()
        j.adopt(t.data_ptr(), n, l, stride, keep_alive=t)
        return ss.Case(how, rows, 15), t
    if how == "sites_assemble":
        other.upload_rows(b.rows)
        cols = [int(c) for c in ss.codon_starts(b.rows.shape[1])]
        j.sites_assemble(other, [(c, capi.SITE_CODON, capi.SITE_NO_FILL) for c in cols])      # plain codon sites: the three columns copied
        return ss.Case(how, np.concatenate([b.rows[:, c:c + 3] for c in cols], axis=1), 16), None
    raise ValueError(how)


def replace_and_check(j, old, old_setting, how, cases, other):
    """All eight pending on `old`; the matrix replaced without a fetch; all eight fetched in the shapes of `old` and equal to its
    mirrors; then all eight on the new matrix, the small setting first (on buffers made for the large one), equal to its mirrors."""
    enqueue_all(j, old, every(old_setting))
    new, keep = replace(j, how, cases, other)
    fetch_all(j, old, every(old_setting), raw=True, where=(how, "after the replacement"))
    matrix_is(j, new.rows)
    for setting in (SMALL, LARGE):
        if setting in new.settings:
            enqueue_all(j, new, every(setting), REVERSE)
            fetch_all(j, new, every(setting), raw=True, where=(how, "on the new matrix"))
    matrix_is(j, new.rows)
    return new, keep


REPLACEMENTS = ("upload_B", "upload_C", "upload_A2", "take", "alloc_synth_fill", "records_window", "adopt", "sites_assemble")


@pytest.mark.parametrize("how", REPLACEMENTS)
def test_results_outlive_their_matrix(ctx, second, cases, how):
    a = cases["A"]
    ctx.upload_rows(a.rows)
    new, keep = replace_and_check(ctx, a, LARGE, how, cases, second)
    assert new.rows.shape != a.rows.shape or how == "upload_A2" or how == "records_window"
    del keep


def test_results_outlive_their_matrix_growing_then_shrinking(ctx, second, cases):
    """A -> B -> C -> A in one context: every buffer grows once, then serves matrices smaller than it."""
    ctx.upload_rows(cases["A"].rows)
    replace_and_check(ctx, cases["A"], LARGE, "upload_B", cases, second)
    replace_and_check(ctx, cases["B"], LARGE, "upload_C", cases, second)
    replace_and_check(ctx, cases["C"], SMALL, "upload_A", cases, second)


# ------------------------------------------------------------------------------------------------ 4. the run and the stages
RUN_KEYS = ("pos_cols", "hap_count", "hap_pattern", "hit", "read_hap", "cooc")


def run_copy(j):
    out = j.run_fetch(True, True, cap_var=64)
    pile = j.pileup_fetch()
    return dict(variants=out["variants"].copy(), phase={k: (np.array(v) if not isinstance(v, dict) else dict(v)) for k, v in out["phase"].items()},
                pile={k: v.copy() for k, v in pile.items()})


def assert_same_run(a, b, where):
    assert a["variants"].tobytes() == b["variants"].tobytes(), where          # every field, bit for bit
    assert a["phase"]["summary"] == b["phase"]["summary"], where
    for key in RUN_KEYS:
        assert (a["phase"][key] == b["phase"][key]).all(), (where, key)
    for key in a["pile"]:
        assert (a["pile"][key] == b["pile"][key]).all(), (where, key)


@pytest.fixture(scope="module")
def run_case(cases, oracle):
    """B's shape in the synthetic mixture of test_gpu_class.test_stage_results_are_kept: rows, the stage parameters and mirrors, the
    oracle's run, the same run alone on a fresh context, and a control matrix with the control call's expected table."""
    import control_mirror as cm
    n, l = 2049, 130
    sp = synth.SynthParams(seed=5, minor_permille=(150, 120, 100, 80))
    ref = synth.reference(sp.seed, l)
    rows = synth.rows(sp, l, 0, n, ref)
    genes = np.array([(1, l + 1)], dtype=capi.GENE)
    case = ss.Case("run", rows, 21)
    exp_v = oracle.call(rows, genes, refseq=ref)
    exp_p = oracle.phase(rows, exp_v)
    pos_col = np.arange(0, l - 2, 3, dtype=np.uint32)
    hist, cov = oracle.codon_hist(rows, pos_col)
    j = capi.Juliet(0)
    j.upload_rows(rows)
    j.run_async(genes, ref, capi.default_params(), None, True, 10, True)
    alone = run_copy(j)
    j.close()
    control_rows = synth.rows(synth.SynthParams(seed=6, minor_permille=(10, 0, 0, 0)), l, 0, 1025, ref)
    pg, pk, pc, rc, n_tests = cm.positions([(1, l + 1)], l, ref)
    want, want_cov = cm.call_rows(cm.hists(rows, pc), cm.hists(control_rows, pc), pg, pk, pc, rc, 0.01, n_tests)
    assert len(exp_v) >= 2 and exp_p["summary"]["n_haplotypes"] >= 2 and len(want) >= 2      # something to keep
    return dict(rows=rows, ref=ref, genes=genes, case=case, exp_v=exp_v, exp_p=exp_p, col_counts=oracle.pileup(rows), pos_col=pos_col,
                hist=hist, cov=cov, alone=alone, control_rows=control_rows, control=(want, want_cov))


def assert_run_is_the_oracles(got, d):
    exp_v, exp_p = d["exp_v"], d["exp_p"]
    v = got["variants"]
    assert len(v) == len(exp_v)
    for key in ("gene", "codon_pos", "col", "ref_codon", "codon", "count", "coverage", "expected"):
        assert (v[key] == exp_v[key]).all(), key
    assert np.abs(v["p_value"] - exp_v["p_value"]).max() <= 1e-10          # (the bound of the smoke run against the same oracle)
    assert got["phase"]["summary"] == exp_p["summary"]
    for key in ("pos_cols", "hap_count", "hap_pattern", "read_hap"):
        assert (got["phase"][key] == exp_p[key]).all(), key
    assert (got["pile"]["col_counts"] == d["col_counts"]).all()
    assert (got["pile"]["pos_col"] == d["pos_col"]).all()
    assert (got["pile"]["hist"] == d["hist"]).all() and (got["pile"]["coverage"] == d["cov"]).all()


def test_run_and_stages_do_not_see_each_other(ctx, second, run_case):
    from test_gpu_control import assert_table
    d = run_case
    case, genes, ref = d["case"], d["genes"], d["ref"]
    assert_run_is_the_oracles(d["alone"], d)
    second.upload_rows(d["control_rows"])
    second.pileup_async(genes, ref)
    ctx.upload_rows(d["rows"])

    def run():
        ctx.run_async(genes, ref, capi.default_params(), None, True, 10, True)

    def control():
        ctx.control_call_async(second, capi.default_params(alpha=0.01))

    def check(setting, where):
        got = run_copy(ctx)
        assert_same_run(got, d["alone"], where)
        assert_run_is_the_oracles(got, d)
        fetch_all(ctx, case, every(setting), PERM_A, where=(where,))
        rows, cov = ctx.control_call_fetch()
        assert_table(rows, cov, *d["control"], where)
        assert_same_run(run_copy(ctx), d["alone"], (where, "fetched again"))

    run()                                           # the stages and a control call behind the run, before its fetch
    enqueue_all(ctx, case, every(LARGE))
    control()
    check(LARGE, "stages behind the run")
    enqueue_all(ctx, case, every(SMALL), REVERSE)   # the other way round: the run behind the stages and the control call
    control()
    run()
    check(SMALL, "the run behind the stages")
    run()                                           # no upload in between: the captured graph again, stages behind it
    enqueue_all(ctx, case, every(LARGE), PERM_B)
    control()
    check(LARGE, "the graph replayed")
    run()                                           # ... and with nothing around it
    assert_same_run(run_copy(ctx), d["alone"], "the graph replayed alone")
    matrix_is(ctx, d["rows"])


# ------------------------------------------------------------------------------------------------ 5. a refusal in the middle
def test_refusal_between_enqueue_and_fetch(ctx, second, cases):
    """All eight pending on A; one refused call per stage, with the arguments of each stage's own test_refusals*; all eight
    fetched.  codon_deletions and read_stats take no argument that can be wrong while a matrix is resident: their refusals are the
    call without a context (JL_ERR_ARG) and on a second context that holds no matrix (JL_ERR_STATE)."""
    a, lib = cases["A"], ctx.lib
    prm = a.prm[LARGE]
    n_cols = a.rows.shape[1]
    ctx.upload_rows(a.rows)
    enqueue_all(ctx, a, every(LARGE))

    def refused(rc, status, word, j=ctx):
        assert rc == status
        assert word in lib.jl_last_error(j.h).decode(), lib.jl_last_error(j.h)

    ptr = lambda arr: arr.ctypes.data_as(C.c_void_p)
    label, pos, pat = prm["label"], prm["pos_cols"], prm["pattern"]
    beyond = pos.copy()
    beyond[-1] = n_cols - 2                                              # a codon that ends past the window
    refused(lib.jl_class_pileup_async(ctx.h, ptr(label), 705), -1, "at most 704")
    refused(lib.jl_class_codons_async(ctx.h, ptr(label), 17, ptr(beyond), len(beyond)), -1, "ends beyond")
    refused(lib.jl_phase_rescue_async(ctx.h, ptr(beyond), len(beyond), ptr(pat), pat.shape[1], pat.shape[0], 1), -1, "ends beyond")
    refused(lib.jl_phase_nearest_async(ctx.h, ptr(pos), len(pos), ptr(pat), pat.shape[1], pat.shape[0], 1, 8), -1, "max_distance 8")
    refused(lib.jl_phase_recombinants_async(ctx.h, ptr(pos), len(pos), ptr(pat), pat.shape[1], pat.shape[0], 0), -1, "min_positions 0")
    bad_var = prm["var_pos"].copy()
    bad_var[-1] = len(prm["link_pos"])                                   # an index past the positions
    refused(lib.jl_variant_linkage_async(ctx.h, ptr(prm["link_pos"]), len(prm["link_pos"]), ptr(bad_var), ptr(prm["var_codon"]), len(bad_var)), -1, "beyond the 17 positions")
    assert lib.jl_codon_deletions_async(None) == -1 and lib.jl_read_stats_async(None, None) == -1
    refused(lib.jl_codon_deletions_async(second.h), -4, "no resident matrix", second)
    refused(lib.jl_read_stats_async(second.h, None), -4, "no resident matrix", second)
    fetch_all(ctx, a, every(LARGE), PERM_C, raw=True)
    matrix_is(ctx, a.rows)


# ------------------------------------------------------------------------------------------------ 6. one context across shapes
def test_repeat_on_one_context_across_shapes(ctx, cases):
    """A -> B -> C -> A' with every stage called and fetched at each step; C takes the small setting directly after B's large one,
    on mask rows, count tables and staging made for B."""
    for name, settings in (("A", (LARGE,)), ("B", (SMALL, LARGE)), ("C", (SMALL,)), ("A2", (LARGE, SMALL))):
        case = cases[name]
        ctx.upload_rows(case.rows)
        for setting in settings:
            for stage in STAGES:
                enqueue(ctx, stage, case.prm[setting])
                assert_stage(fetch(ctx, stage), case.exp[setting][stage], (name, stage, setting))
        matrix_is(ctx, case.rows)
