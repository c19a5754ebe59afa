"""jl_phase_rescue_async on the device (docs/SPEC.md §14): which reported haplotype a read agrees with at the variant positions
where it can be read, and `juliet --mode-phasing --rescue-damaged` on top of it.  Every expectation is tests/rescue_mirror.py —
the rule in plain loops — over the rows that were uploaded, compared for equality on every read; never another device result."""
import json
import os
import subprocess

import numpy as np
import pytest

import rescue_mirror
import second_turn as st
from minorseq_amd import capi, msa, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JULIET = os.path.join(ROOT, "minorseq_amd", "bin", "juliet")
SYNTH = os.path.join(ROOT, "minorseq_amd", "bin", "juliet-synth")


@pytest.fixture(scope="module", autouse=True)
def built():
    """The binaries normally travel with the tree; build them only if they are missing (never under a loaded .so)."""
    if not os.path.exists(os.path.join(ROOT, "minorseq_amd", "libjuliet_hip.so")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "csrc")])
    if not (os.path.exists(JULIET) and os.path.exists(SYNTH)):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "host")])


@pytest.fixture(scope="module")
def ctx():
    j = capi.Juliet(0)
    yield j
    j.close()


def positions(vp):
    """Vp codon starts on a window just large enough: the first at column 0, the second overlapping it (columns 0 and 1, two
    frames), the last at n_cols - 3.  Returns (pos_cols, n_cols)."""
    cols = [0, 1][:vp] + [3 * k - 2 for k in range(2, vp)]
    return np.array(cols, dtype=np.uint32), cols[-1] + 3


def codons_at(base_rows, pos_cols):
    c = pos_cols.astype(np.int64)
    return (16 * base_rows[:, c] + 4 * base_rows[:, c + 1] + base_rows[:, c + 2]).astype(np.uint8)


def make_case(n, vp, n_hap, seed):
    """Seeded haplotype rows of bases — every odd one a copy of its predecessor with ONE base of one codon changed — and reads that
    are copies of them with seeded damage: '-' and N cells, ragged code-6 ends, reads of code 6 throughout, single-base
    substitutions (such a read agrees with nobody), and reads whose only damage opens the position at which their haplotype
    differs from its twin (both agree then).  Returns (rows, pos_cols, pattern)."""
    rng = np.random.default_rng(seed)
    pos_cols, n_cols = positions(vp)
    haps = rng.integers(0, 4, size=(n_hap, n_cols), dtype=np.uint8)
    twin_col = np.zeros(n_hap, dtype=np.int64)
    for h in range(1, n_hap, 2):
        haps[h] = haps[h - 1]
        twin_col[h] = twin_col[h - 1] = int(pos_cols[rng.integers(0, vp)]) + 2     # the third base of a codon
        haps[h, twin_col[h]] = (haps[h, twin_col[h]] + 1 + rng.integers(0, 3)) % 4
    of = rng.integers(0, n_hap, size=n)
    rows = haps[of].copy()
    kind = rng.integers(0, 10, size=n)
    cell = rng.random(size=rows.shape)
    some = (kind == 0) | (kind == 1) | (kind == 2)                    # scattered damage, about one cell a read and more
    rows[some[:, None] & (cell < 1.5 / n_cols)] = 4
    rows[some[:, None] & (cell > 1.0 - 1.5 / n_cols)] = 5
    lo, hi = rng.integers(0, n_cols // 3 + 1, size=n), n_cols - rng.integers(0, n_cols // 3 + 1, size=n)
    ci = np.arange(n_cols)[None, :]
    rows[(kind == 3)[:, None] & ((ci < lo[:, None]) | (ci >= hi[:, None]))] = 6
    rows[kind == 4] = 6                                               # nothing of the read lies in the window
    for i in np.flatnonzero(kind == 5):                               # a substitution in a codon
        c = int(pos_cols[rng.integers(0, vp)]) + int(rng.integers(0, 3))
        rows[i, c] = (rows[i, c] + 1 + rng.integers(0, 3)) % 4
    for i in np.flatnonzero(kind == 6):                               # open exactly where the twins differ
        rows[i, twin_col[of[i]]] = 4 + int(rng.integers(0, 3))
    return rows, pos_cols, codons_at(haps, pos_cols)


def check(j, rows, pos_cols, pattern, min_positions, all_four=False):
    exp_rescue, exp_reads, exp_tally = rescue_mirror.rescue(rows, pos_cols, pattern, min_positions)
    if all_four:
        assert (exp_tally > 0).all(), exp_tally                       # no category passes vacuously
    out = j.phase_rescue(pos_cols, pattern, min_positions)
    assert out["rescue"].dtype == np.uint16 and out["rescue"].shape == (len(rows),)
    assert (out["rescue"] == exp_rescue).all()
    assert (out["hap_reads"] == exp_reads).all()
    assert (out["tally"] == exp_tally).all()
    assert int(out["tally"].sum()) == len(rows)
    return out


# (reads, positions, haplotypes, min_positions or "vp", all four categories occur): the word / run of 64 / two-workgroup edges of
# the reads, the tile of 64 positions and the dword of four, the chunk of 64 haplotypes (ids with bit 9 at 513 and 702), sparsely paired
CASES = [
    (1, 1, 1, 1, False), (31, 2, 2, 1, True), (32, 63, 63, 2, True), (33, 64, 64, "vp", False), (1023, 65, 65, 1, True),
    (1024, 130, 128, 2, True), (1025, 1, 129, 1, False), (2049, 2, 513, 2, False), (2049, 130, 702, 1, True), (33, 65, 702, "vp", False),
    (1025, 64, 2, 1, True), (31, 130, 1, 1, False), (1023, 63, 129, "vp", False), (1024, 2, 64, 1, True), (32, 1, 2, 1, False),
    (2049, 65, 513, 2, True), (1, 130, 702, 1, False), (1025, 63, 65, 2, True),
]


@pytest.mark.parametrize("n,vp,n_hap,min_positions,all_four", CASES)
def test_rescue_equals_mirror(ctx, n, vp, n_hap, min_positions, all_four):
    rows, pos_cols, pattern = make_case(n, vp, n_hap, 1000 * n + 7 * vp + n_hap)
    assert pos_cols[0] == 0 and pos_cols[-1] == rows.shape[1] - 3 and (vp < 2 or pos_cols[1] == 1)
    ctx.upload_rows(rows, win_begin=3)
    check(ctx, rows, pos_cols, pattern, vp if min_positions == "vp" else min_positions, all_four)
    assert (msa.unpack_columns(ctx.download_columns(), n) == rows).all()     # the matrix is untouched


def test_adopted_matrix_with_its_own_stride():
    """A torch tensor as the matrix: 2049 reads in planes of 272 bytes (the library's own stride is 384), garbage in the bytes
    past ceil(n / 8) of every plane row.  None of it may show in any read's answer or in a count."""
    import torch
    n, vp, n_hap, stride = 2049, 65, 129, 272
    assert stride != msa.plane_stride(n) and stride % 16 == 0
    rows, pos_cols, pattern = make_case(n, vp, n_hap, 99)
    planes = msa.pack_planes(rows, stride)
    planes[:, :, (n + 7) // 8:] = np.random.default_rng(1).integers(0, 256, size=(rows.shape[1], 3, stride - (n + 7) // 8), dtype=np.uint8)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t = torch.from_numpy(planes).cuda(non_blocking=False)
    stream.synchronize()
    j = capi.Juliet(0, stream=stream.cuda_stream)
    j.adopt(t.data_ptr(), n, rows.shape[1], stride, keep_alive=t)
    check(j, rows, pos_cols, pattern, 1, all_four=True)
    check(j, rows, pos_cols[:3], pattern[:2, :3], 3)
    j.close()


# (positions, haplotypes): two chunks of haplotypes at few positions, two tiles of positions at few haplotypes
SECOND_TURN_SHAPES = [(5, 65), (65, 2)]


def second_turn_block(vp, n_hap):
    """The 2049-read case of this file's builder at the shape, cut to the block of st.BLOCK reads; (block, pos_cols, pattern)."""
    rows, pos_cols, pattern = make_case(2049, vp, n_hap, 1000 * 2049 + 7 * vp + n_hap)
    return rows[:st.BLOCK], pos_cols, pattern


def second_turn_expectation(block, pos_cols, pattern, n):
    """(rescue, hap_reads, tally) of the n tiled reads from the mirror over the block and over the tail."""
    whole = rescue_mirror.rescue(block, pos_cols, pattern, 1)
    tail = rescue_mirror.rescue(block[:st.split(n)[1]], pos_cols, pattern, 1)
    return st.tiled(whole[0], n), st.summed(whole[1], tail[1], n, st.BLOCK), st.summed(whole[2], tail[2], n, st.BLOCK)


@pytest.mark.parametrize("vp,n_hap", SECOND_TURN_SHAPES)
@pytest.mark.parametrize("n,what", st.COUNTS)
def test_a_workgroups_second_turn(n, what, vp, n_hap):
    """More than 4096 runs: a workgroup walks a second run — its verdicts and `informative` start again, its histogram and tallies
    are carried into one flush.  The rows are the block repeated (tests/second_turn.py)."""
    block, pos_cols, pattern = second_turn_block(vp, n_hap)
    exp_rescue, exp_reads, exp_tally = second_turn_expectation(block, pos_cols, pattern, n)
    assert int(exp_tally.sum()) == n
    if n - st.ONE_TURN > 1:                                 # all four categories among the reads of the second turns
        late = exp_rescue[st.second_turn_reads(n)]
        assert (late < n_hap).any() and (late == rescue_mirror.AMBIGUOUS).any() and (late == rescue_mirror.NONE).any() and (late == rescue_mirror.UNINFORMATIVE).any()
    j = capi.Juliet(0)
    try:
        st.adopt_tiled(j, block, n)
        out = j.phase_rescue(pos_cols, pattern, 1)
        assert out["rescue"].shape == (n,) and (out["rescue"] == exp_rescue).all(), np.flatnonzero(out["rescue"] != exp_rescue)[:8]
        assert (out["hap_reads"] == exp_reads).all() and (out["tally"] == exp_tally).all()
        assert int(out["tally"].sum()) == n
    finally:
        j.close()


def test_repeat_on_one_context(ctx):
    """(130, 702), then (2, 2), then (65, 129) on one matrix: no stale pattern, position, id or count shows.  Then a call that
    only enqueues, its inputs overwritten at once: they were copied before it returned."""
    n = 1025
    rows, pos_cols, pattern = make_case(n, 130, 702, 12)
    ctx.upload_rows(rows)
    check(ctx, rows, pos_cols, pattern, 1)
    check(ctx, rows, pos_cols[:2], pattern[:2, :2].copy(), 2)
    check(ctx, rows, pos_cols[:65], pattern[:129, :65].copy(), 1)
    cols, pat = pos_cols[:64].copy(), pattern[:65, :64].copy()
    exp = rescue_mirror.rescue(rows, cols, pat, 2)
    assert ctx.phase_rescue(cols, pat, 2, wait=False) is None
    cols[:] = 0
    pat[:] = 63
    out = ctx.phase_rescue_fetch()
    assert (out["rescue"] == exp[0]).all() and (out["hap_reads"] == exp[1]).all() and (out["tally"] == exp[2]).all()


def test_staging_grows_and_is_reused(ctx):
    """1500 reads and 3 positions, then 5000 and 40, then 1500 and 3 again, at 60 columns on one context: the staging of positions
    and pattern and the buffers of the ids grow for the second call and serve the third, larger than it needs."""
    l, n_hap = 60, 9
    for seed, (n, cols) in enumerate(((1500, [0, 1, 57]), (5000, list(range(20)) + list(range(38, 58))), (1500, [0, 1, 57]))):
        rng = np.random.default_rng(70 + seed)
        pos_cols = np.array(cols, dtype=np.uint32)
        haps = rng.integers(0, 4, size=(n_hap, l), dtype=np.uint8)
        rows = haps[rng.integers(0, n_hap, size=n)]
        cell = rng.random(size=rows.shape)
        rows[cell < 0.01] = 4                       # scattered '-', N and uncovered cells
        rows[cell > 0.99] = 5
        rows[(cell > 0.49) & (cell < 0.50)] = 6
        sub = (cell > 0.200) & (cell < 0.203) & (rows < 4)      # a substitution: such a read may agree with nobody
        rows[sub] = (rows[sub] + 1) % 4
        ctx.upload_rows(rows)
        check(ctx, rows, pos_cols, codons_at(haps, pos_cols), 1 if len(cols) == 3 else 2)


def fetch_copy(j):
    out = j.run_fetch(True, True, cap_var=64)
    return dict(variants=out["variants"].copy(), phase={k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in out["phase"].items()})


def assert_same_run(a, b):
    assert (a["variants"] == b["variants"]).all()
    pa, pb = a["phase"], b["phase"]
    assert pa["summary"] == pb["summary"]
    for key in ("pos_cols", "hap_count", "hap_pattern", "hit", "read_hap", "cooc"):
        assert (pa[key] == pb[key]).all(), key


def test_after_a_real_run(ctx):
    """A run with phasing over reads with deletions, masked bases and partial reads; then the rule with the run's own positions
    and haplotypes, over all reads: the consequences of §14 hold, the run's results are what they were, a second run equals the first."""
    n, l = 2049, 130
    sp = synth.SynthParams(seed=5, del_rate=4e-3, mask_rate=2e-2, partial_rate=0.1, minor_permille=(150, 120, 100, 80))
    ref = synth.reference(sp.seed, l)
    rows = synth.rows(sp, l, 0, n, ref)
    genes = np.array([(1, l + 1)], dtype=capi.GENE)
    ctx.upload_rows(rows)
    ctx.run_async(genes, ref, capi.default_params(), None, True, 10, True)
    first = fetch_copy(ctx)
    ph = first["phase"]
    n_hap, vp = ph["summary"]["n_haplotypes"], ph["summary"]["n_positions"]
    read_hap, pos_cols, pattern = ph["read_hap"], ph["pos_cols"][:vp], ph["hap_pattern"][:n_hap, :vp]
    damaged = read_hap == capi.HAP_DAMAGED
    assert n_hap >= 2 and vp >= 2 and damaged.sum() >= 1 and damaged.sum() == ph["summary"]["damaged_reads"]
    for min_positions in (1, vp):
        out = check(ctx, rows, pos_cols, pattern, min_positions)
        res = out["rescue"]
        for h in range(n_hap):
            assert (res[read_hap == h] == h).all()                                     # a clean read keeps its haplotype
            assert out["hap_reads"][h] - ph["hap_count"][h] == (damaged & (res == h)).sum()
        assert (res[read_hap == capi.HAP_INSUFFICIENT] == capi.RESCUE_NONE).all()
    assert (damaged & (res == capi.RESCUE_UNINFORMATIVE)).sum() == damaged.sum()       # min_positions = Vp: no damaged read has them all
    assert_same_run(first, fetch_copy(ctx))
    assert (msa.unpack_columns(ctx.download_columns(), n) == rows).all()
    ctx.run_async(genes, ref, capi.default_params(), None, True, 10, True)
    assert_same_run(first, fetch_copy(ctx))


def test_refusals_change_nothing():
    lib = capi.load_library()
    j = capi.Juliet(0)
    rows, pos_cols, pattern = make_case(40, 3, 4, 1)           # 8 columns: codons at 0, 1, 4
    n_cols = rows.shape[1]

    def refused(status, word, cols=pos_cols, n_pos=3, pat=pattern, stride=3, n_hap=4, min_positions=1):
        rc = lib.jl_phase_rescue_async(j.h, None if cols is None else cols.ctypes.data, n_pos, None if pat is None else pat.ctypes.data,
                                       stride, n_hap, min_positions)
        assert rc == status
        assert word in lib.jl_last_error(j.h).decode(), lib.jl_last_error(j.h)

    refused(-4, "no resident matrix")
    j.upload_rows(rows)
    res = np.zeros(40, dtype=np.uint16)
    assert lib.jl_phase_rescue_fetch(j.h, res.ctypes.data, None, None) == -4          # a fetch before any call
    assert "before jl_phase_rescue_async" in lib.jl_last_error(j.h).decode()
    good = j.phase_rescue(pos_cols, pattern, 2)
    exp = rescue_mirror.rescue(rows, pos_cols, pattern, 2)
    assert (good["rescue"] == exp[0]).all()
    big_cols = np.arange(4097, dtype=np.uint32)
    big_pat = np.zeros((703, 3), dtype=np.uint8)
    refused(-1, "no positions array", cols=None)
    refused(-1, "no pattern array", pat=None)
    refused(-1, "0 positions", n_pos=0)
    refused(-1, "4097 positions", cols=big_cols, n_pos=4097, stride=4097)
    refused(-1, "0 haplotypes", n_hap=0)
    refused(-1, "703 haplotypes", pat=big_pat, n_hap=703)
    refused(-1, "pattern_stride", stride=2)
    refused(-1, "min_positions 0", min_positions=0)
    refused(-1, "min_positions 4", min_positions=4)
    refused(-1, "ends beyond the window", cols=np.array([0, 1, n_cols - 2], dtype=np.uint32))
    refused(-1, "not strictly ascending", cols=np.array([0, 4, 4], dtype=np.uint32))
    refused(-1, "not strictly ascending", cols=np.array([1, 0, 4], dtype=np.uint32))
    bad = pattern.copy()
    bad[3, 2] = 64
    refused(-1, "is no codon", pat=bad)
    again = j.phase_rescue_fetch()                                                    # what was enqueued before is still there
    for key in good:
        assert (again[key] == good[key]).all(), key
    # any pointer of the fetch may be NULL
    tally = np.zeros(4, dtype=np.uint64)
    assert lib.jl_phase_rescue_fetch(j.h, None, None, tally.ctypes.data) == 0 and (tally == exp[2]).all()
    assert lib.jl_phase_rescue_fetch(j.h, None, None, None) == 0
    assert (msa.unpack_columns(j.download_columns(), 40) == rows).all()
    j.close()


def test_the_limits_themselves_are_accepted(ctx):
    """H = 702 and Vp = 130 (CASES), and the variant table's capacity itself: 4096 positions on 4098 columns, every codon
    overlapping its neighbours."""
    n, n_cols = 70, 4098
    rng = np.random.default_rng(8)
    haps = rng.integers(0, 4, size=(3, n_cols), dtype=np.uint8)
    rows = haps[rng.integers(0, 3, size=n)].copy()
    rows[rng.random(size=rows.shape) < 2e-4] = 4
    rows[5] = 6
    pos_cols = np.arange(4096, dtype=np.uint32)
    ctx.upload_rows(rows)
    out = check(ctx, rows, pos_cols, codons_at(haps, pos_cols), 4000)
    assert out["tally"][0] > 0 and out["tally"][3] > 0


# ---------------------------------------------------------------------------------------------- the command line
N_CLI, L_CLI, SEED_CLI = 3000, 300, 41
MINOR = (150, 120, 100, 80)
NEW_HAP_KEYS = ("rescued_reads", "rescued_read_names", "frequency_with_rescued")


def read_msa(path):
    raw = open(path, "rb").read()
    n, l, wb = (int(x) for x in np.frombuffer(raw[:24], dtype=np.uint64))
    return np.frombuffer(raw[24:], dtype=np.uint8).reshape(n, l), wb


def juliet(d, *args):
    return subprocess.run([JULIET, *args], cwd=d, capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    """Reads with deletions and filtered bases (the generator's default rates) and one in ten partial; the rows from --dump-msa;
    one run with the flag (JSON, HTML, FASTA) and one without."""
    d = tmp_path_factory.mktemp("rescue_cli")
    subprocess.check_call([SYNTH, "--reads", str(N_CLI), "--cols", str(L_CLI), "--seed", str(SEED_CLI), "--partial", "0.1",
                           "--minor-permille", *map(str, MINOR), "-o", str(d / "in.bam"), "--config-out", str(d / "cfg.json")])
    subprocess.check_call([JULIET, "-c", "cfg.json", "--dump-msa", "in.msa", "in.bam"], cwd=d)      # host only: no GPU involved
    rows, wb = read_msa(d / "in.msa")
    assert rows.shape[0] == N_CLI
    r = juliet(d, "-c", "cfg.json", "--mode-phasing", "--rescue-damaged", "--haplotype-fasta", "r.fasta", "--timing", "in.bam", "r.json", "r.html")
    assert r.returncode == 0, r.stderr
    assert "rescue" in r.stderr                                # the stage line of --timing
    p = juliet(d, "-c", "cfg.json", "--mode-phasing", "--haplotype-fasta", "plain.fasta", "in.bam", "plain.json", "plain.html")
    assert p.returncode == 0, p.stderr
    return d, rows, wb


def index_of(name):
    return int(name.split("/")[1])


def mirror_of_json(j, rows, wb, min_positions):
    """The rule over the JSON's own positions and codons: (rescue per read, damaged per read, pattern)."""
    hb = j["haplotype"]
    pos_cols = np.array([p - wb - 1 for p in hb["variant_positions_abs"]], dtype=np.uint32)
    pattern = np.array([[16 * "ACGT".index(c[0]) + 4 * "ACGT".index(c[1]) + "ACGT".index(c[2]) for c in h["codons"]] for h in hb["haplotypes"]],
                       dtype=np.uint8).reshape(len(hb["haplotypes"]), len(pos_cols))
    damaged = np.zeros(len(rows), dtype=bool)                  # §8: a code above T at any cell of any variant codon
    for c in pos_cols:
        damaged |= (rows[:, c:c + 3] >= 4).any(axis=1)
    return rescue_mirror.rescue(rows, pos_cols, pattern, min_positions)[0], damaged


def check_json_against_mirror(j, rows, wb, min_positions, subset=None):
    hb = j["haplotype"]
    haps = hb["haplotypes"]
    res, damaged = mirror_of_json(j, rows, wb, min_positions)
    if subset is not None:
        damaged = damaged & subset
    rs = hb["rescue"]
    assert rs["min_positions"] == min_positions
    assert rs["assigned_reads"] + rs["ambiguous_reads"] + rs["incompatible_reads"] + rs["uninformative_reads"] == hb["damaged_reads"]
    if subset is None:
        assert damaged.sum() == hb["damaged_reads"]
        assert rs["assigned_reads"] == (damaged & (res < len(haps))).sum()
        assert rs["ambiguous_reads"] == (damaged & (res == rescue_mirror.AMBIGUOUS)).sum()
        assert rs["incompatible_reads"] == (damaged & (res == rescue_mirror.NONE)).sum()
        assert rs["uninformative_reads"] == (damaged & (res == rescue_mirror.UNINFORMATIVE)).sum()
    total = sum(h["reads"] + h["rescued_reads"] for h in haps)
    for k, h in enumerate(haps):
        got = [index_of(name) for name in h["rescued_read_names"]]
        assert h["rescued_reads"] == len(got)
        if subset is None:
            assert got == np.flatnonzero(damaged & (res == k)).tolist()          # exactly the mirror's reads, in read order
        else:
            assert got == sorted(got) and all(damaged[i] and res[i] == k for i in got)
        assert h["frequency_with_rescued"] == ((h["reads"] + h["rescued_reads"]) / total if total else 0.0)
        assert all(res[index_of(name)] == k for name in h["read_names"])         # a clean read keeps its haplotype
    return rs


def test_cli_json_equals_the_mirror(cli):
    d, rows, wb = cli
    j = json.load(open(d / "r.json"))
    assert len(j["haplotype"]["haplotypes"]) >= 3 and j["haplotype"]["damaged_reads"] >= 100     # nothing passes vacuously
    rs = check_json_against_mirror(j, rows, wb, 1)
    assert rs["assigned_reads"] > 0 and sum(h["rescued_reads"] for h in j["haplotype"]["haplotypes"]) == rs["assigned_reads"]
    html = open(d / "r.html").read()
    assert 'id="hap-rescue"' in html and 'data-key="assigned_reads"' in html and 'id="hap-rescued"' in html
    assert 'hap-rescue' not in open(d / "plain.html").read()


def strip(j):
    j["input"].pop("timestamp")
    j["input"].pop("command_line")
    j["haplotype"].pop("rescue", None)
    for h in j["haplotype"]["haplotypes"]:
        for key in NEW_HAP_KEYS:
            h.pop(key, None)
    return j


def test_cli_without_the_new_keys_the_json_is_the_plain_run(cli):
    d, rows, wb = cli
    with_flag, plain = json.load(open(d / "r.json")), json.load(open(d / "plain.json"))
    assert "rescue" in with_flag["haplotype"] and "rescue" not in plain["haplotype"]
    assert all(key in h for h in with_flag["haplotype"]["haplotypes"] for key in NEW_HAP_KEYS)
    assert not any(key in h for h in plain["haplotype"]["haplotypes"] for key in NEW_HAP_KEYS)
    assert strip(with_flag) == strip(plain)


def json_number(v):
    """A number as the JSON writer prints it."""
    return "%.0f" % v if v == int(v) else "%.17g" % v


def expected_fasta(j, rows, wb, source, rescued):
    """§13 in numpy: per haplotype of the JSON, in its order, the consensus of the rows its read_names — and, with the flag, its
    rescued_read_names — name."""
    out = []
    n_cols = rows.shape[1]
    for h in j["haplotype"]["haplotypes"]:
        names = h["read_names"] + (h["rescued_read_names"] if rescued else [])
        members = rows[[index_of(name) for name in names]]
        counts = np.stack([(members == s).sum(axis=0) for s in range(5)], axis=1)
        best = np.argmax(counts, axis=1)                    # the first maximum: the lowest code on ties
        seq = "".join("N" if counts[c].max() == 0 else "ACGT"[best[c]] for c in range(n_cols) if counts[c].max() == 0 or best[c] != 4)
        extra = f" rescued={h['rescued_reads']}" if rescued else ""
        out.append(f">{h['name']} reads={h['reads']}{extra} frequency={json_number(h['frequency'])} window={wb + 1}-{wb + n_cols} source={source}\n")
        out.extend(seq[i:i + 70] + "\n" for i in range(0, len(seq), 70))
    return "".join(out)


def test_cli_fasta_takes_the_rescued_reads_in(cli):
    d, rows, wb = cli
    j = json.load(open(d / "r.json"))
    assert open(d / "r.fasta").read() == expected_fasta(j, rows, wb, "in.bam", True)
    assert open(d / "plain.fasta").read() == expected_fasta(j, rows, wb, "in.bam", False)     # without the flag: as it was


def test_cli_follows_the_taken_window_and_the_threshold(cli):
    d, rows, wb = cli
    r = juliet(d, "-c", "cfg.json", "--mode-phasing", "--downsample", "1000", "--rescue-damaged", "--rescue-min-positions", "2",
               "--haplotype-fasta", "ds.fasta", "in.bam", "ds.json")
    assert r.returncode == 0, r.stderr
    j = json.load(open(d / "ds.json"))
    assert j["target_config"]["n_reads"] == 1000 and len(j["haplotype"]["haplotypes"]) >= 2
    rs = check_json_against_mirror(j, rows, wb, 2, subset=np.ones(len(rows), dtype=bool))
    assert 0 < rs["assigned_reads"] <= j["haplotype"]["damaged_reads"] <= 1000
    assert open(d / "ds.fasta").read() == expected_fasta(j, rows, wb, "in.bam", True)
    # more informative positions asked for than the run has: nobody can be judged
    r = juliet(d, "-c", "cfg.json", "--mode-phasing", "--rescue-damaged", "--rescue-min-positions", "4000", "in.bam", "k.json")
    assert r.returncode == 0, r.stderr
    hb = json.load(open(d / "k.json"))["haplotype"]
    assert hb["rescue"] == dict(min_positions=4000, assigned_reads=0, ambiguous_reads=0, incompatible_reads=0, uninformative_reads=hb["damaged_reads"])
    assert all(h["rescued_reads"] == 0 and h["rescued_read_names"] == [] for h in hb["haplotypes"])


def test_cli_no_reported_haplotype_is_the_zero_block(tmp_path):
    """Reads without a minor clone: nothing is called, nothing is phased, no call is made; the block has zeros and exit status 0."""
    subprocess.check_call([SYNTH, "--reads", "400", "--cols", "90", "--seed", "3", "--minor-permille", "0", "0", "0", "0",
                           "-o", str(tmp_path / "in.bam"), "--config-out", str(tmp_path / "cfg.json")])
    r = juliet(tmp_path, "-c", "cfg.json", "--mode-phasing", "--rescue-damaged", "in.bam", "out.json")
    assert r.returncode == 0, r.stderr
    hb = json.load(open(tmp_path / "out.json"))["haplotype"]
    assert hb["haplotypes"] == []
    assert hb["rescue"] == dict(min_positions=1, assigned_reads=0, ambiguous_reads=0, incompatible_reads=0, uninformative_reads=hb["damaged_reads"])
