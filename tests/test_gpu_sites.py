"""jl_sites_assemble on the device (docs/SPEC.md §18): the site matrix of a resident matrix, called deletions recoded, and the
phasing that exists run on it.  Every expectation is tests/sites_mirror.py — the rule in plain numpy — over the rows that were
uploaded, and the oracle's phasing of the mirror's rows: every cell of the download, and of the phasing the summary, counts,
patterns, hit, every read's id and cooc; never another device result."""
import ctypes as C

import numpy as np
import pytest

import deletion_mirror as dm
import oracle_lib
import sites_mirror as sm
from minorseq_amd import capi, msa

pytestmark = pytest.mark.gpu

GAP, N_, OUT = 4, 5, 6
NF = sm.NO_FILL
MIN_READS = 2


@pytest.fixture(scope="module")
def oracle():
    return oracle_lib.load()


@pytest.fixture(scope="module")
def ctxs():
    src, pc = capi.Juliet(0), capi.Juliet(0)
    yield src, pc
    pc.close()
    src.close()


def make_rows(n, n_cols, dels, seed, n_hap=4):
    """Copies of `n_hap` haplotype rows of bases; haplotype h has the codons at dels[h] deleted.  One read in four is damaged
    somewhere: a one-base deletion, an N, an uncovered cell, or uncovered from there on."""
    rng = np.random.default_rng(seed)
    haps = rng.integers(0, 4, size=(n_hap, n_cols), dtype=np.uint8)
    for h, cols in dels.items():
        for c in cols:
            haps[h, c:c + 3] = GAP
    rows = haps[rng.integers(0, n_hap, size=n)].copy()
    kind = rng.integers(0, 16, size=n)
    at = rng.integers(0, n_cols, size=n)
    for i in np.nonzero(kind < 4)[0]:
        if kind[i] == 3:
            rows[i, at[i]:] = OUT
        else:
            rows[i, at[i]] = (GAP, N_, OUT)[kind[i]]
    return rows


def plant(rows, codon_col, del_col, partial_col):
    """Read 0: a whole codon, a deleted codon and a partly deleted one at three disjoint codon starts."""
    rows[0, codon_col:codon_col + 3] = (0, 1, 2)
    rows[0, del_col:del_col + 3] = GAP
    rows[0, partial_col:partial_col + 3] = (GAP, 1, 2)
    return rows


def holds_all_classes(rows, sites):
    """Nothing passes vacuously: over the sites there are codon reads, del3 reads and damaged ones."""
    codon = del3 = other = 0
    for col, _, _ in sites:
        a, b = sm.classes(rows, col)
        codon, del3, other = codon + a.sum(), del3 + b.sum(), other + (~(a | b)).sum()
    return codon > 0 and del3 > 0 and other > 0


def table_for(rows, sites):
    """A phasing table for the sites (what the front end would build from a variant table): per CODON site up to two observed
    codons other than the commonest as rows, ref_codon the commonest; per DELETION site the pseudo-row."""
    var = []
    for col, kind, _ in sites:
        if kind != sm.CODON or any(v[0] == col for v in var):
            continue
        codon, _ = sm.classes(rows, col)
        idx = 16 * rows[codon, col].astype(np.int64) + 4 * rows[codon, col + 1] + rows[codon, col + 2]
        hist = np.bincount(idx, minlength=64)
        ref = int(hist.argmax())
        seen = [int(c) for c in np.argsort(-hist, kind="stable") if hist[c] and c != ref][:2] or [(ref + 1) % 64]
        var += [(col, ref, c) for c in sorted(seen)]
    out = np.zeros(len(var), dtype=capi.VARIANT)
    for k, (col, ref, c) in enumerate(var):
        out[k]["col"], out[k]["ref_codon"], out[k]["codon"] = col, ref, c
    return sm.build_table(out, sites)


def same_phase(got, exp, nv, n):
    assert got["summary"] == exp["summary"], (got["summary"], exp["summary"])
    h = exp["summary"]["n_haplotypes"]
    s = exp["summary"]
    assert s["reported_reads"] + s["insufficient_reads"] + s["damaged_reads"] == n
    assert (got["pos_cols"] == exp["pos_cols"]).all()
    assert (got["hap_count"] == exp["hap_count"]).all()
    assert (got["hap_pattern"] == exp["hap_pattern"]).all()
    assert (got["hit"][:nv, :h] == exp["hit"]).all()
    assert (got["read_hap"] == exp["read_hap"]).all(), np.nonzero(got["read_hap"] != exp["read_hap"])[0][:8]
    if got["cooc"] is not None:
        assert (got["cooc"][:nv, :nv] == exp["cooc"]).all()


def check(pc, src, rows, sites, oracle, phase=True):
    """`pc` after sites_assemble(src, sites), `rows` what `src` holds."""
    n = rows.shape[0]
    assert holds_all_classes(rows, sites)
    exp = sm.recode(rows, sites)
    assert (pc.n_reads, pc.n_cols) == exp.shape
    packed = pc.download_columns()
    got = msa.unpack_columns(packed, n)
    assert (got == exp).all(), np.argwhere(got != exp)[:8]
    beyond = msa.unpack_columns(packed, 2 * packed.shape[1])[n:]        # what the download shows of the padding
    assert (beyond == OUT).all()
    cnt = pc.codon_deletions()                                          # set pad bits would show in span
    assert (cnt == dm.counts(exp)).all(), np.argwhere(cnt != dm.counts(exp))[:8]
    if phase:
        table = table_for(rows, sites)
        pc.phase_async(table, MIN_READS)
        same_phase(pc.phase_fetch(cap_var=max(64, len(table))), oracle.phase(exp, table, MIN_READS), len(table), n)


# the mixed layout on 20 columns: sites at column 0 and at n_cols - 3, three overlapping sites at c, c + 1, c + 2, a filled codon
# site plus a deletion site at one column.  Haplotype 1 has the codons at 11 and 17 deleted and is a reported haplotype with both
# deletions; haplotype 2 has the codon at 6 deleted, which the overlapping codon sites at 5 and 7 copy as the damage it is there.
L_MIXED = 20


def mixed_sites():
    return [(0, sm.CODON, NF), (5, sm.CODON, NF), (6, sm.DELETION, NF), (7, sm.CODON, NF), (11, sm.CODON, 27), (11, sm.DELETION, NF),
            (17, sm.DELETION, NF)]


def mixed_case(n, seed):
    rows = plant(make_rows(n, L_MIXED, {1: (11, 17), 2: (6,)}, seed), 0, 11, 17)
    return rows, mixed_sites()


# reads: the word (32), the 16-byte piece a lane owns (128), the 128-byte line (1024), a second workgroup's lanes (2049 reads are
# 3 lines = 24 pieces of one 256-lane workgroup; the grid's y carries the sites)
@pytest.mark.parametrize("n", [1, 31, 32, 33, 127, 128, 129, 1023, 1024, 1025, 2049])
def test_mixed_layout_by_reads(ctxs, oracle, n):
    src, pc = ctxs
    rows, sites = mixed_case(n, 100 + n)
    src.upload_rows(rows, win_begin=7)
    pc.sites_assemble(src, sites)
    check(pc, src, rows, sites, oracle)


def test_one_site_in_a_three_column_source(ctxs, oracle):
    src, pc = ctxs
    n = 129
    rows = make_rows(n, 3, {1: (0,)}, 5)
    rows[0], rows[1], rows[2] = (0, 1, 2), GAP, (GAP, 1, 2)
    for sites in ([(0, sm.DELETION, NF)], [(0, sm.CODON, 9)], [(0, sm.CODON, NF)], [(0, sm.CODON, 9), (0, sm.DELETION, NF)]):
        src.upload_rows(rows)
        pc.sites_assemble(src, sites)
        check(pc, src, rows, sites, oracle)


def test_43_sites_are_129_compact_columns(ctxs, oracle):
    src, pc = ctxs
    n, n_cols = 1025, 64
    dels = (9, 30, 60)
    rows = plant(make_rows(n, n_cols, {1: dels}, 43), 0, 30, 60)
    frame = list(range(0, 63, 3))                                       # 21 codon starts of one frame
    sites = [(c, sm.CODON, 5 if c in dels else NF) for c in frame] + [(c, sm.DELETION, NF) for c in frame] + [(1, sm.CODON, NF)]
    sites.sort(key=lambda x: (x[0], x[1]))
    assert len(sites) == 43 and len(set((s[0], s[1]) for s in sites)) == 43
    src.upload_rows(rows)
    pc.sites_assemble(src, sites)
    check(pc, src, rows, sites, oracle)


def test_4096_sites_at_33_reads(ctxs, oracle):
    """The largest table: both kinds at 2048 columns.  Few reads are clean over 4096 positions; the phasing is the multi-word form."""
    src, pc = ctxs
    n, n_cols = 33, 2050
    rng = np.random.default_rng(4096)
    haps = rng.integers(0, 4, size=(2, n_cols), dtype=np.uint8)
    haps[1, 300:303] = GAP
    rows = haps[rng.integers(0, 2, size=n)].copy()
    rows[0, 900:903] = (GAP, 1, 2)
    rows[1, 1200] = N_
    rows[2, 2000:] = OUT
    sites = [(c, k, (int(16 * haps[0, c] + 4 * haps[0, c + 1] + haps[0, c + 2]) if k == sm.CODON and c % 3 == 0 else NF))
             for c in range(2048) for k in (sm.CODON, sm.DELETION)]
    assert len(sites) == sm.SITES_MAX
    src.upload_rows(rows)
    pc.sites_assemble(src, sites)
    n = rows.shape[0]
    assert holds_all_classes(rows, sites)
    exp = sm.recode(rows, sites)
    got = msa.unpack_columns(pc.download_columns(), n)
    assert (got == exp).all(), np.argwhere(got != exp)[:8]
    # one row per site: 4096 positions, the table's capacity
    table = np.zeros(len(sites), dtype=capi.VARIANT)
    table["col"] = 3 * np.arange(len(sites))
    table["codon"] = [sm.DELETED if k == sm.DELETION else 63 for _, k, _ in sites]
    pc.phase_async(table, MIN_READS)
    same_phase(pc.phase_fetch(cap_var=4096), oracle.phase(exp, table, MIN_READS), len(table), n)


def garbage_planes(rows, stride, seed):
    """The planes of `rows` at `stride` bytes a row, every bit past the last read garbage: whole bytes and the rest of the last one,
    among them plane 2 clear (a base that does not exist) and plane 2 alone set (a '-' that does not exist)."""
    n, n_cols = rows.shape
    planes = msa.pack_planes(rows, stride)
    rng = np.random.default_rng(seed)
    nb = (n + 7) // 8
    planes[:, :, nb:] = rng.integers(0, 256, size=(n_cols, 3, stride - nb), dtype=np.uint8)
    if n % 8:
        keep = np.uint8((1 << (n % 8)) - 1)
        last = planes[:, :, nb - 1]
        planes[:, :, nb - 1] = (last & keep) | (rng.integers(0, 256, size=last.shape, dtype=np.uint8) & ~keep)
        planes[::2, 2, nb - 1] &= keep
        planes[1::4, 2, nb - 1] |= ~keep
        planes[1::4, :2, nb - 1] &= keep
    planes[::2, 2, nb:] = 0
    planes[1::4, 2, nb:] = 0xFF
    planes[1::4, :2, nb:] = 0
    return planes


# (reads, the adopted source's plane stride): jl_msa_adopt takes any multiple of 16 that holds the reads.  jl_plane_stride is 128
# for 33 and 129 reads and 384 for 2049: 16, 32 and 272 are smaller (the source ends before the destination's row does, for 2049
# reads inside its third line), 144, 272 and 528 larger.
@pytest.mark.parametrize("n,stride", [(33, 16), (129, 32), (129, 144), (129, 272), (2049, 272), (2049, 528), (1024, 128)])
def test_adopted_source_with_its_own_stride_and_garbage_past_the_reads(oracle, n, stride):
    import torch
    assert stride % 16 == 0 and stride >= (n + 7) // 8
    rows, sites = mixed_case(n, 7 * n + stride)
    planes = garbage_planes(rows, stride, n)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t = torch.from_numpy(planes).cuda(non_blocking=False)
    stream.synchronize()
    src = capi.Juliet(0, stream=stream.cuda_stream)
    src.adopt(t.data_ptr(), n, L_MIXED, stride, keep_alive=t)
    pc = capi.Juliet(0)
    pc.sites_assemble(src, sites)
    assert pc.plane_stride == msa.plane_stride(n)
    check(pc, src, rows, sites, oracle)
    with torch.cuda.stream(stream):
        back = t.cpu().numpy()
    assert (back == planes).all()                                       # the source, garbage included, is what it was
    pc.close()
    src.close()


def test_repeated_calls_growing_and_shrinking(ctxs, oracle):
    src, pc = ctxs
    for n in (40, 3000, 40, 700, 5000, 1):
        rows, sites = mixed_case(n, n)
        src.upload_rows(rows)
        pc.sites_assemble(src, sites)
        check(pc, src, rows, sites, oracle)
        if n > 1:
            pc.sites_assemble(src, sites[2:5])                          # fewer sites into the same context
            check(pc, src, rows, sites[2:5], oracle)


def test_the_source_is_untouched(ctxs, oracle):
    src, pc = ctxs
    rows, sites = mixed_case(1500, 77)
    src.upload_rows(rows, win_begin=3)
    genes = np.array([(4, 4 + 18)], dtype=capi.GENE)
    src.pileup_async(genes)
    pile = src.pileup_fetch()
    dels = src.codon_deletions()
    before = src.download_columns().copy()
    pc.sites_assemble(src, sites)
    check(pc, src, rows, sites, oracle)
    again = src.pileup_fetch()
    for key in pile:
        assert (pile[key] == again[key]).all(), key
    assert (src.codon_deletions_fetch() == dels).all() and (dels == dm.counts(rows)).all()
    assert (src.download_columns() == before).all()
    assert (src.n_reads, src.n_cols) == rows.shape


def test_refusals_leave_the_destination_as_it_was(ctxs, oracle):
    lib = capi.load_library()
    src, pc = ctxs
    rows, sites = mixed_case(200, 9)
    src.upload_rows(rows)
    pc.sites_assemble(src, sites)
    table = table_for(rows, sites)
    pc.phase_async(table, MIN_READS)
    exp_phase = oracle.phase(sm.recode(rows, sites), table, MIN_READS)

    def arr(s):
        a = np.zeros(max(1, len(s)), dtype=capi.SITE)
        for k, x in enumerate(s):
            a[k] = (*x, 0)
        return a

    def refused(src_h, s, n, status, word):
        a = arr(s)
        assert lib.jl_sites_assemble(pc.h, src_h, a.ctypes.data, n) == status
        assert word in lib.jl_last_error(pc.h).decode(), lib.jl_last_error(pc.h).decode()

    good = [(0, sm.CODON, NF)]
    empty = capi.Juliet(0)
    refused(empty.h, good, 1, -4, "no resident matrix")
    empty.close()
    assert lib.jl_sites_assemble(pc.h, None, arr(good).ctypes.data, 1) == -1
    assert lib.jl_sites_assemble(pc.h, src.h, None, 1) == -1
    assert lib.jl_sites_assemble(None, src.h, arr(good).ctypes.data, 1) == -1 and "NULL" in lib.jl_last_error(None).decode()
    refused(pc.h, good, 1, -1, "destination itself")
    refused(src.h, good, 0, -1, "0 sites")
    big = np.zeros(sm.SITES_MAX + 1, dtype=capi.SITE)
    assert lib.jl_sites_assemble(pc.h, src.h, big.ctypes.data, sm.SITES_MAX + 1) == -1 and "4097 sites" in lib.jl_last_error(pc.h).decode()
    refused(src.h, [(L_MIXED - 2, sm.CODON, NF)], 1, -1, "beyond")
    refused(src.h, [(0xFFFFFFFF, sm.CODON, NF)], 1, -1, "beyond")
    refused(src.h, [(0, 2, NF)], 1, -1, "kind 2")
    refused(src.h, [(0, sm.CODON, 64)], 1, -1, "fill 64")
    refused(src.h, [(0, sm.CODON, 0xFE)], 1, -1, "fill 254")
    refused(src.h, [(0, sm.DELETION, 3)], 1, -1, "deletion site with a fill")
    refused(src.h, [(5, sm.CODON, NF), (4, sm.CODON, NF)], 2, -1, "ascending")
    refused(src.h, [(5, sm.DELETION, NF), (5, sm.CODON, NF)], 2, -1, "ascending")
    refused(src.h, [(5, sm.CODON, NF), (5, sm.CODON, 3)], 2, -1, "the same")
    if lib.jl_device_count() > 1:
        far = capi.Juliet(1)
        far.upload_rows(rows)
        refused(far.h, good, 1, -1, "device")
        far.close()
    # what the destination held is still there, its phasing still fetchable
    assert (pc.n_reads, pc.n_cols) == (200, 3 * len(sites))
    assert (msa.unpack_columns(pc.download_columns(), 200) == sm.recode(rows, sites)).all()
    same_phase(pc.phase_fetch(cap_var=64), exp_phase, len(table), 200)


# ---------------------------------------------------------------------------------------------- the command line
import json
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JULIET = os.path.join(ROOT, "minorseq_amd", "bin", "juliet")
SYNTH = os.path.join(ROOT, "minorseq_amd", "bin", "juliet-synth")
FLAGS = ("--mode-phasing", "--call-deletions", "--phase-deletions")


def to_bam(tmp, rows, ref, name):
    mpath, bam, cfg = (str(tmp / f"{name}.{x}") for x in ("msa", "bam", "json"))
    with open(mpath, "wb") as f:
        f.write(np.array([rows.shape[0], rows.shape[1], 0], dtype=np.uint64).tobytes())
        f.write(np.ascontiguousarray(rows, dtype=np.uint8).tobytes())
    refs = "".join("ACGT"[b] for b in ref)
    subprocess.check_call([SYNTH, "--from-rows", mpath, "--ref", refs, "-o", bam])
    json.dump({"genes": [dict(name="G", begin=1, end=len(ref) + 1, drms=[])], "referenceName": "printed", "referenceSequence": refs,
               "version": "tests/test_gpu_sites.py", "databaseVersion": "none"}, open(cfg, "w"))


def juliet(d, *args):
    return subprocess.run([JULIET, *args], cwd=d, capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    if not (os.path.exists(JULIET) and os.path.exists(SYNTH)):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "host")])
    d = tmp_path_factory.mktemp("sites_cli")
    cases = {}
    for name, make in (("a", sm.scenario_a), ("b", sm.scenario_b)):
        rows, ref, var, dels, _ = make()
        to_bam(d, rows, ref, name)
        r = juliet(d, "-c", f"{name}.json", *FLAGS, "--timing", "--haplotype-fasta", f"{name}.fasta", f"{name}.bam", f"{name}_s.json", f"{name}_s.html")
        assert r.returncode == 0, r.stderr
        assert re.search(r"timing sites\s", r.stderr)
        for out, flags in (("d", FLAGS[:2]), ("d2", FLAGS[:2])):
            p = juliet(d, "-c", f"{name}.json", *flags, f"{name}.bam", f"{name}_{out}.json", f"{name}_{out}.html")
            assert p.returncode == 0, p.stderr
        cases[name] = (rows, ref, var, dels)
    return d, cases


def expected_run(oracle, rows, ref, var, dels):
    """The variant table by the oracle, the called deletions by §16's mirror and exact test, the sites, the table and the report
    by §18's mirror, the phasing by the oracle over the mirror's rows."""
    l = rows.shape[1]
    table = oracle.call(rows, np.array([(1, l + 1)], dtype=oracle_lib.GENE), refseq=ref)
    assert table["col"].tolist() == var["col"].tolist() and table["codon"].tolist() == var["codon"].tolist()
    cnt = dm.counts(rows)
    called = [3 * k for k in range(l // 3) if dm.test(cnt[3 * k], 1.0e-3, l // 3)["called"]]
    assert called == dels
    sites = sm.build_sites(table, called)
    rows_t = sm.build_table(table, sites)
    ph = oracle.phase(sm.recode(rows, sites), rows_t)
    return table, sites, ph, sm.report(ph, sites, rows_t)


@pytest.mark.parametrize("name", ["a", "b"])
def test_cli_json_equals_the_mirror_and_the_oracle(cli, oracle, name):
    d, cases = cli
    rows, ref, var, dels = cases[name]
    table, sites, ph, rep = expected_run(oracle, rows, ref, var, dels)
    j = json.load(open(d / f"{name}_s.json"))
    hb, s = j["haplotype"], ph["summary"]
    assert list(hb) == ["reported_reads", "insufficient_coverage_reads", "damaged_reads", "marginal_gaps", "marginal_heteroduplexes",
                        "marginal_partial", "haplotypes", "variant_positions_abs", "deletion_positions_abs"]
    assert [hb[k] for k in list(hb)[:6]] == [s["reported_reads"], s["insufficient_reads"], s["damaged_reads"], s["marginal_gap"],
                                             s["marginal_heteroduplex"], s["marginal_partial"]]
    assert hb["variant_positions_abs"] == rep["variant_positions_abs"] and hb["deletion_positions_abs"] == rep["deletion_positions_abs"]
    assert len(hb["haplotypes"]) == s["n_haplotypes"] == (4 if name == "a" else 3)
    for h, (got, exp) in enumerate(zip(hb["haplotypes"], rep["haplotypes"])):
        assert list(got) == ["name", "reads", "frequency", "deletions", "codons", "read_names"]
        assert got["reads"] == ph["hap_count"][h] and got["frequency"] == ph["hap_count"][h] / s["reported_reads"]
        assert got["codons"] == exp["codons"] and got["deletions"] == exp["deletions"]
        assert sorted(int(n.split("/")[1]) for n in got["read_names"]) == np.nonzero(ph["read_hap"] == h)[0].tolist()
    gene = j["genes"][0]
    hits = [vc["haplotype_hit"] for vp in gene["variant_positions"] for aa in vp["variant_amino_acids"] for vc in aa["variant_codons"]]
    by_codon = {(vp["ref_position"], vc["codon"]): vc["haplotype_hit"] for vp in gene["variant_positions"] for aa in vp["variant_amino_acids"]
                for vc in aa["variant_codons"]}
    assert len(hits) == len(table)
    for v, exp_hit in zip(table, rep["codon_hit"]):
        assert by_codon[(int(v["codon_pos"]), sm.CODONS[v["codon"]])] == exp_hit
    dps = gene["deletion_positions"]
    assert [3 * (e["ref_position"] - 1) for e in dps] == dels
    for e in dps:
        assert list(e)[-1] == "haplotype_hit" and e["haplotype_hit"] == rep["deletion_hit"][3 * (e["ref_position"] - 1)]
    if name == "b":
        plain = json.load(open(d / "b_d.json"))["haplotype"]
        assert plain["damaged_reads"] == 25 and plain["marginal_gaps"] == 25 and hb["damaged_reads"] == 0
        assert hb["haplotypes"][2]["codons"] == ["---"]
    else:
        assert len(json.load(open(d / "a_d.json"))["haplotype"]["haplotypes"]) == 3
    # everything else of the document is the plain run's
    plain = json.load(open(d / f"{name}_d.json"))
    for doc in (j, plain):
        doc["input"].pop("timestamp"), doc["input"].pop("command_line"), doc.pop("haplotype")
        for g in doc["genes"]:
            for e in g["deletion_positions"]:
                e.pop("haplotype_hit", None)
            for vp in g["variant_positions"]:
                for aa in vp["variant_amino_acids"]:
                    for vc in aa["variant_codons"]:
                        vc.pop("haplotype_hit")
    assert j == plain


@pytest.mark.parametrize("name", ["a", "b"])
def test_cli_html_parses_back_to_the_new_leaves(cli, name):
    d, _ = cli
    j = json.load(open(d / f"{name}_s.json"))
    html = open(d / f"{name}_s.html").read()
    hb = j["haplotype"]
    spans = re.search(r'<p id="hap-deletion-positions">(.*?)</p>', html).group(1)
    assert [int(x) for x in re.findall(r"<span>(\d+)</span>", spans)] == hb["deletion_positions_abs"]
    spans = re.search(r'<p id="hap-positions">(.*?)</p>', html).group(1)
    assert [int(x) for x in re.findall(r"<span>(\d+)</span>", spans)] == hb["variant_positions_abs"]
    table = re.search(r'<table id="hap-table">.*?</table>', html, flags=re.S).group(0)
    assert "<th>Deletions</th>" in table
    trs = re.findall(r"<tr><td>(.*?)</td><td>.*?</td><td>(\d+)</td><td>(.*?)</td><td class=\"hap-deletions\">(.*?)</td>", table)
    assert len(trs) == len(hb["haplotypes"])
    for (nm, reads, codons, dels), h in zip(trs, hb["haplotypes"]):
        assert (nm, int(reads), codons.split(" ")) == (h["name"], h["reads"], h["codons"])
        assert [x == "x" for x in dels.split(" ")] == h["deletions"]
    block = re.search(r'<details open id="deletions">.*?</details>', html, flags=re.S).group(0)
    assert re.findall(r'<th class="hapname">(.*?)</th>', block) == [h["name"] for h in hb["haplotypes"]]
    rows_ = re.findall(r'<tr class="deletion">.*?</tr>', block)
    entries = j["genes"][0]["deletion_positions"]
    assert len(rows_) == len(entries)
    for tr, e in zip(rows_, entries):
        assert [c == "hit" for c in re.findall(r'<td class="(hit|nohit)">', tr)] == e["haplotype_hit"]


def test_cli_without_the_flag_nothing_changes(cli):
    d, _ = cli
    for name in ("a", "b"):
        one, two = (open(d / f"{name}_{x}.json").read() for x in ("d", "d2"))
        assert "deletion_positions_abs" not in one and '"deletions"' not in one
        strip = lambda t: re.sub(r'"(timestamp|command_line)": "[^"]*"', "", t)
        assert strip(one) == strip(two)
        assert "hap-deletion-positions" not in open(d / f"{name}_d.html").read()
        h1, h2 = (re.sub(r"<tr><th>(timestamp|command_line)</th>.*?</tr>\n", "", open(d / f"{name}_{x}.html").read()) for x in ("d", "d2"))
        assert h1 == h2


def test_cli_haplotype_fasta_has_one_record_per_haplotype(cli):
    d, _ = cli
    for name, h in (("a", 4), ("b", 3)):
        heads = [ln for ln in open(d / f"{name}.fasta") if ln.startswith(">")]
        hb = json.load(open(d / f"{name}_s.json"))["haplotype"]
        assert len(heads) == h == len(hb["haplotypes"])
        assert [int(re.search(r"reads=(\d+)", ln).group(1)) for ln in heads] == [x["reads"] for x in hb["haplotypes"]]


@pytest.mark.parametrize("args", [["--call-deletions"], ["--mode-phasing"], ["--mode-phasing", "--call-deletions", "--rescue-damaged"],
                                  ["--mode-phasing", "--call-deletions", "--windows", "2"], ["--mode-phasing", "--call-deletions", "--devices", "0,0"]])
def test_cli_refused_combinations_open_nothing(tmp_path, args):
    r = juliet(tmp_path, "--phase-deletions", *args, "no_such.bam", "o.json")
    assert r.returncode == 1 and "-deletions" in r.stderr, (r.returncode, r.stderr)
    assert not list(tmp_path.iterdir())


def test_cli_refused_with_batch_and_as_fuse(tmp_path):
    (tmp_path / "l.tsv").write_text("no_such.bam\ta.json\n")
    r = juliet(tmp_path, "--phase-deletions", "--mode-phasing", "--call-deletions", "--batch", "l.tsv")
    assert r.returncode == 1 and "--batch" in r.stderr
    r = subprocess.run([os.path.join(ROOT, "minorseq_amd", "bin", "fuse"), "--phase-deletions", "no_such.bam", "o.fasta"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "fuse" in r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == ["l.tsv"]
