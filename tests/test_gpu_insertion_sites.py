"""Called insertion alleles as haplotype sites on the device (docs/SPEC.md §19): the per-read events of a record build
(jl_msa_track_insertion_reads, jl_insertion_reads_fetch), the site matrix with insertion sites (jl_sites_assemble_alleles), the
phasing that exists run on it, and `juliet --phase-insertions`.  Every expectation is tests/insertion_sites_mirror.py — the rules as
plain loops over the record arrays and the expanded rows — and the oracle's phasing of the mirror's rows; never another device
result."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import deletion_mirror as dm
import insertion_mirror as im
import insertion_sites_mirror as ism
import oracle_lib
import records_expand
import sites_mirror as sm
from minorseq_amd import capi, msa
from test_gpu_insertions import CASES, JULIET, L_CLI, N_CLI, PLANT_COL, PLANT_LEN, PLANT_PERMILLE, QMASK, SPLIT_COL, SYNTH, WB, expected_entries, \
    make_reads, read_bam, rows_of, upload, with_anchors
from test_gpu_sites import garbage_planes, same_phase
from test_insertion_sites_host import J_FIRST, J_LAST, J_MANY, J_MIXED, L, NF, holds_all_classes, key, listed_alleles, site_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = 6
MIN_READS = 2


@pytest.fixture(scope="module", autouse=True)
def built():
    """The binaries normally travel with the tree; build them only if they are missing (never under a loaded .so)."""
    if not os.path.exists(os.path.join(ROOT, "minorseq_amd", "libjuliet_hip.so")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "csrc")])
    if not (os.path.exists(JULIET) and os.path.exists(SYNTH)):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "host")])


@pytest.fixture(scope="module")
def oracle():
    return oracle_lib.load()


@pytest.fixture(scope="module")
def ctx():
    j = capi.Juliet(0)
    j.track_insertion_reads()                                # (implies the alleles)
    yield j
    j.close()


@pytest.fixture(scope="module")
def ctxs():
    src, pc = capi.Juliet(0), capi.Juliet(0)
    src.track_insertion_reads()
    yield src, pc
    pc.close()
    src.close()


# ---------------------------------------------------------------------------------------------- the events
def check_events(j, rec, n_cols, form="bytes", min_qv=20, wb=WB, need_all=True):
    """Build with the read switch on; the events row for row, and in the same build jcnt and the allele table, against the mirrors."""
    upload(j, rec, n_cols, form, min_qv, wb)
    qmask = QMASK(rec) if form == "mask" else None
    exp = ism.events(rec, n_cols, wb, min_qv, qmask)
    exp_cnt, exp_alleles = im.walk(rec, n_cols, wb, min_qv, qmask)
    if need_all:                                             # nothing passes vacuously
        assert {e[3] for e in exp} == {1, 2, 3} and len(exp_alleles) >= 2
    got = j.insertion_reads()
    exp_rows = ism.event_rows(exp)
    assert got.dtype == capi.INSERTION_EVENT and len(got) == len(exp_rows)
    assert (got == exp_rows).all(), (got[got != exp_rows][:4], exp_rows[got != exp_rows][:4])
    jcnt, rows = j.insertion_alleles()
    assert (jcnt == exp_cnt).all() and len(rows) == len(exp_alleles) and (rows == rows_of(exp_alleles)).all()
    return got


@pytest.mark.parametrize("n,n_cols", CASES)
def test_events_equal_mirror(ctx, n, n_cols):
    rec = im.records(make_reads(n, n_cols, 1000 * n + n_cols), with_qual=True)
    check_events(ctx, rec, n_cols)
    assert (msa.unpack_columns(ctx.download_columns(), n) == records_expand.expand_reference(rec, n_cols, WB, 20)).all()


@pytest.mark.parametrize("form,min_qv", [("bytes", 20), ("mask", 20), ("chunks", 20), ("bytes", 0), ("mask", 0)])
def test_events_in_the_filter_forms(ctx, form, min_qv):
    reads = make_reads(300, 40, 5)
    reads += [(WB, [("=", 5), ("I", 3), ("=", 5)], "ACGTA" + "GGG" + "ACGTA", [40] * 5 + [40, 19, 40] + [40] * 5)]
    rec = im.records(reads, with_qual=True)
    got = check_events(ctx, rec, 40, form, min_qv)
    last = got[got["read"] == 300]
    assert len(last) == 1 and last[0]["col"] == 5 and last[0]["kind"] == (im.UNREAD if min_qv else im.INFRAME)


def test_contention_one_allele_in_every_read(ctx):
    """257 reads with the same insertion: four full waves and one lane append, one atomic each."""
    s = "ACGTACGTAC"
    rec = im.records(with_anchors([(0, [("=", 5), ("I", 6), ("=", 5)], s[:5] + "GATTAC" + s[5:])] * 257), with_qual=True)
    got = check_events(ctx, rec, 10, wb=0)
    assert len(got) == 261 and (got["read"] == np.arange(261)).all() and (got["col"] == 5).all()


def test_every_read_its_own_allele(ctx):
    s = "ACGTACGTAC"
    word = lambda i: "".join("ACGT"[(i >> (2 * (5 - j))) & 3] for j in range(6))     # noqa: E731
    reads = [(0, [("=", 5), ("I", 6), ("=", 3), ("I", 3), ("=", 2)], s[:5] + word(i) + s[5:8] + word(i)[:3] + s[8:]) for i in range(1025)]
    rec = im.records(with_anchors(reads), with_qual=True)
    got = check_events(ctx, rec, 10, wb=0)
    assert len(got) == 2 * 1025 + 4 and len(set(got["seq"][got["col"] == 5].tolist())) >= 1025


def test_switch_off_take_and_room():
    lib = capi.load_library()
    rec = im.records(make_reads(300, 40, 9), with_qual=True)
    a = (rec["pos"], rec["cigar"], rec["cig_off"], rec["seq4"], rec["seq_off"], rec["qual"], rec["qual_off"])
    j = capi.Juliet(0)
    j.track_insertion_alleles()                              # the alleles alone leave no events
    j.ingest_records(40, WB, *a, min_qv=20)
    j.insertion_alleles()
    with pytest.raises(capi.JulietError) as e:
        j.insertion_reads()
    assert e.value.status == -4 and "jl_msa_track_insertion_reads" in str(e.value)
    j.track_insertion_alleles(False)
    j.track_insertion_reads()
    check_events(j, rec, 40)
    n = np.zeros(1, dtype=np.uint32)
    assert lib.jl_insertion_reads_fetch(j.h, None, 0, n.ctypes.data) == 0 and n[0] >= 3            # rows == NULL: only the count
    small = np.zeros(1, dtype=capi.INSERTION_EVENT)
    assert lib.jl_insertion_reads_fetch(j.h, small.ctypes.data, 1, None) == -1 and "room for 1 rows" in lib.jl_last_error(j.h).decode()
    other = capi.Juliet(0)
    other.upload_rows(records_expand.expand_reference(rec, 40, WB, 20))
    j.take([(other, np.arange(100, dtype=np.uint32))])       # another producer replaces the matrix
    with pytest.raises(capi.JulietError) as e:
        j.insertion_reads()
    assert e.value.status == -4
    j.track_insertion_reads(False)                           # off again: the next build leaves nothing to fetch
    j.ingest_records(40, WB, *a, min_qv=20)
    with pytest.raises(capi.JulietError):
        j.insertion_reads()
    with pytest.raises(capi.JulietError):
        j.insertion_alleles()
    other.close()
    j.close()


# ---------------------------------------------------------------------------------------------- the site matrix
def ingest(src, rec, n_cols=L):
    src.ingest_records(n_cols, 0, rec["pos"], rec["cigar"], rec["cig_off"], rec["seq4"], rec["seq_off"], rec["qual"], rec["qual_off"], min_qv=0)


def variants_for(rows, sites):
    """Variant rows for the codon sites (what the front end would bring from a variant table): per site up to two observed codons
    other than the commonest, ref_codon the commonest."""
    var = []
    for col, kind, _ in sites:
        if kind != sm.CODON:
            continue
        codon, _ = sm.classes(rows, col)
        hist = np.bincount(16 * rows[codon, col].astype(np.int64) + 4 * rows[codon, col + 1] + rows[codon, col + 2], minlength=64)
        ref = int(hist.argmax())
        seen = [int(c) for c in np.argsort(-hist, kind="stable") if hist[c] and c != ref][:2] or [(ref + 1) % 64]
        var += [(col, ref, c) for c in sorted(seen)]
    return sm.variant_rows(var).astype(capi.VARIANT)


def check_matrix(pc, n, exp):
    assert (pc.n_reads, pc.n_cols) == exp.shape
    packed = pc.download_columns()
    got = msa.unpack_columns(packed, n)
    assert not (got == 7).any()
    assert (got == exp).all(), np.argwhere(got != exp)[:8]
    beyond = msa.unpack_columns(packed, 2 * packed.shape[1])[n:]        # what the download shows of the padding
    assert (beyond == OUT).all()
    cnt = pc.codon_deletions()                                          # set pad bits anywhere in a row would show in span
    assert (cnt == dm.counts(exp)).all()


# reads: the word (32), the 16-byte piece a lane owns (128), the plane row's 128-byte line (1024)
@pytest.mark.parametrize("n", [31, 32, 33, 127, 128, 129, 1023, 1024, 1025])
def test_site_matrix_and_its_phasing(ctxs, oracle, n):
    src, pc = ctxs
    rec, rows, evs, sites, alleles = site_case(n, 50 + n)
    exp = ism.site_matrix(rows, evs, sites, alleles)
    assert holds_all_classes(exp, sites, alleles)                       # all six classes of the table, from the mirror
    ingest(src, rec)
    pc.sites_assemble_alleles(src, sites, alleles)
    check_matrix(pc, n, exp)
    table = ism.build_table(variants_for(rows, sites), sites, alleles)
    pc.phase_async(table, MIN_READS)
    same_phase(pc.phase_fetch(cap_var=max(64, len(table))), oracle.phase(exp, table, MIN_READS), len(table), n)
    # the source is what it was
    assert (msa.unpack_columns(src.download_columns(), n) == rows).all() and (src.insertion_reads() == ism.event_rows(evs)).all()


def test_insertion_sites_alone_and_one_allele(ctxs, oracle):
    """No codon or deletion site at all (the first kernel has nothing to do); then the single-allele site alone."""
    src, pc = ctxs
    n = 129
    rec, rows, evs, sites, alleles = site_case(n, 77)
    ingest(src, rec)
    for js in ((J_FIRST, J_MIXED, J_MANY, J_LAST), (J_FIRST,)):
        only, al = [(j, ism.INSERTION, NF) for j in js], listed_alleles(js)
        pc.sites_assemble_alleles(src, only, al)
        check_matrix(pc, n, ism.site_matrix(rows, evs, only, al))
    # repeated, growing and shrinking, into the same context
    for m in (2000, 40):
        rec, rows, evs, sites, alleles = site_case(m, m)
        ingest(src, rec)
        pc.sites_assemble_alleles(src, sites, alleles)
        check_matrix(pc, m, ism.site_matrix(rows, evs, sites, alleles))


def test_no_insertion_site_is_sites_assemble(ctxs):
    """Byte for byte — also from an adopted source with its own stride and garbage past the reads (such a source holds no events,
    so the insertion sites themselves are checked past the reads on record builds only: check_matrix's `beyond`)."""
    import torch
    src, pc = ctxs
    n = 129
    rec, rows, evs, sites, alleles = site_case(n, 5)
    plain = [s for s in sites if s[1] != ism.INSERTION]
    ingest(src, rec)
    pc.sites_assemble(src, plain)
    one = pc.download_columns().copy()
    pc.sites_assemble_alleles(src, plain, [])
    assert (pc.download_columns() == one).all() and (msa.unpack_columns(one, n) == sm.recode(rows, plain)).all()
    planes = garbage_planes(rows, 144, 3)
    t = torch.from_numpy(planes).cuda()
    torch.cuda.synchronize()
    adopted = capi.Juliet(0)
    adopted.adopt(t.data_ptr(), n, L, 144, keep_alive=t)
    pc.sites_assemble_alleles(adopted, plain, [])
    check_matrix(pc, n, sm.recode(rows, plain))
    with pytest.raises(capi.JulietError) as e:                         # ... and an adopted matrix has no events
        pc.sites_assemble_alleles(adopted, sites, alleles)
    assert e.value.status == -4
    adopted.close()


def test_refusals_leave_the_destination_as_it_was(ctxs):
    lib = capi.load_library()
    src, pc = ctxs
    n = 200
    rec, rows, evs, sites, alleles = site_case(n, 9)
    ingest(src, rec)
    pc.sites_assemble_alleles(src, sites, alleles)
    exp = ism.site_matrix(rows, evs, sites, alleles)

    def refused(s, al, status, word, src_h=None, n_al=None):
        a = np.zeros(max(1, len(s)), dtype=capi.SITE)
        for k, x in enumerate(s):
            a[k] = (*x, 0)
        b = np.zeros(max(1, len(al)), dtype=capi.INSERTION_ALLELE)
        for k, x in enumerate(al):
            b[k] = (x[0], x[1], x[2], 0, 0)
        rc = lib.jl_sites_assemble_alleles(pc.h, src.h if src_h is None else src_h, a.ctypes.data, len(s), b.ctypes.data, len(al) if n_al is None else n_al)
        assert rc == status and word in lib.jl_last_error(pc.h).decode(), (rc, lib.jl_last_error(pc.h).decode())

    site, al = [(J_MIXED, ism.INSERTION, NF)], listed_alleles([J_MIXED])
    refused([(0, ism.INSERTION, NF)], [key(0, "AAA")], -1, "junction 0")
    refused([(L, ism.INSERTION, NF)], [key(L, "AAA")], -1, "junction %d" % L)
    refused([(J_MIXED, ism.INSERTION, 5)], al, -1, "insertion site with a fill")
    refused([(J_MIXED, 3, NF)], al, -1, "kind 3")
    refused([(J_MIXED, ism.INSERTION, NF), (J_MIXED, sm.CODON, NF)], al, -1, "ascending")
    refused(site + site, al, -1, "the same")
    refused([(L - 2, sm.CODON, NF)], [], -1, "beyond")                 # §18's rules hold for kinds 0 and 1
    refused([(3, sm.DELETION, 3)], [], -1, "deletion site with a fill")
    refused(site, [], -1, "has no allele")
    refused(site, [key(J_MIXED, word) for word in sorted(POOL_63)], -1, "63 alleles")
    refused(site, al + [key(J_MANY, "AAA")], -1, "no insertion site")
    refused([(3, sm.CODON, NF)], [key(3, "AAA")], -1, "no insertion site")
    refused(site, [al[1], al[0]], -1, "strictly ascending")
    refused(site, [al[0], al[0]], -1, "strictly ascending")
    refused(site, [(J_MIXED, 4, 0)], -1, "length 4")
    refused(site, [(J_MIXED, 0, 0)], -1, "length 0")
    refused(site, [(J_MIXED, 33, 0)], -1, "length 33")
    refused(site, [(J_MIXED, 3, 1 << 6)], -1, "above its 3 bases")
    refused(site, al, -1, "4097 alleles", n_al=sm.SITES_MAX + 1)
    assert lib.jl_sites_assemble_alleles(pc.h, src.h, np.zeros(1, dtype=capi.SITE).ctypes.data, 1, None, 1) == -1
    assert "NULL" in lib.jl_last_error(pc.h).decode()
    plain = capi.Juliet(0)                                             # a source whose build did not track reads
    plain.track_insertion_alleles()
    ingest(plain, rec)
    refused(site, al, -4, "jl_msa_track_insertion_reads", src_h=plain.h)
    plain.close()
    empty = capi.Juliet(0)
    refused(site, al, -4, "no resident matrix", src_h=empty.h)
    empty.close()
    check_matrix(pc, n, exp)                                            # what the destination held is still there


POOL_63 = ["".join("ACGT"[(i >> (2 * (2 - j))) & 3] for j in range(3)) for i in range(63)]


# ---------------------------------------------------------------------------------------------- the command line
FLAGS = ("--mode-phasing", "--call-insertions", "--phase-insertions")
CODONS = sm.CODONS


def juliet(d, *args):
    return subprocess.run([JULIET, *args], cwd=d, capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    d = tmp_path_factory.mktemp("insertion_sites_cli")
    subprocess.check_call([SYNTH, "--reads", str(N_CLI), "--cols", str(L_CLI), "--seed", "23", "--insert", f"{PLANT_COL}:{PLANT_LEN}:{PLANT_PERMILLE}",
                           "--insert", f"{SPLIT_COL}:{PLANT_LEN}:{PLANT_PERMILLE}", "-o", "in.bam", "--config-out", "in.json"], cwd=d)
    r = juliet(d, "-c", "in.json", *FLAGS, "--timing", "in.bam", "p.json", "p.html")
    assert r.returncode == 0, r.stderr
    assert re.search(r"timing sites\s", r.stderr)
    for out, flags in (("i", FLAGS[:2]), ("both", FLAGS + ("--call-deletions", "--phase-deletions"))):
        p = juliet(d, "-c", "in.json", *flags, "in.bam", f"{out}.json", f"{out}.html")
        assert p.returncode == 0, p.stderr
    return d, read_bam(d / "in.bam")


def test_cli_json_equals_the_mirrors_and_the_oracle(cli, oracle):
    d, rec = cli
    cfg = json.load(open(d / "in.json"))
    ref = np.array(["ACGT".index(b) for b in cfg["referenceSequence"].upper()], dtype=np.uint8)
    rows = records_expand.expand_reference(rec, L_CLI, 0, 0)
    table = oracle.call(rows, np.array([(1, L_CLI + 1)], dtype=oracle_lib.GENE), refseq=ref)
    walked = im.walk(rec, L_CLI)
    called = expected_entries(walked, L_CLI // 3, 1.0e-3)
    assert [e[0] for e in called] == [PLANT_COL // 3]
    alleles_called = [key(3 * after, "".join(codons)) for after, codons, _ in called]
    sites, alleles = ism.build_sites(table, [], alleles_called, phase_deletions=False)
    assert (PLANT_COL, ism.INSERTION, NF) in sites and len(alleles) == 1
    rows_t = ism.build_table(table, sites, alleles)
    ph = oracle.phase(ism.site_matrix(rows, ism.events(rec, L_CLI), sites, alleles), rows_t)
    rep = ism.report(ph, sites, alleles)
    codon_k = [k for k, x in enumerate(sites) if x[1] == sm.CODON]
    assert [int(c) for c in ph["pos_cols"]] == [3 * k for k in range(len(sites))]
    j = json.load(open(d / "p.json"))
    hb, s = j["haplotype"], ph["summary"]
    assert list(hb) == ["reported_reads", "insufficient_coverage_reads", "damaged_reads", "marginal_gaps", "marginal_heteroduplexes",
                        "marginal_partial", "haplotypes", "variant_positions_abs", "insertion_alleles"]
    assert [hb[k] for k in list(hb)[:6]] == [s["reported_reads"], s["insufficient_reads"], s["damaged_reads"], s["marginal_gap"],
                                             s["marginal_heteroduplex"], s["marginal_partial"]]
    assert s["reported_reads"] + s["insufficient_reads"] + s["damaged_reads"] == N_CLI
    assert hb["variant_positions_abs"] == [sites[k][0] + 1 for k in codon_k]
    assert hb["insertion_alleles"] == [dict(gene=cfg["genes"][0]["name"], after_position=after, inserted_codons=codons) for after, codons, _ in called]
    assert len(hb["haplotypes"]) == s["n_haplotypes"] >= 2
    for h, got in enumerate(hb["haplotypes"]):
        assert list(got) == ["name", "reads", "frequency", "insertions", "codons", "read_names"]
        assert got["reads"] == ph["hap_count"][h] and got["insertions"] == rep["insertions"][h]
        assert got["codons"] == [CODONS[ph["hap_pattern"][h][k]] for k in codon_k]
        assert sorted(int(n.split("/")[1]) for n in got["read_names"]) == np.nonzero(ph["read_hap"] == h)[0].tolist()
    assert any(any(g["insertions"]) for g in hb["haplotypes"])          # the plant's carriers are a haplotype of their own
    entries = j["genes"][0]["insertion_positions"]
    assert len(entries) == len(called)
    for e, a in zip(entries, alleles):
        assert list(e)[-1] == "haplotype_hit" and e["haplotype_hit"] == rep["hit"][a]
    by_codon = {(vp["ref_position"], vc["codon"]): vc["haplotype_hit"] for vp in j["genes"][0]["variant_positions"] for aa in vp["variant_amino_acids"]
                for vc in aa["variant_codons"]}
    is_codon_row = np.array([sites[int(c) // 3][1] == sm.CODON for c in rows_t["col"]])
    assert len(by_codon) == len(table) == int(is_codon_row.sum())
    for v, exp_hit in zip(table, np.asarray(ph["hit"])[is_codon_row].astype(bool).tolist()):
        assert by_codon[(int(v["codon_pos"]), CODONS[v["codon"]])] == exp_hit


def test_cli_html_holds_every_new_leaf(cli):
    d, _ = cli
    j = json.load(open(d / "p.json"))
    hb = j["haplotype"]
    html = open(d / "p.html").read()
    spans = re.findall(r'<span data-gene="(.*?)" data-after="(\d+)">(.*?)</span>', re.search(r'<p id="hap-insertion-alleles">(.*?)</p>', html).group(1))
    assert [(g, int(a), c.split(" ")) for g, a, c in spans] == [(a["gene"], a["after_position"], a["inserted_codons"]) for a in hb["insertion_alleles"]]
    table = re.search(r'<table id="hap-table">.*?</table>', html, flags=re.S).group(0)
    assert "<th>Insertions</th>" in table and "<th>Deletions</th>" not in table
    cells = re.findall(r'<td class="hap-insertions">(.*?)</td>', table)
    assert [[x == "x" for x in c.split(" ")] for c in cells] == [h["insertions"] for h in hb["haplotypes"]]
    block = re.search(r'<details open id="insertions">.*?</details>', html, flags=re.S).group(0)
    assert re.findall(r'<th class="hapname">(.*?)</th>', block) == [h["name"] for h in hb["haplotypes"]]
    trs = re.findall(r'<tr class="insertion">.*?</tr>', block)
    entries = j["genes"][0]["insertion_positions"]
    assert len(trs) == len(entries) >= 1
    for tr, e in zip(trs, entries):
        assert [c == "hit" for c in re.findall(r'<td class="(hit|nohit)">', tr)] == e["haplotype_hit"]


def test_cli_without_the_flag_nothing_changes(cli):
    d, _ = cli
    p = juliet(d, "-c", "in.json", *FLAGS[:2], "in.bam", "i2.json", "i2.html")
    assert p.returncode == 0, p.stderr
    strip = lambda t: re.sub(r'"(timestamp|command_line)": "[^"]*"', "", t)     # noqa: E731
    one, two = open(d / "i.json").read(), open(d / "i2.json").read()
    assert strip(one) == strip(two) and "insertion_alleles" not in one and '"insertions"' not in one
    h1, h2 = (re.sub(r"<tr><th>(timestamp|command_line)</th>.*?</tr>\n", "", open(d / f"{x}.html").read()) for x in ("i", "i2"))
    assert h1 == h2 and "hap-insertion" not in h1
    # ... and everything but the phasing leaves is the --call-insertions run's
    a, b = json.load(open(d / "p.json")), json.load(open(d / "i.json"))
    for doc in (a, b):
        doc["input"].pop("timestamp"), doc["input"].pop("command_line"), doc.pop("haplotype")
        for g in doc["genes"]:
            for e in g["insertion_positions"]:
                e.pop("haplotype_hit", None)
            for vp in g["variant_positions"]:
                for aa in vp["variant_amino_acids"]:
                    for vc in aa["variant_codons"]:
                        vc.pop("haplotype_hit")
    assert a == b


def test_cli_with_phased_deletions_both_kinds_of_site_appear(cli):
    d, _ = cli
    hb = json.load(open(d / "both.json"))["haplotype"]
    assert "deletion_positions_abs" in hb and "insertion_alleles" in hb and len(hb["insertion_alleles"]) == 1
    for h in hb["haplotypes"]:
        assert list(h) == ["name", "reads", "frequency", "deletions", "insertions", "codons", "read_names"]
        assert len(h["insertions"]) == 1 and len(h["deletions"]) == len(hb["deletion_positions_abs"])
    one = json.load(open(d / "p.json"))["haplotype"]
    if not hb["deletion_positions_abs"]:                                # no deletion called: the insertion sites alone
        assert [h["reads"] for h in hb["haplotypes"]] == [h["reads"] for h in one["haplotypes"]]
    html = open(d / "both.html").read()
    assert "<th>Insertions</th>" in html and "<th>Deletions</th>" in html


@pytest.mark.parametrize("args", [["--call-insertions"], ["--mode-phasing"], ["--mode-phasing", "--call-insertions", "--rescue-damaged"],
                                  ["--mode-phasing", "--call-insertions", "--windows", "2"], ["--mode-phasing", "--call-insertions", "--devices", "0,0"],
                                  ["--mode-phasing", "--call-insertions", "--downsample", "100"]])
def test_cli_refused_combinations_open_nothing(tmp_path, args):
    r = juliet(tmp_path, "--phase-insertions", *args, "no_such.bam", "o.json")
    assert r.returncode == 1 and "-insertions" in r.stderr, (r.returncode, r.stderr)
    assert not list(tmp_path.iterdir())


def test_cli_refused_with_batch_and_as_fuse(tmp_path):
    (tmp_path / "l.tsv").write_text("no_such.bam\ta.json\n")
    r = juliet(tmp_path, "--phase-insertions", "--mode-phasing", "--call-insertions", "--batch", "l.tsv")
    assert r.returncode == 1 and "--batch" in r.stderr
    r = subprocess.run([os.path.join(ROOT, "minorseq_amd", "bin", "fuse"), "--phase-insertions", "no_such.bam", "o.fasta"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "fuse" in r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == ["l.tsv"]
