"""The record ingest on the device fed by a BAM that the project's own writer never touched: the variety sample of tests/bam_diff.py
(every cigar op but M, zero-length ops, the undefined op codes 9..15, an empty read, every aux type, tracks of every length, qualities
on both sides of the threshold, kept and dropped flags, three references) is written by tests/bam_py.py, decoded by the front end's
pipelined reader through tests/cpp/records_dump.cpp — which refuses to write anything unless every record satisfies what the device
takes on trust — and handed to jl_records_append / jl_records_window.  Every cell of the resident matrix is compared with
tests/records_expand.py, without a filter, with quality bytes and with the bit mask.

Then `juliet -c cfg --mode-phasing` end to end on a bam_py-written sample of two planted haplotypes — soft clips, N skips,
supplementary records, records of a second reference and dropped records in between: the variant table and the haplotype block of the
JSON against the oracle on records_expand's rows.  No byte of either input passed through the project's BamWriter."""
import json
import os
import subprocess

import numpy as np
import pytest

import bam_diff
import bam_py
import records_expand
from minorseq_amd import capi, msa

ROOT = bam_diff.ROOT
JULIET = os.path.join(ROOT, "minorseq_amd", "bin", "juliet")

pytestmark = pytest.mark.gpu

N_COLS, WIN_BEGIN = 597, 2          # the kept reads lie on a reference of 600 columns; the window cuts both ends
MIN_QV = bam_diff.VARIETY_MIN_QV
FIVE = ("pos", "cigar", "cig_off", "seq4", "seq_off")


@pytest.fixture(scope="module")
def dump_exe(tmp_path_factory):
    return bam_diff.build_records_dump(tmp_path_factory.mktemp("records_dump"))


@pytest.fixture(scope="module")
def decoded(tmp_path_factory, dump_exe):
    d = tmp_path_factory.mktemp("bam_independent")
    exe = dump_exe
    records = bam_diff.variety_records()
    assert len(records) <= 300
    bam = str(d / "variety.bam")
    bam_py.write_bam(bam, "@HD\tVN:1.5\n", bam_diff.VARIETY_REFS, records, block=4000)
    out = {}
    for form in ("none", "bytes", "mask"):
        status, msg, got = bam_diff.run_dump(exe, bam, str(d / (form + ".bin")), reader="pipe", threads=4, min_qv=MIN_QV, form=form)
        assert status == 0, msg                                             # 4 would be a record the device must never see
        bam_diff.assert_same(got, bam_diff.expected(records, min_qv=MIN_QV, form=form), form)
        out[form] = got
    return out


@pytest.fixture(scope="module")
def ctxs():
    pair = [capi.Juliet(0), capi.Juliet(0)]
    yield pair
    for j in pair:
        j.close()


def rows_of(j):
    return msa.unpack_columns(j.download_columns(), j.n_reads)


@pytest.mark.parametrize("form", ["none", "bytes", "mask"])
def test_ingest_of_independently_written_records(decoded, ctxs, form):
    rec = decoded[form]
    n = len(rec["pos"])
    assert 150 < n <= 300 and ((rec["cigar"] & 15) >= 9).any() and (np.diff(rec["seq_off"]) == 0).any()
    min_qv = 0 if form == "none" else MIN_QV
    quals = decoded["bytes"]
    want = records_expand.expand(dict(quals), N_COLS, WIN_BEGIN, min_qv)
    assert want.shape == (n, N_COLS) and len(np.unique(want)) == 7
    if min_qv:
        assert (want != records_expand.expand(dict(quals), N_COLS, WIN_BEGIN, 0)).any()      # the filter decides some cells
    five = [rec[k] for k in FIVE]
    holder, win = ctxs
    if form == "bytes":
        holder.records_upload(*five, qual=rec["qual"], qual_off=rec["qual_off"])
    elif form == "mask":
        holder.records_upload(*five, qmask=bam_diff.qmask_bits(rec["qmask2"]))
    else:
        holder.records_upload(*five)
    try:
        win.records_window(holder, N_COLS, WIN_BEGIN, min_qv)
        got = rows_of(win)
        assert got.shape == want.shape and (got == want).all(), np.argwhere(got != want)[:8]
        win.records_window(holder, 40, 311, min_qv)                                           # a second, narrow window of the same records
        got = rows_of(win)
        assert (got == want[:, 311 - WIN_BEGIN:351 - WIN_BEGIN]).all(), np.argwhere(got != want[:, 309:349])[:8]
    finally:
        holder.records_drop()


# ---------------------------------------------------------------------------------------------- the command line
CLI_L, CLI_READS, CLI_SEED = 240, 1500, 29
PLANTED = {30: "GAT", 99: "TTC", 171: "CCA"}          # column of a codon's first base -> the minor haplotype's codon (30 % of the reads)


def cli_sample():
    """(reference string, records).  Reads of the first reference: the reference sequence or the minor haplotype, from a random
    start to a random end, a soft clip of 0..6 bases at either end, every seventh with an N skip of 9..40 columns somewhere inside,
    every fifth supplementary (0x800), a substitution here and there (an X op); in between, records of a second reference (with edits
    of their own, which must not count), unmapped and secondary records, and records without a position."""
    rng = np.random.default_rng(CLI_SEED)
    ref = "".join("ACGT"[int(v)] for v in rng.integers(0, 4, CLI_L))
    for col, codon in PLANTED.items():                                # the reference differs from the planted codon in every base
        ref = ref[:col] + "".join("ACGT"[("ACGT".index(c) + 1) % 4] for c in codon) + ref[col + 3:]
    minor = ref
    for col, codon in PLANTED.items():
        minor = minor[:col] + codon + minor[col + 3:]
    other = "".join("ACGT"[int(v)] for v in rng.integers(0, 4, 400))

    def aligned(target, template, b, e, skip):
        """Cigar ops and bases of template[b:e] against target, runs of = and X, `skip` = (from, to) left out as an N op."""
        ops, seq, c = [], [], b
        while c < e:
            if skip and c == skip[0]:
                ops.append(("N", skip[1] - skip[0]))
                c = skip[1]
                continue
            base = template[c]
            if rng.random() < 0.002:
                base = "ACGT"[("ACGT".index(base) + 1 + int(rng.integers(3))) % 4]
            op = "=" if base == target[c] else "X"
            if ops and ops[-1][0] == op:
                ops[-1] = (op, ops[-1][1] + 1)
            else:
                ops.append((op, 1))
            seq.append(base)
            c += 1
        return ops, "".join(seq)

    def read(i, ref_id=0, flag=0):
        target = ref if ref_id == 0 else other
        template = (minor if rng.random() < 0.3 else ref) if ref_id == 0 else other
        b = int(rng.integers(0, 25)) if rng.random() < 0.5 else 0
        e = len(target) - (int(rng.integers(0, 25)) if rng.random() < 0.5 else 0)
        skip = None
        if i % 7 == 3:
            s0 = int(rng.integers(b + 5, e - 50))
            skip = (s0, s0 + int(rng.integers(9, 41)))
        ops, seq = aligned(target, template, b, e, skip)
        left, right = int(rng.integers(0, 7)), int(rng.integers(0, 7))
        clip = lambda n: "".join("ACGT"[int(v)] for v in rng.integers(0, 4, n))
        ops = ([("S", left)] if left else []) + ops + ([("S", right)] if right else [])
        seq = clip(left) + seq + clip(right)
        return dict(ref_id=ref_id, pos=b, flag=flag, mapq=60, name="m/%d/ccs" % i, cigar=ops, seq=seq, qual=bytes([60]) * len(seq),
                    tags=[("rq", "f", 0.999), ("np", "i", 12)])

    records = []
    for i in range(CLI_READS):
        k = i % 20
        if k == 6 or k == 13:
            records.append(read(i, ref_id=1))
        elif k == 9:
            records.append(read(i, flag=0x4 if i % 40 < 20 else 0x100))
        elif k == 16 and i % 60 == 16:
            records.append(dict(read(i), pos=-1))
        else:
            records.append(read(i, flag=0x800 if i % 5 == 2 else 0))
    return ref, other, records


def flat_variants(j):
    rows = []
    for gi, g in enumerate(j["genes"]):
        for vp in g["variant_positions"]:
            for aa in vp["variant_amino_acids"]:
                for vc in aa["variant_codons"]:
                    rows.append((gi, vp["ref_position"], msa.codon_index(vc["codon"]), vc, vp))
    return sorted(rows, key=lambda r: r[:3])


def test_cli_phasing_of_an_independently_written_sample(tmp_path, oracle, dump_exe):
    ref, other, records = cli_sample()
    d = tmp_path
    bam, cfg, out = str(d / "two.bam"), str(d / "two.json"), str(d / "o.json")
    text = "@HD\tVN:1.5\tSO:unknown\tpb:3.0.1\n@SQ\tSN:main\tLN:%d\n@SQ\tSN:other\tLN:400\n@RG\tID:x\tPL:PACBIO\tPM:SEQUEL\tDS:READTYPE=CCS\n" % CLI_L
    bam_py.write_bam(bam, text, [("main", CLI_L), ("other", len(other))], records, block=20000)
    json.dump({"genes": [{"name": "g", "begin": 1, "end": CLI_L + 1}], "referenceName": "main", "referenceSequence": ref}, open(cfg, "w"))
    # the host's hand-over first: nothing goes to the device that records_dump would refuse
    status, msg, got = bam_diff.run_dump(dump_exe, bam, str(d / "dump.bin"), reader="pipe", threads=4)
    assert status == 0, msg
    exp_rec = bam_diff.expected(records)
    bam_diff.assert_same(got, exp_rec)
    keep, ref_id = bam_diff.kept(records)
    assert ref_id == 0 and 1000 < len(keep) < CLI_READS and any(r["flag"] & 0x800 for r in keep)
    rows = records_expand.expand(exp_rec, CLI_L, 0, 0)
    refcodes = np.array(["ACGT".index(c) for c in ref], dtype=np.uint8)

    r = subprocess.run([JULIET, "-c", cfg, "--mode-phasing", bam, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    j = json.load(open(out))
    exp = oracle.call(rows, np.array([(1, CLI_L + 1)], dtype=capi.GENE), refseq=refcodes)
    found = flat_variants(j)
    assert len(found) == len(exp) >= len(PLANTED)
    planted = {(col // 3 + 1, msa.codon_index(c)) for col, c in PLANTED.items()}
    assert planted <= {(int(e["codon_pos"]), int(e["codon"])) for e in exp}
    col = oracle.pileup(rows)
    for (gi, pos, cod, vc, vp), e in zip(found, exp):
        assert (gi, pos, cod) == (e["gene"], e["codon_pos"], e["codon"])
        assert vc["count"] == e["count"] and vp["coverage"] == e["coverage"] and vc["expected"] == e["expected"]
        assert vc["frequency"] == e["count"] / e["coverage"]
        assert abs(vc["pValue"] - e["p_value"]) <= 1e-10
        assert vp["ref_codon"] == msa.codon_string(e["ref_codon"])
        for m in vp["msa"]:
            c = m["abs_pos"] - 1
            assert [m[s] for s in "ACGT-N"] == col[c].tolist() and m["wt"] == ref[c]
    ph = oracle.phase(rows, exp)
    hb, s = j["haplotype"], ph["summary"]
    assert s["n_haplotypes"] >= 2
    assert (hb["reported_reads"], hb["insufficient_coverage_reads"], hb["damaged_reads"]) == \
        (s["reported_reads"], s["insufficient_reads"], s["damaged_reads"])
    assert hb["reported_reads"] + hb["insufficient_coverage_reads"] + hb["damaged_reads"] == len(keep)
    assert hb["insufficient_coverage_reads"] > 0                                    # the N skips and short reads leave sites uncovered
    assert (hb["marginal_gaps"], hb["marginal_heteroduplexes"], hb["marginal_partial"]) == \
        (s["marginal_gap"], s["marginal_heteroduplex"], s["marginal_partial"])
    assert [h["reads"] for h in hb["haplotypes"]] == ph["hap_count"].tolist()
    names = [r["name"] for r in keep]
    for hi, h in enumerate(hb["haplotypes"]):
        assert [msa.codon_index(c) for c in h["codons"]] == ph["hap_pattern"][hi].tolist()
        assert sorted(h["read_names"]) == sorted(names[k] for k in np.nonzero(ph["read_hap"] == hi)[0])
    for k, (gi, pos, cod, vc, vp) in enumerate(found):
        assert vc["haplotype_hit"] == [bool(x) for x in ph["hit"][k]]
    assert j["target_config"]["n_reads"] == len(keep)
