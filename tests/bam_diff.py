"""Shared by the independent-writer tests (test_bam_differential_host.py, test_gpu_bam_independent.py): builds tests/cpp/records_dump,
reads what it writes, states in Python what the front end must hand over for a list of bam_py records, and makes the 'variety' sample.
Test infrastructure; nothing of the product imports it.

The rules restated here are the ones written in minorseq_amd/host/bam.hpp, msa_builder.hpp and docs/SPEC.md (input):
  dropped: flag 0x4 or 0x100, ref_id < 0, pos < 0; with --min-rq, a read whose `rq` tag (type f, not negative) is below it;
  the reference read: the one asked for, else the one of the first kept record; records of other references are dropped;
  effective quality of a base: the lowest of QUAL (0xFF = nothing known) and the characters - 33 (as an unsigned byte) of the Z tags
  dq, iq and sq, each over the bases it has; the mask form flags a base whose effective quality is below min(min_qv, 127)."""
import os
import struct
import subprocess

import numpy as np

import bam_py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "minorseq_amd", "host")
INCLUDES = ["-I" + HOST, "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "minorseq_amd", "csrc"),
            "-I" + os.path.join(ROOT, "tests", "cpp")]
_DTYPES = dict(pos=np.int32, cigar=np.uint32, cig_off=np.uint64, seq_off=np.uint64, qual_off=np.uint64, seq4=np.uint8, qual=np.uint8,
               qmask2=np.uint8, chunks=np.uint64, extent=np.int64)


def build_records_dump(out_dir):
    """g++ only: the program links neither the device library nor the HIP runtime."""
    exe = os.path.join(str(out_dir), "records_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", *INCLUDES, "-o", exe, os.path.join(ROOT, "tests", "cpp", "records_dump.cpp"),
                           "-lz", "-lpthread"])
    return exe


def run_dump(exe, bam, out, reader="seq", threads=1, chunk_reads=8192, min_qv=0, min_rq=0.0, form="none", ref=-1):
    """(exit status, last line of stderr, sections or None)."""
    env = {k: v for k, v in os.environ.items() if k not in ("JL_BGZF_THREADS", "JL_DECODE_THREADS")}
    r = subprocess.run([exe, bam, out, "--reader", reader, "--threads", str(threads), "--chunk-reads", str(chunk_reads), "--min-qv", str(min_qv),
                        "--min-rq", repr(min_rq), "--form", form, "--ref", str(ref)], capture_output=True, text=True, env=env, timeout=120)
    msg = r.stderr.strip().splitlines()[-1] if r.stderr.strip() else ""
    return r.returncode, msg, (read_dump(out) if r.returncode == 0 else None)


def read_dump(path):
    raw = open(path, "rb").read()
    out, at = {}, 0
    while at < len(raw):
        name = raw[at:at + 8].rstrip(b"\0").decode()
        n, = struct.unpack_from("<Q", raw, at + 8)
        body = raw[at + 16:at + 16 + n]
        out[name] = np.frombuffer(body, dtype=_DTYPES[name]) if name in _DTYPES else body
        at += 16 + n
    out["names"] = [x.decode("latin-1") for x in out["names"].split(b"\0")[:-1]]
    refs, b, o = [], out["refs"], 0
    while o < len(b):
        e = b.index(b"\0", o + 4)
        refs.append((b[o + 4:e].decode("latin-1"), struct.unpack_from("<I", b, o)[0]))
        o = e + 1
    out["refs"] = refs
    out["text"] = out["text"].decode("latin-1")
    return out


def _tag(r, name, ty):
    v = None
    for t, y, value in r.get("tags", ()):
        if t == name and y == ty:
            v = value                       # the last one counts
    return v


def kept(records, ref=-1, min_rq=0.0):
    """(the records the front end keeps, the reference it reads)."""
    out = []
    for r in records:
        if r.get("flag", 0) & 0x104 or r.get("ref_id", -1) < 0 or r.get("pos", -1) < 0:
            continue
        rq = _tag(r, "rq", "f")
        if min_rq > 0 and rq is not None:
            rq = struct.unpack("<f", struct.pack("<f", rq))[0]
            if 0 <= rq < min_rq:
                continue
        if ref < 0:
            ref = r["ref_id"]
        if r["ref_id"] == ref:
            out.append(r)
    return out, ref


def effective_quals(r):
    seq = "" if r["seq"] == "*" else r["seq"]
    q = np.frombuffer(b"\xff" * len(seq) if r.get("qual") is None else bytes(r["qual"]), dtype=np.uint8).copy()
    for name in ("dq", "iq", "sq"):
        t = _tag(r, name, "Z")
        if t is not None:
            v = (np.frombuffer(t.encode("latin-1"), dtype=np.uint8)[:len(q)].astype(np.int16) - 33).astype(np.uint8)
            q[:len(v)] = np.minimum(q[:len(v)], v)
    return q


def expected(records, ref=-1, min_qv=0, min_rq=0.0, form="none"):
    """What records_dump must write for `records`, computed from the record list alone."""
    keep, ref = kept(records, ref, min_rq)
    out = bam_py.record_arrays(keep, want_qual=False)
    out["names"] = [r.get("name", "") for r in keep]
    eq = [effective_quals(r) for r in keep]
    if form == "bytes":
        out["qual"] = np.concatenate(eq + [np.zeros(0, dtype=np.uint8)])
        out["qual_off"] = np.cumsum([0] + [len(q) for q in eq]).astype(np.uint64)
    else:
        out["qual"], out["qual_off"] = np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64)
    if form == "mask":
        m = []
        for q in eq:
            low = (q < min(min_qv, 127)).astype(np.uint8)
            low = np.concatenate([low, np.zeros(len(low) & 1, dtype=np.uint8)])
            m.append(low[0::2] | (low[1::2] << 1))
        out["qmask2"] = np.concatenate(m + [np.zeros(0, dtype=np.uint8)])
    else:
        out["qmask2"] = np.zeros(0, dtype=np.uint8)
    span = [sum(ln for op, ln in r["cigar"] if bam_py._op_code(op) in (2, 3, 7, 8)) for r in keep]
    out["extent"] = np.array([len(keep), min([r["pos"] for r in keep], default=np.iinfo(np.int64).max),
                              max([r["pos"] + s for r, s in zip(keep, span)], default=0), ref], dtype=np.int64)
    return out


ARRAYS = ("pos", "cigar", "cig_off", "seq4", "seq_off", "qual", "qual_off", "qmask2", "extent")


def assert_same(got, exp, what=""):
    for k in ARRAYS:
        assert got[k].shape == exp[k].shape and (got[k] == exp[k]).all(), (what, k, got[k][:16], exp[k][:16])
    assert got["names"] == exp["names"], what


def qmask_bits(qmask2):
    """The device's mask of a whole record array (bit 2 * byte of seq4 + base of the byte) from a byte of two bits per byte of seq4."""
    bits = np.zeros(2 * len(qmask2), dtype=np.uint8)
    bits[0::2], bits[1::2] = qmask2 & 1, qmask2 >> 1
    return np.packbits(np.concatenate([bits, np.zeros(-len(bits) % 32, dtype=np.uint8)]), bitorder="little")


# ---------------------------------------------------------------------------------------------- the variety sample
VARIETY_REFS = [("first ref", 600), ("second", 5000), ("third", 900)]
VARIETY_MIN_QV = 20
_EVERY_TAG = [("XA", "A", "q"), ("Xc", "c", -7), ("XC", "C", 200), ("Xs", "s", -3000), ("XS", "S", 60000), ("Xi", "i", -70000),
              ("XI", "I", 4000000000), ("Xf", "f", 0.25), ("XZ", "Z", "text with spaces"), ("XH", "H", "1AE301"),
              ("Bc", "B", ("c", [-1, 2])), ("BC", "B", ("C", [1, 255, 3])), ("Bs", "B", ("s", [-300])), ("BS", "B", ("S", [65535, 1])),
              ("Bi", "B", ("i", [-70000, 5])), ("BI", "B", ("I", [])), ("Bf", "B", ("f", [1.5, -2.0]))]


def variety_records(n=260, seed=11):
    """At most 300 records on three references: every cigar op the specification names except M, zero-length ops, the undefined op
    codes 9..15, hard clips before soft clips, a padding in the middle, skips, an empty read, one- and two-base reads, names of 0 and
    254 characters, every aux type around the rq / dq / iq / sq tags, tracks shorter and longer than the read or absent, QUAL absent,
    qualities on both sides of VARIETY_MIN_QV, flags kept (0x800, 0x10, 0x400) and dropped (0x4, 0x100), records without a reference
    or a position, and records of the other references in between.  The kept reads lie on the first reference (600 columns)."""
    rng = np.random.default_rng(seed)
    letters = "ACGT" * 6 + "N" + "MRK="

    def quals(n_bases):
        q = rng.integers(0, 60, n_bases, dtype=np.uint8)
        q[rng.random(n_bases) < 0.05] = 0xFF
        return bytes(q)

    def track(n_bases):
        return "".join(chr(33 + int(v)) for v in rng.integers(5, 70, n_bases))

    def read(i, ref_id=0, flag=0):
        ops = []
        if rng.random() < 0.3:
            ops.append(("H", int(rng.integers(0, 40))))
        if rng.random() < 0.4:
            ops.append(("S", int(rng.integers(0, 9))))
        for _ in range(int(rng.integers(1, 9))):
            k = rng.random()
            if k < 0.45:
                ops.append((("=", "X")[int(rng.integers(2))], int(rng.integers(1, 60))))
            elif k < 0.55:
                ops.append(("I", int(rng.integers(0, 8))))
            elif k < 0.65:
                ops.append(("D", int(rng.integers(0, 12))))
            elif k < 0.72:
                ops.append(("N", int(rng.integers(0, 150))))
            elif k < 0.79:
                ops.append(("P", int(rng.integers(0, 30))))
            elif k < 0.88:
                ops.append((int(rng.integers(9, 16)), int(rng.integers(0, 1000))))
            else:
                ops.append((("=", "X", "S", "H")[int(rng.integers(4))], 0))
        if rng.random() < 0.4:
            ops.append(("S", int(rng.integers(0, 9))))
        if rng.random() < 0.3:
            ops.append(("H", int(rng.integers(0, 40))))
        l_seq = sum(ln for op, ln in ops if op in ("=", "X", "I", "S"))
        seq = "".join(letters[int(v)] for v in rng.integers(0, len(letters), l_seq))
        tags = []
        order = list(rng.permutation(len(_EVERY_TAG)))[:int(rng.integers(0, 6))]
        special = [("rq", "f", float(rng.choice([0.9, 0.99, 0.999, 0.9999])))] if rng.random() < 0.8 else []
        for name in ("dq", "iq", "sq"):
            k = rng.random()
            if k < 0.5:
                special.append((name, "Z", track(l_seq)))
            elif k < 0.65:
                special.append((name, "Z", track(int(rng.integers(0, l_seq + 1)))))
            elif k < 0.8:
                special.append((name, "Z", track(l_seq + int(rng.integers(1, 20)))))
        for t in special:                        # other tags before, between and after the four that are read
            if order:
                tags.append(_EVERY_TAG[order.pop()])
            tags.append(t)
        tags += [_EVERY_TAG[k] for k in order]
        return dict(ref_id=ref_id, pos=int(rng.integers(0, 520)), flag=flag, mapq=int(rng.integers(0, 255)), name="read/%d/ccs" % i,
                    cigar=ops, seq=seq if l_seq else "*", qual=None if rng.random() < 0.15 else quals(l_seq), tags=tags)

    out = []
    for i in range(n):
        k = rng.random()
        if k < 0.70:
            out.append(read(i, 0, int(rng.choice([0, 0, 0, 0x800, 0x10, 0x400, 0x810]))))
        elif k < 0.80:
            out.append(read(i, int(rng.integers(1, 3)), 0))
        elif k < 0.86:
            out.append(read(i, 0, int(rng.choice([0x4, 0x100, 0x104, 0x904]))))
        elif k < 0.90:
            out.append(dict(read(i, 0, 0), ref_id=-1))
        elif k < 0.94:
            out.append(dict(read(i, 0, 0), pos=-1))
        else:
            out.append(dict(read(i, 0, 0), tags=[_EVERY_TAG[j] for j in rng.permutation(len(_EVERY_TAG))]))
    hand = [
        dict(ref_id=0, pos=17, flag=0, mapq=1, name="", cigar=[], seq="*", qual=None, tags=[]),                      # l_read_name 1, no bases
        dict(ref_id=0, pos=3, flag=0, mapq=1, name="n" * 254, cigar=[("=", 1)], seq="G", qual=bytes([19]), tags=[]),   # l_read_name 255
        dict(ref_id=0, pos=599, flag=0, mapq=1, name="two", cigar=[("X", 1), ("I", 1)], seq="TC", qual=bytes([20, 0]), tags=[]),
        dict(ref_id=0, pos=100, flag=0, mapq=1, name="hs", cigar=[("H", 5), ("S", 2), ("=", 3), ("P", 4), ("=", 2), ("N", 300), ("X", 4)],
             seq="ACGTACGTACG", qual=bytes(range(15, 26)), tags=[("sq", "Z", "5" * 11)]),
        dict(ref_id=0, pos=0, flag=0, mapq=1, name="undefined ops", cigar=[(9, 5), ("=", 4), (15, 0xFFFFFFF), (12, 1), ("D", 2), ("=", 3)],
             seq="ACGTTGA", qual=None, tags=[("dq", "Z", chr(33 + 19) * 7)]),
    ]
    for k, r in enumerate(hand):
        out.insert(7 + 31 * k, r)
    return out
