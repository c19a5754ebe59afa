"""An independent BAM / BGZF writer and reader in plain Python (struct, zlib), written from the SAM specification (SAMv1 sections
4.1 BGZF and 4.2 BAM).  Test infrastructure: it imports nothing of the product and shares no code with its reader or writer, so a
layout misunderstanding that the product's reader and writer have in common shows as a difference against this file.

A record is a dictionary:
    ref_id, pos, flag, mapq, name (str), cigar [(op, len)] with op a letter of "MIDNSHP=X" or a code 0..15, seq (str, "*" = none),
    qual (bytes, or None = all 0xFF), tags [(tag, type, value)]
with aux types A c C s S i I f Z H and B (value = (subtype, [elements])); optional bin, next_ref_id, next_pos, tlen.
"""
import struct
import zlib

CIGAR_OPS = "MIDNSHP=X"
SEQ_CODES = "=ACMGRSVTWYHKDBN"
_AUX_FMT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}
MAX_BLOCK = 65536          # the largest payload ISIZE may announce
EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


# ------------------------------------------------------------------------------------------------------ BGZF
def bgzf_member(payload, level=6, extra=b""):
    """One BGZF block (a gzip member whose extra field holds the BC subfield = total block size - 1).  `extra`: further subfields
    (SI1 SI2 SLEN data), placed BEFORE the BC subfield, which the specification allows."""
    assert len(payload) <= MAX_BLOCK
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = co.compress(payload) + co.flush()
    xlen = len(extra) + 6
    bsize = 12 + xlen + len(body) + 8 - 1
    if bsize > 0xFFFF:
        raise ValueError("BGZF block of %d bytes: payload does not fit at this level" % (bsize + 1))
    head = struct.pack("<BBBBIBBH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, xlen)
    return head + extra + struct.pack("<BBHH", 66, 67, 2, bsize) + body + struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF, len(payload))


def bgzf_wrap(raw, block=0xff00, level=6, cuts=None, empty_at=(), eof=True, extra=b"", extra_on=None):
    """The stream `raw` as BGZF.  `block`: payload bytes per block (1 .. 65536); `cuts`: explicit payload boundaries (stream offsets,
    ascending) instead, with `block` applied between them; `empty_at`: indices of blocks in front of which an empty block is put;
    `eof`: the empty end-of-file block; `extra`: another extra subfield, on the blocks whose index is in `extra_on` (None = all)."""
    edges = [0] + sorted(c for c in (cuts or ()) if 0 < c < len(raw)) + [len(raw)]
    pieces = []
    for a, b in zip(edges, edges[1:]):
        pieces += [raw[o:min(o + block, b)] for o in range(a, b, block)]
    out = []
    for i, piece in enumerate(pieces):
        if i in empty_at:
            out.append(bgzf_member(b"", level))
        out.append(bgzf_member(piece, level, extra if (extra_on is None or i in extra_on) else b""))
    if eof:
        out.append(EOF_BLOCK)
    return b"".join(out)


def bgzf_unwrap(data):
    """The inflated stream of a BGZF file, block by block, checking every block's BC size, CRC-32 and ISIZE."""
    out, at = [], 0
    while at < len(data):
        magic, cm, flg, _mtime, _xfl, _os, xlen = struct.unpack_from("<HBBIBBH", data, at)
        if magic != 0x8b1f or cm != 8 or not flg & 4:
            raise ValueError("not a BGZF block at %d" % at)
        x, end, bsize = at + 12, at + 12 + xlen, None
        while x < end:
            si1, si2, slen = struct.unpack_from("<BBH", data, x)
            if (si1, si2) == (66, 67):
                bsize, = struct.unpack_from("<H", data, x + 4)
            x += 4 + slen
        if bsize is None:
            raise ValueError("BGZF block without a BC subfield at %d" % at)
        body = data[end:at + bsize + 1 - 8]
        crc, isize = struct.unpack_from("<II", data, at + bsize + 1 - 8)
        payload = zlib.decompress(body, -15)
        if len(payload) != isize or zlib.crc32(payload) & 0xFFFFFFFF != crc:
            raise ValueError("BGZF block at %d fails its ISIZE or CRC-32" % at)
        out.append(payload)
        at += bsize + 1
    return b"".join(out)


# ------------------------------------------------------------------------------------------------------ BAM: writing
def _op_code(op):
    return CIGAR_OPS.index(op) if isinstance(op, str) else int(op)


def pack_seq(seq):
    """Bases two to a byte, the FIRST base of a pair in the HIGH nibble; an odd last base leaves the low nibble 0."""
    codes = [SEQ_CODES.index(c) if c in SEQ_CODES else 15 for c in seq.upper()]
    if len(codes) & 1:
        codes.append(0)
    return bytes(codes[i] << 4 | codes[i + 1] for i in range(0, len(codes), 2))


def pack_aux(tags):
    out = bytearray()
    for tag, ty, value in tags:
        out += tag.encode("ascii") + ty.encode("ascii")
        if ty == "A":
            out += value.encode("ascii") if isinstance(value, str) else bytes([value])
        elif ty in _AUX_FMT:
            out += struct.pack(_AUX_FMT[ty], value)
        elif ty in "ZH":
            out += (value.encode("latin-1") if isinstance(value, str) else bytes(value)) + b"\0"
        elif ty == "B":
            sub, elems = value
            out += sub.encode("ascii") + struct.pack("<I", len(elems))
            for e in elems:
                out += struct.pack(_AUX_FMT[sub], e)
        else:
            raise ValueError("aux type " + ty)
    return bytes(out)


def reg2bin(beg, end):
    """SAMv1 section 5.3."""
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def pack_record(r, with_size=True):
    """One alignment record, block_size word first."""
    seq = "" if r.get("seq", "*") == "*" else r["seq"]
    qual = r.get("qual")
    qual = b"\xff" * len(seq) if qual is None else bytes(qual)
    assert len(qual) == len(seq)
    name = r.get("name", "").encode("latin-1") + b"\0"
    assert 1 <= len(name) <= 255
    cigar = [(_op_code(op), ln) for op, ln in r.get("cigar", ())]
    assert len(cigar) <= 65535
    span = sum(ln for op, ln in cigar if op in (0, 2, 3, 7, 8))
    pos = r.get("pos", -1)
    b = r["bin"] if "bin" in r else reg2bin(max(pos, 0), max(pos, 0) + max(span, 1)) & 0xFFFF
    body = struct.pack("<iiBBHHHIiii", r.get("ref_id", -1), pos, len(name), r.get("mapq", 0), b, len(cigar), r.get("flag", 0),
                       len(seq), r.get("next_ref_id", -1), r.get("next_pos", -1), r.get("tlen", 0))
    body += name + b"".join(struct.pack("<I", (ln << 4 | op) & 0xFFFFFFFF) for op, ln in cigar) + pack_seq(seq) + qual
    body += pack_aux(r.get("tags", ()))
    return (struct.pack("<i", len(body)) if with_size else b"") + body


def pack_header(text, refs, text_nul=False):
    """Magic, header text (`text_nul`: NUL-terminated, which the specification permits), the reference list [(name, length)]."""
    t = text.encode("latin-1") + (b"\0" if text_nul else b"")
    out = b"BAM\x01" + struct.pack("<i", len(t)) + t + struct.pack("<i", len(refs))
    for name, length in refs:
        n = name.encode("latin-1") + b"\0"
        out += struct.pack("<i", len(n)) + n + struct.pack("<i", length)
    return out


def bam_stream(text, refs, records, text_nul=False):
    """(the uncompressed BAM stream, the offset of every record's block_size word)."""
    out = bytearray(pack_header(text, refs, text_nul))
    at = []
    for r in records:
        at.append(len(out))
        out += pack_record(r)
    return bytes(out), at


def write_bam(path, text, refs, records, text_nul=False, **bgzf):
    """Writes the file; returns the record offsets in the uncompressed stream.  **bgzf: the knobs of bgzf_wrap."""
    raw, at = bam_stream(text, refs, records, text_nul)
    with open(path, "wb") as f:
        f.write(bgzf_wrap(raw, **bgzf))
    return at


# ------------------------------------------------------------------------------------------------------ BAM: reading
def unpack_aux(b):
    tags, o = [], 0
    while o < len(b):
        tag, ty = b[o:o + 2].decode("ascii"), chr(b[o + 2])
        o += 3
        if ty == "A":
            value, o = chr(b[o]), o + 1
        elif ty in _AUX_FMT:
            value, = struct.unpack_from(_AUX_FMT[ty], b, o)
            o += struct.calcsize(_AUX_FMT[ty])
        elif ty in "ZH":
            e = b.index(b"\0", o)
            value, o = b[o:e].decode("latin-1"), e + 1
        elif ty == "B":
            sub = chr(b[o])
            n, = struct.unpack_from("<I", b, o + 1)
            fmt = "<%d%s" % (n, _AUX_FMT[sub][1])
            value = (sub, list(struct.unpack_from(fmt, b, o + 5)))
            o += 5 + struct.calcsize(fmt)
        else:
            raise ValueError("aux type " + ty)
        tags.append((tag, ty, value))
    return tags


def unpack_stream(raw):
    """(text, refs, records) of an uncompressed BAM stream."""
    if raw[:4] != b"BAM\x01":
        raise ValueError("not a BAM stream")
    l_text, = struct.unpack_from("<i", raw, 4)
    text = raw[8:8 + l_text].decode("latin-1")
    at = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, at)
    at += 4
    refs = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", raw, at)
        name = raw[at + 4:at + 4 + l_name].rstrip(b"\0").decode("latin-1")
        length, = struct.unpack_from("<i", raw, at + 4 + l_name)
        refs.append((name, length))
        at += 8 + l_name
    records = []
    while at < len(raw):
        size, = struct.unpack_from("<i", raw, at)
        ref_id, pos, l_name, mapq, b, n_cig, flag, l_seq, nref, npos, tlen = struct.unpack_from("<iiBBHHHIiii", raw, at + 4)
        o = at + 36
        name = raw[o:o + l_name - 1].decode("latin-1")
        o += l_name
        words = struct.unpack_from("<%dI" % n_cig, raw, o)
        o += 4 * n_cig
        packed = raw[o:o + (l_seq + 1) // 2]
        o += (l_seq + 1) // 2
        seq = "".join(SEQ_CODES[packed[i >> 1] >> 4 if not i & 1 else packed[i >> 1] & 15] for i in range(l_seq))
        qual = raw[o:o + l_seq]
        o += l_seq
        records.append(dict(ref_id=ref_id, pos=pos, flag=flag, mapq=mapq, name=name, bin=b, next_ref_id=nref, next_pos=npos, tlen=tlen,
                            cigar=[(CIGAR_OPS[w & 15] if w & 15 < 9 else w & 15, w >> 4) for w in words], seq=seq if l_seq else "*",
                            qual=None if qual == b"\xff" * l_seq else qual, tags=unpack_aux(raw[o:at + 4 + size])))
        at += 4 + size
    return text, refs, records


def read_bam(path):
    with open(path, "rb") as f:
        return unpack_stream(bgzf_unwrap(f.read()))


def record_arrays(records, want_qual=True):
    """Records -> the flat arrays of the product's ingest (numpy): pos, cigar words, packed bases and QUAL with their offsets."""
    import numpy as np
    pos, cigar, cig_off, seq4, seq_off, qual, qual_off = [], [], [0], bytearray(), [0], bytearray(), [0]
    for r in records:
        seq = "" if r["seq"] == "*" else r["seq"]
        pos.append(r["pos"])
        cigar += [(ln << 4) | _op_code(op) for op, ln in r["cigar"]]
        seq4 += pack_seq(seq)
        qual += b"\xff" * len(seq) if r.get("qual") is None else bytes(r["qual"])
        cig_off.append(len(cigar)), seq_off.append(len(seq4)), qual_off.append(len(qual))
    out = dict(pos=np.array(pos, dtype=np.int32), cigar=np.array(cigar, dtype=np.uint32), cig_off=np.array(cig_off, dtype=np.uint64),
               seq4=np.frombuffer(bytes(seq4), dtype=np.uint8), seq_off=np.array(seq_off, dtype=np.uint64))
    if want_qual:
        out.update(qual=np.frombuffer(bytes(qual), dtype=np.uint8), qual_off=np.array(qual_off, dtype=np.uint64))
    return out
