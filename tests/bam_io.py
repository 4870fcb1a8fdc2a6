"""Test-only BAM writer and reader for the dwgsim_eval BAM tests: zlib and struct, nothing from the product.

sam_to_bam() encodes SAM text as a BAM file (BGZF blocks of a chosen uncompressed size, zlib level and strategy); bam_to_sam() is an
independent decoder that prints records by the rules of dwgsim_eval-hip's -p output.  The expected result of every BAM test is
the plain-Python model (eval_model.py) on bam_to_sam(bam): the model never sees product code."""
from __future__ import annotations
import struct, zlib

CIGAR_OPS = "MIDNSHP=X"
SEQ_CODES = "=ACMGRSVTWYHKDBN"
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def split_header(sam: bytes):
    i = 0
    while i < len(sam) and sam[i] == 64:
        j = sam.find(b"\n", i)
        i = len(sam) if j < 0 else j + 1
    return sam[:i], sam[i:]


def header_refs(header: bytes):
    refs = []
    for line in header.split(b"\n"):
        if line.startswith(b"@SQ"):
            name, length = None, 0
            for f in line.split(b"\t")[1:]:
                if f.startswith(b"SN:"):
                    name = f[3:]
                elif f.startswith(b"LN:"):
                    length = int(f[3:])
            if name is not None:
                refs.append((name, length))
    return refs


def _int_tag(v: int) -> bytes:
    """the smallest type that holds v, as samtools chooses it"""
    if v >= 0:
        return b"C" + struct.pack("<B", v) if v <= 0xFF else b"S" + struct.pack("<H", v) if v <= 0xFFFF else b"I" + struct.pack("<I", v & 0xFFFFFFFF)
    return b"c" + struct.pack("<b", v) if v >= -128 else b"s" + struct.pack("<h", v) if v >= -32768 else b"i" + struct.pack("<i", max(v, -(1 << 31)))


B_FMT = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}


def _aux(field: bytes) -> bytes:
    tag, ty, val = field[:2], chr(field[3]), field[5:]
    if ty == "i":
        return tag + _int_tag(int(val))
    if ty == "A":
        return tag + b"A" + val[:1]
    if ty == "f":
        return tag + b"f" + struct.pack("<f", float(val))
    if ty in "ZH":
        return tag + ty.encode() + val + b"\0"
    if ty == "B":
        sub = chr(val[0]); vals = [x for x in val[2:].split(b",") if x]
        conv = float if sub == "f" else int
        return tag + b"B" + sub.encode() + struct.pack("<I", len(vals)) + b"".join(struct.pack("<" + B_FMT[sub], conv(x)) for x in vals)
    raise ValueError("aux type %r" % ty)


def encode_record(line: bytes, ref_index: dict) -> bytes:
    f = line.split(b"\t")
    qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = f[:11]
    # (a name outside the reference list has no index: the record says "no reference", as for "*")
    ref_id = ref_index.get(rname, -1)
    next_id = ref_id if rnext == b"=" else ref_index.get(rnext, -1)
    ops = []
    if cigar != b"*":
        num = 0
        for ch in cigar.decode():
            if ch.isdigit():
                num = num * 10 + int(ch)
            else:
                ops.append(num << 4 | CIGAR_OPS.index(ch)); num = 0
    if seq == b"*":
        l_seq, packed, q = 0, b"", b""
    else:
        l_seq = len(seq)
        codes = [SEQ_CODES.index(chr(c).upper()) for c in seq] + [0]
        packed = bytes(codes[i] << 4 | codes[i + 1] for i in range(0, l_seq, 2))
        q = b"\xff" * l_seq if qual == b"*" else bytes(c - 33 for c in qual)
    body = struct.pack("<iiBBHHHiiii", ref_id, int(pos) - 1, len(qname) + 1, int(mapq), 4680, len(ops), int(flag), l_seq, next_id, int(pnext) - 1, int(tlen))
    body += qname + b"\0" + b"".join(struct.pack("<I", o) for o in ops) + packed + q + b"".join(_aux(x) for x in f[11:])
    return struct.pack("<I", len(body)) + body


def bam_payload(sam: bytes, refs=None, text=None):
    """(uncompressed BAM bytes, offset of every record in them); refs / text replace the header's @SQ list / the header text"""
    header, body = split_header(sam)
    refs = header_refs(header) if refs is None else refs
    text = header if text is None else text
    out = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, length in refs:
        out += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", length)
    ref_index = {}
    for k, (name, _) in enumerate(refs):
        ref_index.setdefault(name, k)
    parts, offs, at = [out], [], len(out)
    for line in body.split(b"\n"):
        if line:
            rec = encode_record(line, ref_index)
            offs.append(at); parts.append(rec); at += len(rec)
    return b"".join(parts), offs


def bgzf_block(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=None) -> bytes:
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush_every:
        z = b"".join(co.compress(data[i:i + flush_every]) + co.flush(zlib.Z_FULL_FLUSH) for i in range(0, len(data), flush_every)) + co.flush()
    else:
        z = co.compress(data) + co.flush()
    size = 18 + len(z) + 8
    assert size <= 65536, size
    return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", size - 1) + z + struct.pack("<II", zlib.crc32(data), len(data))


def bgzf(payload: bytes, block_bytes=65280, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=None, eof=True) -> bytes:
    blocks = [bgzf_block(payload[i:i + block_bytes], level, strategy, flush_every) for i in range(0, len(payload), block_bytes)]
    return b"".join(blocks) + (EOF_BLOCK if eof else b"")


def sam_to_bam(sam: bytes, block_bytes=65280, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=None, eof=True) -> bytes:
    return bgzf(bam_payload(sam)[0], block_bytes, level, strategy, flush_every, eof)


# ---- the decoder ----

def bgzf_inflate(bam: bytes) -> bytes:
    out, i = [], 0
    while i < len(bam):
        assert bam[i:i + 4] == b"\x1f\x8b\x08\x04", i
        xlen = struct.unpack_from("<H", bam, i + 10)[0]
        q, size = i + 12, None
        while q < i + 12 + xlen:
            si, slen = bam[q:q + 2], struct.unpack_from("<H", bam, q + 2)[0]
            if si == b"BC":
                size = struct.unpack_from("<H", bam, q + 4)[0] + 1
            q += 4 + slen
        data = zlib.decompress(bam[i + 12 + xlen:i + size - 8], -15)
        crc, isize = struct.unpack_from("<II", bam, i + size - 8)
        assert zlib.crc32(data) == crc and len(data) == isize
        out.append(data); i += size
    return b"".join(out)


def _g(v: float) -> str:
    return "%g" % v


def _aux_text(b: bytes) -> list:
    """the aux fields as SAM text, up to the first one that cannot be read whole"""
    out, p, n = [], 0, len(b)
    while n - p >= 3:
        tag, ty, v = b[p:p + 2].decode("latin-1"), chr(b[p + 2]), p + 3
        if ty == "A":
            if n - v < 1:
                break
            out.append("%s:A:%s" % (tag, chr(b[v]))); p = v + 1
        elif ty in "ZH":
            e = b.find(b"\0", v)
            if e < 0:
                break
            out.append("%s:%s:%s" % (tag, ty, b[v:e].decode("latin-1"))); p = e + 1
        elif ty == "B":
            if n - v < 5 or chr(b[v]) not in B_FMT:
                break
            sub = chr(b[v]); cnt = struct.unpack_from("<I", b, v + 1)[0]; es = struct.calcsize(B_FMT[sub])
            if n - (v + 5) < es * cnt:
                break
            vals = struct.unpack_from("<%d%s" % (cnt, B_FMT[sub]), b, v + 5)
            out.append("%s:B:%s" % (tag, sub) + "".join("," + (_g(x) if sub == "f" else str(x)) for x in vals)); p = v + 5 + es * cnt
        elif ty in B_FMT:
            es = struct.calcsize(B_FMT[ty])
            if n - v < es:
                break
            x = struct.unpack_from("<" + B_FMT[ty], b, v)[0]
            out.append("%s:f:%s" % (tag, _g(x)) if ty == "f" else "%s:i:%d" % (tag, x)); p = v + es
        else:
            break
    return out


def decode_record(rec: bytes, names) -> bytes:
    """one record (behind its block_size) as a SAM line"""
    ref_id, pos, l_name, mapq, _bin, n_cigar, flag, l_seq, next_id, next_pos, tlen = struct.unpack_from("<iiBBHHHiiii", rec, 0)
    ref = lambda t: names[t].decode("latin-1") if 0 <= t < len(names) else "*"
    p = 32
    qname = rec[p:p + l_name].split(b"\0")[0].decode("latin-1"); p += l_name
    cig = struct.unpack_from("<%dI" % n_cigar, rec, p); p += 4 * n_cigar
    seq = rec[p:p + (l_seq + 1) // 2]; p += (l_seq + 1) // 2
    qual = rec[p:p + l_seq]; p += l_seq
    f = [qname, str(flag), ref(ref_id), str(pos + 1), str(mapq),
         "".join("%d%s" % (c >> 4, CIGAR_OPS[c & 15]) for c in cig) or "*",
         "*" if next_id < 0 else "=" if next_id == ref_id else ref(next_id), str(next_pos + 1), str(tlen),
         "".join(SEQ_CODES[(seq[k >> 1] >> (0 if k & 1 else 4)) & 15] for k in range(l_seq)) or "*",
         "*" if not l_seq or qual[0] == 0xFF else "".join(chr(c + 33) for c in qual)]
    return "\t".join(f + _aux_text(rec[p:])).encode("latin-1")


def bam_to_sam(bam: bytes, sq_from_refs=False) -> bytes:
    """the SAM text of a BAM file: its header text (cut at a NUL; with sq_from_refs, @SQ lines made from the binary list are put in front) and
    every record"""
    d = bgzf_inflate(bam)
    assert d[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", d, 4)[0]
    text = d[8:8 + l_text].split(b"\0")[0]
    p = 8 + l_text
    n_ref = struct.unpack_from("<i", d, p)[0]; p += 4
    names, lens = [], []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", d, p)[0]; p += 4
        names.append(d[p:p + l_name].split(b"\0")[0]); p += l_name
        lens.append(struct.unpack_from("<i", d, p)[0]); p += 4
    if sq_from_refs:
        text = b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (n, l) for n, l in zip(names, lens)) + text
    lines = []
    while p < len(d):
        bs = struct.unpack_from("<I", d, p)[0]
        lines.append(decode_record(d[p + 4:p + 4 + bs], names)); p += 4 + bs
    return text + b"".join(l + b"\n" for l in lines)
