"""Plain-Python model of dwgsim_eval (SAM text only), restated from the semantics listed in DESIGN.md
"dwgsim_eval-hip".  It is the yardstick the GPU evaluator (dwgsim_amd/csrc/dw_eval.*) is held to byte for byte,
and it is itself held to the hand-worked fixtures of tests/test_eval_model.py.

Inputs are the raw bytes of each SAM file (header lines first).  Options are those of the command line:
a, d, g, q, n, s, e (ints), b, c, i, m, p, z (flags), P (bytes or None).
"""
from __future__ import annotations
import math
from dataclasses import dataclass, field

MINAS = -5000
MAXQ = 255
BREAK = "************************************************************\n"
# error codes, shared with include/dwgsim_hip.h (DWGSIM_HIP_EVAL_E_*)
E_MALFORMED, E_PREFIX, E_NAME, E_CONTIG, E_RANDOM_CORRECT, E_PAIRED, E_NOT_PAIRED = 1, 2, 3, 4, 5, 6, 7
TO_RM = b"_::_::_______"
MC, MI, MU, UM, UU = range(5)
WS = b" \t\n\v\f\r"


def wrap32(v: int) -> int:
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v


def cdiv(a: int, b: int) -> int:
    """C division (truncation toward zero) of int32 values, wrapped as int32"""
    q = abs(a) // abs(b)
    return wrap32(q if (a < 0) == (b < 0) else -q)


def strtoll(s: bytes) -> int:
    """strtoll(s, 0, 10): leading white space, sign, digits; saturates; 0 when there are no digits"""
    i = 0
    while i < len(s) and s[i] in WS:
        i += 1
    neg = False
    if i < len(s) and s[i] in b"+-":
        neg = s[i] == ord("-"); i += 1
    v = 0; nd = 0
    while i < len(s) and 48 <= s[i] <= 57:
        v = v * 10 + s[i] - 48; i += 1; nd += 1
    if nd == 0:
        return 0
    v = -v if neg else v
    return max(-(1 << 63), min((1 << 63) - 1, v))


def scan_name(s: bytes):
    """sscanf(s, "%s %d %d %1d %1d %1d %1d %d %d %d %d %d %d %s"): the 14 values, or None when fewer convert
    (%d is glibc's: a saturating long stored into an int, i.e. its low 32 bits; a width counts the sign)"""
    out = []; i = 0; n = len(s)
    for k, spec in enumerate(["s", "d", "d", "1", "1", "1", "1", "d", "d", "d", "d", "d", "d", "s"]):
        while i < n and s[i] in WS:           # ' ' in the format and every directive but %c skip white space
            i += 1
        if i >= n:
            return None
        if spec == "s":
            j = i
            while j < n and s[j] not in WS:
                j += 1
            out.append(s[i:j]); i = j
            continue
        width = 1 if spec == "1" else 1 << 30
        j = i; neg = False
        if s[j] in b"+-":
            neg = s[j] == ord("-"); j += 1; width -= 1
        v = 0; nd = 0
        while j < n and width > 0 and 48 <= s[j] <= 57:
            v = v * 10 + s[j] - 48; j += 1; nd += 1; width -= 1
        if nd == 0:
            return None
        v = -v if neg else v
        v = max(-(1 << 63), min((1 << 63) - 1, v))
        out.append(wrap32(v)); i = j
    return out


def replace_separators(q: bytes) -> bytes:
    """the last 13 of `_ : : _ : : _ _ _ _ _ _ _`, matched from the right, become spaces"""
    b = bytearray(q); j = 0
    for i in range(len(b) - 1, -1, -1):
        if j >= 13:
            break
        if b[i] == TO_RM[j]:
            b[i] = 32; j += 1
    return bytes(b)


def parse_uint(f: bytes, hi: int):
    if not f or not f.isdigit() or len(f) > 10:
        return None
    v = int(f)
    return v if v <= hi else None


def leading_clip(cigar: bytes) -> int:
    clip = 0; i = 0
    if cigar == b"*":
        return 0
    while i < len(cigar):
        j = i
        while j < len(cigar) and 48 <= cigar[j] <= 57:
            j += 1
        if j == len(cigar):
            break
        op = cigar[j]
        if op in b"SH":
            clip += int(cigar[i:j] or b"0")
        else:
            break
        i = j + 1
    return clip


def aux_int(fields, tag: bytes):
    """bam_aux_get + bam_aux2i on SAM text: None when the tag is missing; an i value wraps to int32; other types give 0"""
    for f in fields:
        if len(f) >= 5 and f[:2] == tag and f[2] == 58 and f[4] == 58:
            return wrap32(strtoll(f[5:])) if f[3] == ord("i") else 0
    return None


@dataclass
class Opts:
    a: int = 0; b: int = 0; c: int = 0; d: int = 1; e: int = -1; g: int = 5; i: int = 0; m: int = 0
    n: int = 0; p: int = 0; q: int = 0; s: int = -1; z: int = 0; P: bytes | None = None


@dataclass
class Result:
    status: int = 0
    stdout: bytes = b""
    stderr: bytes = b""
    n: int = 0
    error_code: int = 0
    error_record: int = -1          # 0-based index among all record lines of the run
    table: bytes = b""
    incorrect: bytes = b""          # the -p part of stdout: first header, then the incorrect records verbatim
    hist: dict = field(default_factory=dict)


def error_block(fn: str, var, msg: str, fatal: bool = True) -> str:
    s = BREAK + '\rIn function "%s": %s[%s]. ' % (fn, "Fatal Error" if fatal else "Warning", "OutOfRange")
    if var is not None:
        s += "Variable/Value: %s.\n" % var
    s += "Message: %s.\n" % msg
    s += (" ***** Exiting due to errors *****\n" if fatal else " ***** Warning *****\n") + BREAK
    return s


def split_header(data: bytes):
    """leading lines that start with '@' are the header"""
    i = 0
    while i < len(data) and data[i] == ord("@"):
        j = data.find(b"\n", i)
        i = len(data) if j < 0 else j + 1
    return data[:i], data[i:]


def header_targets(header: bytes):
    names = []
    for line in header.split(b"\n"):
        if line.startswith(b"@SQ"):
            for f in line.split(b"\t")[1:]:
                if f.startswith(b"SN:"):
                    names.append(f[3:]); break
    return names


def eval_record(line: bytes, prev: bytes | None, targets, tset, o: Opts):
    """(error code, error variable text, skipped by -m, counts in n, class or -1, score)"""
    f = line.split(b"\t")
    if len(f) < 11:
        return E_MALFORMED, None, False, 0, -1, 0
    qname = f[0]
    flag = parse_uint(f[1], 0xFFFF); pos1 = parse_uint(f[3], 0x7FFFFFFF); mapq = parse_uint(f[4], 255)
    if not qname or len(qname) > 254 or flag is None or pos1 is None or mapq is None:
        return E_MALFORMED, None, False, 0, -1, 0
    read1 = flag & 0x40
    if o.m and prev is not None:
        pf = prev.split(b"\t")
        if pf[0] == qname and (int(pf[1]) & 0x40) == read1:
            return 0, None, True, 0, -1, 0
    paired = flag & 1
    n_inc = 1 if (not paired or read1) else 0

    def zcheck(cls, score):
        if paired and o.z:
            return E_PAIRED, None, False, n_inc, -1, 0
        if not paired and not o.z:
            return E_NOT_PAIRED, None, False, n_inc, -1, 0
        return 0, None, False, n_inc, cls, score

    if mapq < o.q:
        return zcheck(-1, 0)
    name = replace_separators(qname)
    if o.P is not None:
        if len(name) < len(o.P) or name[:len(o.P)] != o.P:
            return E_PREFIX, name, False, n_inc, -1, 0
        name = name[len(o.P) + 1:] if len(name) > len(o.P) else b""
    v = scan_name(name)
    if v is None:
        return E_NAME, name, False, n_inc, -1, 0
    chr_name, p1, p2, s1, s2, r1, r2, e1, u1, i1, e2, u2, i2, _ = v
    first = o.z or read1
    rand = r1 if first else r2
    if rand == 0:
        if not any(name[:min(len(name), len(t))] == t[:min(len(name), len(t))] for t in targets):
            return E_CONTIG, name, False, n_inc, -1, 0
    unmapped = flag & 4
    if o.a == 0:
        metric = min(cdiv(mapq, o.d), MAXQ)
    elif unmapped or mapq == 0:
        metric = MINAS
    elif o.a in (1, 2, 3):
        opt = f[11:]
        AS = aux_int(opt, b"AS") if o.a in (1, 3) else 0
        XS = aux_int(opt, b"XS") if o.a in (2, 3) else 0
        if AS is None or XS is None:
            metric = MINAS
        else:
            metric = AS if o.a == 1 else XS if o.a == 2 else wrap32(AS - XS)
    else:
        metric = MINAS
    metric = cdiv(metric, o.d)
    metric = max(metric, MINAS)
    if o.i:
        if (i1 if first else i2) == 0:
            return zcheck(-1, 0)
    elif o.e >= 0 and e1 != o.e:
        return zcheck(-1, 0)
    elif o.s >= 0 and u1 != o.s:
        return zcheck(-1, 0)
    pos, strand = (p1, s1) if first else (p2, s2)
    if unmapped:
        pred = 2
    else:
        left = pos1 - 1 - leading_clip(f[5])
        rname = f[2]
        if rand == 1 or strand != (1 if flag & 16 else 0) or rname not in tset or rname != chr_name or abs(pos - left) > o.g:
            pred = 1
        else:
            pred = 0
    if rand == 1:
        if pred == 0:
            return E_RANDOM_CORRECT, None, False, n_inc, -1, 0
        cls = UM if pred == 1 else UU
    else:
        cls = (MC, MI, MU)[pred]
    return zcheck(cls, metric)


ERR_TEXT = {
    E_MALFORMED: ("process_bam", "[dwgsim_eval-hip] malformed SAM record"),
    E_PREFIX: ("process_bam", "[dwgsim_eval] could not match read name with given read name prefix (-P)"),
    E_NAME: ("process_bam", "[dwgsim_eval] read was not generated by dwgsim?"),
    E_CONTIG: ("process_bam", "[dwgsim_eval] the mapped contig does not exist in the SAM header; perhaps you have a read name prefix?"),
    E_RANDOM_CORRECT: ("dwgsim_eval_counts_add", "predicted value cannot be mapped correctly when the read is unmappable"),
    E_PAIRED: ("run", "Found a read that was paired end"),
    E_NOT_PAIRED: ("run", "Found a read that was not paired"),
}


def error_text(code: int, var) -> str:
    fn, msg = ERR_TEXT[code]
    if code == E_RANDOM_CORRECT:
        var = b"predicted_value"
    return error_block(fn, None if var is None else var.decode("latin-1"), msg)


def format_table(hist: dict, a: int, d: int) -> bytes:
    lo = min([0] + list(hist)); hi = max([0] + list(hist))
    rows = [hist.get(s, [0] * 5) for s in range(lo, hi + 1)]
    total = sum(sum(r) for r in rows)
    m_total = sum(r[0] + r[1] + r[2] for r in rows)
    u_total = sum(r[3] + r[4] for r in rows)
    w = int(1 + math.log10(total)) if total > 0 else 1
    out = ["# thr | the minimum %s threshold\n" % ("mapping quality" if a == 0 else "alignment score")]
    out += [l + "\n" for l in HEADER_LINES]
    sums = [0] * 5; mm_total = 0
    for k in range(len(rows) - 1, -1, -1):
        r = rows[k]
        for c in range(5):
            sums[c] += r[c]
        mm_total += r[0] + r[1]
        den = r[0] + r[1] + r[2]; sens_at = r[0] / den if den else 0.0
        sens_ge = sums[0] / m_total if m_total else 0.0
        den = r[0] + r[1]; ppv_at = r[0] / den if den else 0.0
        ppv_ge = sums[0] / mm_total if mm_total else 0.0
        den = r[3] + r[4]; fdr_at = r[3] / den if den else 0.0
        fdr_ge = sums[3] / u_total if u_total else 0.0
        ints = list(r) + [sum(r)] + sums + [sum(sums)]
        out.append("%.2d " % wrap32((k + lo) * d) + "".join("%*d " % (w, v) for v in ints)
                   + "%.3e %.3e %.3e %.3e %.3e %.3e\n" % (sens_at, ppv_at, fdr_at, sens_ge, ppv_ge, fdr_ge))
    return "".join(out).encode()


HEADER_LINES = [
    "# mc | the number of correctly mapped reads that should be mapped at the threshold",
    "# mi | the number of incorrectly mapped reads that should be mapped at the threshold",
    "# mu | the number of unmapped reads that should be mapped at the threshold",
    "# um | the number of mapped reads that should be unmapped at the threshold",
    "# uu | the number of unmapped reads that should be unmapped at the threshold",
    "# mc + mi + mu + um + uu | the total number of reads at the threshold",
    "# mc' | the number of correctly mapped reads that should be mapped at or greater than that threshold",
    "# mi' | the number of incorrectly mapped reads that should be mapped at or greater than that threshold",
    "# mu' | the number of unmapped reads that should be mapped at or greater than that threshold",
    "# um' | the number of mapped reads that should be unmapped at or greater than that threshold",
    "# uu' | the number of unmapped reads that should be unmapped at or greater than that threshold",
    "# mc' + mi' + mu' + um' + uu' | the total number of reads at or greater than the threshold",
    "# (mc / (mc' + mi' + mu')) | sensitivity: the fraction of mappable reads that are mapped correctly at the threshold",
    "# (mc / (mc' + mi')) | positive predictive value: the fraction of mapped mappable reads that are mapped correctly at the threshold",
    "# (um / (um' + uu')) | false discovery rate: the fraction of random reads that are mapped at the threshold",
    "# (mc' / (mc' + mi' + mu')) | sensitivity: the fraction of mappable reads that are mapped correctly at or greater than the threshold",
    "# (mc' / (mc' + mi')) | positive predictive value: the fraction of mapped mappable reads that are mapped correctly at or greater than the threshold",
    "# (um' / (um' + uu')) | false discovery rate: the fraction of random reads that are mapped at or greater than the threshold",
]


def record_lines(body: bytes):
    """the record lines of a file body (a last line without its newline still counts)"""
    if not body:
        return []
    lines = body.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    return lines


def run(files, o: Opts | None = None, on_record=None) -> Result:
    """Evaluate the SAM texts in `files` (bytes each, or iterables of (header, body) pairs).  on_record, when given,
    replaces the files' bodies with an iterator of lines per file (the >2^31-byte test streams its input)."""
    o = o or Opts()
    if o.d == 0:
        raise ValueError("-d 0")
    res = Result()
    err = "Analyzing...\nCurrently on:\n0"
    hist: dict = {}
    incorrect = []
    n = 0; idx = 0; prev = None
    for fi, data in enumerate(files):
        if isinstance(data, tuple):
            header, lines = data
        else:
            header, body = split_header(data)
            lines = record_lines(body)
        targets = header_targets(header)
        tset = set(targets)
        if fi == 0 and o.p:
            incorrect.append(header)
        for line in lines:
            code, var, skipped, n_inc, cls, score = eval_record(line, prev, targets, tset, o)
            if code:
                res.status = 1; res.error_code = code; res.error_record = idx; res.n = n + n_inc
                res.stderr = (err + error_text(code, var)).encode()
                return res
            idx += 1
            prev = line
            if skipped:
                continue
            n += n_inc
            if cls >= 0:
                hist.setdefault(score, [0] * 5)[cls] += 1
                if o.p and cls in (MI, UM):
                    incorrect.append(line + b"\n")
    res.n = n
    err += "\r%d\n" % n
    if o.n > 0 and n != o.n:
        err += "(-n)=%d\tn=%d\n" % (o.n, n)
        err += error_block("run", None, "Number of reads found differs from the number specified (-n)", fatal=False)
    err += "Analysis complete.\n"
    res.hist = hist
    res.table = format_table(hist, o.a, o.d)
    res.incorrect = b"".join(incorrect)
    res.stdout = res.incorrect + res.table
    res.stderr = err.encode()
    return res
