"""Plain-Python model of dwgsim_eval-hip's truth section (dw_eval.hpp TRUTH), written from the rule and not from the kernels: it expands both
CIGARs into one state per query base and compares the states base by base.  parse_truth() reads a truth SAM (and says what is wrong with a
bad one, in the library's words), judge() is the rule for one aligned record, run() evaluates whole files next to eval_model.run() and gives
the section's text.  Test infrastructure only."""
from __future__ import annotations
import functools
import re
from dataclasses import dataclass, field

import eval_model as M

COLS = ["missing", "random", "unusable", "compared", "exact", "bases", "right", "clipped", "ibases", "iright"]
HEAD = b"# mapq\t" + "\t".join(COLS).encode() + b"\n"
CIG = re.compile(rb"(\d{1,9})([MIDNSHP=X])")
MAX_COUNT = (1 << 28) - 1


class TruthError(Exception):
    """a truth that the library refuses; str(e) is its last_error text"""


def key_of(qname: bytes, flag: int):
    """(QNAME, end), or None for a key that no truth record has"""
    if not flag & 1:
        return qname, 0
    end = (flag >> 6) & 3
    return (qname, end) if end in (1, 2) else None


@functools.lru_cache(maxsize=4096)
def cigar_ops(text: bytes):
    """((count, op), ...) of a CIGAR text, or None when it is no sequence of <count><operation> with counts below 2^28 (`*` is none)"""
    ops, at = [], 0
    while at < len(text):
        m = CIG.match(text, at)
        if not m or int(m.group(1)) > MAX_COUNT:
            return None
        ops.append((int(m.group(1)), m.group(2).decode()))
        at = m.end()
    return tuple(ops)


@dataclass
class TruthRec:
    unmapped: bool
    contig: bytes = b""
    pos0: int = 0
    reverse: bool = False
    ops: list = field(default_factory=list)

    @property
    def indel(self):
        return any(op in "ID" for _, op in self.ops)


def parse_truth(data: bytes) -> dict:
    """{key: TruthRec} of a truth SAM text; TruthError with the library's message for a bad one"""
    header, body = M.split_header(data)
    contigs = set(M.header_targets(header))
    out, first_line = {}, {}
    twice = None
    def bad(why):
        raise TruthError("truth: record line %d %s" % (no, why))

    for no, line in enumerate(M.record_lines(body), 1):
        f = line.split(b"\t", 11)
        if len(f) < 11:
            bad("has fewer than 11 fields")
        flag, pos1 = M.parse_uint(f[1], 0xFFFF), M.parse_uint(f[3], 0x7FFFFFFF)
        if not f[0] or len(f[0]) > 254 or flag is None or pos1 is None or key_of(f[0], flag) is None:
            bad("is not a truth record (QNAME, FLAG, POS or the end bits of FLAG)")
        if flag & 4:
            rec = TruthRec(True)
        else:
            if pos1 == 0:
                bad("is mapped at POS 0")
            if f[2] not in contigs:
                bad("has an RNAME that is not one of the truth's @SQ names")
            ops = cigar_ops(f[5])
            if not ops or any(op not in "MID" or n == 0 for n, op in ops) or not any(op in "MI" for _, op in ops):
                bad("has a CIGAR that is no sequence of M, I and D runs with a query base")
            rec = TruthRec(False, f[2], pos1 - 1, bool(flag & 16), ops)
        key = key_of(f[0], flag)
        if key in out:
            # (a bad line anywhere is reported before a repeated key: the index is built after the last line)
            twice = twice or (no, first_line[key])
        else:
            out[key] = rec
            first_line[key] = no
    if twice:
        raise TruthError("truth: the truth holds read of record line %d twice (its name and end are those of record line %d)" % twice)
    return out


def states(pos0: int, ops, truth: bool):
    """one (kind, r) per query base, kind M, I or C"""
    out, r = [], pos0
    for n, op in ops:
        if op in "M=X":
            out += [("M", r + k) for k in range(n)]
            r += n
        elif op == "I":
            out += [("I", r)] * n
        elif op in "SH":
            assert not truth
            out += [("C", None)] * n
        elif op in "DN":
            r += n
        else:
            assert op == "P" and not truth
    return out


def judge(t: TruthRec | None, rname, flag: int, pos1: int, cigar: bytes):
    """(outcome, counts) for one participating record; rname: the record's contig as the truth names it, or None for another contig.
    counts: {column: value} of a compared record plus "indel"."""
    if t is None:
        return "missing", {}
    if t.unmapped:
        return "random", {}
    ops = cigar_ops(cigar)
    if ops is None:
        return "unusable", {}
    a = states(pos1 - 1, ops, False)
    b = states(t.pos0, t.ops, True)
    if len(a) != len(b):
        return "unusable", {}
    same = rname is not None and rname == t.contig and bool(flag & 16) == t.reverse
    right = [same and x == y and x[0] in "MI" for x, y in zip(a, b)]
    c = {"bases": len(b), "right": sum(right), "clipped": sum(1 for x in a if x[0] == "C"), "ibases": sum(1 for y in b if y[0] == "I"),
         "iright": sum(1 for ok, y in zip(right, b) if ok and y[0] == "I"), "indel": t.indel}
    c["exact"] = int(c["right"] == c["bases"])
    return "compared", c


def section(counts) -> bytes:
    """the text of counts[stratum][mapq] = {column: value}"""
    out = b""
    for st in ("all", "indel"):
        out += b"## truth " + st.encode() + b"\n" + HEAD
        cum = dict.fromkeys(COLS, 0)
        rows = counts.get(st, {})
        for q in sorted(rows, reverse=True):
            for k in COLS:
                cum[k] += rows[q].get(k, 0)
            out += ("%d\t" % q + "\t".join(str(cum[k]) for k in COLS) + "\n").encode()
        if not rows:
            out += ("0" + "\t0" * len(COLS) + "\n").encode()
    return out


def count(counts, mapq, outcome, c):
    row = counts.setdefault("all", {}).setdefault(mapq, dict.fromkeys(COLS, 0))
    row[outcome] += 1
    if outcome == "compared":
        strata = [row] + ([counts.setdefault("indel", {}).setdefault(mapq, dict.fromkeys(COLS, 0))] if c["indel"] else [])
        if c["indel"]:
            strata[1]["compared"] += 1
        for r in strata:
            for k in ("exact", "bases", "right", "clipped", "ibases", "iright"):
                r[k] += c[k]


def run(truth: bytes, files, o: M.Opts | None = None):
    """(eval_model.Result of the files, the truth section's text: empty after a fatal record)"""
    o = o or M.Opts()
    tr = parse_truth(truth)
    tcontigs = set(M.header_targets(M.split_header(truth)[0]))
    main = M.run(files, o)
    if main.status:
        return main, b""
    counts: dict = {}
    prev = None
    for data in files:
        header, body = M.split_header(data)
        targets = M.header_targets(header)
        tset = set(targets)
        for line in M.record_lines(body):
            code, _, skipped, _, cls, _ = M.eval_record(line, prev, targets, tset, o)
            assert not code
            prev = line
            f = line.split(b"\t")
            flag = int(f[1])
            if skipped or cls < 0 or flag & 4:
                continue
            key = key_of(f[0], flag)
            rname = f[2] if f[2] in tset and f[2] in tcontigs else None
            outcome, c = judge(tr.get(key) if key else None, rname, flag, int(f[3]), f[5])
            count(counts, int(f[4]), outcome, c)
    return main, section(counts)
