"""Test-only generator for the truth section of dwgsim_eval-hip: a truth SAM with random CIGARs over M, I and D (leading and trailing I, unmapped
random reads) under names of eval_sam's generator, and an aligner's output over it in which every record is in one of the STATES below, at
least 5 % of the records in each.  make() returns both texts; the expected section is eval_truth_model's."""
from __future__ import annotations
import random

import eval_sam as S

STATES = ["exact", "shifted", "soft", "hard", "eqx", "indel_moved", "ins_to_mismatch", "n_for_d", "strand", "contig", "rname_star", "unmapped",
          "random_mapped", "unknown_name", "trimmed", "cigar_star", "secondary"]
CONTIGS = [("chr1", 5000), ("chr10", 3000), ("chr2_alt", 2000)]
EXTRA = ("chrUn", 1500)           # in the aligner's headers only: a target that no truth contig has
MAPQS = [0, 0, 1, 3, 17, 20, 37, 60, 254, 255]


def header(contigs) -> bytes:
    return S.header(contigs)


def truth_cigar(rng: random.Random):
    """[(count, op)] over M I D: most reads one M run, the others with up to three indels, some with an I at an end"""
    n = rng.randrange(30, 70)
    if rng.random() < 0.45:
        return [(n, "M")]
    ops = []
    if rng.random() < 0.2:
        ops.append((rng.randrange(1, 4), "I"))
    for _ in range(rng.randrange(1, 4)):
        ops.append((rng.randrange(4, 25), "M"))
        ops.append((rng.randrange(1, 5), rng.choice("ID")))
    ops.append((rng.randrange(4, 25), "M"))
    if rng.random() < 0.2:
        ops.append((rng.randrange(1, 4), "I"))
    return ops


def text(ops) -> str:
    return "".join("%d%s" % (n, op) for n, op in ops)


def merged(ops):
    out = []
    for n, op in ops:
        if n == 0:
            continue
        if out and out[-1][1] == op:
            out[-1] = (out[-1][0] + n, op)
        else:
            out.append((n, op))
    return out


def clip_ends(ops, pos, a, b, ch):
    """the first a and the last b query bases become clips of kind ch: (ops, pos)"""
    ops = list(ops)
    left = a
    while left:
        n, op = ops[0]
        if op == "D":
            ops.pop(0); pos += n
            continue
        k = min(n, left)
        left -= k
        if op == "M":
            pos += k
        ops[0] = (n - k, op)
        if n == k:
            ops.pop(0)
    while ops and ops[0][1] == "D":
        pos += ops.pop(0)[0]
    left = b
    while left:
        n, op = ops[-1]
        if op == "D":
            ops.pop()
            continue
        k = min(n, left)
        left -= k
        ops[-1] = (n - k, op)
        if n == k:
            ops.pop()
    while ops and ops[-1][1] == "D":
        ops.pop()
    return ([(a, ch)] if a else []) + ops + ([(b, ch)] if b else []), pos


def qlen(ops):
    return sum(n for n, op in ops if op in "MIS=XH")


def perturb(rng, state, ops, pos):
    """(cigar text, pos) of the aligner's record in `state`, from the truth's ops and 1-based POS"""
    if state == "shifted":
        d = rng.randrange(1, 21) * rng.choice([-1, 1])
        return text(ops), max(1, pos + d) if pos + d != pos else pos + 1
    if state in ("soft", "hard"):
        q = qlen(ops)
        a, b = rng.randrange(0, min(6, q // 3)), rng.randrange(0, min(6, q // 3))
        if a + b == 0:
            a = 1
        new, p = clip_ends(ops, pos, a, b, "S" if state == "soft" else "H")
        return text(new), p
    if state == "eqx":
        new = []
        for n, op in ops:
            while op == "M" and n:
                k = rng.randrange(1, n + 1)
                new.append((k, rng.choice("=X"))); n -= k
            if op != "M":
                new.append((n, op))
        return text(new), pos
    if state == "indel_moved":
        for i in range(1, len(ops) - 1):
            if ops[i][1] in "ID" and ops[i - 1][1] == "M" and ops[i + 1][1] == "M" and ops[i - 1][0] > 1:
                new = list(ops)
                new[i - 1] = (ops[i - 1][0] - 1, "M"); new[i + 1] = (ops[i + 1][0] + 1, "M")
                return text(new), pos
        n = ops[0][0] if ops[0][1] == "M" else 0
        if n > 3:       # no movable indel: a false one, query length kept
            return text(merged([(n // 2, "M"), (1, "I"), (n - n // 2 - 1, "M")] + list(ops[1:]))), pos
        return text(ops), pos + 1
    if state == "ins_to_mismatch":
        if ops[0][1] == "I":      # a leading insertion as matches: the alignment starts that much earlier
            pos = max(1, pos - ops[0][0])
        return text(merged([(n, "M" if op == "I" else op) for n, op in ops])), pos
    if state == "n_for_d":
        if any(op == "D" for _, op in ops):
            return text([(n, "N" if op == "D" else op) for n, op in ops]), pos
        i = next(k for k, (n, op) in enumerate(ops) if op == "M" and n >= 2)
        n = ops[i][0]
        return text(list(ops[:i]) + [(n // 2, "M"), (rng.randrange(1, 50), "N"), (n - n // 2, "M")] + list(ops[i + 1:])), pos
    if state == "trimmed":
        q = qlen(ops)
        new, p = clip_ends(ops, pos, 0, rng.randrange(1, min(8, q - 1)), "S")
        return text(new[:-1]), p
    return text(ops), pos


def make(seed: int, n_reads: int, paired: bool = True, contigs=CONTIGS, rand_frac=0.09):
    """(truth SAM text, aligner's record lines, the state of every line).  n_reads names: two truth records each when paired."""
    rng = random.Random(seed)
    names = S.synth_names(rng, contigs, n_reads + n_reads // 8, rand_frac=rand_frac)
    unknown = names[n_reads:]
    names = names[:n_reads]
    truth, recs = [], []          # recs: (qname, flag, rname, pos, ops or None)
    for name in names:
        chrom, pos, strand, rnd = S.parse_name(name)
        for e in ((0, 1) if paired else (0,)):
            flag = ((0x1 | (0x40 if e == 0 else 0x80)) if paired else 0) | (0x10 if strand[e] else 0)
            if rnd[e]:
                truth.append("\t".join([name, str(flag | 4), "*", "0", "0", "*", "*", "0", "0", "ACGT", "IIII"]))
                recs.append((name, flag, chrom, pos[e] + 1, None))
            else:
                ops = truth_cigar(rng)
                truth.append("\t".join([name, str(flag), chrom, str(pos[e] + 1), "255", text(ops), "*", "0", "0", "ACGT", "IIII"]))
                recs.append((name, flag, chrom, pos[e] + 1, ops))
    rng.shuffle(truth)        # (the index does not depend on the order)
    cnames = [c for c, _ in contigs] + [EXTRA[0]]
    lines, states = [], []

    def emit(state, qname, flag, rname, pos, cigar):
        mapq = 0 if flag & 4 else rng.choice(MAPQS + [rng.randrange(256)])
        f = [qname, str(flag), rname, str(pos), str(mapq), cigar, "=", "0", "0", "ACGT", "IIII", "AS:i:%d" % rng.randrange(0, 100), "XS:i:%d" % rng.randrange(0, 60)]
        lines.append("\t".join(f).encode())
        states.append(state)

    turn = []
    for k, (qname, flag, rname, pos, ops) in enumerate(recs):
        if ops is None:
            emit("random_mapped", qname, flag, rname, pos, "50M")
            continue
        if not turn:          # every other state once per sixteen reads, in a fresh order
            turn = [s for s in STATES if s != "random_mapped"]
            rng.shuffle(turn)
        state = turn.pop()
        cigar, p, f, rn = text(ops), pos, flag, rname
        if state == "unmapped":
            emit(state, qname, flag | 4, rname if rng.random() < 0.5 else "*", pos, "*")
            continue
        if state == "secondary":
            emit("exact", qname, flag, rname, pos, cigar)
            emit(state, qname, flag | 0x100, rname, max(1, pos + rng.randrange(-300, 300)), text(clip_ends(ops, pos, 3, 2, "H")[0]))
            continue
        if state == "unknown_name":
            uq = unknown[k % len(unknown)]
            emit(state, uq, flag, S.parse_name(uq)[0], pos, cigar)
            continue
        if state == "strand":
            f ^= 0x10
        elif state == "contig":
            rn = rng.choice([c for c in cnames if c != rname])
        elif state == "rname_star":
            rn = "*"
        elif state == "cigar_star":
            cigar = "*"
        else:
            cigar, p = perturb(rng, state, ops, pos)
        emit(state, qname, f, rn, p, cigar)
    for s in STATES:
        assert states.count(s) >= 0.05 * len(states), (s, states.count(s), len(states))
    theader = header(contigs)
    return theader + "".join(t + "\n" for t in truth).encode(), lines, states


def sam(lines, contigs=None) -> bytes:
    """an alignment file of these record lines; its @SQ list also holds a target that the truth lacks"""
    return header(list(contigs or CONTIGS) + [EXTRA]) + b"".join(l + b"\n" for l in lines)
