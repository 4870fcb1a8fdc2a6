"""Test-only SAM writer for the dwgsim_eval tests: a seeded stand-in for an aligner.  It places each read where its dwgsim name says and then
perturbs the records (strand flips, wrong contigs, position offsets around -g, soft / hard clips, unmapped records, random MAPQ, AS / XS tags of
several types, runs of multi-mapped duplicates, names with and without /1), so that every class and option of dwgsim_eval is exercised."""
from __future__ import annotations
import random

def dwgsim_name(chrom, p1, p2, s1, s2, r1, r2, e1, u1, i1, e2, u2, i2, idx, prefix=None):
    core = "%s_%d_%d_%d_%d_%d_%d_%d:%d:%d_%d:%d:%d_%x" % (chrom, p1, p2, s1, s2, r1, r2, e1, u1, i1, e2, u2, i2, idx)
    return (prefix + "_" + core) if prefix else core


def synth_names(rng: random.Random, contigs, n, prefix=None, rand_frac=0.1):
    """names of n simulated reads (pairs) in dwgsim's format: contigs is [(name, length)]"""
    out = []
    for k in range(n):
        c, l = rng.choice(contigs)
        r = 1 if rng.random() < rand_frac else 0
        p1 = rng.randrange(1, max(2, l - 300)); p2 = p1 + rng.randrange(0, 300)
        out.append(dwgsim_name(c, p1, p2, rng.randrange(2), rng.randrange(2), r, r, rng.randrange(4), rng.randrange(3), rng.randrange(2),
                               rng.randrange(4), rng.randrange(3), rng.randrange(2), k, prefix))
    return out


def parse_name(name: str, prefix=None):
    """(chrom, [p1, p2], [s1, s2], [r1, r2]) of a dwgsim name (the test writer's own inverse, not the evaluator's)"""
    if prefix:
        name = name[len(prefix) + 1:]
    parts = name.rsplit("_", 9)
    chrom = parts[0]
    p1, p2, s1, s2, r1, r2 = (int(x) for x in parts[1:7])
    return chrom, [p1, p2], [s1, s2], [r1, r2]


def header(contigs) -> bytes:
    h = "@HD\tVN:1.0\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (c, l) for c, l in contigs) + "@PG\tID:fake\tPN:fake\n"
    return h.encode()


def _aux(rng, a_val, x_val):
    tags = []
    kind = rng.random()
    if kind < 0.8:
        tags.append("AS:i:%d" % a_val)
    elif kind < 0.87:
        tags.append("AS:f:%d.5" % a_val)          # not an integer: counts 0
    elif kind < 0.92:
        tags.append("AS:Z:x%d" % a_val)
    # else: no AS tag
    kind = rng.random()
    if kind < 0.75:
        tags.append("XS:i:%d" % x_val)
    elif kind < 0.8:
        tags.append("XS:A:q")
    rng.shuffle(tags)
    return tags


def records(rng: random.Random, names, contigs, paired=True, prefix=None, g=5, dup_frac=0.05, slash_frac=0.3, wide_scores=False):
    """SAM record lines (bytes, no newline) for the reads `names`"""
    cnames = [c for c, _ in contigs]
    out = []
    for name in names:
        chrom, pos, strand, rnd = parse_name(name, prefix)
        ends = (0, 1) if paired else (0,)
        for e in ends:
            qname = name + ("/%d" % (e + 1) if rng.random() < slash_frac else "")
            flag = (0x1 | (0x40 if e == 0 else 0x80)) if paired else 0
            reps = 1 + (rng.randrange(1, 4) if rng.random() < dup_frac else 0)
            for _ in range(reps):
                f = flag
                rname, p, st = chrom, pos[e], strand[e]
                u = rng.random()
                clip = ""
                if u < 0.1:
                    f |= 0x4
                elif u < 0.15:
                    st ^= 1
                elif u < 0.2:
                    rname = rng.choice(cnames)
                elif u < 0.45:
                    p += rng.choice([-g - 1, -g, -g + 1, g - 1, g, g + 1, 0, 50])
                if rng.random() < 0.2:
                    clip = "%d%s" % (rng.randrange(1, 6), rng.choice("SH"))
                    if rng.random() < 0.3:
                        clip += "%dS" % rng.randrange(1, 3)
                if f & 0x4:
                    line = [qname, str(f | (0x10 if st else 0)), "*" if rng.random() < 0.5 else rname, "0" if rng.random() < 0.5 else str(max(1, p)), "0", "*"]
                else:
                    # POS is 1-based: the evaluator compares pos with POS - 1 - clips
                    sam_pos = max(1, p + 1 + _clip_len(clip))
                    line = [qname, str(f | (0x10 if st else 0)), rname, str(sam_pos), str(rng.choice([0, 0, 1, 3, 17, 37, 60, 254, 255, rng.randrange(256)])),
                            (clip + "50M") if clip else rng.choice(["50M", "20M1I29M", "50M2S"])]
                line += ["=", "0", "0", "ACGT", "IIII"]
                # wide: scores far outside the kernel's LDS window (its spill list), but not so far apart that the table has millions of rows
                av = rng.randrange(-40, 160) if not wide_scores else rng.randrange(-12000, 12000)
                xv = rng.randrange(-10, av + 20 if av > -10 else 30) if not wide_scores else rng.randrange(-12000, 12000)
                line += _aux(rng, av, xv)
                if rng.random() < 0.3:
                    line.append("NM:i:%d" % rng.randrange(5))
                out.append("\t".join(line).encode())
    return out


def _clip_len(clip: str) -> int:
    n = 0; num = ""
    for ch in clip:
        if ch.isdigit():
            num += ch
        else:
            if ch in "SH":
                n += int(num)
            num = ""
    return n


def sam_file(rng, contigs, n, paired=True, prefix=None, **kw) -> bytes:
    names = synth_names(rng, contigs, n, prefix)
    return header(contigs) + b"".join(l + b"\n" for l in records(rng, names, contigs, paired, prefix, **kw))
