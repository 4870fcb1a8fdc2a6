"""The rule of dwgsim_eval-hip's truth section (dw_eval.hpp TRUTH) pinned on hand-written cases, through the plain-Python model
(eval_truth_model.py) and through the host code itself: tests/eval_truth_main.cpp, a stand-alone program over ev::truth_compare (both record
fronts) and the gzip member reader of dw_inflate.hpp, built with -fsanitize=address,undefined."""
import gzip, os, random, subprocess
import pytest

import bam_io as B
import eval_truth_cases as X
import eval_truth_model as T

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "dwgsim_amd", "csrc")


def truth(pos1=10, cigar="5M2I3M", reverse=False, contig=b"chr1"):
    return T.TruthRec(False, contig, pos1 - 1, reverse, T.cigar_ops(cigar.encode()))


def judged(t, pos1, cigar, flag=0, rname=b"chr1"):
    outcome, c = T.judge(t, rname, flag, pos1, cigar.encode())
    return (outcome,) + tuple(c.get(k, 0) for k in ("right", "clipped", "ibases", "iright", "exact"))


# the worked cases of the rule: right clipped ibases iright exact
@pytest.mark.parametrize("pos1,cigar,flag,want", [
    (10, "10M", 0, (5, 0, 2, 0, 0)),
    (10, "5M2I3M", 0, (10, 0, 2, 2, 1)),
    (12, "2S3M2I3M", 0, (8, 2, 2, 2, 0)),
    (10, "4M2I4M", 0, (7, 0, 2, 0, 0)),
    (10, "5M2I3M", 16, (0, 0, 2, 0, 0)),
], ids=["ins-as-mismatch", "exact", "soft-clip", "ins-moved", "other-strand"])
def test_worked_cases(pos1, cigar, flag, want):
    assert judged(truth(), pos1, cigar, flag) == ("compared",) + want


# one case per rule, numbers by hand: right clipped ibases iright exact
@pytest.mark.parametrize("t,pos1,cigar,flag,rname,want", [
    (None, 10, "10M", 0, b"chr1", ("missing", 0, 0, 0, 0, 0)),
    (T.TruthRec(True), 10, "10M", 0, b"chr1", ("random", 0, 0, 0, 0, 0)),
    (truth(), 10, "*", 0, b"chr1", ("unusable", 0, 0, 0, 0, 0)),
    (truth(), 10, "10B", 0, b"chr1", ("unusable", 0, 0, 0, 0, 0)),
    (truth(), 10, "10", 0, b"chr1", ("unusable", 0, 0, 0, 0, 0)),
    (truth(), 10, "9M", 0, b"chr1", ("unusable", 0, 0, 0, 0, 0)),
    (truth(), 10, "268435456M", 0, b"chr1", ("unusable", 0, 0, 0, 0, 0)),
    # = and X are M; P does nothing
    (truth(), 10, "2=3X2I1P3=", 0, b"chr1", ("compared", 10, 0, 2, 2, 1)),
    # a hard clip consumes query positions: POS 12 after two clipped bases
    (truth(), 12, "2H3M2I3M", 0, b"chr1", ("compared", 8, 2, 2, 2, 0)),
    # clipped whatever the contig and the strand, and nothing right there
    (truth(), 12, "2S3M2I1M2H", 0, None, ("compared", 0, 4, 2, 0, 0)),
    (truth(), 12, "2S3M2I1M2H", 16, b"chr1", ("compared", 0, 4, 2, 0, 0)),
    (truth(), 10, "5M2I3M", 0, b"chr10", ("compared", 0, 0, 2, 0, 0)),
    # POS off by one: no cursor agrees, but an insertion still counts as inserted
    (truth(), 11, "5M2I3M", 0, b"chr1", ("compared", 0, 0, 2, 0, 0)),
    # N as D: truth 4M3D6M at POS 100
    (truth(100, "4M3D6M"), 100, "4M3N6M", 0, b"chr1", ("compared", 10, 0, 0, 0, 1)),
    # the deletion one base late: the base between is wrong, both sides right
    (truth(100, "4M3D6M"), 100, "5M3D5M", 0, b"chr1", ("compared", 9, 0, 0, 0, 0)),
    # a deletion missed: everything behind it is three bases off
    (truth(100, "4M3D6M"), 100, "10M", 0, b"chr1", ("compared", 4, 0, 0, 0, 0)),
    # leading and trailing insertions: I at the cursor of the first M, and of the base after the last
    (truth(50, "2I6M1I"), 50, "2I6M1I", 0, b"chr1", ("compared", 9, 0, 3, 3, 1)),
    (truth(50, "2I6M1I"), 50, "2S6M1S", 0, b"chr1", ("compared", 6, 3, 3, 0, 0)),
    (truth(50, "2I6M1I"), 48, "9M", 0, b"chr1", ("compared", 6, 0, 3, 0, 0)),
    # the reverse strand agrees with a reverse truth
    (truth(10, "10M", reverse=True), 10, "10M", 16, b"chr1", ("compared", 10, 0, 0, 0, 1)),
], ids=lambda v: None)
def test_one_case_per_rule(t, pos1, cigar, flag, rname, want):
    assert judged(t, pos1, cigar, flag, rname) == want


def test_key():
    assert T.key_of(b"r", 0) == (b"r", 0) and T.key_of(b"r", 0x40 | 0x80) == (b"r", 0)      # 0x1 clear: end 0 whatever the other bits
    assert T.key_of(b"r", 0x41) == (b"r", 1) and T.key_of(b"r", 0x81 | 0x900) == (b"r", 2)
    assert T.key_of(b"r", 0x1) is None and T.key_of(b"r", 0xC1) is None


HEAD = b"@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:chr2\tLN:1000\n"


def tline(name, flag, rname, pos, cigar):
    return ("%s\t%d\t%s\t%d\t255\t%s\t*\t0\t0\tACGT\tIIII\n" % (name, flag, rname, pos, cigar)).encode()


def aline(name, flag, rname, pos, mapq, cigar):
    return ("%s\t%d\t%s\t%d\t%d\t%s\t=\t0\t0\tACGT\tIIII\n" % (name, flag, rname, pos, mapq, cigar)).encode()


NAME = "chr1_9_60_0_1_0_0_0:0:0_0:0:0_%x"


def test_cumulative_rows_and_strata():
    tr = HEAD + tline(NAME % 1, 0x41, "chr1", 10, "5M2I3M") + tline(NAME % 1, 0x91, "chr1", 61, "10M") + tline(NAME % 2, 0x45, "*", 0, "*")
    al = (HEAD + aline(NAME % 1, 0x41, "chr1", 10, 60, "5M2I3M") + aline(NAME % 1, 0x91, "chr1", 63, 60, "2S8M") + aline(NAME % 1, 0x41, "chr1", 10, 7, "10M") +
          aline(NAME % 3, 0x41, "chr1", 10, 7, "10M") + aline(NAME % 2, 0x41, "chr1", 10, 0, "10M") + aline(NAME % 1, 0x41, "chr1", 10, 0, "*") +
          aline(NAME % 1, 0x45, "chr1", 10, 0, "10M"))
    main, text = T.run(tr, [al])
    assert main.status == 0
    assert text == (b"## truth all\n" + T.HEAD +
                    b"60\t0\t0\t0\t2\t1\t20\t18\t2\t2\t2\n"
                    b"7\t1\t0\t0\t3\t1\t30\t23\t2\t4\t2\n"
                    b"0\t1\t1\t1\t3\t1\t30\t23\t2\t4\t2\n"
                    b"## truth indel\n" + T.HEAD +
                    b"60\t0\t0\t0\t1\t1\t10\t10\t0\t2\t2\n"
                    b"7\t0\t0\t0\t2\t1\t20\t15\t0\t4\t2\n")


def test_empty_strata():
    tr = HEAD + tline(NAME % 1, 0x41, "chr1", 10, "10M")
    zeros = b"0" + b"\t0" * 10 + b"\n"
    main, text = T.run(tr, [HEAD + aline(NAME % 1, 0x45, "*", 0, 0, "*")])
    assert text == b"## truth all\n" + T.HEAD + zeros + b"## truth indel\n" + T.HEAD + zeros
    main, text = T.run(tr, [HEAD + aline(NAME % 1, 0x41, "chr1", 10, 3, "10M")])
    assert text == b"## truth all\n" + T.HEAD + b"3\t0\t0\t0\t1\t1\t10\t10\t0\t0\t0\n" + b"## truth indel\n" + T.HEAD + zeros
    # a fatal record: no section
    main, text = T.run(tr, [HEAD + aline("not_a_dwgsim_name", 0x41, "chr1", 10, 3, "10M")])
    assert main.status == 1 and text == b""


BAD = [
    (b"r\t0\tchr1\t5\t255\t4M\t*\t0\t0\tACGT\n", "truth: record line 2 has fewer than 11 fields"),
    (b"\n", "truth: record line 2 has fewer than 11 fields"),
    (tline("r", 0xC1, "chr1", 5, "4M"), "truth: record line 2 is not a truth record (QNAME, FLAG, POS or the end bits of FLAG)"),
    (tline("r", 0x1, "chr1", 5, "4M"), "truth: record line 2 is not a truth record (QNAME, FLAG, POS or the end bits of FLAG)"),
    (tline("", 0, "chr1", 5, "4M"), "truth: record line 2 is not a truth record (QNAME, FLAG, POS or the end bits of FLAG)"),
    (tline("r", 0, "chr1", 5, "4M").replace(b"\t5\t", b"\t5x\t"), "truth: record line 2 is not a truth record (QNAME, FLAG, POS or the end bits of FLAG)"),
    (tline("r", 0, "chr1", 0, "4M"), "truth: record line 2 is mapped at POS 0"),
    (tline("r", 0, "chr3", 5, "4M"), "truth: record line 2 has an RNAME that is not one of the truth's @SQ names"),
    (tline("r", 0, "*", 5, "4M"), "truth: record line 2 has an RNAME that is not one of the truth's @SQ names"),
    (tline("r", 0, "chr1", 5, "2S2M"), "truth: record line 2 has a CIGAR that is no sequence of M, I and D runs with a query base"),
    (tline("r", 0, "chr1", 5, "*"), "truth: record line 2 has a CIGAR that is no sequence of M, I and D runs with a query base"),
    (tline("r", 0, "chr1", 5, "4M0I"), "truth: record line 2 has a CIGAR that is no sequence of M, I and D runs with a query base"),
    (tline("r", 0, "chr1", 5, "4D"), "truth: record line 2 has a CIGAR that is no sequence of M, I and D runs with a query base"),
    (tline("r", 0, "chr1", 5, "4M3"), "truth: record line 2 has a CIGAR that is no sequence of M, I and D runs with a query base"),
    (tline("ok", 0, "chr2", 7, "4M"), "truth: the truth holds read of record line 2 twice (its name and end are those of record line 1)"),
]


@pytest.mark.parametrize("line,why", BAD, ids=[str(i) for i in range(len(BAD))])
def test_every_truth_error(line, why):
    good = tline("ok", 0, "chr1", 5, "4M")
    with pytest.raises(T.TruthError) as e:
        T.parse_truth(HEAD + good + line + tline("later", 0, "chr1", 5, "4M"))
    assert str(e.value) == why
    assert len(T.parse_truth(HEAD + good + tline("ok", 0x41, "chr1", 5, "4M") + tline("ok", 0x81, "*", 0, "*").replace(b"\t129\t", b"\t133\t"))) == 3


# ---- the host code, stand-alone under the sanitizers ----

@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("truth") / "eval_truth_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(HERE, "eval_truth_main.cpp"), "-o", exe], check=True)
    return exe


def test_host_compare_equals_the_model(prog, tmp_path):
    """every record of the generator's cases, and the hand-written ones above, through ev::truth_compare from the SAM and the BAM front"""
    tr, lines, states = X.make(5, 400)
    contigs = [c.encode() for c, _ in X.CONTIGS]
    targets = contigs + [X.EXTRA[0].encode()]
    ref_index = {n: i for i, n in enumerate(targets)}
    recs = T.parse_truth(tr)
    tlines = {}
    for l in tr.split(b"\n"):
        f = l.split(b"\t")
        if len(f) >= 11:
            tlines[T.key_of(f[0], int(f[1]))] = l
    cases, want = [], []
    extra = [(tline(NAME % 1, 0, "chr1", 10, "5M2I3M")[:-1], aline(NAME % 1, 0, "chr1", p, 9, c)[:-1]) for p, c in
             [(10, "10M"), (12, "2S3M2I3M"), (12, "2H3M2I3M"), (10, "2=3X2I1P3="), (10, "*"), (10, "10"), (10, "3M2I5M1D2N")]]
    pairs = [(tlines[T.key_of(l.split(b"\t")[0], int(l.split(b"\t")[1]))], l) for l in lines
             if not int(l.split(b"\t")[1]) & 4 and T.key_of(l.split(b"\t")[0], int(l.split(b"\t")[1])) in tlines]
    for tl, al in extra + pairs:
        f, g = al.split(b"\t"), tl.split(b"\t")
        flag = int(f[1])
        t = T.TruthRec(True) if int(g[1]) & 4 else T.TruthRec(False, g[2], int(g[3]) - 1, bool(int(g[1]) & 16), T.cigar_ops(g[5]))
        rname = f[2] if f[2] in contigs else None
        outcome, c = T.judge(t, rname, flag, int(f[3]), f[5])
        want.append("%s %d %d %d %d %d %d %d" % ((outcome,) + tuple(int(c.get(k, 0)) for k in ("bases", "right", "clipped", "ibases", "iright", "exact", "indel"))))
        contig = contigs.index(f[2]) if f[2] in contigs else -1
        cases.append(tl + b"|" + al + b"|" + ("%d %d " % (contig, len(targets))).encode() + B.encode_record(al, ref_index).hex().encode())
    assert len(cases) > 600 and {w.split()[0] for w in want} == {"random", "unusable", "compared"}
    path = tmp_path / "cases.txt"
    path.write_bytes(b"contigs\t" + b"\t".join(contigs) + b"\n" + b"\n".join(cases) + b"\n")
    p = subprocess.run([prog, "cmp", str(path)], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert p.stdout.decode().splitlines() == want


@pytest.mark.parametrize("members", [1, 3, 40])
def test_host_gzip_members(prog, tmp_path, members):
    """a chain of gzip members without size fields (and one with a name and a comment in its header), as dwgsim_eval-hip -T reads it"""
    tr, _, _ = X.make(6, 300)
    rng = random.Random(members)
    cuts = sorted(rng.randrange(1, len(tr) - 200) for _ in range(members - 1))
    parts = [tr[a:b] for a, b in zip([0] + cuts, cuts + [len(tr)])]
    gz = b"".join(gzip.compress(p, compresslevel=rng.choice([1, 6, 9]), mtime=0) for p in parts)
    if members == 3:
        import io
        buf = io.BytesIO()
        with gzip.GzipFile(filename="truth.sam", mode="wb", fileobj=buf, mtime=1) as f:
            f.write(parts[0])
        gz = buf.getvalue() + b"".join(gzip.compress(p, mtime=0) for p in parts[1:])
    (tmp_path / "t.gz").write_bytes(gz)
    (tmp_path / "t.sam").write_bytes(tr)
    p = subprocess.run([prog, "gz", str(tmp_path / "t.gz"), str(tmp_path / "t.sam")], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert p.stdout.decode().startswith("gz ok %d bytes, 64 cuts refused" % len(tr))
