"""The cases on which dwgsim_eval-hip, the emulated kernels and the plain-Python model (eval_model.py) are held to the UNMODIFIED reference
evaluator (oracle/_ref/dwgsim_eval: the reference's dwgsim_eval.c linked with oracle/samshim).  One list, shared by the recorder
(tests/golden/make_eval_reference_runs.py -> tests/golden/eval_reference_runs.json) and the tests (test_eval_reference.py,
test_gpu_eval_reference.py), which read the recorded answers and never need the reference.

Inputs are made again from seeds (eval_sam.py, bam_io.py) or read from the fixtures under tests/golden/eval/; the record keeps the sha256 of
each.  Only inputs on which the reference is defined are listed ("Differences from the reference, on purpose"): no -d 0, no
run in which nothing is counted (it takes log10(0)), no mapped record whose RNAME is `*` or unknown (it reads target_name[-1]), counts far
below 2^31, and no score so far from 0 that its table has 2^30 rows.

Dropped, with the reason:
  * "predicted value cannot be mapped correctly when the read is unmappable": the reference cannot reach it (dwgsim_eval.c sets both the
    actual and the predicted value from the same `1 == rand`, so an unmappable read is never "mapped correctly"); neither can the model.
"""
from __future__ import annotations
import functools, hashlib, json, os, random, re, struct

import bam_io as B
import eval_model as M
import eval_sam as S

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
RECORD = os.path.join(GOLD, "eval_reference_runs.json")
AWKWARD = os.path.join(GOLD, "eval", "awkward.sam")
REF_EVAL = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "dwgsim_eval")
CONTIGS = [("chr1", 5000), ("chr10", 3000), ("chr2_alt", 2000)]          # test_eval_emu.CONTIGS
CONTIGS_B = [("chr2_alt", 2000), ("scaffold_7:1", 4000), ("chr1", 5000)]
STORE_STDOUT = 4096


def sha256(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()


def normalize_stderr(err: bytes) -> bytes:
    """the one rule, for the reference's stderr only: its progress marks `\\r<digits>` go where another `\\r` follows at once"""
    return re.sub(rb"\r[0-9]+(?=\r)", b"", err)


def table_part(out: bytes) -> bytes:
    """stdout from the line `# thr |` on: with -p the header and the records in front of it are not compared"""
    i = out.find(b"# thr |")
    return out[i:] if i >= 0 else b""


def argv(o: dict, sam: bool) -> list:
    """the command line of an option set, for the reference and for dwgsim_eval-hip (-m takes an argument in both: getopt's `m:`)"""
    out = ["-S"] if sam else []
    for k in "adegnqs":
        if k in o:
            out += ["-" + k, str(o[k])]
    for k in "bcipz":
        if o.get(k):
            out.append("-" + k)
    if o.get("m"):
        out += ["-m", "x"]
    if o.get("P") is not None:
        out += ["-P", o["P"]]
    return out


def model_opts(o: dict) -> M.Opts:
    return M.Opts(**{k: (v.encode() if k == "P" else v) for k, v in o.items()})


def lines_of(sam: bytes):
    head, body = M.split_header(sam)
    return head, M.record_lines(body)


def join(head: bytes, lines) -> bytes:
    return head + b"".join(l + b"\n" for l in lines)


# ---- inputs ----

GOOD_PAIR = b"chr1_100_200_0_1_0_0_0:0:0_0:0:0_1"
FATAL = {          # input, options, the fatal record
    "prefix": ("prefix", {"P": "pfx"}, GOOD_PAIR + b"\t65\tchr1\t101\t60\t50M\t=\t0\t0\tA\tI"),
    "name": ("paired", {}, b"not_from_dwgsim\t65\tchr1\t100\t60\t50M\t=\t0\t0\tA\tI"),
    "contig": ("paired", {}, b"nochr_100_200_0_0_0_0_0:0:0_0:0:0_1\t65\tchr1\t100\t0\t*\t*\t0\t0\tA\tI"),
    "paired": ("single", {"z": 1}, GOOD_PAIR + b"\t65\tchr1\t101\t60\t50M\t=\t0\t0\tA\tI"),
    "not_paired": ("paired", {}, GOOD_PAIR + b"\t0\tchr1\t101\t60\t50M\t=\t0\t0\tA\tI"),
}
FATAL_CODE = {"prefix": M.E_PREFIX, "name": M.E_NAME, "contig": M.E_CONTIG, "paired": M.E_PAIRED, "not_paired": M.E_NOT_PAIRED}
FATAL_LINES = 400


def aux_records():
    """BAM records written directly: AS and XS in every integer type, `I` at and above 2^31, AS behind a B array and behind Z, H, A and f
    tags, AS:f, XS alone"""
    u = struct.pack
    front = b"ZBBs" + u("<I", 3) + u("<3h", -1, 2, 300) + b"ZZZtext\0" + b"ZHH1AE3\0" + b"ZAAq" + b"ZFf" + u("<f", 2.5)
    auxes = [
        b"ASc" + u("<b", -7) + b"XSc" + u("<b", -128), b"ASC" + u("<B", 200) + b"XSC" + u("<B", 255),
        b"ASs" + u("<h", -32768) + b"XSs" + u("<h", -300), b"ASS" + u("<H", 65535) + b"XSS" + u("<H", 40),
        b"ASi" + u("<i", -70000) + b"XSi" + u("<i", -69000), b"ASi" + u("<i", -2147483648) + b"XSi" + u("<i", -2147483648),
        b"ASI" + u("<I", 1000) + b"XSI" + u("<I", 900), b"ASI" + u("<I", 0x80000001) + b"XSI" + u("<I", 0x80000000),
        b"ASI" + u("<I", 0xFFFFFFFF) + b"XSI" + u("<I", 0xFFFFFFF0), b"ASI" + u("<I", 0x80000000) + b"XSi" + u("<i", -2147483647),
        front + b"ASC" + u("<B", 77) + b"XSc" + u("<b", 5), b"XSC" + u("<B", 9) + front + b"ASs" + u("<h", -5),
        b"ASf" + u("<f", 31.0) + b"XSC" + u("<B", 3), b"XSS" + u("<H", 500), b"ASC" + u("<B", 50), front,
        b"ZBBI" + u("<I", 2) + u("<2I", 1, 0xFFFFFFFF) + b"ZCBc" + u("<I", 0) + b"ASC" + u("<B", 12) + b"XSC" + u("<B", 2),
    ]
    out = []
    for k, aux in enumerate(auxes):
        for flag, pos, mapq in ((65, 101, 7 + k % 3), (145, 205 if k % 2 else 201, 30)):
            line = GOOD_PAIR + b"\t%d\tchr1\t%d\t%d\t3S47M\t=\t0\t0\tACGT\tIIII" % (flag, pos + 3, mapq)
            rec = B.encode_record(line, {b"chr1": 0, b"chr10": 1, b"chr2_alt": 2}) + aux
            out.append(struct.pack("<I", len(rec) - 4) + rec[4:])
    return out


@functools.lru_cache(maxsize=None)
def inputs() -> dict:
    """name -> bytes of every input file of the recorded runs (SAM text or BAM)"""
    rng = random.Random(11)          # the inputs of test_eval_emu.py, in its order
    d = {"paired": S.sam_file(rng, CONTIGS, 1200), "paired2": S.sam_file(rng, CONTIGS, 300),
         "single": S.sam_file(rng, CONTIGS, 900, paired=False), "prefix": S.sam_file(rng, CONTIGS, 800, prefix="pfx"),
         "wide": S.sam_file(rng, CONTIGS, 600, wide_scores=True)}
    # several files: another @SQ list, and a file that begins with the last record of "paired2" and ends with its first (-m across files)
    d["other_sq"] = S.sam_file(random.Random(12), CONTIGS_B, 400)
    head, lines = lines_of(d["paired2"])
    d["straddle"] = join(head, [lines[-1]] + lines[:100] + [lines[0]])
    for key, (src, _, bad) in FATAL.items():
        head, lines = lines_of(d[src])
        lines = lines[:FATAL_LINES]
        for where, k in (("first", 0), ("middle", FATAL_LINES // 2 + 1), ("last", FATAL_LINES)):
            d["fatal_%s_%s" % (key, where)] = join(head, lines[:k] + [bad] + lines[k:])
    for name in ("paired", "single", "prefix", "wide"):
        for blk in (700, 5000, 65280):
            d["%s_b%d.bam" % (name, blk)] = B.sam_to_bam(d[name], block_bytes=blk)
    d["paired2.bam"] = B.sam_to_bam(d["paired2"], block_bytes=5000)
    d["straddle.bam"] = B.sam_to_bam(d["straddle"], block_bytes=700)
    head, lines = lines_of(d["paired2"])
    payload, offs = B.bam_payload(join(head, lines[:60]))
    recs = aux_records()
    d["aux.bam"] = B.bgzf(payload[:offs[30]] + b"".join(recs) + payload[offs[30]:], 700)
    return d


def is_bam(name: str) -> bool:
    return name.endswith(".bam")


@functools.lru_cache(maxsize=None)
def model_text(name: str) -> bytes:
    """what the model reads for an input: the SAM text itself, or the text that the test's own decoder makes of the BAM bytes"""
    data = inputs()[name]
    return B.bam_to_sam(data) if is_bam(name) else data


def true_n(sam: bytes, paired: bool) -> int:
    """the reference's n without -m: first ends of pairs, or every record of single-end input"""
    _, lines = lines_of(sam)
    return sum(1 for l in lines if not paired or int(l.split(b"\t")[1]) & 0x40)


# ---- the runs ----

OPTS = [{}, {"a": 1}, {"a": 2}, {"a": 3}, {"a": 0, "d": 3}, {"a": 3, "d": 3}, {"g": 0}, {"g": 5, "a": 1, "d": 3}, {"q": 20}, {"m": 1},
        {"m": 1, "p": 1, "q": 10}, {"i": 1}, {"e": 1}, {"s": 0}, {"e": 0, "s": 1}, {"i": 1, "e": 2}, {"p": 1}, {"n": 12345},
        {"b": 1, "c": 1}]          # test_gpu_eval.OPTS
MORE_OPTS = [{"d": -2}, {"d": 7, "g": -1}, {"a": 0, "d": 300}, {"q": 255}, {"b": 1}, {"c": 1}, {"a": 3, "d": -2}, {"a": 1, "e": 1, "b": 1, "c": 1}]
SYNTH = {"paired": {}, "single": {"z": 1}, "prefix": {"P": "pfx"}, "wide": {}}
BAM_OPTS = [{}, {"a": 3, "m": 1, "p": 1}, {"a": 1, "d": 3, "q": 20}]


def opt_id(o: dict) -> str:
    return "_".join("%s%s" % (k, v) for k, v in o.items()) or "default"


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    """id -> {"files": [input names], "opts": {...}, "fatal": key or None}"""
    out = {}

    def add(cid, files, o, fatal=None):
        assert cid not in out, cid
        out[cid] = {"files": list(files), "opts": dict(o), "fatal": fatal}

    for name, base in SYNTH.items():
        sets = OPTS + MORE_OPTS + [{"n": true_n(inputs()[name], name != "single")}]
        for o in sets:
            add("synth/%s/%s" % (name, opt_id(o)), [name], dict(base, **o))
    add("multi/other_sq", ["paired", "other_sq", "paired2"], {"a": 3})
    add("multi/other_sq_p", ["other_sq", "paired"], {"p": 1, "a": 1, "d": 3})
    add("multi/straddle_m", ["paired2", "straddle", "paired2"], {"m": 1, "p": 1})
    add("multi/straddle_no_m", ["paired2", "straddle", "paired2"], {"p": 1})
    add("multi/three", ["paired", "paired2", "paired"], {"m": 1, "p": 1, "a": 3})
    for key, (_, o, _) in FATAL.items():
        for where in ("first", "middle", "last"):
            add("fatal/%s/%s" % (key, where), ["fatal_%s_%s" % (key, where)], o, fatal=key)
    for name, base in SYNTH.items():
        for blk in (700, 5000, 65280):
            for o in BAM_OPTS:
                add("bam/%s_b%d/%s" % (name, blk, opt_id(o)), ["%s_b%d.bam" % (name, blk)], dict(base, **o))
    for o in ({"a": 1}, {"a": 2}, {"a": 3}, {"a": 3, "d": 2, "p": 1}, {}):
        add("bam/aux/%s" % opt_id(o), ["aux.bam"], o)
    add("bam/straddle_m", ["paired2.bam", "straddle.bam"], {"m": 1, "p": 1})
    return out


# ---- single-record runs on awkward names ----

SINGLE_OPTS = {"default": {}, "a3_d2": {"a": 3, "d": 2}, "i": {"i": 1}, "e1": {"e": 1}}
AWK_CONTIGS = CONTIGS + [("HLA:A_01:02", 3000), ("a_b:c", 1000), ("chr1_100", 500)]


def awkward_names():
    def nm(c="chr1", p1="100", p2="300", s1="0", s2="1", r1="0", r2="0", e1="1", u1="0", i1="0", e2="2", u2="1", i2="1", idx="1f"):
        return "%s_%s_%s_%s_%s_%s_%s_%s:%s:%s_%s:%s:%s_%s" % (c, p1, p2, s1, s2, r1, r2, e1, u1, i1, e2, u2, i2, idx)
    out = []
    # contig names with _ and : in them; a target that is a prefix of the name's contig, and the other way round; unknown contigs
    out += [nm(c=c) for c in ("chr1", "chr10", "chr2_alt", "HLA:A_01:02", "a_b:c", "chr1_100", "chr1x", "chr100", "chr", "ch", "c", "chr2",
                              "chr2_al", "chr2_alt_x", "HLA:A", "a_b", "nochr", "1", "_", ":")]
    # a trailing /1, /2 or _x
    out += [nm(c=c) + t for c in ("chr1", "chr2_alt") for t in ("/1", "/2", "_x", "_x/1", "_", ":0")]
    # %1d fields
    out += [nm(s1=v) for v in ("-1", "+3", "12", "01", "2", "9", "1")] + [nm(s2=v) for v in ("-0", "10", "0")]
    out += [nm(r1=v) for v in ("-1", "+1", "12", "01", "2", "1")] + [nm(r2=v) for v in ("1", "11", "2")] + [nm(r1="1", r2="1")]
    # %d fields at the edges of int and long
    wide = (str(2**31 - 1), str(2**31), str(2**32 + 1), str(-2**31 - 1), "12345678901234567890", "-99999999999999999999",
            str(2**63 - 1), str(2**63), str(2**32 + 100), str(2**32 + 300))
    out += [nm(p1=v) for v in wide] + [nm(p2=v) for v in wide[:4] + wide[8:]]
    out += [nm(e1=v) for v in (str(2**32 + 1), str(2**31), "-1", "01", "+1", "3", "0")]
    out += [nm(u1=v) for v in (str(2**32), "00", "-0")] + [nm(i1=v) for v in (str(2**32), str(2**32 + 1), "00", "1", "-1")]
    out += [nm(i2=v) for v in (str(2**32), "0", "7")] + [nm(e2=v) for v in ("1", str(2**32 + 1))]
    # leading zeros and signs
    out += [nm(p1=v) for v in ("007", "0100", "+100", "-0", "-100", "00000000000000000000100")] + [nm(p2="0300"), nm(p2="+300")]
    # blanks inside the name
    out += ["chr1 _100_300_0_1_0_0_1:0:0_2:1:1_1f", "chr1_100 _300_0_1_0_0_1:0:0_2:1:1_1f", " chr1_100_300_0_1_0_0_1:0:0_2:1:1_1f",
            "chr1_100_300_0_1_0_0_1:0:0_2:1:1_ab cd", "chr1_100_300_0_1_0_0_1:0:0_2:1:1_ ", "chr1_1 0_300_0_1_0_0_1:0:0_2:1:1_1f",
            "chr1 100 300 0 1 0 0 1 0 0 2 1 1 1f", "chr 1_100_300_0_1_0_0_1:0:0_2:1:1_1f"]
    # too few or too many fields, other separators
    out += ["chr1_100_300_0_1_0_0_1:0:0_2:1:1", "chr1_100_300_0_1_0_0_1:0:0_2:1:1_", "chr1_100", "x", "chr1_100_300_0_1_0_0_1_0_0_2_1_1_1f",
            "chr1:100:300:0:1:0:0:1:0:0:2:1:1:1f", "chr1_100_300_0_1_0_0_1:0:0_2:1:1_1f_1:0:0_2:1:1_2e", "chr1_100_300_0_1_0_0_a:0:0_2:1:1_1f",
            "chr1_100_300_0_1_0_0_1:0:0_2:1:x_1f", "chr1__300_0_1_0_0_1:0:0_2:1:1_1f", "_100_300_0_1_0_0_1:0:0_2:1:1_1f"]
    assert len(set(out)) == len(out)
    return out


AWK_TAILS = [          # FLAG RNAME POS MAPQ CIGAR, then the tags (names say pos 100 forward for the first end, 300 reverse for the second)
    "65\tchr1\t101\t3\t50M\t=\t0\t0\tACGT\tIIII\tAS:i:40\tXS:i:10",
    "145\tchr1\t301\t3\t50M\t=\t0\t0\tACGT\tIIII\tXS:i:3\tAS:i:9",
    "65\tchr1\t1\t2\t2H3S45M\t=\t0\t0\tACGT\tIIII\tAS:i:4\tXS:i:6",                    # POS 1 and 5 clipped: left is -5
    "65\tchr1\t106\t1\t45M5S\t=\t0\t0\tACGT\tIIII\tAS:i:7",                             # a trailing clip only: left is 105
    "69\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII",                                              # unmapped
    "81\tchr2_alt\t95\t4\t*\t=\t0\t0\tACGT\tIIII\tAS:i:30\tXS:i:30",                    # mapped, CIGAR *
    "65\tHLA:A_01:02\t107\t1\t50M\t=\t0\t0\tACGT\tIIII\tAS:i:3\tXS:i:1",                # left is 106: one past -g
    "129\ta_b:c\t297\t2\t1S1H48M\t=\t0\t0\tACGT\tIIII\tAS:i:12\tXS:i:-4",
]
AWK_SCORES = [          # AS, XS on a well-named record: near +-2^15 and +-2^31, and such that AS - XS wraps (to a small number)
    ("32767", "32766"), ("32768", "32767"), ("-32768", "-32769"), ("-32769", "-32768"), ("65535", "65536"), ("65536", "65535"),
    ("2147483647", "2147483646"), ("2147483648", "2147483647"), ("4294967295", "4294967294"), ("-2147483648", "2147483647"),
    ("2147483647", "-2147483648"), ("4294967296", "0"), ("-2147483648", "-2147483647"), ("-100000", "0"), ("32767", "-32768"),
    ("-2147483649", "2147483646"), ("9223372036854775807", "-2"), ("-9223372036854775808", "1"),
]


ANCHOR = b"chr10_50_150_0_1_0_0_1:0:1_1:0:1_a0\t65\tchr10\t51\t5\t50M\t=\t0\t0\tACGT\tIIII\tAS:i:20\tXS:i:10"


def single_input(k: int) -> bytes:
    """the input of single-record run k: the header, ANCHOR (a plain record that every option set of SINGLE_OPTS counts, so that the table is
    defined when a filter drops the awkward record) and record k of the fixture"""
    head, lines = awkward()
    return join(head, [ANCHOR, lines[k]])


def awkward_sam() -> bytes:
    """the text of tests/golden/eval/awkward.sam (the recorder writes it; the tests read the committed file): every name with half of the
    tails, alternating"""
    lines = [(n + "\t" + t) for k, n in enumerate(awkward_names()) for j, t in enumerate(AWK_TAILS) if (k + j) % 2 == 0]
    good = "chr1_100_300_0_1_0_0_1:0:0_2:1:1_1f"
    lines += ["%s\t65\tchr1\t101\t3\t50M\t=\t0\t0\tACGT\tIIII\tAS:i:%s\tXS:i:%s" % (good, a, x) for a, x in AWK_SCORES]
    lines += [good + "\t65\tchr1\t101\t3\t50M\t=\t0\t0\tACGT\tIIII\t" + t for t in ("AS:f:3.5\tXS:i:1", "XS:i:5", "AS:Z:12\tXS:A:3", "NM:i:1")]
    return S.header(AWK_CONTIGS) + "".join(l + "\n" for l in lines).encode()


@functools.lru_cache(maxsize=None)
def awkward():
    """(header, record lines) of the committed fixture"""
    with open(AWKWARD, "rb") as f:
        return lines_of(f.read())


def single_ids():
    n = len(awkward()[1])
    return ["single/%s/%d" % (name, k) for name in SINGLE_OPTS for k in range(n)]


# ---- the record ----

@functools.lru_cache(maxsize=None)
def record() -> dict:
    with open(RECORD) as f:
        return json.load(f)


def recorded(cid: str) -> dict:
    """the reference's answer on a case: rc, stderr, and unless the run was fatal stdout_sha256, stdout_len and, when short, stdout"""
    r = record()
    if cid.startswith("single/"):
        _, name, k = cid.split("/")
        return r["single"]["answers"][r["single"]["index"][name][int(k)]]
    return r["runs"][cid]


def first_difference(want: bytes, got: bytes) -> str:
    a, b = want.split(b"\n"), got.split(b"\n")
    for k in range(max(len(a), len(b))):
        x = a[k] if k < len(a) else None; y = b[k] if k < len(b) else None
        if x != y:
            return "line %d: expected %r, got %r" % (k + 1, x, y)
    return "no difference"


def check_answer(cid: str, rec: dict, status: int, stderr: bytes, table: bytes, model_table=None):
    """status, stderr and table (stdout from `# thr |` on) of one run against the recorded answer of the reference"""
    assert status == rec["rc"], (cid, status, rec["rc"])
    assert stderr == rec["stderr"].encode("latin-1"), (cid, stderr, rec["stderr"])
    if rec["rc"]:
        assert table == b"", cid          # on a fatal record nothing goes to our stdout, on purpose
        return
    if (sha256(table), len(table)) != (rec["stdout_sha256"], rec["stdout_len"]):
        want = rec["stdout"].encode("latin-1") if "stdout" in rec else model_table() if model_table else None
        why = first_difference(want, table) if want is not None else ""
        raise AssertionError("%s: the table differs from the reference's (%d bytes, recorded %d): %s" % (cid, len(table), rec["stdout_len"], why))
    if "stdout" in rec:
        assert table == rec["stdout"].encode("latin-1"), cid
