"""CPU-only check of dwgsim_eval-hip's truth section (dw_eval.hpp TRUTH): dw_eval.hip and dw_eval.cpp compiled against the SIMT emulation shim
(tests/emu/build_eval.sh) must give the truth section, main table, stderr and status of the plain-Python model (eval_truth_model.py) byte for
byte.  Chunks of 4096 bytes and reads of 7 and 1000 bytes, so that truth lines and records cross every kind of boundary.  Test infrastructure:
the product has no CPU path."""
import gzip, io, os, random, subprocess
import pytest

import bam_io as B
import eval_model as M
import eval_truth_cases as X
import eval_truth_model as T
from dwgsim_amd import api
from test_eval_truth_model import BAD, HEAD, tline

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
ERR_ARG, ERR_STATE, ERR_FAILED = -1, -6, -5


@pytest.fixture(scope="module")
def lib():
    subprocess.run([os.path.join(EMU, "build_eval.sh")], check=True, stdout=subprocess.DEVNULL)
    return api.load_eval(os.path.join(EMU, "libdwgsim_eval_emu.so"))


def test_error_codes():
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "dwgsim_hip.h")).read()
    for name, v in (("ARG", ERR_ARG), ("STATE", ERR_STATE), ("FAILED", ERR_FAILED)):
        assert int(hdr.split("#define DWGSIM_HIP_ERR_%s" % name)[1].split()[0]) == v


@pytest.fixture(scope="module")
def cases():
    """paired: 1 400 truth records and about 1 500 aligned ones; single: 1 000 and about 1 060"""
    out = {}
    for key, seed, n, paired in (("paired", 21, 700, True), ("single", 22, 1000, False)):
        truth, lines, states = X.make(seed, n, paired)
        out[key] = (truth, lines)
    return out


def run(lib, truth, files, chunk=4096, read=1000, bam=False, **o):
    fn = api.eval_bam if bam else api.eval_sam
    files = [B.sam_to_bam(f, block_bytes=700) for f in files] if bam else files
    return fn([io.BytesIO(f) for f in files], lib=lib, chunk_bytes=chunk, read_bytes=read, truth=None if truth is None else io.BytesIO(truth), **o)


def same(got, want):
    table, sm = got
    main, section = want
    assert (sm.status, sm.stderr, table, sm.incorrect) == (main.status, main.stderr, main.table, main.incorrect)
    assert sm.truth == section
    if main.status:
        assert (sm.error_code, sm.error_record) == (main.error_code, main.error_record)
    else:
        assert sm.n == main.n


OPTS = [{}, {"m": 1}, {"q": 20}, {"p": 1}, {"a": 3, "d": 2, "m": 1, "q": 20, "p": 1}, {"i": 1}, {"z": 1}]
RUNS = [("paired", o, 1000) for o in OPTS] + [("single", {"z": 1}, 1000), ("single", {"z": 1, "m": 1, "q": 20}, 1000), ("single", {}, 1000),
                                             ("paired", {}, 7), ("paired", {"m": 1, "p": 1}, 7), ("single", {"z": 1}, 7)]


@pytest.mark.parametrize("bam", [False, True], ids=["sam", "bam"])
@pytest.mark.parametrize("key,o,read", RUNS, ids=str)
def test_equals_the_model(lib, cases, key, o, read, bam):
    truth, lines = cases[key]
    sam = X.sam(lines)
    # (a BAM run prints -p records as it decodes them: the model reads the test decoder's text of the same file)
    want = T.run(truth, [B.bam_to_sam(B.sam_to_bam(sam, block_bytes=700)) if bam else sam], M.Opts(**o))
    assert want[0].status == (1 if bool(o.get("z")) != (key == "single") else 0)
    got = run(lib, truth, [sam], read=read, bam=bam, **o)
    same(got, want)
    if not want[0].status:
        # the section is not trivial, and nothing else moved: the run without a truth prints the same table
        assert want[1].count(b"\n") > 20 and b"## truth indel\n" in want[1]
        table, sm = run(lib, None, [sam], read=read, bam=bam, **o)
        assert (table, sm.stderr, sm.incorrect, sm.truth) == (want[0].table, want[0].stderr, want[0].incorrect, b"")


def test_two_files_with_other_target_orders(lib, cases):
    truth, lines = cases["paired"]
    half = len(lines) // 2
    a = X.sam(lines[:half], X.CONTIGS)
    b = X.sam(lines[half:], list(reversed(X.CONTIGS)))
    want = T.run(truth, [a, b])
    assert want == T.run(truth, [X.sam(lines)])         # (the order of the targets changes nothing)
    same(run(lib, truth, [a, b]), want)
    same(run(lib, truth, [a, b], bam=True), want)
    # a SAM file and a BAM file in one run
    with api.EvalContext(lib=lib, chunk_bytes=4096) as ctx:
        ctx.load_truth(io.BytesIO(truth), 333)
        head, body = M.split_header(a)
        ctx.header(head); ctx.feed(body)
        ctx.bam_begin(); ctx.feed_bam(B.sam_to_bam(b, block_bytes=900))
        same(ctx.finish(), want)
    # an alignment file whose header lacks one of the truth's contigs: its records are on "another contig"
    short = [c for c in X.CONTIGS if c[0] != "chr10"]
    c = X.header(short) + M.split_header(a)[1]
    want = T.run(truth, [c, b])
    assert want[0].status == 0 and want[1] != T.run(truth, [a, b])[1]
    same(run(lib, truth, [c, b]), want)


def test_truth_text_split_anywhere_and_gzip(lib, cases, tmp_path):
    truth, lines = cases["single"]
    sam = X.sam(lines)
    want = T.run(truth, [sam], M.Opts(z=1))
    for piece in (1, 4096, 5000):
        with api.EvalContext(lib=lib, chunk_bytes=4096, z=1) as ctx:
            head, body = M.split_header(truth)
            assert ctx.truth_header(head) == 0
            if piece == 1:
                body = body[:body.rfind(b"\n", 0, 3000) + 1]          # (byte by byte: a short truth is enough)
            for i in range(0, len(body), piece):
                assert ctx.truth_feed(body[i:i + piece]) == 0
            assert ctx.truth_commit() == 0
            ctx.header(M.split_header(sam)[0]); ctx.feed(M.split_header(sam)[1])
            if piece == 1:
                same(ctx.finish(), T.run(head + body, [sam], M.Opts(z=1)))
            else:
                same(ctx.finish(), want)
    # a last line without its newline, and a gzip file of several members
    same(run(lib, truth[:-1], [sam], z=1), want)
    path = tmp_path / "truth.sam.gz"
    path.write_bytes(gzip.compress(truth[:20000]) + gzip.compress(truth[20000:]))
    same(api.eval_sam([io.BytesIO(sam)], lib=lib, chunk_bytes=4096, truth=str(path), z=1), want)


def test_an_empty_truth_and_no_records(lib, cases):
    truth, lines = cases["paired"]
    sam = X.sam(lines[:200])
    head = M.split_header(truth)[0]
    same(run(lib, head, [sam]), T.run(head, [sam]))
    same(run(lib, b"", [sam]), T.run(b"", [sam]))
    same(run(lib, truth, [X.sam([])]), T.run(truth, [X.sam([])]))


def test_state_errors(lib, cases):
    truth, lines = cases["paired"]
    head, body = M.split_header(truth)
    shead, sbody = M.split_header(X.sam(lines[:50]))
    with api.EvalContext(lib=lib, chunk_bytes=4096) as ctx:
        assert ctx.truth_header(head) == 0 and ctx.truth_header(head) == 0 and ctx.truth_feed(body[:5000]) == 0
        assert ctx.truth_header(head) == ERR_STATE          # (the records already loaded hold contig indices of the header before)
        # a truth that is not committed refuses the alignments
        assert lib.dwgsim_hip_eval_header(ctx.ctx, shead, len(shead)) == ERR_STATE
        assert lib.dwgsim_hip_eval_bam_begin(ctx.ctx) == ERR_STATE
        assert lib.dwgsim_hip_eval_feed(ctx.ctx, sbody, len(sbody)) == ERR_STATE
        assert ctx.set_breakdown("snps") == ERR_ARG and "breakdown" in ctx.last_error()
        assert ctx.truth_feed(body[5000:]) == 0 and ctx.truth_commit() == 0
        assert ctx.truth_commit() == ERR_STATE and ctx.truth_feed(b"x") == ERR_STATE and ctx.truth_header(head) == ERR_STATE
        ctx.header(shead)
        assert ctx.truth_header(head) == ERR_STATE and ctx.truth_feed(b"x") == ERR_STATE and ctx.truth_commit() == ERR_STATE
        ctx.feed(sbody)
        same(ctx.finish(), T.run(truth, [shead + sbody]))
        assert ctx.truth_commit() == ERR_STATE
    for first in ("header", "bam_begin", "feed"):
        with api.EvalContext(lib=lib, chunk_bytes=4096) as ctx:
            ctx.header(shead) if first == "header" else ctx.bam_begin() if first == "bam_begin" else ctx.feed(sbody)
            assert ctx.truth_header(head) == ERR_STATE and ctx.truth_feed(body) == ERR_STATE and ctx.truth_commit() == ERR_STATE
            assert lib.dwgsim_hip_eval_debug_truth_slots(ctx.ctx, 12) == ERR_STATE
    with api.EvalContext(lib=lib, chunk_bytes=4096, breakdown="snps") as ctx:
        for r in (ctx.truth_header(head), ctx.truth_feed(body), ctx.truth_commit()):
            assert r == ERR_ARG and "breakdown" in ctx.last_error()
        ctx.header(shead); ctx.feed(sbody)
        table, sm = ctx.finish()
        assert sm.truth == b"" and table == M.run([shead + sbody]).table
    with pytest.raises(api.DwgsimError):
        api.eval_sam([io.BytesIO(shead + sbody)], lib=lib, truth=io.BytesIO(truth), breakdown="snps")


@pytest.mark.parametrize("line,why", BAD, ids=[str(i) for i in range(len(BAD))])
def test_a_bad_truth_is_refused_with_the_models_words(lib, line, why):
    # the good line in front fills more than one 4096-byte chunk, so that the line number counts across chunks
    pad = b"".join(tline("pad%d" % i, 0, "chr2", 9, "4M") for i in range(150))
    text = HEAD + tline("ok", 0, "chr1", 5, "4M") + line + pad + tline("later", 0, "chr1", 5, "4M")
    with pytest.raises(T.TruthError) as e:
        T.parse_truth(text)
    assert str(e.value) == why
    with api.EvalContext(lib=lib, chunk_bytes=4096) as ctx:
        head, body = M.split_header(text)
        assert ctx.truth_header(head) == 0
        r = ctx.truth_feed(body) or ctx.truth_commit()
        assert r == ERR_FAILED and ctx.last_error() == why
        assert ctx.truth_commit() == ERR_FAILED and ctx.last_error() == why
    text = HEAD + pad + tline("ok", 0, "chr1", 5, "4M") + line
    with pytest.raises(T.TruthError) as e:
        T.parse_truth(text)
    with pytest.raises(api.DwgsimError) as f:
        api.eval_sam([], lib=lib, chunk_bytes=4096, truth=io.BytesIO(text))
    assert str(f.value) == str(e.value) and ("record line 152" in str(e.value))


def test_a_bam_record_without_a_cigar_is_unusable(lib):
    """n_cigar 0 is BAM's `*`: unusable like the text, never compared"""
    name = "chr1_9_60_0_1_0_0_0:0:0_0:0:0_1"
    truth = HEAD + tline(name, 0, "chr1", 10, "10M")
    sam = HEAD + ("%s\t0\tchr1\t10\t9\t*\t=\t0\t0\tACGT\tIIII\n" % name).encode()
    want = T.run(truth, [sam], M.Opts(z=1))
    assert b"9\t0\t0\t1\t0\t" in want[1]
    for bam in (False, True):
        same(run(lib, truth, [sam], bam=bam, z=1), want)


def test_a_truth_without_a_header_holds_only_unmapped_reads(lib):
    with api.EvalContext(lib=lib) as ctx:
        assert ctx.truth_feed(tline("r", 4, "*", 0, "*")) == 0
        assert ctx.truth_feed(tline("s", 0, "chr1", 5, "4M")) == 0 and ctx.truth_commit() == ERR_FAILED
        assert ctx.last_error() == "truth: record line 2 has an RNAME that is not one of the truth's @SQ names"


def stress_truth(n):
    """n truth records and aligned records for 3 000 of them, most of them exact"""
    rng = random.Random(n)
    names = ["chr1_%d_%d_0_1_0_0_0:0:0_0:0:0_%x" % (1 + k % 900, 61 + k % 900, k) for k in range(n)]
    cig = [rng.choice(["30M", "30M", "10M2I18M", "12M3D18M"]) for _ in range(n)]
    truth = HEAD + b"".join(tline(names[k], 0, "chr1", 2 + k % 900, cig[k]) for k in range(n))
    picks = rng.sample(range(n), 3000)
    lines = [("%s\t0\tchr1\t%d\t%d\t%s\t=\t0\t0\tACGT\tIIII" % (names[k], 2 + k % 900 + (k % 7 == 0), k % 256, cig[k] if k % 5 else "30M")).encode() for k in picks]
    return truth, HEAD + b"".join(l + b"\n" for l in lines)


@pytest.mark.parametrize("apart", [False, True], ids=["round-robin", "waves-apart"])
@pytest.mark.parametrize("n", [4000, 4095])
def test_a_nearly_full_table(lib, n, apart, monkeypatch):
    """4 000 and 4 095 records in 4 096 slots: long probe chains that wrap around the end; with 4 095 one slot stays empty.  The result must
    be that of the default size, which is the model's"""
    if apart:
        monkeypatch.setenv("HIPEMU_WAVES_APART", "all")
    truth, sam = stress_truth(n)
    want = T.run(truth, [sam], M.Opts(z=1))
    assert want[0].status == 0
    got = {}
    for log2 in (None, 12):
        with api.EvalContext(lib=lib, chunk_bytes=1 << 16, z=1) as ctx:
            if log2:
                assert lib.dwgsim_hip_eval_debug_truth_slots(ctx.ctx, log2) == 0
            ctx.load_truth(io.BytesIO(truth))
            head, body = M.split_header(sam)
            ctx.header(head); ctx.feed(body)
            got[log2] = ctx.finish()
        same(got[log2], want)
    # a table without an empty slot is refused, and so is a key held twice, whatever the table's size
    with api.EvalContext(lib=lib, chunk_bytes=1 << 16, z=1) as ctx:
        assert lib.dwgsim_hip_eval_debug_truth_slots(ctx.ctx, 11) == 0
        head, body = M.split_header(truth)
        assert ctx.truth_header(head) == 0 and ctx.truth_feed(body) == 0 and ctx.truth_commit() == ERR_ARG
    twice = truth + truth.split(b"\n")[2 + 1234] + b"\n"
    with pytest.raises(T.TruthError) as e:
        T.parse_truth(twice)
    assert "line %d twice" % (n + 1) in str(e.value) and "record line 1235)" in str(e.value)
    for log2 in (None, 13):
        with api.EvalContext(lib=lib, chunk_bytes=1 << 16, z=1) as ctx:
            if log2:
                assert lib.dwgsim_hip_eval_debug_truth_slots(ctx.ctx, log2) == 0
            head, body = M.split_header(twice)
            assert ctx.truth_header(head) == 0 and ctx.truth_feed(body) == 0
            assert ctx.truth_commit() == ERR_FAILED and ctx.last_error() == str(e.value)


def test_command_line(lib, cases, tmp_path):
    truth, lines = cases["paired"]
    sam = X.sam(lines)
    a = tmp_path / "a.sam"; a.write_bytes(sam)
    t = tmp_path / "truth.sam"; t.write_bytes(truth)
    tz = tmp_path / "truth.sam.gz"; tz.write_bytes(b"".join(gzip.compress(truth[i:i + 30000]) for i in range(0, len(truth), 30000)))
    bam = tmp_path / "a.bam"; bam.write_bytes(B.sam_to_bam(sam))
    cli = os.path.join(EMU, "dwgsim_eval-emu")
    env = dict(os.environ, DWGSIM_EVAL_CHUNK="8192")
    main, section = T.run(truth, [sam], M.Opts(a=1, p=1))
    for tr, args in ((t, ["-S", str(a)]), (tz, ["-S", str(a)]), (tz, [str(bam)])):
        p = subprocess.run([cli, "-a", "1", "-p", "-T", str(tr)] + args, capture_output=True, env=env, timeout=300)
        if args[0] == "-S":
            assert (p.returncode, p.stdout, p.stderr) == (0, main.stdout + section, main.stderr)
        else:
            assert p.returncode == 0 and p.stdout.endswith(main.table + section) and p.stderr == main.stderr
    # without -T: what it printed before
    p = subprocess.run([cli, "-a", "1", "-p", "-S", str(a)], capture_output=True, env=env, timeout=300)
    assert (p.returncode, p.stdout, p.stderr) == (0, main.stdout, main.stderr)
    # a fatal record: nothing on stdout
    p = subprocess.run([cli, "-z", "-T", str(t), "-S", str(a)], capture_output=True, env=env, timeout=300)
    assert p.returncode == 1 and p.stdout == b""
    # usage errors and a bad truth
    p = subprocess.run([cli, "-T", str(t), "-B", "snps", "-S", str(a)], capture_output=True, env=env, timeout=300)
    assert p.returncode == 1 and p.stdout == b"" and b"-T and -B" in p.stderr
    p = subprocess.run([cli, "-T", str(tmp_path / "none.sam"), "-S", str(a)], capture_output=True, env=env, timeout=300)
    assert p.returncode == 1 and p.stdout == b"" and b"-T" in p.stderr
    bad = tmp_path / "bad.sam"; bad.write_bytes(truth + truth.split(b"\n")[5] + b"\n")
    p = subprocess.run([cli, "-T", str(bad), "-S", str(a)], capture_output=True, env=env, timeout=300)
    assert p.returncode == 1 and p.stdout == b"" and b"twice" in p.stderr
    cut = tmp_path / "cut.gz"; cut.write_bytes(tz.read_bytes()[:-5])
    p = subprocess.run([cli, "-T", str(cut), "-S", str(a)], capture_output=True, env=env, timeout=300)
    assert p.returncode == 1 and p.stdout == b"" and b"gzip member" in p.stderr
    p = subprocess.run([cli, "-h"], capture_output=True, env=env, timeout=300)
    assert b"-T\tFILE" in p.stderr
