"""The truth section of dwgsim_eval-hip (dw_eval.hpp TRUTH) on the MI355X against the plain-Python model (eval_truth_model.py), byte for byte:
the cases of tests/test_eval_truth_emu.py through the product library and dwgsim_eval-hip -T, plain and gzipped truth, at 4 KiB chunks and at
the default chunk size; the nearly full index; the loop closed with dwgsim-hip's own truth SAM; and a truth larger than one chunk."""
import gzip, io, os, random, subprocess
import pytest

import bam_io as B
import eval_model as M
import eval_truth_cases as X
import eval_truth_model as T
from dwgsim_amd import api
from hapfasta_common import synth
from test_eval_truth_emu import ERR_ARG, ERR_FAILED, same, stress_truth
from test_eval_truth_model import BAD, HEAD, tline

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dwgsim_amd", "dwgsim_eval-hip")
SIM = os.path.join(ROOT, "dwgsim_amd", "dwgsim-hip")
CHUNKS = [4096, 0]


@pytest.fixture(scope="module")
def cases():
    out = {}
    for key, seed, n, paired in (("paired", 21, 700, True), ("single", 22, 1000, False)):
        truth, lines, _ = X.make(seed, n, paired)
        out[key] = (truth, X.sam(lines))
    return out


def run(truth, files, chunk, bam=False, **o):
    fn = api.eval_bam if bam else api.eval_sam
    files = [B.sam_to_bam(f, block_bytes=3000) for f in files] if bam else files
    return fn([io.BytesIO(f) for f in files], chunk_bytes=chunk, read_bytes=1 << 16, truth=None if truth is None else io.BytesIO(truth), **o)


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("bam", [False, True], ids=["sam", "bam"])
@pytest.mark.parametrize("key,o", [("paired", {}), ("paired", {"m": 1}), ("paired", {"q": 20}), ("paired", {"a": 3, "d": 2, "m": 1, "q": 20, "p": 1}),
                                   ("paired", {"i": 1}), ("paired", {"z": 1}), ("single", {"z": 1}), ("single", {"z": 1, "m": 1, "p": 1})], ids=str)
def test_gpu_equals_the_model(cases, key, o, bam, chunk):
    truth, sam = cases[key]
    want = T.run(truth, [B.bam_to_sam(B.sam_to_bam(sam, block_bytes=3000)) if bam else sam], M.Opts(**o))
    same(run(truth, [sam], chunk, bam, **o), want)
    if not want[0].status:
        table, sm = run(None, [sam], chunk, bam, **o)
        assert (table, sm.stderr, sm.incorrect, sm.truth) == (want[0].table, want[0].stderr, want[0].incorrect, b"")


@pytest.mark.parametrize("chunk", CHUNKS)
def test_gpu_two_files_with_other_target_orders(cases, chunk):
    truth, sam = cases["paired"]
    head, body = M.split_header(sam)
    lines = M.record_lines(body)
    a = X.sam(lines[:len(lines) // 2], X.CONTIGS)
    b = X.sam(lines[len(lines) // 2:], list(reversed(X.CONTIGS)))
    want = T.run(truth, [a, b])
    same(run(truth, [a, b], chunk), want)
    with api.EvalContext(chunk_bytes=chunk) as ctx:
        ctx.load_truth(io.BytesIO(gzip.compress(truth)))
        ctx.header(M.split_header(a)[0]); ctx.feed(M.split_header(a)[1])
        ctx.bam_begin(); ctx.feed_bam(B.sam_to_bam(b, block_bytes=900))
        same(ctx.finish(), want)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_gpu_command_line(cases, tmp_path, chunk):
    truth, sam = cases["paired"]
    a = tmp_path / "a.sam"; a.write_bytes(sam)
    t = tmp_path / "truth.sam"; t.write_bytes(truth)
    tz = tmp_path / "truth.sam.gz"; tz.write_bytes(b"".join(gzip.compress(truth[i:i + 30000]) for i in range(0, len(truth), 30000)))
    env = dict(os.environ)
    env.pop("DWGSIM_EVAL_CHUNK", None)
    if chunk:
        env["DWGSIM_EVAL_CHUNK"] = str(chunk)
    main, section = T.run(truth, [sam], M.Opts(a=1, p=1))
    for tr in (t, tz):
        p = subprocess.run(["timeout", "-k", "10", "120", CLI, "-a", "1", "-p", "-T", str(tr), "-S", str(a)], capture_output=True, env=env, timeout=140)
        assert (p.returncode, p.stdout, p.stderr) == (0, main.stdout + section, main.stderr)
    p = subprocess.run(["timeout", "-k", "10", "120", CLI, "-a", "1", "-p", "-S", str(a)], capture_output=True, env=env, timeout=140)
    assert (p.returncode, p.stdout, p.stderr) == (0, main.stdout, main.stderr)


@pytest.mark.parametrize("chunk", CHUNKS + [1 << 16])
@pytest.mark.parametrize("n", [4000, 4095])
def test_gpu_a_nearly_full_table(n, chunk):
    lib = api.load()
    truth, sam = stress_truth(n)
    want = T.run(truth, [sam], M.Opts(z=1))
    for log2 in (None, 12):
        with api.EvalContext(chunk_bytes=chunk, z=1) as ctx:
            if log2:
                assert lib.dwgsim_hip_eval_debug_truth_slots(ctx.ctx, log2) == 0
            ctx.load_truth(io.BytesIO(truth))
            head, body = M.split_header(sam)
            ctx.header(head); ctx.feed(body)
            same(ctx.finish(), want)
    twice = truth + truth.split(b"\n")[2 + 1234] + b"\n"
    with pytest.raises(T.TruthError) as e:
        T.parse_truth(twice)
    with api.EvalContext(chunk_bytes=chunk, z=1) as ctx:
        assert lib.dwgsim_hip_eval_debug_truth_slots(ctx.ctx, 13) == 0
        head, body = M.split_header(twice)
        assert ctx.truth_header(head) == 0 and ctx.truth_feed(body) == 0
        assert ctx.truth_commit() == ERR_FAILED and ctx.last_error() == str(e.value)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_gpu_a_bad_truth_is_refused_with_the_models_words(chunk):
    """every kind of bad truth line through the device's own parse: the first bad line of the truth decides, counted across chunks (at 4096
    the lines in front of it fill two chunks), and the truth calls stay refused afterwards"""
    pad = b"".join(tline("pad%d" % i, 0, "chr2", 9, "4M") for i in range(150))
    for line, why in BAD:
        # (a second bad line behind it does not matter; a repeated key is only looked for once every line is good)
        text = HEAD + pad + tline("ok", 0, "chr1", 5, "4M") + line + tline("later", 0, "chr1", 5 if "twice" in why else 0, "4M")
        with pytest.raises(T.TruthError) as e:
            T.parse_truth(text)
        assert "record line 152" in str(e.value) and str(e.value) == why.replace("line 2", "line 152").replace("line 1)", "line 151)")
        with api.EvalContext(chunk_bytes=chunk) as ctx:
            head, body = M.split_header(text)
            assert ctx.truth_header(head) == 0
            r = ctx.truth_feed(body) or ctx.truth_commit()
            assert r == ERR_FAILED and ctx.last_error() == str(e.value), line
            assert ctx.truth_commit() == ERR_FAILED and ctx.truth_feed(b"x") == ERR_FAILED and ctx.last_error() == str(e.value)
            assert ctx.lib.dwgsim_hip_eval_header(ctx.ctx, head, len(head)) == -6        # DWGSIM_HIP_ERR_STATE: the truth is not committed
    # a good truth of the same shape passes, and a header after the first record text is refused
    with api.EvalContext(chunk_bytes=chunk) as ctx:
        assert ctx.truth_header(HEAD) == 0 and ctx.truth_header(HEAD) == 0 and ctx.truth_feed(pad) == 0
        assert ctx.truth_header(HEAD) == -6 and ctx.truth_commit() == 0


def test_gpu_a_bam_record_without_a_cigar_is_unusable():
    """n_cigar 0 is BAM's `*`: unusable like the text, never compared"""
    name = "chr1_9_60_0_1_0_0_0:0:0_0:0:0_1"
    truth = HEAD + tline(name, 0, "chr1", 10, "10M")
    sam = HEAD + ("%s\t0\tchr1\t10\t9\t*\t=\t0\t0\tACGT\tIIII\n" % name).encode()
    want = T.run(truth, [sam], M.Opts(z=1))
    assert b"9\t0\t0\t1\t0\t" in want[1]
    for bam in (False, True):
        same(run(truth, [sam], 0, bam, z=1), want)


# ---- the loop closed: dwgsim-hip's truth SAM as the truth and as the alignments ----
INDELS = "-r 0.02 -R 0.3 -X 0.5 -1 50 -2 50"       # (the indel run of tests/test_gpu_truth_sam.py, at 2 x 50)


def last_rows(section: bytes):
    """{stratum: the counts of its last row, which hold everything}"""
    out = {}
    for line in section.decode().splitlines():
        if line.startswith("## truth "):
            key = line[9:]
        elif not line.startswith("#"):
            out[key] = dict(zip(["mapq"] + T.COLS, (int(x) for x in line.split("\t"))))
    return out


def all_m(sam: bytes) -> bytes:
    """every mapped record's CIGAR as <query length>M at the same POS"""
    head, body = M.split_header(sam)
    out = []
    for line in M.record_lines(body):
        f = line.split(b"\t")
        if not int(f[1]) & 4:
            f[5] = b"%dM" % sum(n for n, op in T.cigar_ops(f[5]) if op in "MI")
        out.append(b"\t".join(f))
    return head + b"".join(l + b"\n" for l in out)


@pytest.mark.parametrize("kind", ["pairs", "single"])
def test_gpu_the_truth_scored_against_itself(kind, tmp_path):
    contigs = [("loop", synth(91, 9000))]
    flags = "-z 47 -N 2000 " + INDELS + (" -2 0" if kind == "single" else "")
    res = api.run_job(api.parse_flags(flags), contigs, truth_sam=True)
    truth = api.truth_sam_header(contigs) + res.truth_sam
    o = {"z": 1} if kind == "single" else {}
    assert len(M.record_lines(res.truth_sam)) == (2000 if kind == "single" else 4000)
    table, sm = api.eval_sam([io.BytesIO(truth)], truth=io.BytesIO(truth), **o)
    assert sm.status == 0, sm.stderr
    rows = last_rows(sm.truth)
    a, i = rows["all"], rows["indel"]
    assert a["compared"] == a["exact"] > 0 and a["right"] == a["bases"] > 0 and a["iright"] == a["ibases"] > 0
    assert a["missing"] == a["random"] == a["unusable"] == a["clipped"] == 0
    assert 0 < i["compared"] == i["exact"] < a["compared"] and i["ibases"] == a["ibases"]
    same((table, sm), T.run(truth, [truth], M.Opts(**o)))
    # every CIGAR as one M run at the same POS: what an aligner without gaps would report
    flat = all_m(truth)
    want = T.run(truth, [flat], M.Opts(**o))
    got = api.eval_sam([io.BytesIO(flat)], truth=io.BytesIO(truth), chunk_bytes=1 << 16, **o)
    same(got, want)
    f = last_rows(got[1].truth)["all"]
    assert f["compared"] == a["compared"] and f["exact"] < a["exact"] and f["right"] < f["bases"] and f["iright"] == 0 < f["ibases"]


def test_gpu_the_simulators_own_truth_file(tmp_path):
    """out.truth.sam.gz as DWGSIM_HIP_TRUTH_SAM=1 dwgsim-hip wrote it, given to -T as it is"""
    contigs = [("loop", synth(91, 9000))]
    fa = tmp_path / "in.fa"
    s = bytes(bytearray(contigs[0][1])).decode()
    fa.write_text(">loop\n" + "".join(s[i:i + 70] + "\n" for i in range(0, len(s), 70)))
    env = dict(os.environ, DWGSIM_HIP_TRUTH_SAM="1")
    subprocess.run(["timeout", "-k", "10", "120", SIM] + ("-z 47 -N 2000 " + INDELS).split() + [str(fa), str(tmp_path / "out")], check=True,
                   stderr=subprocess.DEVNULL, env=env, timeout=140)
    tz = tmp_path / "out.truth.sam.gz"
    truth = gzip.decompress(tz.read_bytes())
    flat = tmp_path / "flat.sam"; flat.write_bytes(all_m(truth))
    main, section = T.run(truth, [all_m(truth)])
    env = {k: v for k, v in os.environ.items() if k != "DWGSIM_EVAL_CHUNK"}
    p = subprocess.run(["timeout", "-k", "10", "120", CLI, "-T", str(tz), "-S", str(flat)], capture_output=True, env=env, timeout=140)
    assert (p.returncode, p.stdout, p.stderr) == (0, main.table + section, main.stderr)
    assert last_rows(section)["indel"]["compared"] > 0


def test_gpu_a_truth_larger_than_one_chunk():
    """300 000 truth records, more than 32 MiB of text, against 50 000 aligned records"""
    n = 300000
    rng = random.Random(4)
    names = ["chr1_%d_%d_0_1_0_0_0:0:0_0:0:0_%x" % (1 + k % 900, 61 + k % 900, k) for k in range(n)]
    cigs = ["60M", "60M", "20M2I38M", "25M3D35M", "1I30M1D29M"]
    seq = "ACGT" * 15
    truth = HEAD + "".join("%s\t0\tchr%d\t%d\t255\t%s\t*\t0\t0\t%s\t%s\n" % (names[k], 1 + k % 2, 2 + k % 900, cigs[k % 5], seq, seq) for k in range(n)).encode()
    assert len(truth) > (32 << 20)
    lines = []
    for k in rng.sample(range(n), 50000):
        cig = cigs[k % 5] if k % 3 else "60M"
        lines.append("%s\t0\tchr%d\t%d\t%d\t%s\t=\t0\t0\tACGT\tIIII" % (names[k], 1 + (k + (k % 11 == 0)) % 2, 2 + k % 900 + (k % 7 == 0), k % 256, cig))
    sam = HEAD + "".join(l + "\n" for l in lines).encode()
    want = T.run(truth, [sam], M.Opts(z=1))
    assert want[0].status == 0
    same(api.eval_sam([io.BytesIO(sam)], truth=io.BytesIO(truth), z=1), want)
