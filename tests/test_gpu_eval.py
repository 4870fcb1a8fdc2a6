"""dwgsim_eval-hip on the MI355X against the plain-Python model (tests/eval_model.py), byte for byte.  Reads are simulated with the library
(Illumina paired, single-end, -P, -y, SOLiD), turned into SAM by the seeded test aligner of tests/eval_sam.py, and evaluated through the
Python API and the command line with many option sets, feeds split across chunk boundaries, a run of more than 2^31 bytes, and every
fatal error."""
import io, os, random, subprocess
import pytest

import eval_model as M
import eval_sam as S
from dwgsim_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CLI = os.path.join(ROOT, "dwgsim_amd", "dwgsim_eval-hip")
pytestmark = pytest.mark.gpu

SIMS = {
    "illumina": ("ex1.fa", "-z 13 -N 3000 -r 0.01", True, None),
    "single": ("tiny.fa", "-z 5 -N 2500 -2 0", False, None),
    "prefix": ("tiny.fa", "-z 7 -N 2000 -P pfx -y 0.2", True, "pfx"),
    "solid": ("tiny.fa", "-z 9 -N 1500 -c 1 -1 50 -2 50 -y 0.1", True, None),
}


def simulate(fa, flags):
    contigs = api.read_fasta(os.path.join(GOLD, fa))
    res = api.run_job(api.parse_flags(flags), contigs)
    lines = res.streams[0].split(b"\n")
    names = [l[1:].decode().rsplit("/", 1)[0] for l in lines[0::4] if l.startswith(b"@")]
    return [(n, len(a)) for n, a in contigs], names


@pytest.fixture(scope="module")
def sams():
    out = {}
    for key, (fa, flags, paired, prefix) in SIMS.items():
        contigs, names = simulate(fa, flags)
        rng = random.Random(len(names))
        recs = S.records(rng, names, contigs, paired, prefix, wide_scores=(key == "solid"))
        out[key] = (S.header(contigs) + b"".join(r + b"\n" for r in recs), paired, prefix)
    return out


def model(files, **o):
    return M.run(files, M.Opts(**{k: (v.encode() if k == "P" else v) for k, v in o.items()}))


def api_run(files, chunk=0, read_bytes=1 << 20, **o):
    return api.eval_sam([io.BytesIO(f) for f in files], chunk_bytes=chunk, read_bytes=read_bytes, **o)


def same(files, chunk=0, **o):
    want = model(files, **o)
    table, sm = api_run(files, chunk, **o)
    assert (sm.status, sm.stderr) == (want.status, want.stderr)
    assert table == want.table and sm.incorrect == want.incorrect
    if want.status:
        assert (sm.error_code, sm.error_record) == (want.error_code, want.error_record)
    else:
        assert sm.n == want.n
    return want


OPTS = [{}, {"a": 1}, {"a": 2}, {"a": 3}, {"a": 0, "d": 3}, {"a": 3, "d": 3}, {"g": 0}, {"g": 5, "a": 1, "d": 3}, {"q": 20}, {"m": 1},
        {"m": 1, "p": 1, "q": 10}, {"i": 1}, {"e": 1}, {"s": 0}, {"e": 0, "s": 1}, {"i": 1, "e": 2}, {"p": 1}, {"n": 12345}, {"b": 1, "c": 1}]


@pytest.mark.parametrize("key", list(SIMS))
@pytest.mark.parametrize("oi", range(len(OPTS)))
def test_gpu_eval_matches_model(sams, key, oi):
    data, paired, prefix = sams[key]
    o = dict(OPTS[oi])
    if not paired:
        o["z"] = 1
    if prefix:
        o["P"] = prefix
    same([data], chunk=(64 << 10) if oi % 2 else 0, **o)


def test_gpu_eval_z_mismatch(sams):
    same([sams["illumina"][0]], z=1)
    same([sams["single"][0]])


def test_gpu_eval_several_files_and_small_chunks(sams):
    d = sams["illumina"][0]
    same([d, d, sams["solid"][0]], chunk=4096, m=1, p=1, a=3)


def test_gpu_eval_cli(sams, tmp_path):
    a = tmp_path / "a.sam"; a.write_bytes(sams["illumina"][0])
    b = tmp_path / "b.sam"; b.write_bytes(sams["solid"][0])
    il, so = sams["illumina"][0], sams["solid"][0]
    for args, files, o in [(["-S", str(a)], [il], {}),
                           (["-S", "-a", "3", "-d", "3", "-m", "x", "-p", str(a), str(b)], [il, so], {"a": 3, "d": 3, "m": 1, "p": 1}),
                           (["-S", "-n", "7", "-q", "5", str(a), "-"], [il, so], {"n": 7, "q": 5}),
                           (["-S", "-z", "-"], [so], {"z": 1})]:
        want = model(files, **o)
        p = subprocess.run(["timeout", "-k", "10", "300", CLI] + args, input=sams["solid"][0], capture_output=True, timeout=320)
        assert p.returncode == want.status and p.stdout == want.stdout and p.stderr == want.stderr, args


def test_gpu_eval_feed_split_at_every_offset(sams):
    head, body = M.split_header(sams["illumina"][0])
    body = body[:20000]
    body = body[:body.rfind(b"\n") + 1]
    want = model([head + body], m=1, p=1)
    for cut in range(4096 - 300, 4096 + 300):
        with api.EvalContext(chunk_bytes=4096, m=1, p=1) as ctx:
            ctx.header(head)
            ctx.feed(body[:cut]); ctx.feed(body[cut:])
            table, sm = ctx.finish()
        assert table == want.table and sm.incorrect == want.incorrect and sm.n == want.n, cut


def test_gpu_eval_more_than_2_to_31_bytes(sams):
    """one run of > 2^31 bytes of SAM: one block of records fed again and again; the model's answer is the block's, times the repeats"""
    head, body = M.split_header(sams["illumina"][0])
    block = body * max(1, (8 << 20) // len(body))
    reps = (1 << 31) // len(block) + 2
    one = model([head + block], a=1)
    hist = {k: [v * reps for v in vs] for k, vs in one.hist.items()}
    with api.EvalContext(a=1) as ctx:
        ctx.header(head)
        for _ in range(reps):
            ctx.feed(block)
        table, sm = ctx.finish()
    assert len(block) * reps > (1 << 31)
    assert sm.status == 0 and sm.n == one.n * reps and sm.records == len(M.record_lines(block)) * reps
    assert table == M.format_table(hist, 1, 1)


BAD = {
    M.E_NAME: b"not_from_dwgsim\t65\tchr1\t100\t60\t50M\t=\t0\t0\tA\tI\n",
    M.E_MALFORMED: b"three\tfields\tonly\n",
    M.E_NOT_PAIRED: None,          # a single-end copy of a good record
    M.E_CONTIG: b"nochr_100_200_0_0_0_0_0:0:0_0:0:0_1\t65\t*\t0\t0\t*\t*\t0\t0\tA\tI\n",
}


@pytest.mark.parametrize("code", list(BAD))
@pytest.mark.parametrize("where", [0.0, 0.37, 0.93])
def test_gpu_eval_fatal_errors(sams, code, where):
    head, body = M.split_header(sams["illumina"][0])
    lines = M.record_lines(body)
    k = int(where * len(lines))
    if code == M.E_NOT_PAIRED:
        f = lines[k].split(b"\t"); f[1] = b"0"; bad = b"\t".join(f) + b"\n"
    else:
        bad = BAD[code]
    later = BAD[M.E_NAME] if code != M.E_NAME else BAD[M.E_MALFORMED]
    text = head + b"".join(l + b"\n" for l in lines[:k]) + bad + b"".join(l + b"\n" for l in lines[k:k + 500]) + later + \
        b"".join(l + b"\n" for l in lines[k + 500:])
    for chunk in (4096, 0):
        want = same([text], chunk=chunk)
        assert (want.status, want.error_code, want.error_record) == (1, code, k)


def test_gpu_eval_prefix_and_z_errors(sams):
    data = sams["prefix"][0]
    assert same([data], P="pfq").error_code == M.E_PREFIX
    assert same([data], z=1, P="pfx").error_code == M.E_PAIRED
