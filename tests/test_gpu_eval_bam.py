"""dwgsim_eval-hip's BAM input on the MI355X against the plain-Python model, byte for byte: the simulated inputs and option sets of
test_gpu_eval.py, encoded to BAM by the test's own writer (bam_io.py); the model runs on the SAM text that the test's own decoder makes of the
same BAM bytes.  Python API and command line, mixed formats in one run, feeds split everywhere, a record longer than a chunk, and every fatal
record, malformed record and container error once."""
import io, os, random, struct, subprocess
import pytest

import bam_io as B
import eval_model as M
import eval_sam as S
from dwgsim_amd import api
from test_gpu_eval import SIMS, OPTS, simulate
from test_eval_bam_emu import damage, DAMAGE, with_line, patch_l_read_name, patch_no_nul, patch_ref_id, patch_block_size_31, patch_block_size_short, START

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dwgsim_amd", "dwgsim_eval-hip")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sams():
    out = {}
    for key, (fa, flags, paired, prefix) in SIMS.items():
        contigs, names = simulate(fa, flags)
        rng = random.Random(len(names))
        recs = S.records(rng, names, contigs, paired, prefix, wide_scores=(key == "solid"))
        out[key] = (S.header(contigs) + b"".join(r + b"\n" for r in recs), paired, prefix)
    return out


@pytest.fixture(scope="module")
def bams(sams):
    """per input: the BAM bytes, and the SAM text that the model reads (decoded once, shared)"""
    out = {}
    for key, (sam, paired, prefix) in sams.items():
        bam = B.sam_to_bam(sam, block_bytes=65280 if key != "single" else 5000)
        out[key] = (bam, B.bam_to_sam(bam), paired, prefix)
    return out


@pytest.fixture(scope="module")
def small(sams):
    head, body = M.split_header(sams["illumina"][0])
    return head + b"".join(l + b"\n" for l in M.record_lines(body)[:150])


def model(files, **o):
    return M.run(files, M.Opts(**{k: (v.encode() if k == "P" else v) for k, v in o.items()}))


def check(got, want):
    table, sm = got
    assert (sm.status, sm.stderr) == (want.status, want.stderr)
    assert table == want.table and sm.incorrect == want.incorrect
    if want.status:
        assert (sm.error_code, sm.error_record) == (want.error_code, want.error_record)
    else:
        assert sm.n == want.n
    return want


def same(bam_files, chunk=0, read_bytes=1 << 20, **o):
    return check(api.eval_bam([io.BytesIO(f) for f in bam_files], chunk_bytes=chunk, read_bytes=read_bytes, **o),
                 model([B.bam_to_sam(f) for f in bam_files], **o))


@pytest.mark.parametrize("key", list(SIMS))
@pytest.mark.parametrize("oi", range(len(OPTS)))
def test_gpu_eval_bam_matches_model(bams, key, oi):
    bam, text, paired, prefix = bams[key]
    o = dict(OPTS[oi])
    if not paired:
        o["z"] = 1
    if prefix:
        o["P"] = prefix
    got = api.eval_bam([io.BytesIO(bam)], chunk_bytes=(64 << 10) if oi % 2 else 0, read_bytes=(1 << 20) if oi % 3 else 3001, **o)
    check(got, model([text], **o))


def test_gpu_eval_bam_cli(bams, sams, tmp_path):
    il, so = bams["illumina"], bams["solid"]
    a = tmp_path / "a.bam"; a.write_bytes(il[0])
    b = tmp_path / "b.bam"; b.write_bytes(so[0])
    for args, files, o in [([str(a)], [il[1]], {}),
                           (["-a", "3", "-d", "3", "-m", "x", "-p", str(a), str(b)], [il[1], so[1]], {"a": 3, "d": 3, "m": 1, "p": 1}),
                           (["-n", "7", "-q", "5", str(a), "-"], [il[1], so[1]], {"n": 7, "q": 5}),
                           (["-z", "-"], [so[1]], {"z": 1})]:
        want = model(files, **o)
        env = dict(os.environ, DWGSIM_EVAL_THREADS="4")
        p = subprocess.run(["timeout", "-k", "10", "300", CLI] + args, input=so[0], capture_output=True, timeout=320, env=env)
        assert p.returncode == want.status and p.stdout == want.stdout and p.stderr == want.stderr, args
    # the SAM text of the same file with -S: the same table
    s = tmp_path / "a.sam"; s.write_bytes(il[1])
    p = subprocess.run(["timeout", "-k", "10", "300", CLI, "-S", str(s)], capture_output=True, timeout=320)
    q = subprocess.run(["timeout", "-k", "10", "300", CLI, str(a)], capture_output=True, timeout=320)
    assert p.returncode == 0 and (q.returncode, q.stdout, q.stderr) == (0, p.stdout, p.stderr)


def test_gpu_eval_two_bam_files_and_a_sam_file(bams, sams):
    il, so = bams["illumina"], bams["solid"]
    sam = sams["illumina"][0]
    o = dict(m=1, p=1, a=3)
    with api.EvalContext(chunk_bytes=4096, **o) as ctx:
        ctx.bam_begin(); ctx.feed_bam(il[0])
        head, body = M.split_header(sam)
        ctx.header(head); ctx.feed(body)
        ctx.bam_begin()
        for i in range(0, len(so[0]), 777):
            ctx.feed_bam(so[0][i:i + 777])
        got = ctx.finish()
    check(got, model([il[1], sam, so[1]], **o))


def test_gpu_eval_bam_feed_split_at_every_offset(small):
    """one file fed in two pieces, split at every offset of its first 3 000 compressed bytes: the 3 000 copies are the files of one run (a
    context per cut would spend the test's time on creating contexts), so the expected counts are one copy's, times 3 000"""
    bam = B.sam_to_bam(small, block_bytes=700)
    text = B.bam_to_sam(bam)
    assert len(bam) > 3000
    one, two = model([text], m=1, p=1), model([text, text], m=1, p=1)
    head = M.split_header(text)[0]
    assert two.n == 2 * one.n and two.incorrect == one.incorrect + one.incorrect[len(head):]      # -m sees nothing across the file boundary
    cuts = range(1, 3001)
    with api.EvalContext(chunk_bytes=4096, m=1, p=1) as ctx:
        for cut in cuts:
            ctx.bam_begin()
            ctx.feed_bam(bam[:cut]); ctx.feed_bam(bam[cut:])
        table, sm = ctx.finish()
    assert sm.status == 0 and sm.n == one.n * len(cuts) and sm.records == 150 * len(cuts)
    assert table == M.format_table({k: [v * len(cuts) for v in vs] for k, vs in one.hist.items()}, 0, 1)
    assert sm.incorrect == head + one.incorrect[len(head):] * len(cuts)


def test_gpu_eval_bam_record_longer_than_the_chunk(small):
    head, body = M.split_header(small)
    lines = M.record_lines(body)
    rng = random.Random(3)
    f = lines[40].split(b"\t")
    f[9] = bytes(rng.choice(b"ACGTN") for _ in range(20000)); f[10] = bytes(rng.randrange(33, 74) for _ in range(20000))
    sam = head + b"".join(l + b"\n" for l in lines[:40]) + b"\t".join(f) + b"\n" + b"".join(l + b"\n" for l in lines[40:])
    same([B.sam_to_bam(sam, block_bytes=700)], chunk=4096, m=1, p=1)


FATAL = {
    M.E_NAME: ("illumina", {}, b"not_from_dwgsim\t65\t*\t0\t60\t*\t*\t0\t0\tA\tI\n"),
    M.E_CONTIG: ("illumina", {}, b"nochr_100_200_0_0_0_0_0:0:0_0:0:0_1\t65\t*\t0\t0\t*\t*\t0\t0\tA\tI\n"),
    M.E_NOT_PAIRED: ("illumina", {}, None),
    M.E_PAIRED: ("illumina", {"z": 1}, None),
    M.E_PREFIX: ("prefix", {"P": "pfq"}, None),
}


@pytest.mark.parametrize("code", list(FATAL))
def test_gpu_eval_bam_fatal_records(sams, code):
    key, o, bad = FATAL[code]
    sam, k = sams[key][0], 0
    if code == M.E_NOT_PAIRED:
        head, body = M.split_header(sam)
        k = 137
        f = M.record_lines(body)[k].split(b"\t"); f[1] = b"0"; bad = b"\t".join(f) + b"\n"
    if bad:
        k = k or 211
        sam = with_line(sam, k, bad, n_lines=2000)
    want = same([B.sam_to_bam(sam, block_bytes=3000)], chunk=4096, **o)
    assert (want.status, want.error_code, want.error_record) == (1, code, k)


@pytest.mark.parametrize("patch", [patch_l_read_name, patch_no_nul, patch_ref_id, patch_block_size_31, patch_block_size_short],
                         ids=lambda f: f.__name__)
def test_gpu_eval_bam_malformed_records(small, patch):
    payload, offs = B.bam_payload(small)
    p = bytearray(payload)
    patch(p, offs[77])
    table, sm = api.eval_bam([io.BytesIO(B.bgzf(bytes(p), 700))], chunk_bytes=4096, m=1)
    assert (sm.status, sm.error_code, sm.error_record) == (1, M.E_MALFORMED, 77)
    assert table == b"" and sm.stderr == (START + M.error_text(M.E_MALFORMED, None)).encode()


@pytest.mark.parametrize("name", DAMAGE)
def test_gpu_eval_bam_container_errors(small, name):
    with pytest.raises(api.DwgsimError, match=r"BAM input: .+ at byte \d+ of the compressed file"):
        api.eval_bam([io.BytesIO(damage(name, small))], chunk_bytes=4096)


def test_gpu_eval_bam_fatal_record_in_front_of_the_damage_wins(small):
    bad = with_line(small, 10, FATAL[M.E_NAME][2])
    table, sm = api.eval_bam([io.BytesIO(damage("crc", bad))], chunk_bytes=4096, read_bytes=500)
    assert (sm.status, sm.error_code, sm.error_record) == (1, M.E_NAME, 10) and table == b""
    assert sm.stderr == M.run([bad]).stderr
