"""The breakdown of dwgsim_eval-hip (dw_eval.hpp BREAKDOWN) on the MI355X: the four simulations of test_gpu_eval.py, evaluated with all four
dimensions, must keep the main table, -p text, stderr and n of the plain-Python model, and every section must be the table of the model's
filter run that it stands for (eval_breakdown.expected), through SAM text and through BAM, at 4 KiB chunks and at the default chunk size."""
import io, os, random, subprocess
import pytest

import bam_io as B
import eval_breakdown as X
import eval_model as M
import eval_sam as S
from dwgsim_amd import api
from test_gpu_eval import SIMS, CLI, simulate

pytestmark = pytest.mark.gpu
CHUNKS = [4096, 0]


@pytest.fixture(scope="module")
def sams():
    out = {}
    for key, (fa, flags, paired, prefix) in SIMS.items():
        contigs, names = simulate(fa, flags)
        rng = random.Random(len(names))
        recs = S.records(rng, names, contigs, paired, prefix, wide_scores=(key == "solid"))
        out[key] = (S.header(contigs) + b"".join(r + b"\n" for r in recs), paired, prefix)
    return out


def base_opts(sams, key, **o):
    _, paired, prefix = sams[key]
    if not paired:
        o["z"] = 1
    if prefix:
        o["P"] = prefix
    return o


def max_count(data):
    """the largest n_err_1 / n_sub_1 of the file's names (read by the test's own rule: the fields before the last two colons-groups)"""
    top = 0
    for line in M.record_lines(M.split_header(data)[1]):
        f = line.split(b"\t")[0].split(b"/")[0].rsplit(b"_", 3)
        e1, u1, _ = f[1].split(b":")
        top = max(top, int(e1), int(u1))
    return top


def run(files, chunk, dims=X.ALL, cap=0, **o):
    return api.eval_sam([io.BytesIO(f) for f in files], chunk_bytes=chunk, read_bytes=1 << 20, breakdown=dims, breakdown_cap=cap, **o)


def same_main(sm, table, want):
    assert (sm.status, sm.stderr) == (want.status, want.stderr)
    assert table == want.table and sm.incorrect == want.incorrect
    if want.status:
        assert (sm.error_code, sm.error_record) == (want.error_code, want.error_record)
    else:
        assert sm.n == want.n


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("key,o", [("illumina", {}), ("illumina", {"a": 3, "g": 0}), ("illumina", {"q": 20, "m": 1, "p": 1}), ("single", {"p": 1}),
                                   ("illumina", {"z": 1}), ("solid", {"a": 3, "d": 2})], ids=str)
def test_gpu_nothing_else_moves(sams, key, o, chunk):
    o = base_opts(sams, key, **o)
    want = M.run([sams[key][0]], X.opts(o))
    table, sm = run([sams[key][0]], chunk, **o)
    same_main(sm, table, want)
    assert want.status == (1 if o.get("z") and key == "illumina" else 0)
    assert list(sm.breakdown) == ([] if want.status else X.labels(X.ALL, 8))


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("keys,o", [(["illumina"], {"a": 0}), (["solid"], {"a": 3, "d": 2}), (["single"], {"a": 1}), (["prefix"], {"a": 3}),
                                    (["illumina", "solid", "illumina"], {"m": 1, "a": 3, "d": 16})], ids=str)
def test_gpu_a_stratum_is_a_filter_run(sams, keys, o, chunk):
    files = [sams[k][0] for k in keys]
    o = base_opts(sams, keys[0], **o)
    top = max(max_count(f) for f in files)
    cap = 3
    table, sm = run(files, chunk, cap=cap, **o)
    same_main(sm, table, M.run(files, X.opts(o)))
    end = not o.get("m")
    X.check_sections(sm.breakdown, X.expected(files, o, X.ALL, cap, max(top, cap), end=end), X.ALL, cap, end=end)


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("o", [{"e": 1}, {"i": 1}, {"q": 20}], ids=str)
def test_gpu_partition_under_the_users_filters(sams, o, chunk):
    files = [sams["illumina"][0]]
    table, sm = run(files, chunk, **o)
    same_main(sm, table, M.run(files, X.opts(o)))
    X.check_partition(sm.breakdown, table, X.ALL, 8)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_gpu_bam_front(sams, chunk):
    il, so = sams["illumina"][0], sams["solid"][0]
    for sam, o in ((il, {}), (so, {"a": 3, "d": 16, "m": 1, "p": 1})):       # (-d 16: still outside the kernel's window, in short tables)
        t_sam, s_sam = run([sam], chunk, **o)
        t_bam, s_bam = api.eval_bam([io.BytesIO(B.sam_to_bam(sam, block_bytes=3000))], chunk_bytes=chunk, read_bytes=1 << 16, breakdown=X.ALL, **o)
        assert t_bam == t_sam and s_bam.breakdown == s_sam.breakdown and len(s_bam.breakdown) == 22
        assert s_bam.breakdown["snps=0"] == M.run([sam], X.opts(o, s=0)).table
    # a SAM file and a BAM file in one run
    with api.EvalContext(chunk_bytes=chunk, breakdown=X.ALL, a=3, d=16) as ctx:
        head, body = M.split_header(il)
        ctx.header(head); ctx.feed(body)
        ctx.bam_begin(); ctx.feed_bam(B.sam_to_bam(so))
        table, sm = ctx.finish()
    same_main(sm, table, M.run([il, so], M.Opts(a=3, d=16)))
    top = max(max_count(il), max_count(so), 8)
    X.check_sections(sm.breakdown, X.expected([il, so], {"a": 3, "d": 16}, X.ALL, 8, top), X.ALL, 8)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_gpu_the_largest_layout(chunk):
    contigs = [("chr1", 5000), ("chr10", 3000), ("chr2_alt", 2000)]
    names = X.many_count_names(contigs)
    files = [S.header(contigs) + b"".join(l + b"\n" for l in S.records(random.Random(5), names, contigs))]
    for o in ({"a": 0}, {"a": 1}):
        table, sm = run(files, chunk, cap=32, **o)
        same_main(sm, table, M.run(files, X.opts(o)))
        X.check_sections(sm.breakdown, X.expected(files, o, X.ALL, 32, 40), X.ALL, 32)


def test_gpu_merge_inside_the_record_loop(sams):
    """one device chunk whose blocks make more turns than the kernel allows between two merges of its packed counters (see
    eval_breakdown.sparse_chunk): every count must arrive (-a 0: every score is inside the window)"""
    import ctypes as C
    il = sams["illumina"][0]
    head, body = M.split_header(il)
    small = head + b"".join(l + b"\n" for l in M.record_lines(body)[:1500])
    head, text, turns = X.sparse_chunk(small)
    assert turns > 127
    lib = api.load()
    with api.EvalContext(breakdown=X.ALL) as ctx:
        ctx.header(head)
        ms = C.c_double()
        assert lib.dwgsim_hip_eval_debug_device_chunk(ctx.ctx, text, len(text), 1, C.byref(ms)) == 0
        table, sm = ctx.finish()
    assert table == M.run([small]).table
    X.check_sections(sm.breakdown, X.expected([small], {}, X.ALL, 8, max(8, max_count(small))), X.ALL, 8)


def test_gpu_command_line(sams, tmp_path):
    il = sams["illumina"][0]
    a = tmp_path / "a.sam"; a.write_bytes(il)
    want = M.run([il], M.Opts(a=1))
    sections = X.expected([il], {"a": 1}, X.ALL, 8, max(8, max_count(il)))
    text = b"".join(b"## " + l.encode() + b"\n" + sections[l] for l in X.labels(X.ALL, 8))
    p = subprocess.run(["timeout", "-k", "10", "300", CLI, "-S", "-a", "1", "-B", "snps,errors,indels,end", str(a)], capture_output=True, timeout=320)
    assert p.returncode == 0 and p.stdout == want.table + text and p.stderr == want.stderr
