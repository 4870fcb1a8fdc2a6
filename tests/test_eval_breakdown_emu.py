"""CPU-only check of dwgsim_eval-hip's breakdown (dw_eval.hpp BREAKDOWN): dw_eval.hip and dw_eval.cpp compiled against the SIMT emulation shim
(tests/emu/build_eval.sh).  A run with a breakdown must leave the main table, -p text, stderr and n as they are, and every section must be the
table that the plain-Python model gives for the filter run it stands for (-s k, -e k, -i; eval_breakdown.expected).  Chunks of 4096 bytes, so
that strata, -m pairs and context lines cross many chunk boundaries.  Test infrastructure: the product has no CPU path."""
import io, os, random, subprocess
import pytest

import bam_io as B
import eval_breakdown as X
import eval_model as M
import eval_sam as S
from dwgsim_amd import api
from test_eval_emu import CASES, CONTIGS

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
ERR_ARG, ERR_STATE = -1, -6       # DWGSIM_HIP_ERR_ARG, DWGSIM_HIP_ERR_STATE


@pytest.fixture(scope="module")
def lib():
    subprocess.run([os.path.join(EMU, "build_eval.sh")], check=True, stdout=subprocess.DEVNULL)
    return api.load_eval(os.path.join(EMU, "libdwgsim_eval_emu.so"))


@pytest.fixture(scope="module")
def sams():
    rng = random.Random(11)
    return {"paired": S.sam_file(rng, CONTIGS, 1200), "paired2": S.sam_file(rng, CONTIGS, 300),
            "single": S.sam_file(rng, CONTIGS, 900, paired=False), "prefix": S.sam_file(rng, CONTIGS, 800, prefix="pfx"),
            "wide": S.sam_file(rng, CONTIGS, 600, wide_scores=True)}


def run(lib, files, dims=X.ALL, cap=0, chunk=4096, **o):
    return api.eval_sam([io.BytesIO(f) for f in files], lib=lib, chunk_bytes=chunk, read_bytes=1000, breakdown=dims, breakdown_cap=cap, **o)


def same_main(sm, table, want):
    assert sm.status == want.status and sm.stderr == want.stderr
    assert table == want.table and sm.incorrect == want.incorrect
    if want.status:
        assert (sm.error_code, sm.error_record) == (want.error_code, want.error_record)
    else:
        assert sm.n == want.n


SIX = [CASES[0], CASES[3], CASES[4], CASES[8], CASES[9], CASES[12]]


@pytest.mark.parametrize("name,o", SIX, ids=[f"{n}-{'_'.join(f'{k}{v}' for k, v in o.items())}" for n, o in SIX])
def test_nothing_else_moves(lib, sams, name, o):
    want = M.run([sams[name]], X.opts(o))
    table, sm = run(lib, [sams[name]], **o)
    same_main(sm, table, want)
    if want.status:
        assert (name, o) == ("single", {}) and sm.breakdown == {}
    else:
        assert list(sm.breakdown) == X.labels(X.ALL, 8)


def test_six_hold_a_z_mismatch(sams):
    assert [M.run([sams[n]], X.opts(o)).status for n, o in SIX].count(1) == 1


@pytest.mark.parametrize("names,o", [(["paired"], {"a": 0}), (["wide"], {"a": 3, "d": 2}), (["paired", "paired2", "paired"], {"m": 1, "a": 3})],
                         ids=["a0", "wide-a3-d2", "three-files-m"])
def test_a_stratum_is_a_filter_run(lib, sams, names, o):
    files = [sams[n] for n in names]
    table, sm = run(lib, files, cap=4, **o)
    same_main(sm, table, M.run(files, X.opts(o)))
    end = not o.get("m")
    X.check_sections(sm.breakdown, X.expected(files, o, X.ALL, 4, 3, end=end), X.ALL, 4, end=end)


def test_single_end_with_z(lib, sams):
    files = [sams["single"]]
    table, sm = run(lib, files, z=1)
    want = X.expected(files, {"z": 1}, X.ALL, 8, 3)
    X.check_sections(sm.breakdown, want, X.ALL, 8)
    assert sm.breakdown["end=2"] == M.format_table({}, 0, 1) and sm.breakdown["end=1"] == table


def test_the_last_stratum(lib, sams):
    files = [sams["paired"]]
    table, sm = run(lib, files, dims="errors,snps", cap=2, a=3)
    e2, e3 = (M.run(files, M.Opts(a=3, e=k)).hist for k in (2, 3))
    assert sm.breakdown["errors=2+"] == M.format_table(X.add(e2, e3), 3, 1)
    X.check_sections(sm.breakdown, X.expected(files, {"a": 3}, "snps,errors", 2, 3), "snps,errors", 2)
    # a hand-made name with n_sub_1 = -1
    name = S.dwgsim_name("chr1", 100, 200, 0, 1, 0, 0, 1, -1, 0, 0, 0, 0, 7)
    one = S.header(CONTIGS) + b"".join(l + b"\n" for l in S.records(random.Random(3), [name], CONTIGS, dup_frac=0))
    want = M.run([one], M.Opts())
    assert sum(sum(r) for r in want.hist.values()) == 2
    table, sm = run(lib, [one], dims="snps", cap=2)
    assert table == want.table and sm.breakdown["snps=2+"] == want.table
    assert sm.breakdown["snps=0"] == sm.breakdown["snps=1"] == M.format_table({}, 0, 1)


def test_the_largest_layout(lib):
    names = X.many_count_names(CONTIGS)
    files = [S.header(CONTIGS) + b"".join(l + b"\n" for l in S.records(random.Random(5), names, CONTIGS))]
    for o in ({"a": 0}, {"a": 1}):
        table, sm = run(lib, files, cap=32, **o)
        same_main(sm, table, M.run(files, X.opts(o)))
        want = X.expected(files, o, X.ALL, 32, 40)
        assert want["snps=32+"] != M.format_table({}, o["a"], 1) and want["errors=31"] != M.format_table({}, o["a"], 1)
        X.check_sections(sm.breakdown, want, X.ALL, 32)


@pytest.mark.parametrize("o", [{"e": 1}, {"i": 1}, {"q": 20}], ids=["e1", "i1", "q20"])
def test_partition_under_the_users_filters(lib, sams, o):
    files = [sams["paired"]]
    table, sm = run(lib, files, **o)
    same_main(sm, table, M.run(files, X.opts(o)))
    X.check_partition(sm.breakdown, table, X.ALL, 8)
    if "e" in o:
        assert sm.breakdown["errors=1"] == table and sm.breakdown["errors=0"] == M.format_table({}, 0, 1)
    if "i" in o:
        assert sm.breakdown["indels=1+"] == table


def run_items(lib, items, chunk=4096, piece=1000, **o):
    with api.EvalContext(lib=lib, chunk_bytes=chunk, breakdown=X.ALL, **o) as ctx:
        for kind, data in items:
            if kind == "bam":
                ctx.bam_begin()
                for i in range(0, len(data), piece):
                    ctx.feed_bam(data[i:i + piece])
            else:
                head, body = M.split_header(data)
                ctx.header(head)
                ctx.feed(body)
        return ctx.finish()


@pytest.mark.parametrize("name,o", [("paired", {}), ("paired", {"a": 3, "m": 1, "p": 1}), ("wide", {"a": 3, "d": 16, "m": 1})], ids=str)
def test_bam_front(lib, sams, name, o):
    """(wide with -d 16: scores in +-1500, outside the kernel's window, in tables of a few thousand rows)"""
    sam = sams[name]
    t_sam, s_sam = run_items(lib, [("sam", sam)], **o)
    t_bam, s_bam = run_items(lib, [("bam", B.sam_to_bam(sam, block_bytes=700))], **o)
    assert t_bam == t_sam and s_bam.breakdown == s_sam.breakdown and len(s_bam.breakdown) == 22
    assert s_bam.breakdown["snps=0"] == M.run([sam], X.opts(o, s=0)).table


def test_sam_and_bam_in_one_run(lib, sams):
    a, b = sams["paired2"], sams["paired"]
    t_mixed, s_mixed = run_items(lib, [("sam", a), ("bam", B.sam_to_bam(b, block_bytes=700))], a=3)
    t_sam, s_sam = run_items(lib, [("sam", a), ("sam", b)], a=3)
    assert t_mixed == t_sam and s_mixed.breakdown == s_sam.breakdown
    X.check_sections(s_mixed.breakdown, X.expected([a, b], {"a": 3}, X.ALL, 8, 3), X.ALL, 8)


def test_arguments(lib, sams):
    head, body = M.split_header(sams["paired2"])
    with api.EvalContext(lib=lib, chunk_bytes=4096) as ctx:
        assert ctx.set_breakdown("snps,mapq") == ERR_ARG
        assert ctx.set_breakdown("snps,end,snps") == ERR_ARG
        assert ctx.set_breakdown("snps,") == ERR_ARG
        assert ctx.set_breakdown("snps", 33) == ERR_ARG
        assert ctx.set_breakdown("snps", -1) == ERR_ARG
        assert ctx.set_breakdown("errors", 32) == 0
        assert ctx.set_breakdown("", 0) == 0 and ctx.set_breakdown(None, 0) == 0
        ctx.header(head)
        assert ctx.set_breakdown("snps", 0) == ERR_STATE
        ctx.feed(body)
        table, sm = ctx.finish()
        assert table == M.run([sams["paired2"]]).table and sm.breakdown == {}
        assert ctx.set_breakdown("snps", 0) == ERR_STATE
    with pytest.raises(api.DwgsimError):
        api.EvalContext(lib=lib, breakdown="nothing")
    # cap 0 is 8
    _, s0 = run(lib, [sams["paired2"]], dims="snps,errors", cap=0)
    _, s8 = run(lib, [sams["paired2"]], dims="snps,errors", cap=8)
    assert s0.breakdown == s8.breakdown and list(s0.breakdown) == X.labels("snps,errors", 8)


def test_merge_inside_the_record_loop(lib, sams):
    """one device chunk whose blocks make more turns than the kernel allows between two merges of its packed counters: the counts made
    before and after the merges inside the loop must all arrive (-a 0: every score is inside the window)"""
    import ctypes as C
    head, text, turns = X.sparse_chunk(sams["paired2"])
    assert turns > 127
    with api.EvalContext(lib=lib, breakdown=X.ALL) as ctx:
        ctx.header(head)
        ms = C.c_double()
        assert lib.dwgsim_hip_eval_debug_device_chunk(ctx.ctx, text, len(text), 1, C.byref(ms)) == 0
        table, sm = ctx.finish()
    assert table == M.run([sams["paired2"]]).table
    X.check_sections(sm.breakdown, X.expected([sams["paired2"]], {}, X.ALL, 8, 3), X.ALL, 8)


def test_off_by_default(lib, sams):
    table, sm = api.eval_sam([io.BytesIO(sams["paired2"])], lib=lib, chunk_bytes=4096)
    assert sm.breakdown == {} and table == M.run([sams["paired2"]]).table


def test_command_line(lib, sams, tmp_path):
    a = tmp_path / "a.sam"; a.write_bytes(sams["paired"])
    cli = os.path.join(EMU, "dwgsim_eval-emu")
    env = dict(os.environ, DWGSIM_EVAL_CHUNK="8192")
    want = M.run([sams["paired"]], M.Opts(a=1))
    sections = X.expected([sams["paired"]], {"a": 1}, "snps,end", 3, 3)
    text = b"".join(b"## " + l.encode() + b"\n" + sections[l] for l in X.labels("snps,end", 3))
    p = subprocess.run([cli, "-S", "-a", "1", "-B", "snps,end", "-K", "3", str(a)], capture_output=True, env=env, timeout=300)
    assert p.returncode == 0 and p.stdout == want.table + text and p.stderr == want.stderr
    p = subprocess.run([cli, "-S", "-a", "1", str(a)], capture_output=True, env=env, timeout=300)
    assert p.returncode == 0 and p.stdout == want.stdout and p.stderr == want.stderr
    p = subprocess.run([cli, "-S", "-B", "snps,what", str(a)], capture_output=True, env=env, timeout=300)
    assert p.returncode == 1 and p.stdout == b"" and b"-B" in p.stderr
    for args in (["-K", "3"], ["-B", "snps", "-K", "junk"], ["-B", "snps", "-K", "33"]):
        p = subprocess.run([cli, "-S"] + args + [str(a)], capture_output=True, env=env, timeout=300)
        assert p.returncode == 1 and p.stdout == b"" and b"-K" in p.stderr, args
