"""CPU-only check of the dwgsim_eval kernels' logic: dw_eval.hip and dw_eval.cpp compiled against the SIMT emulation shim in tests/emu
(tests/emu/build_eval.sh; one OS thread per GPU thread) must give the model's table, -p text and stderr byte for byte, at chunk sizes of a
few KiB so that lines, -m pairs and the context line cross many chunk boundaries.  Test infrastructure: the product has no CPU path."""
import io, os, random, subprocess
import pytest

import eval_model as M
import eval_sam as S
from dwgsim_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
GOLD = os.path.join(HERE, "golden", "eval")
CONTIGS = [("chr1", 5000), ("chr10", 3000), ("chr2_alt", 2000)]


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


def model_opts(o):
    return M.Opts(**{k: (v.encode() if k == "P" else v) for k, v in o.items()})


def check(lib, files, chunk, read_bytes=1000, **o):
    want = M.run(files, model_opts(o))
    table, sm = api.eval_sam([io.BytesIO(f) for f in files], lib=lib, chunk_bytes=chunk, read_bytes=read_bytes, **o)
    assert sm.status == want.status and sm.stderr == want.stderr
    assert table == want.table and sm.incorrect == want.incorrect
    if want.status:
        assert (sm.error_code, sm.error_record) == (want.error_code, want.error_record)
    else:
        assert sm.n == want.n
    return want


CASES = [
    ("paired", {}), ("paired", {"a": 1}), ("paired", {"a": 2, "d": 3}), ("paired", {"a": 3, "g": 0}), ("paired", {"q": 20, "m": 1, "p": 1}),
    ("paired", {"i": 1, "e": 1}), ("paired", {"e": 2, "s": 1}), ("paired", {"n": 99}), ("single", {"z": 1, "p": 1}), ("single", {}),
    ("prefix", {"P": "pfx", "a": 3, "p": 1}), ("prefix", {}), ("wide", {"a": 3, "d": 2}), ("wide", {"a": 1, "m": 1}),
]


@pytest.mark.parametrize("name,o", CASES, ids=[f"{n}-{'_'.join(f'{k}{v}' for k, v in o.items())}" for n, o in CASES])
def test_emu_matches_model(lib, sams, name, o):
    check(lib, [sams[name]], 4096, **o)


def test_emu_several_files_and_large_chunks(lib, sams):
    check(lib, [sams["paired"], sams["paired2"], sams["paired"]], 1 << 20, read_bytes=1 << 16, m=1, p=1, a=3)


def test_emu_fixtures(lib):
    for fn in sorted(os.listdir(GOLD)):
        with open(os.path.join(GOLD, fn), "rb") as f:
            data = f.read()
        z = int(fn.startswith("single"))
        for o in ({"z": z}, {"z": z, "m": 1, "p": 1, "a": 3, "g": 0}):
            check(lib, [data], 4096, read_bytes=7, **o)


def test_emu_feed_split_everywhere(lib):
    """one file fed in two pieces, split at every offset of a stretch that crosses a chunk boundary"""
    with open(os.path.join(GOLD, "multi.sam"), "rb") as f:
        head, body = M.split_header(f.read())
    body = body * 12                          # about 1.1 KiB of records per copy; chunks of 4 KiB
    want = M.run([head + body], M.Opts(m=1, p=1))
    for cut in range(3900, 4400, 7):
        with api.EvalContext(lib=lib, chunk_bytes=4096, m=1, p=1) as ctx:
            ctx.header(head)
            ctx.feed(body[:cut]); ctx.feed(body[cut:])
            table, sm = ctx.finish()
        assert table == want.table and sm.incorrect == want.incorrect and sm.n == want.n, cut


def test_emu_cli_stdin_and_files(lib, sams, tmp_path):
    a = tmp_path / "a.sam"; a.write_bytes(sams["paired"])
    b = tmp_path / "b.sam"; b.write_bytes(sams["paired2"])
    cli = os.path.join(EMU, "dwgsim_eval-emu")
    want = M.run([sams["paired"], sams["paired2"]], M.Opts(m=1, p=1, a=1))
    env = dict(os.environ, DWGSIM_EVAL_CHUNK="8192")
    p = subprocess.run([cli, "-S", "-m", "1", "-p", "-a", "1", str(a), "-"], input=sams["paired2"], capture_output=True, env=env, timeout=300)
    assert p.returncode == 0 and p.stdout == want.stdout
    assert p.stderr == want.stderr
    p = subprocess.run([cli, "-S", "-z", str(a)], capture_output=True, env=env, timeout=300)
    want = M.run([sams["paired"]], M.Opts(z=1))
    assert p.returncode == 1 and p.stdout == b"" and p.stderr == want.stderr
