"""The host-only text code of dwgsim_eval-hip's breakdown (dwgsim_amd/csrc/dw_eval_table.hpp: the dimension list, the counter layout, the spill
decoding, the tables and sections) in a stand-alone program (tests/eval_table_main.cpp) built with -fsanitize=address,undefined: hand-filled
records must come out as the tables that the plain-Python model's formatter makes of the same counts, without a sanitizer report."""
import os, random, subprocess
import pytest

import eval_breakdown as X
import eval_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "dwgsim_amd", "csrc")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("evaltable") / "eval_table_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(HERE, "eval_table_main.cpp"), "-o", exe], check=True)
    return exe


def run(prog, tmp_path, head, recs):
    path = tmp_path / "case.txt"
    path.write_text(head + "\n" + "".join("%d %d %d %d %d %d\n" % r for r in recs))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([prog, str(path)], capture_output=True, env=env, timeout=120)
    assert p.returncode == 0 and p.stderr == b"", p.stderr.decode(errors="replace")[-2000:]
    return p.stdout


def records(rng, n, top, lo, hi, floor):
    """(score, class, n_sub_1, n_err_1, indel flag, end): scores in the window, at both of its edges, outside it (a table has one row per
    score between its extremes, so not far outside) and at the floor score; counts from -2 to top"""
    edge = [lo, hi, -1, 0, 255, 256, -64, -65, 191, 192, floor, floor + 1, floor - 1 if floor > -5000 else floor, -5000, 1500, -1500]
    return [(rng.choice(edge) if rng.random() < 0.3 else rng.randrange(lo, hi), rng.randrange(5), rng.randrange(-2, top + 1), rng.randrange(-2, top + 1),
             rng.randrange(2), rng.randrange(2)) for _ in range(n)]


def want_text(recs, dims, cap, a, d):
    def stratum(v):
        return v if 0 <= v < cap else cap
    def table(keep):
        hist = {}
        for r in recs:
            if keep(r):
                hist.setdefault(r[0], [0] * 5)[r[1]] += 1
        return M.format_table(hist, a, d)
    out = table(lambda r: True)
    pick = {"snps": lambda r: stratum(r[2]), "errors": lambda r: stratum(r[3]), "indels": lambda r: r[4], "end": lambda r: r[5]}
    for k, label in enumerate(X.labels(dims, cap)):
        dim, val = label.split("=")
        index = {"0": 0, "1+": 1}[val] if dim == "indels" else int(val) - 1 if dim == "end" else int(val.rstrip("+"))
        out += b"## " + label.encode() + b"\n" + table(lambda r: pick[dim](r) == index)
    return out


@pytest.mark.parametrize("dims,cap,a,d", [(X.ALL, 0, 0, 1), (X.ALL, 32, 3, 1), ("errors", 1, 1, 7), ("end,snps", 5, 3, -3), ("indels", 0, 2, 5000), (X.ALL, 8, 0, 2)])
def test_sections_equal_the_models_tables(prog, tmp_path, dims, cap, a, d):
    floor = max(M.cdiv(-5000, d), -5000)
    recs = records(random.Random(cap * 10 + a), 3000, 40, -300, 400, floor)
    out = run(prog, tmp_path, "%s %d %d %d 32768 2048" % (dims, cap, a, d), recs)
    first, rest = out.split(b"\n", 1)
    assert first.startswith(b"window ")
    assert rest == want_text(recs, dims, cap or 8, a, d)


def test_off_and_empty(prog, tmp_path):
    recs = records(random.Random(1), 200, 3, -20, 50, -5000)
    out = run(prog, tmp_path, "- 0 0 1 32768 2048", recs)
    assert out.split(b"\n", 1)[1] == want_text(recs, "", 8, 0, 1)
    out = run(prog, tmp_path, "snps,end 2 1 1 32768 2048", [])
    assert out.split(b"\n", 1)[1] == M.format_table({}, 1, 1) + b"".join(b"## " + l.encode() + b"\n" + M.format_table({}, 1, 1) for l in X.labels("snps,end", 2))


def test_window_fits_the_block(prog, tmp_path):
    """the window is as wide as the block's counters allow, at most the plain kernel's; -a 0 starts at score 0"""
    for dims, cap, rows in ((X.ALL, 0, 22), (X.ALL, 32, 70), ("end", 0, 2), ("snps", 1, 2)):
        for a in (0, 3):
            first = run(prog, tmp_path, "%s %d %d 1 32768 2048" % (dims, cap, a), []).split(b"\n")[0].split()
            win, lo = int(first[1]), int(first[2])
            assert int(first[4]) == rows and win == min(2048, 32768 // (rows * 5) - 1) and rows * 5 * (win + 1) <= 32768
            assert lo == (0 if a == 0 else -(win // 4))


@pytest.mark.parametrize("head", ["snps,mapq 0", "snps,snps 0", "snps, 0", ",snps 0", "snps 33", "end -1", "SNPS 0", "snp 0", "snpss 0"])
def test_refused(prog, tmp_path, head):
    assert run(prog, tmp_path, head + " 0 1 32768 2048", []).startswith(b"error: breakdown:")
