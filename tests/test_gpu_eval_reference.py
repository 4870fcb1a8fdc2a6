"""dwgsim_eval-hip on the MI355X against the recorded answers of the UNMODIFIED reference evaluator (tests/golden/eval_reference_runs.json,
cases of eval_reference_cases.py): table (by hash, and by text where stored), exit status and stderr of every synthetic, multi-file, fatal
and BAM case through api.eval_sam / api.eval_bam, a dozen of them through the command line (files and stdin), and the single-record runs on
awkward names through the API.  Nothing here runs or reads the reference.  The plain kernels at the chunk sizes of test_gpu_eval.py."""
import io, os, subprocess
import pytest

import eval_model as M
import eval_reference_cases as R
from dwgsim_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dwgsim_amd", "dwgsim_eval-hip")
pytestmark = pytest.mark.gpu
CASES = sorted(R.cases())
SINGLES = R.single_ids()
BLOCK = 200          # contexts per test function


def model_table(cid):
    c = R.cases()[cid]
    return M.run([R.model_text(f) for f in c["files"]], R.model_opts(c["opts"])).table


@pytest.mark.parametrize("k", range(len(CASES)), ids=CASES)
def test_gpu_eval_gives_the_reference_answer(k):
    cid = CASES[k]
    c = R.cases()[cid]
    run = api.eval_bam if R.is_bam(c["files"][0]) else api.eval_sam
    table, sm = run([io.BytesIO(R.inputs()[f]) for f in c["files"]], chunk_bytes=(64 << 10) if k % 2 else 0, read_bytes=1 << 20, **c["opts"])
    R.check_answer(cid, R.recorded(cid), sm.status, sm.stderr, table, lambda: model_table(cid))
    if c["fatal"]:
        assert sm.error_code == R.FATAL_CODE[c["fatal"]]


def true_n_case(name):
    return next(c for c in CASES if c.startswith("synth/%s/n" % name) and not c.endswith("/n12345"))


# case id, index of the file that goes through stdin (or None)
CLI_CASES = [("synth/paired/default", None), ("synth/paired/m1_p1_q10", None), ("synth/single/a3", 0), ("synth/prefix/a3_d3", None),
             ("synth/wide/a3_d-2", None), (true_n_case("paired"), 0), ("multi/straddle_m", 1), ("multi/other_sq_p", None),
             ("fatal/name/middle", None), ("fatal/not_paired/last", 0), ("bam/paired_b700/a3_m1_p1", None), ("bam/aux/a3_d2_p1", 0),
             ("bam/straddle_m", None)]


@pytest.mark.parametrize("cid,stdin", CLI_CASES, ids=[c for c, _ in CLI_CASES])
def test_gpu_eval_cli_gives_the_reference_answer(tmp_path, cid, stdin):
    c = R.cases()[cid]
    paths = []
    for k, f in enumerate(c["files"]):
        if k == stdin:
            paths.append("-")
        else:
            p = tmp_path / ("%d_%s" % (k, f)); p.write_bytes(R.inputs()[f]); paths.append(str(p))
    args = R.argv(c["opts"], not R.is_bam(c["files"][0]))
    p = subprocess.run(["timeout", "-k", "10", "300", CLI] + args + paths, input=R.inputs()[c["files"][stdin]] if stdin is not None else b"",
                       capture_output=True, timeout=320)
    if p.returncode:
        assert p.stdout == b""
    elif c["opts"].get("p"):
        assert p.stdout.startswith(M.split_header(R.model_text(c["files"][0]))[0])
    R.check_answer(cid, R.recorded(cid), p.returncode, p.stderr, R.table_part(p.stdout), lambda: model_table(cid))


@pytest.mark.parametrize("b", range((len(SINGLES) + BLOCK - 1) // BLOCK))
def test_gpu_eval_gives_the_reference_answer_on_single_records(b):
    for cid in SINGLES[b * BLOCK:(b + 1) * BLOCK]:
        _, name, k = cid.split("/")
        o = R.SINGLE_OPTS[name]
        data = R.single_input(int(k))
        table, sm = api.eval_sam([io.BytesIO(data)], chunk_bytes=4096, **o)
        R.check_answer(cid, R.recorded(cid), sm.status, sm.stderr, table, lambda: M.run([data], R.model_opts(o)).table)
