"""The evaluator's anchor: the plain-Python model (eval_model.py) and the emulated kernels (dw_eval.hip and dw_eval.cpp on the SIMT emulation
shim) must give what the UNMODIFIED reference evaluator gave on every case of eval_reference_cases.py -- table (by hash, and by text where it
is stored), exit status and stderr.  The reference's answers are read from tests/golden/eval_reference_runs.json
(tests/golden/make_eval_reference_runs.py wrote them from oracle/_ref/dwgsim_eval), so nothing here needs the reference; where its binary has
been built, one test runs it again on every case so that the record cannot go stale.  CPU only."""
import io, os, subprocess, sys
import pytest

import eval_model as M
import eval_reference_cases as R
from dwgsim_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
CASES = sorted(R.cases())


@pytest.fixture(scope="module")
def lib():
    subprocess.run([os.path.join(EMU, "build_eval.sh")], check=True, stdout=subprocess.DEVNULL)
    return api.load_eval(os.path.join(EMU, "libdwgsim_eval_emu.so"))


def model(cid):
    c = R.cases()[cid]
    return M.run([R.model_text(f) for f in c["files"]], R.model_opts(c["opts"]))


def emu(lib, files, o, bam):
    run = api.eval_bam if bam else api.eval_sam
    table, sm = run([io.BytesIO(f) for f in files], lib=lib, chunk_bytes=4096, read_bytes=1000, **o)
    return sm.status, sm.stderr, table


def test_case_list_and_record_are_the_same_set():
    rec = R.record()
    assert set(rec["runs"]) == set(R.cases()), sorted(set(rec["runs"]) ^ set(R.cases()))
    s = rec["single"]
    assert set(s["options"]) == set(R.SINGLE_OPTS) == set(s["index"])
    assert s["options"] == {name: R.argv(o, True) for name, o in R.SINGLE_OPTS.items()}
    n = len(R.awkward()[1])
    assert n >= 400 and s["records"] == n and all(len(v) == n for v in s["index"].values())
    assert all(0 <= i < len(s["answers"]) for v in s["index"].values() for i in v)
    for cid, c in R.cases().items():
        assert rec["runs"][cid]["files"] == c["files"]
        assert rec["runs"][cid]["args"] == R.argv(c["opts"], not R.is_bam(c["files"][0])) + c["files"], cid


def test_inputs_are_the_recorded_ones():
    """the inputs are made again from seeds; a changed writer changes them, and then the record has to be made again (never a skip)"""
    rec = R.record()
    got = {name: R.sha256(data) for name, data in R.inputs().items()}
    changed = sorted(k for k in set(got) | set(rec["inputs"]) if got.get(k) != rec["inputs"].get(k))
    assert not changed, "inputs differ from the recorded ones, run tests/golden/make_eval_reference_runs.py again: %s" % changed
    assert R.sha256(R.join(*R.awkward())) == rec["single"]["sha256"], "awkward.sam changed: run make_eval_reference_runs.py again"
    assert R.join(*R.awkward()) == R.awkward_sam(), "awkward.sam is not what the case list writes: run make_eval_reference_runs.py again"


def test_the_record_covers_what_it_should():
    rec = R.record()
    for key, code in R.FATAL_CODE.items():
        for where in ("first", "middle", "last"):
            r = rec["runs"]["fatal/%s/%s" % (key, where)]
            assert r["rc"] == 1 and M.ERR_TEXT[code][1] in r["stderr"] and "stdout_sha256" not in r
    assert all(r["rc"] == 0 for cid, r in rec["runs"].items() if not cid.startswith("fatal/"))
    ans = rec["single"]["answers"]
    assert {a["rc"] for a in ans} == {0, 1}
    assert any(M.ERR_TEXT[M.E_NAME][1] in a["stderr"] for a in ans) and any(M.ERR_TEXT[M.E_CONTIG][1] in a["stderr"] for a in ans)
    assert os.path.getsize(R.RECORD) < 300_000


@pytest.mark.parametrize("cid", CASES)
def test_model_gives_the_reference_answer(cid):
    want = model(cid)
    R.check_answer(cid, R.recorded(cid), want.status, want.stderr, want.table if not want.status else b"")
    if R.cases()[cid]["fatal"]:
        assert want.error_code == R.FATAL_CODE[R.cases()[cid]["fatal"]]


@pytest.mark.parametrize("name", list(R.SINGLE_OPTS))
def test_model_gives_the_reference_answer_on_single_records(name):
    o = R.model_opts(R.SINGLE_OPTS[name])
    for k in range(len(R.awkward()[1])):
        cid = "single/%s/%d" % (name, k)
        want = M.run([R.single_input(k)], o)
        R.check_answer(cid, R.recorded(cid), want.status, want.stderr, want.table if not want.status else b"")


@pytest.mark.parametrize("cid", CASES)
def test_emulated_kernels_give_the_reference_answer(lib, cid):
    c = R.cases()[cid]
    status, stderr, table = emu(lib, [R.inputs()[f] for f in c["files"]], c["opts"], R.is_bam(c["files"][0]))
    R.check_answer(cid, R.recorded(cid), status, stderr, table, lambda: model(cid).table)


@pytest.mark.parametrize("name", list(R.SINGLE_OPTS))
def test_emulated_kernels_give_the_reference_answer_on_single_records(lib, name):
    o = R.SINGLE_OPTS[name]
    for k in range(len(R.awkward()[1])):
        cid = "single/%s/%d" % (name, k)
        status, stderr, table = emu(lib, [R.single_input(k)], o, False)
        R.check_answer(cid, R.recorded(cid), status, stderr, table, lambda: M.run([R.single_input(k)], R.model_opts(o)).table)


@pytest.mark.skipif(not os.path.exists(R.REF_EVAL), reason="oracle/_ref/dwgsim_eval is not built here (the reference sources are absent)")
def test_reference_still_answers_as_recorded():
    sys.path.insert(0, R.GOLD)
    try:
        import make_eval_reference_runs as rec
    finally:
        sys.path.remove(R.GOLD)
    diff = rec.differences(R.record(), rec.make())
    assert not diff, "the reference no longer answers as recorded: %s" % diff[:20]
