"""On the device: the truth SAM (dwgsim_hip_set_truth_sam, DWGSIM_HIP_STREAM_SAM, dwgsim_hip_job_set_truth_sam, DWGSIM_HIP_TRUTH_SAM) against the plain-Python
checker of tests/truth_sam_common.py -- the cases of tests/test_emu_truth_sam.py on api.load() and dwgsim_amd/dwgsim-hip -- and the loop closed through
dwgsim_eval-hip: scored as alignments, the truth is never wrong."""
import os

import pytest

import eval_model
import truth_sam_common as T
from dwgsim_amd import api
from hapfasta_common import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return api.load()


def test_placed_edits(lib, tmp_path):
    T.check_placed(lib, tmp_path)


@pytest.mark.parametrize("errors", [False, True], ids=["error-free", "default-errors"])
def test_random_walk(lib, errors):
    T.check_random_walk(lib, errors)


@pytest.mark.parametrize("which", T.SURFACE_IDS)
def test_option_surface(lib, tmp_path, which):
    T.check_surface(lib, tmp_path, which)


def test_batch_shapes(lib):
    T.check_batch_shapes(lib)


def test_levels(lib):
    T.check_levels(lib)


@pytest.mark.parametrize("gzip_mode", ["gpu", "cpu"])
def test_command_line(lib, tmp_path, gzip_mode):
    T.check_cli(lib, os.path.join(ROOT, "dwgsim_amd", "dwgsim-hip"), tmp_path, gzip_mode)


def test_errors(lib):
    T.check_errors(lib)


def _eval(lib, tmp_path, flags):
    contigs = [("evA", synth(81, 12000)), ("evB", synth(82, 8000))]
    res = T.run_ctx(lib, flags, contigs, group_bp=1 << 30)
    path = os.path.join(str(tmp_path), "truth.sam")
    with open(path, "wb") as f:
        f.write(api.truth_sam_header(contigs, lib) + res.truth_sam)
    table, summary = api.eval_sam(path)
    assert summary.status == 0, summary.stderr
    return res, path, table


def test_eval_scores_the_truth_as_never_wrong(lib, tmp_path):
    """-r 0 at the default -g 5: no record mapped incorrectly, and the unmapped ones are exactly the random reads"""
    res, path, table = _eval(lib, tmp_path, "-z 41 -r 0 -N 1500 -y 0.1")
    rows = [line.split() for line in table.decode().splitlines() if line and not line.startswith("#")]
    assert rows
    n_rand = sum(1 for line in res.truth_sam.decode().splitlines() if int(line.split("\t")[1]) & 4)
    assert n_rand > 0
    # a row (dwgsim_eval): thr, mc mi mu um uu and their total at the threshold, then mc' mi' mu' um' uu' and their total at or above it: the last row's hold everything
    last = [int(x) for x in rows[-1][:13]]
    mc, mi, mu, um, uu, total = last[7:13]
    assert (mc, mi, mu, um, uu, total) == (3000 - n_rand, 0, 0, 0, n_rand, 3000), last


def test_eval_table_equals_the_model_on_an_indel_run(lib, tmp_path):
    res, path, table = _eval(lib, tmp_path, "-z 43 -r 0.02 -R 0.3 -X 0.5 -N 1500")
    want = eval_model.run([open(path, "rb").read()])
    assert want.status == 0 and table == want.table
