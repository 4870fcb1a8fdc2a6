"""On the device: the NM and MD tags of the truth SAM (dwgsim_hip_set_truth_md, dwgsim_hip_job_set_truth_md, DWGSIM_HIP_TRUTH_MD) against the plain-Python
checker of tests/truth_md_common.py -- the cases of tests/test_emu_truth_md.py on api.load() and dwgsim_amd/dwgsim-hip -- and dwgsim_eval-hip, which must not
see the tags."""
import os

import pytest

import truth_md_common as M
from dwgsim_amd import api
from hapfasta_common import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    lib = api.load()
    assert hasattr(lib, "dwgsim_hip_set_truth_md") and hasattr(lib, "dwgsim_hip_job_set_truth_md")
    return lib


def test_checker_on_written_out_cases(lib):
    M.check_model()


def test_placed_edits(lib, tmp_path):
    M.check_placed(lib, tmp_path)


def test_reference_with_n_and_gap(lib):
    M.check_ref_n(lib)


@pytest.mark.parametrize("errors", [False, True], ids=["error-free", "default-errors"])
def test_random_walk(lib, errors):
    M.check_random_walk(lib, errors)


@pytest.mark.parametrize("which", M.SURFACE_IDS)
def test_option_surface(lib, tmp_path, which):
    M.check_surface(lib, tmp_path, which)


def test_batch_shapes(lib):
    M.check_batch_shapes(lib)


def test_second_run_forced(lib):
    M.check_second_run_forced(lib)


def test_second_run_leaves_no_trace(lib):
    M.check_second_run_leaves_no_trace(lib)


def test_second_run_with_gzip(lib):
    M.check_second_run_gzip(lib)


def test_second_run_natural(lib, tmp_path):
    M.check_second_run_natural(lib, tmp_path)


def test_levels(lib):
    M.check_levels(lib)


@pytest.mark.parametrize("gzip_mode", ["gpu", "cpu"])
def test_command_line(lib, tmp_path, gzip_mode):
    M.check_cli(lib, os.path.join(ROOT, "dwgsim_amd", "dwgsim-hip"), tmp_path, gzip_mode)


def test_errors(lib):
    M.check_errors(lib)


def test_eval_ignores_the_tags(lib, tmp_path):
    """api.eval_sam on a tagged truth SAM gives the table of the untagged one"""
    contigs = [("evA", synth(81, 12000)), ("evB", synth(82, 8000))]
    tagged, plain, st = M.run_pair(lib, "-z 43 -r 0.02 -R 0.3 -X 0.5 -N 1500 -y 0.05", contigs, group_bp=1 << 30)
    tables = []
    for tag, res in (("tagged", tagged), ("plain", plain)):
        path = os.path.join(str(tmp_path), tag + ".sam")
        with open(path, "wb") as f:
            f.write(api.truth_sam_header(contigs, lib) + res.truth_sam)
        table, summary = api.eval_sam(path)
        assert summary.status == 0, summary.stderr
        tables.append(table)
    assert tables[0] == tables[1] and tables[0] and st.mapped > 0 and st.mapped < st.records
