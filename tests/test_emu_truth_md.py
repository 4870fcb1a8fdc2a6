"""CPU-only: the NM and MD tags of the truth SAM (dwgsim_hip_set_truth_md, dwgsim_hip_job_set_truth_md, DWGSIM_HIP_TRUTH_MD) on the CPU emulation build of the
product's own sources, against the plain-Python checker of tests/truth_md_common.py.  tests/test_gpu_truth_md.py runs the same cases on the device."""
import os
import subprocess

import pytest

import truth_md_common as M
from dwgsim_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.run([os.path.join(HERE, "emu", "build.sh")], check=True, stdout=subprocess.DEVNULL)
    lib = api.load(os.path.join(HERE, "emu", "libdwgsim_emu.so"))
    assert hasattr(lib, "dwgsim_hip_set_truth_md") and hasattr(lib, "dwgsim_hip_job_set_truth_md")
    return lib


def test_checker_on_written_out_cases(emu_lib):
    M.check_model()


def test_placed_edits(emu_lib, tmp_path):
    M.check_placed(emu_lib, tmp_path)


def test_reference_with_n_and_gap(emu_lib):
    M.check_ref_n(emu_lib)


@pytest.mark.parametrize("errors", [False, True], ids=["error-free", "default-errors"])
def test_random_walk(emu_lib, errors):
    M.check_random_walk(emu_lib, errors)


@pytest.mark.parametrize("which", M.SURFACE_IDS)
def test_option_surface(emu_lib, tmp_path, which):
    M.check_surface(emu_lib, tmp_path, which)


def test_batch_shapes(emu_lib):
    M.check_batch_shapes(emu_lib)


def test_second_run_forced(emu_lib):
    M.check_second_run_forced(emu_lib)


def test_second_run_leaves_no_trace(emu_lib):
    M.check_second_run_leaves_no_trace(emu_lib)


def test_second_run_with_gzip(emu_lib):
    M.check_second_run_gzip(emu_lib)


def test_second_run_natural(emu_lib, tmp_path):
    M.check_second_run_natural(emu_lib, tmp_path)


def test_levels(emu_lib):
    M.check_levels(emu_lib)


def test_command_line(emu_lib, tmp_path):
    M.check_cli(emu_lib, os.path.join(HERE, "emu", "dwgsim-emu"), tmp_path, "cpu")


def test_errors(emu_lib):
    M.check_errors(emu_lib)
