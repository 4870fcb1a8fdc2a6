"""CPU-only: the truth SAM (dwgsim_hip_set_truth_sam, DWGSIM_HIP_STREAM_SAM, dwgsim_hip_job_set_truth_sam, DWGSIM_HIP_TRUTH_SAM) on the CPU emulation build of
the product's own sources, against the plain-Python checker of tests/truth_sam_common.py.  tests/test_gpu_truth_sam.py runs the same cases on the device."""
import os
import subprocess

import pytest

import truth_sam_common as T
from dwgsim_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.run([os.path.join(HERE, "emu", "build.sh")], check=True, stdout=subprocess.DEVNULL)
    return api.load(os.path.join(HERE, "emu", "libdwgsim_emu.so"))


def test_checker_on_written_out_cases():
    T.check_model()


def test_placed_edits(emu_lib, tmp_path):
    T.check_placed(emu_lib, tmp_path)


@pytest.mark.parametrize("errors", [False, True], ids=["error-free", "default-errors"])
def test_random_walk(emu_lib, errors):
    T.check_random_walk(emu_lib, errors)


@pytest.mark.parametrize("which", T.SURFACE_IDS)
def test_option_surface(emu_lib, tmp_path, which):
    T.check_surface(emu_lib, tmp_path, which)


def test_batch_shapes(emu_lib):
    T.check_batch_shapes(emu_lib)


def test_levels(emu_lib):
    T.check_levels(emu_lib)


def test_command_line(emu_lib, tmp_path):
    T.check_cli(emu_lib, os.path.join(HERE, "emu", "dwgsim-emu"), tmp_path, "cpu")


def test_errors(emu_lib):
    T.check_errors(emu_lib)
