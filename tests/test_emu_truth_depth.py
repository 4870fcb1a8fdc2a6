"""CPU-only: the truth VCF and its counters (dwgsim_hip_set_truth_depth, dwgsim_hip_truth_depth_fetch, dwgsim_hip_mutlist_truth_vcf_text, dwgsim_hip_truth_vcf_header,
dwgsim_hip_job_set_truth_vcf_sink, DWGSIM_HIP_TRUTH_VCF) on the CPU emulation build of the product's own sources, against the plain-Python model of
tests/truth_depth_common.py.  tests/test_gpu_truth_depth.py runs the same cases on the device."""
import os
import subprocess

import pytest

import truth_depth_common as D
from dwgsim_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.run([os.path.join(HERE, "emu", "build.sh")], check=True, stdout=subprocess.DEVNULL)
    return api.load(os.path.join(HERE, "emu", "libdwgsim_emu.so"))


def test_model_on_written_out_cases():
    D.check_model()


@pytest.mark.parametrize("kind", list(D.WALK_KINDS))
def test_random_walk(emu_lib, kind):
    D.check_random_walk(emu_lib, kind)


def test_placed_edits(emu_lib, tmp_path):
    D.check_placed(emu_lib, tmp_path)


def test_random_reads(emu_lib):
    D.check_random_reads(emu_lib)


def test_regions(emu_lib, tmp_path):
    D.check_regions(emu_lib, tmp_path)


def test_listed_cell_without_a_record(emu_lib, tmp_path):
    D.check_non_acgt(emu_lib, tmp_path)


def test_contigs_resident_together(emu_lib):
    D.check_group(emu_lib)


def test_batches_and_contexts_add_up(emu_lib):
    D.check_batches(emu_lib)


def test_second_run_counts_once(emu_lib):
    D.check_rerun(emu_lib)


def test_without_the_truth_sam(emu_lib):
    D.check_alone(emu_lib)


def test_switched_off(emu_lib):
    D.check_off(emu_lib)


def test_job_level(emu_lib):
    D.check_levels(emu_lib)


def test_command_line(emu_lib, tmp_path):
    D.check_cli(emu_lib, os.path.join(HERE, "emu", "dwgsim-emu"), tmp_path, "cpu")
