"""On the device: the truth VCF and its counters (dwgsim_hip_set_truth_depth, dwgsim_hip_truth_depth_fetch, dwgsim_hip_mutlist_truth_vcf_text,
dwgsim_hip_truth_vcf_header, dwgsim_hip_job_set_truth_vcf_sink, DWGSIM_HIP_TRUTH_VCF) against the plain-Python model of tests/truth_depth_common.py -- the cases of
tests/test_emu_truth_depth.py on api.load() and dwgsim_amd/dwgsim-hip."""
import os

import pytest

import truth_depth_common as D
from dwgsim_amd import api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return api.load()


@pytest.mark.parametrize("kind", list(D.WALK_KINDS))
def test_random_walk(lib, kind):
    D.check_random_walk(lib, kind)


def test_placed_edits(lib, tmp_path):
    D.check_placed(lib, tmp_path)


def test_random_reads(lib):
    D.check_random_reads(lib)


def test_regions(lib, tmp_path):
    D.check_regions(lib, tmp_path)


def test_listed_cell_without_a_record(lib, tmp_path):
    D.check_non_acgt(lib, tmp_path)


def test_contigs_resident_together(lib):
    D.check_group(lib)


def test_batches_and_contexts_add_up(lib):
    D.check_batches(lib)


def test_second_run_counts_once(lib):
    D.check_rerun(lib)


def test_without_the_truth_sam(lib):
    D.check_alone(lib)


def test_switched_off(lib):
    D.check_off(lib)


def test_job_level(lib):
    D.check_levels(lib)


@pytest.mark.parametrize("gzip_mode", ["gpu", "cpu"])
def test_command_line(lib, tmp_path, gzip_mode):
    D.check_cli(lib, os.path.join(ROOT, "dwgsim_amd", "dwgsim-hip"), tmp_path, gzip_mode)
