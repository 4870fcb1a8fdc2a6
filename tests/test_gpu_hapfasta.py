"""On the device: the haplotype FASTA (dwgsim_hip_haplotype_fasta / _layout / _fetch, dwgsim_hip_job_set_haplotype_sink, DWGSIM_HIP_HAPLOTYPES) against
the plain-Python model of tests/hapfasta_common.py -- the cases of tests/test_emu_hapfasta.py, on api.load() and dwgsim_amd/dwgsim-hip."""
import os

import pytest

import hapfasta_common as H
from dwgsim_amd import api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return api.load()


def test_unmutated_layout(lib):
    H.check_layout(lib)


def test_placed_edits(lib, tmp_path):
    H.check_placed_edits(lib, tmp_path)


@pytest.mark.parametrize("flags", H.RANDOM_WALKS, ids=["substitutions", "indels"])
def test_random_walk_against_mutations_txt(lib, flags):
    H.check_random_walk(lib, flags)


@pytest.mark.parametrize("haploid", [False, True], ids=["diploid", "haploid"])
def test_reads_come_from_the_written_genomes(lib, haploid):
    H.check_reads(lib, haploid)


def test_job_level_equals_context_level(lib, tmp_path):
    H.check_levels(lib, tmp_path)


def test_command_line(lib, tmp_path):
    H.check_cli(lib, os.path.join(ROOT, "dwgsim_amd", "dwgsim-hip"), tmp_path, "gpu")


def test_argument_and_state_errors(lib):
    H.check_errors(lib)
