"""On the device: the chain files (dwgsim_hip_haplotype_chain / dwgsim_hip_chain_blocks / dwgsim_hip_chain_format, dwgsim_hip_job_set_chain_sink,
DWGSIM_HIP_CHAIN) against the plain-Python model of tests/chain_common.py, the haplotype FASTA and the truth SAM -- the cases of
tests/test_emu_chain.py, on api.load() and dwgsim_amd/dwgsim-hip."""
import os

import pytest

import chain_common as K
from dwgsim_amd import api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return api.load()


def test_formatter(lib):
    K.check_formatter(lib)


def test_unmutated_contigs(lib):
    K.check_unmutated(lib)


def test_placed_edits(lib, tmp_path):
    K.check_placed_edits(lib, tmp_path)


def test_placed_edits_second_case(lib, tmp_path):
    K.check_placed_edits_2(lib, tmp_path)


@pytest.mark.parametrize("flags", K.WALKS, ids=K.WALK_IDS)
def test_random_walk_against_mutations_txt(lib, flags):
    K.check_random_walk(lib, flags)


@pytest.mark.parametrize("flags", K.H.RANDOM_WALKS, ids=["substitutions", "indels"])
def test_chain_against_haplotype_fasta(lib, flags):
    K.check_against_fasta(lib, flags)


@pytest.mark.parametrize("haploid", [False, True], ids=["diploid", "haploid"])
def test_chain_against_truth_sam(lib, haploid):
    K.check_against_truth_sam(lib, haploid)


def test_job_level_equals_context_level(lib, tmp_path):
    K.check_levels(lib, tmp_path)


def test_command_line(lib, tmp_path):
    K.check_cli(lib, os.path.join(ROOT, "dwgsim_amd", "dwgsim-hip"), tmp_path, "gpu")


def test_argument_and_state_errors(lib):
    K.check_errors(lib)
