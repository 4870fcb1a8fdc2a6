"""CPU-only: the chain files (dwgsim_hip_haplotype_chain / dwgsim_hip_chain_blocks / dwgsim_hip_chain_format, dwgsim_hip_job_set_chain_sink,
DWGSIM_HIP_CHAIN) on the CPU emulation build of the product's own sources, against the plain-Python model of tests/chain_common.py, the haplotype FASTA
and the truth SAM.  tests/test_gpu_chain.py runs the same cases on the device."""
import os
import subprocess

import pytest

import chain_common as K
from dwgsim_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.run([os.path.join(HERE, "emu", "build.sh")], check=True, stdout=subprocess.DEVNULL)
    return api.load(os.path.join(HERE, "emu", "libdwgsim_emu.so"))


def test_model_on_the_worked_example():
    K.check_model()


def test_formatter(emu_lib):
    K.check_formatter(emu_lib)


def test_unmutated_contigs(emu_lib):
    K.check_unmutated(emu_lib)


def test_placed_edits(emu_lib, tmp_path):
    K.check_placed_edits(emu_lib, tmp_path)


def test_placed_edits_second_case(emu_lib, tmp_path):
    K.check_placed_edits_2(emu_lib, tmp_path)


@pytest.mark.parametrize("flags", K.WALKS, ids=K.WALK_IDS)
def test_random_walk_against_mutations_txt(emu_lib, flags):
    K.check_random_walk(emu_lib, flags)


@pytest.mark.parametrize("flags", K.H.RANDOM_WALKS, ids=["substitutions", "indels"])
def test_chain_against_haplotype_fasta(emu_lib, flags):
    K.check_against_fasta(emu_lib, flags)


@pytest.mark.parametrize("haploid", [False, True], ids=["diploid", "haploid"])
def test_chain_against_truth_sam(emu_lib, haploid):
    K.check_against_truth_sam(emu_lib, haploid)


def test_job_level_equals_context_level(emu_lib, tmp_path):
    K.check_levels(emu_lib, tmp_path)


def test_command_line(emu_lib, tmp_path):
    K.check_cli(emu_lib, os.path.join(HERE, "emu", "dwgsim-emu"), tmp_path, "cpu")


def test_argument_and_state_errors(emu_lib):
    K.check_errors(emu_lib)
