"""CPU-only: the haplotype FASTA (dwgsim_hip_haplotype_fasta / _layout / _fetch, dwgsim_hip_job_set_haplotype_sink, DWGSIM_HIP_HAPLOTYPES) on the CPU
emulation build of the product's own sources, against the plain-Python model of tests/hapfasta_common.py.  tests/test_gpu_hapfasta.py runs the
same cases on the device."""
import os
import subprocess

import pytest

import hapfasta_common as H
from dwgsim_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.run([os.path.join(HERE, "emu", "build.sh")], check=True, stdout=subprocess.DEVNULL)
    return api.load(os.path.join(HERE, "emu", "libdwgsim_emu.so"))


def test_model_wraps_and_applies_edits():
    """the model itself, on cases small enough to write out"""
    assert H.wrap("x", "ACGTA", 2) == b">x\nAC\nGT\nA\n" and H.wrap("x", "ACGT", 2) == b">x\nAC\nGT\n" and H.wrap("x", "ACGT", 0) == b">x\nACGT\n" and H.wrap("x", "", 7) == b">x\n"
    ref = "ACGTN"
    edits = [(0, "S", "T", 3), (1, "D", "", 1), (2, "I", "AA", 2), (4, "I", "C", 3)]
    assert H.apply_edits(ref, edits, 0) == "TGTNC" and H.apply_edits(ref, edits, 1) == "TCGAATNC"
    txt = H.edits_to_txt("c", "ACGTA", [(0, "S", "T", 3), (1, "S", "G", 2), (2, "D", "", 1), (3, "I", "AC", 3)])
    assert txt == "c\t1\tA\tT\t3\nc\t2\tC\tS\t2\nc\t3\tG\t-\t1\nc\t4\t-\tAC\t3\n"
    assert H.parse_mutations_txt(txt.encode()) == {"c": [(0, "S", "T", 3), (1, "S", "G", 2), (2, "D", "", 1), (3, "I", "AC", 3)]}
    assert H.normalise(b"acgtRn-.") == "ACGTNNNN" and H.revcomp("AACGN") == "NCGTT"


def test_unmutated_layout(emu_lib):
    H.check_layout(emu_lib)


def test_placed_edits(emu_lib, tmp_path):
    H.check_placed_edits(emu_lib, tmp_path)


@pytest.mark.parametrize("flags", H.RANDOM_WALKS, ids=["substitutions", "indels"])
def test_random_walk_against_mutations_txt(emu_lib, flags):
    H.check_random_walk(emu_lib, flags)


@pytest.mark.parametrize("haploid", [False, True], ids=["diploid", "haploid"])
def test_reads_come_from_the_written_genomes(emu_lib, haploid):
    H.check_reads(emu_lib, haploid)


def test_job_level_equals_context_level(emu_lib, tmp_path):
    H.check_levels(emu_lib, tmp_path)


def test_command_line(emu_lib, tmp_path):
    H.check_cli(emu_lib, os.path.join(HERE, "emu", "dwgsim-emu"), tmp_path, "cpu")


def test_argument_and_state_errors(emu_lib):
    H.check_errors(emu_lib)
