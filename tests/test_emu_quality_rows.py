"""CPU-only: the quality line in the wave's staging rows (k_simulate's lockstep instances, reads of 137 bases on) on the CPU emulation build of the
product's own sources, against the oracle byte for byte, with the row buffer and with "qrows" = 0 (tests/quality_rows.py: read lengths around the edge
at which the rows hold 72 bytes per lane, quality settings that fill the buffer to its last byte).  The 150- and 137-base cases run again with the
lanes of a block in reverse order and with the waves of a block apart, in shuffled order: the schedules under which a hand-over of the rows without a
point of reconvergence, or a write into another wave's rows, goes wrong (tests/emu/hip_emu.cpp).
tests/test_gpu_quality_rows.py runs the same cases on the device."""
import os
import subprocess

import pytest

import quality_rows as Q
from dwgsim_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.run([os.path.join(HERE, "emu", "build.sh")], check=True, stdout=subprocess.DEVNULL)
    return api.load(os.path.join(HERE, "emu", "libdwgsim_emu.so"))


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    return Q.write_fasta(tmp_path_factory.mktemp("quality_rows") / "three.fa")


@pytest.mark.parametrize("case", Q.CASES, ids=Q.CASE_IDS)
def test_case_against_the_oracle_on_cpu_emulation(emu_lib, oracle_bin, fasta, case):
    Q.check_case(emu_lib, oracle_bin, fasta, case)


@pytest.mark.parametrize("case", Q.SCHEDULED, ids=Q.SCHEDULED_IDS)
def test_row_lengths_with_the_lanes_in_reverse_order(emu_lib, oracle_bin, fasta, case, monkeypatch):
    monkeypatch.setenv("HIPEMU_REVERSE_LANES", "k_simulate")
    Q.check_case(emu_lib, oracle_bin, fasta, case)


@pytest.mark.parametrize("seed", ["1", "7"])
@pytest.mark.parametrize("case", Q.SCHEDULED, ids=Q.SCHEDULED_IDS)
def test_row_lengths_with_the_waves_apart_in_shuffled_order(emu_lib, oracle_bin, fasta, case, seed, monkeypatch):
    monkeypatch.setenv("HIPEMU_WAVES_APART", "all")
    monkeypatch.setenv("HIPEMU_WAVES_SEED", seed)
    Q.check_case(emu_lib, oracle_bin, fasta, case, batch_pairs=333)
