"""CPU-only: the lockstep sequence line of k_simulate's FIFO instances on the CPU emulation build of the product's own sources, against the oracle byte
for byte (tests/text_bursts.py: read lengths on every edge of the cut into head, units and tail; record starts on every byte phase).  The 150-base
cases run again with the lanes of a block in reverse order and with the waves of a block apart, in shuffled order: the schedules under which code
that counts on a lock step no wave operation enforces, or on another wave's LDS, goes wrong (tests/emu/hip_emu.cpp).
tests/test_gpu_text_bursts.py runs the same cases on the device."""
import os
import subprocess

import pytest

import text_bursts as T
from dwgsim_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.run([os.path.join(HERE, "emu", "build.sh")], check=True, stdout=subprocess.DEVNULL)
    return api.load(os.path.join(HERE, "emu", "libdwgsim_emu.so"))


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    return T.write_fasta(tmp_path_factory.mktemp("text_bursts") / "three.fa")


@pytest.mark.parametrize("case", T.CASES, ids=T.CASE_IDS)
def test_case_against_the_oracle_on_cpu_emulation(emu_lib, oracle_bin, fasta, case):
    T.check_case(emu_lib, oracle_bin, fasta, case)


@pytest.mark.parametrize("case", T.HEADLINE, ids=T.HEADLINE_IDS)
def test_headline_lengths_with_the_lanes_in_reverse_order(emu_lib, oracle_bin, fasta, case, monkeypatch):
    monkeypatch.setenv("HIPEMU_REVERSE_LANES", "k_simulate")
    T.check_case(emu_lib, oracle_bin, fasta, case, batch_pairs=333)


@pytest.mark.parametrize("seed", ["1", "7"])
@pytest.mark.parametrize("case", T.HEADLINE, ids=T.HEADLINE_IDS)
def test_headline_lengths_with_the_waves_apart_in_shuffled_order(emu_lib, oracle_bin, fasta, case, seed, monkeypatch):
    monkeypatch.setenv("HIPEMU_WAVES_APART", "all")
    monkeypatch.setenv("HIPEMU_WAVES_SEED", seed)
    T.check_case(emu_lib, oracle_bin, fasta, case, batch_pairs=333)
