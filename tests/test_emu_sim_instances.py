"""CPU-only: every k_simulate<LPP, OUT, DT, NTHR, WR, SPLIT> form on the CPU emulation build of the product's own sources against the oracle, byte for
byte and with the form of every launch read back; the instances the matrix covers against the library's own list; the host's choice of a form swept for
one that has no instance (tests/sim_instances.py).  tests/test_gpu_sim_instances.py runs the same on the device."""
import os
import subprocess

import pytest

import sim_instances as S
from dwgsim_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.run([os.path.join(HERE, "emu", "build.sh")], check=True, stdout=subprocess.DEVNULL)
    return api.load(os.path.join(HERE, "emu", "libdwgsim_emu.so"))


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    return S.write_fasta(tmp_path_factory.mktemp("sim_instances") / "three.fa")


@pytest.mark.parametrize("form", S.FORMS, ids=S.FORM_IDS)
def test_form_against_the_oracle_on_cpu_emulation(emu_lib, oracle_bin, fasta, form):
    S.check_form(emu_lib, oracle_bin, fasta, form)


def test_every_instance_is_compared_on_cpu_emulation(emu_lib):
    S.check_every_instance_is_compared(emu_lib)


def test_host_asks_only_for_instances_that_exist_on_cpu_emulation(emu_lib):
    S.check_host_asks_only_for_instances_that_exist(emu_lib)
