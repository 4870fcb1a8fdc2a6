"""On the device: every k_simulate<LPP, OUT, DT, NTHR, WR, SPLIT> form against the oracle, byte for byte and with the form of every launch read back; the
instances the matrix covers against the library's own list; the host's choice of a form swept for one that has no instance -- the cases of
tests/test_emu_sim_instances.py (tests/sim_instances.py), on api.load()."""
import pytest

import sim_instances as S
from dwgsim_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return api.load()


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    return S.write_fasta(tmp_path_factory.mktemp("sim_instances") / "three.fa")


@pytest.mark.parametrize("form", S.FORMS, ids=S.FORM_IDS)
def test_form_against_the_oracle(lib, oracle_bin, fasta, form):
    S.check_form(lib, oracle_bin, fasta, form)


def test_every_instance_is_compared(lib):
    S.check_every_instance_is_compared(lib)


def test_host_asks_only_for_instances_that_exist(lib):
    S.check_host_asks_only_for_instances_that_exist(lib)
