"""On the device: the lockstep sequence line of k_simulate's FIFO instances against the oracle, byte for byte -- the cases of
tests/test_emu_text_bursts.py (tests/text_bursts.py), on api.load()."""
import pytest

import text_bursts as T
from dwgsim_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return api.load()


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    return T.write_fasta(tmp_path_factory.mktemp("text_bursts") / "three.fa")


@pytest.mark.parametrize("case", T.CASES, ids=T.CASE_IDS)
def test_case_against_the_oracle(lib, oracle_bin, fasta, case):
    T.check_case(lib, oracle_bin, fasta, case)
