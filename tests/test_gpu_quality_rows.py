"""On the device: the quality line in the wave's staging rows (k_simulate's lockstep instances) against the oracle, byte for byte, with the row
buffer and with "qrows" = 0 -- the cases of tests/test_emu_quality_rows.py (tests/quality_rows.py), on api.load()."""
import pytest

import quality_rows as Q
from dwgsim_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return api.load()


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    return Q.write_fasta(tmp_path_factory.mktemp("quality_rows") / "three.fa")


@pytest.mark.parametrize("case", Q.CASES, ids=Q.CASE_IDS)
def test_case_against_the_oracle(lib, oracle_bin, fasta, case):
    Q.check_case(lib, oracle_bin, fasta, case)
