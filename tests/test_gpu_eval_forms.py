"""On the MI355X: the three forms of dwgsim_eval-hip's record kernels behind both fronts agree with each other and with the plain-Python model
in everything that the shared record loop makes (eval_forms.py), through the product library."""
import pytest

import eval_forms as F
from dwgsim_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sam():
    return F.sam_file()


@pytest.mark.parametrize("front", F.FRONTS)
def test_gpu_forms_agree(sam, front):
    F.check_forms_agree(api.load(), front, sam)


@pytest.mark.parametrize("front", F.FRONTS)
@pytest.mark.parametrize("code", F.CODES)
def test_gpu_fatal_record(sam, code, front):
    F.check_fatal_record(api.load(), front, sam, code)
