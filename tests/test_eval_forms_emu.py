"""CPU-only: the three forms of dwgsim_eval-hip's record kernels behind both fronts agree with each other and with the plain-Python model in
everything that the shared record loop makes (eval_forms.py).  dw_eval.hip and dw_eval.cpp compiled against the SIMT emulation shim
(tests/emu/build_eval.sh).  Test infrastructure: the product has no CPU path."""
import os, subprocess
import pytest

import eval_forms as F
from dwgsim_amd import api

EMU = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")


@pytest.fixture(scope="module")
def lib():
    subprocess.run([os.path.join(EMU, "build_eval.sh")], check=True, stdout=subprocess.DEVNULL)
    return api.load_eval(os.path.join(EMU, "libdwgsim_eval_emu.so"))


@pytest.fixture(scope="module")
def sam():
    return F.sam_file()


@pytest.mark.parametrize("front", F.FRONTS)
def test_forms_agree(lib, sam, front):
    F.check_forms_agree(lib, front, sam)


@pytest.mark.parametrize("front", F.FRONTS)
@pytest.mark.parametrize("code", F.CODES)
def test_fatal_record(lib, sam, code, front):
    F.check_fatal_record(lib, front, sam, code)
