"""CPU suite: the PRS window search and the coarse corrector (sync_find_body of k_sync.hip with sync_window.h, as compiled into k_sync_find,
k_sync_find_wide and k_sync_find_chain) on the execution model of tests/hipemu, case by case through dabphy_test_sync_find on the directed
inputs of tests/sync_cases.py, against the restatement's findIndex / processPRS on the same samples -- which tests/test_oracle_vs_ref.py
pins to the reference on the same inputs.  tests/test_gpu_sync.py runs the same cases on the device."""
import pytest

import parity_cases as P
from conftest import EMU_LIB
from welle_io_amd import capi


def factory(**kw):
    return capi.DabPhy(lib_path=EMU_LIB, **kw)


@pytest.mark.parametrize("kernel", ["serial", "wide", "chain"])
def test_sync_window_cases(emu, kernel):
    P.check_sync_cases_window(factory, kernel)


@pytest.mark.parametrize("kernel", ["serial", "wide", "chain"])
def test_sync_coarse_cases(emu, kernel):
    P.check_sync_cases_coarse(factory, kernel)


def test_sync_chain_two_frames(emu):
    P.check_sync_cases_two_frames(factory)


def test_sync_find_entry_errors(emu):
    P.check_sync_find_errors(factory)
