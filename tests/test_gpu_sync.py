"""GPU suite: the PRS window search and the coarse corrector on the device -- the three kernels that hold sync_find_body (k_sync_find,
k_sync_find_wide, k_sync_find_chain), case by case through dabphy_test_sync_find on the directed inputs of tests/sync_cases.py, against the
restatement's findIndex / processPRS on the same samples: exact integers, impulse responses bit for bit."""
import pytest

import parity_cases as P
from conftest import GPU_LIB
from welle_io_amd import capi

pytestmark = pytest.mark.gpu


def factory(**kw):
    return capi.DabPhy(lib_path=GPU_LIB, **kw)


@pytest.mark.parametrize("kernel", ["serial", "wide", "chain"])
def test_sync_window_cases(gpu, kernel):
    P.check_sync_cases_window(factory, kernel)


@pytest.mark.parametrize("kernel", ["serial", "wide", "chain"])
def test_sync_coarse_cases(gpu, kernel):
    P.check_sync_cases_coarse(factory, kernel)


def test_sync_chain_two_frames(gpu):
    P.check_sync_cases_two_frames(factory)


def test_sync_find_entry_errors(gpu):
    P.check_sync_find_errors(factory)
