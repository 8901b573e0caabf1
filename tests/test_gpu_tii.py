"""GPU suite: the TII kernels (k_tii_measure, k_tii_accumulate) on the device, driven pair by pair through dabphy_test_tii_pairs,
against the TIIDecoder restatement on the same (NULL, PRS) pairs: all 24 x 70 comb/pattern pairs and every branch of the decoder."""
import pytest

import parity_cases as P
from conftest import GPU_LIB
from welle_io_amd import capi

pytestmark = pytest.mark.gpu


def factory(**kw):
    return capi.DabPhy(lib_path=GPU_LIB, **kw)


def test_tii_pairs_every_pair(gpu):
    P.check_tii_pairs_every_pair(factory, full=True)


def test_tii_pairs_likely_limit(gpu):
    P.check_tii_pairs_likely_limit(factory)


def test_tii_pairs_slot_exhaustion(gpu):
    P.check_tii_pairs_slot_exhaustion(factory)


def test_tii_pairs_ties(gpu):
    P.check_tii_pairs_ties(factory)


def test_tii_pairs_scaled(gpu):
    P.check_tii_pairs_scaled(factory)


def test_tii_pairs_small_output(gpu):
    P.check_tii_pairs_small_output(factory)
