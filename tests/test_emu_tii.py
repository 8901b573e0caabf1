"""CPU suite: the TII kernels (k_tii_measure, k_tii_accumulate) compiled for tests/hipemu, driven pair by pair through
dabphy_test_tii_pairs, against the TIIDecoder restatement on the same (NULL, PRS) pairs -- which tests/test_oracle_vs_ref.py pins to the
real class on the same sets.  tests/test_gpu_tii.py runs the same cases on the device."""
import os

import pytest

import parity_cases as P
from conftest import EMU_LIB
from welle_io_amd import capi


def factory(**kw):
    return capi.DabPhy(lib_path=EMU_LIB, **kw)


def test_tii_pairs_every_comb_and_pattern(emu):
    """every comb, every pattern and the two pairs at the ends of the rotator table; the device suite sweeps all 1 680 pairs"""
    P.check_tii_pairs_every_pair(factory, full=False)


@pytest.mark.skipif(not os.environ.get("DABPHY_FULL_CPU_SUITE"), reason="the device twin sweeps all 1 680 pairs (-m gpu); DABPHY_FULL_CPU_SUITE=1 runs them here too")
def test_tii_pairs_every_pair(emu):
    P.check_tii_pairs_every_pair(factory, full=True)


def test_tii_pairs_likely_limit(emu):
    P.check_tii_pairs_likely_limit(factory)


def test_tii_pairs_slot_exhaustion(emu):
    P.check_tii_pairs_slot_exhaustion(factory)


def test_tii_pairs_ties(emu):
    P.check_tii_pairs_ties(factory)


def test_tii_pairs_scaled(emu):
    P.check_tii_pairs_scaled(factory)


def test_tii_pairs_small_output(emu):
    P.check_tii_pairs_small_output(factory)


def test_tii_pairs_entry_needs_the_side_path(emu):
    """dabphy_test_tii_pairs without dabphy_set_tii(h, 1), with more frames than max_frames or another ensemble count: the usual error code"""
    nul, prs, want = P.tii_set_scaled()
    d = factory(n_ensembles=1, max_frames=2, want_constellation=False, want_impulse_response=False)
    try:
        with pytest.raises(capi.DabPhyError):
            d.test_tii_pairs(nul[:1, :2], prs[:1, :2])
        d.set_tii(True)
        d.test_tii_pairs(nul[:1, :2], prs[:1, :2])
        with pytest.raises(capi.DabPhyError):
            d.test_tii_pairs(nul[:1, :3], prs[:1, :3])
        d.set_tii(False)
        with pytest.raises(capi.DabPhyError):
            d.test_tii_pairs(nul[:1, :2], prs[:1, :2])
    finally:
        d.close()
