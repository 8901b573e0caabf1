"""Device suite: the wideband front end (one capture channelised into the batch's ensembles) against the float64 model of
tests/wideband_model.py and, end to end, against the oracle on each ensemble's direct stream.  Cases: tests/wideband_cases.py."""
import pytest

import wideband_cases as W
from conftest import GPU_LIB
from welle_io_amd import capi

pytestmark = pytest.mark.gpu


def factory(**kw):
    return capi.DabPhy(lib_path=GPU_LIB, **kw)


@pytest.mark.parametrize("D,n_taps", W.SHAPES)
def test_filter_and_oscillator_vs_model(gpu, D, n_taps):
    W.check_filter_vs_model(factory, D, n_taps, "u8")


@pytest.mark.parametrize("fmt", [f for f in W.FORMATS if f != "u8"])
def test_sample_formats_vs_model(gpu, fmt):
    W.check_filter_vs_model(factory, 4, 64, fmt)


def test_chunking_is_bit_identical(gpu):
    W.check_chunking(factory)


def test_phase_over_a_long_run(gpu):
    W.check_phase_long_run(factory)


def test_ring_wrap(gpu):
    W.check_ring_wrap(factory)


def test_reset_keeps_the_configuration_and_clears_the_carry(gpu):
    W.check_reset(factory)


def test_limits_and_state_errors(gpu):
    W.check_errors(factory)


def test_end_to_end_vs_oracle_on_the_direct_streams(gpu):
    W.check_end_to_end(factory, D=4, offsets=(-107, 0, 107))
