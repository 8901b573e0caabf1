"""Device suite: the wideband front end (one capture channelised into the batch's ensembles) against the float64 model of
tests/wideband_model.py and, end to end, against the oracle on each ensemble's direct stream.  Cases: tests/frontend_cases.py."""
import pytest

import frontend_cases as F
from conftest import GPU_LIB
from welle_io_amd import capi

pytestmark = pytest.mark.gpu

K = F.INTEGER                           # the kind's default shapes


def factory(**kw):
    return capi.DabPhy(lib_path=GPU_LIB, **kw)


@pytest.mark.parametrize("D,n_taps", F.INTEGER_SHAPES)
def test_filter_and_oscillator_vs_model(gpu, D, n_taps):
    F.check_filter_vs_model(factory, F.Integer(D), n_taps, "u8")


@pytest.mark.parametrize("fmt", [f for f in F.FORMATS if f != "u8"])
def test_sample_formats_vs_model(gpu, fmt):
    F.check_filter_vs_model(factory, K["rate"], K["n_taps"], fmt)


def test_chunking_is_bit_identical(gpu):
    F.check_chunking(factory, K["rate"], K["n_taps"])


def test_phase_over_a_long_run(gpu):
    F.check_phase_long_run(factory, **K["long_run"])


def test_ring_wrap(gpu):
    F.check_ring_wrap(factory, **K["wrap"])


def test_reset_keeps_the_configuration_and_clears_the_carry(gpu):
    F.check_reset(factory, K["rate"], K["n_taps"], K["reset_n1"])


def test_limits_and_state_errors(gpu):
    F.check_errors(factory, K["rate"], K["n_taps"])


def test_end_to_end_vs_oracle_on_the_direct_streams(gpu):
    F.check_end_to_end(factory, F.Integer(4), offsets=(-107, 0, 107))
