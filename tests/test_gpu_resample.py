"""Device suite: the wideband front end at a rational rate (one capture at 2.048 MS/s x M / L resampled into the batch's ensembles)
against the float64 model of tests/resample_model.py and, end to end, against the oracle on each ensemble's direct stream.
Cases: tests/resample_cases.py."""
import pytest

import resample_cases as RC
from conftest import GPU_LIB
from welle_io_amd import capi

pytestmark = pytest.mark.gpu


def factory(**kw):
    return capi.DabPhy(lib_path=GPU_LIB, **kw)


@pytest.mark.parametrize("L,M,n_taps", RC.SHAPES)
def test_filter_and_oscillator_vs_model(gpu, L, M, n_taps):
    RC.check_filter_vs_model(factory, L, M, n_taps, "u8")


@pytest.mark.parametrize("fmt", [f for f in RC.FORMATS if f != "u8"])
def test_sample_formats_vs_model(gpu, fmt):
    RC.check_filter_vs_model(factory, 32, 125, 500, fmt)


def test_chunking_is_bit_identical(gpu):
    RC.check_chunking(factory)


def test_phase_over_a_long_run(gpu):
    RC.check_phase_long_run(factory)


def test_ring_wrap(gpu):
    RC.check_ring_wrap(factory)


def test_reset_keeps_the_configuration_and_clears_the_carry(gpu):
    RC.check_reset(factory)


def test_limits_and_state_errors(gpu):
    RC.check_errors(factory)


def test_end_to_end_vs_oracle_on_the_direct_streams(gpu):
    RC.check_end_to_end(factory, L=32, Mx=125, n_taps=2000, offsets=(-107, 0, 107))


def test_end_to_end_at_10_ms_per_s(gpu):
    RC.check_end_to_end(factory, L=128, Mx=625, n_taps=10000, offsets=(-107, 0, 107))
