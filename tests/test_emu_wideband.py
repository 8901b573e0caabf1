"""Execution-model suite: the wideband front end (one capture channelised into the batch's ensembles) against the float64 model of
tests/wideband_model.py and, end to end, against the oracle on each ensemble's direct stream.  Cases: tests/frontend_cases.py."""
import pytest

import frontend_cases as F
from conftest import EMU_LIB
from welle_io_amd import capi

K = F.INTEGER                           # the kind's default shapes


def factory(**kw):
    return capi.DabPhy(lib_path=EMU_LIB, **kw)


@pytest.mark.parametrize("D,n_taps", F.INTEGER_SHAPES)
def test_filter_and_oscillator_vs_model(emu, D, n_taps):
    F.check_filter_vs_model(factory, F.Integer(D), n_taps, "u8")


@pytest.mark.parametrize("fmt", [f for f in F.FORMATS if f != "u8"])
def test_sample_formats_vs_model(emu, fmt):
    F.check_filter_vs_model(factory, K["rate"], K["n_taps"], fmt)


def test_chunking_is_bit_identical(emu):
    F.check_chunking(factory, K["rate"], K["n_taps"])


def test_phase_over_a_long_run(emu):
    F.check_phase_long_run(factory, **K["long_run"])


def test_ring_wrap(emu):
    F.check_ring_wrap(factory, **K["wrap"])


def test_reset_keeps_the_configuration_and_clears_the_carry(emu):
    F.check_reset(factory, K["rate"], K["n_taps"], K["reset_n1"])


def test_nothing_left_behind(emu):
    """every buffer the front end creates goes with the handle (the execution model counts what is alive)"""
    import ctypes as C
    import numpy as np

    def live():
        out = (C.c_int64 * 4)(); C.CDLL(EMU_LIB).hipemu_live_counts(out); return tuple(out)
    before = live()
    raw, taps, offsets = F.filter_case(K["rate"], K["n_taps"], "u8")
    d = factory(n_ensembles=3, max_frames=1, want_constellation=False)
    d.stream_open_wideband(F.RING_MIN, 4, taps, offsets, "u8")
    d.stream_write_wideband(raw)
    d.stream_write_wideband_async(np.ascontiguousarray(raw[:64])); d.stream_commit()
    d.stream_open_wideband(F.RING_MIN, 2, taps, F.Integer(2).filter_offsets(), "s16le")          # a second open reuses or replaces, never leaks
    d.close()
    assert live() == before


def test_limits_and_state_errors(emu):
    F.check_errors(factory, K["rate"], K["n_taps"])


def test_end_to_end_vs_oracle_on_the_direct_streams(emu):
    F.check_end_to_end(factory, F.Integer(4), offsets=(-107, 0, 107))
