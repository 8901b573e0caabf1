"""Execution-model suite: the wideband front end (one capture channelised into the batch's ensembles) against the float64 model of
tests/wideband_model.py and, end to end, against the oracle on each ensemble's direct stream.  Cases: tests/wideband_cases.py."""
import pytest

import wideband_cases as W
from conftest import EMU_LIB
from welle_io_amd import capi


def factory(**kw):
    return capi.DabPhy(lib_path=EMU_LIB, **kw)


@pytest.mark.parametrize("D,n_taps", W.SHAPES)
def test_filter_and_oscillator_vs_model(emu, D, n_taps):
    W.check_filter_vs_model(factory, D, n_taps, "u8")


@pytest.mark.parametrize("fmt", [f for f in W.FORMATS if f != "u8"])
def test_sample_formats_vs_model(emu, fmt):
    W.check_filter_vs_model(factory, 4, 64, fmt)


def test_chunking_is_bit_identical(emu):
    W.check_chunking(factory)


def test_phase_over_a_long_run(emu):
    W.check_phase_long_run(factory)


def test_ring_wrap(emu):
    W.check_ring_wrap(factory)


def test_reset_keeps_the_configuration_and_clears_the_carry(emu):
    W.check_reset(factory)


def test_nothing_left_behind(emu):
    """every buffer the front end creates goes with the handle (the execution model counts what is alive)"""
    import ctypes as C
    import numpy as np

    def live():
        out = (C.c_int64 * 4)(); C.CDLL(EMU_LIB).hipemu_live_counts(out); return tuple(out)
    before = live()
    raw, taps, offsets = W.filter_case(4, 64, "u8")
    d = factory(n_ensembles=3, max_frames=1, want_constellation=False)
    d.stream_open_wideband(W.RING_MIN, 4, taps, offsets, "u8")
    d.stream_write_wideband(raw)
    d.stream_write_wideband_async(np.ascontiguousarray(raw[:64])); d.stream_commit()
    d.stream_open_wideband(W.RING_MIN, 2, taps, W.filter_offsets(2), "s16le")          # a second open reuses or replaces, never leaks
    d.close()
    assert live() == before


def test_limits_and_state_errors(emu):
    W.check_errors(factory)


def test_end_to_end_vs_oracle_on_the_direct_streams(emu):
    W.check_end_to_end(factory, D=4, offsets=(-107, 0, 107))
