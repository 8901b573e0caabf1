"""The float64 model of the rational resampler (tests/resample_model.py) against the definition it restates, and against the integer
model where the two coincide; the host-side helpers of welle_io_amd.wideband.  No library needed."""
import numpy as np
import pytest

import resample_model as RM
import wideband_model as WM
from frontend_cases import random_taps
from welle_io_amd import wideband


@pytest.mark.parametrize("L,M,n_taps", [(2, 3, 7), (3, 4, 37), (32, 125, 500)])
def test_model_is_the_definition(L, M, n_taps):
    """zero-stuff by L, np.convolve, every M-th sample from M - 1 (offset 0: the definition has no oscillator)"""
    rng = np.random.RandomState(L + M)
    x = rng.standard_normal(2000) + 1j * rng.standard_normal(2000)
    taps = random_taps(n_taps, rng)
    y, bound = RM.resample(x, taps, 0, L, M)
    want = RM.by_definition(x, taps.astype(np.float64), L, M)
    assert len(y) == len(want) == 2000 * L // M
    assert np.abs(y - want).max() < 1e-13 * np.abs(want).max()
    assert bound.min() > 0


@pytest.mark.parametrize("L,M,n_taps,offset", [(2, 3, 7, 5), (32, 125, 500, -107)])
def test_model_mixes_before_it_filters(L, M, n_taps, offset):
    """the oscillator: the definition applied to the capture turned by exp(-2 pi j offset L i / P)"""
    rng = np.random.RandomState(3)
    x = rng.standard_normal(2000) + 1j * rng.standard_normal(2000)
    taps = random_taps(n_taps, rng)
    w = np.exp(-2j * np.pi * offset * L * np.arange(2000) / (128.0 * M))
    y, _ = RM.resample(x, taps, offset, L, M)
    want = RM.by_definition(x * w, taps.astype(np.float64), L, M)
    assert np.abs(y - want).max() < 1e-11 * np.abs(want).max()


def test_model_with_L_1_is_the_integer_model():
    rng = np.random.RandomState(4)
    raw = WM.random_capture(4 * 1000 + 3, "u8", rng); x = WM.convert(raw, "u8"); taps = random_taps(64, rng)
    for offset in (0, 256, -255):
        y, bound = RM.resample(x, taps, offset, 1, 4)
        y4, bound4 = WM.channelise(x, taps, offset, 4)
        assert len(y) == len(y4) == 1000
        assert np.abs(y - y4).max() < 1e-13 * np.abs(y4).max()
        assert np.allclose(bound, bound4, rtol=1e-12)               # J = n_taps


def test_output_count():
    for L, M in ((32, 125), (1, 4), (512, 4095)):
        for n in (0, 1, 3, 4, 125, 126, 4001):
            q = np.arange(n * L // M + 2, dtype=np.int64) * M + M - 1
            assert RM.n_outputs(n, L, M) == int(np.sum(q // L < n))  # outputs whose newest sample a_m has been written


def test_design_taps_rational():
    h = wideband.design_taps_rational(32, 125)
    assert h.dtype == np.float32 and len(h) == 2000 and -(-len(h) // 32) == 63
    assert abs(float(h.astype(np.float64).sum()) - 32.0) < 1e-4
    assert np.allclose(h, h[::-1], atol=1e-6)
    assert len(wideband.design_taps_rational(128, 625)) == 10000
    # with L = 1 the prototype is design_taps' filter
    assert np.allclose(wideband.design_taps_rational(1, 4), wideband.design_taps(4), atol=1e-7)
    # a Kaiser window with beta = 8 (about 80 dB) over 16 output periods has a transition about 0.65 MHz wide around the 1.024 MHz cutoff
    H = np.abs(np.fft.fft(h.astype(np.float64), 1 << 18)) / 32.0
    f = np.fft.fftfreq(1 << 18, 1.0 / (125 * 2.048e6))
    assert H[np.abs(f) >= 1.4e6].max() < 10 ** (-60 / 20.0) and abs(H[np.abs(f) <= 0.65e6] - 1.0).max() < 0.01


def test_synth_capture_rational_holds_each_stream_at_its_offset():
    """a tone at +100 kHz in a stream, placed at offset 107 in an 8 MS/s capture, stands at 107 x 16 kHz + 100 kHz; L = 1 is synth_capture"""
    n = 8192
    tone = 0.25 * np.exp(2j * np.pi * 100e3 / 2.048e6 * np.arange(n))
    tone = tone * np.hanning(n)                                     # (band-limited, periodic in the padded length)
    cap = wideband.synth_capture_rational([tone], [107], 32, 125)
    assert len(cap) == n * 125 // 32
    S = np.abs(np.fft.fft(cap)); f = np.fft.fftfreq(len(cap), 1.0 / 8e6)
    assert abs(f[int(np.argmax(S))] - (107 * 16e3 + 100e3)) < 2 * 8e6 / len(cap)
    assert np.allclose(wideband.synth_capture_rational([tone], [107], 1, 4), wideband.synth_capture([tone], [107], 4), atol=1e-12)
    noisy = wideband.synth_capture_rational([np.zeros(n)], [0], 32, 125, snr_db=20, seed=1)
    assert abs(np.mean(np.abs(noisy) ** 2) / (125 / 32 * 0.25 ** 2 / 100) - 1) < 0.05
