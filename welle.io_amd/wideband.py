"""Wideband front end, host side: the low-pass design for dabphy_stream_open_wideband and a synthetic multi-block capture.

A capture at decimation x 2.048 MS/s holds several DAB blocks side by side; the library mixes each one down by its offset (in units of
16 kHz = 2 048 000 / 128), filters with the real taps given here and keeps every decimation-th sample (include/dabphy.h).  The
*_rational functions are the same for a capture at 2.048 MS/s x decimation / interpolation (dabphy_stream_open_resampled)."""
import numpy as np

RATE = 2048000
OFFSET_UNIT_HZ = RATE // 128            # 16 kHz: every DAB block centre is a multiple of it


def _kaiser_lowpass(n, rate_multiple, beta):
    """n float64 taps of a windowed-sinc Kaiser low-pass with its cutoff at 1.024 MHz, at rate_multiple x 2.048 MS/s; not normalised"""
    fc = 1024000.0 / (rate_multiple * float(RATE))           # cycles per sample
    k = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    return 2.0 * fc * np.sinc(2.0 * fc * k) * np.kaiser(n, float(beta))


def design_taps(decimation, taps_per_branch=16, beta=8.0):
    """Windowed-sinc Kaiser low-pass for a capture at decimation x 2.048 MS/s: taps_per_branch * decimation real taps (float32), unit DC
    gain, computed in float64.  Cutoff 1.024 MHz: the transition may run from 768 kHz, the edge of the DAB signal, to 1 280 kHz, the
    lowest frequency that decimation folds onto that edge (1 280 - 2 048 = -768 kHz) -- a neighbour 1.712 MHz away reaches from 944 kHz
    upwards, and what it has below 1 280 kHz lands outside the carriers.  The cutoff sits in the middle of that band."""
    decimation = int(decimation); n = int(taps_per_branch) * decimation
    if decimation < 1 or n < 1:
        raise ValueError("design_taps: decimation and taps_per_branch must be positive")
    h = _kaiser_lowpass(n, decimation, beta)
    return (h / h.sum()).astype(np.float32)


def synth_capture(streams, offsets, decimation, snr_db=None, seed=0, amplitude=0.25):
    """One capture (complex128, at decimation x 2.048 MS/s) out of noise-free 2.048 MS/s streams (synth.make_stream without snr_db): each
    is upsampled by zero-padding its spectrum (exact for these band-limited streams), shifted up by its offset x 16 kHz, and all are
    summed; white noise is added so that every channel sees snr_db in ITS 2.048 MHz (a signal of power amplitude ** 2: the noise power
    of the capture is decimation times the channel's).  The length is that of the longest stream, rounded up to a multiple of 4 096,
    times the decimation.  (synth_capture_rational with interpolation 1: the same samples, bit for bit.)"""
    return synth_capture_rational(streams, offsets, 1, decimation, snr_db=snr_db, seed=seed, amplitude=amplitude)


def design_taps_rational(interpolation, decimation, periods=16, beta=8.0):
    """The prototype for dabphy_stream_open_resampled, a capture at 2.048 MS/s x decimation / interpolation: a windowed-sinc Kaiser
    low-pass at interpolation x the capture's rate = decimation x 2.048 MS/s, round(periods * decimation) real taps (float32) -- `periods`
    output samples long, about periods * decimation / interpolation taps per phase.  Cutoff 1.024 MHz as design_taps, DC gain
    `interpolation` (every phase then has gain about 1), computed in float64."""
    L, M = int(interpolation), int(decimation); n = int(round(periods * M))
    if L < 1 or M < L or n < 1:
        raise ValueError("design_taps_rational: needs 1 <= interpolation <= decimation and a positive length")
    h = _kaiser_lowpass(n, M, beta)                           # (at the prototype's rate)
    return (h * (L / h.sum())).astype(np.float32)


def synth_capture_rational(streams, offsets, interpolation, decimation, snr_db=None, seed=0, amplitude=0.25):
    """The same at 2.048 MS/s x decimation / interpolation: every stream's spectrum (padded to n points, a multiple of 4 096 and
    of the interpolation) is zero-padded to n * decimation / interpolation points, the stream shifted up by its offset x 16 kHz --
    (offset * interpolation * i) mod P of P = 128 * decimation cycles at capture sample i -- and white noise of decimation /
    interpolation times the channel's power added, so that every channel sees snr_db in ITS 2.048 MHz."""
    L, M = int(interpolation), int(decimation)
    if len(streams) != len(offsets):
        raise ValueError("synth_capture_rational: %d streams, %d offsets" % (len(streams), len(offsets)))
    unit = 4096 * L // np.gcd(4096, L)
    n = -(-max(len(s) for s in streams) // unit) * unit
    n2 = n // L * M; P = 128 * M
    cap = np.zeros(n2, np.complex128)
    i = np.arange(n2, dtype=np.int64)
    for s, off in zip(streams, offsets):
        X = np.fft.fft(np.concatenate([np.asarray(s, np.complex128), np.zeros(n - len(s), np.complex128)]))
        Y = np.zeros(n2, np.complex128)
        Y[:n // 2] = X[:n // 2]; Y[-(n // 2):] = X[n // 2:]
        cap += np.fft.ifft(Y) * (n2 / n) * np.exp(2j * np.pi * ((int(off) * L * i) % P) / P)
    if snr_db is not None:
        rng = np.random.RandomState(seed)
        sigma = np.sqrt(M / L * amplitude ** 2 / (10 ** (snr_db / 10.0)) / 2)
        cap = cap + sigma * (rng.randn(n2) + 1j * rng.randn(n2))
    return cap


def to_u8_capture(cap, headroom=0.99):
    """-> (u8 array [n][2], the scale applied): the capture scaled so that its largest component sits at `headroom` of full scale --
    nothing clips -- and quantised as the u8 front ends deliver it ((b - 128) / 128 on the way in)"""
    scale = headroom / max(np.abs(cap.real).max(), np.abs(cap.imag).max())
    iq = np.stack([cap.real, cap.imag], 1) * scale
    return np.clip(np.round(iq * 127.0) + 128, 0, 255).astype(np.uint8), scale
