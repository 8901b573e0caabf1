"""Float64 model of the wideband channeliser (include/dabphy.h, dabphy_stream_open_wideband): double-precision oscillator, np.convolve.

    y_e[m] = sum_k taps[k] * c(x[m D + D - 1 - k]) * exp(-2 pi j ((offset_e * (m D + D - 1 - k)) mod P) / P),   P = 128 D,  x[i < 0] = 0

and the accuracy condition the library's fp32 sums are held to, for every output:

    |y - y_model| <= (n_taps + 16) * 2^-23 * sum_k |taps[k]| * |c(x[.])|

(n u with u = 2^-24 bounds an fp32 inner product of n terms in any order; a handful of roundings per term for the table entry, the
complex product and the per-ensemble tap; a factor 2.  A mistake in an index, a phase or the carry is wrong by the size of the signal.)"""
import numpy as np


def random_capture(n, fmt, rng):
    """-> raw array as the format stores it: [n][2] integers (s16: in the reference's byte order for that name), or complex64"""
    if fmt == "cf32":
        return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    if fmt == "u8":
        return rng.randint(0, 256, (n, 2)).astype(np.uint8)
    if fmt == "s8":
        return rng.randint(-128, 128, (n, 2)).astype(np.int8)
    v = rng.randint(-32768, 32768, (n, 2)).astype(np.int16)
    return v.astype(">i2" if fmt == "s16le" else "<i2")            # "S16LE" reads (byte0 << 8) | byte1, "S16BE" (byte1 << 8) | byte0


def convert(raw, fmt):
    """c(): the capture as complex128, exactly what CRAWFile::convertSamples makes of it (every value is exact in float32)"""
    if fmt == "cf32":
        return np.asarray(raw, np.complex64).astype(np.complex128)
    v = np.asarray(raw).astype(np.float64)
    if fmt == "u8":
        v = (v - 128.0) / 128.0
    elif fmt == "s8":
        v = v / 128.0
    return v[:, 0] + 1j * v[:, 1]


def channelise(x, taps, offset, decimation):
    """x: the whole converted capture since the open call (complex128) -> (y [n // D] complex128, bound [n // D] of the accuracy condition)"""
    D = int(decimation); P = 128 * D
    taps = np.asarray(taps, np.float32).astype(np.float64)
    n = len(x) // D * D
    x = np.asarray(x, np.complex128)[:n]
    w = np.exp(-2j * np.pi * ((np.arange(n, dtype=np.int64) * int(offset)) % P) / P)
    pick = np.arange(n // D) * D + D - 1
    y = np.convolve(x * w, taps)[pick]
    bound = (len(taps) + 16) * 2.0 ** -23 * np.convolve(np.abs(x), np.abs(taps))[pick]
    return y, bound
