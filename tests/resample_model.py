"""Float64 model of the rational resampler (include/dabphy.h, dabphy_stream_open_resampled), vectorised over the outputs m:

    y_e[m] = sum_{j < J} h[r_m + j L] * c(x[a_m - j]) * w_e[a_m - j],   a_m = (m M + M - 1) div L,  r_m = (m M + M - 1) mod L,
    J = ceil(n_taps / L),  h[k >= n_taps] = 0,  x[i < 0] = 0,  w_e[i] = exp(-2 pi j ((offset_e L i) mod P) / P),  P = 128 M

and the accuracy condition the library's fp32 sums are held to, for every output -- the integer model's (tests/wideband_model.py) with J,
the taps one output adds, in place of n_taps:

    |y - y_model| <= (J + 16) * 2^-23 * sum_j |h[r_m + j L]| * |c(x[a_m - j])|

(J u with u = 2^-24 bounds the fp32 accumulation; a handful of roundings per term for the table entry, the mixing product and the tap; a
factor 2.  A mistake in an index, a phase or the carry is wrong by the size of the signal.)"""
import numpy as np


def n_outputs(n, L, M):
    """samples the stream holds after n capture samples"""
    return n * int(L) // int(M)


def resample(x, taps, offset, L, M):
    """x: the whole converted capture since the open call (complex128) -> (y [n L // M] complex128, bound of the accuracy condition)"""
    L, M = int(L), int(M); P = 128 * M
    taps = np.asarray(taps, np.float32).astype(np.float64)
    J = -(-len(taps) // L)
    H = np.zeros(J * L, np.float64); H[:len(taps)] = taps
    H = H.reshape(J, L)                                              # H[j][r] = h[r + j L]
    x = np.asarray(x, np.complex128); n = len(x)
    i = np.arange(n, dtype=np.int64)
    w = np.exp(-2j * np.pi * ((int(offset) * L * i) % P) / P)
    xw = np.concatenate([np.zeros(J, np.complex128), x * w])         # entry J + i is sample i: zeros in front of the stream
    xa = np.abs(np.concatenate([np.zeros(J, np.float64), np.abs(x)]))
    q = np.arange(n_outputs(n, L, M), dtype=np.int64) * M + (M - 1)
    a, r = q // L + J, q % L
    y = np.zeros(len(q), np.complex128); s = np.zeros(len(q), np.float64)
    for j in range(J):
        hj = H[j][r]
        y += hj * xw[a - j]; s += np.abs(hj) * xa[a - j]
    return y, (J + 16) * 2.0 ** -23 * s


def by_definition(x, taps, L, M):
    """the unmixed sum as the textbook states it: L - 1 zeros behind every sample, the prototype, every M-th sample from M - 1"""
    up = np.zeros(len(x) * int(L), np.complex128); up[::int(L)] = x
    return np.convolve(up, np.asarray(taps, np.float64))[int(M) - 1:len(up):int(M)]
