"""The rational resampler alone (k_resample + k_resample_carry, dabphy_time_wideband) on a capture that is already staged on the device:
u8 captures of one frame (96 ms of signal) at 8 MS/s (2.048 x 125/32) with 3 ensembles, 10 MS/s (625/128) with 5, 20 MS/s (625/64) with
11 and 56 MS/s (875/32) with 32, prototypes from wideband.design_taps_rational (16 output periods); and L = 1, M = 4 with 3 ensembles
beside k_wideband at D = 4 with the same taps.  Per shape: warm-up passes, then REPEATS passes timed one by one with device events ->
median, minimum and maximum; microseconds per 96 ms of signal, x real time, the bytes the launch has to move (capture read once, every
ensemble's ring samples written once) against the library's measured plain-copy rate (dabphy_time_copy), and the FMAs of the sums
(2 per tap, ensemble and output, taps per phase as the kernel adds them) against the fp32 vector rate.  The captures are random bytes:
the kernel has no path that depends on the data.  Prints a table and one JSON line.
Usage (GPU box): python tools/bench_resample.py [repeats] [warmup]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: F401,E402
from conftest import GPU_LIB  # noqa: E402
from welle_io_amd import capi, wideband  # noqa: E402

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 5
T_F = 196608
# (name, L, M, ensembles); L = 0: k_wideband at D = M, for the row beside it
SHAPES = (("8 MS/s", 32, 125, 3), ("10 MS/s", 128, 625, 5), ("20 MS/s", 64, 625, 11), ("56 MS/s", 32, 875, 32), ("L = 1, M = 4", 1, 4, 3), ("k_wideband D = 4", 0, 4, 3))
# fp32 vector rate of the device: 256 compute units x 4 SIMDs x 32 FMAs per clock at 2.4 GHz = 78.6 T FMA/s (157.3 TFLOP/s, data sheet)
PEAK_FMA_PER_S = 256 * 4 * 32 * 2.4e9


def offsets_for(L, M, B):
    """B block centres 1.712 MHz = 107 x 16 kHz apart around the capture's centre (closer where they would not fit |offset| L <= 64 M)"""
    step = min(107, (128 * M // L) // max(B, 1))
    return [int(round((e - (B - 1) / 2.0) * step)) for e in range(B)]


def main():
    import torch
    assert torch.cuda.is_available(), "bench_resample needs the device"
    torch.cuda.init()
    out = dict(tool="bench_resample", repeats=REPEATS, warmup=WARMUP, signal_ms=96.0, shapes=[])
    rng = np.random.RandomState(3)
    copy_gbps = None
    for name, L, M, B in SHAPES:
        d = capi.DabPhy(n_ensembles=B, max_frames=1, lib_path=GPU_LIB, want_constellation=False, want_impulse_response=False)
        try:
            out["device"] = d.device_name
            if copy_gbps is None:
                copy_gbps = [d.time_copy(1 << 30, 0, 5) for _ in range(3)]
            Lx = max(L, 1)
            taps = wideband.design_taps_rational(Lx, M)
            offs = offsets_for(Lx, M, B)
            n = T_F * M // Lx                                       # one frame of signal
            raw = rng.randint(0, 256, (n, 2)).astype(np.uint8)
            if L:
                d.stream_open_resampled(4 * T_F, L, M, taps, offs, "u8")
                per_phase = -(-(-(-len(taps) // L)) // 4) * 4          # as the kernel adds them: whole fetch steps
                fma_per_tap = 2.0
            else:
                d.stream_open_wideband(4 * T_F, M, taps, offs, "u8")
                per_phase, fma_per_tap = len(taps), 4.0
            d.stream_write_wideband(raw)
            ms = np.sort(d.time_wideband(WARMUP, REPEATS).astype(np.float64))
            med = float(np.median(ms))
            n_out = n * Lx // M
            bytes_moved = n * 2 + B * n_out * 8
            fmas = fma_per_tap * per_phase * B * n_out
            t_copy = bytes_moved / (float(np.median(copy_gbps)) * 1e9) * 1e3
            t_fma = fmas / PEAK_FMA_PER_S * 1e3
            out["shapes"].append(dict(name=name, L=L, M=M, ensembles=B, n_taps=len(taps), taps_per_output=per_phase, offsets_first_last=[offs[0], offs[-1]],
                                      capture_samples=n, outputs=n_out, us_median=med * 1e3, us_min=float(ms[0]) * 1e3, us_max=float(ms[-1]) * 1e3,
                                      us_p10=float(ms[len(ms) // 10]) * 1e3, us_p90=float(ms[(9 * len(ms)) // 10]) * 1e3, x_real_time=96.0 / med,
                                      bytes_moved=bytes_moved, GBps=bytes_moved / (med * 1e-3) / 1e9, share_of_copy_rate=t_copy / med,
                                      fma_per_s=fmas / (med * 1e-3), share_of_fp32_vector_peak=t_fma / med))
        finally:
            d.close()
    out["copy_GBps_runs"] = [float(c) for c in copy_gbps]; out["copy_GBps_median"] = float(np.median(copy_gbps))
    print("rational resampler alone, u8 capture of one frame (96 ms of signal) staged on the device; %d repeats after %d warm-up passes" % (REPEATS, WARMUP))
    print("plain copy (dabphy_time_copy, 1 GiB): %s GB/s read + write; fp32 vector peak taken as %.1f T FMA/s" % (", ".join("%.0f" % c for c in copy_gbps), PEAK_FMA_PER_S / 1e12))
    print("%-17s %4s %6s %4s | %9s %9s %9s | %9s | %8s %7s | %9s %7s" % ("shape", "ens", "taps", "/out", "us median", "us min", "us max", "x real t.", "GB/s", "of copy", "T FMA/s", "of peak"))
    for s in out["shapes"]:
        print("%-17s %4d %6d %4d | %9.1f %9.1f %9.1f | %9.0f | %8.1f %7.3f | %9.2f %7.3f" % (s["name"], s["ensembles"], s["n_taps"], s["taps_per_output"], s["us_median"], s["us_min"], s["us_max"],
                                                                                    s["x_real_time"], s["GBps"], s["share_of_copy_rate"], s["fma_per_s"] / 1e12, s["share_of_fp32_vector_peak"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
