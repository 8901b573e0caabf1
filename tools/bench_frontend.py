"""The wideband front end alone (dabphy_time_wideband: the launches of one write -- k_wideband or k_resample, then k_capture_carry) on a
capture that is already staged on the device, in two tables:
  integer rates   u8 captures of one frame (96 ms of signal) at D = 4 with 3 ensembles, D = 16 with 16 and D = 32 with 32, 16 taps
                  per branch;
  rational rates  at 8 MS/s (2.048 x 125/32) with 3 ensembles, 10 MS/s (625/128) with 5, 20 MS/s (625/64) with 11 and 56 MS/s (875/32)
                  with 32, prototypes of 16 output periods; and L = 1, M = 4 with 3 ensembles beside k_wideband at D = 4, the same filter.
Every filter is wideband.design_taps_rational(L, M) (L = 1: design_taps' filter).  Per shape: warm-up passes, then REPEATS passes timed
one by one with device events -> median, minimum and maximum; microseconds per 96 ms of signal, x real time, the bytes the launch has to
move (capture read once, every ensemble's ring samples written once) against the library's measured plain-copy rate (dabphy_time_copy),
the FMAs of the sums per second (k_wideband: 4 per tap, ensemble and output, padding ensembles not counted; k_resample: 2, taps per
phase as the kernel adds them) against the fp32 vector rate, and which of the two limits it sits nearer.  The captures are random bytes:
the kernels have no path that depends on the data, and a synthesised multi-block capture (wideband.synth_capture, what the tests decode)
would time the same.  Prints the two tables and one JSON line each.
Usage (GPU box): python tools/bench_frontend.py [repeats] [warmup]"""
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
# (name, integer kind, L, M, ensembles)
INTEGER_SHAPES = tuple(("D = %d" % D, True, 1, D, B) for D, B in ((4, 3), (16, 16), (32, 32)))
RATIONAL_SHAPES = (("8 MS/s", False, 32, 125, 3), ("10 MS/s", False, 128, 625, 5), ("20 MS/s", False, 64, 625, 11), ("56 MS/s", False, 32, 875, 32),
                   ("L = 1, M = 4", False, 1, 4, 3), ("k_wideband D = 4", True, 1, 4, 3))
# fp32 vector rate of the device: 256 compute units x 4 SIMDs x 32 FMAs per clock at 2.4 GHz = 78.6 T FMA/s (157.3 TFLOP/s, data sheet)
PEAK_FMA_PER_S = 256 * 4 * 32 * 2.4e9


def offsets_for(L, M, B):
    """B block centres 1.712 MHz = 107 x 16 kHz apart around the capture's centre (closer where they would not fit |offset| L <= 64 M)"""
    step = min(107, (128 * M // L) // max(B, 1))
    return [int(round((e - (B - 1) / 2.0) * step)) for e in range(B)]


def measure(table, shapes, copy_gbps):
    out = dict(tool="bench_frontend", table=table, repeats=REPEATS, warmup=WARMUP, signal_ms=96.0, shapes=[])
    rng = np.random.RandomState(3)
    for name, integer, L, M, B in shapes:
        d = capi.DabPhy(n_ensembles=B, max_frames=1, lib_path=GPU_LIB, want_constellation=False, want_impulse_response=False)
        try:
            out["device"] = d.device_name
            if not copy_gbps:
                copy_gbps.extend(d.time_copy(1 << 30, 0, 5) for _ in range(3))
            taps = wideband.design_taps_rational(L, M)
            offs = offsets_for(L, M, B)
            n = T_F * M // L                                        # one frame of signal
            raw = rng.randint(0, 256, (n, 2)).astype(np.uint8)
            if integer:
                d.stream_open_wideband(4 * T_F, M, taps, offs, "u8")
                per_output, fma_per_tap = len(taps), 4.0
            else:
                d.stream_open_resampled(4 * T_F, L, M, taps, offs, "u8")
                per_output, fma_per_tap = -(-(-(-len(taps) // L)) // 4) * 4, 2.0      # per phase, as the kernel adds them: whole fetch steps
            d.stream_write_wideband(raw)
            ms = np.sort(d.time_wideband(WARMUP, REPEATS).astype(np.float64))
            med = float(np.median(ms))
            n_out = n * L // M
            bytes_moved = n * 2 + B * n_out * 8
            fmas = fma_per_tap * per_output * B * n_out
            t_copy = bytes_moved / (float(np.median(copy_gbps)) * 1e9) * 1e3
            t_fma = fmas / PEAK_FMA_PER_S * 1e3
            out["shapes"].append(dict(name=name, kind="integer" if integer else "rational", L=L, M=M, ensembles=B, n_taps=len(taps), taps_per_output=per_output,
                                      offsets_first_last=[offs[0], offs[-1]], capture_samples=n, outputs=n_out, us_median=med * 1e3, us_min=float(ms[0]) * 1e3,
                                      us_max=float(ms[-1]) * 1e3, us_p10=float(ms[len(ms) // 10]) * 1e3, us_p90=float(ms[(9 * len(ms)) // 10]) * 1e3,
                                      x_real_time=96.0 / med, bytes_moved=bytes_moved, GBps=bytes_moved / (med * 1e-3) / 1e9, share_of_copy_rate=t_copy / med,
                                      fma_per_s=fmas / (med * 1e-3), share_of_fp32_vector_peak=t_fma / med,
                                      nearer_limit="fp32 vector rate" if t_fma > t_copy else "copy rate"))
        finally:
            d.close()
    out["copy_GBps_runs"] = [float(c) for c in copy_gbps]; out["copy_GBps_median"] = float(np.median(copy_gbps))
    return out


def main():
    import torch
    assert torch.cuda.is_available(), "bench_frontend needs the device"
    torch.cuda.init()
    copy_gbps = []                                                  # measured once, with the first handle
    tables = [measure("integer", INTEGER_SHAPES, copy_gbps), measure("rational", RATIONAL_SHAPES, copy_gbps)]
    about = "u8 capture of one frame (96 ms of signal) staged on the device; %d repeats after %d warm-up passes" % (REPEATS, WARMUP)
    copy = "plain copy (dabphy_time_copy, 1 GiB): %s GB/s read + write; fp32 vector peak taken as %.1f T FMA/s" % (", ".join("%.0f" % c for c in copy_gbps), PEAK_FMA_PER_S / 1e12)
    print("wideband channeliser alone, " + about)
    print(copy)
    print("%3s %4s %5s | %9s %9s %9s | %9s | %8s %7s | %9s %7s | %s" % ("D", "ens", "taps", "us median", "us min", "us max", "x real t.", "GB/s", "of copy", "T FMA/s", "of peak", "nearer limit"))
    for s in tables[0]["shapes"]:
        print("%3d %4d %5d | %9.1f %9.1f %9.1f | %9.0f | %8.1f %7.3f | %9.2f %7.3f | %s" % (s["M"], s["ensembles"], s["n_taps"], s["us_median"], s["us_min"], s["us_max"], s["x_real_time"],
                                                                                   s["GBps"], s["share_of_copy_rate"], s["fma_per_s"] / 1e12, s["share_of_fp32_vector_peak"], s["nearer_limit"]))
    print(json.dumps(tables[0]))
    print("rational resampler alone, " + about)
    print(copy)
    print("%-17s %4s %6s %4s | %9s %9s %9s | %9s | %8s %7s | %9s %7s" % ("shape", "ens", "taps", "/out", "us median", "us min", "us max", "x real t.", "GB/s", "of copy", "T FMA/s", "of peak"))
    for s in tables[1]["shapes"]:
        print("%-17s %4d %6d %4d | %9.1f %9.1f %9.1f | %9.0f | %8.1f %7.3f | %9.2f %7.3f" % (s["name"], s["ensembles"], s["n_taps"], s["taps_per_output"], s["us_median"], s["us_min"], s["us_max"],
                                                                                    s["x_real_time"], s["GBps"], s["share_of_copy_rate"], s["fma_per_s"] / 1e12, s["share_of_fp32_vector_peak"]))
    print(json.dumps(tables[1]))


if __name__ == "__main__":
    main()
