"""The wideband channeliser alone (k_wideband + k_wideband_carry, dabphy_time_wideband) on a capture that is already staged on the
device: u8 captures of one frame (96 ms of signal) at D = 4 with 3 ensembles, D = 16 with 16 and D = 32 with 32, taps from
wideband.design_taps (16 per branch).  Per shape: warm-up passes, then REPEATS passes timed one by one with device events -> median,
minimum and maximum; microseconds per 96 ms of signal, x real time, the bytes the launch has to move (capture read once, every
ensemble's ring samples written once) against the library's measured plain-copy rate (dabphy_time_copy), the FMAs it issues per second
(4 per tap, ensemble and output, padding ensembles not counted) and which of the two limits -- copy rate or the fp32 vector rate --
it sits nearer.  The captures are random bytes: the kernel has no path that depends on the data, and a synthesised multi-block
capture (wideband.synth_capture, what the tests decode) would time the same.  Prints a table and one JSON line.
Usage (GPU box): python tools/bench_wideband.py [repeats] [warmup]"""
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
SHAPES = ((4, 3), (16, 16), (32, 32))             # (D, ensembles)
# fp32 vector rate of the device: 256 compute units x 4 SIMDs x 32 FMAs per clock at 2.4 GHz = 78.6 T FMA/s (157.3 TFLOP/s, data sheet)
PEAK_FMA_PER_S = 256 * 4 * 32 * 2.4e9


def offsets_for(D, B):
    """B block centres spread over the capture, |offset| <= 64 D, 1.712 MHz = 107 x 16 kHz apart where they fit"""
    step = min(107, (128 * D) // max(B, 1))
    return [int(round((e - (B - 1) / 2.0) * step)) for e in range(B)]


def main():
    import torch
    assert torch.cuda.is_available(), "bench_wideband needs the device"
    torch.cuda.init()
    out = dict(tool="bench_wideband", repeats=REPEATS, warmup=WARMUP, signal_ms=96.0, shapes=[])
    rng = np.random.RandomState(3)
    copy_gbps = None
    for D, B in SHAPES:
        d = capi.DabPhy(n_ensembles=B, max_frames=1, lib_path=GPU_LIB, want_constellation=False, want_impulse_response=False)
        try:
            out["device"] = d.device_name
            if copy_gbps is None:
                copy_gbps = [d.time_copy(1 << 30, 0, 5) for _ in range(3)]
            taps = wideband.design_taps(D)
            offs = offsets_for(D, B)
            raw = rng.randint(0, 256, (T_F * D, 2)).astype(np.uint8)
            d.stream_open_wideband(4 * T_F, D, taps, offs, "u8")
            d.stream_write_wideband(raw)
            ms = np.sort(d.time_wideband(WARMUP, REPEATS).astype(np.float64))
            med = float(np.median(ms))
            bytes_moved = T_F * D * 2 + B * T_F * 8
            fmas = 4.0 * len(taps) * B * T_F
            t_copy = bytes_moved / (float(np.median(copy_gbps)) * 1e9) * 1e3
            t_fma = fmas / PEAK_FMA_PER_S * 1e3
            out["shapes"].append(dict(D=D, ensembles=B, n_taps=len(taps), offsets_first_last=[offs[0], offs[-1]], us_median=med * 1e3, us_min=float(ms[0]) * 1e3, us_max=float(ms[-1]) * 1e3,
                                      us_p10=float(ms[len(ms) // 10]) * 1e3, us_p90=float(ms[(9 * len(ms)) // 10]) * 1e3, x_real_time=96.0 / med,
                                      bytes_moved=bytes_moved, GBps=bytes_moved / (med * 1e-3) / 1e9, share_of_copy_rate=t_copy / med,
                                      fma_per_s=fmas / (med * 1e-3), share_of_fp32_vector_peak=t_fma / med,
                                      nearer_limit="fp32 vector rate" if t_fma > t_copy else "copy rate"))
        finally:
            d.close()
    out["copy_GBps_runs"] = [float(c) for c in copy_gbps]; out["copy_GBps_median"] = float(np.median(copy_gbps))
    print("wideband channeliser alone, u8 capture of one frame (96 ms of signal) staged on the device; %d repeats after %d warm-up passes" % (REPEATS, WARMUP))
    print("plain copy (dabphy_time_copy, 1 GiB): %s GB/s read + write; fp32 vector peak taken as %.1f T FMA/s" % (", ".join("%.0f" % c for c in copy_gbps), PEAK_FMA_PER_S / 1e12))
    print("%3s %4s %5s | %9s %9s %9s | %9s | %8s %7s | %9s %7s | %s" % ("D", "ens", "taps", "us median", "us min", "us max", "x real t.", "GB/s", "of copy", "T FMA/s", "of peak", "nearer limit"))
    for s in out["shapes"]:
        print("%3d %4d %5d | %9.1f %9.1f %9.1f | %9.0f | %8.1f %7.3f | %9.2f %7.3f | %s" % (s["D"], s["ensembles"], s["n_taps"], s["us_median"], s["us_min"], s["us_max"], s["x_real_time"],
                                                                                   s["GBps"], s["share_of_copy_rate"], s["fma_per_s"] / 1e12, s["share_of_fp32_vector_peak"], s["nearer_limit"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
