"""Cost of the channel BER pass (dabphy_set_channel_ber; k_chanber.hip) on the headline geometry: bench.py's handle (HBM-resident
looping IQ, the canonical multiplex, superframe filter inside dabphy_process) timed with the pass off and with it on in ONE device
session, the pass's own device time (profiling events around its two launches) and its algorithmic bytes against the 8 TB/s roofline.
Every leg: warm-up steps, then `steps` timed steps one by one; the spread (min / median / max) is reported, not only a mean.
Prints one JSON line.
Usage (GPU box): python tools/bench_chanber.py [B] [F] [steps] [--lib PATH] [--off-only]
  --lib PATH   another build of the library (a build of the parent commit, for the "off costs nothing" comparison in the same session)
  --off-only   only the leg with the pass off (the one a library without the feature can run)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: F401,E402
from conftest import GPU_LIB  # noqa: E402
from welle_io_amd import capi, workload  # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
LIB = GPU_LIB
if "--lib" in sys.argv:
    LIB = sys.argv[sys.argv.index("--lib") + 1]
    ARGS.remove(LIB)
OFF_ONLY = "--off-only" in sys.argv
B = int(ARGS[0]) if len(ARGS) > 0 else 256
F = int(ARGS[1]) if len(ARGS) > 1 else 32
STEPS = int(ARGS[2]) if len(ARGS) > 2 else 10
WARMUP = 3
HBM_BYTES_PER_S = 8e12


def spread(ms):
    ms = np.asarray(ms, np.float64)
    return dict(min=float(ms.min()), median=float(np.median(ms)), max=float(ms.max()), mean=float(ms.mean()), n=len(ms))


def algorithmic_bytes(subchs):
    """what the pass must move at least: the soft-bit ring once, the decoded bytes, every class's map once, the counters"""
    classes = {(s.bitrate, s.profile_b, s.level, s.uep is not None) for s in subchs}
    ring = B * F * 230400
    decoded = B * F * 384 + sum(B * 4 * F * 3 * s.bitrate for s in subchs)
    maps = 2 * 4 * 774 + sum(2 * 4 * (24 * br + 6) for br, _, _, _ in classes)
    n_cw = B * F * 4 + B * 4 * F * len(subchs)
    counters = 8 * n_cw + 8 * n_cw + 16 * B * (1 + len(subchs))       # records written, read again by the totals, the totals
    return dict(ring=ring, decoded=decoded, maps=maps, counters=counters, total=ring + decoded + maps + counters, code_words=n_cw)


def main():
    import torch
    rec = workload.rec_frames_for(F)
    iq, _, _, txs = workload.make_batch(B, device="cuda", rec_frames=rec, n_distinct=min(4, B))
    subchs = txs[0].subchs
    torch.cuda.synchronize()
    dev = workload.open_receiver(capi, LIB, iq, F, subchs)          # (profiling on: the stage times and the pass's events)
    out = dict(tool="bench_chanber", lib=os.path.relpath(LIB, ROOT), B=B, F=F, steps=STEPS, warmup=WARMUP, services=len(subchs), device=dev.device_name)

    def leg(name, on):
        if on is not None:
            dev.set_channel_ber(on)
        for _ in range(WARMUP):
            dev.process(F); dev.superframes_stats()
        torch.cuda.synchronize()
        step_ms, pass_ms, stages = [], [], []
        tot = np.zeros(2, np.float64)
        for _ in range(STEPS):
            t0 = time.perf_counter()
            dev.process(F)
            dev.superframes_stats()
            if on:
                e, c = dev.channel_ber_totals()                    # (the one small array a monitor reads per step)
            step_ms.append((time.perf_counter() - t0) * 1e3)
            stages.append(dev.stage_times())
            if on:
                pass_ms.append(dev.chanber_ms()); tot += (float(e.sum()), float(c.sum()))
        out[name] = dict(step_ms=spread(step_ms), x_real_time=B * F * 96.0 / float(np.median(step_ms)),
                         demod_ms=float(np.median([s["demod"] for s in stages])), msc_viterbi_ms=float(np.median([s["msc_viterbi"] for s in stages])))
        if on:
            ab = algorithmic_bytes(subchs)
            p = spread(pass_ms)
            out[name].update(pass_ms=p, algorithmic_bytes=ab, roofline_ms=ab["total"] / HBM_BYTES_PER_S * 1e3,
                             fraction_of_roofline=ab["total"] / HBM_BYTES_PER_S * 1e3 / p["median"] if p["median"] > 0 else None,
                             errors=tot[0], compared=tot[1], channel_ber=tot[0] / tot[1] if tot[1] else None)

    if OFF_ONLY:
        leg("off", None)
    else:
        leg("off", False)
        leg("on", True)
        leg("off_again", False)
    dev.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
