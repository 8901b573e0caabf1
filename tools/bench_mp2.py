"""Cost of the MP2 frame check on the headline geometry: bench.py's handle (HBM-resident looping IQ, superframe filter inside
dabphy_process) on the canonical multiplex with every 4th of its 18 services carrying Layer II frames (workload.make_mp2_base_streams),
timed three ways -- no kinds set (every service through the DAB+ filter, as bench.py runs), kinds set without the MP2 pass, kinds set with
dabphy_set_auto_mp2 -- plus the MP2 pass' own device time (profiling events around its launches).  Prints one JSON line.
Usage (GPU box): python tools/bench_mp2.py [B] [F] [steps]"""
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

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
F = int(sys.argv[2]) if len(sys.argv) > 2 else 32
STEPS = int(sys.argv[3]) if len(sys.argv) > 3 else 10


def main():
    import torch
    rec = workload.rec_frames_for(F)
    base, subchs, mp2_pos = workload.make_mp2_base_streams(min(4, B), rec)
    iq, _, _, _ = workload.make_batch(B, device="cuda", base=(base, None), rec_frames=rec, n_distinct=min(4, B))
    torch.cuda.synchronize()
    dev = workload.open_receiver(capi, GPU_LIB, iq, F, subchs)          # (profiling on: the stage times and the MP2 pass' events)
    kinds = [capi.AUDIO_MP2 if i in mp2_pos else capi.AUDIO_DABPLUS for i in range(len(subchs))]
    out = dict(tool="bench_mp2", B=B, F=F, steps=STEPS, services=len(subchs), mp2_services=len(mp2_pos), device=dev.device_name)
    tot = np.zeros(4, np.int64)

    def leg(name, auto):
        nonlocal tot
        dev.set_auto_mp2(auto)
        for _ in range(3):                                   # warm-up (and the first batch after a change of kinds)
            dev.process(F); dev.superframes_stats()
            if auto:
                dev.mp2_stats()
        torch.cuda.synchronize()
        ms_pass = []
        t0 = time.perf_counter()
        for _ in range(STEPS):
            dev.process(F)
            dev.superframes_stats()
            if auto:
                st = dev.mp2_stats()                         # (the pass rode in dabphy_process: this fetches its totals)
                tot += st.sum(axis=0)
                ms_pass.append(dev.mp2_ms())
        dt = (time.perf_counter() - t0) / STEPS
        out[name] = dict(ms_per_step=dt * 1e3, x_real_time=B * F * 0.096 / dt)
        if ms_pass:
            out[name]["mp2_pass_ms"] = float(np.mean(ms_pass))
            out[name]["mp2_pass_ms_min"] = float(np.min(ms_pass))

    leg("no_kinds", False)
    for b in range(B):
        dev.set_audio_kinds_ensemble(b, kinds)
    leg("kinds_no_mp2_pass", False)
    leg("kinds_auto_mp2", True)
    out["mp2_totals"] = dict(frames=int(tot[0]), crc_failures=int(tot[1]), bytes_skipped=int(tot[2]), unverified_frames=int(tot[3]))
    dev.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
