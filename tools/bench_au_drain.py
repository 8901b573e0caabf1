"""Cost of the bulk access-unit drain on the headline geometry: bench.py's handle (HBM-resident looping IQ, 18 DAB+ services per ensemble)
with the superframe filter DEFERRED (dabphy_set_auto_superframes 2), timed three ways -- drain off, DABPHY_AU_RAW and DABPHY_AU_LOAS with
every step doing  au_drain_begin -> the next process -> au_drain_wait  into page-locked memory (bench.py's msc_drain_leg is the model) --
plus the bytes that leave per step, the pack kernel's own device time (profiling events around its launches) and, for comparison, the
library's float4 device copy of the same number of bytes (dabphy_time_copy).  Prints one JSON line.
Usage (GPU box): python tools/bench_au_drain.py [B] [F] [steps] [--no-table]"""
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
B = int(ARGS[0]) if len(ARGS) > 0 else 256
F = int(ARGS[1]) if len(ARGS) > 1 else 32
STEPS = int(ARGS[2]) if len(ARGS) > 2 else 10
TABLE = "--no-table" not in sys.argv


def main():
    import torch
    rec = workload.rec_frames_for(F)
    iq, _, _, txs = workload.make_batch(B, device="cuda", rec_frames=rec, n_distinct=min(4, B))
    torch.cuda.synchronize()
    subchs = txs[0].subchs
    dev = workload.open_receiver(capi, GPU_LIB, iq, F, subchs, deferred_filter=True)      # (profiling on: the pack pass' events)
    out = dict(tool="bench_au_drain", B=B, F=F, steps=STEPS, services=B * len(subchs), device=dev.device_name, au_table=TABLE)

    def step():
        dev.process(F); sf = dev.superframes_stats(); dev.fibs_host()
        return sf

    def timed(body):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(STEPS):
            body()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / STEPS * 1e3

    for _ in range(4):                                                  # acquisition, de-interleaver fill, superframe synchronisation
        step()
    out["off_ms"] = [timed(step) for _ in range(2)]
    for name, fmt in (("raw", capi.AU_RAW), ("loas", capi.AU_LOAS)):
        dev.set_au_drain(fmt)
        step(); sf = step()                                             # the second one queues the first pack pass
        nb, ns, na = dev.au_batch_size()
        buf = dev.host_alloc((nb,), np.uint8); svc = np.zeros(ns, capi.AU_SERVICE_DTYPE)
        aus = dev.host_alloc((na,), capi.AU_DESC_DTYPE) if TABLE else None
        try:
            _, s, _ = dev.au_batch(buf, svc, aus if TABLE else False)
            alone = []
            for _ in range(3):                                          # the drain alone: the device otherwise idle
                step(); t0 = time.perf_counter(); dev.au_batch(buf, svc, aus if TABLE else False); alone.append(time.perf_counter() - t0)
            pack_ms = []
            state = {}

            def body():
                dev.au_drain_begin(buf, svc, aus if TABLE else False)   # batch k - 1 leaves ...
                state["sf"] = step()                                    # ... while batch k + 1 is decoded and batch k filtered and packed
                pack_ms.append(dev.au_ms())
                _, state["svc"], _ = dev.au_drain_wait()
            step()
            ms = timed(body)
            s = state["svc"]
            stored = int(s["bytes"].sum())
            assert int(s["n_superframes"].sum()) >= B * len(subchs) * (4 * F // 5) and int(s["n_failed"].sum()) == 0, "the benchmark signal lost access units"
            out[name] = dict(ms_per_step=ms, ratio_to_off=min(out["off_ms"]) / ms, buffer_bytes=int(nb), stored_bytes_per_step=stored, aus_per_step=int(s["n_aus"].sum()),
                             table_bytes=int(na) * capi.AU_DESC_DTYPE.itemsize if TABLE else 0, drain_alone_ms=min(alone) * 1e3, drain_alone_GBps=nb / min(alone) / 1e9,
                             pack_kernel_ms=float(np.median(pack_ms)), copy_f4_ms_same_bytes=2 * stored / (dev.time_copy(max(stored, 1 << 20), 0, 5) * 1e9) * 1e3)
        finally:
            dev.au_drain_wait()
            dev.host_free(buf)
            if TABLE:
                dev.host_free(aus)
    dev.set_au_drain(capi.AU_OFF)
    step()
    out["off_again_ms"] = timed(step)
    dev.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
