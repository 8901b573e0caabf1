"""Not a test: times the superframe filter's wide pass (k_superframe_wide) ALONE on the benchmark batch (dabphy_time_superframe_wide: the wide
launches of the last filter pass run again with nothing else on the device) and prints what the pass settled.
usage: python tools/time_sf_wide.py [B] [F] ; DABPHY_LIB selects the library."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package, PKG_DIR  # noqa: E402

load_package()
import torch  # noqa: E402
from welle_io_amd import capi, workload  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
F = int(sys.argv[2]) if len(sys.argv) > 2 else 32
lib = os.environ.get("DABPHY_LIB", os.path.join(PKG_DIR, "libdabphy_hip.so"))
rec = workload.rec_frames_for(F)
iq, cfo, base, txs = workload.make_batch(B, rec_frames=rec)
dev = workload.open_receiver(capi, lib, iq, F, txs[0].subchs)
for _ in range(4):
    dev.process(F)
torch.cuda.synchronize()
settled, tried = dev.wide_superframe_stats()
times = [dev.time_superframe_wide(20) for _ in range(5)]
pairs = B * len(txs[0].subchs)
print("k_superframe_wide alone (%s): %s ms per launch, five means of 20 (%d x %d: %d pairs, %d CIFs each; pair batches settled / tried so far %d / %d)"
      % (os.path.basename(lib), " ".join("%.4f" % t for t in times), B, F, pairs, 4 * F, settled, tried))
dev.close()
