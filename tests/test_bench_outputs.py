"""bench.py without --full and its --dump-outputs: the plain line carries the headline alone, two runs with the same arguments dump the
same outputs, and a dump larger than its budget becomes a fixed sample of ensembles.  The runs are on the kernels' CPU execution model
(DABPHY_BENCH_EMU=1, TEST ONLY: the glue, not a measurement); tests/test_gpu_bench_entry.py runs the same on the device."""
import json
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT


def run_bench_emu(args):
    env = dict(os.environ, DABPHY_BENCH_EMU="1", OMP_NUM_THREADS="1", DABPHY_PIPELINE="1", DABPHY_SP_MAX_CW="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_line_and_dumped_outputs_on_the_execution_model(emu, tmp_path):
    # (2 frames per step: the superframe filter is synchronised after seven warm-up steps, as in tests/test_dist_gloo.py)
    args = ["--gpus", "1", "--steps", "2", "--warmup", "7", "--ensembles", "2", "--frames", "2"]
    runs = [run_bench_emu(args + ["--dump-outputs", str(tmp_path / d)]) for d in ("a", "b")]
    for j in runs:
        assert j["steps"] == 2 and j["warmup"] == 7 and j["ms_per_step"] > 0
        assert abs(j["value"] - 2 * 2 * 0.096 / (j["ms_per_step"] * 1e-3)) < 1e-6 * j["value"]
        for k in ("metric", "unit", "higher_is_better", "dtype", "roofline", "stages_ms"):
            assert k in j, k
        for k in ("cpu_baseline", "parity_check", "extras", "facade", "host_u8", "msc_drain", "alt_schedules"):
            assert k not in j, k
    for name, shape, dtype in (("fibs", (2, 2, 12, 32), np.float32), ("crc_ok", (2, 2, 12), np.float32), ("superframes", (2, 4), np.float64)):
        a, b = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert a.shape == shape and a.dtype == dtype and np.array_equal(a, b), name
    assert np.load(tmp_path / "a" / "crc_ok.npy").all()
    assert not os.path.exists(tmp_path / "a" / "ensembles.npy")


def test_dump_of_a_large_batch_is_a_fixed_sample(tmp_path):
    import bench
    rs = np.random.RandomState(5)
    E, F = 1400, 32                                        # 1400 x 32 x 396 x 4 bytes = 71 MB as float32: over the budget
    fib = rs.randint(0, 256, (E, F, 12, 32)).astype(np.uint8)
    ok = rs.randint(0, 2, (E, F, 12)).astype(np.uint8)
    sf = rs.randint(0, 100, (E, 4)).astype(np.int32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), fib, ok, sf)
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in os.listdir(tmp_path / "a")) <= bench.DUMP_MAX_BYTES
    rows = np.load(tmp_path / "a" / "ensembles.npy").astype(np.int64)
    assert np.array_equal(rows, np.load(tmp_path / "b" / "ensembles.npy")) and len(rows) < E
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < E
    assert np.array_equal(np.load(tmp_path / "a" / "fibs.npy"), fib[rows].astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "a" / "crc_ok.npy"), ok[rows].astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "a" / "superframes.npy"), sf.astype(np.float64))
