"""Host-side check of welle.io_amd/csrc/batch_rows.h (tests/native/batch_rows_check.cpp): the first row a pair emits in a batch equals
the loop the kernels carried (clamped to the batch's rows) and the expression the host getter carried (not clamped) for c0 - cif0 in
-4 .. 40 and 0, 4 .. 24 rows; the layout of the superframe filter's carried window is asserted when the checker compiles."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_first_row_and_window_state_layout(tmp_path):
    exe = str(tmp_path / "batch_rows_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "tests", "hipemu"), "-I", os.path.join(ROOT, "welle.io_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "native", "batch_rows_check.cpp")])
    r = json.loads(subprocess.check_output([exe]).decode())
    assert r["errors"] == 0 and r["cases"] == 4 * 45 * 7             # first frame numbers x distances x row counts
