"""Host-side check of welle.io_amd/csrc/decode_work.h (tests/native/decode_work_check.cpp): the work-item word of the decoders' work
lists round-trips at both of its limits, and the state-parallel kernels' history geometry -- what the host reserves and the kernels
store into -- equals the literal formulas (nsteps / 30 + 1) * 32 and * 64 for every code word length there is."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_work_items_and_history_geometry(tmp_path):
    exe = str(tmp_path / "decode_work_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "tests", "hipemu"), "-I", os.path.join(ROOT, "welle.io_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "native", "decode_work_check.cpp")])
    r = json.loads(subprocess.check_output([exe]).decode())
    assert r["item_errors"] == 0 and r["items"] == 24
    assert r["geometry_errors"] == 0 and r["lengths"] == 49          # 48 bit rates and the FIC
    assert (r["hist_steps"], r["max_classes"], r["max_groups"]) == (30, 255, 0xffffff)
