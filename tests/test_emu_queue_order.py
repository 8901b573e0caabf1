"""What dabphy_process hands to which stream, in which order.  The CPU execution model of tests/hipemu runs every launch, copy and
wait at once, so a hipStreamWaitEvent on the wrong stream or a kernel moved to another stream passes every other GPU-less test; its
queue-order trace (hipemu_trace_start / hipemu_trace_read: one line per launch, event record, wait, synchronisation and asynchronous
copy or fill -- op, stream, event, kernel, grid, block, bytes; streams and events named by the order in which the handle created
them) is compared here, byte for byte, with the text files of tests/queue_order: one per scenario, a few small batches each, the
first call after creation left out (it grows the buffers and acquires).

The files pin the schedule of the commit that introduced them; they were recorded from its PARENT (the library before dabphy_process
was split into steps) with only the trace hook added.  A deliberate change of the schedule records them again:
DABPHY_RECORD_QUEUE_ORDER=1 python -m pytest tests/test_emu_queue_order.py, and the diff of tests/queue_order is the review.  The two
emulated builds differ in the demod kernel's block (DEMOD_WAVES); the product build's files are <scenario>.product.txt."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mp2_chain
import parity_cases as P
from conftest import EMU_LIB, PKG_DIR, ROOT
from welle_io_amd import capi, synth

PRODUCT_LIB = os.path.join(ROOT, "tests", "hipemu", "libdabphy_emu_product.so")
EXPECTED_DIR = os.path.join(ROOT, "tests", "queue_order")
B = 2


@pytest.fixture(scope="module")
def low_snr():
    """the stream of test_exact_batch_mode's replay=True cases (3 dB, -1000 Hz, seed 5): four frames per call, its first batch is decoded twice"""
    return synth.make_stream(25, snr_db=3, cfo_hz=-1000, delay=150, return_tx=True, seed=5)


@pytest.fixture(scope="module")
def mp2_stream():
    subchs, payload = mp2_chain.ensemble()
    return synth.make_stream(13, snr_db=20, cfo_hz=20, delay=50, seed=3, payload_fn=payload, subchs=subchs), subchs


def plain(d):
    pass


# name: (configuration, frames per call, calls, set-up after the sub-channels, environment of the experiments build, must replay)
SCENARIOS = {
    "pipeline_sync_0": (dict(pipeline_sync=0, exact_batch=False), 3, 4, plain, {}, False),
    "pipeline_sync_1": (dict(pipeline_sync=1, exact_batch=False), 3, 4, plain, {}, False),
    "pipeline_sync_2": (dict(pipeline_sync=2, exact_batch=False), 3, 4, plain, {}, False),
    "pipeline_sync_3": (dict(pipeline_sync=3, exact_batch=False), 3, 4, plain, {}, False),
    "sync_early_0_schedule_1": (dict(pipeline_sync=1, sync_early=0), 3, 4, plain, {}, False),
    "sync_early_1_schedule_1": (dict(pipeline_sync=1, sync_early=1), 3, 4, plain, {}, False),
    "replay_schedule_0": (dict(pipeline_sync=0), 4, 3, plain, {}, True),
    "replay_schedule_1": (dict(pipeline_sync=1), 4, 3, plain, {}, True),
    "replay_state_parallel": (dict(pipeline_sync=0, decode_shape=2), 4, 3, plain, {}, True),
    "auto_superframes_1": (dict(pipeline_sync=0), 3, 4, lambda d: d.set_auto_superframes(1), {}, False),
    "auto_superframes_2": (dict(pipeline_sync=1), 3, 4, lambda d: d.set_auto_superframes(2), {}, False),
    "auto_superframes_2_schedule_3": (dict(pipeline_sync=3), 3, 4, lambda d: d.set_auto_superframes(2), {}, False),
    "auto_mp2": (dict(pipeline_sync=0), 3, 4, None, {}, False),
    "tii": (dict(pipeline_sync=0), 3, 4, lambda d: d.set_tii(True), {}, False),
    "two_kernel_msc": (dict(pipeline_sync=0), 3, 3, plain, {"DABPHY_FUSED_MSC": "0"}, False),
    "fic_own_pair": (dict(pipeline_sync=0), 3, 3, plain, {"DABPHY_FUSED_FIC": "0"}, False),
    "one_frame_schedule_1": (dict(pipeline_sync=1), 1, 5, plain, {}, False),
    "traceback_split": (dict(pipeline_sync=0, decode_shape=1), 3, 3, plain, {"DABPHY_TB_SPLIT": "1"}, False),
}


def trace_text(lib):
    n = lib.hipemu_trace_read(None, C.c_int64(0))
    buf = C.create_string_buffer(max(n, 1))
    assert lib.hipemu_trace_read(buf, C.c_int64(n)) == n
    return buf.raw[:n].decode()


def run_scenario(lib_path, name, low_snr, mp2_stream):
    cfg, F, calls, setup, _, must_replay = SCENARIOS[name]
    lib = C.CDLL(lib_path)
    lib.hipemu_trace_read.restype = C.c_int64
    lib.hipemu_trace_start()                    # (in front of dabphy_create: the handle's streams and events count from 0)
    d = capi.DabPhy(lib_path=lib_path, n_ensembles=B, max_frames=F, want_constellation=False, want_impulse_response=False, **cfg)
    try:
        if name == "auto_mp2":
            x, subchs = mp2_stream
            d.stream_upload(np.tile(np.asarray(x, np.complex64), (B, 1)))
            d.set_subchannels([(s.subch_id, s.start_cu, s.size_cu, P.dev_prot(d, s)) for s in subchs])
            for b in range(B):
                d.set_audio_kinds_ensemble(b, [1, 0, 0, 0, 0])          # one MP2 position
            d.set_auto_mp2(True)
        else:
            x, tx = low_snr
            d.stream_upload(np.tile(np.asarray(x, np.complex64), (B, 1)))
            d.set_subchannels([(s.subch_id, s.start_cu, s.size_cu, P.dev_prot(d, s)) for s in (tx.subchs[0], tx.subchs[5], tx.subchs[9])])
            setup(d)
        d.process(F)
        if must_replay:
            # with these inputs (F = 4) it is the batch that acquires which is decoded twice: the stream starts over behind the first
            # call, so that the replayed batch is a traced one
            d.reset()
        skip = len(trace_text(lib))
        for _ in range(calls - 1):
            d.process(F)
        text = trace_text(lib)[skip:]
        if must_replay:
            assert d.replayed_batches() >= 1, "no batch of this scenario was decoded twice"
        return text
    finally:
        d.close()


# (the product build reads no environment -- dabphy_internal.h, debug_env --: the scenarios behind a switch run on the experiments build)
CASES = [("experiments", n) for n in sorted(SCENARIOS)] + [("product", n) for n in sorted(SCENARIOS) if not SCENARIOS[n][4]]


@pytest.mark.parametrize("build,name", CASES)
def test_queue_order(emu, low_snr, mp2_stream, build, name, monkeypatch):
    env = SCENARIOS[name][4]
    for k in ("DABPHY_FUSED_MSC", "DABPHY_FUSED_FIC", "DABPHY_TB_SPLIT", "DABPHY_STREAM_LAYOUT", "DABPHY_CHAIN_EARLY", "DABPHY_DEBUG_TIMING"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    lib_path = EMU_LIB
    if build == "product":
        subprocess.run(["make", "-j8", "emu-product"], cwd=os.path.join(PKG_DIR, "csrc"), check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
        lib_path = PRODUCT_LIB
    text = run_scenario(lib_path, name, low_snr, mp2_stream)
    assert text.count("\n") > 10
    path = os.path.join(EXPECTED_DIR, name + (".product.txt" if build == "product" else ".txt"))
    if os.environ.get("DABPHY_RECORD_QUEUE_ORDER"):
        os.makedirs(EXPECTED_DIR, exist_ok=True)
        with open(path, "w") as f:
            f.write(text)
        return
    with open(path) as f:
        want = f.read()
    got_lines, want_lines = text.splitlines(), want.splitlines()
    first = next((i for i, (a, b) in enumerate(zip(got_lines, want_lines)) if a != b), min(len(got_lines), len(want_lines)))
    assert text == want, "%s: %d records, %d expected; first difference at record %d: got %r, expected %r" % (
        name, len(got_lines), len(want_lines), first, got_lines[first:first + 1], want_lines[first:first + 1])
