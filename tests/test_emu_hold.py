"""The execution model's held stream (tests/hipemu: hipemu_hold_stream).  The model runs every op when it is queued -- the EARLIEST order the
device may choose -- so a missing cross-stream wait passes unless host order happens to expose it.  Holding one stream gives it the latest
legal order instead: its ops run only when something the runtime orders behind them is met.  Self-test on toy programs, then the receiver
with each of its working streams held in turn: every result must still be the oracle's.

Limit: a kernel of an eager stream that spins on a flag a kernel of the held stream publishes makes the held order one the device cannot
produce.  The only such pair in the library is the split traceback (DABPHY_TB_SPLIT: walkers on tb_stream consume what the fused decoder
on the main stream publishes); it is off in every scenario here, so no stream is left out."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

import parity_cases as P
from conftest import EMU_LIB, ROOT
from welle_io_amd import capi


def test_held_stream_self_test(tmp_path):
    """two-stream toy programs: with the wait the consumer reads the producer's value whichever stream is held; without it the eager model
    still does (the defect is invisible) and holding the producer shows it.  Every covered op queues in order, every drain point drains,
    a wait drains only as far as the awaited record."""
    exe = str(tmp_path / "hold_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "tests", "hipemu"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "hold_check.cpp"), os.path.join(ROOT, "tests", "hipemu", "hipemu.cpp")])
    r = json.loads(subprocess.check_output([exe]).decode())
    assert r["wait_eager"] == r["wait_hold_producer"] == r["wait_hold_consumer"] == 7, r
    assert r["nowait_eager"] == 7 and r["nowait_hold_consumer"] == 7 and r["nowait_hold_producer"] == 0, r
    assert r["ops"] == [1] * 6 and r["partial_drain"] == 1, r


@pytest.fixture(scope="module")
def lib(emu):
    l = C.CDLL(EMU_LIB)
    l.hipemu_trace_read.restype = C.c_int64
    l.hipemu_hold_stream.argtypes = [C.c_int64]
    return l


def trace_text(lib):
    n = lib.hipemu_trace_read(None, C.c_int64(0))
    buf = C.create_string_buffer(max(n, 1))
    lib.hipemu_trace_read(buf, C.c_int64(n))
    return buf.raw[:n].decode()


def held_factory(lib, index):
    def make(**kw):
        lib.hipemu_trace_start()                # (in front of dabphy_create: the handle's streams count from 0, as in tests/queue_order)
        d = capi.DabPhy(lib_path=EMU_LIB, **kw)
        if index is not None:
            lib.hipemu_hold_stream(index)
        return d
    return make


SCENARIOS = {
    "deferred_schedule_3_F1": lambda f: P.check_deferred_superframes(f, 3, 1),
    "deferred_schedule_3_F3": lambda f: P.check_deferred_superframes(f, 3, 3),
    "immediate_schedule_3": lambda f: P.check_deferred_superframes(f, 3, 3, mode=1),
    "plain_schedule_3": lambda f: P.check_stream_vs_oracle(f, 16, -20, 50, 14, False, F=3, pipeline_sync=3, disable_coarse=True),
}
_working = {}


def working_streams(lib, name):
    """the streams that carry launches, copies or fills in the scenario, read from the trace of a run with nothing held (which must pass)"""
    if name not in _working:
        SCENARIOS[name](held_factory(lib, None))
        _working[name] = sorted({int(m) for m in re.findall(r"^(?:launch|memcpy|memcpy2d|memset) s(\d+) ", trace_text(lib), re.M)})
    return _working[name]


# the working streams, by creation order in dabphy_create behind its five placeholder streams (dabphy_api.hip): main s5, synchroniser s6,
# auxiliary s7 (the deferred pass rides on it), FIC verdict s9; s8, the split traceback's, carries nothing here.  An exact list, so that a
# run that holds nothing, or misses a stream, cannot look like coverage
EXPECTED_STREAMS = [5, 6, 7, 9]


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_receiver_with_each_working_stream_held(lib, name):
    streams = working_streams(lib, name)
    assert streams == EXPECTED_STREAMS, streams
    for index in streams:
        try:
            SCENARIOS[name](held_factory(lib, index))
        except AssertionError as e:
            raise AssertionError("with stream s%d held: %s" % (index, e)) from e
        finally:
            lib.hipemu_hold_none()
