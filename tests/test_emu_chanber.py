"""The channel BER pass (k_chanber.hip) in the CPU execution model of tests/hipemu: the stateless entry against the model
(tests/chanber_model.py) on every case of tests/chanber_cases.py, and the pass inside dabphy_process on small geometries against the model
fed with the oracle run's soft bits and bytes.  The device twin is tests/test_gpu_chanber.py."""
import ctypes as C

import numpy as np
import pytest

import chanber_cases as K
from conftest import EMU_LIB
from welle_io_amd import capi


def factory(**kw):
    return capi.DabPhy(lib_path=EMU_LIB, **kw)


def test_linear_entry_matches_the_model(emu):
    assert K.check_directed(emu) == 6 * (1 + 3 + 65)


def test_linear_entry_on_a_profile_sweep(emu):
    """the lin_sweep_profiles() subset here (all 304 with DABPHY_FULL_CPU_SUITE=1, and on the device)"""
    assert K.check_profile_sweep(emu, K.sweep_profiles(full=False)) >= 64


def test_entry_errors(emu):
    K.check_entry_errors(emu, capi)


@pytest.mark.parametrize("pipeline_sync", [0, 1, 2, 3])
@pytest.mark.parametrize("F", [1, 3])
def test_streaming_small(emu, F, pipeline_sync):
    K.check_streaming_small(factory, F, pipeline_sync)


def test_counts_through_a_replayed_batch(emu):
    K.check_replayed_batch(factory)


def test_service_change_in_mid_stream(emu):
    K.check_service_change(factory)


def test_off_means_off(emu):
    K.check_off_means_off(factory, capi)


def test_the_handle_owns_the_pass_buffers(emu):
    """the execution model counts the device blocks, page-locked blocks, streams and events alive: switching the pass off gives its six
    device buffers back, closing the handle leaves nothing behind, and with the pass never switched on not one block more exists"""
    x, subs, _ = K.mixed_stream()
    lib = C.CDLL(EMU_LIB)

    def live():
        out = (C.c_int64 * 4)()
        lib.hipemu_live_counts(out)
        return tuple(out)
    before = live()
    seen = {}
    for on in (False, True):
        d = factory(n_ensembles=2, max_frames=2, want_constellation=False)
        try:
            d.stream_upload(np.tile(np.asarray(x, np.complex64), (2, 1)))
            d.set_subchannels([K.sub_tuple(d, s) for s in subs])
            if on:
                d.set_channel_ber(True)
            d.process(2); d.process(2)
            seen[on] = live()
            if on:
                d.set_channel_ber(False)
                seen["released"] = live()
        finally:
            d.close()
        assert live() == before
    assert seen[True][0] == seen[False][0] + 6 and seen[True][1:] == seen[False][1:], seen
    assert seen["released"] == seen[False], seen


def trace_text(lib):
    n = lib.hipemu_trace_read(None, C.c_int64(0))
    buf = C.create_string_buffer(max(n, 1))
    assert lib.hipemu_trace_read(buf, C.c_int64(n)) == n
    return buf.raw[:n].decode()


@pytest.mark.parametrize("cfg", [dict(pipeline_sync=0), dict(pipeline_sync=1), dict(pipeline_sync=3, sync_early=1)])
def test_launch_sequence_with_the_feature_off_and_on(emu, cfg):
    """the queue-order trace of the execution model (tests/test_emu_queue_order.py pins the sequence with the feature off against the
    recorded files): with the feature on, the same sequence plus the pass's two launches per batch on the main stream, directly in
    front of the call's wait for that stream -- nothing else moves, nothing else is added"""
    x, subs, _ = K.mixed_stream()
    lib = C.CDLL(EMU_LIB)
    lib.hipemu_trace_read.restype = C.c_int64
    texts = []
    for on in (False, True):
        lib.hipemu_trace_start()
        d = factory(n_ensembles=2, max_frames=2, want_constellation=False, want_impulse_response=False, **cfg)
        try:
            d.stream_upload(np.tile(np.asarray(x, np.complex64), (2, 1)))
            d.set_subchannels([K.sub_tuple(d, s) for s in subs])
            if on:
                d.set_channel_ber(True)
            d.process(2)
            skip = len(trace_text(lib))
            for _ in range(2):
                d.process(2)
            texts.append(trace_text(lib)[skip:].splitlines())
        finally:
            d.close()
    off, on = texts
    mine = [i for i, l in enumerate(on) if "k_chanber" in l]
    assert len(mine) == 4 and all("k_chanber" not in l for l in off)
    assert [l for l in on if "k_chanber" not in l] == off
    for i in mine[1::2]:
        assert on[i - 1].split()[1] == on[i].split()[1] == on[i + 1].split()[1] and on[i + 1].startswith("stream_sync"), on[i - 1:i + 2]
