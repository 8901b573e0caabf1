"""What a handle leaves behind.  The CPU execution model of tests/hipemu counts the device blocks, page-locked blocks, streams and events
that are alive (hipemu_live_counts) and aborts on the release of something that is not.  Every check here is a delta -- the session's
`emu` handle stays open in this process --: read the counts, run a scenario on handles of its own, close them, read again; all four
counts must be what they were.  One more test pins the order, flags and priorities in which a fresh handle creates its streams
(dabphy_create_v2, "stream placement": the order is worth 3 % of the benchmark step on the device)."""
import contextlib
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mp2_cases
import mp2_chain
import parity_cases as P
from conftest import EMU_LIB, PKG_DIR, ROOT
from welle_io_amd import capi, synth

PRODUCT_LIB = os.path.join(ROOT, "tests", "hipemu", "libdabphy_emu_product.so")
KINDS = ("device blocks", "page-locked blocks", "streams", "events")
T_F = 196608


def factory(**kw):
    return capi.DabPhy(lib_path=EMU_LIB, **kw)


def live(lib_path=EMU_LIB):
    out = (C.c_int64 * 4)()
    C.CDLL(lib_path).hipemu_live_counts(out)
    return tuple(out)


@contextlib.contextmanager
def nothing_left_behind(lib_path=EMU_LIB):
    before = live(lib_path)
    yield
    after = live(lib_path)
    assert after == before, "left behind: " + ", ".join("%d %s" % (a - b, k) for a, b, k in zip(after, before, KINDS) if a != b)


@pytest.fixture(scope="module")
def stream18():
    """six frames of the default multiplex (18 sub-channels of 64 kbit/s), clean enough that every frame decodes"""
    return synth.make_stream(6, snr_db=20, cfo_hz=30, delay=77, return_tx=True, seed=9)


def subs_of(d, tx, idx):
    return [(tx.subchs[i].subch_id, tx.subchs[i].start_cu, tx.subchs[i].size_cu, P.dev_prot(d, tx.subchs[i])) for i in idx]


@contextlib.contextmanager
def receiver(x, tx, idx=(3, 10), B=1, F=2, **kw):
    """a handle of its own with the stream uploaded and the sub-channels applied; closed on the way out whatever happened"""
    d = factory(n_ensembles=B, max_frames=F, **kw)
    try:
        d.stream_upload(np.tile(np.asarray(x, np.complex64), (B, 1)))
        d.set_subchannels(subs_of(d, tx, idx))
        yield d
    finally:
        d.close()


def test_create_and_destroy(emu):
    with nothing_left_behind():
        factory().close()
        factory(n_ensembles=3, max_frames=4, want_constellation=False, want_impulse_response=False).close()


def test_refused_configuration_destroys_the_half_built_handle(emu):
    """dabphy_create_v2 refuses pipeline_sync = 9 after the handle object exists: dabphy_destroy runs on a handle without streams, events
    or buffers"""
    with nothing_left_behind():
        for kw in (dict(pipeline_sync=9), dict(decode_shape=4), dict(sync_early=-1)):
            with pytest.raises(capi.DabPhyError):
                factory(**kw)


@pytest.mark.parametrize("pipeline", [0, 3])
def test_sub_channel_lists_in_turn(emu, stream18, pipeline):
    """two lists in turn -- sub-channel 5 stays (its state is carried), 0 goes, 9 is new; then a third with another protection profile
    and an empty one --: apply_subchannels carries, swaps and frees.  Exact batch mode is on (the default)"""
    x, tx = stream18
    with nothing_left_behind():
        with receiver(x, tx, idx=(0, 5), B=2, F=2, pipeline_sync=pipeline, want_constellation=False) as d:
            d.process(2)
            d.set_subchannels(subs_of(d, tx, (5, 9)))
            d.process(2)
            assert d.msc(0)[0].any() and d.msc(1)[0].any()
            p = d.protection_eep(64, True, 2)
            d.set_subchannels_ensemble(1, [(1, 0, 48, p)] + subs_of(d, tx, (9,)))      # a class of its own for one ensemble, applied by process()
            d.process(2)
            d.set_subchannels([])
            d.process(2)
            with pytest.raises(capi.DabPhyError):
                d.set_subchannels([(1, 850, 48, p)])                                    # refused: nothing half-built stays


def test_growing_batches_reallocate(emu, stream18):
    """one, then two, then four frames per call on the serial schedule: every grow-only buffer is replaced twice"""
    x, tx = stream18
    with nothing_left_behind():
        with receiver(x, tx, F=4, want_constellation=True, want_impulse_response=True) as d:
            for n in (1, 2, 4):
                d.process(n)
                d.fibs(); d.msc(0); d.constellation(); d.impulse_response(); d.null_symbols(); d.soft_bits(0, 0)


def test_tii_impulse_response_and_constellation(emu, stream18):
    x, tx = stream18
    with nothing_left_behind():
        with receiver(x, tx, F=2, want_constellation=True, want_impulse_response=True) as d:
            d.set_tii(True)
            d.set_track_slevel(True)
            d.process(2)
            d.tii(); d.constellation(); d.impulse_response(); d.null_symbols()
            d.reset()
            d.process(1)


@pytest.mark.parametrize("mode", [1, 2])
def test_automatic_superframes(emu, stream18, mode):
    """the filter inside dabphy_process (1) and deferred to the next call on a stream of its own (2); the one-sub-channel getter too"""
    x, tx = stream18
    with nothing_left_behind():
        with receiver(x, tx, F=2, want_constellation=False, pipeline_sync=1 if mode == 2 else 0) as d:
            d.set_auto_superframes(mode)
            for _ in range(2):
                d.process(2)
                d.superframes_stats()
            d.superframes(0, tx.subchs[3].bitrate)
            d.superframes_ensemble(0, 1, tx.subchs[10].bitrate)


def test_mp2_kinds_with_the_automatic_pass(emu):
    """MP2 and DAB+ services side by side, the MP2 pass inside dabphy_process with profiling on, a kind switched between batches; the unit
    entry on a handle of its own"""
    subchs, payload = mp2_chain.ensemble()
    x = synth.make_stream(11, snr_db=20, cfo_hz=20, delay=50, seed=3, payload_fn=payload, subchs=subchs)
    with nothing_left_behind():
        d = factory(n_ensembles=1, max_frames=2, want_constellation=False)
        try:
            d.stream_upload(np.asarray(x, np.complex64)[None])
            d.set_subchannels([(s.subch_id, s.start_cu, s.size_cu, P.dev_prot(d, s)) for s in subchs])
            d.set_audio_kinds_ensemble(0, [1, 0, 1, 0, 0])
            d.set_auto_mp2(True); d.set_auto_superframes(True); d.set_profiling(True)
            checked = 0
            for _ in range(3):
                d.process(2)
                checked += int(d.mp2_stats()[0, 0])
                d.mp2_ms(); d.mp2_frames_ensemble(0, 0)
            assert checked > 0
            d.set_audio_kinds_ensemble(0, [1, 0, 0, 1, 0])
            d.set_auto_mp2(False)
            d.process(2)
            d.mp2_stats()
            d.set_subchannels([(s.subch_id, s.start_cu, s.size_cu, P.dev_prot(d, s)) for s in subchs[1:]])      # the MP2 classes go
            d.process(1)
        finally:
            d.close()
        u = factory()
        try:
            s, fl = mp2_cases.clean(64, n=4)
            ev, ne, fe, fu = u.mp2_check(s, fl)
            assert ne[0] == 4
        finally:
            u.close()


@pytest.mark.parametrize("own_drain_stream", [False, True])
def test_raw_asynchronous_ingest_and_the_bulk_drain(emu, stream18, own_drain_stream):
    """a live ring fed through dabphy_stream_write_raw_async (the drain then takes a stream of its own) or through the synchronous entry
    (the drain rides on the ingest stream: an alias, not a second stream); a drain begun and waited for, and one left in flight"""
    x, tx = stream18
    raw, _ = P.raw_encode(x, "u8")
    with nothing_left_behind():
        d = factory(n_ensembles=1, max_frames=1, want_constellation=False)
        try:
            d.stream_open(4 * T_F)
            d.set_subchannels(subs_of(d, tx, (2, 11)))
            pinned = None
            for k in range(3):
                piece = np.ascontiguousarray(raw[k * T_F:(k + 1) * T_F + (T_F // 2 if k == 2 else 0)])
                if own_drain_stream:
                    d.stream_write_raw_async(piece, "u8"); d.stream_commit()
                else:
                    d.stream_write_raw(piece, "u8")
                d.process(1)
                if k == 0:
                    d.msc_batch()
                    nb, nd = d.msc_batch_size()
                    pinned = d.host_alloc((max(nb, 1),), np.uint8)
                else:
                    d.msc_drain_begin(pinned, np.zeros(nd, capi.MSC_DESC_DTYPE))      # completed by the next process() / by close()
            d.close()
            d.host_free(pinned)
        finally:
            d.close()


@pytest.mark.parametrize("shape", [2, 3])
def test_state_parallel_decoders_and_the_one_class_seams(emu, stream18, shape):
    """decode_shape 2 / 3: k_viterbi_sp2 + k_traceback_sp2 / k_viterbi_sp for the batch and for the seams' one-class launches"""
    x, tx = stream18
    with nothing_left_behind():
        with receiver(x, tx, idx=(3,), F=1, want_constellation=False, decode_shape=shape) as d:
            d.process(1)
            assert d.last_decode_plan() == (shape, 1)
            P.check_viterbi(d, 768, 3, seed=5, kind="uniform")
            P.check_fic_arbitrary_int8(d, n_frames=1)
            P.check_msc_deconvolve(d, "eep", 32, False, 3, 2, seed=4)


def test_profiling_and_the_two_kernel_decode(emu, stream18, monkeypatch):
    x, tx = stream18
    monkeypatch.setenv("DABPHY_FUSED_MSC", "0")
    monkeypatch.setenv("DABPHY_FUSED_FIC", "0")
    with nothing_left_behind():
        with receiver(x, tx, F=2, want_constellation=False) as d:
            d.set_profiling(True)
            d.process(2)
            assert d.stage_times()["msc_gather"] > 0.0
            d.rs_decode_msc(0, np.zeros(1, np.int32))
        u = factory()
        try:
            u.rs_superframes(np.zeros((2, 120 * 8), np.uint8), 8)
        finally:
            u.close()


@pytest.mark.parametrize("walkers", [False, True])
def test_traceback_split_of_the_experiments_build(emu, stream18, walkers, monkeypatch):
    """the lane-per-code-word kernel's traceback as a pass of its own: per-group flags, a stream and two events created on first use
    (with the walker waves: a page-locked word too)"""
    x, tx = stream18
    with nothing_left_behind():
        with receiver(x, tx, F=2, want_constellation=False, decode_shape=1) as d:
            d.traceback_split(3 if walkers else 1)
            d.process(2)
            assert d.last_decode_plan() == (1, 1)
            assert d.time_fused_msc(1) > 0.0
    monkeypatch.setenv("DABPHY_TB_SPLIT", "1")
    with nothing_left_behind():
        with receiver(x, tx, F=1, want_constellation=False, decode_shape=1) as d:
            d.process(1)


def test_self_tests_and_timing_drivers(emu, stream18):
    x, tx = stream18
    frames = P.cut_frames(x, 1)
    with nothing_left_behind():
        d = factory(n_ensembles=1, max_frames=2)
        try:
            assert d.selftest_unit_twiddle()[0] == 0
            assert d.selftest_pair_exchange()[0] == 0
            assert d.selftest_div127()[:2] == [0, 0]
            assert d.time_demod(frames, 1, 1, iters=1) >= 0.0
            assert min(d.time_viterbi(192, 64, iters=1)) >= 0.0
            assert d.time_copy(1 << 16, 0, 1) > 0.0
        finally:
            d.close()
        P.check_timing_driver_refuses_a_stale_launch(factory)


def stream_creations(lib_path):
    lib = C.CDLL(lib_path)
    lib.hipemu_stream_creations.restype = C.c_int64
    n = lib.hipemu_stream_creations(None, C.c_int64(0))
    buf = (C.c_int64 * (2 * max(n, 1)))()
    assert lib.hipemu_stream_creations(buf, C.c_int64(n)) == n
    return [(buf[2 * i], buf[2 * i + 1]) for i in range(n)]


NON_BLOCKING, DEFAULT, HIGH = 1, 0, -1          # hipStreamNonBlocking; the execution model's priority range is (least 0, greatest -1)
# five placeholders (the second one high priority), main, synchroniser (high priority), auxiliary, copy, FIC
STREAMS_OF_A_FRESH_HANDLE = [(NON_BLOCKING, DEFAULT), (NON_BLOCKING, HIGH), (NON_BLOCKING, DEFAULT), (NON_BLOCKING, DEFAULT), (NON_BLOCKING, DEFAULT),
                             (NON_BLOCKING, DEFAULT), (NON_BLOCKING, HIGH), (NON_BLOCKING, DEFAULT), (NON_BLOCKING, DEFAULT), (NON_BLOCKING, DEFAULT)]


@pytest.mark.parametrize("build", ["experiments", "product"])
def test_stream_creation_order(emu, stream18, build, monkeypatch):
    """order, flags and priorities of the streams a handle creates: ten at creation, nothing more through a plain batch; the drain stream
    on the first bulk drain of a handle that ingests asynchronously, never before"""
    monkeypatch.delenv("DABPHY_STREAM_LAYOUT", raising=False)
    lib_path = EMU_LIB
    if build == "product":
        subprocess.run(["make", "-j8", "emu-product"], cwd=os.path.join(PKG_DIR, "csrc"), check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
        lib_path = PRODUCT_LIB
    x, tx = stream18
    with nothing_left_behind(lib_path):
        n0 = len(stream_creations(lib_path))
        d = capi.DabPhy(lib_path=lib_path, n_ensembles=1, max_frames=1, want_constellation=False, decode_shape=1)
        try:
            assert stream_creations(lib_path)[n0:] == STREAMS_OF_A_FRESH_HANDLE
            raw, _ = P.raw_encode(x, "u8")
            d.stream_open(4 * T_F)
            d.set_subchannels(subs_of(d, tx, (3,)))
            piece = np.ascontiguousarray(raw[:2 * T_F])
            d.stream_write_raw_async(piece, "u8"); d.stream_commit()
            d.process(1)
            assert stream_creations(lib_path)[n0:] == STREAMS_OF_A_FRESH_HANDLE
            d.msc_batch()
            assert stream_creations(lib_path)[n0:] == STREAMS_OF_A_FRESH_HANDLE + [(NON_BLOCKING, DEFAULT)]
        finally:
            d.close()
