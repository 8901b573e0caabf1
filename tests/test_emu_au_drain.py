"""CPU suite: the bulk access-unit drain (dabphy_set_au_drain, k_au.hip unchanged under the execution model of tests/hipemu) against
tests/au_model.py on the oracle's events -- tests/au_cases.py, the cases the device suite runs too (tests/test_gpu_au_drain.py) -- and what only the execution
model can show: what a handle with drains in flight leaves behind, when the drain's stream is created, and where the pack pass stands
in the queues."""
import ctypes as C

import numpy as np
import pytest

import au_cases as A
import parity_cases as P
from conftest import EMU_LIB
from welle_io_amd import capi

RAW, LOAS = capi.AU_RAW, capi.AU_LOAS
T_F = 196608


def factory(**kw):
    return capi.DabPhy(lib_path=EMU_LIB, **kw)


@pytest.mark.parametrize("fmt", A.FORMATS)
def test_unit_corners(emu, fmt):
    A.check_unit_corners(emu, fmt)


@pytest.mark.parametrize("fmt", A.FORMATS)
def test_unit_length_and_alignment_sweep(emu, fmt):
    A.check_unit_sweep(emu, fmt)


@pytest.mark.parametrize("fmt", A.FORMATS)
def test_unit_capacity(emu, fmt):
    A.check_unit_capacity(emu, fmt)


@pytest.mark.parametrize("fmt", A.FORMATS)
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("F", [3, 5])
def test_through_the_stream(emu, F, mode, fmt):
    A.check_stream(factory, F, mode, fmt)


def test_manual_filter_pass(emu):
    """dabphy_superframes_stats runs the pass itself (no automatic mode): the pack pass follows it there too"""
    A.check_stream(factory, 3, 0, LOAS)


@pytest.mark.parametrize("fmt", A.FORMATS)
def test_mp2_beside_dabplus(emu, fmt):
    A.check_mp2_beside_dabplus(factory, fmt)


@pytest.mark.parametrize("fmt", A.FORMATS)
def test_two_ensembles_with_different_lists(emu, fmt):
    A.check_two_lists(factory, fmt)


@pytest.mark.parametrize("fmt", A.FORMATS)
def test_list_change_behind_a_deferred_pass(emu, fmt):
    A.check_list_change(factory, fmt)


@pytest.mark.parametrize("fmt", A.FORMATS)
@pytest.mark.parametrize("mode", [1, 2])
def test_behind_a_replayed_batch(emu, fmt, mode):
    A.check_replay(factory, fmt, mode)


@pytest.mark.parametrize("fmt", A.FORMATS)
@pytest.mark.parametrize("mode", [1, 2])
def test_replayed_batch_that_stores_access_units(emu, fmt, mode):
    A.check_replay_storing(factory, fmt, mode)


@pytest.mark.parametrize("fmt", A.FORMATS)
def test_protocol(emu, fmt):
    A.check_protocol(factory, fmt)


def test_abi_of_the_new_structures(emu):
    emu.lib.dabphy_struct_size.restype = C.c_size_t
    assert emu.lib.dabphy_struct_size(8) == capi.AU_SERVICE_DTYPE.itemsize == 48 and emu.lib.dabphy_struct_size(9) == capi.AU_DESC_DTYPE.itemsize == 24
    assert emu.lib.dabphy_abi_version() == 6


# ---- execution model only
def live():
    out = (C.c_int64 * 4)()
    C.CDLL(EMU_LIB).hipemu_live_counts(out)
    return tuple(out)


def n_streams():
    lib = C.CDLL(EMU_LIB); lib.hipemu_stream_creations.restype = C.c_int64
    return int(lib.hipemu_stream_creations(None, C.c_int64(0)))


def test_nothing_left_behind_and_one_stream_at_the_first_drain(emu):
    """both drains, the access-unit drain left in flight at close(): every device block, page-locked block, stream and event is released.
    A handle creates no stream beyond the ten of dabphy_create until its first drain.  The first drain of either kind then creates
    EXACTLY ONE on a handle that ingests asynchronously (dabphy_stream_write_raw_async keeps the ingest stream for its transfers) and
    NONE on a handle whose samples are resident in HBM (the drains share the idle ingest stream: drain_stream_ready, as the MSC drain
    always did -- the issue's "then exactly one" holds for the ingesting handle only); no later drain of either kind creates another"""
    x, subs, _ = A.layouts_reference()
    raw, _ = P.raw_encode(x, "u8")
    before = live()
    for ingest, created in ((False, 0), (True, 1)):
        for first in ("au", "msc"):
            s0 = n_streams()
            d = factory(n_ensembles=1, max_frames=3, want_constellation=False)
            try:
                if ingest:
                    d.stream_open(16 * T_F)
                    piece = np.ascontiguousarray(raw[:13 * T_F]); d.stream_write_raw_async(piece, "u8"); d.stream_commit()
                else:
                    d.stream_upload(x[None])
                d.set_subchannels([(s.subch_id, s.start_cu, s.size_cu, d.protection_eep(s.bitrate, s.profile_b, s.level)) for s in subs[:3]])
                d.set_auto_superframes(2); d.set_au_drain(LOAS)
                assert n_streams() == s0 + 10
                d.process(3); d.process(3)
                assert n_streams() == s0 + 10                           # a batch, a deferred pass and its pack pass create none
                if first == "au":
                    d.au_drain_begin()
                else:
                    d.msc_drain_begin()
                assert n_streams() == s0 + 10 + created, (ingest, first)
                d.process(3)
                d.msc_drain_begin(); d.au_drain_begin()
                d.process(3)
                d.msc_drain_wait()
                d.au_drain_begin()                                      # (waits for the one in flight; left in flight itself)
                assert n_streams() == s0 + 10 + created
            finally:
                d.close()
    assert live() == before


def trace(lib):
    lib.hipemu_trace_read.restype = C.c_int64
    n = lib.hipemu_trace_read(None, C.c_int64(0))
    buf = C.create_string_buffer(n + 1)
    assert lib.hipemu_trace_read(buf, C.c_int64(n)) == n
    return [ln.split() for ln in buf.value.decode().splitlines()]


@pytest.mark.parametrize("mode", [1, 2])
def test_queue_order_of_the_pack_pass(emu, mode):
    """the pack launch stands on the filter pass's stream, directly behind that pass's last launch, and waits for the access-unit
    drain's event whenever a drain was begun and not waited for -- and only then"""
    x, subs, _ = A.layouts_reference()
    lib = C.CDLL(EMU_LIB)
    lib.hipemu_trace_start()                                            # (in front of dabphy_create: streams and events count from 0)
    d = A.open_stream(factory, x, subs[:3], 1, 3, mode, RAW)
    try:
        d.process(3); d.process(3)
        mark = [len(trace(lib))]
        d.au_drain_begin()                                              # in flight across the next pass
        d.process(3); mark.append(len(trace(lib)))
        d.au_drain_wait(); d.au_drain_begin(); d.au_drain_wait()        # waited for: the next pass has nothing to wait for
        mark.append(len(trace(lib)))
        d.process(3); mark.append(len(trace(lib)))
    finally:
        d.close()
    ops = trace(lib)
    # the drain's stream and its done event: the first copy behind the first au_drain_begin and the record that follows on its stream
    begin_ops = ops[mark[0]:]
    drain_stream = next(o for o in begin_ops if o[0] == "memcpy")[1]
    done = next(o[2] for o in begin_ops if o[0] == "record" and o[1] == drain_stream)
    for lo, hi, must_wait in ((mark[0], mark[1], True), (mark[2], mark[3], False)):
        seg = ops[lo:hi]
        packs = [i for i, o in enumerate(seg) if o[0] == "launch" and o[3] == "k_au_pack"]
        assert packs, "no pack launch"
        st = seg[packs[0]][1]
        launches = [i for i, o in enumerate(seg) if o[0] == "launch" and o[1] == st]
        before = [seg[i][3] for i in launches if i < packs[0]]
        assert before and before[-1].startswith("k_superframe"), before[-3:]
        waits = [i for i, o in enumerate(seg) if o[0] == "wait" and o[1] == st and o[2] == done and i < packs[0]]
        assert bool(waits) == must_wait, (must_wait, seg[max(0, packs[0] - 6):packs[0] + 1])
