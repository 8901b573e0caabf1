"""The MP2 frame check (k_mp2.hip) in the CPU execution model of tests/hipemu: the unit entry against the model on every case of
tests/mp2_cases.py, and the pass through dabphy_process on small geometries (tests/mp2_chain.py).  The device twin is tests/test_gpu_mp2.py."""
import numpy as np
import pytest

import mp2_cases
import mp2_chain
from conftest import EMU_LIB
from welle_io_amd import capi, synth


def factory(**kw):
    return capi.DabPhy(lib_path=EMU_LIB, **kw)


def test_unit_entry_matches_the_model(emu):
    assert mp2_chain.check_unit_entry(emu, mp2_cases.cases()) > 1000


def test_unit_entry_on_long_streams(emu):
    assert mp2_chain.check_unit_entry(emu, mp2_cases.long_cases()) > 2000


def test_unit_entry_rejects_what_it_cannot_hold(emu):
    with pytest.raises(capi.DabPhyError):
        emu.mp2_check(np.zeros((1, 4 * 2049), np.uint8), 2049)


def test_chain_mixed_ensembles_and_the_dabplus_totals(emu):
    """two ensembles with different kinds at the same positions: every MP2 service's events, error counts and totals equal the model on
    the bytes the device decoded; the DAB+ filter's totals then leave the MP2 services out -- they equal those of a receiver that selects
    only the DAB+ services -- while without kinds the MP2 services still run through the DAB+ filter, as before"""
    checks, sf_kinds, mp2 = mp2_chain.run(factory, F=3, nf=15, B=2)
    assert sorted(checks) == [(0, 0), (0, 2), (0, 3), (1, 0)]
    assert mp2[:, 0].min() > 0 and mp2[0, 1] > 0 and mp2[0, 2] > 0, mp2          # frames everywhere; the damage: CRC failures, a resync
    assert all(c.m.first_unverified < 0 for c in checks.values())
    # DAB+ totals with kinds = the DAB+ positions' own filter results, one service at a time on a receiver without kinds
    dab = [[i for i, k in enumerate(kk) if k == 0] for kk in ([1, 0, 1, 1, 0], [1, 0, 0, 0, 0])]
    _, sf_each, _ = mp2_chain.run(factory, F=3, nf=15, B=2, kinds=[[0] * 5, [0] * 5], sf_auto=False, sf_positions=dab)
    assert np.array_equal(sf_kinds, sf_each), (sf_kinds, sf_each)
    # ... and without kinds the MP2 services run through the DAB+ filter as before: attempts that never synchronise
    _, sf_none, _ = mp2_chain.run(factory, F=3, nf=15, B=2, kinds=[[0] * 5, [0] * 5])
    assert np.array_equal(sf_none[:, 0], sf_kinds[:, 0]) and (sf_none[:, 2] > sf_kinds[:, 2]).all(), (sf_none, sf_kinds)


def test_a_service_switched_to_mp2_mid_stream(emu):
    """position 0 of ensemble 0 becomes MP2 in front of the third batch (fresh parser from there) while position 2, MP2 from the start,
    keeps its parser state through the change of kinds"""
    kinds = [[0, 0, 1, 0, 0]]
    checks, _, _ = mp2_chain.run(factory, F=3, nf=15, B=1, kinds=kinds, switch=(2, 0, 0))
    assert sorted(checks) == [(0, 0), (0, 2)]
    assert checks[(0, 0)].m.feed_no < checks[(0, 2)].m.feed_no
    assert len(checks[(0, 0)].m.events) > 0


@pytest.mark.parametrize("F,auto", [(1, True), (4, False)])
def test_chain_batch_sizes(emu, F, auto):
    """one frame per batch (a logical frame's Feed at a time across batches: the carry) and the pass run by the first getter"""
    mp2_chain.run(factory, F=F, nf=12, B=1, auto_mp2=auto)


def test_mp2_through_a_replayed_batch(emu):
    """exact batch mode at 3.5 dB: a batch decoded twice is checked once, on its final bytes (the parser state is put back with the
    rest), whether the pass rides in dabphy_process or runs after it; a stream this noisy also walks long resyncs across batches"""
    for auto in (True, False):
        st = {}
        checks, _, mp2 = mp2_chain.run(factory, F=3, nf=22, B=1, snr_db=3.5, seed=10, cfo=40, stats=st, auto_mp2=auto)
        assert st["replayed"] >= 1 and mp2[0, 0] > 0 and mp2[0, 2] > 10000, (st, mp2)


def test_getters_refuse_the_other_kind(emu):
    subchs, _ = mp2_chain.ensemble()
    d = factory(n_ensembles=1, max_frames=2, want_constellation=False)
    try:
        x = synth.make_stream(6, snr_db=20, seed=1, subchs=subchs)
        d.stream_upload(np.asarray(x, np.complex64)[None])
        d.set_subchannels([(s.subch_id, s.start_cu, s.size_cu, d.protection_eep(s.bitrate, s.profile_b, s.level)) for s in subchs])
        with pytest.raises(capi.DabPhyError):
            d.set_audio_kinds_ensemble(0, [1, 0])                   # not the list's length
        d.set_audio_kinds_ensemble(0, [1, 0, 0, 0, 0])
        d.process(2)
        with pytest.raises(capi.DabPhyError):
            d.superframes_ensemble(0, 0, 64)                        # an MP2 position has no superframes
        with pytest.raises(capi.DabPhyError):
            d.mp2_frames_ensemble(0, 1)                             # a DAB+ position no MP2 frames
        d.superframes_ensemble(0, 1, 64)
        # a new list resets every position to DAB+
        d.set_subchannels([(s.subch_id, s.start_cu, s.size_cu, d.protection_eep(s.bitrate, s.profile_b, s.level)) for s in subchs])
        d.process(2)
        with pytest.raises(capi.DabPhyError):
            d.mp2_frames_ensemble(0, 0)
        assert d.mp2_stats().sum() == 0
    finally:
        d.close()
