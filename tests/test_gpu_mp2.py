"""The MP2 frame check (k_mp2.hip) on the device: the unit entry on every case of tests/mp2_cases.py, the pass through dabphy_process
on small geometries (every schedule, one and several frames per batch, a replayed batch) and one batch at the headline size with MP2
services in every ensemble, against the model (tests/mp2_model.py).  The execution-model twin is tests/test_emu_mp2.py."""
import numpy as np
import pytest

import mp2_cases
import mp2_chain
import mp2_model as M
from conftest import GPU_LIB
from welle_io_amd import capi, workload

pytestmark = pytest.mark.gpu


def factory(**kw):
    return capi.DabPhy(lib_path=GPU_LIB, **kw)


def test_unit_entry_matches_the_model(gpu):
    assert mp2_chain.check_unit_entry(gpu, mp2_cases.cases()) > 1000


def test_unit_entry_on_long_streams(gpu):
    assert mp2_chain.check_unit_entry(gpu, mp2_cases.long_cases()) > 2000


def test_chain_mixed_ensembles_and_the_dabplus_totals(gpu):
    checks, sf_kinds, mp2 = mp2_chain.run(factory, F=3, nf=15, B=2)
    assert sorted(checks) == [(0, 0), (0, 2), (0, 3), (1, 0)]
    assert mp2[:, 0].min() > 0 and mp2[0, 1] > 0 and mp2[0, 2] > 0, mp2
    dab = [[i for i, k in enumerate(kk) if k == 0] for kk in ([1, 0, 1, 1, 0], [1, 0, 0, 0, 0])]
    _, sf_each, _ = mp2_chain.run(factory, F=3, nf=15, B=2, kinds=[[0] * 5, [0] * 5], sf_auto=False, sf_positions=dab)
    assert np.array_equal(sf_kinds, sf_each), (sf_kinds, sf_each)
    _, sf_none, _ = mp2_chain.run(factory, F=3, nf=15, B=2, kinds=[[0] * 5, [0] * 5])
    assert np.array_equal(sf_none[:, 0], sf_kinds[:, 0]) and (sf_none[:, 2] > sf_kinds[:, 2]).all(), (sf_none, sf_kinds)


def test_a_service_switched_to_mp2_mid_stream(gpu):
    checks, _, _ = mp2_chain.run(factory, F=3, nf=15, B=1, kinds=[[0, 0, 1, 0, 0]], switch=(2, 0, 0))
    assert sorted(checks) == [(0, 0), (0, 2)] and len(checks[(0, 0)].m.events) > 0


@pytest.mark.parametrize("pipeline_sync", [0, 1, 2, 3])
@pytest.mark.parametrize("F", [1, 3])
def test_chain_on_every_schedule(gpu, pipeline_sync, F):
    mp2_chain.run(factory, F=F, nf=15, B=2, pipeline_sync=pipeline_sync, auto_mp2=F == 1)


def test_mp2_through_a_replayed_batch(gpu):
    """exact batch mode at 3.5 dB with the coarse corrector in play: a batch decoded twice is checked once, on its final bytes (the parser
    state is put back with the rest), whether the pass rides in dabphy_process or runs after it"""
    for auto in (True, False):
        st = {}
        checks, _, mp2 = mp2_chain.run(factory, F=3, nf=22, B=1, snr_db=3.5, seed=10, cfo=40, stats=st, auto_mp2=auto)
        assert st["replayed"] >= 1, st
        assert mp2[0, 0] > 0


def test_headline_geometry_with_mp2_services(gpu):
    """256 ensembles x 32 frames, every 4th of the 18 services MP2 (workload.make_mp2_base_streams: tools/bench_mp2.py's signal), the
    pass inside dabphy_process: the totals of a sample of ensembles equal the model fed with the rows the device decoded for them"""
    import torch
    B, F = 256, 32
    rec = workload.rec_frames_for(F)
    base, subchs, mp2_pos = workload.make_mp2_base_streams(4, rec)
    iq, _, _, _ = workload.make_batch(B, device="cuda", base=(base, None), rec_frames=rec)
    dev = workload.open_receiver(capi, GPU_LIB, iq, F, subchs, profiling=False)
    sample = (0, 1, 2, 3, 129, 254, 255)
    models = {(b, i): M.Mp2Model() for b in sample for i in mp2_pos}
    try:
        kinds = [capi.AUDIO_MP2 if i in mp2_pos else capi.AUDIO_DABPLUS for i in range(len(subchs))]
        for b in range(B):
            dev.set_audio_kinds_ensemble(b, kinds)
        dev.set_auto_mp2(True)
        tot = np.zeros((B, 4), np.int64)
        for _ in range(3):
            dev.process(F)
            dev.superframes_stats()
            tot += dev.mp2_stats()
            for i in mp2_pos:
                out, fv = dev.msc(i)
                for b in sample:
                    for row in out[b, fv[b]:dev.msc_rows[b]]:
                        models[(b, i)].feed(row.tobytes())
        for b in sample:
            ms = [models[(b, i)] for i in mp2_pos]
            want = (sum(len(m.events) for m in ms), sum(sum(m.errors) for m in ms), sum(m.skipped for m in ms),
                    sum(m.feed_no + 1 - m.first_unverified for m in ms if m.first_unverified >= 0))
            assert tuple(tot[b]) == want, (b, tuple(tot[b]), want)
        assert (tot[:, 0] > 0).all()
    finally:
        dev.close()
        del iq
        torch.cuda.empty_cache()
