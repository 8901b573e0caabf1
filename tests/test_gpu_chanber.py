"""The channel BER pass (k_chanber.hip) on the device: the stateless entry against the model (tests/chanber_model.py) on every case of
tests/chanber_cases.py and on all 304 protection profiles, the pass inside dabphy_process on small geometries (every schedule, one and
three frames per batch, a replayed batch, a service change) against the model fed with the oracle run's soft bits and bytes, and one
batch at the headline size.  The execution-model twin is tests/test_emu_chanber.py."""
import numpy as np
import pytest

import chanber_cases as K
import chanber_model as M
import refapi as R
from conftest import GPU_LIB
from welle_io_amd import capi, workload

pytestmark = pytest.mark.gpu


def factory(**kw):
    return capi.DabPhy(lib_path=GPU_LIB, **kw)


def test_linear_entry_matches_the_model(gpu):
    assert K.check_directed(gpu) == 6 * (1 + 3 + 65)


def test_linear_entry_on_every_profile(gpu):
    assert K.check_profile_sweep(gpu, K.sweep_profiles(full=True)) == 304


def test_entry_errors(gpu):
    K.check_entry_errors(gpu, capi)


@pytest.mark.parametrize("pipeline_sync", [0, 1, 2, 3])
@pytest.mark.parametrize("F", [1, 3])
def test_streaming_small(gpu, F, pipeline_sync):
    K.check_streaming_small(factory, F, pipeline_sync)


def test_counts_through_a_replayed_batch(gpu):
    K.check_replayed_batch(factory)


def test_service_change_in_mid_stream(gpu):
    K.check_service_change(factory)


def test_off_means_off(gpu):
    K.check_off_means_off(factory, capi)


def test_headline_geometry(gpu):
    """256 ensembles x 32 frames, the benchmark's signal and sub-channel list, three steps: the totals of a sample of ensembles equal the
    model fed with the soft bits and bytes read back from the device for them (no oracle run of this batch exists; the oracle-fed
    checks are the small geometries above)"""
    import torch
    B, F = 256, 32
    rec = workload.rec_frames_for(F)
    iq, _, _, txs = workload.make_batch(B, device="cuda", rec_frames=rec)
    subchs = txs[0].subchs
    dev = workload.open_receiver(capi, GPU_LIB, iq, F, subchs, profiling=False)
    sample = (0, 1, 129, 255)
    po = [R.orc_prot_of(s) for s in subchs]; po_fic = R.orc_prot_fic()
    soft = {b: {} for b in sample}                  # frame number -> [75][3072], the frames a later row may still reach
    try:
        dev.set_channel_ber(True)
        n_rows = 0
        for _ in range(3):
            dev.process(F)
            info = dev.frame_info(); fib, _ = dev.fibs()
            te, tc = dev.channel_ber_totals()
            assert te.shape == (B, 1 + len(subchs))
            msc = [dev.msc(i) for i in range(len(subchs))]
            for b in sample:
                for f in range(F):
                    if info[b, f]["valid"] == 1:
                        soft[b][int(info[b, f]["frame_no"])] = dev.soft_bits(b, f)
                n0 = int(info[b, 0]["frame_no"])
                frames = [soft[b].get(k) for k in range(n0 + F)]
                want = np.zeros((1 + len(subchs), 2), np.int64)
                for f in range(F):
                    if info[b, f]["valid"] == 1:
                        want[0] += M.fic_counts(po_fic, frames[int(info[b, f]["frame_no"])], fib[b, f]).sum(0)
                for i, s in enumerate(subchs):
                    out, fv = msc[i]
                    for r in range(int(fv[b]), int(dev.msc_rows[b])):
                        sb, present = M.msc_row_soft(frames, 4 * n0 + r, s.start_cu, po[i].n_in)
                        assert present.all()
                        want[1 + i] += M.counts(po[i], sb, out[b, r], present); n_rows += 1
                got = np.stack([te[b], tc[b]], 1).astype(np.int64)
                assert np.array_equal(got, want), (b, got.tolist(), want.tolist())
                for k in [k for k in soft[b] if k < n0 + F - 4]:
                    del soft[b][k]
            assert (tc[:, 0] > 0).all()
        assert n_rows >= len(sample) * len(subchs) * (3 * 4 * F - 16 - 4 * F)
    finally:
        dev.close()
        del iq
        torch.cuda.empty_cache()
