"""The automatic choice of the Viterbi kernel (dabphy_config.decode_shape = 0; dabphy_fused.hip: choose_shape, sp_two_for) on the device,
at the smallest batches on either side of both thresholds: one wavefront per code word up to 1 024 code words per call, two code words
per wavefront up to 40 960, the lane-per-code-word kernel beyond.  One four-frame stream tiled over the ensembles; bytes against the
oracle where checked.  The execution-model twin is test_default_choice_of_the_viterbi_kernel (tests/test_emu_product_build.py)."""
import numpy as np
import pytest

import parity_cases as P
import refapi as R
from conftest import GPU_LIB
from welle_io_amd import capi, synth

pytestmark = pytest.mark.gpu


def factory(**kw):
    return capi.DabPhy(lib_path=GPU_LIB, want_constellation=False, **kw)


@pytest.fixture(scope="module")
def stream():
    return synth.make_stream(4, snr_db=15, cfo_hz=30, delay=77, return_tx=True, seed=9)


def subs_of(d, subchs):
    return [(s.subch_id, s.start_cu, s.size_cu, P.dev_prot(d, s)) for s in subchs]


def test_one_frame_of_one_ensemble_is_state_parallel(gpu, stream):
    """76 code words per call, the live receiver's shape: k_viterbi_sp, the one MSC class in the launch; so is a seam call of three"""
    x, tx = stream
    subs = [tx.subchs[3], tx.subchs[10]]
    o = R.orc_receiver_run(x, subchs=subs)
    d = factory(n_ensembles=1, max_frames=1)
    try:
        assert d.last_decode_plan() == (0, 0)
        d.stream_upload(x)
        d.set_subchannels(subs_of(d, subs))
        fibs = []
        for _ in range(3):
            d.process(1)
            assert d.last_decode_plan() == (3, 1), d.last_decode_plan()
            if d.frame_info()[0, 0]["valid"] == 1:
                fibs.append(d.fibs()[0][0, 0])
        assert len(fibs) >= 2 and np.array_equal(np.array(fibs), o["fib"][:12 * len(fibs)].reshape(len(fibs), 12, 33)[:, :, 1:])
        P.check_viterbi(d, 768, 3, seed=5, kind="uniform")
    finally:
        d.close()


def test_above_1024_code_words_two_share_a_wavefront(gpu, stream):
    """4 x 4 frames x (4 FIC + 72 MSC) = 1 216 code words: k_viterbi_sp2 + k_traceback_sp2; the lane-per-code-word kernel
    (decode_shape 1) decodes the same bytes"""
    x, tx = stream
    got = []
    for shape in (0, 1):
        d = factory(n_ensembles=4, max_frames=4, decode_shape=shape)
        try:
            d.stream_upload(np.tile(x, (4, 1)))
            d.set_subchannels(subs_of(d, tx.subchs))
            d.process(4)
            assert d.last_decode_plan() == ((2, 1) if shape == 0 else (1, 1)), d.last_decode_plan()
            got.append([d.fibs()[0].copy()] + [d.msc(i)[0][:, :8].copy() for i in range(18)])      # the rows the batch decoded
            assert (d.msc_rows == 8).all()
        finally:
            d.close()
    assert all(np.array_equal(a, b) for a, b in zip(*got)) and got[0][0].any() and got[0][18].any()


def test_beyond_40960_code_words_a_lane_per_code_word(gpu, stream):
    """135 x 4 frames x (4 FIC + 72 MSC) = 41 040 code words with 18 sub-channels"""
    x, tx = stream
    d = factory(n_ensembles=135, max_frames=4)
    try:
        d.stream_upload(np.tile(x, (135, 1)))
        d.set_subchannels(subs_of(d, tx.subchs))
        d.process(4)
        assert d.last_decode_plan() == (1, 1), d.last_decode_plan()
    finally:
        d.close()
