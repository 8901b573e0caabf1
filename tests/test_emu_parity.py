"""CPU suite: the kernel SOURCES, compiled unchanged for the tests/hipemu execution model, against the oracle.
Checks indexing / barrier / packing logic without a GPU; the GPU suite repeats these on the device."""
import numpy as np
import pytest

import parity_cases as P


@pytest.mark.parametrize("nbits,kind", [(768, "uniform"), (1536, "coded"), (192, "extreme"), (768, "zeros"), (2304, "coded")])
def test_viterbi(emu, nbits, kind):
    P.check_viterbi(emu, nbits, 70 if nbits < 2000 else 5, seed=nbits, kind=kind)


@pytest.mark.parametrize("args", [("eep", 64, 0, 3), ("eep", 8, 0, 2), ("eep", 32, 1, 1), ("eep", 128, 0, 4), ("uep", 80, 1, 0), ("uep", 32, 5, 0)])
def test_msc_deconvolve(emu, args):
    P.check_msc_deconvolve(emu, *args, n=3, seed=7)


def test_msc_deconvolve_every_profile(emu):
    """all 304 protection profiles through Protection::deconvolve's seam, one code word of random int8 each"""
    P.check_msc_profiles(emu, P.all_protection_profiles(), n=1, seed=7)


def test_msc_deconvolve_profiles_lane_per_code_word(emu):
    """... and with the lane-per-code-word kernels forced (decode_shape = 1: k_lin_gather + k_viterbi): every short-form row, the long
    forms at the shortest code words and on either side of 32 767 punctured soft bits"""
    from welle_io_amd import capi
    import conftest
    d = capi.DabPhy(lib_path=conftest.EMU_LIB, decode_shape=1)
    try:
        P.check_msc_profiles(d, P.lin_sweep_profiles(), n=1, seed=7)
    finally:
        d.close()


@pytest.mark.parametrize("shape", [2, 3])
def test_msc_deconvolve_longest_profiles_state_parallel(emu, shape):
    """the state-parallel kernels unpack four map entries from two dwords: the profiles with the longest punctured code words (EEP 1-A on
    either side of 32 767 soft bits and at 384 kbit/s, UEP 384 kbit/s level 1), an odd number of code words"""
    from welle_io_amd import capi
    import conftest
    d = capi.DabPhy(lib_path=conftest.EMU_LIB, decode_shape=shape)
    try:
        P.check_msc_profiles(d, P.FULL_GROUP_PROFILES, n=3, seed=7)
    finally:
        d.close()


def test_fic(emu):
    assert P.check_fic(emu, 3, snr_db=9, seed=4) > 0


def test_fic_arbitrary_int8(emu):
    P.check_fic_arbitrary_int8(emu)


def test_demod(emu):
    P.check_demod(emu, 2, snr_db=14, seed=2)


def test_demod_degenerate_magnitudes(emu):
    P.check_demod_degenerate(emu)


def test_demod_zero_carriers(emu):
    """r1 == 0 (the reference's inf*0 -> NaN -> int8 case, SURVEY C-3): all-zero symbols give soft bit 0"""
    frames = np.zeros((1, 2048 + 75 * 2552), np.complex64)
    soft, con, _ = emu.demod_frames(frames)
    assert not soft.any()


def test_seams_state_parallel(emu):
    """the seams of INTEGRATION.md level 2 (Viterbi::deconvolve, Protection::deconvolve, FicHandler::processFicBlock) decode small calls
    with one wavefront per code word (k_viterbi_sp, kinds 1 and 2; dabphy_config.decode_shape = 2 here, the default's choice on the device):
    arbitrary int8 input incl. -128 (the clamp of viterbi.cpp:233-236), every EEP / UEP profile kind, the FIC"""
    from welle_io_amd import capi
    import conftest
    d = capi.DabPhy(lib_path=conftest.EMU_LIB, decode_shape=3)              # round 4's kernel (one code word per wavefront) stays selectable
    try:
        P.check_viterbi(d, 192, 7, seed=6, kind="extreme")
        P.check_msc_deconvolve(d, "uep", 80, 1, 0, 3, seed=11)
        P.check_fic_arbitrary_int8(d, n_frames=1)
    finally:
        d.close()
    d = capi.DabPhy(lib_path=conftest.EMU_LIB, decode_shape=2)              # k_viterbi_sp2: two code words per wavefront, odd counts included
    try:
        P.check_viterbi(d, 768, 9, seed=5, kind="uniform")
        P.check_viterbi(d, 192, 70, seed=6, kind="extreme")
        P.check_viterbi(d, 2304, 3, seed=7, kind="coded")
        P.check_viterbi(d, 32, 5, seed=8, kind="uniform")                 # 38 trellis steps: not a multiple of six -> the lane-per-code-word kernel
        P.check_msc_deconvolve(d, "eep", 64, 0, 3, 5, seed=9)
        P.check_msc_deconvolve(d, "eep", 32, 1, 1, 4, seed=10)
        P.check_msc_deconvolve(d, "uep", 80, 1, 0, 3, seed=11)
        assert P.check_fic(d, 3, 14, seed=12) > 0
        P.check_fic_arbitrary_int8(d)                                     # -128 through kind 1 (round 4 clamped only kind 2: ADVICE)
    finally:
        d.close()


def test_error_behaviour(emu):
    from welle_io_amd import capi
    import conftest
    P.check_error_behaviour(lambda **kw: capi.DabPhy(lib_path=conftest.EMU_LIB, **kw))


def test_timing_driver_refuses_a_stale_launch(emu):
    from welle_io_amd import capi
    import conftest
    P.check_timing_driver_refuses_a_stale_launch(lambda **kw: capi.DabPhy(lib_path=conftest.EMU_LIB, **kw))


def test_demod_chunk_sizes(emu):
    from welle_io_amd import capi
    import conftest
    P.check_demod_chunks(lambda **kw: capi.DabPhy(lib_path=conftest.EMU_LIB, **kw))


def test_reed_solomon_random_error_patterns(emu):
    P.check_rs_random(emu, n_sf=120)


@pytest.mark.parametrize("s", sorted(P.RS_GEOMETRIES))
def test_reed_solomon_random_error_patterns_odd_geometries(emu, s):
    """one code word per superframe to 48: thread -> (superframe, column) with s that divides no work-group"""
    P.check_rs_random(emu, n_sf=P.RS_GEOMETRIES[s], seed=77 + s, s_per_sf=s)


@pytest.mark.parametrize("s", [1, 9, 48])
def test_reed_solomon_directed_words(emu, s):
    P.check_rs_directed(emu, s)
