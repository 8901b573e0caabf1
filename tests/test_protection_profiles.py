"""The whole space of protection profiles -- 240 long-form (EEP) and the 64 short-form (UEP) rows, tests/parity_cases.py:
all_protection_profiles -- on the HOST: the library's profile records against the oracle's and the reference's sub-channel sizes, and the
fused decode's window schedules.  No handle, no device, no kernel of the execution model runs here (the library is only loaded)."""
import ctypes as C
import os

import pytest

import conftest
import parity_cases as P
import refapi as R
from welle_io_amd import capi

PROFILES = P.all_protection_profiles()


@pytest.fixture(scope="module")
def host():
    """the library's host-side entry points (kernel sources built for the CPU execution model: the same dabphy_host.cpp / dabphy_fused.hip)"""
    conftest._make(["-j8", "emu"], os.path.join(conftest.PKG_DIR, "csrc"))
    return capi.load_library(conftest.EMU_LIB)


def lib_prot(lib, prof):
    p = capi.Protection()
    r = lib.dabphy_protection_uep(C.byref(p), *prof[1:]) if prof[0] == "uep" else lib.dabphy_protection_eep(C.byref(p), prof[1], int(prof[2]), prof[3])
    assert r == 0, prof
    return p


def test_the_enumerator_yields_304_distinct_profiles():
    assert len(PROFILES) == 304 and len(set(PROFILES)) == 304
    fam = [P.profile_family(p) for p in PROFILES]
    assert (fam.count("eep_a"), fam.count("eep_b"), fam.count("uep")) == (192, 48, 64)
    assert {p[1] for p in PROFILES if P.profile_family(p) == "eep_a"} == set(range(8, 385, 8))
    assert {p[1] for p in PROFILES if P.profile_family(p) == "eep_b"} == set(range(32, 385, 32))
    assert set(P.lin_sweep_profiles()) <= set(PROFILES) and set(P.FULL_GROUP_PROFILES) <= set(PROFILES)


def test_short_form_table_equals_the_oracles(host):
    size, level, bitrate = C.c_int(), C.c_int(), C.c_int()
    for i in range(64):
        assert host.dabphy_uep_table_entry(i, C.byref(size), C.byref(level), C.byref(bitrate)) == 0
        assert (bitrate.value, level.value, size.value) == R.orc_uep_table(i), i
    for i in (-1, 64):
        assert host.dabphy_uep_table_entry(i, C.byref(size), C.byref(level), C.byref(bitrate)) != 0, i


def test_profile_records(host):
    """what every profile's record says: the punctured soft bits a code word consumes equal the oracle's, the blocks add up to the code
    word (3 * bitrate / 4 blocks of 32 bits), every puncturing index in use is one of the 24 vectors.  A short-form sub-channel consumes
    its table size but for the padding of EN 300 401 table 8 (0, 4 or 8 bits) -- and but for 80 kbit/s level 1, where the reference's row
    has PI2 = 7 for the standard's 17 (uep-protection.cpp:66; parity is with the reference): 10 blocks of 4 * 10 fewer bits, 400 + 4"""
    for prof in PROFILES:
        p = lib_prot(host, prof); po = P.orc_profile(prof)
        n_in = host.dabphy_protection_input_bits(C.byref(p))
        assert n_in == po.n_in, prof
        assert p.nbits == 24 * prof[1] and sum(p.L) == 3 * prof[1] // 4 and 4 * sum(p.L) == 3 * prof[1], prof
        assert list(p.L) == list(po.L) and all(p.PI[s] == po.PI[s] for s in range(4) if p.L[s] > 0), prof
        assert all(1 <= p.PI[s] <= 24 for s in range(4) if p.L[s] > 0) and all(l >= 0 for l in p.L), prof
        if prof[0] == "uep":
            _, size = R.orc_uep_row(*prof[1:])
            assert 64 * size - n_in in ((404,) if prof[1:] == (80, 1) else (0, 4, 8)), (prof, size, n_in)


@pytest.mark.skipif(not R.have_ref_subch(), reason="oracle/_ref/libwelle_ref_subch.so not built (needs /root/reference)")
def test_sub_channel_sizes_are_the_references(host):
    """a long-form sub-channel consumes exactly its size: 64 soft bits per capacity unit of Subchannel::numCU, asked of the reference itself;
    the short-form sizes of the oracle's table are the reference's ProtLevel column"""
    for prof in PROFILES:
        n_in = host.dabphy_protection_input_bits(C.byref(lib_prot(host, prof)))
        if prof[0] == "eep":
            assert n_in == 64 * R.ref_eep_size_cu(*prof[1:]), prof
        else:
            i, size = R.orc_uep_row(*prof[1:])
            assert size == R.ref_uep_size_cu(i) and n_in <= 64 * size, prof


def test_every_profile_has_a_fused_window_schedule(host):
    """the lane-per-code-word fused decode follows every profile's depuncturing map with each of its three row counts (a class without a
    schedule would take the two-kernel path: right bytes, one more pass through memory), and the FIC's"""
    p = capi.Protection(); assert host.dabphy_protection_fic(C.byref(p)) == 0
    none = [("FIC", capi.fused_windows(host, p))] if 0 in capi.fused_windows(host, p) else []
    assert capi.fused_windows(host, p) == (144, 144, 144)                       # 2304 punctured bits in windows of 16
    for prof in PROFILES:
        p = lib_prot(host, prof)
        w = capi.fused_windows(host, p)
        if min(w) <= 0:
            none.append((P.profile_name(prof), w))
        else:
            assert w == ((host.dabphy_protection_input_bits(C.byref(p)) + 15) // 16,) * 3, prof
    assert not none, "no window schedule: %s" % none
    bad = capi.Protection(); bad.nbits = 64; bad.L[0] = 3                       # 3 blocks for a code word of 2: refused, not scheduled
    with pytest.raises(capi.DabPhyError):
        capi.fused_windows(host, bad)
