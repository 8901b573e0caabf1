"""Pins the access-unit model (tests/au_model.py, the contract k_au.hip is tested against) to the reference's own SuperframeFilter:
tests/native/latm_ref_check.cpp feeds the same logical frames to SuperframeFilter(observer, false, false) with an
UntouchedStreamConsumer attached and prints every LATM/LOAS frame it forwards and its duration.  The model's LOAS stream on the oracle's
events must equal it byte for byte.  Skipped where the reference build is absent (oracle/_ref, built with the reference's sources: see
tests/test_oracle_vs_ref.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import au_cases as A
import au_model as M
import refapi as R
import sf_cases as S
from conftest import ROOT

REF_SO = os.path.join(ROOT, "oracle", "_ref", "libwelle_ref.so")


def _ref_src():
    """the reference's source tree, as oracle/Makefile names it (REF ?= ...)"""
    m = re.search(r"^REF \?= *(\S+)", open(os.path.join(ROOT, "oracle", "Makefile")).read(), re.M)
    return os.environ.get("REF", m.group(1) if m else "")


def _have():
    return R.have_ref() and os.path.exists(REF_SO) and os.path.exists(os.path.join(_ref_src(), "src", "backend", "dabplus_decoder.h"))


pytestmark = pytest.mark.skipif(not _have(), reason="oracle/_ref or the reference's headers not present")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    s = os.path.join(_ref_src(), "src")
    exe = str(tmp_path_factory.mktemp("latm") / "latm_ref_check")
    subprocess.run(["g++", "-std=c++14", "-O1", "-w", "-DHAVE_CONFIG_H", "-DDABLIN_AAC_FAAD2", "-I" + s, "-I" + os.path.join(s, "backend"), "-I" + os.path.join(s, "various"),
                    "-I" + os.path.join(s, "libs", "fec"), "-I" + os.path.join(s, "libs", "faad2", "include"), os.path.join(ROOT, "tests", "native", "latm_ref_check.cpp"), "-o", exe, REF_SO,
                    "-Wl,-rpath," + os.path.dirname(REF_SO), "-lpthread"], check=True)
    return exe


def check(exe, tmp, superframes, bitrate):
    """the reference's forwarded frames over `superframes` fed as logical frames = the model's, frame by frame, with their durations;
    returns the model's access units"""
    fb = 3 * bitrate
    frames = np.concatenate([np.asarray(sf, np.uint8).reshape(5, fb) for sf in superframes])
    path = os.path.join(tmp, "frames.bin")
    frames.tofile(path)
    out = subprocess.run([exe, path, str(fb)], capture_output=True, text=True, check=True).stdout.split("\n")
    ref = [(int(t[1]), int(t[2]), bytes.fromhex(t[4]) if len(t) > 4 else b"") for t in (ln.split() for ln in out) if t and t[0] == "U"]
    assert all(len(r[2]) == int(t[3]) for r, t in zip(ref, (ln.split() for ln in out if ln.startswith("U"))))
    eo, so = R.orc_superframe_run(frames)
    aus, raw, loas, failed = M.model(eo, so)
    assert [(a[1], M.au_duration_ms(a[3]), M.loas_frame(a[4], a[3])) for a in aus] == ref
    assert b"".join(r[2] for r in ref) == loas
    return eo, aus


@pytest.mark.parametrize("bitrate", [8, 24, 40, 72, 136, 384])
def test_layouts_and_channel_modes(harness, tmp_path, bitrate):
    """the four layouts at this bit rate, flags that toggle aac_channel_mode (and ps / surround, which the stream ignores)"""
    rng = np.random.RandomState(bitrate)
    sfs = [S.make_superframe(bitrate, rng, lay, flags) for lay in S.LAYOUTS for flags in (0x00, 0x10, 0x0B, 0x1F)]
    eo, aus = check(harness, str(tmp_path), sfs, bitrate)
    assert sum(e[3] for e in eo) == len(sfs) and {a[3] & 0x70 for a in aus} == {lay[0] << 6 | lay[1] << 5 | ch for lay in S.LAYOUTS for ch in (0, 0x10)}


@pytest.mark.parametrize("layout,bitrate,au_lengths", A.UNIT_SUPERFRAMES, ids=["%d%d@%d" % (c[0] + (c[1],)) for c in A.UNIT_SUPERFRAMES])
def test_explicit_lengths(harness, tmp_path, layout, bitrate, au_lengths):
    """the superframes of the device's unit sweep.  One difference: an access unit of ONE byte is fed to the reference as one of two (a
    CRC over nothing).  On a one-byte unit the reference computes au_len - 2 in size_t (dabplus_decoder.cpp:126-127), reads the byte in
    front of the unit and runs its CRC over 2^64 - 1 bytes until it leaves its heap: the harness dies with SIGSEGV, there is nothing to
    compare with.  The oracle's filter counts such a unit as failed, the model skips it, and the device's sweep keeps it
    (tests/au_cases.py: UNIT_SUPERFRAMES)."""
    rng = np.random.RandomState(7)
    if au_lengths:
        au_lengths = tuple(2 if v == 1 else v for v in au_lengths)
    eo, aus = check(harness, str(tmp_path), [S.make_superframe(bitrate, rng, layout, fl, au_lengths) for fl in (0x00, 0x10)], bitrate)
    if au_lengths:
        want = {v - 2 for v in au_lengths if v is not None and v >= 2}
        assert want <= {len(a[4]) for a in aus}, (want, sorted(len(a[4]) for a in aus))


def test_rejects(harness, tmp_path):
    """every way CheckSync rejects a superframe, between superframes that synchronise: nothing of a rejected one is forwarded"""
    rng = np.random.RandomState(11)
    sfs = []
    for rej in ("zero_table", "fire", "order:1", "order:2", "past_end", "all_zero"):
        sfs += [S.make_superframe(40, rng, (1, 1), 0x10), S.make_superframe(40, rng, (1, 1), 0x00, None, rej)]
    sfs.append(S.make_superframe(40, rng, (0, 0), 0x10))
    eo, aus = check(harness, str(tmp_path), sfs, 40)
    assert sum(e[3] for e in eo) >= 7 and len(aus) >= 7 * 3
