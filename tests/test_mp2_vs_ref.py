"""Pins the MP2 frame-check model (tests/mp2_model.py, the contract k_mp2.hip is tested against) to the reference's own MP2Decoder:
tests/native/mp2_ref_check.cpp feeds the same logical frames to it, one Feed each, and records what its observer sees.  Every frame
before the model's first_unverified must be the reference's; first_unverified lies at or before the first difference.
Skipped where the reference build is absent (oracle/_ref, built with the reference's sources: see tests/test_oracle_vs_ref.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import mp2_cases
import mp2_model as M
import refapi as R
from conftest import ROOT

REF_SO = os.path.join(ROOT, "oracle", "_ref", "libwelle_ref.so")


def _ref_src():
    """the reference's source tree, as oracle/Makefile names it (REF ?= ...)"""
    m = re.search(r"^REF \?= *(\S+)", open(os.path.join(ROOT, "oracle", "Makefile")).read(), re.M)
    return os.environ.get("REF", m.group(1) if m else "")


def _have():
    src = _ref_src()
    return R.have_ref() and os.path.exists(REF_SO) and os.path.exists(os.path.join(src, "src", "backend", "dab_decoder.h"))


pytestmark = pytest.mark.skipif(not _have(), reason="oracle/_ref or the reference's headers not present")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    s = os.path.join(_ref_src(), "src")
    exe = str(tmp_path_factory.mktemp("mp2") / "mp2_ref_check")
    subprocess.run(["g++", "-std=c++14", "-O1", "-w", "-DHAVE_CONFIG_H", "-I" + s, "-I" + os.path.join(s, "backend"), "-I" + os.path.join(s, "various"),
                    "-I" + os.path.join(s, "libs", "mpg123"), os.path.join(ROOT, "tests", "native", "mp2_ref_check.cpp"), "-o", exe, REF_SO,
                    "-Wl,-rpath," + os.path.dirname(REF_SO), "-lpthread"], check=True)
    return exe


def ref_run(exe, stream, fl, tmp):
    path = os.path.join(tmp, "frames.bin")
    with open(path, "wb") as f:
        f.write(stream)
    out = subprocess.run([exe, path, str(fl)], capture_output=True, text=True, check=True).stdout.split("\n")
    ev, err, threw = [], {}, -1
    for line in out:
        t = line.split()
        if not t:
            continue
        if t[0] == "E":
            ev.append(tuple(int(v) for v in t[1:]))
        elif t[0] == "F":
            err[int(t[1])] = int(t[2])
        elif t[0] == "T":
            threw = int(t[1])
    return ev, err, threw


def model_as_ref(stream, events):
    """the model's events in the harness' terms: feed, new_format, crc_ok, F-PAD, X-PAD length, first 4 body bytes"""
    out = []
    for (feed, off, h, ok, nf, scf, f0, f1) in events:
        fs = M.header_info(h)[4]
        body = stream[off + 4:off + 8]
        out.append((feed, nf, ok, f0, f1, fs - 2 - scf) + tuple(body))
    return out


CASES = mp2_cases.cases() + mp2_cases.long_cases()


@pytest.mark.parametrize("name,stream,fl", CASES, ids=[c[0] for c in CASES])
def test_model_equals_reference(harness, tmp_path, name, stream, fl):
    ev, errs, fu, _ = M.run(stream, fl)
    rev, rerr, threw = ref_run(harness, stream, fl, str(tmp_path))
    lim = fu if fu >= 0 else len(errs)
    assert threw < 0 or threw >= lim, "the reference threw at logical frame %d, the model claims it" % threw
    assert model_as_ref(stream, ev) == [e for e in rev if e[0] < lim]
    assert errs[:lim] == [rerr[k] for k in range(lim)]
    if name.endswith("_beyond"):
        assert fu == 1
    elif "_k" not in name:                # the clean streams: every frame checked, every CRC good, the first one returned once the next header is in
        lsf = name.startswith("lsf") or "_24000_" in name
        assert fu == -1 and sum(errs) == 0 and len(ev) == len(errs) // (2 if lsf else 1)
        assert ev[0][0] == (2 if lsf else 1) and ev[0][4] == 1 and all(not e[4] for e in ev[1:])


def test_damage_is_seen():
    """the damaged streams exercise what they are meant to: CRC failures, resyncs (bytes skipped), unverified paths"""
    seen = {}
    for name, stream, fl in CASES:
        if "_k" not in name:
            continue
        kind = name.split("_", 2)[2].rsplit("_k", 1)[0]
        ev, errs, fu, skipped = M.run(stream, fl)
        s = seen.setdefault(kind, [0, 0, 0])
        s[0] += sum(errs); s[1] += skipped; s[2] += fu >= 0
    assert seen["crc_flip"][0] > 0 and seen["header_crc_flip"][0] > 0 and seen["uncovered_flip"][0] == 0
    assert seen["sync"][1] > 0 and seen["false_sync"][1] + seen["drop"][1] > 0 and seen["junk_start"][1] > 0
    assert seen["TAG"][2] > 0 and seen["ID3"][2] > 0 and seen["samplerate"][2] > 0
