"""One SHA-256 per case of what the wideband front end writes into the ring rows, to compare two builds of the library on ONE platform
(the execution model with itself, the device with itself; the project holds each to the float64 model, not to each other): every shape
of tests/frontend_cases.py with u8 captures, each kind's default shape with the other four formats, and its four ways of cutting one
capture into writes.
Usage: python tools/frontend_digest.py <library>"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: F401,E402
import frontend_cases as F  # noqa: E402
from welle_io_amd import capi  # noqa: E402


def digest(lib, rate, n_taps, fmt, way=None):
    raw, taps, offsets = F.filter_case(rate, n_taps, fmt)
    sizes = rate.chunkings(len(raw))[way] if way else []
    cuts = list(np.cumsum([0] + list(sizes))) + [len(raw)]
    d = capi.DabPhy(lib_path=lib, n_ensembles=3, max_frames=1, want_constellation=False)
    try:
        rate.open(d, F.RING_MIN, taps, offsets, fmt)
        hold = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            if a == b:
                continue
            if way == "async":
                hold.append(np.ascontiguousarray(raw[a:b]).copy())
                d.stream_write_wideband_async(hold[-1]); d.stream_commit()
            else:
                d.stream_write_wideband(raw[a:b])
        sha = hashlib.sha256()
        for row in F.read_all(d, rate.n_outputs(len(raw))):
            sha.update(np.ascontiguousarray(row).tobytes())
    finally:
        d.close()
    print("%-10s %6d taps %-6s %-24s %s" % (rate.name, n_taps, fmt, way or "one piece", sha.hexdigest()))


def main():
    lib = os.path.abspath(sys.argv[1])
    cases = [(F.Integer(D), n) for D, n in F.INTEGER_SHAPES] + [(F.Rational(L, M), n) for L, M, n in F.RATIONAL_SHAPES]
    for rate, n_taps in cases:
        digest(lib, rate, n_taps, "u8")
    for K in (F.INTEGER, F.RATIONAL):
        for fmt in F.FORMATS:
            if fmt != "u8":
                digest(lib, K["rate"], K["n_taps"], fmt)
        for way in K["rate"].chunkings(0):
            digest(lib, K["rate"], K["n_taps"], "u8", way)


if __name__ == "__main__":
    main()
