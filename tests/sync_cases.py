"""Directed inputs for the synchroniser's two decisions -- the PRS window search (PhaseReference::findIndex, three FFTPlacementMethods) and
the coarse corrector (OFDMProcessor::processPRS, three FreqsyncMethods) -- as dabphy_test_sync_find takes them: one buffer of 4096 cf32
samples per case, the search reads samples 0 .. 2047, the coarse corrector 2048 samples from the index found.

Generators only, fixed seed, everything built from the restatement's reference table: sums of circularly delayed copies of the
time-domain PRS (its inverse FFT, peak-normalised), plus complex Gaussian noise where stated.  Every list is followed by assertions ON THE
RESTATEMENT's results that the outcome classes it exists for are reached: a generator that is altered so that it no longer reaches a
branch makes this module fail on import, on the CPU.  tests/parity_cases.py (check_sync_cases_*) runs the lists through the kernels,
tests/test_oracle_vs_ref.py pins the restatement to the reference on the same lists."""
import collections

import numpy as np

import refapi as R

T_U, T_S, T_NULL, CASE, RING = 2048, 2552, 2656, 4096, 8192
FRAME_ADVANCE = T_U + 75 * T_S + T_NULL          # a frame's search at ring index p and window index s puts the next one at p + s + this
SEED = 20240611
METHODS = (0, 1, 2)                              # FFTPlacementMethod: StrongestPeak, EarliestPeakWithBinning, ThresholdBeforePeak
FREQSYNC = (0, 1, 2)                             # FreqsyncMethod: GetMiddle, CorrelatePRS, PatternOfZeros

WindowCase = collections.namedtuple("WindowCase", "name iq")                       # iq [4096]: the window, zeros behind it
CoarseCase = collections.namedtuple("CoarseCase", "name iq coarse fine ratio at")  # iq [4096]; starting correctors; FIC ratio 0 .. 10; where StrongestPeak finds the window (None: see the list)


def _prs_time():
    x = R.orc_fft2048(R.orc_prs_reftable(), inverse=True)
    return (x / np.float32(np.abs(x).max())).astype(np.complex64)


PRS = _prs_time()                                # |PRS| <= 1; a tap of amplitude 1 gives an impulse-response peak of about 16


def _rng(tag):
    return np.random.default_rng([SEED, sum(ord(c) << (8 * (i % 4)) for i, c in enumerate(tag))])


def taps(lst):
    """sum of a * PRS delayed circularly by n0, for (n0, a) in lst (a complex), in the order given"""
    v = np.zeros(T_U, np.complex64)
    for n0, a in lst:
        v = (v + np.complex64(a) * np.roll(PRS, n0)).astype(np.complex64)
    return v


def noise(rng, n, sigma):
    return (np.float32(sigma / np.sqrt(2)) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def _window(name, v):
    iq = np.zeros(CASE, np.complex64); iq[:T_U] = v
    return WindowCase(name, iq)


def _phase(rng):
    return np.exp(2j * np.pi * rng.random())


# ---------------------------------------------------------------------------------------------------------------- window cases
SINGLE_TAPS = ([0, 1, 15, 16, 17, 99, 100, 101, 198, 199, 200, 503, 504, 1259, 1260, 1279, 1280, 1299, 1300,
                1947, 1948, 1949, 2039, 2040, 2046, 2047]
               + [640 + 16 * k + s for k in range(5) for s in (-1, 1)])               # every multiple of 16 +- 1 in 640 .. 704
ECHO_D = (19, 20, 21, 99, 100, 101, 300, 499, 500, 501, 520)
ECHO_A = (0.05, 0.2, 0.45, 0.55, 0.6, 0.95, 1.05)
ECHO_MAIN = (1000, 1290)                                                               # 1290: bin 64 of the binned method, the echoes straddle bins 63 | 64
FLAT_COMBS = (256, 384, 512, 1024, 2048)
# main tap and five echoes of descending amplitude, all in the middle of a bin of 20 (their neighbouring lobes stay inside the bin, the
# side lobes in other bins are below 8 % of their tap) and within 500 of the main tap: (position, amplitude), highest first
FIVE_ECHOES = {
    "fourth_is_earliest": [(1010, 1.0), (1110, 0.9), (1210, 0.8), (610, 0.7), (1310, 0.6), (1410, 0.5)],     # -> 610
    "fifth_is_earliest": [(1010, 1.0), (1110, 0.9), (1210, 0.8), (810, 0.7), (610, 0.6), (1410, 0.5)],       # -> 810, not 610
}
# equal echoes (a single-frequency network seen from its middle): K taps of amplitude 1, `step` samples apart -- their impulse-response
# peaks come out bit-identical often enough that the binned method's choice hangs on the order std::sort leaves equal elements in
TIE_COMBS = ((5, 40), (8, 40), (12, 40), (10, 60), (6, 100), (4, 100))
TIE_TRIALS = 4
# ... two equal taps too far apart for one to be within 500 of the other (which of them std::sort puts first decides what is looked at),
# with a weaker echo behind the second; and an equal pair 499 / 500 / 501 apart among three or four more equal taps
TWIN_STARTS, TWIN_GAPS = (300, 310, 317, 333, 350, 401, 420, 455), (520, 600, 700)
PAIR_STARTS, PAIR_GAPS = (300, 333, 401, 455), (499, 500, 501)
# ... and one tap in quadrature exactly 501 away from the first of five equal taps 40 or 60 apart, in front of them or behind
FAR_STARTS = (907, 928, 949, 970, 991, 1012)
TIE_PHASES = ("random", "same", "quarter")
# ... two equal taps a few samples apart: the maximum magnitude twice inside one aligned stretch of 16 samples (one thread's share of
# StrongestPeak's scan) and inside one bin of 20
NEAR_TAPS = ((640, 2), (640, 9), (641, 5), (645, 3), (645, 10), (649, 6))
# ... and ties with bins around the 3 * mean line among the first four: a tap, an echo and a flat background (256 taps 4 apart, random
# phases) over the first 1024 samples, the whole repeated 1024 samples later -- the two copies of the tap tie, whichever half std::sort
# puts in front is looked at, and there the background lifts the mean until the side-lobe bins next to the tap straddle 3 * mean
WEAK_TRIALS = 6
WEAK_TAPS = ((650, 850), (610, 730))                   # (tap, echo)
WEAK_BACKGROUND = (0.03, 0.034, 0.04, 0.06, 0.08)
WEAK_ECHO = (0.15, 0.25, 0.4)
NOISE_LEVELS = (0.01, 0.1, 1.0)
TAP_IN_NOISE = (0.02, 0.05, 0.1, 0.3, 1.0)                                            # amplitude of the tap at 700, noise sigma 0.1
SCALINGS = (2.0 ** -60, 2.0 ** 40)
SCALED_OF = ("tap@504", "echo@1000-500x0.05", "comb512")                            # the cases the scalings are applied to


def _build_window_cases():
    cases = []
    for n0 in SINGLE_TAPS:
        cases.append(_window("tap@%d" % n0, taps([(n0, 1)])))
    rng = _rng("echo")
    for main in ECHO_MAIN:
        for d in ECHO_D:
            for sign in (-1, 1):
                for a in ECHO_A:
                    cases.append(_window("echo@%d%+dx%g" % (main, sign * d, a), taps([(main, 1), (main + sign * d, a * _phase(rng))])))
    rng = _rng("five")
    for name, lst in FIVE_ECHOES.items():
        cases.append(_window("five_" + name, taps([(n0, a * _phase(rng)) for n0, a in lst])))
    rng = _rng("comb")
    for k in FLAT_COMBS:
        cases.append(_window("comb%d" % k, taps([(i * (T_U // k) if T_U % k == 0 else (i * T_U) // k, _phase(rng)) for i in range(k)])))
    rng = _rng("ties")
    for k, step in TIE_COMBS:
        for trial in range(TIE_TRIALS):
            start = int(rng.integers(0, 400)); ph = [_phase(rng) for _ in range(k)]; q = rng.integers(0, 4, k)
            for kind in TIE_PHASES:
                a = ph if kind == "random" else [1] * k if kind == "same" else [(1, 1j, -1, -1j)[i] for i in q]
                cases.append(_window("equal%dx%d#%d,%s" % (k, step, trial, kind), taps([(start + i * step, a[i]) for i in range(k)])))
    for st in TWIN_STARTS:
        for gap in TWIN_GAPS:
            cases.append(_window("twin%d+%d" % (st, gap), taps([(st, 1), (st + gap, 1), (st + gap + 300, 0.5)])))
    for st in PAIR_STARTS:
        for gap in PAIR_GAPS:
            for extra in (3, 4):
                for q in (1, 1j):
                    cases.append(_window("pair%d+%d,%d more,%s" % (st, gap, extra, "same" if q == 1 else "quarter"),
                                         taps([(st, 1), (st + gap, q)] + [(st + 40 * j, 1) for j in range(1, extra + 1)])))
    for st in FAR_STARTS:
        for sp in (40, 60):
            for q in (1j, -1j):
                for sign in (1, -1):
                    cases.append(_window("far%d%+d,%d apart,%s" % (st, sign * 501, sp, "+j" if q == 1j else "-j"),
                                         taps([(st, 1), (st + sign * 501, q)] + [(st + sign * sp * j, 1) for j in range(1, 5)])))
    for p, k in NEAR_TAPS:
        for q in (1, 1j):
            cases.append(_window("near%d+%d,%s" % (p, k, "same" if q == 1 else "quarter"), taps([(p, 1), (p + k, q)])))
    rng = _rng("weak")
    for trial in range(WEAK_TRIALS):
        bg = taps([(4 * i, _phase(rng)) for i in range(256)])
        for p, pe in WEAK_TAPS:
            for g in WEAK_BACKGROUND:
                for e in WEAK_ECHO:
                    y = (taps([(p, 1), (pe, e * 1j)]) + np.float32(g) * bg).astype(np.complex64)
                    cases.append(_window("weak%d#%d,%g,%g" % (p, trial, g, e), (y + np.roll(y, 1024)).astype(np.complex64)))
    for n0 in (0, 700):
        v = np.zeros(T_U, np.complex64); v[n0] = 1
        cases.append(_window("impulse@%d" % n0, v))
    cases.append(_window("zeros", np.zeros(T_U, np.complex64)))
    cases.append(_window("constant", np.ones(T_U, np.complex64)))
    cases.append(_window("alternating", ((-1.0) ** np.arange(T_U)).astype(np.complex64)))
    rng = _rng("noise")
    for s in NOISE_LEVELS:
        cases.append(_window("noise%g" % s, noise(rng, T_U, s)))
    for a in TAP_IN_NOISE:
        cases.append(_window("tap@700x%g+noise" % a, (taps([(700, a)]) + noise(rng, T_U, 0.1)).astype(np.complex64)))
    by_name = {c.name: c for c in cases}
    for s in SCALINGS:
        for name in SCALED_OF:
            cases.append(WindowCase("%s*2^%d" % (name, int(np.log2(s))), (by_name[name].iq * np.float32(s)).astype(np.complex64)))
    assert len({c.name for c in cases}) == len(cases)
    return cases


WINDOW_CASES = _build_window_cases()
_W = {c.name: c for c in WINDOW_CASES}


def oracle_window(cases=None):
    """{method: [(index, impulse response)]} of the restatement over `cases` (default: WINDOW_CASES); computed once per list"""
    cases = WINDOW_CASES if cases is None else cases
    return {m: [R.orc_find_index(c.iq[:T_U], m) for c in cases] for m in METHODS}


ORACLE_WINDOW = oracle_window()


def _check_window_classes():
    names = [c.name for c in WINDOW_CASES]
    idx = {m: dict(zip(names, (r[0] for r in ORACLE_WINDOW[m]))) for m in METHODS}
    # inputs stay inside the normal float range: no response holds a NaN, an infinity or a denormal (0 itself is allowed: the zero-sum inputs)
    tiny = np.finfo(np.float32).tiny
    for m in METHODS:
        for c, (_, ir) in zip(WINDOW_CASES, ORACLE_WINDOW[m]):
            assert np.isfinite(c.iq.view(np.float32)).all() and np.isfinite(ir).all(), c.name
            assert not ((ir != 0) & (ir < tiny)).any(), c.name
    # StrongestPeak: the tap itself, wherever it is
    assert all(idx[0]["tap@%d" % n0] == n0 for n0 in SINGLE_TAPS)
    # ThresholdBeforePeak: peak in 0 .. 99 -> -1; 100 .. 199 -> 0; from 200 on -> n0 - 199; sample 2047 is never seen
    for n0 in SINGLE_TAPS:
        want = -1 if n0 < 100 else 0 if n0 < 200 else n0 - 199
        if n0 == 2047:
            want = 1846                                            # the neighbouring lobe at 2046 carries it, half a threshold lower
        assert idx[2]["tap@%d" % n0] == want, (n0, idx[2]["tap@%d" % n0])
    # EarliestPeakWithBinning: samples 2040 .. 2047 are never looked at (a tap there is found by its side lobes or not at all)
    assert idx[1]["tap@2039"] > 1900 and idx[1]["tap@2040"] > 1900 and idx[1]["tap@2046"] == 0 and idx[1]["tap@2047"] == 0
    assert all(0 <= idx[1]["tap@%d" % n0] <= n0 for n0 in SINGLE_TAPS)
    # ... the used-bin bookkeeping on both sides of bin 63 | 64 (sample 1280): with the peak in bin 64, results in bins below and from 64 on
    e1290 = [idx[1][n] for n in names if n.startswith("echo@1290")]
    assert any(0 <= i < 1280 for i in e1290) and any(i >= 1280 for i in e1290)
    assert all(1200 < idx[1]["tap@%d" % n0] < 1280 for n0 in (1280, 1299, 1300))       # peak in bin 64 / 65, the side lobe that wins in bin 62 / 63
    # ... within 500 of the peak: the echo 500 earlier wins, the one 501 earlier is not looked at
    assert idx[1]["echo@1000-500x0.05"] == 500 and idx[1]["echo@1000-501x0.05"] == idx[1]["echo@1000+300x0.05"] > 900
    assert idx[1]["echo@1290-500x0.05"] == 790 and idx[1]["echo@1290-501x0.05"] == idx[1]["echo@1290+300x0.05"] > 1190
    # ... four highest, then above 3 * mean, then earliest
    assert idx[1]["five_fourth_is_earliest"] == 610 and idx[1]["five_fifth_is_earliest"] == 810
    # ... bit-identical bin peaks where they matter: the highest peak shared by several bins, the fourth of those within 500 samples equal to
    # the fifth -- and inputs where the order std::sort leaves them in gives another index than their order by position would
    kinds = collections.Counter()
    for n, (i1, ir) in zip(names, ORACLE_WINDOW[1]):
        if not (n.startswith(("equal", "twin", "pair", "far")) or n == "comb256"):
            continue
        val = ir[:2040].reshape(102, 20).max(1); pos = ir[:2040].reshape(102, 20).argmax(1) + 20 * np.arange(102)
        order = np.argsort(-val, kind="stable")                                       # ties by position
        near = [k for k in order if abs(pos[k] - pos[order[0]]) <= 500]
        mean3 = np.float32(3) * np.float32(np.cumsum(ir[:2040], dtype=np.float32)[-1] / np.float32(T_U))
        kept = [pos[k] for k in near[:4] if not val[k] < mean3]
        top, fourth, decides = (val == val[order[0]]).sum() > 1, len(near) > 4 and val[near[3]] == val[near[4]], i1 != (min(kept) if kept else -1)
        kinds["top"] += int(top); kinds["fourth"] += int(fourth); kinds["order decides"] += int(decides)
        kinds["top alone decides"] += int(top and not fourth and decides); kinds["fourth alone decides"] += int(fourth and not top and decides)
        kinds["pair in a tie"] += int(n.startswith("pair") and (top or fourth))
        kinds["501 away in a tie"] += int(n.startswith("far") and (top or fourth) and any(abs(pos[k] - pos[order[0]]) == 501 for k in order[:8]))
    assert kinds["top"] >= 5 and kinds["fourth"] >= 5 and kinds["order decides"] >= 5, kinds
    # ... and StrongestPeak's "first maximum" on the same inputs: the maximum magnitude at two samples or more, the first one is returned
    twice = [n for n, (i0, ir) in zip(names, ORACLE_WINDOW[0]) if i0 >= 0 and (ir == ir.max()).sum() > 1]
    assert len(twice) >= 5 and all(idx[0][n] == int(np.flatnonzero(ORACLE_WINDOW[0][names.index(n)][1] == ORACLE_WINDOW[0][names.index(n)][1].max())[0]) for n in twice), twice
    same16 = [n for n in twice if n.startswith("near") and len({int(i) // 16 for i in np.flatnonzero(ORACLE_WINDOW[0][names.index(n)][1] == ORACLE_WINDOW[0][names.index(n)][1].max())}) == 1]
    assert len(same16) >= 5, same16                               # ... of which inside one thread's 16 samples
    assert kinds["top alone decides"] >= 2 and kinds["fourth alone decides"] >= 2 and kinds["pair in a tie"] >= 6 and kinds["501 away in a tie"] >= 4, kinds
    # ... the 3 * mean rule INSIDE a tie (the kernel's library-order path has its own statement of it): among the first four bins as
    # std::sort leaves them, (a) the earliest lies below 3 * mean but above 2 * mean -- without the filter, or with 2 * mean, it would be
    # the index --, (b) the earliest that is kept lies within [3, 3.2) * mean and is the index: a higher line would drop it
    weak = collections.Counter()
    for n, (i1, ir) in zip(names, ORACLE_WINDOW[1]):
        if not n.startswith("weak"):
            continue
        val = ir[:2040].reshape(102, 20).max(1); pos = (ir[:2040].reshape(102, 20).argmax(1) + 20 * np.arange(102)).astype(np.int32)
        by_pos = np.argsort(-val, kind="stable")
        near_pos = [k for k in by_pos if abs(pos[k] - pos[by_pos[0]]) <= 500]
        tie = (val == val[by_pos[0]]).sum() > 1 or (len(near_pos) > 4 and val[near_pos[3]] == val[near_pos[4]])
        order = R.orc_std_sort_desc(val, pos)
        four = [k for k in order if abs(pos[k] - pos[order[0]]) <= 500][:4]
        mean = np.float32(np.cumsum(ir[:2040], dtype=np.float32)[-1] / np.float32(T_U))
        first = min(four, key=lambda k: pos[k])
        kept = sorted((k for k in four if not val[k] < np.float32(3) * mean), key=lambda k: pos[k])
        weak["tie"] += int(tie)
        weak["below"] += int(tie and np.float32(2) * mean <= val[first] < np.float32(3) * mean and i1 != pos[first] and i1 == pos[kept[0]])
        weak["just above"] += int(tie and len(kept) > 1 and val[kept[0]] < np.float32(3.2) * mean and i1 == pos[kept[0]])
    assert weak["tie"] >= 100 and weak["below"] >= 20 and weak["just above"] >= 5, weak
    # ThresholdBeforePeak: half the maximum decides between "echo - 199" and "main - 199", for an echo in front and one behind
    assert idx[2]["echo@1000-300x0.45"] == 801 and idx[2]["echo@1000-300x0.55"] == 501
    assert idx[2]["echo@1000+300x0.95"] == 801 and idx[2]["echo@1000+300x1.05"] == 801
    # StrongestPeak: the echo wins from amplitude 1.05 on
    assert idx[0]["echo@1000+300x0.95"] == 1000 and idx[0]["echo@1000+300x1.05"] == 1300 and idx[0]["echo@1290-20x1.05"] == 1270
    # flat responses: StrongestPeak's negative return below -1, the other two -1.  Combs of 256 and 384 taps stay on the success side;
    # the unit impulse at 0 does so for the binned method alone (its mean leaves out 8 of the 2048 samples: 2.99 x the mean is a peak to it)
    flat = ["comb%d" % k for k in FLAT_COMBS if k >= 512] + ["impulse@700"]
    for n in flat:
        assert idx[0][n] < -1 and idx[1][n] == -1 and idx[2][n] == -1, (n, idx[0][n], idx[1][n], idx[2][n])
    assert idx[0]["impulse@0"] < -1 and idx[2]["impulse@0"] == -1 and idx[1]["impulse@0"] >= 0
    assert all(idx[m][n] >= 0 for m in METHODS for n in ("comb256", "comb384"))
    # zero sum: all three give -1, on zeros and on non-zero inputs whose energy lies where the reference table is zero
    for n in ("zeros", "constant", "alternating"):
        assert all(idx[m][n] == -1 for m in METHODS), n
        assert all(not ORACLE_WINDOW[m][names.index(n)][1].any() for m in METHODS), n
    # noise alone: both outcomes occur; a tap in noise is found from some amplitude on and missed below it
    nz = [idx[m]["noise%g" % s] for m in METHODS for s in NOISE_LEVELS]
    assert any(i < 0 for i in nz) and any(i >= 0 for i in nz)
    assert idx[1]["tap@700x1+noise"] == idx[1]["tap@703"] + 1 and idx[2]["tap@700x1+noise"] == 501
    assert idx[1]["tap@700x0.02+noise"] < 600 and idx[2]["tap@700x0.02+noise"] != 501
    # power-of-two scalings: same indices, responses scaled bit for bit
    for s in SCALINGS:
        for n in SCALED_OF:
            sn = "%s*2^%d" % (n, int(np.log2(s)))
            for m in METHODS:
                a, b = ORACLE_WINDOW[m][names.index(n)], ORACLE_WINDOW[m][names.index(sn)]
                assert a[0] == b[0], (sn, m)
                assert ((a[1] * np.float32(s)).view(np.uint32) == b[1].view(np.uint32)).all(), (sn, m)


_check_window_classes()

# the two-frame cases of the find chain: the second search reads where the first one's hand-over puts it, so the window index decides
# WHAT the second frame sees.  Successes at several indices, and a failure in front (the second slot then stays empty).
def _tap_then_flat():
    """a tap at 1948 in the window and, behind the window, a flat response 8 times as strong: whatever index the first search finds, the
    second one reads mostly the flat part"""
    rng = _rng("then-flat")
    iq = np.zeros(CASE, np.complex64)
    iq[:T_U] = taps([(1948, 1)])
    iq[T_U:] = np.float32(8) * taps([(2 * i, _phase(rng)) for i in range(1024)])
    return WindowCase("tap@1948,then-flat", iq)


TWO_FRAME_CASES = [_W[n] for n in ("tap@504", "tap@1260", "tap@1948", "tap@2047", "tap@200", "echo@1000-500x0.05", "echo@1290+101x0.6",
                                   "five_fifth_is_earliest", "tap@700x1+noise", "comb512", "zeros", "tap@17", "impulse@0", "noise0.1")] + [_tap_then_flat()]


def second_frame_window(case, start_index):
    """the 2048 samples the find chain's second search reads: the case at position 0 of a looping ring of RING samples, zeros behind"""
    ring = np.zeros(RING, np.complex64); ring[:CASE] = case.iq
    return np.roll(ring, -((start_index + FRAME_ADVANCE) % RING))[:T_U].copy()


def _check_two_frame_classes():
    """per placement method: a second search that succeeds, one that fails behind a success, and a first search that fails"""
    for m in METHODS:
        seen = set()
        for c in TWO_FRAME_CASES:
            i0, _ = R.orc_find_index(c.iq[:T_U], m)
            seen.add("empty" if i0 < 0 else "found" if R.orc_find_index(second_frame_window(c, i0), m)[0] >= 0 else "failed")
        assert seen == {"empty", "found", "failed"}, (m, seen)


_check_two_frame_classes()


# ---------------------------------------------------------------------------------------------------------------- coarse cases
# The search must succeed first, and the coarse corrector reads 2048 samples from the index it found: the two windows overlap.  A case
# puts what the coarse corrector is to see at samples S .. S + 2047 and, in front of it, the first S samples of a strong PRS delayed by S:
# StrongestPeak (the placement these cases run with) finds S whatever the last 100 samples of its window hold.
COARSE_AT = 1948
SEARCH_GAIN = 8.0
SHIFTS = tuple(range(-40, 41))
SNRS_DB = (10, 3, 0)
HALF_SHIFTS = (-36, -1, 0, 35)
RESET_START = (34000, 35000, -34000, -35000)
RESET_SHIFTS = (-2, -1, 0, 1, 2)
RATIO_OPEN, RATIO_CLOSED = (0, 4), (5, 10)         # the gate `ratio * 10 < 50`
COARSE_PLACEMENT = 0
OFFSETS = (1235, 1777, 1901, 1947, 2047)           # other places for the coarse window: odd ones, and the last sample the search can return
OFFSET_SHIFTS = (-7, 0, 12)


def shifted_prs(c):
    """the PRS moved up by c carriers (c may be fractional): what a receiver tuned c carriers low sees"""
    return (PRS * np.exp(2j * np.pi * c * np.arange(T_U) / T_U)).astype(np.complex64)


def _coarse(name, w, coarse=0, ratio=0, at=COARSE_AT):
    iq = np.zeros(CASE, np.complex64)
    iq[:at] = (np.float32(SEARCH_GAIN) * np.roll(PRS, at))[:at]
    iq[at:at + T_U] = w
    return CoarseCase(name, iq, coarse, -coarse, ratio, at)


def _build_coarse_cases():
    cases = []
    for c in SHIFTS:
        cases.append(_coarse("shift%+d" % c, shifted_prs(c)))
    rng = _rng("snr")
    p = float(np.mean(np.abs(PRS) ** 2))
    for snr in SNRS_DB:
        for c in SHIFTS[::5]:
            cases.append(_coarse("shift%+d@%ddB" % (c, snr), (shifted_prs(c) + noise(rng, T_U, np.sqrt(p / 10 ** (snr / 10)))).astype(np.complex64)))
    for c in HALF_SHIFTS:
        cases.append(_coarse("shift%+d.5" % c, shifted_prs(c + 0.5)))
    cases.append(_coarse("nothing", np.zeros(T_U, np.complex64)))
    rng = _rng("coarse-noise")
    cases.append(_coarse("noise-only", noise(rng, T_U, 0.1)))
    for r in RATIO_OPEN[1:] + RATIO_CLOSED:
        cases.append(_coarse("shift+3,ratio%d" % r, shifted_prs(3), ratio=r))
    for start in RESET_START:
        for c in RESET_SHIFTS:
            cases.append(_coarse("shift%+d,from%+d" % (c, start), shifted_prs(c), coarse=start))
    for start, c in ((34500, 0), (34500, 1), (-34500, 0), (-34500, -1), (35999, 0), (-35999, 0)):      # (no multiples of 1000: the bound is 35 000 itself, not the next step)
        cases.append(_coarse("shift%+d,from%+d" % (c, start), shifted_prs(c), coarse=start))
    cases.append(_coarse("nothing,from+34000", np.zeros(T_U, np.complex64), coarse=34000))
    for at in OFFSETS:
        for c in OFFSET_SHIFTS:
            cases.append(_coarse("shift%+d,at%d" % (c, at), shifted_prs(c), at=at))
    assert len({c.name for c in cases}) == len(cases)
    return cases


COARSE_CASES = _build_coarse_cases()


def coarse_rule(coarse, correction):
    """ofdm-processor.cpp:403-408, stated once: what a correction of `correction` carriers does to coarseCorrector"""
    if correction != 100:
        coarse += correction * 1000
        if abs(coarse) > 35000:
            coarse = 0
    return coarse


def oracle_coarse(cases=None, placement=COARSE_PLACEMENT):
    """{freqsync method: [(start_index, correction or None when the gate is closed, coarse_after)]} of the restatement"""
    cases = COARSE_CASES if cases is None else cases
    out = {}
    for fm in FREQSYNC:
        rows = []
        for c in cases:
            s, _ = R.orc_find_index(c.iq[:T_U], placement)
            assert s >= 0, c.name
            if c.ratio * 10 < 50:
                corr = R.orc_coarse_prs_method(c.iq[s:s + T_U], fm)
                rows.append((s, corr, coarse_rule(c.coarse, corr)))
            else:
                rows.append((s, None, c.coarse))
        out[fm] = rows
    return out


ORACLE_COARSE = oracle_coarse()


def _check_coarse_classes():
    names = [c.name for c in COARSE_CASES]
    row = {fm: dict(zip(names, ORACLE_COARSE[fm])) for fm in FREQSYNC}
    for fm in FREQSYNC:
        assert all(r[0] == c.at for c, r in zip(COARSE_CASES, ORACLE_COARSE[fm]))               # the search finds the place every time
        assert all(row[fm]["shift%+d,at%d" % (c, at)][1] == row[fm]["shift%+d" % c][1] for at in OFFSETS for c in OFFSET_SHIFTS)     # ... and the corrector sees the same there
    # clean signal: PatternOfZeros and CorrelatePRS give the shift inside their range of 72 carriers and wrap outside it, GetMiddle is one off at most
    for c in SHIFTS:
        n = "shift%+d" % c
        if -36 <= c <= 35:
            assert row[2][n][1] == c and row[1][n][1] == c, (n, row[2][n], row[1][n])
        else:
            assert row[2][n][1] != c and -36 <= row[2][n][1] <= 35, (n, row[2][n])
        assert abs(row[0][n][1] - c) <= 1, (n, row[0][n])
    # nothing to go by: PatternOfZeros' first index, CorrelatePRS' `index = 100` (64 carriers), GetMiddle's start value; the last two
    # drive the reset from coarse = 0
    assert (row[2]["nothing"][1], row[1]["nothing"][1], row[0]["nothing"][1]) == (-36, 64, -256)
    assert row[1]["nothing"][2] == 0 and row[0]["nothing"][2] == 0 and row[2]["nothing,from+34000"][2] == -2000
    # GetMiddle's reset-the-running-sum quirk: on noise it reports the LAST index with a positive step, far outside +-36
    assert row[0]["noise-only"][1] > 100 and row[0]["noise-only"][2] == 0
    # the gate: closed at 5 and 10, open at 0 and 4
    for r in RATIO_CLOSED:
        assert all(row[fm]["shift+3,ratio%d" % r][1] is None for fm in FREQSYNC)
    assert all(row[fm]["shift+3,ratio4"][1] is not None and row[fm]["shift+3,ratio4"][2] != 0 for fm in FREQSYNC)
    # the reset: both sides of |coarse| > 35 000, from both signs, and the value 35 000 itself survives
    for fm in (1, 2):
        after = {(s, c): row[fm]["shift%+d,from%+d" % (c, s)][2] for s in RESET_START for c in RESET_SHIFTS}
        assert after[(34000, 1)] == 35000 and after[(34000, 2)] == 0 and after[(35000, 0)] == 35000 and after[(35000, 1)] == 0 and after[(35000, -1)] == 34000
        assert after[(-34000, -1)] == -35000 and after[(-34000, -2)] == 0 and after[(-35000, 0)] == -35000 and after[(-35000, -1)] == 0 and after[(-35000, 1)] == -34000
    after0 = [row[0]["shift%+d,from%+d" % (c, s)][2] for s in RESET_START for c in RESET_SHIFTS]
    assert any(a == 0 for a in after0) and any(a != 0 for a in after0)
    # noisy signals: right and wrong answers both occur somewhere, so the comparison with the kernels is not one of constants
    for fm in FREQSYNC:
        got = [(row[fm]["shift%+d@%ddB" % (c, snr)][1], c) for snr in SNRS_DB for c in SHIFTS[::5]]
        assert len({g for g, _ in got}) > 5, fm


_check_coarse_classes()

# The signal as the receiver meets it: null-like noise, the 504-sample guard interval, the PRS, the next symbol's start -- searched by each
# of the three placement methods, which take the coarse window at three different, mostly odd places of it (StrongestPeak at the PRS,
# ThresholdBeforePeak 199 samples into the guard, the binned method on a side lobe about 22 samples early).
RECEIVER_LEAD = (0, 37)
RECEIVER_SHIFTS = (-3, 0, 1, 5)


def _build_receiver_cases():
    rng = _rng("receiver")
    cases = []
    for lead in RECEIVER_LEAD:
        for c in RECEIVER_SHIFTS:
            w = shifted_prs(c)
            iq = noise(rng, CASE, 0.003)
            iq[lead:lead + 504] += w[-504:]; iq[lead + 504:lead + 504 + T_U] += w
            iq[lead + 504 + T_U:] += (np.float32(0.7) * noise(rng, CASE, 1.0))[:CASE - lead - 504 - T_U] * np.float32(np.sqrt(np.mean(np.abs(PRS) ** 2)))
            cases.append(CoarseCase("receiver,lead%d,shift%+d" % (lead, c), iq.astype(np.complex64), 0, 0, 0, None))
    return cases


RECEIVER_CASES = _build_receiver_cases()
ORACLE_RECEIVER = {m: oracle_coarse(RECEIVER_CASES, m) for m in METHODS}


def _check_receiver_classes():
    """every search succeeds (oracle_coarse asserts it); on the unshifted signal each method lands where DESIGN.md says it does, a shifted one
    sends the search elsewhere -- the coarse window is then taken at many places, odd ones among them"""
    starts = {m: [r[0] for r in ORACLE_RECEIVER[m][2]] for m in METHODS}
    zero = RECEIVER_SHIFTS.index(0)
    for j, lead in enumerate(RECEIVER_LEAD):
        k = j * len(RECEIVER_SHIFTS) + zero
        assert starts[0][k] == 504 + lead and starts[2][k] == 305 + lead and 0 <= starts[1][k] < 504 + lead, (lead, starts)
        assert all(ORACLE_RECEIVER[m][fm][k][1] == 0 for m in (0, 2) for fm in (1, 2)), lead      # nothing to correct, guard samples in the window or not
    every = [s for m in METHODS for s in starts[m]]
    assert len({s % 4 for s in every}) >= 3 and len(set(every)) >= 10, every


_check_receiver_classes()
