"""Directed streams for the acquisition head of the synchroniser -- OFDMProcessor::run from notSynced to SyncOnPhase (ofdm-processor.cpp:249-319)
as acquire_body, slevel_replay and k_slevel_catchup of k_sync.hip restate it -- and the checks that run them through the public streaming
calls, case by case, against the restatement's attempt trace (orc_receiver_run_traced).

One seeded, deterministic case set.  A case is a cf32 stream for ONE ensemble; cases of equal length share a handle, case k is ensemble k.
Most streams are an envelope times a carrier: the exact carrier (u = 1: |re| + |im| IS the envelope) or the random-phase carrier
(u = exp(j 2 pi rand): |re| + |im| jitters between 1 and sqrt 2 times the envelope).  P0 = T_F / 2 + 50 is where the first search
starts; a "null" scales the envelope by g over [s, s + w).  Every position that has to hit a limit or a tile edge is DERIVED by running
the restatement, not written down.

validate() asserts, from the restatement's traces alone (no device, nothing the code under test could satisfy), that every family reaches
the branches it exists for.  check_family() runs a family on a device or on the execution model; tests/test_oracle_vs_ref.py pins the
restatement's trace to the reference itself on the same streams."""
import collections
import functools

import numpy as np

import refapi as R
from welle_io_amd import synth

T_U, T_S, T_NULL, T_F = 2048, 2552, 2656, 196608
SYNC_NEED = T_U + (T_U - 1) + 75 * T_S + T_NULL          # k_sync.hip: samples a window search needs in the ring (198 151)
P0 = T_F // 2 + 50                                       # first sample of the first threshold loop
TILE = 1024                                              # ACQ_TILE of k_sync.hip: samples staged per pass of the search
N_SHORT = T_F // 2 + 10000 + SYNC_NEED                   # room for a null within ~7000 samples of P0 and a comparable attempt behind it
N_LONG = P0 + T_F + 4000 + SYNC_NEED                     # ... the same behind a first loop that runs to its limit of T_F samples
PIECE = 30011                                            # live ring: samples per stream_write
MAX_BATCH = 24
SEED = 20250114
NULL_AT = P0 + 3000
FAMILIES = ("degenerate", "widths", "rise_limit", "fall_limit", "thresholds", "tile_edges", "reacquire")

Case = collections.namedtuple("Case", "name family iq")
Attempt = collections.namedtuple("Attempt", "pos start_index coarse fine n_sync_false completed fine_after coarse_after")
Oracle = collections.namedtuple("Oracle", "trace attempts cir n_sync_false n_sync_true n")


def _rng(tag):
    return np.random.default_rng([SEED, sum(ord(c) << (8 * (i % 4)) for i, c in enumerate(tag))])


@functools.lru_cache(maxsize=None)
def carrier(n):
    """the random-phase carrier, one per length: sweeps over a gain or a position change nothing else"""
    return np.exp(2j * np.pi * _rng("carrier%d" % n).random(n))


def stream(env, random_carrier, u=None):
    with np.errstate(over="ignore", invalid="ignore"):
        x = env * (carrier(len(env)) if u is None else u[:len(env)]) if random_carrier else env.astype(np.complex128)
        return x.astype(np.complex64)


def level(n, nulls=(), base=1.0):
    """envelope `base` with (start, width, gain) nulls"""
    env = np.full(n, base, np.float64)
    for s, w, g in nulls:
        env[s:s + w] *= g
    return env


# ---------------------------------------------------------------------------------------------------------------- the restatement's view
def run_oracle(iq, want_cir=True):
    """the restatement over one stream with its attempt trace.  Capacities: the all-zero stream makes one attempt per 2098 samples"""
    cap = len(iq) // 2000 + 16
    o = R.orc_receiver_run(iq, cir_cap=cap if want_cir else 0, trace_cap=4 * cap)
    att = [Attempt(*v) for k, v in o["trace"] if k == R.TR_ATTEMPT]
    assert o["n_cir"] == len(att) and (not want_cir or len(o["cir"]) == len(att))
    return Oracle(o["trace"], att, o["cir"], o["n_sync_false"], o["n_sync_true"], len(iq))


def events(o, kind):
    return [v for k, v in o.trace if k == kind]


def comparable(o):
    """THE comparison rule.  The device starts a window search only when pos + SYNC_NEED <= n_valid (a whole frame with the largest
    window index must be in the ring), the restatement tries whenever 2048 samples are left: the attempts both sides make are the
    restatement's with buf_pos + SYNC_NEED <= n.  -> indices into o.attempts"""
    return [k for k, a in enumerate(o.attempts) if a.pos + SYNC_NEED <= o.n]


def searched_to_the_end(o):
    """no window search the device cannot make: both sides then run the null-symbol search to the last sample, and the number of
    notSynced entries must agree"""
    return len(comparable(o)) == len(o.attempts)


def expected_slots(o):
    """what dabphy_get_frame_info reports for the comparable attempts, in order: a found frame (valid = 1) carries the correctors as they
    are after it, a failed search (valid = 3) the ones it was made with"""
    out = []
    for k in comparable(o):
        a = o.attempts[k]
        if a.start_index >= 0:
            assert a.completed, "a found frame with SYNC_NEED samples behind its search is demodulated to its end"
            out.append((a.pos, a.start_index, 1, a.coarse_after, a.fine_after))
        else:
            out.append((a.pos, a.start_index, 3, a.coarse, a.fine))
    return out


def first_lock_attempts(o):
    for k in comparable(o):
        if o.attempts[k].start_index >= 0:
            return o.attempts[k].n_sync_false
    return -1


# ---------------------------------------------------------------------------------------------------------------- derivations
def _probe(iq):
    return run_oracle(iq, want_cir=False)


def _first(o, kind, field=0):
    ev = events(o, kind)
    return ev[0][field] if ev else None


def _solve(build, measure, target, x0):
    """integer x with measure(oracle(build(x))) == target, for a measure that moves one for one with x"""
    x = x0
    for _ in range(6):
        got = measure(_probe(build(x)))
        assert got is not None, (x, target)
        if got == target:
            return x
        x += target - got
    raise AssertionError("no solution for %r from %r" % (target, x0))


def _bisect32(detected, lo, hi):
    """neighbouring float32 gains lo < hi with detected(lo) != detected(hi)"""
    lo, hi = np.float32(lo), np.float32(hi)
    dlo = detected(lo)
    assert dlo != detected(hi)
    while np.nextafter(lo, np.float32(np.inf)) < hi:
        mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
        if detected(mid) == dlo:
            lo = mid
        else:
            hi = mid
    return lo, hi


# ---------------------------------------------------------------------------------------------------------------- the families
def _degenerate():
    n = N_SHORT; cases = []
    nominal = [(NULL_AT, T_NULL, 0.0)]
    cases.append(("zeros", np.zeros(n, np.complex64)))
    env = level(n); env[T_F // 2:] = 0
    cases.append(("zeros_after_priming", stream(env, False)))
    cases.append(("constant", stream(level(N_LONG), False)))              # no dip: hopeless after T_F samples, again and again
    for what, v in (("nan", np.nan), ("inf", np.inf)):
        for where, at in (("after_priming", P0 + 1000), ("during_priming", 40000)):
            env = level(n, nominal); env[at] = v
            cases.append(("%s_%s" % (what, where), stream(env, False)))
    # denormals in the envelope, the moving sum and sLevel; |re| + |im| overflowing
    for s in (1e-36, 1e-40, 1e-44, 1e30, 3e38):
        cases.append(("nominal*%g" % s, stream(level(n, nominal, base=s), True)))
    for s in (1e-40, 3e38):
        cases.append(("nominal*%g,exact" % s, stream(level(n, nominal, base=s), False)))
    return cases


WIDTHS = (1, 49, 50, 51, 100, T_NULL)


def _widths():
    return [("null%d,%s" % (w, "random" if rc else "exact"), stream(level(N_SHORT, [(NULL_AT, w, 0.0)]), rc)) for rc in (False, True) for w in WIDTHS]


RISE_LIMIT, FALL_LIMIT = T_NULL + 50, T_F


def _rise_limit():
    """null widths that end the second loop with counter = limit - 2 .. limit, and the two next ones, which it does not survive"""
    def build(w):
        return stream(level(N_SHORT, [(NULL_AT, w, 0.0)]), False)
    w_lim = _solve(build, lambda o: _first(o, R.TR_RISE), RISE_LIMIT, RISE_LIMIT)
    cases = [("rise_limit%+d" % k, build(w_lim + k)) for k in range(-2, 3)]
    cases.append(("rise_limit,two_rounds", build(2 * (RISE_LIMIT + 1) + 50 + 1000)))
    return cases


def _fall_limit():
    """null starts that end the first loop with counter = limit - 2 .. limit, and the two next ones; the envelope index passes 32 767"""
    def build(s):
        return stream(level(N_LONG, [(s, T_NULL, 0.0)]), False)
    s_lim = _solve(build, lambda o: _first(o, R.TR_FALL), FALL_LIMIT, P0 + FALL_LIMIT - 30)
    return [("fall_limit%+d" % k, build(s_lim + k)) for k in range(-2, 3)]


PLATEAU_AT, PLATEAU_LEN = NULL_AT + 2000, 4000
SWEEP = (-3e-3, -2e-3, -1e-3, 0.0, 1e-3, 2e-3, 3e-3)


def _depth(g):
    return stream(level(N_SHORT, [(NULL_AT, T_NULL, float(g))]), True)


def _plateau(p):
    return stream(level(N_SHORT, [(NULL_AT, 2000, 0.0), (PLATEAU_AT, PLATEAU_LEN, float(p))]), True)


def fall_detected(o):
    """the first loop ended inside the null"""
    return any(NULL_AT <= v[1] <= NULL_AT + T_NULL + 60 for v in events(o, R.TR_FALL))


def rise_detected(o):
    """the second loop ended by its condition before its limit"""
    return len(events(o, R.TR_RISE)) > 0 and not any(v[1] == R.CAUSE_HOPELESS_RISE for v in events(o, R.TR_NOTSYNCED)[:2])


def _thresholds():
    cases = []
    lo, hi = _bisect32(lambda g: fall_detected(_probe(_depth(g))), 0.2, 0.6)
    for k, r in enumerate(SWEEP):
        cases.append(("depth%+d" % (k - 3), _depth(np.float32(float(lo) * (1 + r)))))
    cases += [("depth,last_detected", _depth(lo)), ("depth,first_missed", _depth(hi))]
    lo, hi = _bisect32(lambda p: rise_detected(_probe(_plateau(p))), 0.3, 0.9)
    for k, r in enumerate(SWEEP):
        cases.append(("plateau%+d" % (k - 3), _plateau(np.float32(float(hi) * (1 + r)))))
    cases += [("plateau,last_missed", _plateau(lo)), ("plateau,first_detected", _plateau(hi))]
    return cases


# (crossing, multiple of the tile, offsets): the loop's condition is met after `multiple * TILE + offset` samples of the search tile
TILE_EDGES = (("fall", 3, range(-3, 4)), ("fall", 1, range(-1, 2)), ("rise", 6, range(-3, 4)), ("rise", 4, range(-1, 2)))


def _tile_edges():
    cases = []
    for kind, m, offs in TILE_EDGES:
        for o in offs:
            target = m * TILE + o
            if kind == "fall":
                def build(s):
                    return stream(level(N_SHORT, [(s, T_NULL, 0.0)]), False)
                x = _solve(build, lambda orc: _first(orc, R.TR_FALL), target, P0 + target - 30)
            else:
                s = P0 + target - 2600
                def build(w, s=s):
                    return stream(level(N_SHORT, [(s, w, 0.0)]), False)
                x = _solve(build, lambda orc: _first(orc, R.TR_RISE, 1) - P0, target, 2580)
            cases.append(("%s@%dx%d%+d" % (kind, m, TILE, o), build(x)))
    # the first loop's condition is met by the 50 samples taken before it: the last null start for which it ends with counter 0, and the next
    def build(s):
        return stream(level(N_SHORT, [(s, T_NULL, 0.0)]), False)
    s = P0 - 45
    while _first(_probe(build(s + 1)), R.TR_FALL) == 0:
        s += 1
        assert s < P0
    cases += [("fall@take50", build(s)), ("fall@take50+1", build(s + 1))]
    return cases


PREFIX_FRAMES, TAIL = 4, T_F // 3 + 2 * T_F              # (the weak tail needs ~2 * 10^5 samples before sLevel has come down to it)
TAIL_NULLS = (700, 3000, 3001, 9999, 60000)


@functools.lru_cache(maxsize=None)
def prefix():
    """4 real frames at +2437 Hz and 25 dB: the receiver locks with coarse = 2000 and a fine corrector that is not 0"""
    return synth.make_stream(PREFIX_FRAMES, snr_db=25, cfo_hz=2437.0, seed=7)


# seed of the tails' random-phase carrier.  ThresholdBeforePeak finds "a window" in most stretches of noise (its index 0), and these cases
# are about what follows a LOSS of lock: a seed with which the window search right behind the prefix fails.  validate() asserts that it does.
TAIL_SEED = 3


@functools.lru_cache(maxsize=None)
def tail_carrier():
    return np.exp(2j * np.pi * _rng("tail%d" % TAIL_SEED).random(TAIL))


@functools.lru_cache(maxsize=None)
def tail_search_at():
    """where in the tail the null-symbol search starts: behind the window search that loses the lock (the frame in front of it takes its
    null symbol from the tail too).  The tails' nulls are placed from here."""
    pre = prefix()
    a = _probe(np.concatenate([pre, stream(level(4 * T_U, base=float(np.mean(np.abs(pre)))), True, tail_carrier())])).attempts[-1]
    assert a.start_index < 0 and a.pos >= len(pre)
    return a.pos + T_U - len(pre)


def _reacquire():
    pre = prefix()
    amp = float(np.mean(np.abs(pre))); at = tail_search_at()
    def with_tail(env):
        return np.concatenate([pre, stream(env, True, tail_carrier())])
    cases = [("tail,null@%d" % s, with_tail(level(TAIL, [(at + s, T_NULL, 0.0)], base=amp))) for s in TAIL_NULLS]
    # a tail at another level: sLevel still is the prefix's and takes ~10^5 samples to follow.  The weak tail's first nulls end in the
    # second loop's limit, round after round, until 0.75 sLevel has come down to the tail: a null every half frame, so that one is left
    periodic = [(at + 3000 + k * (T_F // 2), T_NULL, 0.0) for k in range(4)]
    cases.append(("tail*4", with_tail(level(TAIL, periodic, base=4 * amp))))
    cases.append(("tail*0.3", with_tail(level(TAIL, periodic, base=0.3 * amp))))
    cases.append(("tail,zeros", with_tail(np.zeros(TAIL))))
    cases.append(("tail,then_signal", np.concatenate([pre, stream(level(T_F // 3, base=amp), True, tail_carrier()), pre[:TAIL - T_F // 3]])))
    return cases


_BUILDERS = dict(degenerate=_degenerate, widths=_widths, rise_limit=_rise_limit, fall_limit=_fall_limit, thresholds=_thresholds,
                 tile_edges=_tile_edges, reacquire=_reacquire)


@functools.lru_cache(maxsize=None)
def family(name):
    cases = [Case(n, name, np.ascontiguousarray(x, np.complex64)) for n, x in _BUILDERS[name]()]
    assert len({c.name for c in cases}) == len(cases)
    return cases


@functools.lru_cache(maxsize=None)
def oracle(name):
    """{case name: Oracle}, computed once for every suite that asks"""
    return {c.name: run_oracle(c.iq) for c in family(name)}


def batches(name):
    """cases of equal length share a handle, MAX_BATCH at most"""
    by_len = collections.OrderedDict()
    for c in family(name):
        by_len.setdefault(len(c.iq), []).append(c)
    return [g[i:i + MAX_BATCH] for g in by_len.values() for i in range(0, len(g), MAX_BATCH)]


# ---------------------------------------------------------------------------------------------------------------- validity
def _entry_before(o, pos):
    """start of the search tile that holds stream position `pos`: the last notSynced entry in front of it, 50 samples on"""
    return max(v[0] for v in events(o, R.TR_NOTSYNCED) if v[0] + 50 <= pos) + 50


def validate():
    """every family reaches what it exists for -- from the restatement's traces alone"""
    O = {f: oracle(f) for f in FAMILIES}
    # second-loop limit: exit counters limit - 2 .. limit, one width apart; the next two widths are hopeless; the long null takes two rounds
    o = O["rise_limit"]
    assert [_first(o["rise_limit%+d" % k], R.TR_RISE) for k in (-2, -1, 0)] == [RISE_LIMIT - 2, RISE_LIMIT - 1, RISE_LIMIT]
    for k in (1, 2):
        t = o["rise_limit%+d" % k]
        assert not events(t, R.TR_RISE) and events(t, R.TR_NOTSYNCED)[1][1] == R.CAUSE_HOPELESS_RISE, k
    assert [v[1] for v in events(o["rise_limit,two_rounds"], R.TR_NOTSYNCED)[1:3]] == [R.CAUSE_HOPELESS_RISE] * 2 and events(o["rise_limit,two_rounds"], R.TR_RISE)
    # first-loop limit: the same around T_F; the envelope index has wrapped
    o = O["fall_limit"]
    assert [_first(o["fall_limit%+d" % k], R.TR_FALL) for k in (-2, -1, 0)] == [FALL_LIMIT - 2, FALL_LIMIT - 1, FALL_LIMIT] and FALL_LIMIT > 32767
    for k in (1, 2):
        t = o["fall_limit%+d" % k]
        assert events(t, R.TR_NOTSYNCED)[1][1] == R.CAUSE_HOPELESS_FALL and events(t, R.TR_NOTSYNCED)[1][0] == P0 + FALL_LIMIT + 1, k
    assert all(len(comparable(t)) >= 1 for t in o.values())
    # threshold sweeps: both outcomes, neighbouring floats included
    o = O["thresholds"]
    d = {n: fall_detected(t) for n, t in o.items() if n.startswith("depth")}
    assert d["depth,last_detected"] and not d["depth,first_missed"] and sum(d.values()) >= 3 and sum(not v for v in d.values()) >= 3, d
    p = {n: rise_detected(t) for n, t in o.items() if n.startswith("plateau")}
    assert p["plateau,first_detected"] and not p["plateau,last_missed"] and sum(p.values()) >= 3 and sum(not v for v in p.values()) >= 3, p
    # tile edges: each crossing at its offset from a multiple of the tile, counted from the start of its search tile
    o = O["tile_edges"]
    for kind, m, offs in TILE_EDGES:
        for k in offs:
            t = o["%s@%dx%d%+d" % (kind, m, TILE, k)]
            pos = events(t, R.TR_FALL if kind == "fall" else R.TR_RISE)[0][1]
            assert pos - _entry_before(t, pos) == m * TILE + k, (kind, m, k)
    assert _first(o["fall@take50"], R.TR_FALL) == 0 and _first(o["fall@take50+1"], R.TR_FALL) == 1
    # widths: a null shorter than the ~35 samples the moving sum needs is not seen, the others are
    o = O["widths"]
    for rc in ("exact", "random"):
        assert not events(o["null1,%s" % rc], R.TR_FALL) and all(events(o["null%d,%s" % (w, rc)], R.TR_ATTEMPT) for w in WIDTHS[1:])
    # degenerate: the all-zero stream "locks" every 2098 samples; a NaN makes every later comparison false
    o = O["degenerate"]
    z = o["zeros"].attempts
    assert len(z) > 90 and all(b.pos - a.pos == 2098 for a, b in zip(z, z[1:])) and z[0].pos == P0
    assert not o["constant"].attempts and [v[1] for v in events(o["constant"], R.TR_NOTSYNCED)] == [R.CAUSE_PRIMED, R.CAUSE_HOPELESS_FALL, R.CAUSE_HOPELESS_FALL]
    assert not o["zeros_after_priming"].attempts and o["zeros_after_priming"].n_sync_false > 50
    for what in ("nan", "inf"):                                # both loops end at once, from the sample on that carries it
        assert len(o[what + "_during_priming"].attempts) > 90 and o[what + "_during_priming"].attempts[0].pos == P0
        assert o[what + "_after_priming"].attempts[0].pos == P0 + 1001 and len(o[what + "_after_priming"].attempts) >= 3
    # re-acquisition: locked with the oscillator running, lock lost behind the prefix, then at least one comparable attempt (none on zeros)
    o = O["reacquire"]
    for n, t in o.items():
        c = [t.attempts[k] for k in comparable(t)]
        lost = next(k for k, a in enumerate(c) if a.start_index < 0)
        assert lost >= 2 and all(a.start_index >= 0 for a in c[:lost]) and c[lost].pos >= PREFIX_FRAMES * T_F - T_U, n
        assert c[lost].coarse == 2000 and c[lost].fine != 0, (n, c[lost])
        assert (len(c) == lost + 1) if n == "tail,zeros" else (len(c) > lost + 1), (n, len(c), lost)
    assert any(a.start_index >= 0 and a.pos > PREFIX_FRAMES * T_F for a in o["tail,then_signal"].attempts)      # lock regained
    # the set as a whole: every cause of a notSynced entry; cases with no comparable attempt and cases with many
    every = [t for f in FAMILIES for t in O[f].values()]
    assert {v[1] for t in every for v in events(t, R.TR_NOTSYNCED)} == {R.CAUSE_PRIMED, R.CAUSE_HOPELESS_FALL, R.CAUSE_HOPELESS_RISE, R.CAUSE_WINDOW_FAILED}
    assert sum(len(comparable(t)) == 0 for t in every) >= 10 and sum(len(comparable(t)) >= 3 for t in every) >= 10
    assert all(len(b) <= MAX_BATCH for f in FAMILIES for b in batches(f))


def census():
    """per family: (cases, comparable attempts in total)"""
    return {f: (len(family(f)), sum(len(comparable(t)) for t in oracle(f).values())) for f in FAMILIES}


# ---------------------------------------------------------------------------------------------------------------- the device's view
FEEDS = ("oneshot", "frames", "ring")          # stream_upload with F = 4; F = 1; live ring written in pieces, process(1) until starved


def run_batch(d_factory, cases, feed, track_slevel=False, **cfg):
    """-> per case: dict(slots = [(sample_pos, start_index, valid, coarse, fine)] over all valid = 1 / 3 slots in order, cir = their
    impulse responses, attempts, first_lock, lost, inexact)"""
    B, n = len(cases), len(cases[0].iq)
    x = np.stack([c.iq for c in cases])
    F = 4 if feed == "oneshot" else 1
    d = d_factory(n_ensembles=B, max_frames=F, want_constellation=False, **cfg)
    out = [dict(slots=[], cir=[]) for _ in cases]
    try:
        if track_slevel:
            d.set_track_slevel(True)

        def drain():
            while True:
                d.process(F)
                info = d.frame_info(); ir = d.impulse_response()
                for b in range(B):
                    for f in range(F):
                        i = info[b, f]
                        if i["valid"] in (1, 3):
                            out[b]["slots"].append((int(i["pos"]), int(i["start_index"]), int(i["valid"]), int(i["coarse"]), int(i["fine"])))
                            out[b]["cir"].append(ir[b, f].copy())
                if (info["valid"] == 0).all():
                    return
        if feed == "ring":
            d.stream_open(max(4, n // T_F + 2) * T_F)        # longer than the stream: nothing is overwritten (4 frames: the shortest ring there is)
            for at in range(0, n, PIECE):
                d.stream_write(x[:, at:at + PIECE])
                drain()                                      # the search starves and resumes in the next call, wherever it is
        else:
            d.stream_upload(x)
            drain()
        attempts, first = d.scan_stats()
        lost, _ = d.sync_stats()
        for b in range(B):
            out[b].update(attempts=int(attempts[b]), first_lock=int(first[b]), lost=int(lost[b]), inexact=int(d.relock_inexact[b]))
    finally:
        d.close()
    return out


def same_bits(a, b):
    """bit for bit -- where both hold a number.  Which NaN an operation makes is the processor's choice (x86's default NaN has the sign bit
    set, the device's and most other CPUs' has not), so the reference itself differs there from machine to machine: a NaN equals a NaN"""
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def assert_case(case, o, got, where):
    tag = "%s [%s]" % (case.name, where)
    want = expected_slots(o)
    assert got["slots"] == want, "%s: window searches (pos, index, valid, coarse, fine)\n device   %s\n expected %s" % (tag, got["slots"][:12], want[:12])
    for j, k in enumerate(comparable(o)):
        assert same_bits(got["cir"][j], o.cir[k]), "%s: impulse response of attempt %d at %d differs" % (tag, j, want[j][0])
    assert got["first_lock"] == first_lock_attempts(o), (tag, got["first_lock"], first_lock_attempts(o))
    if searched_to_the_end(o):                              # (a case without a comparable attempt is compared here, on its notSynced count)
        assert got["attempts"] == o.n_sync_false, "%s: %d notSynced entries, the reference makes %d" % (tag, got["attempts"], o.n_sync_false)
    assert got["lost"] == sum(1 for s in want if s[2] == 3), (tag, got["lost"])
    assert got["inexact"] == 0, tag


def check_family(d_factory, name, feed, track_slevel=False, **cfg):
    """every case of the family, no case left out; returns the one-shot-comparable results for callers that compare feeds"""
    orc = oracle(name)
    for batch in batches(name):
        got = run_batch(d_factory, batch, feed, track_slevel=track_slevel, **cfg)
        for c, g in zip(batch, got):
            assert_case(c, orc[c.name], g, feed + (",track" if track_slevel else "") + ("," + repr(cfg) if cfg else ""))
