"""Cases for the Reed-Solomon syndromes taken from the generator-polynomial remainder (rs_codec.h: rs_remainder120 +
rs_syndromes_from_remainder) and for the superframe filter's wide pass with several attempts per work-group (k_superframe_wide); run by
tests/test_emu_rs_remainder.py on the execution model and by tests/test_gpu_rs_remainder.py on the device."""
import functools

import numpy as np

import parity_cases as P
import refapi as R
import sf_cases as S

RS_S = (1, 8, 9, 48)      # code words per superframe: a lone lane, the benchmark's, one over an eight-column boundary, the widest


@functools.lru_cache(maxsize=None)
def rs_words():
    """-> (received [n][120], sent [n][120], outcome [n]) with outcome from the ORACLE alone (each word decoded as a superframe of one column):
    'clean', 'corrected', 'given_up', 'miscorrected'.
      * for every position 0 .. 119 (0 = the first byte into the shift register, 110 .. 119 the parity, 119 the last shift) a code word
        with one error there, the values varying;
      * five errors that include that position (stride 24 around the word), and six (one more, 12 further on);
      * clean words, the all-zero word, the all-0xFF word;
      * the directed sets of sf_cases (roots in the padding, miscorrections written in full, the edges, zero data, S0 = 0, random weights);
    interleaved round-robin, so that words of different kinds are neighbours (pack_columns: neighbouring columns = neighbouring lanes)."""
    rng = np.random.RandomState(2024)
    groups = []
    one, five, six = [], [], []
    for p in range(120):
        c = S.random_codeword(rng); r = c.copy(); r[p] ^= 1 + (p * 37 + 11) % 255
        one.append((r, c))
        pos5 = [(p + 24 * k) % 120 for k in range(5)]
        c = S.random_codeword(rng); r = c.copy(); r[pos5] ^= rng.randint(1, 256, 5).astype(np.uint8)
        five.append((r, c))
        pos6 = pos5 + [(p + 12) % 120]
        c = S.random_codeword(rng); r = c.copy(); r[pos6] ^= rng.randint(1, 256, 6).astype(np.uint8)
        six.append((r, c))
    groups += [one, five, six]
    plain = []
    for _ in range(6):
        c = S.random_codeword(rng); plain.append((c.copy(), c))
    z = np.zeros(120, np.uint8); f = np.full(120, 0xFF, np.uint8)
    plain += [(z.copy(), z), (f.copy(), f), (z.copy(), z), (f.copy(), f)]        # (all-0xFF: `sent` is only what outcome compares with -- the oracle decides)
    groups.append(plain)
    for name, (rx, tx) in sorted(S.directed_sets().items()):
        groups.append(list(zip(rx, tx)))
    words = []
    for k in range(max(len(g) for g in groups)):
        for g in groups:
            if k < len(g):
                words.append(g[k])
    rx = np.array([w[0] for w in words], np.uint8); tx = np.array([w[1] for w in words], np.uint8)
    outcome = []
    for r, c in zip(rx, tx):
        o, n, u = R.orc_rs_superframe(r)
        outcome.append("given_up" if u else "miscorrected" if not np.array_equal(o, c) else "corrected" if n else "clean")
    return rx, tx, tuple(outcome)


@functools.lru_cache(maxsize=None)
def rs_superframes_of(s):
    """the words in superframes of s columns, so many that the last wave of 64 lanes is partly filled; with the oracle's results per superframe"""
    rx, tx, outcome = rs_words()
    rng = np.random.RandomState(300 + s)
    words = list(rx)
    while len(words) % s or (len(words) % 64) == 0:
        words.append(S.random_codeword(rng))
    sfs = S.pack_columns(words, s, rng)
    assert (sfs.shape[0] * s) % 64 != 0
    want = [R.orc_rs_superframe(sf) for sf in sfs]
    return sfs, want


def check_rs_syndromes(d, s):
    """dabphy_rs_superframes (k_rs_superframes: rs_decode120, the one syndrome definition) against orc_rs_superframe: bytes, corrected counts,
    verdicts; every outcome occurs in the run"""
    outcome = rs_words()[2]
    assert {"clean", "corrected", "given_up", "miscorrected"} <= set(outcome), set(outcome)
    sfs, want = rs_superframes_of(s)
    out, corr, unc = d.rs_superframes(sfs.copy(), s)
    for k, (o, c, u) in enumerate(want):
        assert np.array_equal(out[k], o), "s = %d, superframe %d: corrected bytes differ at %s" % (s, k, np.nonzero(out[k] != o)[0][:8])
        assert (int(corr[k]), bool(unc[k])) == (int(c), bool(u)), (s, k, int(corr[k]), int(unc[k]), c, u)


# ---- the grouped wide pass through streams.  Default ensemble: 18 x 64 kbit/s (s = 8: eight attempts per work-group), sub-channels 1 and 6.
# The receiver emits logical frame j at CIF 16 + j of the stream it processes (the time de-interleaver's fill), a batch of F frames is CIFs
# [4 F b, 4 F (b + 1)), emitted frame j carries transmitted frame j + 4, so superframe q of the stream completes at j = 5 q: the attempts of
# a batch in lock are the j = 0 mod 5 it holds, j >= 5.  Batch 0 is always walked (its first window is not aligned), and so is the batch
# behind a lost superframe that was the last of its batch (it starts on a full window that failed).
# name: (F, nf, broken, lost, B, where the lost superframe has to fall: (attempts of its batch, its attempt)).  `broken` is a superframe with
# a code word beyond repair that still synchronises (the error path's workspace of its lane), `lost` one that does not: its pair is walked.
WIDE_CASES = {
    "one_attempt": (2, 22, 3, 7, 2, None),                  # 8 rows a batch: one or two attempts, 0 .. 4 frames carried
    "carried_0_to_4": (3, 22, 6, 8, 3, None),               # 12 rows: the carried count walks through 0 .. 4, attempt 0 reads the state
    "seven_last": (9, 28, 13, 18, 2, (7, 6)),               # 36 rows: a batch of eight (settled), then one of seven with its last attempt lost
    "eight_first": (10, 30, 9, 5, 2, (8, 0)),               # 40 rows: exactly one work-group; its first attempt lost, the others synchronise
    "eight_last": (10, 31, 16, 20, 2, (8, 7)),              # ... its last, behind a batch of eight that is settled
    "nine_second_group": (11, 35, 8, 23, 2, (9, 8)),        # 44 rows: nine attempts = a full work-group and a lone attempt; a batch settled, then the lone attempt lost
}


def broken_and_lost_payload(seed, broken, lost):
    """DAB+ payload whose superframe `broken` (counted from the start of the stream) has a code word beyond the RS capacity inside an access
    unit, and whose superframe `lost` loses a header column, so that the Fire code fails and the window slides (the damage of
    parity_cases.damaged_dabplus_payload, once in the stream instead of once per period)"""
    from welle_io_amd import synth
    base = synth.dabplus_payload_fn(80, seed)

    def payload(sc, r):
        data = bytearray(base(sc, r))
        q, k, s = r // 5, r % 5, sc.bitrate // 8
        if q == broken and k == 2:
            data[40] ^= 0x5A
            for j in range(12): data[3 + j * s] ^= 0x33
        if q == lost and k == 0:
            data[0] ^= 0xFF; data[s] ^= 0xFF; data[2 * s] ^= 1; data[3 * s] ^= 7
            for j in range(4, 10): data[j * s] ^= 0x81
        return bytes(data)
    return payload


def attempt_of(F, j):
    """(attempts of the batch that holds emitted frame j, rank of the attempt completed by j) for a receiver in lock"""
    b = (16 + j) // (4 * F)
    js = [k for k in range(5, 4 * F * (b + 1), 5) if (16 + k) // (4 * F) == b]
    return len(js), js.index(j)


def check_wide_groups(factory, name):
    F, nf, broken, lost, B, placed = WIDE_CASES[name]
    st = {}
    got = P.check_superframes_vs_oracle(factory, F=F, nf=nf, B=B, auto_modes=(True,), stats=st, payload_fn=broken_and_lost_payload(12, broken, lost))
    settled, tried = st["sf_wide"]
    assert 0 < settled < tried, (settled, tried)             # both ways through a batch were taken
    ev = st["oracle_events"][0]
    assert any(e[2] and e[3] for e in ev) and any(e[1] > 0 and e[3] for e in ev), "no superframe with a word given up / with corrections synchronised"
    missed = [e[0] for e in ev if e[0] >= 5 and e[0] % 5 == 0 and not e[3]]
    assert missed == [5 * lost], (missed, lost)
    if placed:
        assert attempt_of(F, 5 * lost) == placed, (attempt_of(F, 5 * lost), placed)
    return got


def check_wide_other_buckets(factory):
    """the 2880- and 5760-byte buckets and their attempts per work-group: 128 / 192 / 256 kbit/s (s = 16 / 24 / 32: four / two / two attempts) and
    32 kbit/s (s = 4: sixteen), five frames a batch = four attempts a pair"""
    from welle_io_amd import synth
    ens = [synth.SubchannelCfg(1, 0, 128), synth.SubchannelCfg(2, 96, 192), synth.SubchannelCfg(3, 240, 256), synth.SubchannelCfg(4, 432, 32)]
    st = {}
    P.check_superframes_vs_oracle(factory, F=5, nf=22, B=2, ensemble=ens, pick=(0, 1, 2, 3), damage_q=(6, 9), auto_modes=(True,), stats=st)
    settled, tried = st["sf_wide"]
    assert 0 < settled < tried, (settled, tried)


def check_wide_layouts(factory):
    """every access-unit layout and rejection rule at 8 .. 384 kbit/s (1 .. 48 code words: 64 attempts per work-group down to one), six frames a
    batch = four or five attempts a pair (the deepest batch that fits inside the ten superframes in a row that sf_cases.TABLE lets synchronise)"""
    P.check_superframe_layouts(factory, F=6, nf=24, B=2, auto_modes=(True,))


def check_wide_timing_driver(factory, F=6, nf=24):
    """dabphy_time_superframe_wide repeats the wide launches of the last pass and leaves the pipeline as it found it: the filter's totals of
    every batch are the same with the driver called after each batch as without it; it refuses (DABPHY_ERR_STATE) before the first pass and
    after the classes' buffers have been replaced"""
    from welle_io_amd import synth
    from welle_io_amd.capi import DabPhyError
    x, tx = synth.make_stream(nf, snr_db=5.0, cfo_hz=20, delay=50, return_tx=True, seed=12, payload_fn=P.damaged_dabplus_payload(12, True, (9, 13)))
    subs = [tx.subchs[i] for i in (1, 6)]

    def run(timed):
        d = factory(n_ensembles=2, max_frames=F, want_constellation=False)
        try:
            def refused():
                try:
                    d.time_superframe_wide(1)
                except DabPhyError as e:
                    assert "status -5" in str(e), str(e)
                    return True
                return False
            if timed:
                assert refused()
            d.stream_upload(np.tile(np.asarray(x, np.complex64), (2, 1)))
            d.set_subchannels([(s.subch_id, s.start_cu, s.size_cu, d.protection_eep(s.bitrate, s.profile_b, s.level)) for s in subs])
            d.set_auto_superframes(True)
            tot = []
            for _ in range(nf // F):
                d.process(F)
                if timed:
                    assert d.time_superframe_wide(2) > 0.0
                tot.append(d.superframes_stats().copy())
            stats = d.wide_superframe_stats()
            if timed:
                d.set_subchannels([(s.subch_id, s.start_cu, s.size_cu, d.protection_eep(s.bitrate, s.profile_b, s.level)) for s in subs[:1]])
                assert refused()
            return np.array(tot), stats
        finally:
            d.close()
    plain, st0 = run(False)
    timed, st1 = run(True)
    assert plain[:, :, 0].sum() > 0 and 0 < st0[0] < st0[1], (plain, st0)        # superframes synchronised; batches settled and batches walked
    assert np.array_equal(plain, timed) and st0 == st1, (plain, timed, st0, st1)
