"""Cases and checks of the channel BER pass (k_chanber.hip) shared by tests/test_emu_chanber.py and tests/test_gpu_chanber.py.

Directed code words for the stateless entry (dabphy_channel_ber): per case one profile, a few code words, the expected counts from
the model (tests/chanber_model.py) fed with the ORACLE's decode of the same soft bits -- never the device's.  And the pass inside the
streaming receiver against the model fed with the oracle run's soft bits, FIBs and MSC bytes."""
import os

import numpy as np

import chanber_model as M
import mp2_chain
import parity_cases as P
import refapi as R
from welle_io_amd import synth

# ---------------------------------------------------------------------------------------------- directed code words
KINDS = ("clean", "flips", "zeros", "minus128", "allzero", "noise", "flips_zeros")
MAX_FLIPS = 8
NOISE_DB = 3.0


def directed_profiles():
    """the FIC (768 bits); EEP 8 kbit/s (198 steps: a last partial round of lanes); EEP 3-A 64 kbit/s; an EEP-B profile; a UEP profile
    with four puncturing segments; a 384 kbit/s code word (9222 steps)"""
    uep4 = [p for p in P.all_protection_profiles() if p[0] == "uep" and all(P.orc_profile(p).L[i] > 0 and P.orc_profile(p).PI[i] > 0 for i in range(4))]
    assert uep4
    return ["fic", ("eep", 8, 0, 2), ("eep", 64, 0, 3), ("eep", 32, 1, 2), uep4[len(uep4) // 2], ("eep", 384, 0, 3)]


def orc_prot(prof):
    return R.orc_prot_fic() if prof == "fic" else P.orc_profile(prof)


def dev_prot(d, prof):
    return d.protection_fic() if prof == "fic" else P.dev_profile(d, prof)


def orc_decode(po, soft):
    """the oracle's decode of punctured soft bits [n][n_in] -> bytes [n][nbits / 8] as dabphy_msc_deconvolve / dabphy_fic_decode return them"""
    prbs = R.orc_prbs(po.nbits)
    return np.stack([np.packbits(R.orc_msc_deconvolve(po, s) ^ prbs) for s in soft])


def clean_codeword(po, rng):
    """-> (payload bytes, soft bits at +-127)"""
    payload = rng.randint(0, 256, po.nbits // 8).astype(np.uint8)
    coded = M.reencode(po, payload)
    return payload, np.where(coded > 0, 127, -127).astype(np.int8)


def flip_positions(po, k, rng):
    """k punctured positions whose mother-code bits lie at least 64 apart"""
    mother = np.flatnonzero(M.mask_of(po))
    step = max(64, len(M.mask_of(po)) // k)
    assert (k - 1) * step + 64 <= len(M.mask_of(po)), "code word too short for %d flips" % k
    first = int(rng.randint(0, len(M.mask_of(po)) - (k - 1) * step - 63))
    pos = [int(np.searchsorted(mother, first + i * step)) for i in range(k)]
    pos = [min(p, len(mother) - 1) for p in pos]
    assert all(mother[b] - mother[a] >= 64 for a, b in zip(pos, pos[1:])) or k == 1, (po.nbits, k)
    return np.array(pos)


def make_codeword(po, kind, rng):
    """-> (soft [n_in], payload bytes or None, flips k, zeros): payload is set where the oracle must recover it"""
    n_in = po.n_in
    payload, s = clean_codeword(po, rng)
    k = zeros = 0
    if kind == "allzero":
        return np.zeros(n_in, np.int8), None, 0, n_in
    if kind == "noise":
        coded = (s > 0).astype(np.float64)
        amp = 40.0; sigma = amp / np.sqrt(2.0 * 10 ** (NOISE_DB / 10))
        v = np.clip(np.round((2 * coded - 1) * amp + rng.randn(n_in) * sigma), -127, 127).astype(np.int8)
        return v, None, 0, int((v == 0).sum())
    if kind in ("flips", "flips_zeros", "minus128"):
        k = int(rng.randint(1, MAX_FLIPS + 1))
        k = min(k, max(1, (len(M.mask_of(po)) - 64) // 64))
        pos = flip_positions(po, k, rng)
        k = len(set(pos.tolist()))
        s = s.copy(); s[pos] = -s[pos]
    if kind == "minus128":
        s = np.where(s < 0, -128, s).astype(np.int8)       # every negative soft bit, the flipped ones included
    if kind in ("zeros", "flips_zeros"):
        free = np.ones(n_in, bool)
        if k:
            free[pos] = False
        z = rng.choice(np.flatnonzero(free), max(1, n_in // 24), replace=False)
        s = s.copy(); s[z] = 0; zeros = len(z)
    return s, payload, k, zeros


_CASES = {}


def directed_case(pi, prof, n):
    """n code words of one profile, the kinds in turn (starting at another kind per profile and count) -> dict(prof, soft, decoded, want)"""
    key = (pi, n)
    if key not in _CASES:
        po = orc_prot(prof)
        rng = np.random.RandomState([17, pi, n])
        kinds = [KINDS[(pi + n + i) % len(KINDS)] for i in range(n)]
        made = [make_codeword(po, kd, rng) for kd in kinds]
        soft = np.stack([m[0] for m in made])
        decoded = orc_decode(po, soft)
        want = M.counts_many(po, soft, decoded)
        for i, (s, payload, k, zeros) in enumerate(made):
            if payload is not None:      # clean / sparse flips / zeros: the oracle recovers the payload, so the counts are known exactly
                assert np.array_equal(decoded[i], payload), "%s code word %d (%s): the oracle did not recover the payload" % (prof, i, kinds[i])
                assert tuple(want[i]) == (k, po.n_in - zeros), (prof, i, kinds[i], tuple(want[i]), k, po.n_in - zeros)
            elif kinds[i] == "allzero":
                assert tuple(want[i]) == (0, 0)
        soft.setflags(write=False); decoded.setflags(write=False); want.setflags(write=False)
        _CASES[key] = dict(prof=prof, kinds=kinds, soft=soft, decoded=decoded, want=want)
    return _CASES[key]


def directed_cases():
    return [directed_case(pi, prof, n) for pi, prof in enumerate(directed_profiles()) for n in (1, 3, 65)]


def check_directed(d):
    """dabphy_channel_ber equals the model on every case, count for count; returns the code words checked"""
    n_cw = 0; kinds = set()
    for c in directed_cases():
        got = d.channel_ber(dev_prot(d, c["prof"]), c["soft"], c["decoded"])
        g = np.stack([got["errors"], got["compared"]], 1).astype(np.int64)
        assert np.array_equal(g, c["want"]), "%s x %d: code words %s differ: got %s, model %s" % (
            c["prof"], len(g), np.flatnonzero((g != c["want"]).any(1))[:5], g[(g != c["want"]).any(1)][:5], c["want"][(g != c["want"]).any(1)][:5])
        n_cw += len(g); kinds |= set(c["kinds"])
    assert kinds == set(KINDS)
    return n_cw


def sweep_profiles(full):
    return P.all_protection_profiles() if full or os.environ.get("DABPHY_FULL_CPU_SUITE") else P.lin_sweep_profiles()


_SWEEP = {}


def sweep_case(prof):
    """two noisy code words (3 dB, -128 among them) of one profile and the model's counts on the oracle's decode"""
    if prof not in _SWEEP:
        po = P.orc_profile(prof)
        rng = np.random.RandomState([23, {"eep": 0, "uep": 1}[prof[0]]] + [int(v) for v in prof[1:]])
        soft = np.stack([make_codeword(po, "noise", rng)[0] for _ in range(2)])
        soft[1, rng.randint(0, po.n_in, 5)] = -128
        decoded = orc_decode(po, soft)
        want = M.counts_many(po, soft, decoded)
        soft.setflags(write=False); decoded.setflags(write=False)
        _SWEEP[prof] = (soft, decoded, want)
    return _SWEEP[prof]


def check_profile_sweep(d, profiles):
    failed = []
    for prof in profiles:
        soft, decoded, want = sweep_case(prof)
        got = d.channel_ber(P.dev_profile(d, prof), soft, decoded)
        g = np.stack([got["errors"], got["compared"]], 1).astype(np.int64)
        if not np.array_equal(g, want):
            failed.append("%s: got %s, model %s" % (P.profile_name(prof), g.tolist(), want.tolist()))
    assert not failed, "%d of %d profiles differ from the model:\n  " % (len(failed), len(profiles)) + "\n  ".join(failed)
    return len(profiles)


def check_entry_errors(d, capi):
    """the stateless entry refuses what it cannot count; the getters refuse while the feature is off"""
    p = d.protection_eep(8, 0, 3)
    soft = np.zeros((1, d.protection_input_bits(p)), np.int8); dec = np.zeros((1, p.nbits // 8), np.uint8); out = np.zeros(1, capi.BER_COUNT_DTYPE)
    import ctypes as C
    assert d.lib.dabphy_channel_ber(d.h, C.byref(p), None, capi._p(dec), 1, capi._p(out)) != 0
    assert d.lib.dabphy_channel_ber(d.h, C.byref(p), capi._p(soft), capi._p(dec), 0, capi._p(out)) != 0
    bad = capi.Protection(); bad.nbits = 100
    assert d.lib.dabphy_channel_ber(d.h, C.byref(bad), capi._p(soft), capi._p(dec), 1, capi._p(out)) != 0
    assert d.lib.dabphy_set_channel_ber(d.h, 2) != 0
    d.lib.dabphy_struct_size.restype = C.c_size_t
    assert d.lib.dabphy_struct_size(12) == capi.BER_COUNT_DTYPE.itemsize == 8        # DABPHY_STRUCT_BER_COUNT


# ---------------------------------------------------------------------------------------------- the pass inside dabphy_process
def small_mixed_subchannels():
    """EEP A and B, four levels, 8 .. 128 kbit/s, and a short-form (UEP) sub-channel: one protection class each"""
    return P.mixed_subchannels(cfgs=P.MIXED_CFGS[:5], uep=((8, 80, 1),))


class StreamModel:
    """the model over an oracle run: expected counts of any frame's FIC and of any logical frame of a sub-channel"""

    def __init__(self, o, subs):
        self.o = o; self.subs = subs
        self.n_frames = o["n_frames"]
        self.soft = [o["soft"][k] for k in range(self.n_frames)]
        self.fib = o["fib"][:12 * (len(o["fib"]) // 12)].reshape(-1, 12, 33)[:, :, 1:]
        self.po_fic = R.orc_prot_fic()
        self.po = [R.orc_prot_of(s) for s in subs]
        self.msc = [np.frombuffer(bytes(o["msc"][i]), np.uint8) for i in range(len(subs))]
        self._fic = {}; self._row = {}

    def fic(self, frame_no):
        if frame_no not in self._fic:
            self._fic[frame_no] = M.fic_counts(self.po_fic, self.soft[frame_no], self.fib[frame_no])
        return self._fic[frame_no]

    def known_frame(self, frame_no):
        return 0 <= frame_no < min(self.n_frames, len(self.fib))

    def known_row(self, i, c, cif0=0):
        """logical frame emitted at CIF c of a service fed from CIF cif0 on: the oracle decoded it and holds its soft bits"""
        fb = self.po[i].nbits // 8
        return c - cif0 >= 16 and (c - 16 + 1) * fb <= len(self.msc[i]) and (c - 1) >> 2 < self.n_frames

    def row(self, i, c):
        if (i, c) not in self._row:
            po = self.po[i]; fb = po.nbits // 8
            soft, present = M.msc_row_soft(self.soft, c, self.subs[i].start_cu, po.n_in)
            self._row[(i, c)] = M.counts(po, soft, self.msc[i][(c - 16) * fb:(c - 15) * fb], present)
        return self._row[(i, c)]


_ORACLE_RUNS = {}


def oracle_stream(key, make):
    """(x, subs, StreamModel) of a stream, computed once for every test that asks"""
    if key not in _ORACLE_RUNS:
        x, subs = make()
        o = R.orc_receiver_run(x, subchs=subs, want_soft=True)
        _ORACLE_RUNS[key] = (x, subs, StreamModel(o, subs))
    return _ORACLE_RUNS[key]


def mixed_stream(nf=9, snr_db=6.0, seed=31):
    def make():
        subs = small_mixed_subchannels()
        return synth.make_stream(nf, subchs=subs, snr_db=snr_db, cfo_hz=-55, delay=123, seed=seed), subs
    return oracle_stream(("mixed", nf, snr_db, seed), make)


def replay_stream(nf=22, snr_db=3.5, seed=10, cfo=40):
    """the stream of test_mp2_through_a_replayed_batch: at 3.5 dB with the coarse corrector in play a batch is decoded twice"""
    def make():
        subs, payload = mp2_chain.ensemble(seed=seed)
        return synth.make_stream(nf, snr_db=snr_db, cfo_hz=cfo, delay=50, seed=seed, payload_fn=payload, subchs=subs), subs
    return oracle_stream(("replay", nf, snr_db, seed, cfo), make)


def sub_tuple(d, s):
    return (s.subch_id, s.start_cu, s.size_cu, P.dev_prot(d, s))


def check_batch(d, model, lists, cif0, stats):
    """the last batch of handle d against the model.  lists[b] = [(index into model.subs, ...)] positions of ensemble b's list;
    cif0[b][position] = CIF from which that position's service has been fed.  All four things the contract names:
    FIC counts, per-service rows and totals equal the model; first_valid / n_rows equal dabphy_get_msc_ensemble's; rows outside
    [first_valid, n_rows) and frames that are not valid have compared == 0; the totals are the sums of the rows"""
    info = d.frame_info()
    B, F = info.shape
    fic = d.channel_ber_fic()
    te, tc = d.channel_ber_totals()
    assert te.shape == (B, 1 + max(len(l) for l in lists))
    for b in range(B):
        for f in range(F):
            g = np.stack([fic[b, f]["errors"], fic[b, f]["compared"]], 1).astype(np.int64)
            fn = int(info[b, f]["frame_no"])
            if info[b, f]["valid"] != 1:
                assert not g.any(), "ensemble %d frame slot %d is not valid but has FIC counts %s" % (b, f, g.tolist())
                stats["invalid"] += 1
            elif model.known_frame(fn):
                assert np.array_equal(g, model.fic(fn)), "ensemble %d frame %d: FIC counts %s, model %s" % (b, fn, g.tolist(), model.fic(fn).tolist())
                stats["fic"] += 4; stats["fic_errors"] += int(g[:, 0].sum())
        assert (int(te[b, 0]), int(tc[b, 0])) == (int(fic[b]["errors"].sum()), int(fic[b]["compared"].sum())), "ensemble %d: FIC totals" % b
        c0 = 4 * int(info[b, 0]["frame_no"])
        for pos, i in enumerate(lists[b]):
            rows, fv, nr = d.channel_ber_ensemble(b, pos)
            _, mfv, mnr = d.msc_ensemble(b, pos)
            assert (fv, nr) == (mfv, mnr), "ensemble %d position %d: rows [%d, %d), dabphy_get_msc_ensemble says [%d, %d)" % (b, pos, fv, nr, mfv, mnr)
            g = np.stack([rows["errors"], rows["compared"]], 1).astype(np.int64)
            for r in range(4 * F):
                if r < fv or r >= nr:
                    assert not g[r].any(), "ensemble %d position %d row %d lies outside [%d, %d) but has counts %s" % (b, pos, r, fv, nr, g[r].tolist())
                    stats["empty_rows"] += 1
                elif model.known_row(i, c0 + r, cif0[b][pos]):
                    assert tuple(g[r]) == model.row(i, c0 + r), "ensemble %d position %d (sub-channel %d) CIF %d: counts %s, model %s" % (b, pos, i, c0 + r, g[r].tolist(), model.row(i, c0 + r))
                    stats["rows"] += 1; stats["row_errors"] += int(g[r, 0])
            assert (int(te[b, 1 + pos]), int(tc[b, 1 + pos])) == (int(g[:, 0].sum()), int(g[:, 1].sum())), "ensemble %d position %d: totals are not the sum of the rows" % (b, pos)
        assert not te[b, 1 + len(lists[b]):].any() and not tc[b, 1 + len(lists[b]):].any()
    return info


def new_stats():
    return dict(fic=0, fic_errors=0, rows=0, row_errors=0, empty_rows=0, invalid=0, replayed=0)


def run_stream(d_factory, stream, F, B=2, pipeline_sync=0, **cfg):
    """the feature on over a whole stream, B copies of it side by side, every batch checked; returns the statistics of what was compared"""
    x, subs, model = stream
    d = d_factory(n_ensembles=B, max_frames=F, want_constellation=False, pipeline_sync=pipeline_sync, **cfg)
    stats = new_stats()
    try:
        d.stream_upload(np.tile(np.asarray(x, np.complex64), (B, 1)))
        d.set_subchannels([sub_tuple(d, s) for s in subs])
        d.set_channel_ber(True)
        lists = [list(range(len(subs)))] * B; cif0 = [[0] * len(subs)] * B
        for _ in range((model.n_frames + F - 1) // F + 1):
            d.process(F)
            info = check_batch(d, model, lists, cif0, stats)
            if not (info["valid"] == 1).any():
                break
        stats["replayed"] = d.replayed_batches()
    finally:
        d.close()
    return stats


def check_streaming_small(d_factory, F, pipeline_sync):
    """B = 2, a mixed sub-channel list (EEP and UEP, six rates) near 6 dB: non-trivial counts everywhere"""
    st = run_stream(d_factory, mixed_stream(), F, B=2, pipeline_sync=pipeline_sync)
    n_subs = len(small_mixed_subchannels())
    assert st["fic"] >= 2 * 4 * 5 and st["rows"] >= 2 * n_subs * 4 and st["empty_rows"] >= 2 * n_subs * 16, st
    assert st["fic_errors"] > 0 and st["row_errors"] > 0, st
    return st


def check_replayed_batch(d_factory):
    """exact batch mode at 3.5 dB: a batch decoded twice is counted on its final bytes"""
    st = run_stream(d_factory, replay_stream(), 3, B=1)
    assert st["replayed"] >= 1, st
    assert st["fic"] >= 4 * 12 and st["rows"] >= 5 * 4 * 8 and st["row_errors"] > 0, st
    return st


def check_service_change(d_factory, F=2, add_step=2, remove_step=4, pipeline_sync=0):
    """ensemble 0 plays positions (0, 1), adds sub-channel 3 in front of step add_step and drops its first in front of step remove_step;
    ensemble 1 plays (2, 4) throughout.  The added service's rows start 16 CIFs after the addition; the others' counts stay the model's"""
    x, subs, model = mixed_stream(nf=13)
    d = d_factory(n_ensembles=2, max_frames=F, want_constellation=False, pipeline_sync=pipeline_sync)
    stats = new_stats(); added = {}
    try:
        d.stream_upload(np.tile(np.asarray(x, np.complex64), (2, 1)))
        lists = [[0, 1], [2, 4]]; cif0 = [[0, 0], [0, 0]]
        for b in range(2):
            d.set_subchannels_ensemble(b, [sub_tuple(d, subs[i]) for i in lists[b]])
        d.set_channel_ber(True)
        for step in range((model.n_frames + F - 1) // F):
            changed = False
            if step == add_step:
                lists[0] = [0, 1, 3]; changed = True
            if step == remove_step:
                lists[0] = [1, 3]; cif0[0] = cif0[0][1:]; changed = True
            if changed:
                d.set_subchannels_ensemble(0, [sub_tuple(d, subs[i]) for i in lists[0]])
                with np.testing.assert_raises(Exception):
                    d.channel_ber_fic()                          # a new list clears the results
            d.process(F)
            if step == add_step:
                added["cif"] = 4 * int(d.frame_info()[0, 0]["frame_no"]); cif0[0] = cif0[0] + [added["cif"]]
            info = check_batch(d, model, lists, cif0, stats)
            if step >= add_step:
                rows, fv, nr = d.channel_ber_ensemble(0, lists[0].index(3))
                c0 = 4 * int(info[0, 0]["frame_no"])
                assert fv == max(0, added["cif"] + 16 - c0), (step, fv, nr, c0, added)      # rows start 16 CIFs after the addition
                added.setdefault("rows", 0); added["rows"] += int((rows["compared"] > 0).sum())
            if not (info["valid"] == 1).any():
                break
    finally:
        d.close()
    assert added["cif"] > 0 and added["rows"] >= 8 and stats["rows"] >= 60, (added, stats)
    return stats


def sf_events(d, b, i, bitrate):
    ev, ne, _ = d.superframes_ensemble(b, i, bitrate)
    return ev[:ne].copy()


def check_off_means_off(d_factory, capi, F=2, n_steps=4):
    """the same short stream with the feature never switched on and with it on: FIBs, MSC bytes and superframe events are equal; the
    getters refuse while it is off, after a reset and after a new list"""
    x, subs, _ = mixed_stream()
    outs = []
    for on in (False, True):
        d = d_factory(n_ensembles=2, max_frames=F, want_constellation=False)
        log = []
        try:
            d.stream_upload(np.tile(np.asarray(x, np.complex64), (2, 1)))
            d.set_subchannels([sub_tuple(d, s) for s in subs])
            if on:
                d.set_channel_ber(True)
                with np.testing.assert_raises(capi.DabPhyError):
                    d.channel_ber_fic()                          # nothing counted yet
            for _ in range(n_steps):
                d.process(F)
                fib, ok = d.fibs()
                log.append((fib.copy(), ok.copy(), [d.msc(i)[0].copy() for i in range(len(subs))], d.superframes_stats().copy(),
                            [sf_events(d, 0, i, subs[i].bitrate) for i in (0, 2)]))
                if not on:
                    for call in (d.channel_ber_fic, d.channel_ber_totals, lambda: d.channel_ber_ensemble(0, 0)):
                        with np.testing.assert_raises(capi.DabPhyError):
                            call()
            if on:
                d.channel_ber_totals()
                d.set_channel_ber(False)
                with np.testing.assert_raises(capi.DabPhyError):
                    d.channel_ber_totals()
                d.set_channel_ber(True)
                d.process(F); d.channel_ber_totals()
                d.reset()
                with np.testing.assert_raises(capi.DabPhyError):
                    d.channel_ber_totals()
        finally:
            d.close()
        outs.append(log)
    for a, b in zip(*outs):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "FIBs differ with the feature on"
        assert all(np.array_equal(p, q) for p, q in zip(a[2], b[2])), "MSC bytes differ with the feature on"
        assert np.array_equal(a[3], b[3]) and all(np.array_equal(p, q) for p, q in zip(a[4], b[4])), "superframe events differ with the feature on"
