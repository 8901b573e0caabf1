"""The MP2 frame check through the whole receiver (dabphy_process -> class outputs -> k_mp2), shared by tests/test_emu_mp2.py and
tests/test_gpu_mp2.py.  The expected events are the model's (tests/mp2_model.py, pinned to the reference by tests/test_mp2_vs_ref.py)
fed with the logical frames the device decoded for the service (their equality with the reference's is the stream tests' business)."""
import numpy as np

import mp2_model as M
from welle_io_amd import capi, synth

# sub-channel id, bit rate, audio: (rate, mode, mode_ext) for MP2, None for DAB+
SERVICES = [(1, 64, (48000, "stereo", 0)), (2, 64, None), (3, 48, (24000, "mono", 0)), (4, 128, (48000, "joint", 1)), (5, 96, None)]


def ensemble(services=SERVICES, period=80, seed=3, damage=True):
    """sub-channels + payload_fn: MP2 frames / DAB+ superframes per service; the first MP2 service gets a CRC-covered bit flip, a broken
    sync word and a planted header (resync onto a false sync)"""
    subchs, fns, cu = [], {}, 0
    dab = synth.dabplus_payload_fn(period, seed)
    for sid, br, audio in services:
        sc = synth.SubchannelCfg(sid, cu, br, False, 3)
        subchs.append(sc); cu += sc.size_cu
        if audio:
            fns[sid] = synth.mp2_payload_fn(period, seed, rate=audio[0], mode=audio[1], mode_ext=audio[2])

    def payload(sc, r):
        if sc.subch_id not in fns:
            return dab(sc, r)
        data = bytearray(fns[sc.subch_id](sc, r))
        if damage and sc.subch_id == services[[s[2] is not None for s in services].index(True)][0]:
            q = r % period
            if q == 21: data[6] ^= 0x80
            if q == 27: data[1] ^= 0x40
            if q == 34: data[40:44] = data[0:4]; data[1] ^= 0x40
        return bytes(data)
    return subchs, payload


def check_unit_entry(d, cases):
    """dabphy_mp2_check on the cases (tests/mp2_cases.py), the streams of one frame length and count in one call, against the model;
    returns the number of frames the model claims"""
    groups = {}
    for name, s, fl in cases:
        groups.setdefault((fl, len(s) // fl), []).append((name, s))
    n_claimed = 0
    for (fl, nf), items in groups.items():
        frames = np.stack([np.frombuffer(s, np.uint8) for _, s in items])
        ev, ne, fe, fu = d.mp2_check(frames, fl)
        for k, (name, s) in enumerate(items):
            mev, merr, mfu, _ = M.run(s, fl)
            got = [(int(e["frame"]), int(e["offset"]), int(e["header"]), int(e["crc_ok"]), int(e["new_format"]), int(e["scf_crc_len"]),
                    int(e["fpad"][0]), int(e["fpad"][1])) for e in ev[k]]
            assert int(fu[k]) == mfu, name
            assert got == mev, name
            assert list(fe[k]) == merr, name
            n_claimed += len(mev)
    return n_claimed


class ServiceCheck:
    """the model of one (ensemble, position) and the device's events of it, batch after batch"""

    def __init__(self):
        self.m = M.Mp2Model()
        self.got, self.got_err = [], []
        self.fu_dev = -1

    def batch(self, rows, fv, ev, n, fe, fu):
        base = self.m.feed_no + 1
        for row in rows:
            self.m.feed(row.tobytes())
        assert n == len(ev), "events beyond what is kept"
        for e in ev:
            self.got.append((base + int(e["frame"]) - fv, int(e["offset"]), int(e["header"]), int(e["crc_ok"]), int(e["new_format"]),
                             int(e["scf_crc_len"]), int(e["fpad"][0]), int(e["fpad"][1])))
        self.got_err += [int(v) for v in fe[fv:fv + len(rows)]]
        if fu >= 0 and self.fu_dev < 0:
            self.fu_dev = base + fu - fv

    def verify(self):
        fu = self.m.first_unverified
        assert self.fu_dev == fu, (self.fu_dev, fu)
        assert self.got == self.m.events, "MP2 events differ"
        assert self.got_err == self.m.errors
        return self.m


def run(factory, F=3, nf=15, B=2, snr_db=6.0, seed=3, cfo=20, kinds=None, auto_mp2=True, switch=None, services=SERVICES, damage=True, stats=None,
        sf_auto=True, sf_positions=None, **cfg):
    """kinds[b] = per-position kinds of ensemble b (None: every position as its audio is; only ensemble 0 in mixed form when B > 1);
    switch = (batch, ensemble, position): that position becomes MP2 in front of that batch; sf_positions[b] = positions whose DAB+ filter
    is run one service at a time (dabphy_superframes_ensemble; with sf_auto off) and summed into the DAB+ totals.
    Returns (per-service checks, DAB+ totals, MP2 totals)"""
    subchs, payload = ensemble(services, seed=seed, damage=damage)
    x = synth.make_stream(nf, snr_db=snr_db, cfo_hz=cfo, delay=50, seed=seed, payload_fn=payload, subchs=subchs)
    natural = [capi.AUDIO_MP2 if s[2] else capi.AUDIO_DABPLUS for s in services]
    if kinds is None:
        kinds = [natural] + [[capi.AUDIO_MP2 if i == 0 else capi.AUDIO_DABPLUS for i in range(len(services))] for _ in range(B - 1)]
    kinds = [list(k) for k in kinds]
    d = factory(n_ensembles=B, max_frames=F, want_constellation=False, **cfg)
    checks = {}
    sf_tot = np.zeros((B, 4), np.int64); mp2_tot = np.zeros((B, 4), np.int64)
    try:
        d.stream_upload(np.tile(np.asarray(x, np.complex64), (B, 1)))
        d.set_subchannels([(s.subch_id, s.start_cu, s.size_cu, d.protection_eep(s.bitrate, s.profile_b, s.level)) for s in subchs])
        if switch is not None:
            kinds[switch[1]][switch[2]] = capi.AUDIO_DABPLUS
        for b in range(B):
            if any(kinds[b]):
                d.set_audio_kinds_ensemble(b, kinds[b])
        d.set_auto_mp2(auto_mp2)
        d.set_auto_superframes(sf_auto)
        for k in range((nf + F - 1) // F):
            if switch is not None and k == switch[0]:
                kinds[switch[1]][switch[2]] = capi.AUDIO_MP2
                d.set_audio_kinds_ensemble(switch[1], kinds[switch[1]])
            d.process(F)
            if not (d.frame_info()["valid"] == 1).any():
                break
            if sf_auto:
                sf_tot += d.superframes_stats()
            for b, positions in enumerate(sf_positions or []):
                for i in positions:
                    ev, ne, _ = d.superframes_ensemble(b, i, services[i][1])
                    for e in ev[:ne]:
                        sf_tot[b] += (int(e["sync"]), int(e["corrected"]), int(e["uncorrectable"]),
                                      int(e["num_aus"]) - bin(int(e["au_crc_ok"])).count("1") if e["sync"] else 0)
            if not any(any(kk) for kk in kinds):
                continue
            mp2_tot += d.mp2_stats()
            for i in range(len(services)):
                if not any(kinds[b][i] for b in range(B)):
                    continue
                out, fv = d.msc(i)
                for b in range(B):
                    if kinds[b][i] != capi.AUDIO_MP2:
                        continue
                    ev, n, fe, fu = d.mp2_frames_ensemble(b, i)
                    checks.setdefault((b, i), ServiceCheck()).batch(out[b, fv[b]:d.msc_rows[b]], int(fv[b]), ev, n, fe, fu)
        if stats is not None:
            stats["replayed"] = d.replayed_batches()
    finally:
        d.close()
    for c in checks.values():
        c.verify()
    for b in range(B):          # the totals are the per-service results' sums
        mine = [c.m for (bb, i), c in checks.items() if bb == b]
        want = (sum(len(m.events) for m in mine), sum(sum(m.errors) for m in mine), sum(m.skipped for m in mine),
                sum(m.feed_no + 1 - m.first_unverified for m in mine if m.first_unverified >= 0))
        assert tuple(mp2_tot[b]) == want, (b, tuple(mp2_tot[b]), want)
    return checks, sf_tot, mp2_tot
