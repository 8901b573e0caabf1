"""Cases of the bulk access-unit drain (dabphy_set_au_drain / dabphy_au_drain_*, k_au.hip), shared by the execution-model suite
(tests/test_emu_au_drain.py) and the device suite (tests/test_gpu_au_drain.py).  Expected output is always tests/au_model.py on the
ORACLE's filter events and corrected superframes."""
import numpy as np

import au_model as M
import mp2_chain
import parity_cases as P
import refapi as R
import sf_cases as S
from welle_io_amd import capi, synth

FORMATS = (capi.AU_RAW, capi.AU_LOAS)
# (layout, bit rate, access-unit lengths): stripped lengths 0, 255, 510 and 765 (a multiple of 255 ends PayloadLengthInfo with a zero
# byte), an access unit of one byte (it fails its CRC and is skipped), both LOAS shifts (5 bits without SBR, 6 with)
UNIT_SUPERFRAMES = (((0, 1), 48, (257, None)), ((1, 1), 72, (512, 2, None)), ((0, 0), 136, (2, 257, 767, None)),
                    ((1, 0), 384, (None, 2, 1, 512, 257, None)), ((0, 1), 8, None))


def filter_of(superframes, bitrate):
    """the oracle's filter over superframes fed as logical frames -> (events, corrected superframes of the synchronised ones)"""
    fb = 3 * bitrate
    frames = np.concatenate([np.asarray(sf, np.uint8).reshape(5, fb) for sf in superframes])
    return R.orc_superframe_run(frames)


def check_pack(d, superframes, bitrate, fmt):
    """dabphy_test_au_pack on the oracle's events of `superframes` against the model; returns the model's access units"""
    eo, so = filter_of(superframes, bitrate)
    assert len(so) == len(superframes), "a superframe of the case did not synchronise"
    aus, raw, loas, failed = M.model(eo, so)
    want = raw if fmt == capi.AU_RAW else loas
    out, recs, svc = d.test_au_pack(np.array(so), M.events_array(eo), bitrate // 8, fmt)
    assert (int(svc["n_superframes"]), int(svc["n_aus"]), int(svc["n_failed"]), int(svc["bytes"])) == (len(so), len(aus), failed, len(want)), (svc, len(aus), failed, len(want))
    assert out[:len(want)].tobytes() == want, "packed bytes differ from the model"
    assert not out[len(want):].any(), "bytes behind the service's extent are not zero"
    at = 0
    for r, a in zip(recs, aus):
        ln = len(a[4]) if fmt == capi.AU_RAW else len(M.loas_frame(a[4], a[3]))
        assert (int(r["cif"]), int(r["au_index"]), int(r["format"]), int(r["length"]), int(r["offset"])) == (a[1], a[2], a[3], ln, at), (r, a[:4], at)
        at += ln
    return aus


def check_unit_corners(d, fmt, seed=3):
    """the named superframes, one call each and all of one bit rate in one call"""
    rng = np.random.RandomState(seed)
    lens = set()
    for layout, br, au_lengths in UNIT_SUPERFRAMES:
        for flags in (0x00, 0x10):
            sfs = [S.make_superframe(br, rng, layout, flags, au_lengths) for _ in range(2)]
            lens |= {len(a[4]) for a in check_pack(d, sfs, br, fmt)}
    assert {0, 255, 510, 765} <= lens, sorted(lens)


def check_unit_sweep(d, fmt, seed=4):
    """stripped lengths 0 .. 40 of the second access unit while the first one's length walks the source and the destination through every
    residue mod 16 (counted on the inputs: the start table and the model's offsets)"""
    rng = np.random.RandomState(seed)
    for layout in ((0, 0), (0, 1)):                                      # no SBR (shift 5), SBR (shift 6)
        n_au = S.LAYOUTS[layout][0]
        sfs = [S.make_superframe(24, rng, layout, 0x10 * (n & 1), (3 + (7 * n) % 23, n + 2) + (None,) * (n_au - 2) if n_au > 2 else (330 - 5 - (n + 2), n + 2)) for n in range(41)]
        aus = check_pack(d, sfs, 24, fmt)
        assert {len(a[4]) for a in aus} >= set(range(41))
        eo, _ = filter_of(sfs, 24)
        src = {(k * 360 + st) % 16 for k, e in enumerate(e for e in eo if e[3]) for st in e[6][:-1]}
        dst, at = set(), 0
        for a in aus:
            dst.add(at % 16); at += len(a[4]) if fmt == capi.AU_RAW else len(M.loas_frame(a[4], a[3]))
        assert src == set(range(16)) and dst == set(range(16)), (sorted(src), sorted(dst))


def check_unit_capacity(d, fmt, seed=6):
    """a reservation too small for the service, and a record table too small: the first access unit that does not fit is left out with
    everything behind it -- what is stored is a whole-unit prefix of the model, in one piece, and the record counts exactly that"""
    rng = np.random.RandomState(seed)
    sfs = [S.make_superframe(40, rng, (1, 0), 0x10, (None, 2, 40, None, None, None)) for _ in range(3)]
    eo, so = filter_of(sfs, 40)
    aus = M.model(eo, so)[0]
    lens = [len(a[4]) if fmt == capi.AU_RAW else len(M.loas_frame(a[4], a[3])) for a in aus]
    full = M.stream_of(aus, fmt)
    ends = np.cumsum(lens)
    for cap in (0, lens[0] - 1, lens[0], int(ends[6]) + 1, int(ends[-1]) - 1, int(ends[-1])):
        out, recs, svc = d.test_au_pack(np.array(so), M.events_array(eo), 5, fmt, out_capacity=cap)
        # (a later, shorter unit that would fit behind a unit that does not is left out too: the extent has no holes)
        k = next((i for i in range(len(lens)) if ends[i] > cap), len(lens))
        want = full[:int(ends[k - 1])] if k else b""
        assert (int(svc["n_aus"]), int(svc["bytes"]), len(recs)) == (k, len(want), k), (cap, svc, k)
        assert out[:len(want)].tobytes() == want and not out[len(want):].any() and len(out) == cap
        assert int(svc["n_superframes"]) == len(so)
    # ... and the record table: aus_capacity = 6 * n_sf in the binding, so hand in fewer superframes' worth of records
    out = np.zeros(int(ends[-1]), np.uint8); tab = np.zeros(4, capi.AU_DESC_DTYPE); svc = np.zeros(1, capi.AU_SERVICE_DTYPE)
    sfa = np.ascontiguousarray(np.array(so), np.uint8); ev = M.events_array(eo)
    d._chk(d.lib.dabphy_test_au_pack(d.h, capi._p(sfa), capi._p(ev), capi.C.c_uint32(len(ev)), capi.C.c_uint32(len(so)), capi.C.c_uint32(5), capi.C.c_int32(int(fmt)),
                                     capi._p(out), capi.C.c_size_t(out.nbytes), capi._p(tab), capi.C.c_uint32(len(tab)), capi._p(svc)))
    assert int(svc[0]["n_aus"]) == 4 and int(svc[0]["bytes"]) == int(ends[3]) and out[:int(ends[3])].tobytes() == full[:int(ends[3])] and not out[int(ends[3]):].any()


# ---- through the stream
def drain_run(d, F, nf, mode, aus=True, on_batch=None):
    """process the bound stream in batches of F with the filter in `mode` (0: dabphy_superframes_stats runs it) and drain every pass ->
    list of (stats of the pass, buf, services, aus) per drained pass.  on_batch(k): called in front of batch k"""
    out = []

    def drain(st):
        try:
            buf, svc, tab = d.au_batch(aus=aus)
        except capi.DabPhyError as e:
            assert "status -5" in str(e), e                               # no pass yet (mode 2 after the first batch)
            return
        out.append((st.copy(), buf.copy(), svc.copy(), None if tab is None else tab.copy()))
    for k in range((nf + F - 1) // F):
        if on_batch:
            on_batch(k)
        d.process(F)
        if not (d.frame_info()["valid"] == 1).any():
            break
        drain(d.superframes_stats())
    if mode == 2:
        drain(d.superframes_stats())                                      # the end of the stream: the waiting pass runs now
    return out


def service_streams(passes):
    """{(ensemble, subch_id): concatenation over the passes of buf[offset : offset + bytes]}"""
    got = {}
    for _, buf, svc, _ in passes:
        for s in svc:
            got.setdefault((int(s["ensemble"]), int(s["subch_id"])), []).append(buf[int(s["offset"]):int(s["offset"]) + int(s["bytes"])].tobytes())
    return {k: b"".join(v) for k, v in got.items()}


def oracle_services(x, subs):
    """{subch_id: (events, access units of the model)} from the oracle receiver and its filter"""
    o = R.orc_receiver_run(x, subchs=subs)
    want = {}
    for i, sc in enumerate(subs):
        fb = 3 * sc.bitrate
        frames = np.frombuffer(bytes(o["msc"][i]), np.uint8)
        frames = frames[:len(frames) // fb * fb].reshape(-1, fb)
        eo, so = R.orc_superframe_run(frames)
        want[sc.subch_id] = (eo, M.model(eo, so)[0])
    return want


def assert_prefix(got, want, fmt, what, slack=4):
    """got = a service's drained stream; want = (oracle events, model access units): a prefix that may fall short of the oracle's
    events by at most `slack`"""
    eo, aus = want
    full = M.stream_of(aus, fmt)
    assert got == full[:len(got)], "%s: drained stream differs from the model" % (what,)
    need = M.stream_of([a for a in aus if a[0] < len(eo) - slack], fmt)
    assert len(got) >= len(need), "%s: %d bytes drained, the events up to the allowance hold %d" % (what, len(got), len(need))


def check_tables(passes, B, fmt, n_dabplus):
    for st, buf, svc, tab in passes:
        assert len(svc) == n_dabplus
        order = [(int(s["ensemble"]), int(s["subch_index"])) for s in svc]
        assert order == sorted(order)
        for b in range(B):
            mine = svc[svc["ensemble"] == b]
            assert int(mine["n_superframes"].sum()) == st[b][0] and int(mine["n_failed"].sum()) == st[b][3], (b, st[b], mine)
        for s in svc:
            if not s["n_superframes"]:
                assert s["n_aus"] == 0 and s["bytes"] == 0
            if tab is not None:
                r = tab[int(s["first_au"]):int(s["first_au"]) + int(s["n_aus"])]
                at = int(s["offset"])
                for a in r:                                               # offsets and lengths tile the service's extent without gaps
                    assert int(a["offset"]) == at, (s, a)
                    at += int(a["length"])
                assert at == int(s["offset"]) + int(s["bytes"])


def layouts_stream(nf=22, seed=12, snr_db=5.0, rates=P.LAYOUT_RATES):
    """the ensemble and payload of parity_cases.check_superframe_layouts"""
    subchs, cu = [], 0
    for i, br in enumerate(rates):
        sc = synth.SubchannelCfg(i + 1, cu, br, False, 3); subchs.append(sc); cu += sc.size_cu
    x, tx = synth.make_stream(nf, snr_db=snr_db, cfo_hz=20, delay=50, return_tx=True, seed=seed, payload_fn=S.payload_fn(80, seed), subchs=subchs)
    return np.asarray(x, np.complex64), list(tx.subchs)


_shared = {}


def layouts_reference():
    """(stream, sub-channels, oracle services): computed once, shared by the cases, never changed"""
    if "layouts" not in _shared:
        x, subs = layouts_stream()
        want = oracle_services(x, subs)
        for sid, (eo, aus) in want.items():                              # asserted on the oracle's output, before anything is compared
            assert len(eo) > 4 and any(a[0] < len(eo) - 4 for a in aus), "service %d: the stream holds too little" % sid
        _shared["layouts"] = (x, subs, want)
    return _shared["layouts"]


def open_stream(d_factory, x, subs, B, F, mode, fmt, **kw):
    d = d_factory(n_ensembles=B, max_frames=F, want_constellation=False, **kw)
    d.stream_upload(np.tile(x, (B, 1)))
    d.set_subchannels([(s.subch_id, s.start_cu, s.size_cu, d.protection_eep(s.bitrate, s.profile_b, s.level)) for s in subs])
    d.set_auto_superframes(mode)
    d.set_au_drain(fmt)
    return d


def check_stream(d_factory, F, mode, fmt, nf=22, B=2):
    x, subs, want = layouts_reference()
    d = open_stream(d_factory, x, subs, B, F, mode, fmt)
    try:
        passes = drain_run(d, F, nf, mode)
    finally:
        d.close()
    check_tables(passes, B, fmt, B * len(subs))
    got = service_streams(passes)
    for b in range(B):
        for sc in subs:
            assert_prefix(got[(b, sc.subch_id)], want[sc.subch_id], fmt, "ensemble %d service %d" % (b, sc.subch_id))
    # the same run without the access-unit table gives the same bytes
    d = open_stream(d_factory, x, subs, B, F, mode, fmt)
    try:
        again = drain_run(d, F, nf, mode, aus=None)
    finally:
        d.close()
    assert len(again) == len(passes) and all(a[3] is None and np.array_equal(a[1], p[1]) and np.array_equal(a[2], p[2]) for a, p in zip(again, passes))


def check_mp2_beside_dabplus(d_factory, fmt, F=3, nf=14):
    """MP2 positions have no service record; the DAB+ services beside them equal the model"""
    kinds = [1, 0, 1, 0, 0]                                              # (position 3 carries MP2 frames and is filtered as DAB+: a service that never synchronises)
    subs, payload = mp2_chain.ensemble()
    x = np.asarray(synth.make_stream(nf, snr_db=25, cfo_hz=20, delay=50, seed=5, payload_fn=payload, subchs=subs), np.complex64)
    dab = [s for s, k in zip(subs, kinds) if k == 0]
    want = oracle_services(x, dab)
    d = d_factory(n_ensembles=1, max_frames=F, want_constellation=False)
    try:
        d.stream_upload(x[None])
        d.set_subchannels([(s.subch_id, s.start_cu, s.size_cu, d.protection_eep(s.bitrate, s.profile_b, s.level)) for s in subs])
        d.set_audio_kinds_ensemble(0, kinds)
        d.set_auto_superframes(1); d.set_au_drain(fmt)
        passes = drain_run(d, F, nf, 1)
    finally:
        d.close()
    check_tables(passes, 1, fmt, len(dab))
    assert [int(s["subch_index"]) for s in passes[0][2]] == [i for i, s in enumerate(subs) if s in dab]
    got = service_streams(passes)
    assert set(got) == {(0, s.subch_id) for s in dab}
    assert sum(1 for s in dab if want[s.subch_id][1]) >= 2
    for s in dab:
        assert_prefix(got[(0, s.subch_id)], want[s.subch_id], fmt, "service %d" % s.subch_id)


def check_two_lists(d_factory, fmt, F=3, nf=22):
    """two ensembles with different lists and classes: records carry the right ensemble, position and SubChId"""
    x, subs, want = layouts_reference()
    lists = [[subs[1], subs[3], subs[0]], [subs[2], subs[1]]]
    d = d_factory(n_ensembles=2, max_frames=F, want_constellation=False)
    try:
        d.stream_upload(np.tile(x, (2, 1)))
        for b, ls in enumerate(lists):
            d.set_subchannels_ensemble(b, [(s.subch_id, s.start_cu, s.size_cu, d.protection_eep(s.bitrate, s.profile_b, s.level)) for s in ls])
        d.set_auto_superframes(1); d.set_au_drain(fmt)
        passes = drain_run(d, F, nf, 1)
    finally:
        d.close()
    for _, _, svc, _ in passes:
        assert [(int(s["ensemble"]), int(s["subch_index"]), int(s["subch_id"])) for s in svc] == [(b, i, s.subch_id) for b, ls in enumerate(lists) for i, s in enumerate(ls)]
    check_tables(passes, 2, fmt, 5)
    got = service_streams(passes)
    for b, ls in enumerate(lists):
        for s in ls:
            assert_prefix(got[(b, s.subch_id)], want[s.subch_id], fmt, "ensemble %d service %d" % (b, s.subch_id))


def check_list_change(d_factory, fmt, F=3, nf=22, change_at=3):
    """mode 2: the drain after the dabphy_process that applied a new list returns the batch BEFORE it, under the old list, and the services
    that stay give the bytes of the uninterrupted run"""
    x, subs, want = layouts_reference()
    old, new = [subs[0], subs[1], subs[2]], [subs[1], subs[2], subs[4]]
    runs = []
    for change in (False, True):
        d = open_stream(d_factory, x, old, 1, F, 2, fmt)
        try:
            def on_batch(k, d=d):
                if change and k == change_at:
                    d.set_subchannels_ensemble(0, [(s.subch_id, s.start_cu, s.size_cu, d.protection_eep(s.bitrate, s.profile_b, s.level)) for s in new])
            runs.append(drain_run(d, F, nf, 2, on_batch=on_batch))
        finally:
            d.close()
    plain, changed = runs
    # pass k is drained behind dabphy_process(k + 1): the one behind the process that applied the new list is batch change_at - 1, old list
    assert [int(s["subch_id"]) for s in changed[change_at - 1][2]] == [s.subch_id for s in old]
    assert [int(s["subch_id"]) for s in changed[change_at][2]] == [s.subch_id for s in new]
    a, b = service_streams(plain), service_streams(changed)
    for s in (subs[1], subs[2]):
        assert len(b[(0, s.subch_id)]) > 0 and b[(0, s.subch_id)] == a[(0, s.subch_id)], "service %d" % s.subch_id
        assert_prefix(b[(0, s.subch_id)], want[s.subch_id], fmt, "service %d" % s.subch_id)


def check_replay(d_factory, fmt, mode=1):
    """the stream of test_superframes_through_a_replayed_batch: behind a batch that was decoded twice the drained stream equals the model,
    every access unit exactly once.  (At 3.5 dB this stream synchronises superframes but every access unit of them fails its CRC, on all
    18 sub-channels: what the case pins is that the second pass overwrites the first -- counts equal the pass's totals, superframes and
    failed access units are not counted twice against the oracle -- and that nothing is stored.)"""
    F, nf, seed = 3, 22, 10
    x, tx = synth.make_stream(nf, snr_db=3.5, cfo_hz=40, delay=50, return_tx=True, seed=seed, payload_fn=P.damaged_dabplus_payload(seed, True, (6, 8)))
    x = np.asarray(x, np.complex64)
    subs = [tx.subchs[i] for i in (1, 6)]
    want = oracle_services(x, subs)
    d = open_stream(d_factory, x, subs, 1, F, mode, fmt)
    try:
        passes = drain_run(d, F, nf, mode)
        assert d.replayed_batches() >= 1
    finally:
        d.close()
    check_tables(passes, 1, fmt, len(subs))
    got = service_streams(passes)
    for s in subs:
        eo, aus = want[s.subch_id]
        assert sum(e[3] for e in eo) >= 2 and not aus               # (said out loud: this stream stores nothing; check_replay_storing is the one that does)
        assert_prefix(got[(0, s.subch_id)], want[s.subch_id], fmt, "service %d" % s.subch_id)
        n_sf = sum(int(p[2][p[2]["subch_id"] == s.subch_id]["n_superframes"][0]) for p in passes)
        n_bad = sum(int(p[2][p[2]["subch_id"] == s.subch_id]["n_failed"][0]) for p in passes)
        assert sum(e[3] for e in eo[:len(eo) - 4]) <= n_sf <= sum(e[3] for e in eo), (n_sf, eo)
        assert n_bad <= sum(e[5] - bin(e[7]).count("1") for e in eo if e[3])


def check_replay_storing(d_factory, fmt, mode=1):
    """the same 3.5 dB channel (seed 10, F = 3, nf = 22, cfo 40) over an ensemble with two services at EEP 2-A beside two at 3-A: a
    batch is still decoded twice, and the better-protected services' superframes survive Reed-Solomon with access units that pass
    their CRC -- behind the replayed batch every one of them is in the drained stream exactly once (a prefix of the model's stream: a
    unit stored by both passes would break it), asserted on the ORACLE to be more than a handful"""
    F, nf, seed = 3, 22, 10
    subchs, cu = [], 0
    for i, (br, lvl) in enumerate([(64, 3), (32, 2), (64, 3), (48, 2)]):
        sc = synth.SubchannelCfg(i + 1, cu, br, False, lvl); subchs.append(sc); cu += sc.size_cu
    x, tx = synth.make_stream(nf, snr_db=3.5, cfo_hz=40, delay=50, return_tx=True, seed=seed, payload_fn=P.damaged_dabplus_payload(seed, True, (6, 8)), subchs=subchs)
    x = np.asarray(x, np.complex64); subs = list(tx.subchs)
    want = oracle_services(x, subs)
    assert all(sum(1 for a in want[s.subch_id][1] if a[0] < len(want[s.subch_id][0]) - 4) >= 6 for s in (subs[1], subs[3])), "the stream stores too little"      # (two whole superframes of three units, in different batches, inside the allowance)
    d = open_stream(d_factory, x, subs, 1, F, mode, fmt)
    try:
        passes = drain_run(d, F, nf, mode)
        assert d.replayed_batches() >= 1
    finally:
        d.close()
    check_tables(passes, 1, fmt, len(subs))
    got = service_streams(passes)
    for s in subs:
        assert_prefix(got[(0, s.subch_id)], want[s.subch_id], fmt, "service %d" % s.subch_id)
        n = sum(int(p[2][p[2]["subch_id"] == s.subch_id]["n_aus"][0]) for p in passes)
        assert n <= len(want[s.subch_id][1])


def check_protocol(d_factory, fmt, F=3, nf=12):
    """begin -> process -> wait gives the bytes of the blocking call; a second begin on the same pass: ERR_STATE; capacities one short:
    ERR_INVALID, nothing written; an MSC drain and an access-unit drain in flight together both arrive intact"""
    x, subs, _ = layouts_reference()
    subs = subs[:4]
    blocking = []
    d = open_stream(d_factory, x, subs, 2, F, 1, fmt)
    try:
        for _ in range(nf // F):
            d.process(F)
            blocking.append((d.au_batch(), d.msc_batch()))
    finally:
        d.close()

    def status(fn):
        try:
            fn()
        except capi.DabPhyError as e:
            return int(str(e).split()[1].rstrip(":"))
        return 0
    d = open_stream(d_factory, x, subs, 2, F, 1, fmt)
    try:
        # before any pass has run with the drain on: the entry itself refuses, and so does the size query
        spare = (np.full(64, 0x5A, np.uint8), np.zeros(8, capi.AU_SERVICE_DTYPE), np.zeros(8, capi.AU_DESC_DTYPE))
        assert status(lambda: d.au_drain_begin(*spare)) == -5 and status(d.au_batch_size) == -5 and (spare[0] == 0x5A).all()
        flight = None
        for k in range(nf // F):
            d.process(F)
            if flight:
                (buf, svc, tab), (mbuf, mdesc) = d.au_drain_wait(), flight[1]
                d.msc_drain_wait()
                (wb, ws, wt), (wm, wd) = blocking[k - 1]
                assert np.array_equal(buf, wb) and np.array_equal(svc, ws) and np.array_equal(mbuf, wm) and np.array_equal(mdesc, wd)
                for s in svc:
                    r = slice(int(s["first_au"]), int(s["first_au"]) + int(s["n_aus"]))
                    assert np.array_equal(tab[r], wt[r])
            nb, ns, na = d.au_batch_size()
            assert ns == 2 * len(subs) and nb > 0 and na > 0
            canary = np.full(nb, 0x5A, np.uint8)
            for kw in (dict(buf=canary[:nb - 1]), dict(buf=canary, services=np.zeros(ns - 1, capi.AU_SERVICE_DTYPE)), dict(buf=canary, aus=np.zeros(na - 1, capi.AU_DESC_DTYPE))):
                assert status(lambda: d.au_drain_begin(**kw)) == -2
            assert (canary == 0x5A).all()
            flight = (d.au_drain_begin(), d.msc_drain_begin())          # both in flight across the next process
            # one drain per pass: the ENTRY refuses (arrays of the right size handed in: no size query stands in front of it), nothing is queued
            spare = (np.full(nb, 0x5A, np.uint8), np.zeros(ns, capi.AU_SERVICE_DTYPE), np.zeros(na, capi.AU_DESC_DTYPE))
            assert status(lambda: d.au_drain_begin(*spare)) == -5
            assert (spare[0] == 0x5A).all() and not spare[1].view(np.uint8).any() and not spare[2].view(np.uint8).any()
            assert d.au_batch_size() == (nb, ns, na)                     # (the size query describes the pass queued last, drained or not)
        d.au_drain_wait(); d.msc_drain_wait()
        (buf, svc, tab), (mbuf, mdesc) = flight
        assert np.array_equal(buf, blocking[-1][0][0]) and np.array_equal(mbuf, blocking[-1][1][0])
        d.set_au_drain(capi.AU_OFF)
        d.process(F)
        assert status(d.au_batch_size) == -5
    finally:
        d.close()
