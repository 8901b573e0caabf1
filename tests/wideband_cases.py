"""Checks of the wideband front end (dabphy_stream_open_wideband / _write_wideband[_async]), shared by the execution-model suite
(tests/test_emu_wideband.py) and the device suite (tests/test_gpu_wideband.py): each takes a handle factory, as parity_cases.py does.
The library is compared with the float64 model of tests/wideband_model.py under the accuracy condition stated there -- the emulator
and the device each against the model, never against each other."""
import ctypes as C

import numpy as np

import refapi as R
import wideband_model as M
from welle_io_amd import capi, synth, wideband

T_F = 196608
RING_MIN = 4 * T_F                      # dabphy_stream_open's shortest ring
FORMATS = ("cf32", "u8", "s8", "s16le", "s16be")
SHAPES = ((1, 1), (1, 3), (2, 32), (2, 7), (4, 64), (16, 256), (32, 1024), (32, 37))      # (D, n_taps)
ERR_INVALID, ERR_STATE = -2, -5


def filter_offsets(D):
    return [0, 64 * D, -(64 * D - 1)]


def random_taps(n_taps, rng):
    """real taps with no structure a mistake could hide behind (no symmetry, no zeros), sum |taps| about 1"""
    t = rng.standard_normal(n_taps)
    t[np.abs(t) < 0.05] = 0.05
    return (t / np.abs(t).sum()).astype(np.float32)


def filter_case(D, n_taps, fmt, seed=0):
    """-> (raw capture of 4 096 D + 3 D samples, taps, offsets): the same for every check that names the same shape"""
    rng = np.random.RandomState(1000 * D + n_taps + seed)
    return M.random_capture(4096 * D + 3 * D, fmt, rng), random_taps(n_taps, rng), filter_offsets(D)


def assert_meets_model(got, x, taps, offset, D, first=0, what=""):
    """got: the library's outputs [first, first + len(got)) of a stream whose whole converted capture is x"""
    y, bound = M.channelise(x, taps, offset, D)
    y, bound = y[first:first + len(got)], bound[first:first + len(got)]
    assert len(y) == len(got), (len(y), len(got))
    err = np.abs(got.astype(np.complex128) - y)
    worst = int(np.argmax(err - bound))
    print("%s offset %d: max |y - model| / bound = %.3f (output %d), max |model| / bound = %.3g"
          % (what, offset, float((err / np.maximum(bound, 1e-300)).max()), first + worst, float(np.abs(y).max() / bound.max())))
    assert np.all(err <= bound), "%s offset %d: output %d is off by %g, bound %g" % (what, offset, first + worst, err[worst], bound[worst])
    assert np.abs(y).max() > 100 * bound.max()           # (the condition is tight: a wrong sample fails it by orders of magnitude)


def read_all(d, n_out, first=0):
    return [d.stream_read(e, first, n_out) for e in range(d.cfg.n_ensembles)]


def check_filter_vs_model(d_factory, D, n_taps, fmt):
    raw, taps, offsets = filter_case(D, n_taps, fmt)
    x = M.convert(raw, fmt)
    d = d_factory(n_ensembles=3, max_frames=1, want_constellation=False)
    try:
        d.stream_open_wideband(RING_MIN, D, taps, offsets, fmt)
        d.stream_write_wideband(raw)
        for e, got in enumerate(read_all(d, len(raw) // D)):
            assert_meets_model(got, x, taps, offsets[e], D, what="D %d, %d taps, %s," % (D, n_taps, fmt))
    finally:
        d.close()


def check_chunking(d_factory, D=4, n_taps=64, fmt="u8"):
    """one piece; pieces of D samples (shorter than the filter); 60, 4, 1 000 and the rest; two asynchronous writes with commits"""
    raw, taps, offsets = filter_case(D, n_taps, fmt)
    n = len(raw)

    def pieces_of(sizes):
        cuts = np.cumsum([0] + list(sizes)); assert cuts[-1] <= n
        return [raw[a:b] for a, b in zip(cuts[:-1], cuts[1:])] + ([raw[cuts[-1]:]] if cuts[-1] < n else [])
    ways = {"one piece": [raw], "pieces of D": pieces_of([D] * (n // D)), "60, 4, 1000, rest": pieces_of([60, 4, 1000]), "async": pieces_of([n // (2 * D) * D])}
    out = {}
    for name, pieces in ways.items():
        assert sum(len(p) for p in pieces) == n
        d = d_factory(n_ensembles=3, max_frames=1, want_constellation=False)
        try:
            d.stream_open_wideband(RING_MIN, D, taps, offsets, fmt)
            hold = []
            for p in pieces:
                if name == "async":
                    hold.append(np.ascontiguousarray(p).copy())            # (each piece its own host buffer, alive to the end)
                    d.stream_write_wideband_async(hold[-1]); d.stream_commit()
                else:
                    d.stream_write_wideband(p)
            out[name] = read_all(d, n // D)
        finally:
            d.close()
    for name in ways:
        for e in range(3):
            assert np.array_equal(out[name][e].view(np.uint32), out["one piece"][e].view(np.uint32)), "%s: ensemble %d differs from one piece" % (name, e)
    # the head of the stream, where the filter still looks at x[i < 0] = 0 (and everything behind it)
    x = M.convert(raw, fmt)
    for e in range(3):
        assert_meets_model(out["pieces of D"][e], x, taps, offsets[e], D, what="chunked,")
        assert np.any(out["one piece"][e][:n_taps // D] != 0)


def check_phase_long_run(d_factory, D=2, n_taps=8, offset=53):
    """the absolute capture index modulo P = 128 D across calls, and beyond 2^16"""
    rng = np.random.RandomState(7)
    n1, n2 = 128 * D * 40 + 2 * D, 128 * D * 300 + 6 * D
    raw = M.random_capture(n1 + n2, "u8", rng); taps = random_taps(n_taps, rng)
    assert n1 % (128 * D) != 0 and n1 + n2 > 1 << 16
    d = d_factory(n_ensembles=1, max_frames=1, want_constellation=False)
    try:
        d.stream_open_wideband(RING_MIN, D, taps, [offset], "u8")
        d.stream_write_wideband(raw[:n1]); d.stream_write_wideband(raw[n1:])
        assert_meets_model(d.stream_read(0, 0, (n1 + n2) // D), M.convert(raw, "u8"), taps, offset, D, what="two writes,")
    finally:
        d.close()


def check_ring_wrap(d_factory, D=1, n_taps=3):
    """the shortest ring; ring - 100 samples, then 300: the second write wraps"""
    rng = np.random.RandomState(11)
    ring = RING_MIN
    raw = M.random_capture((ring + 200) * D, "u8", rng); taps = random_taps(n_taps, rng); offset = -17
    d = d_factory(n_ensembles=1, max_frames=1, want_constellation=False)
    try:
        d.stream_open_wideband(ring, D, taps, [offset], "u8")
        d.stream_write_wideband(raw[:(ring - 100) * D]); d.stream_write_wideband(raw[(ring - 100) * D:])
        x = M.convert(raw, "u8")
        # samples [200, ring + 200) are in the ring now: the end of the first write, the wrap, the head of the ring written over
        assert_meets_model(d.stream_read(0, ring - 4000, 4200), x, taps, offset, D, first=ring - 4000, what="across the wrap,")
        assert_meets_model(d.stream_read(0, 200, 4000), x, taps, offset, D, first=200, what="behind the samples written over,")
        assert np.array_equal(d.stream_read(0, ring, 200), d.stream_read(0, 0, 200))
    finally:
        d.close()


def check_reset(d_factory, D=4, n_taps=64):
    """dabphy_reset: carry cleared, capture index 0, configuration kept -- the same capture gives the bits a fresh open gives"""
    raw, taps, offsets = filter_case(D, n_taps, "u8")
    n1 = 4 * 1001                                                   # (not a multiple of P = 512: a capture index that survived would turn the outputs)
    d = d_factory(n_ensembles=3, max_frames=1, want_constellation=False)
    try:
        d.stream_open_wideband(RING_MIN, D, taps, offsets, "u8")
        d.stream_write_wideband(raw[:n1])
        fresh = read_all(d, n1 // D)
        d.reset()
        d.stream_write_wideband(raw[:n1])                           # (the ring goes on behind the samples written so far)
        again = read_all(d, n1 // D, first=n1 // D)
        for e in range(3):
            assert np.array_equal(fresh[e].view(np.uint32), again[e].view(np.uint32)), "ensemble %d: outputs after dabphy_reset differ from a fresh open's" % e
    finally:
        d.close()


def check_errors(d_factory, D=4, n_taps=64):
    """every DABPHY_ERR_INVALID and DABPHY_ERR_STATE of the contract, one line each"""
    raw, taps, offsets = filter_case(D, n_taps, "u8")
    d = d_factory(n_ensembles=3, max_frames=1, want_constellation=False)
    lib, h = d.lib, d.h
    offs = np.asarray(offsets, np.int32)

    def opened(ring=RING_MIN, decimation=D, n=n_taps, taps_p=taps, offs_p=offs, fmt=1, size=C.sizeof(capi.WidebandConfig), null_cfg=False):
        cfg = capi.WidebandConfig(size, decimation, n, taps_p.ctypes.data_as(C.POINTER(C.c_float)) if taps_p is not None else None,
                                  offs_p.ctypes.data_as(C.POINTER(C.c_int32)) if offs_p is not None else None, fmt)
        return lib.dabphy_stream_open_wideband(h, C.c_uint64(ring), None if null_cfg else C.byref(cfg))

    def write(data, n, fn="dabphy_stream_write_wideband"):
        return getattr(lib, fn)(h, data.ctypes.data_as(C.c_void_p) if data is not None else None, C.c_uint64(n))
    big = np.ascontiguousarray(raw[:4 * D])
    try:
        lib.dabphy_struct_size.restype = C.c_size_t
        assert lib.dabphy_struct_size(10) == C.sizeof(capi.WidebandConfig)
        # ---- a wideband write on a stream that is none
        assert write(big, len(big)) == ERR_STATE
        d.stream_open(RING_MIN)
        assert write(big, len(big)) == ERR_STATE
        assert write(big, len(big), "dabphy_stream_write_wideband_async") == ERR_STATE
        # ---- the open call's limits
        assert opened(null_cfg=True) == ERR_INVALID
        assert lib.dabphy_stream_open_wideband(None, C.c_uint64(RING_MIN), None) == ERR_INVALID
        assert opened(taps_p=None) == ERR_INVALID
        assert opened(offs_p=None) == ERR_INVALID
        assert opened(size=C.sizeof(capi.WidebandConfig) + 8) == ERR_INVALID
        assert opened(decimation=0) == ERR_INVALID
        assert opened(decimation=33) == ERR_INVALID
        assert opened(n=0) == ERR_INVALID
        assert opened(n=1025, taps_p=np.zeros(1025, np.float32)) == ERR_INVALID
        assert opened(offs_p=np.array([0, 64 * D + 1, 0], np.int32)) == ERR_INVALID
        assert opened(offs_p=np.array([0, 0, -(64 * D + 1)], np.int32)) == ERR_INVALID
        assert opened(fmt=5) == ERR_INVALID
        assert opened(fmt=-1) == ERR_INVALID
        assert opened(ring=RING_MIN - 1) == ERR_INVALID
        assert write(big, len(big)) == ERR_STATE                    # (none of them opened anything)
        # ---- the limits at +-64 D and 32 / 1 024 themselves are inside
        assert opened(offs_p=np.array([64 * D, -64 * D, 0], np.int32)) == 0
        assert opened(decimation=32, n=1024, taps_p=np.zeros(1024, np.float32), offs_p=np.array([2048, -2048, 0], np.int32)) == 0
        assert opened() == 0
        # ---- the write calls' limits
        for fn in ("dabphy_stream_write_wideband", "dabphy_stream_write_wideband_async"):
            assert write(None, 4 * D, fn) == ERR_INVALID
            assert getattr(lib, fn)(None, big.ctypes.data_as(C.c_void_p), C.c_uint64(4 * D)) == ERR_INVALID
            assert write(big, 0, fn) == ERR_INVALID
            assert write(big, 4 * D - 1, fn) == ERR_INVALID         # not a multiple of D
            assert write(big, (RING_MIN + 1) * D, fn) == ERR_INVALID      # more outputs than the ring holds (refused before `data` is read)
        # ---- plain writes on a wideband stream
        cf = np.zeros((3, 8), np.complex64)
        assert lib.dabphy_stream_write(h, cf.ctypes.data_as(C.c_void_p), C.c_uint64(8)) == ERR_STATE
        assert lib.dabphy_stream_write_raw(h, cf.ctypes.data_as(C.c_void_p), C.c_uint64(8), 0) == ERR_STATE
        assert lib.dabphy_stream_write_raw(h, big.ctypes.data_as(C.c_void_p), C.c_uint64(4), 1) == ERR_STATE
        assert lib.dabphy_stream_write_raw_async(h, big.ctypes.data_as(C.c_void_p), C.c_uint64(4), 1) == ERR_STATE
        # ---- a synchronous write does not continue asynchronous ones that are not committed
        assert write(big, len(big), "dabphy_stream_write_wideband_async") == 0
        assert write(big, len(big)) == ERR_STATE
        d.stream_commit()
        assert write(big, len(big)) == 0
        # ---- a plain open, a bind or an upload drops the configuration
        d.stream_open(RING_MIN)
        assert write(big, len(big)) == ERR_STATE
        assert opened() == 0 and write(big, len(big)) == 0
        d.stream_upload(np.zeros((3, T_F), np.complex64))
        assert write(big, len(big)) == ERR_STATE
    finally:
        d.close()


def check_end_to_end(d_factory, D=4, offsets=(-107, 0, 107), n_frames=8, snr_db=20):
    """Ensembles side by side in one u8 capture (distinct EIds and seeds, delays 300, 400, 500 ...), channelised with design_taps(D) and
    decoded one frame per call: FIB bytes, CRC flags and the bytes of sub-channels 2 and 11 equal the oracle's on each ensemble's DIRECT
    cf32 stream.  (Soft bits, correctors, impulse responses are not compared: the filtered signal is another signal.)"""
    B = len(offsets)
    clean, want, subs = [], [], None
    for e in range(B):
        kw = dict(eid=0x1000 + 0x111 * e, seed=20 + e, delay=300 + 100 * e)
        x, tx = synth.make_stream(n_frames, return_tx=True, **kw)
        clean.append(x)
        subs = [tx.subchs[2], tx.subchs[11]]
        want.append(R.orc_receiver_run(synth.make_stream(n_frames, snr_db=snr_db, noise_seed=77 + e, **kw), subchs=subs))
    cap = wideband.synth_capture(clean, offsets, D, snr_db=snr_db, seed=5)
    raw, _ = wideband.to_u8_capture(cap)
    assert raw.min() > 0 and raw.max() < 255                       # nothing clips
    d = d_factory(n_ensembles=B, max_frames=1, want_constellation=False)
    try:
        ring = 6 * T_F
        d.stream_open_wideband(ring, D, wideband.design_taps(D), offsets, "u8")
        d.set_subchannels([(s.subch_id, s.start_cu, s.size_cu, d.protection_eep(s.bitrate, s.profile_b, s.level)) for s in subs])
        fibs, oks, msc = [[] for _ in range(B)], [[] for _ in range(B)], [[[] for _ in subs] for _ in range(B)]
        wr = 0

        def feed(n_out):
            nonlocal wr
            n = min(n_out * D, len(raw) - wr)
            if n > 0:
                d.stream_write_wideband(raw[wr:wr + n]); wr += n
        feed(3 * T_F)
        idle = 0
        while idle < 3:
            d.process(1)
            info = d.frame_info()
            if np.any(info[:, 0]["valid"] == 1):
                fb, ok = d.fibs(); idle = 0
                m = [d.msc(i) for i in range(len(subs))]
                for e in range(B):
                    if info[e, 0]["valid"] == 1:
                        fibs[e].append(fb[e, 0]); oks[e].append(ok[e, 0])
                        for i in range(len(subs)):
                            msc[e][i].append(m[i][0][e, m[i][1][e]:4].tobytes())
            else:
                idle += 1
            feed(min(ring - (wr // D - d.stream_consumed()), T_F))
        for e in range(B):
            o = want[e]; n = len(fibs[e])
            assert n >= o["n_frames"] - 1, (e, n, o["n_frames"])
            ofib = o["fib"][:12 * n].reshape(n, 12, 33)
            assert ofib[:, :, 0].all(), "ensemble %d: the oracle's own FIB CRCs fail on the direct stream" % e
            assert np.array_equal(np.array(oks[e]), ofib[:, :, 0]) and np.array_equal(np.array(fibs[e]), ofib[:, :, 1:]), "ensemble %d: FIBs differ" % e
            for i in range(len(subs)):
                got = b"".join(msc[e][i]); ref = bytes(o["msc"][i])
                assert len(got) > 0 and got == ref[:len(got)], "ensemble %d: MSC bytes of sub-channel %d differ" % (e, i)
    finally:
        d.close()
