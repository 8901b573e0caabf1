"""ctypes binding of the C ABI in include/dabphy.h (libdabphy_hip.so).

This is harness plumbing for tests/ and bench.py -- the product boundary is the C ABI itself, bound from the
reference's C++ host code as shown in INTEGRATION.md.  There is no CPU fallback: without the HIP library
(or without a gfx950 device) construction raises.
"""
import ctypes as C
import os
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(HERE, "libdabphy_hip.so")

T_U, T_S, FRAME_SYMS_LEN = 2048, 2552, 2048 + 75 * 2552
ABI_VERSION = 6            # DABPHY_ABI_VERSION of the include/dabphy.h these structures mirror


class Config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_ensembles", C.c_uint32), ("max_frames", C.c_uint32), ("device", C.c_int32),
                ("fft_placement", C.c_int32), ("disable_coarse", C.c_int32), ("want_constellation", C.c_int32),
                ("want_impulse_response", C.c_int32), ("demod_chunk", C.c_int32), ("freqsync_method", C.c_int32), ("pipeline_sync", C.c_int32), ("serial_sync", C.c_int32), ("no_batch_replay", C.c_int32), ("decode_shape", C.c_int32), ("sync_early", C.c_int32)]


class WidebandConfig(C.Structure):
    """dabphy_wideband_config"""
    _fields_ = [("struct_size", C.c_uint32), ("decimation", C.c_uint32), ("n_taps", C.c_uint32), ("taps", C.POINTER(C.c_float)),
                ("offset_16khz", C.POINTER(C.c_int32)), ("format", C.c_int32)]


class ResamplerConfig(C.Structure):
    """dabphy_resampler_config"""
    _fields_ = [("struct_size", C.c_uint32), ("interpolation", C.c_uint32), ("decimation", C.c_uint32), ("n_taps", C.c_uint32),
                ("taps", C.POINTER(C.c_float)), ("offset_16khz", C.POINTER(C.c_int32)), ("format", C.c_int32)]


FORMATS = {"cf32": 0, "u8": 1, "s8": 2, "s16le": 3, "s16be": 4}              # dabphy_sample_format
FORMAT_BYTES = {0: 8, 1: 2, 2: 2, 3: 4, 4: 4}                                # per complex sample


class Protection(C.Structure):
    _fields_ = [("nbits", C.c_int32), ("L", C.c_int32 * 4), ("PI", C.c_int32 * 4)]


class Subchannel(C.Structure):
    _fields_ = [("subch_id", C.c_int32), ("start_cu", C.c_int32), ("size_cu", C.c_int32), ("prot", Protection)]


TII_DTYPE = np.dtype([("frame", "<i4"), ("comb", "<i4"), ("pattern", "<i4"), ("delay_samples", "<i4"), ("error", "<f4")])
SF_EVENT_DTYPE = np.dtype([("cif", "<i4"), ("corrected", "<i4"), ("uncorrectable", "<i4"), ("sync", "<i4"), ("format", "<i4"), ("num_aus", "<i4"),
                           ("au_start", "<i4", 7), ("au_crc_ok", "<i4"), ("sf_slot", "<i4")])


FRAME_INFO_RAW = np.dtype({"names": ["sample_pos", "frame_no", "start_index", "valid", "fine_corrector", "coarse_corrector", "snr"],
                           "formats": ["<i8", "<i8", "<i4", "<i4", "<i4", "<i4", "<f4"], "offsets": [0, 8, 16, 20, 24, 28, 32], "itemsize": 40})      # dabphy_frame_info
MP2_EVENT_DTYPE = np.dtype([("frame", "<i4"), ("header", "<u4"), ("offset", "<i8"), ("crc_ok", "u1"), ("new_format", "u1"), ("scf_crc_len", "u1"),
                            ("fpad", "u1", 2), ("pad_", "u1", 3)])      # dabphy_mp2_event
AUDIO_DABPLUS, AUDIO_MP2 = 0, 1                                           # dabphy_set_audio_kinds_ensemble
MSC_DESC_DTYPE = np.dtype([("ensemble", "<u4"), ("subch_index", "<u4"), ("row_bytes", "<u4"), ("first_valid", "<i4"), ("n_rows", "<i4"), ("subch_id", "<u4"), ("offset", "<u8")])
SYNC_SERIAL, SYNC_WIDE, SYNC_CHAIN = 0, 1, 2                                # dabphy_test_sync_find: k_sync_find, k_sync_find_wide, k_sync_find_chain
SYNC_CASE = 4096                                                            # DABPHY_TEST_SYNC_CASE
SYNC_DESC_DTYPE = np.dtype([("pos", "<i8"), ("start_index", "<i4"), ("valid", "<i4"), ("coarse_ran", "<i4"), ("coarse_after", "<i4"), ("coarse_step", "<i4"), ("L1", "<i4")])   # dabphy_test_sync_desc
SYNC_STATE_DTYPE = np.dtype([("pos", "<i8"), ("synced", "<i4"), ("lost", "<i4")])                                                  # dabphy_test_sync_state
BER_COUNT_DTYPE = np.dtype([("errors", "<u4"), ("compared", "<u4")])                # dabphy_ber_count
AU_OFF, AU_RAW, AU_LOAS = 0, 1, 2                                           # dabphy_set_au_drain
AU_SERVICE_DTYPE = np.dtype([("ensemble", "<u4"), ("subch_index", "<u4"), ("subch_id", "<u4"), ("n_superframes", "<i4"), ("n_aus", "<i4"), ("n_failed", "<i4"),
                             ("first_au", "<u4"), ("pad_", "<u4"), ("offset", "<u8"), ("bytes", "<u8")])      # dabphy_au_service
AU_DESC_DTYPE = np.dtype([("cif", "<i4"), ("au_index", "u1"), ("format", "u1"), ("pad_", "u1", 2), ("length", "<u4"), ("pad2_", "<u4"), ("offset", "<u8")])      # dabphy_au_desc


class DabPhyError(RuntimeError):
    pass


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def load_library(path=None):
    path = path or DEFAULT_LIB
    if not os.path.exists(path):
        raise DabPhyError("HIP library not built: %s (run __graft_entry__.build())" % path)
    lib = C.CDLL(path)
    lib.dabphy_last_error.restype = C.c_char_p
    lib.dabphy_device_name.restype = C.c_char_p
    return lib


def fused_windows(lib, p):
    """dabphy_test_fused_windows on a loaded library: needs no handle and no device"""
    n = (C.c_int32 * 3)()
    r = lib.dabphy_test_fused_windows(C.byref(p), n)
    if r != 0:
        raise DabPhyError("dabphy_test_fused_windows: status %d" % r)
    return tuple(n)


class DabPhy:
    def __init__(self, n_ensembles=1, max_frames=1, device=0, lib_path=None, fft_placement=2, disable_coarse=False,
                 want_constellation=True, want_impulse_response=True, demod_chunk=0, pipeline_sync=False, freqsync_method=2, serial_sync=False, exact_batch=True, decode_shape=0, sync_early=0):
        self.lib = load_library(lib_path)
        cfg = Config(C.sizeof(Config), n_ensembles, max_frames, device, fft_placement, int(disable_coarse), int(want_constellation),
                     int(want_impulse_response), demod_chunk, freqsync_method, int(pipeline_sync), int(serial_sync), int(not exact_batch), int(decode_shape), int(sync_early))   # pipeline_sync: False/True/2
        self.cfg = cfg
        self.h = C.c_void_p()
        if self.lib.dabphy_abi_version() != ABI_VERSION:
            raise DabPhyError("library ABI version %d, this binding was written for %d" % (self.lib.dabphy_abi_version(), ABI_VERSION))
        r = self.lib.dabphy_create_v2(C.byref(cfg), C.byref(self.h))
        if r != 0:
            raise DabPhyError("dabphy_create failed with status %d (no gfx950 device?)" % r)

    def close(self):
        if self.h:
            self.lib.dabphy_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, r):
        if r != 0:
            raise DabPhyError("status %d: %s" % (r, self.lib.dabphy_last_error(self.h).decode()))

    @property
    def device_name(self):
        return self.lib.dabphy_device_name(self.h).decode()

    # ---- protection helpers
    def protection_fic(self):
        p = Protection(); self._chk(self.lib.dabphy_protection_fic(C.byref(p))); return p

    def protection_eep(self, bitrate, profile_b, level):
        p = Protection(); self._chk(self.lib.dabphy_protection_eep(C.byref(p), bitrate, int(profile_b), level)); return p

    def protection_uep(self, bitrate, level):
        p = Protection(); self._chk(self.lib.dabphy_protection_uep(C.byref(p), bitrate, level)); return p

    def protection_input_bits(self, p):
        return self.lib.dabphy_protection_input_bits(C.byref(p))

    def fused_windows(self, p):
        """windows of the fused decode's schedule for its three row counts, 0 = no schedule (dabphy_test_fused_windows: host only)"""
        return fused_windows(self.lib, p)

    # ---- unit-level seams
    def demod_frames(self, frames, want_con=True):
        frames = np.ascontiguousarray(frames, np.complex64).reshape(-1, FRAME_SYMS_LEN)
        n = frames.shape[0]
        soft = np.zeros((n, 75, 3072), np.int8)
        con = np.zeros((n, 1200), np.complex64) if want_con else None
        snr = np.zeros(n, np.float32)
        self._chk(self.lib.dabphy_demod_frames(self.h, _p(frames), n, _p(soft), _p(con) if want_con else None, _p(snr)))
        return soft, con, snr

    def viterbi_batch(self, soft, nbits):
        soft = np.ascontiguousarray(soft, np.int8).reshape(-1, 4 * (nbits + 6))
        n = soft.shape[0]
        out = np.zeros((n, nbits // 8), np.uint8)
        self._chk(self.lib.dabphy_viterbi_batch(self.h, _p(soft), nbits, n, _p(out)))
        return out

    def msc_deconvolve(self, prot, soft):
        nin = self.protection_input_bits(prot)
        soft = np.ascontiguousarray(soft, np.int8).reshape(-1, nin)
        n = soft.shape[0]
        out = np.zeros((n, prot.nbits // 8), np.uint8)
        self._chk(self.lib.dabphy_msc_deconvolve(self.h, C.byref(prot), _p(soft), n, _p(out)))
        return out

    def fic_decode(self, soft):
        soft = np.ascontiguousarray(soft, np.int8).reshape(-1, 9216)
        n = soft.shape[0]
        fib = np.zeros((n, 12, 32), np.uint8); ok = np.zeros((n, 12), np.uint8); ratio = C.c_int32(0)
        self._chk(self.lib.dabphy_fic_decode(self.h, _p(soft), n, _p(fib), _p(ok), C.byref(ratio)))
        return fib, ok, ratio.value

    # ---- diagnostics
    def time_demod(self, frames, n_ens, n_frames, mix=0, f_hz=0, iters=5):
        frames = np.ascontiguousarray(frames, np.complex64).reshape(-1, FRAME_SYMS_LEN)
        ms = C.c_float(0)
        self._chk(self.lib.dabphy_time_demod(self.h, _p(frames), frames.shape[0], n_ens, n_frames, mix, f_hz, iters, C.byref(ms)))
        return ms.value

    def superframes(self, subch_index, bitrate):
        """-> (events structured array [B][4F], n_events [B], corrected superframes [B][n_slots][120*bitrate/8])"""
        B, F = self.cfg.n_ensembles, self._last
        ev = np.zeros((B, 4 * F), SF_EVENT_DTYPE); ne = np.zeros(B, np.int32)
        sf = np.zeros((B, 4 * F // 5 + 1, 15 * bitrate), np.uint8)
        self._chk(self.lib.dabphy_superframes(self.h, subch_index, _p(ev), _p(ne), _p(sf)))
        return ev, ne, sf

    def sync_stats(self):
        """(failed window searches, frames settled by the ordered float sums) per ensemble since reset"""
        lost = np.zeros(self.cfg.n_ensembles, np.int32); ex = np.zeros(self.cfg.n_ensembles, np.int32)
        self.relock_inexact = np.zeros(self.cfg.n_ensembles, np.int32)
        self._chk(self.lib.dabphy_get_sync_stats(self.h, _p(lost), _p(ex), _p(self.relock_inexact)))
        return lost, ex

    def wide_sync_stats(self):
        """(frames per ensemble accepted from the wide synchroniser pass, passes queued, passes that needed the serial chain)"""
        wf = np.zeros(self.cfg.n_ensembles, np.int32); a = C.c_uint64(0); b = C.c_uint64(0)
        self._chk(self.lib.dabphy_get_wide_sync_stats(self.h, _p(wf), C.byref(a), C.byref(b)))
        return wf, a.value, b.value

    def find_chain_stats(self):
        """frames per ensemble whose window search ran in the find chain (of those accepted from the wide synchroniser pass)"""
        cf = np.zeros(self.cfg.n_ensembles, np.int32)
        self._chk(self.lib.dabphy_get_find_chain_stats(self.h, _p(cf)))
        return cf

    def replayed_batches(self):
        a = C.c_uint64(0)
        self._chk(self.lib.dabphy_get_replayed_batches(self.h, C.byref(a)))
        return a.value

    def wide_superframe_stats(self):
        """(sub-channel batches the superframe filter's wide pass settled, batches it was tried on) since create"""
        a = C.c_uint64(0); b = C.c_uint64(0)
        self._chk(self.lib.dabphy_get_wide_superframe_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def osc_stats(self):
        """(symbols mixed with the unchecked oscillator conversion, symbols that took the checked one) since create"""
        a = C.c_uint64(0); b = C.c_uint64(0)
        self._chk(self.lib.dabphy_get_osc_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_track_slevel(self, on=True):
        self._chk(self.lib.dabphy_set_track_slevel(self.h, int(on)))

    def set_auto_superframes(self, on=True):        # (on = 2: the filter pass of a batch deferred to the next process(), beside its FFT stage)
        """run the all-sub-channel superframe filter inside every process() call; superframes_stats() then only fetches the totals"""
        self._chk(self.lib.dabphy_set_auto_superframes(self.h, int(on)))

    def superframes_stats(self):
        st = np.zeros((self.cfg.n_ensembles, 4), np.int32)
        self._chk(self.lib.dabphy_superframes_stats(self.h, _p(st)))
        return st

    def set_tii(self, on=True):
        """RadioReceiverOptions::decodeTII for the following process() calls"""
        self._chk(self.lib.dabphy_set_tii(self.h, int(on)))

    def tii(self, max_per_ensemble=None):
        """onTIIMeasurement calls of the last batch: list per ensemble of records (frame, comb, pattern, delay_samples, error)"""
        B = self.cfg.n_ensembles
        m = 9 * self.cfg.max_frames if max_per_ensemble is None else max_per_ensemble
        ev = np.zeros((B, max(m, 1)), TII_DTYPE); n = np.zeros(B, np.int32)
        self._chk(self.lib.dabphy_get_tii(self.h, _p(ev), _p(n), m))
        return [ev[b, :min(int(n[b]), m)].copy() for b in range(B)], n

    def test_tii_pairs(self, null, prs, valid=None):
        """dabphy_test_tii_pairs: the TII kernels over (NULL [B][F][2656], PRS [B][F][2048]) pairs; valid [B][F] (default: all 1).
        tii() then returns this call's measurements"""
        B = self.cfg.n_ensembles
        null = np.ascontiguousarray(null, np.complex64).reshape(B, -1, 2656); F = null.shape[1]
        prs = np.ascontiguousarray(prs, np.complex64).reshape(B, F, 2048)
        valid = np.ones((B, F), np.int32) if valid is None else np.ascontiguousarray(valid, np.int32).reshape(B, F)
        self._chk(self.lib.dabphy_test_tii_pairs(self.h, _p(null), _p(prs), _p(valid), B, F))

    def test_sync_find(self, kernel, iq, coarse, fine, fic_ratio, n_frames=1):
        """dabphy_test_sync_find: one window-search launch (SYNC_SERIAL / SYNC_WIDE / SYNC_CHAIN) over the cases iq [B][4096], one per
        ensemble, each with its starting correctors and FIC ratio -> (descriptors [B][n_frames] of SYNC_DESC_DTYPE, impulse responses
        [B][n_frames][2048], receiver state [B] of SYNC_STATE_DTYPE).  The handle needs reset() before anything else"""
        B = self.cfg.n_ensembles
        iq = np.ascontiguousarray(iq, np.complex64).reshape(-1, SYNC_CASE)
        coarse = np.ascontiguousarray(coarse, np.int32).reshape(-1); fine = np.ascontiguousarray(fine, np.int32).reshape(-1)
        fic_ratio = np.ascontiguousarray(fic_ratio, np.int32).reshape(-1)
        n = iq.shape[0]
        if not (len(coarse) == len(fine) == len(fic_ratio) == n):
            raise DabPhyError("test_sync_find: %d cases, %d / %d / %d parameters" % (n, len(coarse), len(fine), len(fic_ratio)))
        F = max(int(n_frames), 1)
        desc = np.zeros((n, F), SYNC_DESC_DTYPE); cir = np.zeros((n, F, 2048), np.float32); st = np.zeros(n, SYNC_STATE_DTYPE)
        self._chk(self.lib.dabphy_test_sync_find(self.h, C.c_int32(int(kernel)), _p(iq), _p(coarse), _p(fine), _p(fic_ratio), C.c_uint32(n), C.c_uint32(int(n_frames)),
                                                 _p(desc), _p(cir), _p(st)))
        return desc, cir, st

    def test_tii_dropped(self):
        """dabphy_test_tii_dropped: measurements per ensemble that found all 32 slots taken"""
        n = np.zeros(self.cfg.n_ensembles, np.int32)
        self._chk(self.lib.dabphy_test_tii_dropped(self.h, _p(n)))
        return n

    def selftest_unit_twiddle(self):
        c = (C.c_uint64 * 2)()
        self._chk(self.lib.dabphy_selftest_unit_twiddle(self.h, c))
        return [int(x) for x in c]

    def selftest_pair_exchange(self):
        c = (C.c_uint64 * 2)()
        self._chk(self.lib.dabphy_selftest_pair_exchange(self.h, c))
        return [int(x) for x in c]

    def selftest_div127(self):
        c = (C.c_uint64 * 3)()
        self._chk(self.lib.dabphy_selftest_div127(self.h, c))
        return [int(x) for x in c]

    def time_viterbi(self, nbits, n_codewords, iters=3):
        a = C.c_float(0); b = C.c_float(0)
        self._chk(self.lib.dabphy_time_viterbi(self.h, nbits, n_codewords, iters, C.byref(a), C.byref(b)))
        return a.value, b.value

    def time_copy(self, nbytes=2 << 30, blocks_per_cu=0, iters=5):
        """GB/s (read + write) of a plain float4 device copy of nbytes (dabphy_time_copy)"""
        a = C.c_float(0)
        self._chk(self.lib.dabphy_time_copy(self.h, C.c_uint64(nbytes), blocks_per_cu, iters, C.byref(a)))
        return a.value

    def traceback_split(self, on=True):
        """the lane-per-code-word kernel's traceback as a pass of its own beside the forward pass (dabphy_test_traceback_split)"""
        self._chk(self.lib.dabphy_test_traceback_split(self.h, int(on)))

    def last_decode_plan(self):
        """(kernel that decoded the last process(), numbered like dabphy_config.decode_shape: 1 = lane per code word (k_viterbi_fused), 2 = state-parallel with two code words per wavefront (k_viterbi_sp2 + k_traceback_sp2), 3 = state-parallel with one (k_viterbi_sp), 0 = nothing decoded yet; protection classes in that launch)"""
        a = C.c_int32(0); b = C.c_int32(0)
        self._chk(self.lib.dabphy_last_decode_plan(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def time_fused_msc(self, iters=3):
        a = C.c_float(0)
        self._chk(self.lib.dabphy_time_fused_msc(self.h, iters, C.byref(a)))
        return a.value

    def time_superframe_wide(self, iters=3):
        """mean device time [ms] of the last filter pass' wide launches run again alone (dabphy_time_superframe_wide)"""
        a = C.c_float(0)
        self._chk(self.lib.dabphy_time_superframe_wide(self.h, iters, C.byref(a)))
        return a.value

    # ---- streaming receiver
    def reset(self):
        self._chk(self.lib.dabphy_reset(self.h))

    def stream_upload(self, iq, loop=False):
        """iq: (n_ensembles, n_samples) complex64 host array"""
        iq = np.ascontiguousarray(iq, np.complex64).reshape(self.cfg.n_ensembles, -1)
        self._chk(self.lib.dabphy_stream_upload(self.h, _p(iq), C.c_uint64(iq.shape[1]), int(loop)))

    def stream_bind_device(self, dev_ptr, ring_samples, stride_samples, n_valid, loop=False):
        self._chk(self.lib.dabphy_stream_bind_device(self.h, C.c_void_p(dev_ptr), C.c_uint64(ring_samples), C.c_uint64(stride_samples),
                                                     C.c_uint64(n_valid), int(loop)))

    def set_subchannels(self, subs):
        """subs: list of (subch_id, start_cu, size_cu, Protection)"""
        arr = (Subchannel * max(1, len(subs)))()
        for i, (sid, start, size, prot) in enumerate(subs):
            arr[i].subch_id = sid; arr[i].start_cu = start; arr[i].size_cu = size; arr[i].prot = prot
        self._n_sub = len(subs); self._sub_bytes = [s[3].nbits // 8 for s in subs]; self._ens_bytes = {}
        self._chk(self.lib.dabphy_set_subchannels(self.h, arr, len(subs)))

    def set_subchannels_ensemble(self, ensemble, subs):
        """the list of ONE ensemble of the batch (dabphy_set_subchannels_ensemble): takes effect with the next process()"""
        arr = (Subchannel * max(1, len(subs)))()
        for i, (sid, start, size, prot) in enumerate(subs):
            arr[i].subch_id = sid; arr[i].start_cu = start; arr[i].size_cu = size; arr[i].prot = prot
        self._ens_bytes = getattr(self, "_ens_bytes", {})
        self._ens_bytes[ensemble] = [s[3].nbits // 8 for s in subs]
        self._chk(self.lib.dabphy_set_subchannels_ensemble(self.h, ensemble, arr, len(subs)))

    def msc_ensemble(self, ensemble, idx):
        """-> (out [4F][bytes], first_valid, n_rows) of sub-channel idx (position in ITS list) of one ensemble"""
        F = self._last
        nb = self._ens_bytes[ensemble][idx] if ensemble in getattr(self, "_ens_bytes", {}) else self._sub_bytes[idx]
        out = np.zeros((4 * F, nb), np.uint8); fv = C.c_int32(0); nr = C.c_int32(0)
        self._chk(self.lib.dabphy_get_msc_ensemble(self.h, ensemble, idx, _p(out), C.c_size_t(out.nbytes), C.byref(fv), C.byref(nr)))
        return out, fv.value, nr.value

    def msc_batch_size(self):
        """(bytes, services) the bulk drain of the last batch needs (dabphy_msc_batch_size)"""
        nb = C.c_size_t(0); nd = C.c_uint32(0)
        self._chk(self.lib.dabphy_msc_batch_size(self.h, C.byref(nb), C.byref(nd)))
        return nb.value, nd.value

    def msc_drain_begin(self, buf=None, desc=None):
        """dabphy_msc_drain_begin: queue the bulk drain of every selected sub-channel of every ensemble into `buf` (uint8; page-locked from
        host_alloc for PCIe rate) and return (buf, desc records) at once; msc_drain_wait() completes it"""
        nb, nd = self.msc_batch_size()
        if buf is None:
            buf = np.zeros(max(nb, 1), np.uint8)
        if desc is None:
            desc = np.zeros(max(nd, 1), MSC_DESC_DTYPE)
        n = C.c_uint32(0)
        self._chk(self.lib.dabphy_msc_drain_begin(self.h, _p(desc), C.c_uint32(len(desc)), C.byref(n), _p(buf), C.c_size_t(buf.nbytes)))
        return buf, desc[:n.value]

    def msc_drain_wait(self):
        self._chk(self.lib.dabphy_msc_drain_wait(self.h))

    def msc_batch(self, buf=None, desc=None):
        """dabphy_get_msc_batch -> (buf, desc): service k's logical frames = buf[desc[k].offset:][: 4F * row_bytes].reshape(4F, row_bytes)[first_valid:n_rows]"""
        buf, desc = self.msc_drain_begin(buf, desc)
        self.msc_drain_wait()
        return buf, desc

    # ---- bulk access-unit drain
    def set_au_drain(self, fmt):
        """AU_OFF / AU_RAW / AU_LOAS for the filter passes queued from now on (dabphy_set_au_drain)"""
        self._chk(self.lib.dabphy_set_au_drain(self.h, int(fmt)))

    def au_batch_size(self):
        """(bytes, service records, access-unit records) a drain of the filter pass that ran last needs (dabphy_au_batch_size)"""
        nb = C.c_size_t(0); ns = C.c_uint32(0); na = C.c_uint32(0)
        self._chk(self.lib.dabphy_au_batch_size(self.h, C.byref(nb), C.byref(ns), C.byref(na)))
        return nb.value, ns.value, na.value

    def au_drain_begin(self, buf=None, services=None, aus=True):
        """dabphy_au_drain_begin: queue the drain of the filter pass that ran last and return (buf, services, aus) at once -- all three are
        complete only when au_drain_wait() has returned.  aus: True = allocate the access-unit table, None / False = skip it, or an array"""
        if buf is None or services is None or aus is True:             # (every array given: no size query stands in front of the entry)
            nb, ns, na = self.au_batch_size()
        if buf is None:
            buf = np.zeros(max(nb, 1), np.uint8)
        if services is None:
            services = np.zeros(max(ns, 1), AU_SERVICE_DTYPE)
        if aus is True:
            aus = np.zeros(max(na, 1), AU_DESC_DTYPE)
        elif aus is False:
            aus = None
        self._chk(self.lib.dabphy_au_drain_begin(self.h, _p(services), C.c_uint32(len(services)), _p(aus) if aus is not None else None,
                                                 C.c_uint32(len(aus) if aus is not None else 0), _p(buf), C.c_size_t(buf.nbytes)))
        self._au_out = (buf, services, aus)
        return self._au_out

    def au_drain_wait(self):
        """-> (buf, services [n], aus or None): service k's bytes = buf[offset : offset + bytes], its records aus[first_au : first_au + n_aus]"""
        ns = C.c_uint32(0); na = C.c_uint32(0)
        self._chk(self.lib.dabphy_au_drain_wait(self.h, C.byref(ns), C.byref(na)))
        buf, services, aus = self._au_out
        return buf, services[:ns.value], (aus[:na.value] if aus is not None else None)

    def au_batch(self, buf=None, services=None, aus=True):
        """dabphy_get_au_batch: begin + wait"""
        self.au_drain_begin(buf, services, aus)
        return self.au_drain_wait()

    def au_ms(self):
        """device time of the last pack pass queued with profiling on"""
        ms = C.c_float(0)
        self._chk(self.lib.dabphy_get_au_ms(self.h, C.byref(ms)))
        return ms.value

    def test_au_pack(self, sf, events, s_per_sf, fmt, out_capacity=None):
        """unit entry (dabphy_test_au_pack): corrected superframes sf [n_sf][120 * s_per_sf] and their events as ONE service ->
        (out [out_capacity], aus [n_aus] of AU_DESC_DTYPE, service record)"""
        sf = np.ascontiguousarray(sf, np.uint8).reshape(-1, 120 * s_per_sf)
        ev = np.ascontiguousarray(events, SF_EVENT_DTYPE)
        n_sf = sf.shape[0]
        cap = n_sf * (120 * s_per_sf + 128) if out_capacity is None else out_capacity
        out = np.full(max(cap, 1), 0xA5, np.uint8); aus = np.zeros(max(6 * n_sf, 1), AU_DESC_DTYPE); svc = np.zeros(1, AU_SERVICE_DTYPE)
        self._chk(self.lib.dabphy_test_au_pack(self.h, _p(sf), _p(ev), C.c_uint32(len(ev)), C.c_uint32(n_sf), C.c_uint32(s_per_sf), C.c_int32(int(fmt)),
                                               _p(out), C.c_size_t(cap), _p(aus), C.c_uint32(len(aus)), _p(svc)))
        return out[:cap], aus[:int(svc[0]["n_aus"])], svc[0]

    def superframes_ensemble(self, ensemble, idx, bitrate):
        """-> (events [4F], n_events, corrected superframes [n_slots][120*bitrate/8]) of one ensemble's sub-channel idx"""
        F = self._last
        ev = np.zeros(4 * F, SF_EVENT_DTYPE); ne = C.c_int32(0)
        sf = np.zeros((4 * F // 5 + 1, 15 * bitrate), np.uint8)
        self._chk(self.lib.dabphy_superframes_ensemble(self.h, ensemble, idx, _p(ev), C.byref(ne), _p(sf)))
        return ev, ne.value, sf

    # ---- classic DAB (MP2) services
    def set_audio_kinds_ensemble(self, ensemble, kinds):
        """AUDIO_DABPLUS / AUDIO_MP2 for every position of ONE ensemble's list (set after the list; takes effect with the next process())"""
        k = np.ascontiguousarray(kinds, np.int32)
        self._chk(self.lib.dabphy_set_audio_kinds_ensemble(self.h, ensemble, _p(k), C.c_uint32(len(k))))

    def mp2_frames_ensemble(self, ensemble, idx):
        """-> (events [n] of MP2_EVENT_DTYPE, n_events, frame_errors [4F], first_unverified) of one ensemble's MP2 sub-channel idx"""
        F = self._last
        cap = 8 * F + 8
        ev = np.zeros(cap, MP2_EVENT_DTYPE); ne = C.c_int32(0); fe = np.zeros(4 * F, np.int32); fu = C.c_int32(0)
        self._chk(self.lib.dabphy_mp2_frames_ensemble(self.h, ensemble, idx, _p(ev), C.c_int32(cap), C.byref(ne), _p(fe), C.byref(fu)))
        return ev[:min(ne.value, cap)], ne.value, fe, fu.value

    def mp2_stats(self):
        """[n_ensembles][4]: frames checked, CRC failures, bytes skipped in resync, unverified logical frames"""
        st = np.zeros((self.cfg.n_ensembles, 4), np.int32)
        self._chk(self.lib.dabphy_mp2_stats(self.h, _p(st)))
        return st

    def set_auto_mp2(self, on=True):
        self._chk(self.lib.dabphy_set_auto_mp2(self.h, int(on)))

    def mp2_ms(self):
        """device time of the last MP2 pass run with profiling on"""
        ms = C.c_float(0)
        self._chk(self.lib.dabphy_get_mp2_ms(self.h, C.byref(ms)))
        return ms.value

    def mp2_check(self, frames, frame_len, cap=None):
        """unit entry: frames [n_streams][n_frames * frame_len] (or one stream as bytes) from fresh parsers ->
        (events per stream (lists of MP2_EVENT_DTYPE arrays), n_events [S], frame_errors [S][n_frames], first_unverified [S])"""
        if isinstance(frames, (bytes, bytearray)):
            frames = np.frombuffer(bytes(frames), np.uint8)[None]
        frames = np.ascontiguousarray(frames, np.uint8)
        S = frames.shape[0]
        nf = frames.shape[1] // frame_len
        frames = np.ascontiguousarray(frames[:, :nf * frame_len])
        cap = 2 * nf + 8 if cap is None else cap
        ev = np.zeros((S, max(cap, 1)), MP2_EVENT_DTYPE); ne = np.zeros(S, np.int32); fe = np.zeros((S, nf), np.int32); fu = np.zeros(S, np.int32)
        self._chk(self.lib.dabphy_mp2_check(self.h, _p(frames), C.c_uint32(S), C.c_uint32(nf), C.c_uint32(frame_len), _p(ev), C.c_int32(cap), _p(ne), _p(fe), _p(fu)))
        return [ev[s, :min(ne[s], cap)] for s in range(S)], ne, fe, fu

    # ---- channel BER (pseudo-BER) in front of the Viterbi decoder
    def set_channel_ber(self, on=True):
        self._chk(self.lib.dabphy_set_channel_ber(self.h, int(on)))

    def channel_ber(self, prot, soft, decoded):
        """stateless entry (dabphy_channel_ber): punctured soft bits [n][input bits] and the decoded bytes [n][nbits / 8] -> BER_COUNT_DTYPE [n]"""
        nin = self.protection_input_bits(prot)
        soft = np.ascontiguousarray(soft, np.int8).reshape(-1, nin)
        decoded = np.ascontiguousarray(decoded, np.uint8).reshape(-1, prot.nbits // 8)
        n = soft.shape[0]
        if decoded.shape[0] != n:
            raise DabPhyError("channel_ber: %d code words of soft bits, %d of decoded bytes" % (n, decoded.shape[0]))
        out = np.zeros(n, BER_COUNT_DTYPE)
        self._chk(self.lib.dabphy_channel_ber(self.h, C.byref(prot), _p(soft), _p(decoded), C.c_uint32(n), _p(out)))
        return out

    def channel_ber_fic(self):
        """-> BER_COUNT_DTYPE [B][F][4] of the last batch"""
        out = np.zeros((self.cfg.n_ensembles, getattr(self, "_last", 0) or 1, 4), BER_COUNT_DTYPE)      # (before the first process(): the library refuses)
        self._chk(self.lib.dabphy_get_channel_ber_fic(self.h, _p(out)))
        return out

    def channel_ber_ensemble(self, ensemble, idx):
        """-> (BER_COUNT_DTYPE [4F], first_valid, n_rows) of sub-channel idx of one ensemble"""
        out = np.zeros(4 * (getattr(self, "_last", 0) or 1), BER_COUNT_DTYPE); fv = C.c_int32(0); nr = C.c_int32(0)
        self._chk(self.lib.dabphy_get_channel_ber_ensemble(self.h, ensemble, idx, _p(out), C.c_size_t(len(out)), C.byref(fv), C.byref(nr)))
        return out, fv.value, nr.value

    def channel_ber_totals(self):
        """-> (errors, compared) uint64 [B][1 + longest list]: slot 0 the FIC, slot 1 + i list position i"""
        n = C.c_uint32(0)
        self._chk(self.lib.dabphy_get_channel_ber_totals(self.h, None, None, C.byref(n)))
        e = np.zeros((self.cfg.n_ensembles, n.value), np.uint64); c = np.zeros_like(e)
        self._chk(self.lib.dabphy_get_channel_ber_totals(self.h, _p(e), _p(c), C.byref(n)))
        return e, c

    def chanber_ms(self):
        """device time of the last channel BER pass queued with profiling on"""
        ms = C.c_float(0)
        self._chk(self.lib.dabphy_get_chanber_ms(self.h, C.byref(ms)))
        return ms.value

    def host_alloc(self, shape, dtype):
        """page-locked numpy array (dabphy_host_alloc); release with host_free(arr)"""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        self._chk(self.lib.dabphy_host_alloc(C.c_size_t(nbytes), C.byref(p)))
        arr = np.frombuffer((C.c_uint8 * nbytes).from_address(p.value), dtype=dtype).reshape(shape)
        self._pinned = getattr(self, "_pinned", {}); self._pinned[arr.ctypes.data] = p
        return arr

    def host_free(self, arr):
        self.lib.dabphy_host_free.restype = None
        self.lib.dabphy_host_free(self._pinned.pop(arr.ctypes.data))

    def stream_open(self, ring_samples):
        self._chk(self.lib.dabphy_stream_open(self.h, C.c_uint64(ring_samples)))

    def stream_write(self, iq):
        iq = np.ascontiguousarray(iq, np.complex64).reshape(self.cfg.n_ensembles, -1)
        self._chk(self.lib.dabphy_stream_write(self.h, _p(iq), C.c_uint64(iq.shape[1])))

    def stream_write_raw(self, data, fmt):
        """data: [ensemble][n_samples][2] integers in the sample format fmt ("u8", "s8", "s16le", "s16be": CRAWFileFormat names)"""
        code = {"u8": 1, "s8": 2, "s16le": 3, "s16be": 4}[fmt]
        data = np.ascontiguousarray(data)
        bps = 2 if code <= 2 else 4
        n = data.nbytes // (self.cfg.n_ensembles * bps)
        self._chk(self.lib.dabphy_stream_write_raw(self.h, _p(data), C.c_uint64(n), code))

    def stream_write_raw_async(self, data, fmt):
        code = {"u8": 1, "s8": 2, "s16le": 3, "s16be": 4}[fmt]
        assert data.flags["C_CONTIGUOUS"]
        bps = 2 if code <= 2 else 4
        self._chk(self.lib.dabphy_stream_write_raw_async(self.h, _p(data), C.c_uint64(data.nbytes // (self.cfg.n_ensembles * bps)), code))

    # ---- wideband front end: one capture at decimation x 2.048 MS/s, channelised on the device into every ensemble's ring row
    def stream_open_wideband(self, ring_samples, decimation, taps, offsets, fmt):
        """taps: real low-pass at the capture's rate (wideband.design_taps); offsets: per ensemble, block centre minus capture centre in
        units of 16 kHz; fmt: "cf32", "u8", "s8", "s16le", "s16be" (dabphy_stream_open_wideband: stream_open + the tables)"""
        taps = np.ascontiguousarray(taps, np.float32).reshape(-1); offsets = np.ascontiguousarray(offsets, np.int32).reshape(-1)
        if len(offsets) != self.cfg.n_ensembles:
            raise DabPhyError("stream_open_wideband: %d offsets for %d ensembles" % (len(offsets), self.cfg.n_ensembles))
        cfg = WidebandConfig(C.sizeof(WidebandConfig), int(decimation), len(taps), taps.ctypes.data_as(C.POINTER(C.c_float)),
                             offsets.ctypes.data_as(C.POINTER(C.c_int32)), FORMATS[fmt])
        self._chk(self.lib.dabphy_stream_open_wideband(self.h, C.c_uint64(ring_samples), C.byref(cfg)))
        self._wb = (int(decimation), FORMAT_BYTES[FORMATS[fmt]])

    def stream_open_resampled(self, ring_samples, interpolation, decimation, taps, offsets, fmt):
        """the same for a capture at 2.048 MS/s x decimation / interpolation (coprime): taps = the real prototype low-pass at
        interpolation x the capture's rate (wideband.design_taps_rational); writes go through stream_write_wideband[_async], any
        positive number of samples at a time (dabphy_stream_open_resampled)"""
        taps = np.ascontiguousarray(taps, np.float32).reshape(-1); offsets = np.ascontiguousarray(offsets, np.int32).reshape(-1)
        if len(offsets) != self.cfg.n_ensembles:
            raise DabPhyError("stream_open_resampled: %d offsets for %d ensembles" % (len(offsets), self.cfg.n_ensembles))
        cfg = ResamplerConfig(C.sizeof(ResamplerConfig), int(interpolation), int(decimation), len(taps), taps.ctypes.data_as(C.POINTER(C.c_float)),
                              offsets.ctypes.data_as(C.POINTER(C.c_int32)), FORMATS[fmt])
        self._chk(self.lib.dabphy_stream_open_resampled(self.h, C.c_uint64(ring_samples), C.byref(cfg)))
        self._wb = ((int(interpolation), int(decimation)), FORMAT_BYTES[FORMATS[fmt]])

    def stream_write_wideband(self, data):
        """data: the capture's next samples, [n][2] integers of the configured format (or complex64); n a multiple of the decimation
        (any positive n on a stream opened with stream_open_resampled)"""
        data = np.ascontiguousarray(data)
        self._chk(self.lib.dabphy_stream_write_wideband(self.h, _p(data), C.c_uint64(data.nbytes // self._wb[1])))

    def stream_write_wideband_async(self, data):
        """the same on the copy stream (visible after stream_commit); `data` stays untouched until the next-but-one call returns"""
        assert data.flags["C_CONTIGUOUS"]
        self._chk(self.lib.dabphy_stream_write_wideband_async(self.h, _p(data), C.c_uint64(data.nbytes // self._wb[1])))

    def time_wideband(self, warmup=3, iters=20):
        """device milliseconds of `iters` repeats of the last stream_write_wideband's launches on its staged capture (dabphy_time_wideband)"""
        ms = np.zeros(iters, np.float32)
        self._chk(self.lib.dabphy_time_wideband(self.h, C.c_uint32(warmup), C.c_uint32(iters), _p(ms)))
        return ms

    def stream_read(self, ensemble, pos, n):
        out = np.zeros(n, np.complex64)
        self._chk(self.lib.dabphy_stream_read(self.h, ensemble, C.c_uint64(pos), C.c_uint64(n), _p(out)))
        return out

    def stream_commit(self):
        self._chk(self.lib.dabphy_stream_commit(self.h))

    def stream_consumed(self):
        self.lib.dabphy_stream_consumed.restype = C.c_uint64
        return int(self.lib.dabphy_stream_consumed(self.h))

    def process(self, n_frames):
        self._chk(self.lib.dabphy_process(self.h, n_frames))
        self._last = n_frames

    def frame_info(self):
        B, F = self.cfg.n_ensembles, self._last
        arr = (FrameInfo * (B * F))()
        self._chk(self.lib.dabphy_get_frame_info(self.h, arr))
        raw = np.frombuffer(arr, dtype=FRAME_INFO_RAW)
        out = np.zeros((B, F), dtype=[("pos", np.int64), ("frame_no", np.int64), ("start_index", np.int32), ("valid", np.int32),
                                      ("fine", np.int32), ("coarse", np.int32), ("snr", np.float32)])
        flat = out.reshape(-1)
        for dst, src in (("pos", "sample_pos"), ("frame_no", "frame_no"), ("start_index", "start_index"), ("valid", "valid"), ("fine", "fine_corrector"),
                         ("coarse", "coarse_corrector"), ("snr", "snr")):
            flat[dst] = raw[src]
        return out

    def fibs(self):
        B, F = self.cfg.n_ensembles, self._last
        fib = np.zeros((B, F, 12, 32), np.uint8); ok = np.zeros((B, F, 12), np.uint8)
        self._chk(self.lib.dabphy_get_fibs(self.h, _p(fib), _p(ok)))
        return fib, ok

    def fibs_host(self):
        """the same, as read-only views of the library's page-locked host copies (valid until the next process())"""
        B, F = self.cfg.n_ensembles, self._last
        pf = C.POINTER(C.c_uint8)(); po = C.POINTER(C.c_uint8)()
        self._chk(self.lib.dabphy_get_fibs_host(self.h, C.byref(pf), C.byref(po)))
        fib = np.ctypeslib.as_array(pf, shape=(B * F * 384,)).reshape(B, F, 12, 32)
        ok = np.ctypeslib.as_array(po, shape=(B * F * 12,)).reshape(B, F, 12)
        return fib, ok

    def fic_ratio(self):
        r = np.zeros(self.cfg.n_ensembles, np.int32)
        self._chk(self.lib.dabphy_get_fic_ratio(self.h, _p(r)))
        return r

    def msc(self, idx):
        """-> (out [B][4F][bytes], first_valid [B]); rows [first_valid[b], self.msc_rows[b]) are the batch's logical frames"""
        B, F = self.cfg.n_ensembles, self._last
        out = np.zeros((B, 4 * F, self._sub_bytes[idx]), np.uint8); fv = np.zeros(B, np.int32); self.msc_rows = np.zeros(B, np.int32)
        self._chk(self.lib.dabphy_get_msc(self.h, idx, _p(out), C.c_size_t(out.nbytes), _p(fv), _p(self.msc_rows)))
        return out, fv

    def config(self):
        c = Config(C.sizeof(Config)); self._chk(self.lib.dabphy_get_config_v2(self.h, C.byref(c))); return c

    def demod_chunk(self):
        return self.config().demod_chunk

    def set_options(self, fft_placement=2, freqsync_method=2, disable_coarse=False):
        """RadioReceiver::setReceiverOptions at run time; returns True when the change restarted the synchroniser"""
        r = C.c_int32(0)
        self._chk(self.lib.dabphy_set_options(self.h, fft_placement, freqsync_method, int(disable_coarse), C.byref(r)))
        return bool(r.value)

    def ratio_lag(self):
        """(frames whose coarse-corrector decision used a stale FIC ratio, frame number of the first one or -1) per ensemble"""
        n = np.zeros(self.cfg.n_ensembles, np.int32); f = np.zeros(self.cfg.n_ensembles, np.int64)
        self._chk(self.lib.dabphy_get_ratio_lag(self.h, _p(n), _p(f)))
        return n, f

    def ratio_lag_effect(self):
        """(stale coarse-corrector decisions that can have changed anything, frame number of the first one or -1) per ensemble"""
        n = np.zeros(self.cfg.n_ensembles, np.int32); f = np.zeros(self.cfg.n_ensembles, np.int64)
        self._chk(self.lib.dabphy_get_ratio_lag_effect(self.h, _p(n), _p(f)))
        return n, f

    def scan_stats(self):
        a = np.zeros(self.cfg.n_ensembles, np.int32); f = np.zeros(self.cfg.n_ensembles, np.int32)
        self._chk(self.lib.dabphy_get_scan_stats(self.h, _p(a), _p(f)))
        return a, f

    def fibs_device(self):
        """(fib [B][F][12][32], crc_ok [B][F][12]) as torch uint8 tensors aliasing the library's HBM buffers (valid until the next
        process()); for device-side consumers such as the RCCL gather of the multi-GPU bench"""
        import torch
        B, F = self.cfg.n_ensembles, self._last
        pf = C.c_void_p(); po = C.c_void_p()
        self._chk(self.lib.dabphy_get_fibs_device(self.h, C.byref(pf), C.byref(po)))

        class _Dev:
            def __init__(self, ptr, shape):
                self.__cuda_array_interface__ = {"shape": shape, "typestr": "|u1", "data": (ptr, False), "version": 2}
        dev = "cuda:%d" % self.cfg.device
        return (torch.as_tensor(_Dev(pf.value, (B, F, 12, 32)), device=dev), torch.as_tensor(_Dev(po.value, (B, F, 12)), device=dev))

    def impulse_response(self):
        B, F = self.cfg.n_ensembles, self._last
        out = np.zeros((B, F, 2048), np.float32)
        self._chk(self.lib.dabphy_get_impulse_response(self.h, _p(out)))
        return out

    def null_symbols(self):
        out = np.zeros((self.cfg.n_ensembles, self._last, 2656), np.complex64)
        self._chk(self.lib.dabphy_get_null_symbols(self.h, _p(out)))
        return out

    def constellation(self):
        B, F = self.cfg.n_ensembles, self._last
        out = np.zeros((B, F, 1200), np.complex64)
        self._chk(self.lib.dabphy_get_constellation(self.h, _p(out)))
        return out

    def soft_bits(self, ens, frame):
        out = np.zeros((75, 3072), np.int8)
        self._chk(self.lib.dabphy_get_soft_bits(self.h, ens, frame, _p(out)))
        return out


class FrameInfo(C.Structure):
    _fields_ = [("sample_pos", C.c_int64), ("frame_no", C.c_int64), ("start_index", C.c_int32), ("valid", C.c_int32),
                ("fine_corrector", C.c_int32), ("coarse_corrector", C.c_int32), ("snr", C.c_float)]


def _rs_superframes(self, sf, s_per_sf):
    sf = np.ascontiguousarray(sf, np.uint8).reshape(-1, 120 * s_per_sf).copy()
    n = sf.shape[0]; corr = np.zeros(n, np.int32); unc = np.zeros(n, np.int32)
    self._chk(self.lib.dabphy_rs_superframes(self.h, _p(sf), s_per_sf, n, _p(corr), _p(unc)))
    return sf, corr, unc


def _rs_decode_msc(self, subch_index, first_cif):
    B = self.cfg.n_ensembles
    fc = np.ascontiguousarray(first_cif, np.int32).reshape(B)
    corr = np.zeros(B, np.int32); unc = np.zeros(B, np.int32)
    self._chk(self.lib.dabphy_rs_decode_msc(self.h, int(subch_index), _p(fc), _p(corr), _p(unc)))
    return corr, unc


def _set_profiling(self, on=True):
    self._chk(self.lib.dabphy_set_profiling(self.h, int(on)))


def _stage_times(self):
    ms = np.zeros(7, np.float32)
    self._chk(self.lib.dabphy_get_stage_times(self.h, _p(ms)))
    return dict(zip(["sync", "demod", "snr", "fic", "msc_gather", "msc_viterbi", "rs"], [float(v) for v in ms]))


DabPhy.rs_superframes = _rs_superframes
DabPhy.rs_decode_msc = _rs_decode_msc
DabPhy.set_profiling = _set_profiling
DabPhy.stage_times = _stage_times
