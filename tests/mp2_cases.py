"""Streams of logical frames for the MP2 frame-check tests (tests/test_mp2_vs_ref.py, test_emu_mp2.py, test_gpu_mp2.py): clean Layer II
streams over the bit rates, sampling rates and channel modes DAB uses, and the same streams damaged the ways a receiver meets."""
import numpy as np

from welle_io_amd import synth


def clean(bitrate, rate=48000, mode="stereo", mode_ext=0, n=24, seed=0):
    """n logical frames (3 x bitrate bytes each) of back-to-back Layer II frames -> (bytes, frame_len)"""
    rng = np.random.RandomState(seed)
    per = 2 if rate == 24000 else 1
    frames = b"".join(synth.make_mp2_frame(bitrate, rng, rate, mode, mode_ext) for _ in range((n + per - 1) // per))
    return frames[:n * 3 * bitrate], 3 * bitrate


def damage(stream, fl, kind, k=5, seed=0):
    """the stream with logical frame k damaged (every kind leaves whole logical frames: `drop` / `midstart` remove one)"""
    b = bytearray(stream)
    o = k * fl
    rng = np.random.RandomState(seed)
    if kind == "crc_flip":          # a bit of the allocation (CRC-covered)
        b[o + 6] ^= 0x80
    elif kind == "header_crc_flip":  # header byte 3 (covered by the CRC, decodes the same)
        b[o + 3] ^= 0x08
    elif kind == "uncovered_flip":  # bytes the CRC does not cover: samples, F-PAD
        b[o + fl - 5] ^= 0x10; b[o + fl - 1] ^= 0x01
    elif kind == "sync":
        b[o + 1] ^= 0x40
    elif kind == "sync_byte":
        b[o] = 0x12
    elif kind == "bitrate":         # another valid bit rate: wrong frame size, compatible header
        b[o + 2] ^= 0x10
    elif kind == "bitrate_bad":     # 1111
        b[o + 2] |= 0xF0
    elif kind == "samplerate":      # 44.1 / 32 kHz: no output format for it
        b[o + 2] ^= 0x04
    elif kind == "samplerate_bad":  # 11
        b[o + 2] |= 0x0C
    elif kind == "layer":           # Layer I
        b[o + 1] ^= 0x02
    elif kind == "layer_bad":       # 00
        b[o + 1] &= 0xF9
    elif kind == "TAG":
        b[o:o + 3] = b"TAG"
    elif kind == "ID3":
        b[o:o + 3] = b"ID3"
    elif kind == "false_sync":      # a header planted in the payload of frame k
        b[o + 40:o + 44] = b[o:o + 4]
    elif kind == "resync_false_sync":   # a damaged header, and a planted one that the resync then finds first
        b[o + 40:o + 44] = b[o:o + 4]; b[o + 1] ^= 0x40
    elif kind == "drop":
        del b[o:o + fl]
    elif kind == "midstart":        # the stream starts one logical frame in (mid-frame for LSF)
        del b[:fl]
    elif kind == "noise":           # a few random bit errors anywhere
        for _ in range(6):
            b[rng.randint(len(b))] ^= 1 << rng.randint(8)
    elif kind == "junk_start":      # the first logical frame is noise
        b[:fl] = rng.randint(0, 256, fl).astype(np.uint8).tobytes()
    else:
        raise ValueError(kind)
    return bytes(b)


MP1_RATES = (32, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 384)
LSF_RATES = (8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160)
MODES = (("stereo", 0), ("joint", 0), ("joint", 1), ("joint", 2), ("joint", 3), ("dual", 0), ("mono", 0))
DAMAGES = ("crc_flip", "header_crc_flip", "uncovered_flip", "sync", "sync_byte", "bitrate", "bitrate_bad", "samplerate", "samplerate_bad",
           "layer", "layer_bad", "TAG", "ID3", "false_sync", "resync_false_sync", "drop", "midstart", "noise", "junk_start")


def cases():
    """[(name, stream, frame_len)]"""
    out = []
    for i, br in enumerate(MP1_RATES):
        mode, ext = MODES[i % len(MODES)]
        if mode == "joint" and br // 2 < 56:
            ext = min(ext, 1)           # (bound <= sblimit = 8: see below)
        s, fl = clean(br, 48000, mode, ext, seed=br)
        out.append(("mp1_%d_%s%d" % (br, mode, ext), s, fl))
    # joint stereo with a bound beyond the sub-band limit (64 kbit/s: table B.2c, 8 sub-bands): CheckCRC reads past its nbal table there
    # (dab_decoder.cpp:213-225), which is not restated -- unverified from the first frame returned
    s, fl = clean(64, 48000, "joint", 3, seed=5)
    out.append(("mp1_64_joint3_beyond", s, fl))
    for mode, ext in MODES:
        s, fl = clean(192, 48000, mode, ext, seed=7 + ext)
        out.append(("mp1_192_%s%d" % (mode, ext), s, fl))
    for i, br in enumerate(LSF_RATES):
        mode, ext = MODES[(i + 3) % len(MODES)]
        s, fl = clean(br, 24000, mode, ext, seed=100 + br)
        out.append(("lsf_%d_%s%d" % (br, mode, ext), s, fl))
    for rate, br, mode, ext in ((48000, 128, "joint", 2), (48000, 48, "mono", 0), (24000, 64, "stereo", 0), (24000, 16, "mono", 0)):
        for kind in DAMAGES:
            for k in ((0, 5) if kind in ("crc_flip", "sync", "bitrate", "TAG", "layer") else (5,)):
                s, fl = clean(br, rate, mode, ext, seed=br * 3 + k)
                out.append(("%s_%d_%s_k%d" % ("mp1" if rate == 48000 else "lsf", br, kind, k), damage(s, fl, kind, k, seed=k), fl))
    return out


def long_cases():
    """streams of 300 logical frames: many ring chunks and CRC rounds per call, damage far from the start"""
    out = []
    for rate, br, mode, ext in ((48000, 384, "stereo", 0), (48000, 64, "mono", 0), (24000, 8, "stereo", 0), (24000, 160, "joint", 3)):
        s, fl = clean(br, rate, mode, ext, n=300, seed=br + 1)
        out.append(("long_%d_%d" % (rate, br), s, fl))
        for kind, k in (("sync", 150), ("crc_flip", 201), ("drop", 77), ("resync_false_sync", 250)):
            out.append(("long_%d_%d_%s_k%d" % (rate, br, kind, k), damage(s, fl, kind, k, seed=k), fl))
    return out
