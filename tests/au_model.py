"""The contract of the bulk access-unit drain (dabphy_set_au_drain, k_au.hip), in Python: what a consumer gets behind
SuperframeFilter::Feed (dabplus_decoder.cpp:121-138) from a service's filter events and corrected superframes (refapi.orc_superframe_run):
every access unit that passed its CRC, CRC stripped, in event and index order -- as AACDecoder::DecodeFrame receives it (RAW) or wrapped
into one LATM/LOAS AudioSyncStream frame as ProcessUntouchedStream builds it (:257-312).  tests/test_au_vs_ref.py pins the LOAS stream to the
real SuperframeFilter with an UntouchedStreamConsumer attached."""
import numpy as np

from welle_io_amd import capi


class BitWriter:
    """tools.cpp's BitWriter: bits most significant first, zero bits up to the byte boundary"""

    def __init__(self):
        self.bits = []

    def add(self, value, n):
        assert 0 <= value < (1 << n)
        self.bits.extend((value >> (n - 1 - i)) & 1 for i in range(n))

    def add_bytes(self, data):
        for b in data:
            self.add(int(b), 8)

    def data(self):
        bits = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(int("".join(map(str, bits[i:i + 8])), 2) for i in range(0, len(bits), 8))


def loas_frame(au, fmt):
    """ProcessUntouchedStream (dabplus_decoder.cpp:257-312) for one access unit `au` (CRC stripped) of a superframe with format byte fmt = sf[2]"""
    dac, sbr, stereo = bool(fmt & 0x40), bool(fmt & 0x20), bool(fmt & 0x10)
    core_sr = (6 if sbr else 3) if dac else (8 if sbr else 5)          # dabplus_decoder.h:55-57 GetCoreSrIndex: 24/48/16/32 kHz
    ch = 2 if stereo else 1                                            # :58-60 GetCoreChConfig
    ext_sr = 3 if dac else 5                                           # :61-63 GetExtensionSrIndex: 48/32 kHz
    w = BitWriter()
    w.add(0x2B7, 11)                # :266 syncword
    w.add(0, 13)                    # :267 audioMuxLengthBytes, written later
    w.add(0, 1)                     # :270 useSameStreamMux
    w.add(0, 1)                     # :273 audioMuxVersion
    w.add(1, 1)                     # :274 allStreamsSameTimeFraming
    w.add(0, 6)                     # :275 numSubFrames
    w.add(0, 4)                     # :276 numProgram
    w.add(0, 3)                     # :277 numLayer
    if sbr:                         # :280-286
        w.add(0b00101, 5); w.add(core_sr, 4); w.add(ch, 4); w.add(ext_sr, 4); w.add(0b00010, 5); w.add(0b100, 3)
    else:                           # :288-291
        w.add(0b00010, 5); w.add(core_sr, 4); w.add(ch, 4); w.add(0b100, 3)
    w.add(0, 3)                     # :294 frameLengthType
    w.add(0xFF, 8)                  # :295 latmBufferFullness
    w.add(0, 1); w.add(0, 1)        # :296-297 otherDataPresent, crcCheckPresent
    for _ in range(len(au) // 255):  # :300-302 PayloadLengthInfo
        w.add(0xFF, 8)
    w.add(len(au) % 255, 8)
    w.add_bytes(au)                 # :305 PayloadMux
    out = bytearray(w.data())
    n = len(out) - 3                # :308 WriteAudioMuxLengthBytes (tools.cpp: the 13 bits behind the sync word)
    assert n < (1 << 13)
    out[1] |= n >> 8; out[2] = n & 0xFF
    return bytes(out)


def au_duration_ms(fmt):
    """SuperframeFormat::GetAULengthMs (dabplus_decoder.h:67-69)"""
    dac, sbr = bool(fmt & 0x40), bool(fmt & 0x20)
    return (40 if sbr else 20) if dac else (60 if sbr else 30)


def model(events, sfs):
    """events / sfs as refapi.orc_superframe_run returns them -> (aus, raw, loas): aus = [(event number, cif, access unit index, sf[2],
    payload)] of everything the reference forwards, raw / loas = the service's byte streams in the two formats; failed = access units
    of synchronised superframes that the reference skips is aus' complement and returned as the fourth value"""
    aus, failed, k = [], 0, 0
    for n, e in enumerate(events):
        cif, _, _, sync, fmt, num_aus, starts, ok = e
        if not sync:
            continue
        sf = sfs[k]; k += 1
        for i in range(num_aus):
            lo, hi = starts[i], starts[i + 1]
            if ok >> i & 1:
                assert hi - lo >= 2
                aus.append((n, cif, i, fmt, bytes(sf[lo:hi - 2])))
            else:
                failed += 1
    raw = b"".join(a[4] for a in aus)
    loas = b"".join(loas_frame(a[4], a[3]) for a in aus)
    return aus, raw, loas, failed


def stream_of(aus, fmt):
    return b"".join(a[4] if fmt == capi.AU_RAW else loas_frame(a[4], a[3]) for a in aus)


def events_array(events):
    """the oracle's event tuples as dabphy_sf_event records, sf_slot = number of the synchronised superframe"""
    ev = np.zeros(len(events), capi.SF_EVENT_DTYPE)
    k = 0
    for n, e in enumerate(events):
        cif, corr, unc, sync, fmt, num_aus, starts, ok = e
        ev[n]["cif"] = cif; ev[n]["corrected"] = corr; ev[n]["uncorrectable"] = unc; ev[n]["sync"] = sync
        ev[n]["sf_slot"] = -1
        if sync:
            ev[n]["format"] = fmt; ev[n]["num_aus"] = num_aus; ev[n]["au_start"][:num_aus + 1] = starts; ev[n]["au_crc_ok"] = ok
            ev[n]["sf_slot"] = k; k += 1
    return ev
