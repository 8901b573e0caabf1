"""Plain restatement of the MP2 frame check (csrc/k_mp2.hip) for the tests: what the reference's MP2Decoder::Feed reports when
it is fed one logical frame per call (dab_decoder.cpp:114-250, decoder_adapter.cpp:55-77), with mpg123's feed reader and
frame parser restated as they act on such a stream (libs/mpg123: readers.c bufferchain, parse.c read_frame / skip_junk /
wetwork / do_readahead / decode_header, libmpg123.c get_next_frame / decode_update).

Paths that are not restated end the check of a stream: `first_unverified` is the logical frame at which one was taken (a
header of another layer or sampling rate, free format, a Frankenstein stream, ID3 / TAG / APE / RIFF tags, CRC-covered bits
beyond the frame, a joint-stereo bound beyond the nbal table); the events and error counts of that frame and all later ones are
not claimed and not returned."""
import numpy as np

from welle_io_amd.synth import MP2_BITRATES, MP2_NBAL, mp2_table_index

BLOCK = 4096            # mpg123's feed buffer blocks (frame.c: feedbuffer)
FORGET_INTERVAL = 1024  # parse.c:1101
NEED_MORE = -10
GOOD, BAD, AGAIN, RESYNC = 1, 0, 2, 3
FREQS = (44100, 48000, 32000, 22050, 24000, 16000, 11025, 12000, 8000)
TABSEL = (((0, 32, 64, 96, 128, 160, 192, 224, 256, 288, 320, 352, 384, 416, 448),
           (0,) + MP2_BITRATES[0][1:],
           (0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320)),
          ((0, 32, 48, 56, 64, 80, 96, 112, 128, 144, 160, 176, 192, 224, 256),
           MP2_BITRATES[1],
           MP2_BITRATES[1]))
CMPMASK = 0xFFE00000 | 0x00180000 | 0x00060000 | 0x00000C00


class Unverified(Exception):
    pass


def head_check(h):
    return (h & 0xFFE00000) == 0xFFE00000 and (h >> 17) & 3 != 0 and (h >> 12) & 15 != 15 and (h >> 10) & 3 != 3


def head_compatible(a, b):
    return (a & CMPMASK) == (b & CMPMASK) and (((a >> 6) & 3) == 3) == (((b >> 6) & 3) == 3)


def header_info(h):
    """(lay, lsf, mpeg25, sampling_frequency index, framesize after the header) as decode_header sets them"""
    lay = 4 - ((h >> 17) & 3)
    ver = (h >> 19) & 3
    if ver & 2:
        lsf, m25 = (0 if ver & 1 else 1), 0
        sf = ((h >> 10) & 3) + lsf * 3
    else:
        lsf, m25, sf = 1, 1, 6 + ((h >> 10) & 3)
    bri, pad = (h >> 12) & 15, (h >> 9) & 1
    if bri == 0:
        raise Unverified("free format")
    if lay == 1:
        fs = ((TABSEL[lsf][0][bri] * 12000 // FREQS[sf]) + pad) * 4 - 4
    elif lay == 2:
        fs = TABSEL[lsf][1][bri] * 144000 // FREQS[sf] + pad - 4
    else:
        fs = TABSEL[lsf][2][bri] * 144000 // (FREQS[sf] << lsf) + pad - 4
    return lay, lsf, m25, sf, fs


def crc_ok(h, body):
    """MP2Decoder::CheckCRC (dab_decoder.cpp:195-250); body = the framesize bytes after the header"""
    if (h >> 16) & 1:
        return False                                  # no CRC: counted as a failure
    lay, lsf, m25, sf, fs = header_info(h)
    mode, mode_ext = (h >> 6) & 3, (h >> 4) & 3
    nch = 1 if mode == 3 else 2
    bitrate = TABSEL[lsf][lay - 1][(h >> 12) & 15]
    version1 = not lsf and not m25
    nbal = MP2_NBAL[mp2_table_index(not version1, bitrate, nch)]
    sblimit = len(nbal)
    bound = (mode_ext + 1) * 4 if mode == 1 else sblimit
    if bound > sblimit:
        raise Unverified("joint stereo bound beyond the nbal table: the reference reads past it")
    bits = np.unpackbits(np.frombuffer(bytes(body[2:]), np.uint8))
    p = n = 0
    for sb in range(sblimit):
        for ch in range(nch if sb < bound else 1):
            if p + nbal[sb] > len(bits):
                return False                          # BitReader ran out
            v = int(bits[p:p + nbal[sb]].dot(1 << np.arange(nbal[sb] - 1, -1, -1)))
            p += nbal[sb]
            n += nbal[sb] + ((2 if sb < bound else 2 * nch) if v else 0)
    if n > len(bits):
        raise Unverified("CRC-covered bits run past the frame")
    crc = 0xFFFF
    seq = [(int(body_b) >> (7 - i)) & 1 for body_b in ((h >> 8) & 0xFF, h & 0xFF) for i in range(8)] + [int(b) for b in bits[:n]]
    for b in seq:
        fb = ((crc >> 15) & 1) ^ b
        crc = (crc << 1) & 0xFFFF
        if fb:
            crc ^= 0x8005
    return crc == (body[0] << 8 | body[1])


class Mp2Model:
    """one service: feed() one logical frame at a time"""

    def __init__(self):
        self.data = bytearray()
        self.pos = self.firstpos = self.ks = 0        # read position, where a NEED_MORE rewinds to, start of the first kept block
        self.firsthead = self.oldhead = 0
        self.header_change = 0
        self.framesize = 0
        self.fmt = None
        self.scf_crc_len = -1
        self.feed_no = -1
        self.events = []          # (feed, offset, header, crc_ok, new_format, scf_crc_len, fpad0, fpad1)
        self.errors = []
        self.first_unverified = -1
        self.skipped = 0          # bytes passed over by the resync walks (skip_junk / wetwork shifts)

    # --- the feed reader (readers.c: bc_give / bc_skip / bc_seekback / bc_forget / bc_need_more) ---
    def _more(self):
        self.pos = self.firstpos
        return NEED_MORE

    def _give(self, n):
        if len(self.data) - self.pos < n:
            return self._more()
        b = self.data[self.pos:self.pos + n]
        self.pos += n
        return b

    def _back(self, n):
        if n >= 0:
            if self.pos - n >= self.ks:
                self.pos -= n
                return 0
            return -1
        return 0 if not isinstance(self._give(-n), int) else -1

    def _forget(self):
        if self.pos == len(self.data):
            self.ks = self.pos
        else:
            self.ks += BLOCK * ((self.pos - self.ks) // BLOCK)
        self.firstpos = self.pos

    def _head_read(self):
        b = self._give(4)
        return b if isinstance(b, int) else int.from_bytes(b, "big")

    def _shift(self, h, forget):
        b = self._give(1)
        if isinstance(b, int):
            return b
        self.skipped += 1
        h = ((h << 8) | b[0]) & 0xFFFFFFFF
        if forget and not self._back(4):
            self._forget()
            self._back(-4)
        return h

    # --- parse.c ---
    def _skip_junk(self, h):
        if (h & 0xFFFFFF00) == 0x49443300 or h == 0x52494646:
            raise Unverified("ID3v2 / RIFF at the start")
        forgetcount = 0
        while True:
            forgetcount += 1
            if forgetcount > FORGET_INTERVAL:
                forgetcount = 0
            h = self._shift(h, not forgetcount)
            if h == NEED_MORE:
                return NEED_MORE, 0
            if head_check(h):
                self._decode(h)
                return GOOD, h

    def _wetwork(self, h):
        if (h & 0xFFFFFF00) in (0x54414700, 0x49443300) or h == 0x41504554:
            raise Unverified("TAG / ID3 / APET header")
        forgetcount = 0
        while True:
            forgetcount += 1
            if forgetcount > FORGET_INTERVAL:
                forgetcount = 0
            h = self._shift(h, not forgetcount)
            if h == NEED_MORE:
                return NEED_MORE, 0
            if head_check(h):
                self.oldhead = 0
                return RESYNC, h

    def _decode(self, h):
        self.framesize = header_info(h)[4]

    def _readahead(self, h):
        start = self.pos
        if isinstance(self._give(self.framesize), int):
            return NEED_MORE
        nh = self._head_read()
        self._back(self.pos - start)
        if nh == NEED_MORE:
            return NEED_MORE
        if not head_check(nh) or not head_compatible(h, nh):
            self.oldhead = 0
            self._back(3)
            return AGAIN
        return GOOD

    def _read_frame(self):
        oldsize = self.framesize
        state = "again"
        h = 0
        while True:
            if state == "again":
                self._forget()
                h = self._head_read()
                if h == NEED_MORE:
                    break
            state = "again"
            if not self.firsthead and not head_check(h):
                r, h = self._skip_junk(h)
                if r == NEED_MORE:
                    break
            if head_check(h):
                self._decode(h)
            else:
                r, h = self._wetwork(h)
                if r == NEED_MORE:
                    break
                state = "resync"
                continue
            if not self.firsthead:
                r = self._readahead(h)
                if r == NEED_MORE:
                    self._back(4)
                    break
                if r == AGAIN:
                    continue
            framepos = self.pos - 4
            body = self._give(self.framesize)
            if isinstance(body, int):
                break
            if not self.firsthead:
                self.firsthead = h
            self._forget()
            if self.header_change < 2:
                self.header_change = 2
                if self.oldhead:
                    if self.oldhead == h:
                        self.header_change = 0
                    elif head_compatible(self.oldhead, h):
                        self.header_change = 1
                    else:
                        raise Unverified("big change (Frankenstein stream)")
                elif self.firsthead and not head_compatible(self.firsthead, h):
                    raise Unverified("big change from the first header (Frankenstein stream)")
            self.oldhead = h
            return h, framepos, bytes(body)
        self._forget()
        self.framesize = oldsize
        return None

    def _frame(self, h, off, body):
        lay, lsf, m25, sf, fs = header_info(h)
        if lay != 2:
            raise Unverified("not Layer II")
        new_format = False
        if self.header_change > 1:
            self.header_change = 0
            rate, ch = FREQS[sf], 1 if (h >> 6) & 3 == 3 else 2
            if rate not in (48000, 24000):
                raise Unverified("no output format for this rate: the reference throws")
            if (rate, ch) != self.fmt:
                self.fmt = (rate, ch)
                new_format = True
        if new_format:
            bitrate = TABSEL[lsf][1][(h >> 12) & 15]
            self.scf_crc_len = 2 if (not lsf and not m25 and bitrate < (56 if (h >> 6) & 3 == 3 else 112)) else 4
        ok = crc_ok(h, body)
        return (self.feed_no, off, h, int(ok), int(new_format), self.scf_crc_len, body[-2], body[-1])

    def feed(self, chunk):
        self.feed_no += 1
        if self.first_unverified >= 0:
            self.errors.append(0)
            return
        self.data += bytes(chunk)
        n0 = len(self.events)
        err = 0
        try:
            while True:
                fr = self._read_frame()
                if fr is None:
                    break
                ev = self._frame(*fr)
                self.events.append(ev)
                err += 0 if ev[3] else 1
        except Unverified:
            self.first_unverified = self.feed_no
            del self.events[n0:]
            self.errors.append(0)
            return
        self.errors.append(err)


def run(frames, frame_len):
    """check a stream of logical frames (bytes, n * frame_len): (events, errors per logical frame, first_unverified, skipped)"""
    m = Mp2Model()
    for k in range(len(frames) // frame_len):
        m.feed(frames[k * frame_len:(k + 1) * frame_len])
    return m.events, m.errors, m.first_unverified, m.skipped
