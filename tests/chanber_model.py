"""Model of the channel BER pass (include/dabphy.h "Channel BER", k_chanber.hip), written from EN 300 401 clause 11 with the
transmitter's own encoder (synth.conv_encode) and puncturing (synth.puncture_mask): the decoded bits of a code word are encoded again
and compared with the signs of the soft bits at the positions that were transmitted.

A code word's soft bits are given as the decoder reads them: the PUNCTURED stream, input bit u at index u; `present` says which of
them exist at all (a row of the time de-interleaver from before the stream, a frame that was not demodulated)."""
import numpy as np

import refapi as R
from welle_io_amd import synth

_MASKS = {}


def segments_of(po):
    """(blocks of 128 bits, PI index) of a protection record's L / PI arrays (the oracle's, refapi.OrcProt): what synth.puncture_mask takes"""
    return [(int(po.L[i]), int(po.PI[i])) for i in range(4) if po.L[i] > 0 and po.PI[i] > 0]


def mask_of(po):
    """which of the 4 * nbits + 24 mother-code bits the profile transmits (the 24 tail bits take PI_X: 12 of them)"""
    key = (po.nbits, tuple(po.L), tuple(po.PI))
    if key not in _MASKS:
        m = synth.puncture_mask(segments_of(po), po.nbits)
        m.setflags(write=False)
        _MASKS[key] = m
    return _MASKS[key]


def transmitted_bits(po):
    """soft bits a code word of the profile is compared on at most (a UEP sub-channel carries padding behind them)"""
    return int(mask_of(po).sum())


def reencode(po, decoded, dedispersed=True):
    """decoded bytes (MSB first, as the getters return them) -> the coded bits at the transmitted positions"""
    bits = np.unpackbits(np.frombuffer(bytes(decoded), np.uint8))[:po.nbits]
    assert len(bits) == po.nbits
    if dedispersed:
        bits = bits ^ synth.prbs_cached(po.nbits)
    return synth.conv_encode(bits)[mask_of(po)]


def counts(po, soft, decoded, present=None, dedispersed=True):
    """-> (errors, compared) of ONE code word: soft = its punctured soft bits (int8, at least the transmitted ones)"""
    coded = reencode(po, decoded, dedispersed)
    s = np.asarray(soft, np.int8)[:len(coded)].astype(np.int32)
    assert len(s) == len(coded)
    cmp = s != 0
    if present is not None:
        cmp &= np.asarray(present, bool)[:len(coded)]
    hard = (s > 0).astype(np.uint8)                     # +127 = coded bit 1; -128 is negative like -127
    return int(((hard != coded) & cmp).sum()), int(cmp.sum())


def counts_many(po, soft, decoded):
    """[n][input bits], [n][nbits / 8] -> [n][2]"""
    return np.array([counts(po, soft[i], decoded[i]) for i in range(len(soft))], np.int64).reshape(-1, 2)


def fic_counts(po_fic, frame_soft, fibs):
    """one frame: soft [75][3072] (symbols 1..3 first), fibs [12][32] -> [4][2]"""
    s = np.asarray(frame_soft, np.int8).reshape(-1)[:9216].reshape(4, 2304)
    f = np.asarray(fibs, np.uint8).reshape(4, 96)
    return np.array([counts(po_fic, s[q], f[q]) for q in range(4)], np.int64)


def msc_row_soft(soft_frames, c, start_cu, n_in):
    """punctured soft bits of the logical frame that CIF c's arrival emits: input bit u comes from CIF c - 16 + TI_MAP[u & 15]
    (dab-audio.cpp:113,138-143).  soft_frames[k] = frame k's [75][3072] soft bits; -> (soft [n_in], present [n_in])"""
    u = np.arange(n_in)
    src = c - 16 + synth.TI_MAP[u & 15]
    out = np.zeros(n_in, np.int8); present = np.zeros(n_in, bool)
    for cs in np.unique(src):
        if cs < 0 or (cs >> 2) >= len(soft_frames) or soft_frames[cs >> 2] is None:
            continue
        cif = np.asarray(soft_frames[cs >> 2], np.int8).reshape(-1)[(3 + 18 * (cs & 3)) * 3072:(3 + 18 * (cs & 3) + 18) * 3072]
        sel = src == cs
        out[sel] = cif[start_cu * 64 + u[sel]]; present[sel] = True
    return out, present


def orc_fic():
    return R.orc_prot_fic()
