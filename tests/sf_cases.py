"""Generators for the DAB+ back end's tests (k_rs.hip, k_superframe.hip, dabphy_superframes.hip): superframes of every access-unit layout and bit rate
8 * s (s = 1 .. 48), the ways CheckSync (dabplus_decoder.cpp:171-215) rejects one, and Reed-Solomon words that walk the decoder's corner
paths on purpose -- roots in the padding, miscorrections that are written in full, errors at the edges of the shortened code, zero
data, S0 = 0 -- which random error patterns meet about once in ten thousand words."""
import numpy as np

from welle_io_amd import synth

# (dac_rate, sbr) -> (access units, first start): dabplus_decoder.cpp:185-200
LAYOUTS = {(0, 1): (2, 5), (1, 1): (3, 6), (0, 0): (4, 8), (1, 0): (6, 11)}
REJECTS = ("zero_table", "fire", "order", "past_end", "all_zero")


def pack_starts(sf, starts):
    """the 12-bit start fields of access units 1 .. 5 into sf[3..10], as the layouts pack them (only the given ones are written)"""
    for k, a in enumerate(starts, 1):
        assert 0 <= a < 4096
        o = 3 + 3 * ((k - 1) // 2)
        if k & 1:
            sf[o] = a >> 4; sf[o + 1] = (int(sf[o + 1]) & 0x0F) | ((a & 0xF) << 4)
        else:
            sf[o + 1] = (int(sf[o + 1]) & 0xF0) | (a >> 8); sf[o + 2] = a & 0xFF


def make_superframe(bitrate, rng, layout, flags=0, au_lengths=None, reject=None):
    """a DAB+ superframe of 120 * s bytes (s = bitrate / 8 in 1 .. 48) in one of the four layouts: format byte (dac_rate, sbr and the
    low five bits `flags` = aac_channel_mode, ps, mpeg_surround), the start table as that layout packs it -- what the layout leaves
    unused of sf[3..10] stays random: it lies under the Fire code and must be ignored --, access units closed by CRC-16-CCITT, the Fire
    code over bytes 2..10, RS parity.  au_lengths: per access unit a length or None (shares what is left); 2 is a CRC over nothing,
    1 an access unit shorter than its CRC.  reject (always with valid RS parity): "zero_table", "fire", "order:k" (start k not above
    start k - 1, k = 1 .. access units - 1), "past_end" (last start at or beyond 110 * s; the 12-bit field cannot say that for
    s > 37: ValueError), "all_zero"."""
    s = bitrate // 8
    assert bitrate == 8 * s and 1 <= s <= 48
    n = 110 * s
    num_aus, a0 = LAYOUTS[tuple(layout)]
    sf = np.zeros(120 * s, np.uint8)
    if reject != "all_zero":
        data = rng.randint(0, 256, n).astype(np.uint8)
        lens = list(au_lengths) if au_lengths is not None else [None] * num_aus
        assert len(lens) == num_aus
        # the starts are 12-bit fields: everything but the last access unit has to end below 4096
        reach = min(n, 4090)
        free_i = [i for i, v in enumerate(lens) if v is None]
        left = reach - a0 - sum(v for v in lens if v is not None)
        assert left >= 3 * len(free_i), "access units do not fit"
        w = rng.uniform(0.5, 1.5, len(free_i))
        share = [3 + int((left - 3 * len(free_i)) * v / w.sum()) for v in w]
        if free_i:
            share[-1] += left - sum(share)
        for i, v in zip(free_i, share):
            lens[i] = v
        lens[-1] += n - reach
        assert sum(lens) == n - a0 and lens[-1] >= 1
        starts = [a0]
        for v in lens[:-1]:
            starts.append(starts[-1] + v)
        for lo, ln in zip(starts, lens):
            if ln >= 3:
                data[lo] |= 0xE0                                   # ID_END first: nothing an AAC decoder would half accept (synth.make_superframe)
            if ln >= 2:
                c = synth.crc16(data[lo:lo + ln - 2], True, True, 0x1021)
                data[lo + ln - 2] = c >> 8; data[lo + ln - 1] = c & 0xFF
        table = starts[1:]
        if reject == "zero_table":
            table = None
        elif reject and reject.startswith("order:"):
            k = int(reject[6:])
            assert 1 <= k < num_aus
            table[k - 1] = starts[k - 1] - int(rng.randint(0, 2)) * int(rng.randint(0, starts[k - 1] + 1))      # equal to, or anywhere below, its predecessor
        elif reject == "past_end":
            if n > 4095:
                raise ValueError("a start of 110 * %d does not fit the 12-bit field" % s)
            table[-1] = min(4095, n + int(rng.randint(0, 3)) * int(rng.randint(0, 40)))
        elif reject not in (None, "fire"):
            raise ValueError(reject)
        data[2] = (layout[0] << 6) | (layout[1] << 5) | (flags & 0x1F)
        if table is None:
            data[3] = 0; data[4] = 0
        else:
            pack_starts(data, table)
        c = synth.crc16(data[2:11], False, False, 0x782F)
        if reject == "fire":
            c ^= 1 << int(rng.randint(0, 16))
        data[0] = c >> 8; data[1] = c & 0xFF
        sf[:n] = data
        sf[n:] = synth.rs_parity(data.reshape(110, s)).reshape(-1)
    return sf


# ---- one ensemble's sub-channels meet different variants in different superframes
_L2, _L3, _L4, _L6 = (0, 1), (1, 1), (0, 0), (1, 0)
# (layout, flags, access-unit lengths, reject, damage); "order" takes its k from the sub-channel
TABLE = (
    (_L3, 0x02, None, None, None),
    (_L2, 0x1F, None, None, None),
    (_L4, 0x00, (2, None, None, None), None, None),
    (_L6, 0x11, None, None, "within"),
    (_L2, 0x09, (None, 2), None, None),
    (_L3, 0x04, (None, 1, None), None, None),
    (_L6, 0x00, (None, 2, 1, None, None, 2), None, None),
    (_L4, 0x1A, None, None, "beyond"),
    (_L2, 0x01, (1, None), None, "within"),
    (_L3, 0x03, None, None, None),
    # ten superframes in a row that synchronise (a batch of up to six frames lies inside them whatever its phase: the wide pass settles
    # it), then the ones that do not
    (_L3, 0x02, None, "zero_table", None),
    (_L6, 0x0A, None, None, "header"),
    (_L6, 0x02, None, "fire", None),
    (None, 0x02, None, "order", None),
    (_L4, 0x02, None, "past_end", None),
    (_L3, 0x02, None, "all_zero", None),
)
_ORDER_CASES = tuple((lay, k) for lay in (_L2, _L3, _L4, _L6) for k in range(1, LAYOUTS[lay][0]))


def schedule(subch_id, q):
    """(layout, flags, au_lengths, reject, damage) of superframe q of a sub-channel: a fixed table stepped by q + subch_id; damage =
    byte errors within ("within") or beyond ("beyond") what RS(120,110) corrects, or a header column beyond repair ("header")"""
    layout, flags, au_lengths, reject, damage = TABLE[(q + subch_id) % len(TABLE)]
    if reject == "order":
        layout, k = _ORDER_CASES[(5 * subch_id + q) % len(_ORDER_CASES)]
        reject = "order:%d" % k
    return layout, flags, au_lengths, reject, damage


def apply_damage(sf, s, damage):
    if damage == "within":
        for j in range(5):
            sf[(7 + 9 * j) * s + j % s] ^= 0x21 * (j + 1)
        for j in range(3 if s > 1 else 0):
            sf[(100 + j) * s + (s - 1)] ^= 0x80 >> j
    elif damage == "beyond":
        c = min(3, s - 1)
        for j in range(12):
            sf[(12 + 2 * j) * s + c] ^= 0x33
        sf[60 * s] ^= 0x5A
    elif damage == "header":
        for j in range(4, 11):
            sf[j * s] ^= 0x81
    elif damage is not None:
        raise ValueError(damage)


def scheduled_superframe(sc, q, seed):
    """superframe q of sub-channel sc as `schedule` wants it (past_end where the bit rate cannot say it: a start table out of order)"""
    layout, flags, au_lengths, reject, damage = schedule(sc.subch_id, q)
    rng = np.random.RandomState(seed * 1000003 + sc.subch_id * 1009 + q)
    if reject == "past_end" and 110 * (sc.bitrate // 8) > 4095:
        reject = "order:1"
    sf = make_superframe(sc.bitrate, rng, layout, flags, au_lengths, reject)
    apply_damage(sf, sc.bitrate // 8, damage)
    return sf


def payload_fn(period_cifs=80, seed=0):
    """payload_fn for synth.EnsembleTx over `schedule`, periodic with period_cifs"""
    assert period_cifs % 5 == 0 and period_cifs % 16 == 0
    cache = {}

    def fn(sc, r):
        r = r % period_cifs
        key = (sc.subch_id, r // 5)
        if key not in cache:
            cache[key] = scheduled_superframe(sc, r // 5, seed)
        fb = sc.frame_bytes
        return cache[key][(r % 5) * fb:(r % 5 + 1) * fb].tobytes()
    return fn


# ---- GF(2^8), polynomial 0x11D: log / antilog tables written out here, independent of the encoder under synth and of the decoders
def _gf_tables():
    exp, log = [0] * 510, [0] * 256
    x = 1
    for i in range(255):
        exp[i] = exp[i + 255] = x; log[x] = i
        x <<= 1
        if x & 0x100:
            x ^= 0x11D
    return exp, log


GF_EXP, GF_LOG = _gf_tables()


def gf_mul(a, b):
    return GF_EXP[GF_LOG[a] + GF_LOG[b]] if a and b else 0


def gf_inv(a):
    return GF_EXP[255 - GF_LOG[a]]


def syndromes(word120):
    """S_i = c(alpha^i), i = 0 .. 9, of 120 transmitted bytes (byte pos = coefficient of x^(119 - pos))"""
    out = []
    for i in range(10):
        v = 0
        for pos, b in enumerate(word120):
            if b:
                v ^= GF_EXP[(GF_LOG[int(b)] + i * (119 - pos)) % 255]
        out.append(v)
    return out


def support_word(degrees, rng):
    """the code word of RS(255,245) (roots alpha^0 .. alpha^9) supported on the 11 given degrees: ten equations sum_j v_j alpha^(i d_j)
    = 0 in eleven unknowns, solved by elimination with the last unknown free.  The code is MDS: the solution is a line and nowhere zero.
    -> {degree: value}, scaled by a random non-zero factor"""
    degrees = list(degrees)
    assert len(degrees) == 11 and len(set(degrees)) == 11 and all(0 <= d < 255 for d in degrees)
    m = [[GF_EXP[(i * d) % 255] for d in degrees] for i in range(10)]              # columns 0..9 the unknowns, column 10 the free one's
    for c in range(10):
        p = next(r for r in range(c, 10) if m[r][c])
        m[c], m[p] = m[p], m[c]
        inv = gf_inv(m[c][c])
        m[c] = [gf_mul(v, inv) for v in m[c]]
        for r in range(10):
            if r != c and m[r][c]:
                f = m[r][c]
                m[r] = [a ^ gf_mul(f, b) for a, b in zip(m[r], m[c])]
    scale = int(rng.randint(1, 256))
    v = [gf_mul(m[r][10], scale) for r in range(10)] + [scale]                      # v_j + m[j][10] v_10 = 0, characteristic 2
    assert all(v)
    for i in range(10):
        acc = 0
        for d, x in zip(degrees, v):
            acc ^= GF_EXP[(GF_LOG[x] + i * d) % 255]
        assert acc == 0
    return dict(zip(degrees, v))


def random_codeword(rng):
    d = rng.randint(0, 256, 110).astype(np.uint8)
    return np.concatenate([d, synth.rs_parity(d)])


EDGE = (0, 1, 108, 109, 110, 111, 118, 119)
RANDOM_WEIGHTS = (0, 0, 1, 2, 3, 4, 5, 5, 6, 6, 7, 8, 10, 12)


def directed_sets(seed=5, n=16):
    """{name: (received [n][120], sent [n][120])}: every word a valid random code word plus the pattern.
    pad_roots:k  (k = 1 .. 5) the nearest code word differs from the received one in k bytes of the PADDING: k corrections counted, none written
    applied:j    (j = 1 .. 5) 11 - j bytes of a weight-11 code word inside the 120 transmitted: the decoder writes the other j -- a miscorrection
                 applied in full
    edge         1 .. 5 errors confined to positions 0, 1, 108, 109, 110, 111, 118, 119 (both ends of the data, both ends of the parity),
                 then six there, then five there and one anywhere
    zero         the all-zero word with 1 .. 6 errors; error values that XOR to zero (S0 = 0) on 2 .. 6 positions; errors in the parity only
    random       0 .. 12 errors anywhere, the weights of check_rs_random"""
    rng = np.random.RandomState(seed)
    sets = {}

    def add(name, rx, tx):
        sets[name] = (np.array(rx, np.uint8), np.array(tx, np.uint8))
    for k in range(1, 6):
        rx, tx = [], []
        for _ in range(n):
            deg = list(rng.choice(np.arange(120, 255), k, replace=False)) + list(rng.choice(120, 11 - k, replace=False))
            w = support_word(deg, rng)
            c = random_codeword(rng); r = c.copy()
            for d, v in w.items():
                if d < 120:
                    r[119 - d] ^= v
            rx.append(r); tx.append(c)
        add("pad_roots:%d" % k, rx, tx)
    for j in range(1, 6):
        rx, tx = [], []
        for i in range(n):
            # (some at the very ends of the word)
            deg = list(rng.choice(120, 11, replace=False)) if i % 4 else [119, 0, 10, 9] + list(rng.choice(np.arange(11, 119), 7, replace=False))
            w = support_word(deg, rng)
            c = random_codeword(rng); r = c.copy()
            for d in list(rng.permutation(deg))[:11 - j]:
                r[119 - d] ^= w[d]
            rx.append(r); tx.append(c)
        add("applied:%d" % j, rx, tx)
    rx, tx = [], []
    for i in range(max(n, 24)):
        c = random_codeword(rng); r = c.copy()
        if i % 8 < 5:
            pos = rng.choice(EDGE, i % 8 + 1, replace=False)
        elif i % 8 < 7:
            pos = rng.choice(EDGE, 6, replace=False)
        else:
            pos = np.concatenate([rng.choice(EDGE, 5, replace=False), rng.choice(np.arange(2, 108), 1)])
        r[pos] ^= rng.randint(1, 256, len(pos)).astype(np.uint8)
        rx.append(r); tx.append(c)
    add("edge", rx, tx)
    rx, tx = [], []
    for i in range(max(n, 24)):
        kind = i % 3
        if kind == 0:                                          # zero data: every table look-up of the syndrome loop reads index_of[0]
            c = np.zeros(120, np.uint8); r = c.copy()
            pos = rng.choice(120, i // 3 % 6 + 1, replace=False)
            r[pos] ^= rng.randint(1, 256, len(pos)).astype(np.uint8)
        elif kind == 1:                                        # S0 = 0
            c = random_codeword(rng) if i % 2 else np.zeros(120, np.uint8)
            r = c.copy()
            pos = rng.choice(120, i // 3 % 5 + 2, replace=False)
            v = rng.randint(1, 256, len(pos)).astype(np.uint8)
            v[-1] = np.bitwise_xor.reduce(v[:-1])
            if v[-1] == 0:
                v[0] ^= 1; v[-1] = 1
            r[pos] ^= v
            assert np.bitwise_xor.reduce(r ^ c) == 0
        else:                                                  # the parity bytes only
            c = random_codeword(rng); r = c.copy()
            pos = 110 + rng.choice(10, i // 3 % 6 + 1, replace=False)
            r[pos] ^= rng.randint(1, 256, len(pos)).astype(np.uint8)
        rx.append(r); tx.append(c)
    add("zero", rx, tx)
    rx, tx = [], []
    for i in range(max(n, 2 * len(RANDOM_WEIGHTS))):
        c = random_codeword(rng); r = c.copy()
        w = RANDOM_WEIGHTS[i % len(RANDOM_WEIGHTS)]
        pos = rng.choice(120, w, replace=False)
        r[pos] ^= rng.randint(1, 256, w).astype(np.uint8)
        rx.append(r); tx.append(c)
    add("random", rx, tx)
    return sets


def pack_columns(words, s, rng):
    """code word i into column i % s of superframe i // s ([n_sf][120 * s]); the columns left over in the last superframe are clean
    random code words"""
    words = list(words)
    while len(words) % s:
        words.append(random_codeword(rng))
    w = np.array(words, np.uint8).reshape(-1, s, 120)
    return np.ascontiguousarray(w.transpose(0, 2, 1)).reshape(-1, 120 * s)


def mixed_superframe(sets, name, s, rng):
    """one superframe of s columns that mixes the classes: clean, corrected, given up / miscorrected, counted-not-applied and the set's own
    words side by side, so that the lanes of a wave take different paths through the decoder"""
    own = sets[name][0]
    pools = [None, sets["edge"][0][:5], sets["random"][0][len(RANDOM_WEIGHTS) - 4:len(RANDOM_WEIGHTS)], sets["applied:3"][0], own, sets["pad_roots:2"][0], own]
    cols = []
    for c in range(s):
        p = pools[c % len(pools)] if s > 1 else own
        cols.append(random_codeword(rng) if p is None else p[int(rng.randint(0, len(p)))])
    return np.ascontiguousarray(np.array(cols, np.uint8).T).reshape(120 * s)
