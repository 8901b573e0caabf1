// welle.io_amd/csrc/rs_codec.h -- DAB+ Reed-Solomon RS(120,110) over GF(2^8): the device functions of the code, one thread per codeword.
//
// Replaces (reference file:line):
//   decode_rs_char / decode_rs.h         src/libs/fec/decode_rs.h:71-298  (KA9Q libfec, no erasures)
//   init_rs_char(8, 0x11D, 0, 1, 10, 135)  src/libs/fec/init_rs.h:6-103   (log/antilog tables)
//
// Syndromes -> locator (Massey) -> roots -> values (rs_correct120); corrected bytes, the corrected-symbol count and the
// "uncorrectable" verdict equal the reference's also for words beyond the correction capacity (miscorrections included).  What pins
// it, each against the oracle, which is pinned to decode_rs_char itself
// (tests/test_oracle_vs_ref.py): tests/golden rs vectors; random error patterns of weight 0 .. 12 at 1 .. 48 code words per superframe
// (check_rs_random); words built for the corner paths -- roots in the padding, miscorrections written in full, errors at the edges of
// the shortened code, zero data, S0 = 0 (check_rs_directed, tests/sf_cases.py); k_rs_msc by value on the class outputs of a stream
// (check_rs_decode_msc); the filter over the four access-unit layouts, every rejection rule and 8 .. 384 kbit/s
// (check_superframe_layouts); the syndromes as they are taken now -- from the word's remainder modulo the generator polynomial
// (rs_remainder120, rs_syndromes_from_remainder) -- by an error at every position, five and six errors through the same places and the
// corner words at 1, 8, 9 and 48 code words per superframe (tests/rs_remainder_cases.py).  The tables live in LDS.
// Callers: k_rs.hip (the bare RSDecoder seams) and k_superframe.hip (the DAB+ superframe filter).
#pragma once
#include "dabphy_kernels.h"

namespace dabphy {

constexpr int RS_NN = 255, RS_NROOTS = 10, RS_PAD = 135, RS_LEN = 120;       // (RS_NROOTS = 2t: ten syndromes, locator degree <= 10)

struct RsIo {                         // byte `pos` of codeword i
    uint8_t* base; size_t pos_stride;
    __device__ __forceinline__ uint8_t get(int pos) const { return base[(size_t)pos * pos_stride]; }
    __device__ __forceinline__ void put(int pos, uint8_t v) const { base[(size_t)pos * pos_stride] = v; }
};
// Superframes inside the MSC output of one protection class: byte k of the superframe that starts at logical
// frame r0 of a pair lives in frame r0 + k / frame_bytes at offset k % frame_bytes.
struct RsMscIo {
    uint8_t* frames; size_t frame_stride; int frame_bytes, s, i;
    __device__ __forceinline__ uint8_t* at(int pos) const { const int k = pos * s + i; return frames + (size_t)(k / frame_bytes) * frame_stride + (k % frame_bytes); }
    __device__ __forceinline__ uint8_t get(int pos) const { return *at(pos); }
    __device__ __forceinline__ void put(int pos, uint8_t v) const { *at(pos) = v; }
};

// The syndromes S_i = c(alpha^i), i = 0 .. 9 (FCR = 0, PRIM = 1), of a received word c(x) are those of its remainder r(x) = c(x) mod g(x),
// g(x) = prod (x - alpha^i): g(alpha^i) = 0.  A clean word -- almost every word of a receiver in lock -- has r = 0 and needs nothing else.
// r_k = coefficient of x^k: w0 = r_0 .. r_3 (r_0 in the low byte), w1 = r_4 .. r_7, w2 = r_8 r_9
struct RsRem {
    uint32_t w0, w1, w2;
    __device__ __forceinline__ bool zero() const { return (w0 | w1 | w2) == 0; }
};
// The division as a shift register, byte 0 (the coefficient of x^119) first: r <- r x + d - f g(x), f = r_9 the coefficient that the shift
// moves to x^10 (g is monic).  gtab[f] = the ten products f g_k in the register's layout: one 16-byte look-up, an 80-bit shift and three
// XORs per byte, where Horner's rule at ten roots takes twenty look-ups.
template <typename IO>
__device__ __forceinline__ RsRem rs_remainder120(const IO& io, const uint4* __restrict__ gtab)
{
    RsRem r{0, 0, 0};
#pragma unroll 4
    for (int j = 0; j < RS_LEN; j++) {
        const uint4 g = gtab[r.w2 >> 8];
        const uint32_t d = io.get(j);
        r.w2 = (((r.w2 << 8) | (r.w1 >> 24)) & 0xFFFFu) ^ g.z;
        r.w1 = ((r.w1 << 8) | (r.w0 >> 24)) ^ g.y;
        r.w0 = ((r.w0 << 8) | d) ^ g.x;
    }
    return r;
}
// One term of the syndromes: the value v at x^k adds v alpha^(i k) to S_i, i = 0 .. 9 (k in 0 .. 254).  `syn` is only ever indexed by
// unrolled constants (the array the Berlekamp-Massey iteration indexes dynamically is a copy made in rs_correct120 -- sharing one array
// sent it through scratch memory)
__device__ __forceinline__ void rs_syndrome_term(uint32_t (&syn)[RS_NROOTS], uint32_t v, uint32_t k, const uint8_t* __restrict__ alpha_to, const uint8_t* __restrict__ index_of)
{
    uint32_t ex = index_of[v];                                           // 255 for v = 0: the terms are masked below
    syn[0] ^= v;
#pragma unroll
    for (int i = 1; i < RS_NROOTS; i++) {
        ex += k; ex = ex >= RS_NN ? ex - RS_NN : ex;
        const uint32_t av = alpha_to[ex >= RS_NN ? ex - RS_NN : ex];
        syn[i] ^= v ? av : 0u;
    }
}
// S_i = r(alpha^i) = XOR_k r_k alpha^(i k): ten terms per root, added to syn (the caller's zeros).  Only for r != 0.
__device__ __forceinline__ void rs_syndromes_from_remainder(const RsRem& r, uint32_t (&syn)[RS_NROOTS], const uint8_t* __restrict__ alpha_to, const uint8_t* __restrict__ index_of)
{
#pragma unroll
    for (int k = 0; k < RS_NROOTS; k++)
        rs_syndrome_term(syn, ((k < 4 ? r.w0 : k < 8 ? r.w1 : r.w2) >> (8 * (k & 3))) & 255u, (uint32_t)k, alpha_to, index_of);
}

// Errors from the ten syndromes on.  The polynomials are field VALUES (not logarithms) in a small per-thread LDS workspace -- the
// path is rare and serial, what matters is that it costs the callers' hot loops neither registers nor scratch memory (a fully
// unrolled register-resident version spilled the superframe filter's syndrome loop; the first version indexed per-thread arrays in
// scratch) -- and every data-dependent choice is a select.
// What has to equal the reference (decode_rs.h:117-298, no erasures) is the mathematics, including what it does beyond the
// correction capacity -- a decoder that "detects" more or fewer uncorrectable words, or applies different wrong corrections,
// would not give the reference's bytes:
//   * Massey's iteration in the form that multiplies the auxiliary polynomial by x every round: the locator after ten rounds
//     is the same whatever representation is used;
//   * the word is given up (-1) exactly when the locator's degree differs from the number of its roots among alpha^1 .. alpha^255;
//   * roots at positions inside the 135 bytes of padding are counted but not applied; a zero evaluator value is not applied;
//   * a zero derivative is NOT treated as a failure (the reference checks that only in DEBUG builds): its logarithm reads 255
//     from the table and the division degenerates into a multiplication by one.
constexpr int RS_WS_BYTES = 64;                      // per-thread workspace
struct RsWs {                                        // ... as rs_correct120 sees it: lam[11] aux[11] term[11] omega[10] root[10] syn[10]
    uint8_t *lam, *aux, *term, *omega, *root, *syn;  // (syn: a dynamically indexed copy, the register array is only indexed by unrolled constants)
    __device__ __forceinline__ explicit RsWs(uint8_t* ws) : lam(ws), aux(lam + RS_NROOTS + 1), term(aux + RS_NROOTS + 1), omega(term + RS_NROOTS + 1), root(omega + RS_NROOTS), syn(root + RS_NROOTS) {}
};
static_assert(3 * (RS_NROOTS + 1) + 3 * RS_NROOTS <= RS_WS_BYTES, "the workspace view fits what the kernels reserve per thread");
__device__ __forceinline__ uint32_t gf_mul(uint32_t a, uint32_t b, const uint8_t* __restrict__ alpha_to, const uint8_t* __restrict__ index_of)
{
    uint32_t e = (uint32_t)index_of[a] + index_of[b];            // <= 254 + 254 when both are non-zero
    e = e >= RS_NN ? e - RS_NN : e;
    const uint32_t v = alpha_to[e >= RS_NN ? e - RS_NN : e];      // (index_of[0] = 255 can push e to 510: folded twice, result discarded)
    return (a != 0 && b != 0) ? v : 0u;
}
// a * alpha^k, k in 0 .. 254
__device__ __forceinline__ uint32_t gf_scale(uint32_t a, uint32_t k, const uint8_t* __restrict__ alpha_to, const uint8_t* __restrict__ index_of)
{
    uint32_t e = (uint32_t)index_of[a] + k;
    e = e >= RS_NN ? e - RS_NN : e;
    return a != 0 ? (uint32_t)alpha_to[e >= RS_NN ? e - RS_NN : e] : 0u;
}

// ---- locator polynomial: Massey's iteration, aux <- x aux every round.  Returns the locator's degree.
__device__ __forceinline__ int rs_locator(const RsWs& w, const uint8_t* alpha_to, const uint8_t* index_of)
{
    for (int i = 0; i <= RS_NROOTS; i++) { w.lam[i] = i == 0; w.aux[i] = i == 0; }
    int L = 0;
#pragma unroll 1
    for (int r = 0; r < RS_NROOTS; r++) {
        uint32_t d = 0;                              // discrepancy: sum lam[i] S[r - i]
        for (int i = 0; i <= r; i++) d ^= gf_mul(w.lam[i], w.syn[r - i], alpha_to, index_of);
        for (int i = RS_NROOTS; i > 0; i--) w.aux[i] = w.aux[i - 1];
        w.aux[0] = 0;
        if (d != 0) {
            const bool grow = 2 * L <= r;
            const uint32_t ld = index_of[d];
            const uint32_t dinv = alpha_to[ld == 0 ? 0 : RS_NN - ld];            // 1 / d
            for (int i = 0; i <= RS_NROOTS; i++) {
                const uint32_t li = w.lam[i];
                const uint32_t next = li ^ gf_mul(d, w.aux[i], alpha_to, index_of);
                if (grow) w.aux[i] = (uint8_t)gf_mul(li, dinv, alpha_to, index_of);
                w.lam[i] = (uint8_t)next;
            }
            if (grow) L = r + 1 - L;
        }
    }
    int deg = 0;
    for (int i = 1; i <= RS_NROOTS; i++) if (w.lam[i] != 0) deg = i;
    return deg;
}
// ---- roots: Lambda(alpha^i) for i = 1 .. 255, terms advanced by alpha^j per step; position of a root: i - 1 (of the padded word).
// Returns how many there are (the search ends with the deg-th).
__device__ __forceinline__ int rs_roots(const RsWs& w, int deg, const uint8_t* alpha_to, const uint8_t* index_of)
{
    for (int j = 1; j <= RS_NROOTS; j++) w.term[j] = w.lam[j];
    int count = 0;
#pragma unroll 1
    for (int i = 1; i <= RS_NN && count < deg; i++) {
        uint32_t q = 1;
        for (int j = 1; j <= deg; j++) { const uint32_t t = gf_scale(w.term[j], (uint32_t)j, alpha_to, index_of); w.term[j] = (uint8_t)t; q ^= t; }
        if (q == 0) w.root[count++] = (uint8_t)i;
    }
    return count;
}
// ---- evaluator: omega = S Lambda mod x^deg
__device__ __forceinline__ void rs_evaluator(const RsWs& w, int deg, const uint8_t* alpha_to, const uint8_t* index_of)
{
    for (int k = 0; k < deg; k++) {
        uint32_t v = 0;
        for (int j = 0; j <= k; j++) v ^= gf_mul(w.syn[k - j], w.lam[j], alpha_to, index_of);
        w.omega[k] = (uint8_t)v;
    }
}
// ---- values: omega(alpha^i) alpha^(-i) / Lambda'(alpha^i), applied where the position lies in the 120 transmitted bytes
template <typename IO>
__device__ __forceinline__ void rs_apply_values(const IO& io, const RsWs& w, int deg, int count, const uint8_t* alpha_to, const uint8_t* index_of)
{
#pragma unroll 1
    for (int n = 0; n < count; n++) {
        const uint32_t i = w.root[n];
        uint32_t num = 0, den = 0, p = 0;            // p = (k i) mod 255
        for (int k = 0; k < RS_NROOTS; k++) {
            if (k < deg) num ^= gf_scale(w.omega[k], p, alpha_to, index_of);
            if ((k & 1) == 0) den ^= gf_scale(w.lam[k + 1], p, alpha_to, index_of);  // formal derivative: the odd coefficients
            p += i; p = p >= RS_NN ? p - RS_NN : p;
        }
        const int pos = (int)i - 1 - RS_PAD;
        if (num != 0 && pos >= 0) {
            const uint32_t xinv = i == RS_NN ? 0u : RS_NN - i;                       // log of alpha^(-i)
            const uint32_t lden = index_of[den];                                      // 255 for den = 0 (see above)
            uint32_t e = (uint32_t)index_of[num] + xinv + RS_NN - lden;               // <= 254 + 254 + 255
            e = e >= 2 * RS_NN ? e - 2 * RS_NN : e; e = e >= RS_NN ? e - RS_NN : e;
            io.put(pos, (uint8_t)(io.get(pos) ^ alpha_to[e]));
        }
    }
}
// returns the number of corrected symbols, -1 when uncorrectable (decode_rs.h:71-298, no_eras = 0)
template <typename IO>
__device__ __forceinline__ int rs_correct120(const IO& io, const uint32_t (&syn)[RS_NROOTS], const uint8_t* __restrict__ alpha_to, const uint8_t* __restrict__ index_of, uint8_t* ws /* RS_WS_BYTES of LDS owned by this thread */)
{
    uint32_t any = 0;
#pragma unroll
    for (int i = 0; i < RS_NROOTS; i++) any |= syn[i];
    if (!any) return 0;
    const RsWs w(ws);
#pragma unroll
    for (int i = 0; i < RS_NROOTS; i++) w.syn[i] = (uint8_t)syn[i];
    const int deg = rs_locator(w, alpha_to, index_of);
    const int count = rs_roots(w, deg, alpha_to, index_of);
    if (count != deg) return -1;
    rs_evaluator(w, deg, alpha_to, index_of);
    rs_apply_values(io, w, deg, count, alpha_to, index_of);
    return count;
}

template <typename IO>
__device__ __forceinline__ int rs_decode120(const IO& io, const uint8_t* __restrict__ alpha_to, const uint8_t* __restrict__ index_of, const uint4* __restrict__ gtab, uint8_t* ws)
{
    const RsRem r = rs_remainder120(io, gtab);
    if (r.zero()) return 0;
    uint32_t syn[RS_NROOTS] = {};
    rs_syndromes_from_remainder(r, syn, alpha_to, index_of);
    return rs_correct120(io, syn, alpha_to, index_of, ws);
}

// The code's tables from the copy the host uploaded (RS_GF_BYTES + RS_GTAB_BYTES at gf) into LDS; gtab = nullptr: the GF tables only.
// The callers' barrier follows.
// (NT threads, NT >= 64 dividing 256.  Every load is issued before the first store: a loop of load-then-store waits out one round trip
// to memory per turn, which is what a work-group of one wave spends its time on)
template <int NT>
__device__ __forceinline__ void rs_tables(const uint8_t* __restrict__ gf, uint8_t* alpha_to, uint8_t* index_of, uint4* gtab, int t)
{
    constexpr int PER = RS_GTAB_BYTES / 16 / NT;                            // 4 or 1 (named registers: an array of them went through scratch memory)
    static_assert(PER == 1 || PER == 4, "64 or 256 threads");
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(gf + RS_GF_BYTES) + t;
    uint32_t a = 0, b = 0;
    uint4 g0{}, g1{}, g2{}, g3{};
    if (t < 64) { a = reinterpret_cast<const uint32_t*>(gf)[t]; b = reinterpret_cast<const uint32_t*>(gf + 256)[t]; }
    if (gtab) { g0 = src[0]; if (PER == 4) { g1 = src[NT]; g2 = src[2 * NT]; g3 = src[3 * NT]; } }
    if (t < 64) { reinterpret_cast<uint32_t*>(alpha_to)[t] = a; reinterpret_cast<uint32_t*>(index_of)[t] = b; }
    if (gtab) { gtab[t] = g0; if (PER == 4) { gtab[NT + t] = g1; gtab[2 * NT + t] = g2; gtab[3 * NT + t] = g3; } }
}

} // namespace dabphy
