// welle.io_amd/csrc/k_rs.hip -- DAB+ Reed-Solomon RS(120,110) over GF(2^8), one thread per codeword.
//
// Replaces (reference file:line):
//   RSDecoder::DecodeSuperframe          src/backend/dabplus_decoder.cpp:326-359
//   decode_rs_char / decode_rs.h         src/libs/fec/decode_rs.h:71-298  (KA9Q libfec, no erasures)
//   init_rs_char(8, 0x11D, 0, 1, 10, 135)  src/libs/fec/init_rs.h:6-103   (log/antilog tables)
//
// A superframe of a sub-channel with s = bitrate/8 holds s column-interleaved codewords: codeword i consists of
// bytes sf[pos*s + i], pos = 0..119.  Consecutive threads take consecutive i, so every syndrome step reads s
// consecutive bytes.  Syndromes -> locator (Massey) -> roots -> values, register-resident (rs_correct120); corrected
// bytes, the corrected-symbol count and the "uncorrectable" verdict equal the reference's also for words beyond the
// correction capacity (miscorrections included).  What pins it, each against the oracle, which is pinned to decode_rs_char itself
// (tests/test_oracle_vs_ref.py): tests/golden rs vectors; random error patterns of weight 0 .. 12 at 1 .. 48 code words per superframe
// (check_rs_random); words built for the corner paths -- roots in the padding, miscorrections written in full, errors at the edges of
// the shortened code, zero data, S0 = 0 (check_rs_directed, tests/sf_cases.py); k_rs_msc by value on the class outputs of a stream
// (check_rs_decode_msc); the filter over the four access-unit layouts, every rejection rule and 8 .. 384 kbit/s
// (check_superframe_layouts); the syndromes as they are taken now -- from the word's remainder modulo the generator polynomial
// (rs_remainder120, rs_syndromes_from_remainder) -- by an error at every position, five and six errors through the same places and the
// corner words at 1, 8, 9 and 48 code words per superframe (tests/rs_remainder_cases.py).  The tables live in LDS.
//
// Second half of the file: the DAB+ superframe filter (SuperframeFilter::Feed / CheckSync, dabplus_decoder.cpp:50-213) on the
// class output of a batch -- k_superframe_wide + k_superframe_settle (every attempt a receiver in lock makes in the batch at once,
// accepted per sub-channel iff all of them synchronise) and k_superframe (the reference's walk frame by frame, for what is left).
#include "dabphy_kernels.h"
#include <dabphy_wave_ops.h>

namespace dabphy {

constexpr int RS_NN = 255, RS_NROOTS = 10, RS_PAD = 135, RS_LEN = 120;

__device__ __forceinline__ int rs_modnn(int x)
{
    while (x >= RS_NN) { x -= RS_NN; x = (x >> 8) + (x & RS_NN); }
    return x;
}

struct RsIo {                         // byte `pos` of codeword i
    uint8_t* base; size_t pos_stride;
    __device__ __forceinline__ uint8_t get(int pos) const { return base[(size_t)pos * pos_stride]; }
    __device__ __forceinline__ void put(int pos, uint8_t v) const { base[(size_t)pos * pos_stride] = v; }
};

// returns the number of corrected symbols, -1 when uncorrectable (decode_rs.h:71-298, no_eras = 0)
template <typename IO>
__device__ __forceinline__ int rs_correct120(const IO& io, const uint32_t (&syn)[RS_NROOTS], const uint8_t* __restrict__ alpha_to, const uint8_t* __restrict__ index_of, uint8_t* ws);

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
// S_i = r(alpha^i) = XOR_k r_k alpha^(i k): ten terms per root.  Only for r != 0; `syn` is only ever indexed by unrolled constants (the
// array the Berlekamp-Massey iteration indexes dynamically is a copy made in rs_correct120 -- sharing one array sent it through scratch memory)
__device__ __forceinline__ void rs_syndromes_from_remainder(const RsRem& r, uint32_t (&syn)[RS_NROOTS], const uint8_t* __restrict__ alpha_to, const uint8_t* __restrict__ index_of)
{
#pragma unroll
    for (int i = 0; i < RS_NROOTS; i++) syn[i] = 0;
#pragma unroll
    for (int k = 0; k < RS_NROOTS; k++) {
        const uint32_t rk = ((k < 4 ? r.w0 : k < 8 ? r.w1 : r.w2) >> (8 * (k & 3))) & 255u;
        uint32_t ex = index_of[rk];                                      // 255 for r_k = 0: the terms are masked below
        syn[0] ^= rk;
#pragma unroll
        for (int i = 1; i < RS_NROOTS; i++) {
            ex += (uint32_t)k; ex = ex >= RS_NN ? ex - RS_NN : ex;
            const uint32_t av = alpha_to[ex >= RS_NN ? ex - RS_NN : ex];
            syn[i] ^= rk ? av : 0u;
        }
    }
}

template <typename IO>
__device__ __forceinline__ int rs_decode120(const IO& io, const uint8_t* __restrict__ alpha_to, const uint8_t* __restrict__ index_of, const uint4* __restrict__ gtab, uint8_t* ws)
{
    const RsRem r = rs_remainder120(io, gtab);
    if (r.zero()) return 0;
    uint32_t syn[RS_NROOTS];
    rs_syndromes_from_remainder(r, syn, alpha_to, index_of);
    return rs_correct120(io, syn, alpha_to, index_of, ws);
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
constexpr int RS_WS_BYTES = 64;                      // per-thread workspace: lam[11] aux[11] term[11] omega[10] root[10]
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

template <typename IO>
__device__ __forceinline__ int rs_correct120(const IO& io, const uint32_t (&syn_regs)[RS_NROOTS], const uint8_t* __restrict__ alpha_to, const uint8_t* __restrict__ index_of,
                                             uint8_t* ws /* RS_WS_BYTES of LDS owned by this thread */)
{
    uint32_t any = 0;
#pragma unroll
    for (int i = 0; i < RS_NROOTS; i++) any |= syn_regs[i];
    if (!any) return 0;
    constexpr int T2 = RS_NROOTS;                    // 2t = 10 syndromes, locator degree <= 10
    uint8_t* const lam = ws; uint8_t* const aux = ws + 11; uint8_t* const term = ws + 22; uint8_t* const omega = ws + 33; uint8_t* const root = ws + 43;
    uint8_t* const syn = ws + 53;                    // (a dynamically indexed copy: the register array is only indexed by unrolled constants)
#pragma unroll
    for (int i = 0; i < T2; i++) syn[i] = (uint8_t)syn_regs[i];
    // ---- locator polynomial: Massey's iteration, aux <- x aux every round
    for (int i = 0; i <= T2; i++) { lam[i] = i == 0; aux[i] = i == 0; }
    int L = 0;
#pragma unroll 1
    for (int r = 0; r < T2; r++) {
        uint32_t d = 0;                              // discrepancy: sum lam[i] S[r - i]
        for (int i = 0; i <= r; i++) d ^= gf_mul(lam[i], syn[r - i], alpha_to, index_of);
        for (int i = T2; i > 0; i--) aux[i] = aux[i - 1];
        aux[0] = 0;
        if (d != 0) {
            const bool grow = 2 * L <= r;
            const uint32_t ld = index_of[d];
            const uint32_t dinv = alpha_to[ld == 0 ? 0 : RS_NN - ld];            // 1 / d
            for (int i = 0; i <= T2; i++) {
                const uint32_t li = lam[i];
                const uint32_t next = li ^ gf_mul(d, aux[i], alpha_to, index_of);
                if (grow) aux[i] = (uint8_t)gf_mul(li, dinv, alpha_to, index_of);
                lam[i] = (uint8_t)next;
            }
            if (grow) L = r + 1 - L;
        }
    }
    int deg = 0;
    for (int i = 1; i <= T2; i++) if (lam[i] != 0) deg = i;
    // ---- roots: Lambda(alpha^i) for i = 1 .. 255, terms advanced by alpha^j per step; position of a root: i - 1 (of the padded word)
    for (int j = 1; j <= T2; j++) term[j] = lam[j];
    int count = 0;
#pragma unroll 1
    for (int i = 1; i <= RS_NN && count < deg; i++) {
        uint32_t q = 1;
        for (int j = 1; j <= deg; j++) { const uint32_t t = gf_scale(term[j], (uint32_t)j, alpha_to, index_of); term[j] = (uint8_t)t; q ^= t; }
        if (q == 0) root[count++] = (uint8_t)i;
    }
    if (count != deg) return -1;
    // ---- evaluator: omega = S Lambda mod x^deg
    for (int k = 0; k < deg; k++) {
        uint32_t v = 0;
        for (int j = 0; j <= k; j++) v ^= gf_mul(syn[k - j], lam[j], alpha_to, index_of);
        omega[k] = (uint8_t)v;
    }
    // ---- values: omega(alpha^i) alpha^(-i) / Lambda'(alpha^i), applied where the position lies in the 120 transmitted bytes
#pragma unroll 1
    for (int n = 0; n < count; n++) {
        const uint32_t i = root[n];
        uint32_t num = 0, den = 0, p = 0;            // p = (k i) mod 255
        for (int k = 0; k < T2; k++) {
            if (k < deg) num ^= gf_scale(omega[k], p, alpha_to, index_of);
            if ((k & 1) == 0) den ^= gf_scale(lam[k + 1], p, alpha_to, index_of);    // formal derivative: the odd coefficients
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
    return count;
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

// Contiguous superframes: sf[n_sf][120*s]; result per superframe: corrected-symbol total and uncorrectable flag.
__global__ void __launch_bounds__(256) k_rs_superframes(RsArgs A)
{
    __shared__ __attribute__((aligned(16))) uint8_t alpha_to[256], index_of[256];
    __shared__ uint4 gtab[RS_GTAB_BYTES / 16];
    __shared__ uint8_t ws[256 * RS_WS_BYTES];
    rs_tables<256>(A.gf, alpha_to, index_of, gtab, threadIdx.x);
    __syncthreads();
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int total = A.n_sf * A.s;
    if (idx >= total) return;
    const int sf = idx / A.s, i = idx % A.s;
    RsIo io; io.base = A.data + (size_t)sf * A.sf_stride + i; io.pos_stride = (size_t)A.s;
    const int c = rs_decode120(io, alpha_to, index_of, gtab, ws + threadIdx.x * RS_WS_BYTES);
    if (c < 0) atomicOr(A.uncorr + sf, 1);
    else if (c > 0) atomicAdd(A.corr + sf, c);
}

// Superframes inside the MSC output of one protection class: byte k of the superframe that starts at logical
// frame r0 of a pair lives in frame r0 + k / frame_bytes at offset k % frame_bytes.
struct RsMscIo {
    uint8_t* frames; size_t frame_stride; int frame_bytes, s, i;
    __device__ __forceinline__ uint8_t* at(int pos) const { const int k = pos * s + i; return frames + (size_t)(k / frame_bytes) * frame_stride + (k % frame_bytes); }
    __device__ __forceinline__ uint8_t get(int pos) const { return *at(pos); }
    __device__ __forceinline__ void put(int pos, uint8_t v) const { *at(pos) = v; }
};

__global__ void __launch_bounds__(256) k_rs_msc(RsMscArgs A)
{
    __shared__ __attribute__((aligned(16))) uint8_t alpha_to[256], index_of[256];
    __shared__ uint4 gtab[RS_GTAB_BYTES / 16];
    __shared__ uint8_t ws[256 * RS_WS_BYTES];
    rs_tables<256>(A.gf, alpha_to, index_of, gtab, threadIdx.x);
    __syncthreads();
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int per_pair = A.n_sf_per_pair * A.s;
    if (idx >= A.n_pairs * per_pair) return;
    const int pair = idx / per_pair; const int rem = idx % per_pair;
    const int q = rem / A.s, i = rem % A.s;
    const MscPair pp = A.pairs[pair];
    const int2 rows = A.rows[pair];
    const int fc = A.first_cif[pp.ens];
    const int r0 = fc + 5 * (q + (fc < 0 ? -fc / 5 : 0));        // first logical frame of superframe q (of those that do not end in front of row 0, however far back the alignment was given)
    if (r0 < rows.x || r0 + 5 > rows.y) return;                  // a superframe that touches a row outside the batch's frames is neither decoded nor counted
    RsMscIo io;
    io.frame_bytes = A.frame_bytes; io.s = A.s; io.i = i; io.frame_stride = (size_t)A.frame_bytes;
    io.frames = A.out + ((size_t)pair * A.n_cif + r0) * A.frame_bytes;
    const int c = rs_decode120(io, alpha_to, index_of, gtab, ws + threadIdx.x * RS_WS_BYTES);
    int* cnt =A.result + 2 * ((size_t)pair * A.n_sf_per_pair + q);
    if (c < 0) atomicOr(cnt + 1, 1);
    else if (c > 0) atomicAdd(cnt, c);
}

// ------------------------------------------------------------------------------------------ DAB+ superframe filter
// SuperframeFilter::Feed / CheckSync (dabplus_decoder.cpp:50-213) for one sub-channel of every ensemble: one 64-thread
// work-group per ensemble walks the logical frames of the batch in order with the reference's state machine -- 5-frame
// sliding window, Reed-Solomon on a copy (thread i = codeword i), Fire-code / AU-table check, AU CRCs (thread i = access
// unit i), and after a hit a fresh window -- and carries frame_count + the raw window to the next batch.  Only events and
// corrected, synchronised superframes leave the device.
__device__ __forceinline__ uint16_t crc16_msb(const uint8_t* data, int len, bool initial_invert, bool final_invert, uint16_t poly)
{
    uint16_t crc = initial_invert ? 0xFFFF : 0x0000;                           // CalcCRC, tools.cpp:41-72
    for (int o = 0; o < len; o++) {
        crc ^= (uint16_t)(data[o] << 8);
        for (int i = 0; i < 8; i++) crc = (crc & 0x8000) ? (uint16_t)((crc << 1) ^ poly) : (uint16_t)(crc << 1);
    }
    return final_invert ? (uint16_t)~crc : crc;
}

// the same CRC a byte at a time through a 256-entry table of the polynomial (LDS): crc' = (crc << 8) ^ tab[(crc >> 8) ^ byte]
__device__ __forceinline__ uint16_t crc16_msb_tab(const uint8_t* data, int len, bool initial_invert, bool final_invert, const uint16_t* tab)
{
    uint32_t crc = initial_invert ? 0xFFFFu : 0x0000u;
    for (int o = 0; o < len; o++) crc = ((crc << 8) & 0xFFFFu) ^ tab[(crc >> 8) ^ data[o]];
    return (uint16_t)(final_invert ? ~crc : crc);
}

constexpr int SF_PREFETCH = 6;      // rows of the class output in flight per work-group (serial walk)

// GF(256) tables of the code (init_rs.h:48-60) from the copy the host uploaded, and the byte-wise table of CRC-16-CCITT (0x1021)
__device__ __forceinline__ void sf_tables(const SfArgs& A, uint8_t* alpha_to, uint8_t* index_of, uint4* gtab, uint16_t* crctab, int t)
{
    rs_tables<64>(A.gf, alpha_to, index_of, gtab, t);
    if (crctab)
        for (int v = t; v < 256; v += 64) {
            uint16_t c = (uint16_t)(v << 8);
            for (int i = 0; i < 8; i++) c = (c & 0x8000) ? (uint16_t)((c << 1) ^ 0x1021) : (uint16_t)(c << 1);
            crctab[v] = c;
        }
}

// What the batch holds for one (ensemble, sub-channel) pair: fc frames carried in, of which the window machine still uses the last cu (a full
// window that failed drops its oldest frame with the next one, dabplus_decoder.cpp:78-81); rows [r_first, n_rows) of the class output
// are the frames it will be fed (rows are packed: k_msc_gather lays the logical frames of an ensemble out in CIF order from the first
// frame number of the batch, whatever slots the demodulated frames occupied; frames before the 16-CIF fill of the time de-interleaver,
// dab-audio.cpp:146-149, counted from the CIF at which the pair was selected (MscPair::cif0), are never emitted).  If every attempt synchronises, attempts happen at frames 5q + 4 of that sequence: nq of them.
struct SfPlan { int fc, cu, n_rows, r_first, avail, nq; };
// (called by all 64 lanes of the work-group's wave together: lane t looks at frame t, t + 64, ... -- one round trip to memory for the batch's
// descriptors where a loop over the frames makes one per frame)
__device__ __forceinline__ SfPlan sf_plan(const SfArgs& A, const MscPair& pp, const uint8_t* st, int t)
{
    const int b = pp.ens;
    SfPlan p;
    p.fc = *reinterpret_cast<const int32_t*>(st);
    p.cu = p.fc == 5 ? 4 : p.fc;
    int nv = 0;
    for (int f0 = 0; f0 < A.n_frames; f0 += 64) {
        const int f = f0 + t;
        nv += __popcll(__ballot(f < A.n_frames && A.desc[(size_t)b * A.n_frames + (f < A.n_frames ? f : 0)].valid == 1));
    }
    const long long c0 = 4 * A.desc[(size_t)b * A.n_frames].frame_no;
    p.n_rows = 4 * nv;
    p.r_first = 0;
    while (p.r_first < p.n_rows && c0 + p.r_first - pp.cif0 < 16) p.r_first++;
    p.avail = p.n_rows - p.r_first;
    p.nq = p.avail > 0 ? (p.cu + p.avail) / 5 : 0;
    return p;
}

// Reed-Solomon over the s code words of each of the attempts a_first .. n_att - 1, 5-frame copies sf_len bytes apart in s_sf (dabplus_decoder.cpp:97), by the 64
// lanes of one wave; corr[a] / unc[a] (LDS, zeroed here) = the attempt's corrected symbols / whether a word was given up, valid for all
// threads on return.  Two forms, the caller's choice:
//   SPLIT = false  every lane owns a code word (attempt t / s, word t % s; n_att s <= 64) and divides it by the generator polynomial:
//                  120 dependent steps of one look-up each, and nothing more for a clean word.  64 code words per wave: the wide pass.
//                  gtab = the remainder table in LDS, s_ws = 64 workspaces.
//   SPLIT = true   a_first = 0, n_att = 1, eight code words at a time with the whole wave, each word's positions split over eight lanes: 15 independent
//                  steps per lane.  The serial walk makes one attempt at a time on one wave and at most 48 code words would leave its lanes
//                  idle through 120 dependent steps: it keeps this form.  gtab unused, s_ws = 8 workspaces.
// Both hand rs_correct120 the same syndromes.
template <bool SPLIT>
__device__ __forceinline__ void sf_rs_words(uint8_t* s_sf, int sf_len, int s, int a_first, int n_att, const uint8_t* alpha_to, const uint8_t* index_of, const uint4* gtab,
                                            uint8_t* s_ws, int* corr, int* unc, int t)
{
    if (t < n_att) { corr[t] = 0; unc[t] = 0; }
    __syncthreads();
    if (!SPLIT) {
        const int a = t / s, c = t - a * s;
        if (a >= a_first && a < n_att) {
            RsIo io; io.base = s_sf + a * sf_len + c; io.pos_stride = (size_t)s;
            const int n = rs_decode120(io, alpha_to, index_of, gtab, s_ws + t * RS_WS_BYTES);
            if (n < 0) atomicOr(&unc[a], 1); else if (n > 0) atomicAdd(&corr[a], n);
        }
        __syncthreads();
        return;
    }
    // Syndromes, eight codewords at a time with the whole wave: S_i = XOR_j d_j alpha^(i (119 - j)) is a sum, so lane
    // (codeword c = l & 7, byte group l >> 3 = 15 positions) adds its terms without any chain of dependent look-ups and
    // three butterfly exchanges fold the eight groups (Horner's 119 dependent steps were the whole cost of this kernel).
    for (int c0 = 0; c0 < s; c0 += 8) {
        const int c = c0 + (t & 7), jg = t >> 3;
        uint32_t syn[RS_NROOTS];
#pragma unroll
        for (int i = 0; i < RS_NROOTS; i++) syn[i] = 0;
        if (c < s) {
#pragma unroll 3
            for (int jj = 0; jj < 15; jj++) {
                const int j = jg * 15 + jj;
                const uint32_t dj = s_sf[j * s + c];
                const uint32_t k = (uint32_t)(RS_LEN - 1 - j);               // exponent step: x^(119 - j) at x = alpha^i
                uint32_t ex = index_of[dj];                                  // 255 for dj = 0: the terms are masked below
                syn[0] ^= dj;
#pragma unroll
                for (int i = 1; i < RS_NROOTS; i++) {
                    ex += k; ex = ex >= RS_NN ? ex - RS_NN : ex;
                    const uint32_t av = alpha_to[ex >= RS_NN ? ex - RS_NN : ex];
                    syn[i] ^= dj ? av : 0u;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < RS_NROOTS; i++) {
            syn[i] ^= __shfl_xor(syn[i], 8); syn[i] ^= __shfl_xor(syn[i], 16); syn[i] ^= __shfl_xor(syn[i], 32);
        }
        if (jg == 0 && c < s) {
            RsIo io; io.base = s_sf + c; io.pos_stride = (size_t)s;
            const int n = rs_correct120(io, syn, alpha_to, index_of, s_ws + (t & 7) * RS_WS_BYTES);
            if (n < 0) atomicOr(&unc[0], 1); else if (n > 0) atomicAdd(&corr[0], n);
        }
    }
    __syncthreads();
}

// CheckSync (dabplus_decoder.cpp:160-213) of one corrected superframe by ONE lane -> the attempt's event (cif and sf_slot are the caller's).
// Everything is indexed by unrolled constants: the lane keeps the start table in registers.
__device__ __forceinline__ int sf_check_sync(const uint8_t* sf, int sf_len, int corr, int unc, SfEvent& e)
{
    int sync = 0, num_aus = 0;
    int au[7] = {0, 0, 0, 0, 0, 0, 0};
    if (!(sf[3] == 0x00 && sf[4] == 0x00) && (uint16_t)(sf[0] << 8 | sf[1]) == crc16_msb(sf + 2, 9, false, false, 0x782F)) {
        const int dac_rate = sf[2] & 0x40, sbr_flag = sf[2] & 0x20;
        num_aus = dac_rate ? (sbr_flag ? 3 : 6) : (sbr_flag ? 2 : 4);
        au[0] = dac_rate ? (sbr_flag ? 6 : 11) : (sbr_flag ? 5 : 8);
        au[1] = sf[3] << 4 | sf[4] >> 4;
        au[2] = (sf[4] & 0x0F) << 8 | sf[5];
        au[3] = sf[6] << 4 | sf[7] >> 4;
        au[4] = (sf[7] & 0x0F) << 8 | sf[8];
        au[5] = sf[9] << 4 | sf[10] >> 4;
        sync = 1;
#pragma unroll
        for (int i = 1; i < 7; i++) au[i] = i < num_aus ? au[i] : i == num_aus ? sf_len / 120 * 110 : 0;
#pragma unroll
        for (int i = 0; i < 6; i++) if (i < num_aus && au[i] >= au[i + 1]) sync = 0;
    }
    e = SfEvent{};
    e.corrected = corr; e.uncorrectable = unc; e.sync = sync; e.sf_slot = -1;
    if (sync) {
        e.format = sf[2]; e.num_aus = num_aus;
#pragma unroll
        for (int i = 0; i < 7; i++) e.au_start[i] = au[i];
    }
    return sync;
}

// One attempt of the serial walk on the 5-frame copy in s_sf: Reed-Solomon over its s code words, then CheckSync.
// Thread 0 gets the attempt's event; sh.sync / corr / unc are valid for all threads on return.
struct SfShared { int corr, unc, sync; };
__device__ __forceinline__ void sf_attempt(uint8_t* s_sf, int fb, int s, const uint8_t* alpha_to, const uint8_t* index_of, uint8_t* s_ws,
                                           SfShared& sh, SfEvent& e, int t)
{
    sf_rs_words<true>(s_sf, 5 * fb, s, 0, 1, alpha_to, index_of, nullptr, s_ws, &sh.corr, &sh.unc, t);
    if (t == 0) sh.sync = sf_check_sync(s_sf, 5 * fb, sh.corr, sh.unc, e);
    __syncthreads();
}

// :122-131 AU CRC-16-CCITT of the first ne events of one (ensemble, sub-channel) pair, one lane per access unit.  The verdicts do not steer the
// state machine.  (Events and superframes were written by earlier kernels or, behind a barrier, by this work-group.)  Returns nothing:
// failures are counted into *aubad (LDS).
// (Round 5 tried bringing the superframes into LDS with coalesced loads first and walking LDS bytes: 0.45-0.60 ms for the verdict kernel
// against 0.40 ms as it is -- the staging's barriers and its 12-24 KB of LDS per work-group cost more occupancy than the byte-wise HBM
// reads cost latency; with ~16 work-groups per compute unit in flight those round trips overlap.  profiles/r05_summary.md.)
__device__ __forceinline__ void sf_au_crcs(const SfArgs& A, SfEvent* ev, size_t bm, int ne, int sf_len, const uint16_t* crctab, int* aubad, int t)
{
    for (int base = 0; base < ne * 6; base += 64) {
        const int k = base + t, e_i = k / 6, au_i = k % 6;
        if (e_i < ne && ev[e_i].sync && au_i < ev[e_i].num_aus) {
            const uint8_t* au = A.sf + (bm * A.n_slots + ev[e_i].sf_slot) * sf_len + ev[e_i].au_start[au_i];
            const int au_len = ev[e_i].au_start[au_i + 1] - ev[e_i].au_start[au_i];
            if (au_len >= 2 && (uint16_t)(au[au_len - 2] << 8 | au[au_len - 1]) == crc16_msb_tab(au, au_len - 2, true, true, crctab)) atomicOr(&ev[e_i].au_crc_ok, 1 << au_i);
            else atomicAdd(aubad, 1);
        }
    }
}

// n 8-byte words from memory into LDS by one wave, up to 16 loads of a lane in flight (see rs_tables)
__device__ __forceinline__ void sf_copy_in(uint2* dst, const uint2* __restrict__ src, int n, int t)
{
    for (int base = 0; base < n; base += 16 * 64) {
        uint2 v[16];
#pragma unroll
        for (int u = 0; u < 16; u++) { const int i = base + u * 64 + t; v[u] = i < n ? src[i] : uint2{0, 0}; }
#pragma unroll
        for (int u = 0; u < 16; u++) { const int i = base + u * 64 + t; if (i < n) dst[i] = v[u]; }
    }
}

// ---- The wide pass.  A receiver in lock finds a superframe every five frames: all attempts of the batch are made at once, one
// work-group per (pair, attempt q), each on the window the serial machine WOULD see if every earlier attempt of the batch
// synchronises (sf_plan).  k_superframe_settle then accepts an (ensemble, sub-channel) pair iff all its attempts did -- in that case the serial
// walk makes exactly these attempts on exactly these windows -- and does what the walk does at its end; every other (ensemble, sub-channel) pair
// is walked by k_superframe from the untouched state, as before.  The state machine's 26 dependent attempts per batch were this
// stage's whole time: 0.8 ms of a mostly idle device per step.
// Every class of a bucket (same LDS size) in ONE launch: block -> (class, its block) through the bucket's table of first blocks; the class's
// argument block comes from HBM.  A real multiplex has a handful of protection classes, a batch of independent ensembles a few dozen:
// one launch per class and kernel was 60 dependent launches of a few work-groups each at the end of every step.
__device__ __forceinline__ SfArgs sf_args_of(const SfBatch& Bt, uint32_t& bx)
{
    // (everything here is wave-uniform and read-only: through the constant address space these are scalar loads, the argument block
    // lives in scalar registers as a kernel argument would)
    const DABPHY_CONST_AS int32_t* first = as_constant(Bt.first);
    int c = 0;
    while (c + 1 < Bt.n_cls && bx >= (uint32_t)first[c + 1]) c++;
    bx -= (uint32_t)first[c];
    const DABPHY_CONST_AS SfArgs* cls = as_constant(Bt.cls);
    SfArgs a;
    __builtin_memcpy(&a, (const void DABPHY_CONST_AS*)&cls[c], sizeof a);
    return a;
}

// A work-group takes as many consecutive attempts of its pair as fill its 64 lanes with code words: 64 / s of them (eight at 64 kbit/s, one
// above 256 kbit/s; s <= 48), blockIdx.y = which ones.  Their windows are 64 / s * 120 s <= 7680 bytes of LDS whatever the bit rate; the
// buckets' instances differ in the attempts a work-group can hold (64 / 7 / 2: s >= 1 / 9 / 25).  The launch keeps its grid of one row per
// attempt of the batch -- the queue-order records (tests/queue_order) pin the launches of dabphy_process, grids included --; the rows behind
// the Bt.wide_rows that have work for the launch's largest s return before they touch memory (the heavy rows are dispatched first; measured:
// profiles/sf_wide_remainder.txt).  Once per work-group instead of once per attempt: the class's argument block, sf_plan (a descriptor per frame
// of the batch) and the tables.  Consecutive attempts read consecutive frames: one coalesced copy (two where attempt 0 starts in the carried
// frames of the state), and one copy out when all of them synchronise.
// Bt.replay (dabphy_time_superframe_wide): the launch repeats the pass of a batch that k_superframe_settle has settled since -- the state holds the
// frames carried OUT of the batch, no longer those carried in.  How many were carried in follows from the first event's row; the attempt
// that read them is left out (its event and superframe stay), every other attempt rewrites what it wrote.  Pairs that were walked are left out.
constexpr int SF_WIDE_LANES = 64, SF_WIDE_LDS = SF_WIDE_LANES * RS_LEN;
template <int SF_MAX>       // superframe bytes of the bucket (120 s)
__global__ void __launch_bounds__(64) k_superframe_wide(SfBatch Bt)
{
    if ((int)blockIdx.y >= Bt.wide_rows) return;
    constexpr int MAX_ATT = SF_MAX <= 960 ? SF_WIDE_LANES : SF_MAX <= 2880 ? SF_WIDE_LANES / 9 : SF_WIDE_LANES / 25;
    uint32_t bx = blockIdx.x;
    const SfArgs A = sf_args_of(Bt, bx);
    __shared__ __attribute__((aligned(16))) uint8_t s_sf[SF_WIDE_LDS];
    __shared__ __attribute__((aligned(16))) uint8_t alpha_to[256], index_of[256];
    __shared__ uint4 s_gtab[RS_GTAB_BYTES / 16];
    __shared__ int s_corr[MAX_ATT], s_unc[MAX_ATT], s_sync[MAX_ATT];
    __shared__ uint8_t s_ws[SF_WIDE_LANES * RS_WS_BYTES];       // error-path workspaces, one per code-word lane
    const int t = threadIdx.x, s = A.s;
    const int fb = A.frame_bytes, sf_len = 5 * fb, fw = fb >> 3;
    const int per_group = SF_WIDE_LANES / s < MAX_ATT ? SF_WIDE_LANES / s : MAX_ATT;
    const int q0 = (int)blockIdx.y * per_group;                   // the work-group's first attempt
    const size_t bm = A.run ? (size_t)A.run[bx] : (size_t)bx;      // the pair
    const uint8_t* st = A.state + bm * A.state_stride;
    SfPlan p = sf_plan(A, A.pairs[bm], st, t);
    int q_first = 0;
    if (Bt.replay) {
        if (!A.accepted[bm] || A.n_events[bm] < 1) return;
        const int cu = p.r_first + 4 - A.events[bm * A.n_cif].cif;
        if (cu < 0 || cu > 4) return;
        p.fc = p.cu = cu; p.nq = p.avail > 0 ? (cu + p.avail) / 5 : 0;
        q_first = cu > 0;
    }
    if (q0 >= p.nq) return;
    const int na = p.nq - q0 < per_group ? p.nq - q0 : per_group;
    sf_tables(A, alpha_to, index_of, s_gtab, nullptr, t);
    {
        // frames 5 q0 .. 5 (q0 + na) of (carried frames, then rows): the first n_st from the state, the rest consecutive rows of the class output
        const int g0 = 5 * q0, ng = 5 * na;
        const int n_st = p.cu - g0 <= 0 ? 0 : p.cu - g0 < ng ? p.cu - g0 : ng;
        if (n_st) sf_copy_in(reinterpret_cast<uint2*>(s_sf), reinterpret_cast<const uint2*>(st + 16 + (size_t)(p.fc - p.cu + g0) * fb), n_st * fw, t);
        sf_copy_in(reinterpret_cast<uint2*>(s_sf + n_st * fb), reinterpret_cast<const uint2*>(A.out + (bm * A.n_cif + (p.r_first + g0 + n_st - p.cu)) * fb), (ng - n_st) * fw, t);
    }
    sf_rs_words<false>(s_sf, sf_len, s, q0 < q_first, na, alpha_to, index_of, s_gtab, s_ws, s_corr, s_unc, t);
    if (t < na) {                                                              // one lane per attempt
        const int q = q0 + t;
        SfEvent e;
        const int sync = sf_check_sync(s_sf + t * sf_len, sf_len, s_corr[t], s_unc[t], e);
        e.cif = p.r_first + 5 * q + 4 - p.cu;                                  // the row whose arrival triggers the attempt
        if (sync) e.sf_slot = q;
        s_sync[t] = sync && q >= q_first;
        if (q >= q_first) A.events[bm * A.n_cif + q] = e;
    }
    __syncthreads();
    int n_sync = 0;
    for (int a = 0; a < na; a++) n_sync += s_sync[a];
    uint8_t* gsf = A.sf + (bm * A.n_slots + q0) * sf_len;                       // (slot = attempt: consecutive)
    if (n_sync == na)
        for (int i = t; i < na * 5 * fw; i += 64) reinterpret_cast<uint2*>(gsf)[i] = reinterpret_cast<const uint2*>(s_sf)[i];
    else
        for (int a = 0; a < na; a++)
            if (s_sync[a])
                for (int i = t; i < 5 * fw; i += 64) reinterpret_cast<uint2*>(gsf + (size_t)a * sf_len)[i] = reinterpret_cast<const uint2*>(s_sf + a * sf_len)[i];
}

__global__ void __launch_bounds__(64) k_superframe_settle(SfBatch Bt)
{
    uint32_t bx = blockIdx.x;
    const SfArgs A = sf_args_of(Bt, bx);
    __shared__ uint16_t s_crctab[256];
    __shared__ int s_ok, s_corr, s_unc, s_aubad;
    const int t = threadIdx.x;
    const int fb = A.frame_bytes, sf_len = 5 * fb, fw = fb >> 3;
    const size_t bm = A.run ? (size_t)A.run[bx] : (size_t)bx;      // the pair
    const int b = A.pairs[bm].ens;
    uint8_t* st = A.state + bm * A.state_stride;
    const SfPlan p = sf_plan(A, A.pairs[bm], st, t);
    SfEvent* ev = A.events + bm * A.n_cif;
    for (int v = t; v < 256; v += 64) {
        uint16_t c = (uint16_t)(v << 8);
        for (int i = 0; i < 8; i++) c = (c & 0x8000) ? (uint16_t)((c << 1) ^ 0x1021) : (uint16_t)(c << 1);
        s_crctab[v] = c;
    }
    if (t == 0) { s_ok = p.nq >= 1; s_corr = 0; s_unc = 0; s_aubad = 0; }
    __syncthreads();
    for (int q = t; q < p.nq; q += 64) {
        if (!ev[q].sync) s_ok = 0;                                  // (every writer stores the same value)
        else { if (ev[q].corrected) atomicAdd(&s_corr, ev[q].corrected); if (ev[q].uncorrectable) atomicAdd(&s_unc, ev[q].uncorrectable); }
    }
    __syncthreads();
    const int ok = s_ok;
    if (t == 0) { A.accepted[bm] = ok; if (A.wide_stats && p.nq >= 1) { atomicAdd(A.wide_stats + 1, 1ull); if (ok) atomicAdd(A.wide_stats, 1ull); } }   // (a batch without a full window has nothing the wide pass could settle: not counted as tried)
    if (!ok) return;
    sf_au_crcs(A, ev, bm, p.nq, sf_len, s_crctab, &s_aubad, t);
    // the frames behind the last attempt are the next batch's carried window (a hit empties it, dabplus_decoder.cpp:156)
    const int n_left = p.cu + p.avail - 5 * p.nq;
    for (int k = 0; k < n_left; k++) {
        const uint8_t* src = A.out + (bm * A.n_cif + (p.n_rows - n_left + k)) * fb;
        for (int i = t; i < fw; i += 64) reinterpret_cast<uint2*>(st + 16 + (size_t)k * fb)[i] = reinterpret_cast<const uint2*>(src)[i];
    }
    __syncthreads();
    if (t == 0) {
        *reinterpret_cast<int32_t*>(st) = n_left; A.n_events[bm] = p.nq;
        if (A.stats) { atomicAdd(A.stats + 4 * b, p.nq); atomicAdd(A.stats + 4 * b + 1, s_corr); atomicAdd(A.stats + 4 * b + 2, s_unc); atomicAdd(A.stats + 4 * b + 3, s_aubad); }
    }
}

// ---- The serial walk: SuperframeFilter::Feed / CheckSync (dabplus_decoder.cpp:50-213) for one sub-channel of one ensemble, frame by
// frame with the reference's state machine -- 5-frame sliding window, Reed-Solomon on a copy, Fire-code / AU-table check, AU CRCs, and
// after a hit a fresh window -- carrying frame_count + the raw window to the next batch.  Runs for what the wide pass did not settle.
template <int SF_MAX>       // superframe bytes the instance can hold (120 * bitrate / 8)
__global__ void __launch_bounds__(64, SF_MAX <= 2880 ? 4 : 2) k_superframe(SfBatch Bt)      // (four waves per SIMD: at five the 960-byte build spilled ten registers)
{
    uint32_t bx = blockIdx.x;
    const SfArgs A = sf_args_of(Bt, bx);
    // LDS: the raw 5-frame window (a ring: `head` = oldest frame, nothing is ever shifted) and the working copy
    __shared__ __attribute__((aligned(16))) uint8_t s_dyn[2 * SF_MAX];
    __shared__ __attribute__((aligned(16))) uint8_t alpha_to[256], index_of[256];
    __shared__ SfShared sh;
    __shared__ int s_aubad;
    __shared__ uint8_t s_ws[8 * RS_WS_BYTES];                   // error-path workspaces of the eight code words decoded at a time
    __shared__ uint16_t s_crctab[256];                          // CRC-16-CCITT (0x1021), one byte per step: the AU checks
    const int t = threadIdx.x;
    const size_t bm = A.run ? (size_t)A.run[bx] : (size_t)bx;      // the pair
    const int b = A.pairs[bm].ens;
    if (A.accepted && A.accepted[bm]) return;                  // settled by the wide pass
    sf_tables(A, alpha_to, index_of, nullptr, s_crctab, t);
    if (t == 0) s_aubad = 0;
    const int fb = A.frame_bytes, sf_len = 5 * fb;
    uint8_t* const s_raw = s_dyn;
    uint8_t* const s_sf = s_dyn + SF_MAX;
    uint8_t* st = A.state + bm * A.state_stride;
    const SfPlan p = sf_plan(A, A.pairs[bm], st, t);
    int frame_count = p.fc;
    __syncthreads();
    for (int i = t; i < frame_count * fb; i += 64) s_raw[i] = st[16 + i];     // carried frames, oldest first
    int head = 0;                                                              // ring slot of the oldest frame
    int ne = 0, slot = 0;
    SfEvent* ev = A.events + bm * A.n_cif;
    int tot_sync = 0, tot_corr = 0, tot_unc = 0;
    // A logical frame is fb = 24 * (bitrate / 8) bytes.  Rows travel HBM -> LDS by LDS-DMA, SF_PREFETCH rows ahead, into a ring of
    // their own (no registers, nothing waits until the row is needed).  Every row costs exactly ROW_DMA requests (lanes beyond the row
    // re-fetch its last dword into the slot's padding), so "row r has landed" is a constant vmcnt.
    constexpr int FB_MAX = SF_MAX / 5, ROW_DMA = (FB_MAX / 4 + 63) / 64, PRE_PITCH = ROW_DMA * 256;
    __shared__ __attribute__((aligned(16))) uint8_t s_pre[SF_PREFETCH * PRE_PITCH];
    const int fdw = fb >> 2;                                                   // dwords per row
    const int n_rows = p.n_rows, r_first = p.r_first;
    auto row_issue = [&](int r) {
        const uint8_t* src = A.out + (bm * A.n_cif + r) * fb;
        uint8_t* dst = s_pre + (r % SF_PREFETCH) * PRE_PITCH;
#pragma unroll
        for (int i = 0; i < ROW_DMA; i++) { int w = t + 64 * i; w = w < fdw ? w : fdw - 1; lds_dma4(src + 4 * w, dst + 256 * i); }
    };
    for (int i = 0; i < SF_PREFETCH; i++) if (r_first + i < n_rows) row_issue(r_first + i);
    for (int r = r_first; r < n_rows; r++) {
        if (r + SF_PREFETCH - 1 < n_rows) lds_dma_wait_but<(SF_PREFETCH - 1) * ROW_DMA>(); else lds_dma_wait();
        __syncthreads();
        int dst_slot;
        if (frame_count == 5) { dst_slot = head; head = head == 4 ? 0 : head + 1; }   // :78-81 "shift the previous frames": drop the oldest
        else { dst_slot = head + frame_count; if (dst_slot >= 5) dst_slot -= 5; frame_count++; }
        {
            const uint32_t* src = reinterpret_cast<const uint32_t*>(s_pre + (r % SF_PREFETCH) * PRE_PITCH);
            uint32_t* dst = reinterpret_cast<uint32_t*>(s_raw + dst_slot * fb);
#pragma unroll
            for (int i = 0; i < ROW_DMA; i++) if (t + 64 * i < fdw) dst[t + 64 * i] = src[t + 64 * i];
        }
        lds_reads_done();
        if (r + SF_PREFETCH < n_rows) row_issue(r + SF_PREFETCH);              // into the slot just emptied
        __syncthreads();
        if (frame_count < 5) continue;
        for (int k = 0; k < 5; k++) {                                          // :97 decode on a copy, frames in age order
            int sl = head + k; if (sl >= 5) sl -= 5;
            for (int i = t; i < fdw; i += 64) reinterpret_cast<uint32_t*>(s_sf + k * fb)[i] = reinterpret_cast<const uint32_t*>(s_raw + sl * fb)[i];
        }
        SfEvent e;
        sf_attempt(s_sf, fb, A.s, alpha_to, index_of, s_ws, sh, e, t);
        if (t == 0) {
            e.cif = r;
            if (sh.sync) e.sf_slot = slot;
            ev[ne] = e;
        }
        ne++;
        tot_corr += sh.corr; tot_unc += sh.unc;
        if (sh.sync) {
            uint8_t* gsf = A.sf + (bm * A.n_slots + slot) * sf_len;             // only synchronised superframes are kept
            for (int i = t; i < 5 * fdw; i += 64) reinterpret_cast<uint32_t*>(gsf)[i] = reinterpret_cast<const uint32_t*>(s_sf)[i];
            tot_sync++;
            frame_count = 0; head = 0; if (slot + 1 < A.n_slots) slot++;       // :156 wait for a complete new superframe
        }
    }
    __syncthreads();
    sf_au_crcs(A, ev, bm, ne, sf_len, s_crctab, &s_aubad, t);
    __syncthreads();
    for (int i = t; i < frame_count * fb; i += 64) {                           // carry the window, oldest frame first
        int sl = head + i / fb; if (sl >= 5) sl -= 5;
        st[16 + i] = s_raw[sl * fb + i % fb];
    }
    if (t == 0) {
        *reinterpret_cast<int32_t*>(st) = frame_count; A.n_events[bm] = ne;
        if (A.stats) { atomicAdd(A.stats + 4 * b, tot_sync); atomicAdd(A.stats + 4 * b + 1, tot_corr); atomicAdd(A.stats + 4 * b + 2, tot_unc); atomicAdd(A.stats + 4 * b + 3, s_aubad); }
    }
}

// bucket = index of the kernels' LDS size (superframes of <= 960 / <= 2880 / <= 5760 bytes: <= 64 / 192 / 384 kbit/s); Bt.cls are the
// classes of that bucket (DEVICE array), total_blocks = Bt.first[n_cls] (known to the host), n_cif = CIFs per batch, wide = run the wide pass
// the wide pass alone: a grid row per attempt of the batch, (n_cif + 4) / 5, of which the first wide_rows have work: 64 / s attempts per
// work-group, counted for the launch's largest s (the surplus work-groups of classes with a smaller one leave once they have their plan)
void launch_superframe_wide(SfBatch Bt, int bucket, int total_blocks, int n_cif, int max_s, hipStream_t s)
{
    if (total_blocks <= 0 || max_s < 1 || max_s > SF_WIDE_LANES) return;
    const int per_group = SF_WIDE_LANES / max_s, attempts = (n_cif + 4) / 5;
    Bt.wide_rows = (attempts + per_group - 1) / per_group;
    const dim3 wide(total_blocks, attempts);
    if (bucket == 0) hipLaunchKernelGGL(k_superframe_wide<960>, wide, dim3(64), 0, s, Bt);
    else if (bucket == 1) hipLaunchKernelGGL(k_superframe_wide<2880>, wide, dim3(64), 0, s, Bt);
    else hipLaunchKernelGGL(k_superframe_wide<5760>, wide, dim3(64), 0, s, Bt);
}

void launch_superframe_bucket(const SfBatch& Bt, int bucket, int total_blocks, int n_cif, int max_s, bool wide_pass, hipStream_t s)
{
    if (total_blocks <= 0) return;
    const dim3 grid(total_blocks);
    if (wide_pass) {
        // the wide pass: every attempt a locked receiver makes in this batch at once, then the verdict per (ensemble, sub-channel) pair
        launch_superframe_wide(Bt, bucket, total_blocks, n_cif, max_s, s);
        hipLaunchKernelGGL(k_superframe_settle, grid, dim3(64), 0, s, Bt);
    }
    if (bucket == 0) hipLaunchKernelGGL(k_superframe<960>, grid, dim3(64), 0, s, Bt);            // <= 64 kbit/s
    else if (bucket == 1) hipLaunchKernelGGL(k_superframe<2880>, grid, dim3(64), 0, s, Bt);     // <= 192 kbit/s
    else hipLaunchKernelGGL(k_superframe<5760>, grid, dim3(64), 0, s, Bt);                       // <= 384 kbit/s
}

void launch_rs_superframes(const RsArgs& a, hipStream_t s)
{
    const int total = a.n_sf * a.s;
    hipLaunchKernelGGL(k_rs_superframes, dim3((total + 255) / 256), dim3(256), 0, s, a);
}
void launch_rs_msc(const RsMscArgs& a, hipStream_t s)
{
    const int total = a.n_pairs * a.n_sf_per_pair * a.s;
    if (total <= 0) return;
    hipLaunchKernelGGL(k_rs_msc, dim3((total + 255) / 256), dim3(256), 0, s, a);
}

} // namespace dabphy
