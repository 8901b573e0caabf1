// welle.io_amd/csrc/k_superframe.hip -- the DAB+ superframe filter (SuperframeFilter::Feed / CheckSync, dabplus_decoder.cpp:50-213) on the
// class output of a batch -- k_superframe_wide + k_superframe_settle (every attempt a receiver in lock makes in the batch at once,
// accepted per sub-channel iff all of them synchronise) and k_superframe (the reference's walk frame by frame, for what is left).
// The code of its Reed-Solomon step is rs_codec.h; which rows a pair decoded and how its window is carried: batch_rows.h.
#include "rs_codec.h"
#include <dabphy_wave_ops.h>

namespace dabphy {

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
// ... and that table for CRC-16-CCITT (0x1021), by the 64 lanes of a wave; the callers' barrier follows
__device__ __forceinline__ void crc_ccitt_table(uint16_t* tab, int t)
{
    for (int v = t; v < 256; v += 64) {
        uint16_t c = (uint16_t)(v << 8);
        for (int i = 0; i < 8; i++) c = (c & 0x8000) ? (uint16_t)((c << 1) ^ 0x1021) : (uint16_t)(c << 1);
        tab[v] = c;
    }
}

constexpr int SF_PREFETCH = 6;      // rows of the class output in flight per work-group (serial walk)

// What the three kernels start with: the class's argument block, the work-group's pair and its ensemble, the pair's carried state and
// its events (its plan, sf_plan below, is a call of its own: the walk leaves for a settled pair before it needs one).
// Every class of a bucket (same LDS size) in ONE launch: block -> (class, its block) through the bucket's table of first blocks; the class's
// argument block comes from HBM.  A real multiplex has a handful of protection classes, a batch of independent ensembles a few dozen:
// one launch per class and kernel was 60 dependent launches of a few work-groups each at the end of every step.
struct SfStart { SfArgs A; size_t bm; int ens; uint8_t* st; SfEvent* ev; };
__device__ __forceinline__ SfStart sf_start(const SfBatch& Bt)
{
    // (everything here is wave-uniform and read-only: through the constant address space these are scalar loads, the argument block
    // lives in scalar registers as a kernel argument would)
    const DABPHY_CONST_AS int32_t* first = as_constant(Bt.first);
    uint32_t bx = blockIdx.x; int c = 0;
    while (c + 1 < Bt.n_cls && bx >= (uint32_t)first[c + 1]) c++;
    bx -= (uint32_t)first[c];
    const DABPHY_CONST_AS SfArgs* cls = as_constant(Bt.cls);
    SfStart S;
    __builtin_memcpy(&S.A, (const void DABPHY_CONST_AS*)&cls[c], sizeof S.A);
    S.bm = S.A.run ? (size_t)S.A.run[bx] : (size_t)bx;
    S.ens = S.A.pairs[S.bm].ens;
    S.st = S.A.state + S.bm * S.A.state_stride; S.ev = S.A.events + S.bm * S.A.n_cif;
    return S;
}
// ... and what the two that settle a pair end with, by one lane: the frames carried on, the events there are and the batch's totals
// (by reference: an LDS total is read where it is added)
__device__ __forceinline__ void sf_end(const SfStart& S, int frame_count, int ne, int n_sync, const int& corr, const int& unc, const int& aubad)
{
    sf_state_count(S.st) = frame_count; S.A.n_events[S.bm] = ne;
    if (int32_t* const stats = S.A.stats) { atomicAdd(stats + 4 * S.ens, n_sync); atomicAdd(stats + 4 * S.ens + 1, corr); atomicAdd(stats + 4 * S.ens + 2, unc); atomicAdd(stats + 4 * S.ens + 3, aubad); }
}

// What the batch holds for one (ensemble, sub-channel) pair: fc frames carried in, of which the window machine still uses the last cu (a full
// window that failed drops its oldest frame with the next one, dabplus_decoder.cpp:78-81); rows [r_first, n_rows) of the class output
// are the frames it will be fed (rows are packed: k_msc_gather lays the logical frames of an ensemble out in CIF order from the first
// frame number of the batch, whatever slots the demodulated frames occupied; frames before the 16-CIF fill of the time de-interleaver
// are never emitted: batch_rows.h).  If every attempt synchronises, attempts happen at frames 5q + 4 of that sequence: nq of them.
struct SfPlan { int fc, cu, n_rows, r_first, avail, nq; };
// (called by all 64 lanes of the work-group's wave together: lane t looks at frame t, t + 64, ... -- one round trip to memory for the batch's
// descriptors where a loop over the frames makes one per frame)
__device__ __forceinline__ SfPlan sf_plan(const SfStart& S, int t)
{
    const SfArgs& A = S.A; const MscPair& pp = A.pairs[S.bm]; const int b = pp.ens;
    SfPlan p;
    p.fc = sf_state_count(S.st);
    p.cu = p.fc == 5 ? 4 : p.fc;
    int nv = 0;
    for (int f0 = 0; f0 < A.n_frames; f0 += 64) {
        const int f = f0 + t;
        nv += __popcll(__ballot(f < A.n_frames && A.desc[(size_t)b * A.n_frames + (f < A.n_frames ? f : 0)].valid == 1));
    }
    p.n_rows = 4 * nv;
    p.r_first = batch_first_row(A.desc[(size_t)b * A.n_frames].frame_no, pp.cif0, p.n_rows);
    p.avail = p.n_rows - p.r_first;
    p.nq = p.avail > 0 ? (p.cu + p.avail) / 5 : 0;
    return p;
}

// Reed-Solomon over the code words of 5-frame copies in s_sf (dabplus_decoder.cpp:97) by the 64 lanes of one wave, in two forms that hand
// rs_correct120 the same syndromes; corr[a] / unc[a] (LDS, zeroed here) = attempt a's corrected symbols / whether a word was given up,
// valid for all threads on return.
// A code word per lane: the s code words of each of the attempts a_first .. n_att - 1, copies sf_len bytes apart (attempt t / s, word
// t % s; n_att s <= 64); the lane divides its word by the generator polynomial: 120 dependent steps of one look-up each, and nothing more
// for a clean word.  64 code words per wave: the wide pass.  gtab = the remainder table in LDS, s_ws = 64 workspaces.
__device__ __forceinline__ void sf_rs_word_per_lane(uint8_t* s_sf, int sf_len, int s, int a_first, int n_att, const uint8_t* alpha_to, const uint8_t* index_of, const uint4* gtab, uint8_t* s_ws, int* corr, int* unc, int t)
{
    if (t < n_att) { corr[t] = 0; unc[t] = 0; }
    __syncthreads();
    const int a = t / s, c = t - a * s;
    if (a >= a_first && a < n_att) {
        RsIo io; io.base = s_sf + a * sf_len + c; io.pos_stride = (size_t)s;
        const int n = rs_decode120(io, alpha_to, index_of, gtab, s_ws + t * RS_WS_BYTES);
        if (n < 0) atomicOr(&unc[a], 1); else if (n > 0) atomicAdd(&corr[a], n);
    }
    __syncthreads();
}
// Eight code words per wave: the s code words of ONE attempt, eight at a time with the whole wave, each word's positions split over eight
// lanes: 15 independent steps per lane.  The serial walk makes one attempt at a time on one wave and at most 48 code words would leave
// its lanes idle through 120 dependent steps: it keeps this form.  s_ws = 8 workspaces.
__device__ __forceinline__ void sf_rs_eight_per_wave(uint8_t* s_sf, int s, const uint8_t* alpha_to, const uint8_t* index_of, uint8_t* s_ws, int* corr, int* unc, int t)
{
    if (t < 1) { corr[t] = 0; unc[t] = 0; }              // (one attempt; indexed by the lane like the other form: a fixed address cost k_superframe a register)
    __syncthreads();
    // Syndromes: S_i = XOR_j d_j alpha^(i (119 - j)) is a sum, so lane
    // (codeword c = l & 7, byte group l >> 3 = 15 positions) adds its terms without any chain of dependent look-ups and
    // three butterfly exchanges fold the eight groups (Horner's 119 dependent steps were the whole cost of this kernel).
    for (int c0 = 0; c0 < s; c0 += 8) {
        const int c = c0 + (t & 7), jg = t >> 3;
        uint32_t syn[RS_NROOTS] = {};
        if (c < s) {
#pragma unroll 3
            for (int j = jg * 15; j < jg * 15 + 15; j++) rs_syndrome_term(syn, s_sf[j * s + c], (uint32_t)(RS_LEN - 1 - j), alpha_to, index_of);      // x^(119 - j) at x = alpha^i
        }
#pragma unroll
        for (int i = 0; i < RS_NROOTS; i++) { syn[i] ^= __shfl_xor(syn[i], 8); syn[i] ^= __shfl_xor(syn[i], 16); syn[i] ^= __shfl_xor(syn[i], 32); }
        if (jg == 0 && c < s) {
            RsIo io; io.base = s_sf + c; io.pos_stride = (size_t)s;
            const int n = rs_correct120(io, syn, alpha_to, index_of, s_ws + (t & 7) * RS_WS_BYTES);
            if (n < 0) atomicOr(unc, 1); else if (n > 0) atomicAdd(corr, n);
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
// A work-group takes as many consecutive attempts of its pair as fill its 64 lanes with code words: 64 / s of them (eight at 64 kbit/s, one
// above 256 kbit/s; s <= 48), blockIdx.y = which ones.  Their windows are 64 / s * 120 s <= 7680 bytes of LDS whatever the bit rate; the
// buckets' instances differ in the attempts a work-group can hold (64 / 7 / 2: a bucket's smallest s is one more than the bucket below
// holds).  The launch keeps its grid of one row per
// attempt of the batch -- the queue-order records (tests/queue_order) pin the launches of dabphy_process, grids included --; the rows behind
// the Bt.wide_rows that have work for the launch's largest s return before they touch memory (the heavy rows are dispatched first; measured:
// profiles/sf_wide_remainder.txt).  Once per work-group instead of once per attempt: the class's argument block, sf_plan (a descriptor per frame
// of the batch) and the tables.  Consecutive attempts read consecutive frames: one coalesced copy (two where attempt 0 starts in the carried
// frames of the state), and one copy out when all of them synchronise.
// Bt.replay (dabphy_time_superframe_wide): the launch repeats the pass of a batch that k_superframe_settle has settled since -- the state holds the
// frames carried OUT of the batch, no longer those carried in.  How many were carried in follows from the first event's row; the attempt
// that read them is left out (its event and superframe stay), every other attempt rewrites what it wrote.  Pairs that were walked are left out.
constexpr int SF_WIDE_LANES = 64, SF_WIDE_LDS = SF_WIDE_LANES * RS_LEN;
constexpr int sf_bucket_below(int sf_max) { int v = 0; for (int n : SF_BUCKET_BYTES) if (n < sf_max) v = n; return v; }      // 0 below the first
template <int SF_MAX>       // superframe bytes of the bucket (120 s)
__global__ void __launch_bounds__(64) k_superframe_wide(SfBatch Bt)
{
    if ((int)blockIdx.y >= Bt.wide_rows) return;
    constexpr int MAX_ATT = SF_WIDE_LANES / (sf_bucket_below(SF_MAX) / RS_LEN + 1);
    __shared__ __attribute__((aligned(16))) uint8_t s_sf[SF_WIDE_LDS];
    __shared__ __attribute__((aligned(16))) uint8_t alpha_to[256], index_of[256];
    __shared__ uint4 s_gtab[RS_GTAB_BYTES / 16];
    __shared__ int s_corr[MAX_ATT], s_unc[MAX_ATT], s_sync[MAX_ATT];
    __shared__ uint8_t s_ws[SF_WIDE_LANES * RS_WS_BYTES];       // error-path workspaces, one per code-word lane
    const int t = threadIdx.x;
    const SfStart S = sf_start(Bt);
    const SfArgs& A = S.A; const size_t bm = S.bm;
    const int s = A.s, fb = A.frame_bytes, sf_len = 5 * fb, fw = fb >> 3;
    const int per_group = SF_WIDE_LANES / s < MAX_ATT ? SF_WIDE_LANES / s : MAX_ATT;
    const int q0 = (int)blockIdx.y * per_group;                   // the work-group's first attempt
    SfPlan p = sf_plan(S, t);
    int q_first = 0;
    if (Bt.replay) {
        if (!A.accepted[bm] || A.n_events[bm] < 1) return;
        const int cu = p.r_first + 4 - S.ev[0].cif;
        if (cu < 0 || cu > 4) return;
        p.fc = p.cu = cu; p.nq = p.avail > 0 ? (cu + p.avail) / 5 : 0;
        q_first = cu > 0;
    }
    if (q0 >= p.nq) return;
    const int na = p.nq - q0 < per_group ? p.nq - q0 : per_group;
    rs_tables<64>(A.gf, alpha_to, index_of, s_gtab, t);
    {
        // frames 5 q0 .. 5 (q0 + na) of (carried frames, then rows): the first n_st from the state, the rest consecutive rows of the class output
        const int g0 = 5 * q0, ng = 5 * na;
        const int n_st = p.cu - g0 <= 0 ? 0 : p.cu - g0 < ng ? p.cu - g0 : ng;
        if (n_st) sf_copy_in(reinterpret_cast<uint2*>(s_sf), reinterpret_cast<const uint2*>(sf_state_frames(S.st) + (size_t)(p.fc - p.cu + g0) * fb), n_st * fw, t);
        sf_copy_in(reinterpret_cast<uint2*>(s_sf + n_st * fb), reinterpret_cast<const uint2*>(A.out + (bm * A.n_cif + (p.r_first + g0 + n_st - p.cu)) * fb), (ng - n_st) * fw, t);
    }
    sf_rs_word_per_lane(s_sf, sf_len, s, q0 < q_first, na, alpha_to, index_of, s_gtab, s_ws, s_corr, s_unc, t);
    if (t < na) {                                                              // one lane per attempt
        const int q = q0 + t;
        SfEvent e;
        const int sync = sf_check_sync(s_sf + t * sf_len, sf_len, s_corr[t], s_unc[t], e);
        e.cif = p.r_first + 5 * q + 4 - p.cu;                                  // the row whose arrival triggers the attempt
        if (sync) e.sf_slot = q;
        s_sync[t] = sync && q >= q_first;
        if (q >= q_first) S.ev[q] = e;
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
    __shared__ uint16_t s_crctab[256];
    __shared__ int s_ok, s_corr, s_unc, s_aubad;
    const int t = threadIdx.x;
    const SfStart S = sf_start(Bt);
    const SfArgs& A = S.A; const size_t bm = S.bm; SfEvent* const ev = S.ev;
    const int fb = A.frame_bytes, sf_len = 5 * fb, fw = fb >> 3;
    const SfPlan p = sf_plan(S, t);
    crc_ccitt_table(s_crctab, t);
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
        for (int i = t; i < fw; i += 64) reinterpret_cast<uint2*>(sf_state_frames(S.st) + (size_t)k * fb)[i] = reinterpret_cast<const uint2*>(src)[i];
    }
    __syncthreads();
    if (t == 0) sf_end(S, n_left, p.nq, p.nq, s_corr, s_unc, s_aubad);
}

// ---- The serial walk: SuperframeFilter::Feed / CheckSync (dabplus_decoder.cpp:50-213) for one sub-channel of one ensemble, frame by
// frame with the reference's state machine -- 5-frame sliding window, Reed-Solomon on a copy, Fire-code / AU-table check, AU CRCs, and
// after a hit a fresh window -- carrying frame_count + the raw window to the next batch.  Runs for what the wide pass did not settle.
template <int SF_MAX>       // superframe bytes the instance can hold (120 * bitrate / 8)
__global__ void __launch_bounds__(64, SF_MAX <= 2880 ? 4 : 2) k_superframe(SfBatch Bt)      // (four waves per SIMD: at five the 960-byte build spilled ten registers)
{
    // LDS: the raw 5-frame window (a ring: `head` = oldest frame, nothing is ever shifted) and the working copy
    __shared__ __attribute__((aligned(16))) uint8_t s_dyn[2 * SF_MAX];
    __shared__ __attribute__((aligned(16))) uint8_t alpha_to[256], index_of[256];
    __shared__ struct { int corr, unc, sync; } sh;            // one attempt's verdict, valid for all threads behind its barrier
    __shared__ int s_aubad;
    __shared__ uint8_t s_ws[8 * RS_WS_BYTES];                   // error-path workspaces of the eight code words decoded at a time
    __shared__ uint16_t s_crctab[256];                          // CRC-16-CCITT (0x1021), one byte per step: the AU checks
    const int t = threadIdx.x;
    const SfStart S = sf_start(Bt);
    const SfArgs& A = S.A; const size_t bm = S.bm; SfEvent* const ev = S.ev;
    if (A.accepted && A.accepted[bm]) return;                  // settled by the wide pass
    rs_tables<64>(A.gf, alpha_to, index_of, nullptr, t);
    crc_ccitt_table(s_crctab, t);
    if (t == 0) s_aubad = 0;
    const int fb = A.frame_bytes, sf_len = 5 * fb;
    uint8_t* const s_raw = s_dyn;
    uint8_t* const s_sf = s_dyn + SF_MAX;
    const SfPlan p = sf_plan(S, t);
    int frame_count = p.fc;
    __syncthreads();
    for (int i = t; i < frame_count * fb; i += 64) s_raw[i] = sf_state_frames(S.st)[i];   // carried frames, oldest first
    int head = 0;                                                              // ring slot of the oldest frame
    int ne = 0, slot = 0;
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
        SfEvent e;                                                             // Reed-Solomon over its s code words, then CheckSync by thread 0
        sf_rs_eight_per_wave(s_sf, A.s, alpha_to, index_of, s_ws, &sh.corr, &sh.unc, t);
        if (t == 0) sh.sync = sf_check_sync(s_sf, sf_len, sh.corr, sh.unc, e);
        __syncthreads();
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
        sf_state_frames(S.st)[i] = s_raw[sl * fb + i % fb];
    }
    if (t == 0) sf_end(S, frame_count, ne, tot_sync, tot_corr, tot_unc, s_aubad);
}

// bucket = index of the kernels' LDS size (SF_BUCKET_BYTES); Bt.cls are the
// classes of that bucket (DEVICE array), total_blocks = Bt.first[n_cls] (known to the host), n_cif = CIFs per batch, wide = run the wide pass.
// The bucket's instance of the kernel template K, launched.  (A macro, with the sizes written out: the execution model's queue-order
// records, tests/queue_order, name a launch by the text of its kernel argument)
#define SF_LAUNCH_BUCKET(K, bucket, grid, s, Bt) \
    do { if ((bucket) == 0) hipLaunchKernelGGL(K<960>, grid, dim3(64), 0, s, Bt); \
         else if ((bucket) == 1) hipLaunchKernelGGL(K<2880>, grid, dim3(64), 0, s, Bt); \
         else hipLaunchKernelGGL(K<5760>, grid, dim3(64), 0, s, Bt); } while (0)
static_assert(SF_BUCKET_BYTES[0] == 960 && SF_BUCKET_BYTES[1] == 2880 && SF_BUCKET_BYTES[2] == 5760, "SF_LAUNCH_BUCKET writes the buckets' sizes out");

// the wide pass alone: a grid row per attempt of the batch, (n_cif + 4) / 5, of which the first wide_rows have work: 64 / s attempts per
// work-group, counted for the launch's largest s (the surplus work-groups of classes with a smaller one leave once they have their plan)
void launch_superframe_wide(SfBatch Bt, int bucket, int total_blocks, int n_cif, int max_s, hipStream_t s)
{
    if (total_blocks <= 0 || max_s < 1 || max_s > SF_WIDE_LANES) return;
    const int per_group = SF_WIDE_LANES / max_s, attempts = (n_cif + 4) / 5;
    Bt.wide_rows = (attempts + per_group - 1) / per_group;
    SF_LAUNCH_BUCKET(k_superframe_wide, bucket, dim3(total_blocks, attempts), s, Bt);
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
    SF_LAUNCH_BUCKET(k_superframe, bucket, grid, s, Bt);
}

} // namespace dabphy
