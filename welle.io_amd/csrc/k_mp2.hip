// welle.io_amd/csrc/k_mp2.hip -- the MP2 frame check of classic DAB services: what MP2Decoder::Feed reports for every logical frame
// (src/backend/dab_decoder.cpp:114-250, one Feed per logical frame as DecoderAdapter::addtoFrame calls it, decoder_adapter.cpp:55-77).
//
// Restates, as they act on such a stream:
//   mpg123's feed reader          libs/mpg123/readers.c   bc_give / bc_skip / bc_seekback / bc_forget / bc_need_more (4096-byte blocks)
//   read_frame                    libs/mpg123/parse.c:492-690, head_check :85, head_compatible :434, decode_header :738,
//                                 do_readahead :993, skip_junk :1123, wetwork :1196-1290 (resync byte by byte, no limit)
//   get_next_frame / decode_update  libs/mpg123/libmpg123.c:592-664 (MPG123_NEW_FORMAT), MP2Decoder::ProcessFormat (scf_crc_len)
//   MP2Decoder::CheckCRC          CRC-16 0x8005, inverted initial value (tools.cpp:36) over header bytes 2..3 + allocation + ScFSI
// Not restated (the walk stops claiming equality for the service from that logical frame on: `unverified`): free format, headers of
// another layer or of a sampling rate the decoder has no output format for (the reference throws), Frankenstein streams, ID3 / TAG /
// APE / RIFF tags, CRC-covered bits beyond the frame, a joint-stereo bound beyond the nbal table.  tests/mp2_model.py is the same
// contract in Python; tests/test_mp2_vs_ref.py pins it to the reference itself.  DESIGN.md section 4.7.
//
// Shape: one wavefront per service (k_mp2 below).  Rows of the class output go into an LDS ring of the service's byte stream a chunk at
// a time; lane 0 walks mpg123's parser over them -- headers only -- and queues the frames it returns; the wave checks up to 64 queued
// CRCs at once.  State between batches: the bytes not yet consumed, the reader's positions, the first / old header, the output format
// and scf_crc_len (Mp2State).
#include "dabphy_kernels.h"

namespace dabphy {

namespace {
constexpr int RING = MP2_RING;                    // LDS ring of the byte stream (power of two)
constexpr int NEED_MORE = -10;
constexpr uint32_t CMPMASK = 0xFFE00000u | 0x00180000u | 0x00060000u | 0x00000C00u;

// (the tables as functions of local constants: the CPU execution model of tests/hipemu has no __constant__)
__device__ __forceinline__ int tabsel(int lsf, int lay, int bri)          // tabsel_123 (parse.c:50-62), kbit/s
{
    const int16_t T[2][3][16] = {
        {{0, 32, 64, 96, 128, 160, 192, 224, 256, 288, 320, 352, 384, 416, 448, 0},
         {0, 32, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 384, 0},
         {0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 0}},
        {{0, 32, 48, 56, 64, 80, 96, 112, 128, 144, 160, 176, 192, 224, 256, 0},
         {0, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160, 0},
         {0, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160, 0}}};
    return T[lsf][lay - 1][bri];
}
__device__ __forceinline__ int freq_of(int sf)                              // freqs (parse.c:64)
{
    const int32_t F[9] = {44100, 48000, 32000, 22050, 24000, 16000, 11025, 12000, 8000};
    return F[sf];
}
// MP2Decoder's nbal tables (dab_decoder.cpp:21-50) as runs: how many sub-bands have 4, then 3, then 2 allocation bits
__device__ __forceinline__ int nbal_run(int ti, int k)
{
    const int8_t R[3][3] = {{11, 12, 4}, {2, 6, 0}, {4, 7, 19}};
    return R[ti][k];
}

__device__ __forceinline__ bool head_check(uint32_t h)
{
    return (h & 0xFFE00000u) == 0xFFE00000u && ((h >> 17) & 3) != 0 && ((h >> 12) & 15) != 15 && ((h >> 10) & 3) != 3;
}
__device__ __forceinline__ bool head_compatible(uint32_t a, uint32_t b)
{
    return (a & CMPMASK) == (b & CMPMASK) && ((((a >> 6) & 3) == 3) == (((b >> 6) & 3) == 3));
}
struct HeadInfo { int lay, lsf, m25, sf, framesize; };
__device__ __forceinline__ HeadInfo head_info(uint32_t h)    // decode_header (parse.c:738-880); bit rate index 0 (free format) is caught before
{
    HeadInfo r;
    r.lay = 4 - (int)((h >> 17) & 3);
    const int ver = (h >> 19) & 3;
    if (ver & 2) { r.lsf = (ver & 1) ? 0 : 1; r.m25 = 0; r.sf = (int)((h >> 10) & 3) + r.lsf * 3; }
    else { r.lsf = 1; r.m25 = 1; r.sf = 6 + (int)((h >> 10) & 3); }
    const int bri = (h >> 12) & 15, pad = (h >> 9) & 1;
    const int f = freq_of(r.sf);
    if (r.lay == 1) r.framesize = ((tabsel(r.lsf, 1, bri) * 12000 / f) + pad) * 4 - 4;
    else if (r.lay == 2) r.framesize = tabsel(r.lsf, 2, bri) * 144000 / f + pad - 4;
    else r.framesize = tabsel(r.lsf, 3, bri) * 144000 / (f << r.lsf) + pad - 4;
    return r;
}

// one service's walk: the byte stream lives in the LDS ring at absolute offset & (RING - 1); `total` = bytes fed so far
struct Walk {
    const uint8_t* ring;
    int64_t total, pos, firstpos, ks;
    uint32_t firsthead, oldhead;
    int header_change, framesize, fmt_rate, fmt_ch, scf_crc_len;
    int64_t skipped;
    bool unverified;
    uint32_t memo_h = 0; HeadInfo memo;           // the last header decoded (a stream repeats its header: no table look-up per frame)

    __device__ const HeadInfo& info(uint32_t h) { if (h != memo_h) { memo = head_info(h); memo_h = h; } return memo; }

    __device__ uint8_t at(int64_t a) const { return ring[a & (RING - 1)]; }
    __device__ int more() { pos = firstpos; return NEED_MORE; }
    __device__ bool have(int64_t n) { if (total - pos < n) { more(); return false; } return true; }
    __device__ int back(int64_t n)
    {
        if (n >= 0) { if (pos - n >= ks) { pos -= n; return 0; } return -1; }
        if (!have(-n)) return -1;
        pos -= n; return 0;
    }
    __device__ void forget()
    {
        if (pos == total) ks = pos;
        else ks += (int64_t)4096 * ((pos - ks) / 4096);
        firstpos = pos;
    }
    __device__ bool head_read(uint32_t& h)
    {
        if (!have(4)) return false;
        h = ((uint32_t)at(pos) << 24) | ((uint32_t)at(pos + 1) << 16) | ((uint32_t)at(pos + 2) << 8) | at(pos + 3);
        pos += 4; return true;
    }
    __device__ bool shift(uint32_t& h, bool forget_too)    // forget_head_shift (parse.c:1102-1120)
    {
        if (!have(1)) return false;
        h = (h << 8) | at(pos); pos++; skipped++;
        if (forget_too && !back(4)) { forget(); back(-4); }
        return true;
    }
    // returns 1 with a frame (h, framepos) read, 0 on NEED_MORE; sets `unverified` where the reference's path is not restated
    __device__ int read_frame(uint32_t& h, int64_t& framepos)
    {
        const int oldsize = framesize;
        bool again = true;
        for (;;) {
            if (again) {
                forget();
                if (!head_read(h)) break;
            }
            again = true;
            if (!firsthead && !head_check(h)) {                                  // skip_junk (parse.c:1123-1193)
                if ((h & 0xFFFFFF00u) == 0x49443300u || h == 0x52494646u) { unverified = true; return 0; }
                unsigned fc = 0; bool got = false;
                for (;;) {
                    if (++fc > 1024) fc = 0;
                    if (!shift(h, !fc)) break;
                    if (head_check(h)) { got = true; break; }
                }
                if (!got) break;
            }
            if (head_check(h)) {
                if (((h >> 12) & 15) == 0) { unverified = true; return 0; }      // free format: guess_freeformat_framesize
                framesize = info(h).framesize;
            } else {                                                             // wetwork (parse.c:1196-1290)
                if ((h & 0xFFFFFF00u) == 0x54414700u || (h & 0xFFFFFF00u) == 0x49443300u || h == 0x41504554u) { unverified = true; return 0; }
                unsigned fc = 0; bool got = false;
                for (;;) {
                    if (++fc > 1024) fc = 0;
                    if (!shift(h, !fc)) break;
                    if (head_check(h)) { got = true; break; }
                }
                if (!got) break;
                oldhead = 0;
                again = false;                                                   // PARSE_RESYNC: init_resync with the new header
                continue;
            }
            if (!firsthead) {                                                    // do_readahead (parse.c:993-1047)
                const int64_t start = pos;
                if (!have(framesize)) { back(4); break; }
                pos += framesize;
                uint32_t nh = 0;
                const bool hd = head_read(nh);
                back(pos - start);
                if (!hd) { back(4); break; }
                if (!head_check(nh) || !head_compatible(h, nh)) { oldhead = 0; back(3); continue; }
            }
            framepos = pos - 4;
            if (!have(framesize)) break;                                         // read_frame_body
            pos += framesize;
            if (!firsthead) firsthead = h;
            forget();
            if (header_change < 2) {
                header_change = 2;
                if (oldhead) {
                    if (oldhead == h) header_change = 0;
                    else if (head_compatible(oldhead, h)) header_change = 1;
                    else { unverified = true; return 0; }                        // Frankenstein stream
                } else if (firsthead && !head_compatible(firsthead, h)) { unverified = true; return 0; }
            }
            oldhead = h;
            return 1;
        }
        forget();                                                                // read_frame_bad
        framesize = oldsize;
        return 0;
    }
};

// MP2Decoder::CheckCRC for the frame whose body (after the header) starts at stream offset `b`: 1 / 0, or -1 where it is not restated
// (the covered bits run past the frame, or a joint-stereo bound beyond the nbal table: the reference then reads memory behind it).
// Bytes come from the LDS ring, the CRC runs a byte at a time through crctab (tools.cpp: CalcCRC::FillLUT / ProcessByte), the last
// partial byte bit by bit (ProcessBits).
__device__ int mp2_crc(const uint8_t* ring, const uint16_t* crctab, uint32_t h, int64_t b, int framesize, const HeadInfo& hi)
{
    if ((h >> 16) & 1) return 0;                                                 // no CRC: counted as a failure
    auto at = [&](int64_t a) -> uint32_t { return ring[a & (RING - 1)]; };
    const int mode = (h >> 6) & 3, nch = mode == 3 ? 1 : 2;
    const int bitrate = tabsel(hi.lsf, hi.lay, (h >> 12) & 15);
    const bool v1 = !hi.lsf && !hi.m25;
    const int ti = v1 ? (bitrate / nch >= 56 ? 0 : 1) : 2;
    const int n4 = nbal_run(ti, 0), n3 = nbal_run(ti, 1), sblimit = n4 + n3 + nbal_run(ti, 2);
    const int bound = mode == 1 ? ((int)((h >> 4) & 3) + 1) * 4 : sblimit;
    if (bound > sblimit) return -1;
    const int avail = (framesize - 2) * 8;                                       // BitReader over body[2 ..)
    // the allocation fields one after the other (a 32-bit window refilled a byte at a time); the covered length adds 2 ScFSI bits per
    // channel with a non-zero allocation
    uint32_t win = 0; int wbits = 0, p = 0, n = 0;
    int64_t next = b + 2;
    for (int sb = 0; sb < sblimit; sb++) {
        const int nbal = sb < n4 ? 4 : sb < n4 + n3 ? 3 : 2;
        const int chs = sb < bound ? nch : 1;
        for (int ch = 0; ch < chs; ch++) {
            if (p + nbal > avail) return 0;                                      // BitReader ran out
            while (wbits < nbal) { win = (win << 8) | at(next++); wbits += 8; }
            const uint32_t v = (win >> (wbits - nbal)) & ((1u << nbal) - 1);
            wbits -= nbal; p += nbal;
            n += nbal + (v ? (sb < bound ? 2 : 2 * nch) : 0);
        }
    }
    if (n > avail) return -1;
    uint32_t crc = 0xFFFF;
    crc = ((crc << 8) ^ crctab[((crc >> 8) ^ ((h >> 8) & 0xFF)) & 0xFF]) & 0xFFFF;
    crc = ((crc << 8) ^ crctab[((crc >> 8) ^ (h & 0xFF)) & 0xFF]) & 0xFFFF;
    for (int k = 0; k < (n >> 3); k++) crc = ((crc << 8) ^ crctab[((crc >> 8) ^ at(b + 2 + k)) & 0xFF]) & 0xFFFF;
    const uint32_t last = at(b + 2 + (n >> 3));
    for (int i = 0; i < (n & 7); i++) {
        const uint32_t fb = ((crc >> 15) & 1) ^ ((last >> (7 - i)) & 1);
        crc = (crc << 1) & 0xFFFF;
        if (fb) crc ^= 0x8005;
    }
    return crc == ((at(b) << 8) | at(b + 1)) ? 1 : 0;
}

struct Mp2Queued { int64_t pos; uint32_t h; int32_t r; int16_t framesize; uint8_t new_format, scf_crc_len; };
constexpr int MP2_QCAP = 64;                    // frames whose CRCs the wave checks at once (one per lane)
} // namespace

// One wavefront per service.  Rows travel HBM -> LDS ring a chunk at a time (as many as the ring can take beside what mpg123 may still
// read); lane 0 walks the parser over them and queues the frames it returns; the wave then checks up to 64 queued CRCs at once, and lane 0
// books them in order -- events, the AudioErrors of each logical frame, and the end of the claim where a path is not restated.
__global__ void __launch_bounds__(64) k_mp2(Mp2Args A)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_ring[RING];
    __shared__ uint16_t s_crctab[256];
    __shared__ Mp2Queued s_q[MP2_QCAP];
    __shared__ int s_ok[MP2_QCAP];
    __shared__ int s_k, s_copy, s_qn, s_seg_end;
    __shared__ int64_t s_total, s_from;
    const int t = threadIdx.x;
    const int bm = A.run ? A.run[blockIdx.x] : (int)blockIdx.x;                  // the pair (service)
    const int fb = A.frame_bytes;
    Mp2State* st = reinterpret_cast<Mp2State*>(A.state + (size_t)bm * A.state_stride);
    uint8_t* carry = A.state + (size_t)bm * A.state_stride + sizeof(Mp2State);
    // which rows of this batch the service decoded: every row (unit entry), or as the DAB+ filter counts them (batch_rows.h)
    int r_first = 0, n_rows = A.n_cif;
    const int b = A.pairs ? A.pairs[bm].ens : 0;
    if (A.desc) {
        int nv = 0;
        for (int f = 0; f < A.n_frames; f++) nv += A.desc[(size_t)b * A.n_frames + f].valid == 1 ? 1 : 0;
        n_rows = 4 * nv;
        r_first = batch_first_row(A.desc[(size_t)b * A.n_frames].frame_no, A.pairs[bm].cif0, n_rows);
    }
    const int carry_len = st->carry_len;
    const int64_t origin = st->origin;
    for (int i = t; i < carry_len; i += 64) s_ring[(origin + i) & (RING - 1)] = carry[i];
    for (int v = t; v < 256; v += 64) {                                            // CalcCRC::FillLUT, polynomial 0x8005
        uint32_t c = (uint32_t)v << 8;
        for (int i = 0; i < 8; i++) c = (c & 0x8000) ? ((c << 1) ^ 0x8005) : (c << 1);
        s_crctab[v] = (uint16_t)(c & 0xFFFF);
    }
    int32_t* errs = A.frame_errors ? A.frame_errors + (size_t)bm * A.n_cif : nullptr;
    if (errs) for (int r = t; r < A.n_cif; r += 64) errs[r] = 0;
    Walk w;                                                                      // (lane 0's)
    w.ring = s_ring;
    w.total = origin + carry_len; w.pos = st->pos; w.firstpos = st->firstpos; w.ks = st->ks;
    w.firsthead = st->firsthead; w.oldhead = st->oldhead; w.header_change = st->header_change; w.framesize = st->framesize;
    w.fmt_rate = st->fmt_rate; w.fmt_ch = st->fmt_ch; w.scf_crc_len = st->scf_crc_len;
    w.skipped = 0; w.unverified = st->unverified != 0;
    int ne = 0, n_frames = 0, n_err = 0, first_unv = (w.unverified && r_first < n_rows) ? r_first : -1;
    Mp2Event* ev = A.events ? A.events + (size_t)bm * A.ev_cap : nullptr;
    const int row_frames_max = fb / 48 + 2;                                      // Layer II frames a row can hold (>= 48 bytes each) + one begun before
    __syncthreads();
    for (int r = r_first; r < n_rows;) {
        if (t == 0) {
            const int64_t room = RING - (w.total - (w.firstpos - 4));
            int K = room / fb < (int64_t)(n_rows - r) ? (int)(room / fb) : n_rows - r;
            s_copy = !w.unverified && K > 0;
            if (!w.unverified && K <= 0) { w.unverified = true; if (first_unv < 0) first_unv = r; }   // (bounded by construction: tests/mp2_model.py)
            if (!s_copy) K = n_rows - r;
            s_k = K; s_total = w.total;
        }
        __syncthreads();
        const int K = s_k;
        if (!s_copy) { r += K; __syncthreads(); continue; }
        const int64_t tot0 = s_total;
        for (int k = 0; k < K; k++) {
            const uint8_t* row = A.out + ((size_t)bm * A.n_cif + r + k) * fb;
            for (int i = t; i < fb; i += 64) s_ring[(tot0 + (int64_t)k * fb + i) & (RING - 1)] = row[i];
        }
        __syncthreads();
        for (int done = 0; done < K;) {
            if (t == 0) {
                int qn = 0, rr = r + done;
                while (rr < r + K && qn + row_frames_max <= MP2_QCAP && !w.unverified) {
                    w.total += fb;
                    uint32_t h; int64_t fp;
                    while (w.read_frame(h, fp)) {
                        const HeadInfo hi = w.info(h);
                        if (hi.lay != 2) { w.unverified = true; break; }
                        bool new_format = false;
                        if (w.header_change > 1) {
                            w.header_change = 0;
                            const int rate = freq_of(hi.sf), ch = ((h >> 6) & 3) == 3 ? 1 : 2;
                            if (rate != 48000 && rate != 24000) { w.unverified = true; break; }      // decode_update fails: the reference throws
                            if (rate != w.fmt_rate || ch != w.fmt_ch) { w.fmt_rate = rate; w.fmt_ch = ch; new_format = true; }
                        }
                        if (new_format) {
                            const int bitrate = tabsel(hi.lsf, 2, (h >> 12) & 15);
                            w.scf_crc_len = (!hi.lsf && !hi.m25 && bitrate < (((h >> 6) & 3) == 3 ? 56 : 112)) ? 2 : 4;
                        }
                        Mp2Queued q; q.pos = fp; q.h = h; q.r = rr; q.framesize = (int16_t)w.framesize; q.new_format = new_format; q.scf_crc_len = (uint8_t)w.scf_crc_len;
                        s_q[qn++] = q;
                    }
                    if (w.unverified && first_unv < 0) first_unv = rr;
                    rr++;
                }
                if (w.unverified) {                                              // nothing more is claimed: the rest of the chunk is not walked
                    if (rr < r + K) w.total += (int64_t)(r + K - rr) * fb;
                    rr = r + K;
                }
                s_qn = qn; s_seg_end = rr;
            }
            __syncthreads();
            const int qn = s_qn;
            if (t < qn) {
                const Mp2Queued q = s_q[t];
                s_ok[t] = mp2_crc(s_ring, s_crctab, q.h, q.pos + 4, q.framesize, head_info(q.h));
            }
            __syncthreads();
            if (t == 0) {                                                        // book the frames in stream order
                int row = -1, row_ne0 = ne, row_err = 0;
                for (int j = 0; j < qn; j++) {
                    const Mp2Queued q = s_q[j];
                    if (first_unv >= 0 && q.r >= first_unv) break;
                    if (q.r != row) {
                        if (row >= 0 && errs) errs[row] = row_err;
                        row = q.r; row_ne0 = ne; row_err = 0;
                    }
                    const int ok = s_ok[j];
                    if (ok < 0) { first_unv = q.r; w.unverified = true; n_frames -= ne - row_ne0; n_err -= row_err; ne = row_ne0; row = -1; break; }
                    if (ev && ne < A.ev_cap) {
                        Mp2Event e;
                        e.frame = q.r; e.header = q.h; e.offset = q.pos;
                        e.crc_ok = (uint8_t)ok; e.new_format = q.new_format; e.scf_crc_len = q.scf_crc_len;
                        e.fpad[0] = s_ring[(q.pos + 4 + q.framesize - 2) & (RING - 1)]; e.fpad[1] = s_ring[(q.pos + 4 + q.framesize - 1) & (RING - 1)];
                        e.pad_[0] = e.pad_[1] = e.pad_[2] = 0;
                        ev[ne] = e;
                    }
                    ne++; n_frames++;
                    if (!ok) { row_err++; n_err++; }
                }
                if (row >= 0 && errs) errs[row] = row_err;
            }
            __syncthreads();
            done = s_seg_end - r;
            __syncthreads();
        }
        r += K;
    }
    // the bytes a later feed can still reach: [max(firstpos - 4, ks), total)
    if (t == 0) {
        int64_t from = w.firstpos - 4 > w.ks ? w.firstpos - 4 : w.ks;
        if (from < w.total - MP2_CARRY) { from = w.total - MP2_CARRY; w.unverified = true; }
        s_k = (int)(w.total - from); s_from = from;
        st->origin = from; st->carry_len = (int32_t)(w.total - from);
        st->pos = w.pos; st->firstpos = w.firstpos; st->ks = w.ks;
        st->firsthead = w.firsthead; st->oldhead = w.oldhead; st->header_change = w.header_change; st->framesize = w.framesize;
        st->fmt_rate = w.fmt_rate; st->fmt_ch = w.fmt_ch; st->scf_crc_len = w.scf_crc_len; st->unverified = w.unverified;
        if (A.n_events) A.n_events[bm] = ne;
        if (A.first_unverified) A.first_unverified[bm] = first_unv;
        if (A.stats) {
            atomicAdd(A.stats + 4 * b, n_frames); atomicAdd(A.stats + 4 * b + 1, n_err);
            atomicAdd(A.stats + 4 * b + 2, (int)w.skipped); atomicAdd(A.stats + 4 * b + 3, first_unv >= 0 ? n_rows - first_unv : 0);
        }
    }
    __syncthreads();
    const int64_t from = s_from;
    const int n_carry = s_k;
    for (int i = t; i < n_carry; i += 64) carry[i] = s_ring[(from + i) & (RING - 1)];
}

void launch_mp2(const Mp2Args& a, int n_blocks, hipStream_t s)
{
    if (n_blocks <= 0) return;
    hipLaunchKernelGGL(k_mp2, dim3(n_blocks), dim3(64), 0, s, a);
}

} // namespace dabphy
