// welle.io_amd/csrc/k_au.hip -- the pack pass behind the DAB+ superframe filter: every access unit that passed its CRC, CRC stripped,
// back to back in the service's region of a staging buffer -- as AACDecoder::DecodeFrame receives it (DABPHY_AU_RAW) or wrapped into one
// LATM/LOAS AudioSyncStream frame as SuperframeFilter::ProcessUntouchedStream builds it (DABPHY_AU_LOAS; dabplus_decoder.cpp:121-138,
// :257-312).  tests/au_model.py is the same contract in Python; tests/test_au_vs_ref.py pins it to the reference itself.
//
// A LOAS frame, bit by bit: sync word 0x2B7 (11), audioMuxLengthBytes = frame length - 3 (13), useSameStreamMux 0 (1), StreamMuxConfig
// (audioMuxVersion 0, allStreamsSameTimeFraming 1, numSubFrames 0 (6), numProgram 0 (4), numLayer 0 (3)), the AudioSpecificConfig from
// sf[2] -- with SBR 5+4+4+4+5+3 bits, without 5+4+4+3 --, frameLengthType 0 (3), latmBufferFullness 0xFF (8), two zero bits: H = 69 bits
// without SBR, 78 with.  Then len / 255 bytes 0xFF and len % 255, the payload, zero bits up to the byte boundary.  Everything behind the
// H header bits is a byte stream shifted right by H % 8 = 5 or 6 bits.
//
// Shape: one work-group of four waves per (ensemble, sub-channel) pair.  Wave 0 reads the pair's events, one per lane, and scans the
// lengths of what they store (the exclusive scan over at most (4F/5 + 1) x 6 lengths gives every access unit its place); it writes the
// access-unit table and the service record.  Then every wave takes access units in turn: the lanes write ALIGNED destination dwords,
// each funnel-shifted out of two aligned source dwords -- source misalignment, destination misalignment and the 5/6-bit shift fold into
// one bit offset --; the bytes in front of the first whole dword (header, length bytes) and behind the last are written once per
// access unit, a byte per lane.
#include "dabphy_kernels.h"

namespace dabphy {

namespace {
__device__ __forceinline__ int au_header_bits(int fmt) { return fmt & 0x20 ? 78 : 69; }
// bytes a stored access unit of `len` payload bytes takes
__device__ __forceinline__ int au_stored_len(int len, int fmt, int format)
{
    return format == AU_FORMAT_LOAS ? (au_header_bits(fmt) + 8 * (len / 255 + 1) + 8 * len + 7) / 8 : len;
}
// the H header bits, left-aligned in hi (first 64) and lo (the rest); flen = length of the whole frame in bytes
__device__ __forceinline__ void au_header(int fmt, int flen, uint64_t& hi, uint32_t& lo)
{
    int n = 0; hi = 0; lo = 0;
    auto add = [&](uint32_t v, int nb) {
        if (n + nb <= 64) hi |= (uint64_t)v << (64 - n - nb);
        else if (n >= 64) lo |= v << (32 - (n - 64) - nb);
        else { const int a = 64 - n; hi |= (uint64_t)(v >> (nb - a)); lo |= (v & ((1u << (nb - a)) - 1u)) << (32 - (nb - a)); }
        n += nb;
    };
    const bool dac = fmt & 0x40, sbr = fmt & 0x20;
    const uint32_t core_sr = dac ? (sbr ? 6 : 3) : (sbr ? 8 : 5), ch = fmt & 0x10 ? 2 : 1, ext_sr = dac ? 3 : 5;      // dabplus_decoder.h:55-63
    add(0x2B7, 11); add((uint32_t)(flen - 3), 13);
    add(0, 1);                                                        // useSameStreamMux
    add(0, 1); add(1, 1); add(0, 6); add(0, 4); add(0, 3);            // StreamMuxConfig
    if (sbr) { add(5, 5); add(core_sr, 4); add(ch, 4); add(ext_sr, 4); add(2, 5); add(4, 3); }
    else { add(2, 5); add(core_sr, 4); add(ch, 4); add(4, 3); }
    add(0, 3); add(0xFF, 8); add(0, 1); add(0, 1);
}
__device__ __forceinline__ uint32_t au_header_byte(uint64_t hi, uint32_t lo, int i)
{
    return i < 8 ? (uint32_t)(hi >> (56 - 8 * i)) & 0xFFu : (lo >> (24 - 8 * (i - 8))) & 0xFFu;
}
// byte m of the byte stream behind the header: PayloadLengthInfo, the payload, zeros
__device__ __forceinline__ uint32_t au_tail_byte(const uint8_t* __restrict__ src, int len, int m)
{
    const int n255 = len / 255;
    if (m < n255) return 0xFFu;
    if (m == n255) return (uint32_t)(len % 255);
    const int k = m - n255 - 1;
    return k < len ? src[k] : 0u;
}
}

// access unit i of a synchronised event is stored: it passed its CRC (and lies inside the superframe, which the filter's events always do)
__device__ __forceinline__ bool au_stored_ok(const SfEvent& e, int i, int len, int sf_len)
{
    return (e.au_crc_ok >> i & 1) && len >= 0 && e.au_start[i] >= 0 && e.au_start[i + 1] <= sf_len;
}

struct AuScan { int32_t aus, bytes, sync, failed; };

__global__ void __launch_bounds__(256) k_au_pack(const AuArgs A)
{
    __shared__ int32_t s_total;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int bm = A.run ? A.run[blockIdx.x] : (int)blockIdx.x;              // pair of the class
    const int svc = A.pairs ? A.ens_base[A.pairs[bm].ens] + A.pairs[bm].idx : 0;
    const SfEvent* __restrict__ ev = A.events + (size_t)bm * A.n_cif;
    const uint8_t* __restrict__ sf = A.sf + (size_t)bm * A.n_slots * A.sf_len;
    const uint64_t region = A.region0 + (uint64_t)bm * A.reserve;
    AuRec* __restrict__ rec = A.aus + (size_t)svc * A.au_cap;
    uint2* __restrict__ rsrc = A.au_src + (size_t)svc * A.au_cap;

    if (wave == 0) {
        int ne = A.n_events[bm]; ne = ne < A.n_cif ? ne : A.n_cif;
        AuScan carry{0, 0, 0, 0};
        bool stopped = false;                                                    // an access unit did not fit: nothing behind it is stored
        for (int e0 = 0; e0 < ne; e0 += 64) {
            const int e = e0 + lane;
            AuScan mine{0, 0, 0, 0};
            SfEvent me{};
            if (e < ne) me = ev[e];
            const bool on = me.sync && me.sf_slot >= 0 && me.sf_slot < A.n_slots;
            const int n_au = on ? (me.num_aus < 6 ? me.num_aus : 6) : 0;
            if (on) mine.sync = 1;
#pragma unroll
            for (int i = 0; i < 6; i++) {                                        // (unrolled: the event stays in registers)
                const int len = me.au_start[i + 1] - me.au_start[i] - 2;
                if (i >= n_au) continue;
                if (au_stored_ok(me, i, len, A.sf_len)) { mine.aus++; mine.bytes += au_stored_len(len, me.format, A.format); }
                else mine.failed++;                                             // (the reference `continue`s: neither decoded nor forwarded)
            }
            AuScan inc = mine;
            for (int d = 1; d < 64; d <<= 1) {
                const int a = __shfl_up(inc.aus, d), b = __shfl_up(inc.bytes, d), c = __shfl_up(inc.sync, d), f = __shfl_up(inc.failed, d);
                if (lane >= d) { inc.aus += a; inc.bytes += b; inc.sync += c; inc.failed += f; }
            }
            int idx = carry.aus + inc.aus - mine.aus, off = carry.bytes + inc.bytes - mine.bytes;
            // What does not fit the record table or the pair's reservation is left out, and so is everything behind it: the extent stays
            // one piece and `bytes` is what was stored.  (Through the stream the reservation is a true bound; the unit entry's caller sets it.)
            const bool over = idx + mine.aus > A.au_cap || (uint64_t)off + (uint64_t)mine.bytes > A.reserve;
            const unsigned long long m = __ballot(over);
            const int first = m ? __popcll(~m & (m - 1)) : 64;                   // first lane whose access units do not all fit
            int kept_aus = 0, kept_bytes = 0; bool full = false;                 // (`stopped` is uniform over the wave, `full` is the lane's own)
#pragma unroll
            for (int i = 0; i < 6; i++) {                                        // (unrolled: the event stays in registers)
                const int len = me.au_start[i + 1] - me.au_start[i] - 2;
                if (stopped || full || lane > first || i >= n_au || !au_stored_ok(me, i, len, A.sf_len)) continue;
                const int stored = au_stored_len(len, me.format, A.format);
                if (idx >= A.au_cap || (uint64_t)off + stored > A.reserve) { full = true; continue; }
                AuRec r; r.cif = me.cif; r.au_index = (uint8_t)i; r.format = (uint8_t)me.format; r.pad_[0] = r.pad_[1] = 0;
                r.length = (uint32_t)stored; r.pad2_ = 0; r.offset = region + (uint64_t)off;
                rec[idx] = r;
                rsrc[idx] = make_uint2((uint32_t)(me.sf_slot * A.sf_len + me.au_start[i]), (uint32_t)len);
                idx++; off += stored; kept_aus++; kept_bytes += stored;
            }
            if (!stopped && m) {
                carry.aus += __shfl(inc.aus - mine.aus + kept_aus, first); carry.bytes += __shfl(inc.bytes - mine.bytes + kept_bytes, first);
            } else if (!stopped) { carry.aus += __shfl(inc.aus, 63); carry.bytes += __shfl(inc.bytes, 63); }
            stopped = stopped || m != 0;
            carry.sync += __shfl(inc.sync, 63); carry.failed += __shfl(inc.failed, 63);
        }
        if (lane == 0) {
            AuSvc s; s.n_superframes = carry.sync; s.n_aus = carry.aus; s.n_failed = carry.failed; s.bytes = (uint32_t)carry.bytes;
            A.svc[svc] = s;
            s_total = s.n_aus;
        }
    }
    __syncthreads();
    const int total = s_total;
    for (int a = wave; a < total; a += 4) {
        const uint2 from = rsrc[a];                                          // (offset in the pair's superframes, payload length)
        const AuRec r = rec[a];
        const int len = (int)from.y, fmt = r.format, flen = (int)r.length;
        const uint8_t* __restrict__ src = sf + from.x;
        uint8_t* __restrict__ dst = A.stage + r.offset;
        // the frame: bytes [0, pb] come from the header and the length bytes, byte pb + k (1 <= k < len) from payload bytes k - 1 and k,
        // byte pb + len from the last payload byte alone.  RAW: no header, shift 0
        const bool loas = A.format == AU_FORMAT_LOAS;
        const int H = loas ? au_header_bits(fmt) : 0, P = loas ? H + 8 * (len / 255 + 1) : 0, pb = P >> 3, s = P & 7;
        uint64_t hi = 0; uint32_t lo = 0;
        if (loas) au_header(fmt, flen, hi, lo);
        const int lo_j = loas ? pb + 1 : 0, hi_j = pb + len;                    // whole-dword candidates: frame bytes [lo_j, hi_j)
        int jf0 = lo_j + (int)((0 - (uintptr_t)(dst + lo_j)) & 3);
        int ndw = hi_j - jf0 >= 4 ? (hi_j - jf0) >> 2 : 0;
        if (ndw == 0) jf0 = flen;
        const int jf1 = jf0 + 4 * ndw;
        for (int q = lane; q < ndw; q += 64) {
            const int j = jf0 + 4 * q;
            const uint64_t bit = (uint64_t)(uintptr_t)src * 8 + (uint64_t)(8 * (j - pb) - s);
            const uint32_t* w = reinterpret_cast<const uint32_t*>((uintptr_t)(bit >> 5) * 4);
            const uint64_t v = (uint64_t)__builtin_bswap32(w[0]) << 32 | __builtin_bswap32(w[1]);
            *reinterpret_cast<uint32_t*>(dst + j) = __builtin_bswap32((uint32_t)((v << (bit & 31)) >> 32));
        }
        const int n_slow = jf0 + (flen - jf1);
        for (int q = lane; q < n_slow; q += 64) {
            const int j = q < jf0 ? q : jf1 + (q - jf0);
            uint32_t b;
            if (!loas) b = src[j];
            else {
                const int h8 = H >> 3, sh = H & 7;
                if (j < h8) b = au_header_byte(hi, lo, j);
                else {
                    const int m = j - h8;
                    const uint32_t prev = m == 0 ? au_header_byte(hi, lo, h8) : (au_tail_byte(src, len, m - 1) << (8 - sh)) & 0xFFu;
                    b = prev | (au_tail_byte(src, len, m) >> sh);
                }
            }
            dst[j] = (uint8_t)b;
        }
    }
}

void launch_au_pack(const AuArgs& a, int n_blocks, hipStream_t s)
{
    if (n_blocks <= 0) return;
    hipLaunchKernelGGL(k_au_pack, dim3(n_blocks), dim3(256), 0, s, a);
}

} // namespace dabphy
