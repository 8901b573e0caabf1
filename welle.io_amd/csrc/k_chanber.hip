// welle.io_amd/csrc/k_chanber.hip -- channel BER in front of the Viterbi decoder (pseudo-BER): the decoded bits of a code word encoded
// again with the mother code and compared with the signs of the soft bits the decoder read (include/dabphy.h has the definition).
//
// No counterpart in the reference: what a professional monitor shows per sub-channel, computed from what the decoders leave behind.
//
// k_chanber: one wavefront per code word, lanes take the trellis steps lane, lane + 64, ...  The mother code is feed-forward -- the
// four coded bits of step s are parities of the decoded bits s - 6 .. s (the encoder whose branch table viterbi_acs.h restates from
// viterbi.cpp:36) --, so no step waits for another.  A step reads the two decoded bytes that hold its seven bits (and the PRBS bytes
// where the traceback's store removed the energy dispersal), its four map entries as one 8-byte load and the four soft bits where the
// decoder's own gather finds them: locate() and fetch_step() of viterbi_gather.h, the one statement of the ring's layout.  fetch_step
// returns 0 for an erasure, for a row that does not exist and for a soft bit of 0 alike -- none of them is counted -- and -127 for
// -128.  The two counters of a lane share a register (errors | compared << 16: at most 4 * 9222 each), six exchanges fold the wave,
// lane 0 stores the pair: no atomics, no second pass, no LDS beyond locate()'s sixteen row offsets.
//
// An MSC code word is counted when its row is one the batch decoded (the rule of dabphy_get_msc_ensemble and of the superframe
// filter, batch_rows.h: rows [first_valid, n_rows) counted from MscPair::cif0); the others store {0, 0}.
//
// k_chanber_totals: the batch's per-code-word counts -> per-service totals [ensemble][1 + list positions], one wavefront each.
#include "dabphy_kernels.h"
#include <dabphy_wave_ops.h>
#include "viterbi_gather.h"

namespace dabphy {

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m);
    return v;
}

__global__ void __launch_bounds__(64) k_chanber(BerArgs B)
{
    __shared__ long long s_rowoff[16];
    const FusedArgs& A = B.f;
    const int lane = threadIdx.x;
    const uint32_t wk = as_constant(A.work)[blockIdx.x >> 6];
    const uint32_t ci = work_class(wk);
    const DABPHY_CONST_AS FusedClass& C = as_constant(A.cls)[ci];
    const int cw = (int)work_group(wk) * 64 + (int)(blockIdx.x & 63u);
    if (cw >= C.n_cw) return;
    const int nsteps = C.nsteps, nbytes = C.nbits / 8;

    bool counted = true;
    if (C.kind == 0) {                                                  // a row the batch decoded?  (batch_rows.h)
        const int F = A.n_frames, R = 4 * F, pair = cw / R, r = cw - pair * R;
        const MscPair pp = C.pairs[pair];
        int nv = 0;
        for (int f = 0; f < F; f++) nv += A.desc[(size_t)pp.ens * F + f].valid == 1 ? 1 : 0;
        counted = r < 4 * nv && r >= batch_first_row(A.desc[(size_t)pp.ens * F].frame_no, pp.cif0) && pp.cif0 >= 0;
    }
    const int8_t* const base = locate(A, C, cw, lane, s_rowoff);
    __syncthreads();

    uint32_t acc = 0;                                                   // errors | compared << 16
    if (counted) {
        const map_t* __restrict__ map = C.map;
        const uint8_t* __restrict__ dec = C.out + (size_t)cw * nbytes;
        const uint8_t* __restrict__ prbs = reinterpret_cast<const uint8_t*>(A.prbs_words);   // byte k = PRBS bits 8k .. 8k + 7, MSB first, like the output
        const bool disperse = C.dedisperse != 0;
        for (int s = lane; s < nsteps; s += 64) {
            // bits s - 6 .. s lie in bytes (s >> 3) - 1 and s >> 3; bytes outside the code word are the zeros in front and the tail
            const int k = s >> 3;
            uint32_t hi = 0, lo = 0;
            if (k >= 1 && k - 1 < nbytes) { hi = dec[k - 1]; if (disperse) hi ^= prbs[k - 1]; }
            if (k < nbytes) { lo = dec[k]; if (disperse) lo ^= prbs[k]; }
            const uint32_t reg = (((hi << 8) | lo) >> (7 - (s & 7))) & 0x7fu;          // newest bit = LSB
            const uint32_t c0 = __popc(reg & 0155u) & 1u, c1 = __popc(reg & 0117u) & 1u, c2 = __popc(reg & 0123u) & 1u;
            const uint32_t coded = c0 | (c1 << 1) | (c2 << 2) | (c0 << 3);
            int v[4];
            fetch_step(map, s, base, s_rowoff, v);
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (v[q] != 0) acc += 0x10000u + (((v[q] > 0 ? 1u : 0u) ^ (coded >> q)) & 1u);
        }
    }
    acc = wave_sum(acc);                                                // (no carry between the halves: at most 4 * 9222 a counter)
    if (lane == 0) B.out[(size_t)as_constant(B.first)[ci] + (size_t)cw] = make_uint2(acc & 0xffffu, acc >> 16);
}

// slot (b, j) of the totals: the n records from `slots[b * row_len + j]` on (0xffffffff: no such list position)
__global__ void __launch_bounds__(64) k_chanber_totals(BerTotalsArgs T)
{
    const int lane = threadIdx.x;
    const uint32_t first = T.slots[blockIdx.x];
    uint32_t e = 0, c = 0;
    if (first != 0xffffffffu)
        for (uint32_t i = lane; i < T.n; i += 64) { const uint2 v = T.counts[(size_t)first + i]; e += v.x; c += v.y; }
    e = wave_sum(e); c = wave_sum(c);
    if (lane == 0) { T.totals[2 * (size_t)blockIdx.x] = e; T.totals[2 * (size_t)blockIdx.x + 1] = c; }
}

void launch_chanber(const BerArgs& a, hipStream_t s)
{
    if (a.f.n_work == 0) return;
    hipLaunchKernelGGL(k_chanber, dim3(a.f.n_work * 64u), dim3(64), 0, s, a);
}

void launch_chanber_totals(const BerTotalsArgs& a, int n_slots, hipStream_t s)
{
    if (n_slots <= 0) return;
    hipLaunchKernelGGL(k_chanber_totals, dim3((unsigned)n_slots), dim3(64), 0, s, a);
}

} // namespace dabphy
