// welle.io_amd/csrc/viterbi_gather.h -- the gather of the state-parallel decoders (k_viterbi_sp.hip, k_viterbi_sp2.hip): the soft bits
// of ONE code word straight from the soft-bit ring (soft_layout.h) or a seam's plain array, depunctured by the class's map.
#pragma once
#include "dabphy_kernels.h"
#include <dabphy_wave_ops.h>
#include "soft_layout.h"

namespace dabphy {

// Where code word cw of class C lies: its base pointer, and -- filled by the caller's lanes j < 16 -- 16 row offsets, one per column
// u & 15 of the time de-interleaver; -1 = no such CIF / frame not valid.  Kinds 0, 1, 2 of FusedClass.
__device__ __forceinline__ const int8_t* locate(const FusedArgs& A, const DABPHY_CONST_AS FusedClass& C, int cw, int j, long long* rowoff)
{
    const int F = A.n_frames;
    const int8_t* base;
    if (C.kind == 0) {
        const int R = 4 * F, pair = cw / R, r = cw - pair * R;
        const MscPair pp = C.pairs[pair];                                   // every ensemble selects its own sub-channels (msc-handler.cpp:61-103)
        const int b = pp.ens;
        base = A.soft + (size_t)b * A.ens_stride + (size_t)pp.start_bit;
        if (j < 16) {
            const long long c_src = 4 * A.desc[(size_t)b * F].frame_no + r - 16 + layout::tdi_row(j);
            rowoff[j] = c_src >= 0 ? (long long)layout::cif_row_bytes(c_src, A.soft_ring) : -1;
        }
    } else if (C.kind == 1) {
        const int bf = layout::fic_frame_of(cw, F, A.fic_frame_sel), b = bf / F;
        const FrameDesc& d = A.desc[bf];
        const size_t fstride = A.fic_frame_stride ? A.fic_frame_stride : (size_t)SOFT_PER_FRAME;
        base = A.soft + (size_t)b * A.ens_stride + layout::fic_cw_bytes(d.frame_no, A.soft_ring, fstride, cw);
        if (j < 16) rowoff[j] = d.valid == 1 ? 0 : -1;
    } else {
        base = A.lin_in + (size_t)cw * A.lin_stride;                        // a code word of the linear seams: no de-interleaver
        if (j < 16) rowoff[j] = 0;
    }
    return base;
}

// The four soft values of trellis step s: four map entries (no map: the input is already depunctured), the indexed byte reads,
// erasures as 0; -128 maps to symbol 0 like -127 (viterbi.cpp:233-236): the demapper never produces it, a seam's caller may
__device__ __forceinline__ void fetch_step(const map_t* __restrict__ map, int s, const int8_t* base, const long long* rowoff, int (&v)[4])
{
    uint2 mm = make_uint2(0, 0);
    if (map) mm = *reinterpret_cast<const uint2*>(map + 4 * s);
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int u = map ? map_index(((q < 2 ? mm.x : mm.y) >> (16 * (q & 1))) & 0xffffu) : 4 * s + q;
        long long off = -1;
        if (u >= 0) off = rowoff[u & 15];
        v[q] = off >= 0 ? (int)base[off + u] : 0;
        if (v[q] < -127) v[q] = -127;
    }
}

} // namespace dabphy
