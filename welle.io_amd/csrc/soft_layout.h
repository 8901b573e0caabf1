// welle.io_amd/csrc/soft_layout.h -- where a code word's soft bits lie in the soft-bit ring: the one definition every gather takes
// (k_viterbi.hip, k_viterbi_sp.hip and k_viterbi_sp2.hip through viterbi_gather.h, the step tables of dabphy_fused.hip).
//
// The ring.  [ensemble][soft_ring frame slots (+ one frame of zeros in the streaming receiver)][75 symbols][SOFT_PER_SYM] int8: frame
// frame_no lies in slot frame_no % soft_ring; symbols 1..3 (rows 0..2) are the FIC, CIF q of the frame is rows 3 + 18 q .. 3 + 18 q + 17.
//
// Code word orders.
//   MSC class   cw = pair * R + r: (ensemble, sub-channel) pair of the class's table -- every ensemble selects its own sub-channels,
//               msc-handler.cpp:61-103 --, CIF r of this batch, R = 4 * n_frames.  Soft bit u of the logical frame emitted at CIF c comes
//               from CIF c - 16 + tdi_row(u & 15) (dab-audio.cpp:113,138-143: tempX[i] = hist[(idx + map[i & 15]) & 15][i], read BEFORE
//               the current CIF is stored): the time de-interleaver is an address computation on the ring, never a copy.
//   FIC         cw = (b F + f) 4 + q: quarter q of symbols 1..3 of frame slot f of ensemble b (F = n_frames), 2304 soft bits;
//               under frame_sel = f + 1, cw = 4 b + q of frame f alone (the replay of exact batch mode decodes one frame at a time).
#pragma once
#include "dabphy_common.h"

namespace dabphy { namespace layout {

// row of the time de-interleaver for column i & 15: map16[i] of dab-audio.cpp:113, a 4-bit reversal
__host__ __device__ constexpr int tdi_row(int i) { return ((i & 1) << 3) | ((i & 2) << 1) | ((i & 4) >> 1) | ((i & 8) >> 3); }
static_assert(tdi_row(0) == 0 && tdi_row(1) == 8 && tdi_row(2) == 4 && tdi_row(3) == 12 && tdi_row(4) == 2 && tdi_row(5) == 10 &&
              tdi_row(6) == 6 && tdi_row(7) == 14 && tdi_row(8) == 1 && tdi_row(9) == 9 && tdi_row(10) == 5 && tdi_row(11) == 13 &&
              tdi_row(12) == 3 && tdi_row(13) == 11 && tdi_row(14) == 7 && tdi_row(15) == 15, "map16 of dab-audio.cpp:113");

// byte offset of CIF c_src's row inside an ensemble's ring slice (c_src = 4 * frame_no + q, counted from the start of the stream);
// defined for c_src >= 0 only: a CIF from before the stream has no row, every caller tests that first
__host__ __device__ constexpr size_t cif_row_bytes(long long c_src, int soft_ring)
{
    return ((size_t)((c_src >> 2) % soft_ring) * 75 + 3 + 18 * (int)(c_src & 3)) * SOFT_PER_SYM;
}
static_assert(cif_row_bytes(0, 9) == 3 * SOFT_PER_SYM && cif_row_bytes(5, 9) == (75 + 3 + 18) * SOFT_PER_SYM &&
              cif_row_bytes(4 * 9 + 3, 9) == (3 + 18 * 3) * SOFT_PER_SYM && cif_row_bytes(4 * 8, 9) == (8 * 75 + 3) * SOFT_PER_SYM, "CIF rows of the ring");

// FIC code word -> index b * n_frames + f of its frame descriptor
__host__ __device__ constexpr int fic_frame_of(int cw, int n_frames, int frame_sel)
{
    return frame_sel ? (cw >> 2) * n_frames + (frame_sel - 1) : cw >> 2;
}
static_assert(fic_frame_of(4 * 7 + 2, 3, 0) == 7 && fic_frame_of(4 * 2 + 1, 3, 2) == 2 * 3 + 1, "FIC code word order");
// ... and the byte offset of its 2304 soft bits inside the ensemble's slice (frame_stride: bytes between frame slots)
__host__ __device__ constexpr size_t fic_cw_bytes(int64_t frame_no, int soft_ring, size_t frame_stride, int cw)
{
    return (size_t)(frame_no % soft_ring) * frame_stride + (size_t)2304 * (cw & 3);
}
static_assert(fic_cw_bytes(11, 9, SOFT_PER_FRAME, 4 * 5 + 3) == (size_t)2 * SOFT_PER_FRAME + 3 * 2304, "FIC quarters");

} } // namespace dabphy::layout
