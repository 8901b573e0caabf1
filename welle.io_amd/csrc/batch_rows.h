// welle.io_amd/csrc/batch_rows.h -- two facts about what a batch holds for one (ensemble, sub-channel) pair, each stated once for the
// kernels and the host: which rows of the class output the service decoded (k_superframe.hip: sf_plan, k_mp2.hip, k_chanber.hip;
// dabphy_getters.hip: msc_rows_info) and how the superframe filter's window lies in the state it carries from batch to batch
// (k_superframe.hip; reserved by dabphy_internal.h: MscClass::sf_stride).  Pure integer arithmetic on top of dabphy_common.h:
// tests/native/batch_rows_check.cpp compiles it for the host.
#pragma once
#include "dabphy_common.h"

namespace dabphy {

// ---- The rows a pair decoded: rows [batch_first_row, n_rows) of its class output, n_rows = 4 * (valid frames of the batch).  DabAudio
// emits its first logical frame on the 17th CIF its time de-interleaver is fed (dab-audio.cpp:146-149), counted from the CIF at which
// the sub-channel was selected (MscPair::cif0); row r of a batch is CIF 4 * frame_no + r, frame_no the batch's first frame's.
// Not clamped: a batch that lies wholly inside the fill gets a first row beyond n_rows, and dabphy_get_msc* report it so;
constexpr int TDI_FILL_CIFS = 16;
__host__ __device__ constexpr int64_t batch_first_row(int64_t frame_no, int64_t cif0)
{
    const int64_t fed = 4 * frame_no - cif0;                       // CIFs fed in front of row 0
    return fed >= TDI_FILL_CIFS ? 0 : TDI_FILL_CIFS - fed;
}
// ... clamped to the batch's rows, as the kernels take it
__host__ __device__ constexpr int batch_first_row(int64_t frame_no, int64_t cif0, int n_rows) { const int64_t r = batch_first_row(frame_no, cif0); return r < n_rows ? (int)r : n_rows; }
static_assert(batch_first_row(0, 0) == 16 && batch_first_row(3, 0) == 4 && batch_first_row(4, 0) == 0 && batch_first_row(2, 12) == 20, "16 CIFs from cif0");

// ---- The filter's carried window of a pair: an int32 count of frames at byte 0, the frames (oldest first, at most 5) from byte
// SF_STATE_HEAD on, records a multiple of 16 bytes apart.
constexpr size_t SF_STATE_HEAD = 16;
__host__ __device__ constexpr size_t sf_state_stride(size_t frame_bytes) { return (SF_STATE_HEAD + 5 * frame_bytes + 15) & ~(size_t)15; }
__host__ __device__ inline int32_t& sf_state_count(uint8_t* st) { return *reinterpret_cast<int32_t*>(st); }
__host__ __device__ inline uint8_t* sf_state_frames(uint8_t* st) { return st + SF_STATE_HEAD; }

} // namespace dabphy
