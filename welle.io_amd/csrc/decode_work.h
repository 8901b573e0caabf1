// welle.io_amd/csrc/decode_work.h -- two facts the decoders' kernels and their host side share, each stated once: the work-item word of
// a work list (FusedArgs::work: k_viterbi.hip, k_viterbi_sp.hip, k_viterbi_sp2.hip, k_chanber.hip; packed in dabphy_fused.hip and
// dabphy_chanber.hip) and the geometry of the state-parallel kernels' decision history (what a kernel stores and what the host reserves:
// a formula of one that the other does not follow is an out-of-bounds decision store).  Pure integer arithmetic on top of
// dabphy_common.h: tests/native/decode_work_check.cpp compiles it for the host.
#pragma once
#include "dabphy_common.h"
#include <stddef.h>

namespace dabphy {

// ---- The work item: class << 24 | group of 64 code words of that class.
constexpr int WORK_CLASS_SHIFT = 24;
constexpr uint32_t WORK_MAX_CLASSES = 255;                         // classes of one launch (a handle has at most 255, the FIC included)
constexpr uint32_t WORK_MAX_GROUPS = (1u << WORK_CLASS_SHIFT) - 1; // groups of one class
__host__ __device__ constexpr uint32_t work_item(uint32_t cls, uint32_t group) { return (cls << WORK_CLASS_SHIFT) | group; }
__host__ __device__ constexpr uint32_t work_class(uint32_t wk) { return wk >> WORK_CLASS_SHIFT; }
__host__ __device__ constexpr uint32_t work_group(uint32_t wk) { return wk & WORK_MAX_GROUPS; }
static_assert(work_class(work_item(WORK_MAX_CLASSES, WORK_MAX_GROUPS)) == WORK_MAX_CLASSES && work_group(work_item(WORK_MAX_CLASSES, WORK_MAX_GROUPS)) == WORK_MAX_GROUPS &&
              work_item(1, 2) == 0x01000002u, "class << 24 | group");

// ---- The decision history of the state-parallel kernels: every lane keeps the decisions of its state, HIST_STEPS trellis steps to a
// word, and a code word's 64 words leave as one 256-byte row = HIST_ROW_CELLS cells (uint2) of the decision scratch.  (30, not 32: a
// multiple of the six-step code word granule and of both kernels' layout periods.)  A code word of nsteps steps has hist_rows(nsteps)
// rows -- the whole blocks and the last, partial one --, a work-group the rows of its one code word (k_viterbi_sp) or two (k_viterbi_sp2).
constexpr int HIST_STEPS = 30;
constexpr size_t HIST_ROW_CELLS = 32;
__host__ __device__ constexpr size_t hist_rows(size_t nsteps) { return nsteps / HIST_STEPS + 1; }
__host__ __device__ constexpr size_t hist_cells(size_t nsteps, bool two) { return hist_rows(nsteps) * HIST_ROW_CELLS * (two ? 2 : 1); }
static_assert(hist_rows(774) == 26 && hist_cells(774, false) == 26 * 32 && hist_cells(9222, true) == 308 * 64, "history rows of the FIC and of 384 kbit/s");

} // namespace dabphy
