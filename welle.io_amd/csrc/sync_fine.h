// welle.io_amd/csrc/sync_fine.h -- the fine frequency corrector's step (ofdm-processor.cpp:450-451) and the interval test that
// decides it without the reference's 37 800 ordered float additions (k_sync.hip: sync_finish_body's fast path).
// Pure arithmetic on top of dabphy_common.h: tests/native/fine_check.cpp compiles it for the host.
#pragma once
#include "dabphy_common.h"
#include <cmath>

namespace dabphy {

// ofdm-processor.cpp:450-451: fineCorrector (int16) += 0.1 * arg(FreqCorr) / M_PI * (carrierDiff / 2)
__host__ __device__ __forceinline__ int32_t fine_from_arg(int32_t fine_old, float a)
{
    return (int32_t)(int16_t)((double)fine_old + 0.1 * (double)a / M_PI * (1000 / 2));
}

// next float towards +inf (up) or -inf
__host__ __device__ __forceinline__ float f32_step(float x, bool up)
{
    union { float f; uint32_t u; } v; v.f = x;
    if ((v.u & 0x7fffffffu) == 0) { v.u = up ? 1u : 0x80000001u; return v.f; }
    const bool neg = (v.u >> 31) != 0;
    v.u += (neg != up) ? 1u : 0xffffffffu;                  // away from zero when the step and the sign agree
    return v.f;
}
__host__ __device__ __forceinline__ float f32_down(double x) { float f = (float)x; if ((double)f > x) f = f32_step(f, false); return f; }
__host__ __device__ __forceinline__ float f32_up(double x) { float f = (float)x; if ((double)f < x) f = f32_step(f, true); return f; }

// The only thing the reference takes from FreqCorr is the int16 it adds to the fine corrector.  The float sums it accumulates in
// index order differ from the exact sums by at most E = u Q / (1 - (n + 1) u), Q >= sum over all prefixes |S_k|, u = 2^-24 (each
// addition errs by at most u times its own result; Higham, "Accuracy and Stability of Numerical Algorithms", section 4.2, with the
// computed prefixes bounded by the exact ones plus E).  Q comes from block sums: a prefix that ends inside block b is at most
// |sum of the blocks before b| + sum of the magnitudes inside b.  atan2 is monotone along the edges of a box that avoids the
// origin and the branch cut, atan2f is within 2 ulp of it, and the corrector expression is monotone in the angle.  So evaluating
// it at the ends of the interval decides the int16 whenever both ends agree -- all but about one frame in 5000 -- and otherwise the
// caller falls back to the ordered float sums.  blk[b][0..3] = sum re, sum im, sum |re|, sum |im| of block b (double precision, any
// order); block b holds m = 504 x its rows products (8 rows, the last block 3).  Returns true when decided.
constexpr int FIN_BLOCK_ROWS = 8, FIN_BLOCKS = (75 + FIN_BLOCK_ROWS - 1) / FIN_BLOCK_ROWS;
__host__ __device__ __forceinline__ bool fine_decided(int32_t fine_old, const double (*blk)[4], int32_t& fine_new)
{
    constexpr double n = 75.0 * 504.0, u = 0x1p-24;
    double sre = 0.0, sim = 0.0, are = 0.0, aim = 0.0, qre = 0.0, qim = 0.0;
    for (int b = 0; b < FIN_BLOCKS; b++) {
        const double m = 504.0 * ((b + 1) * FIN_BLOCK_ROWS <= 75 ? FIN_BLOCK_ROWS : 75 - b * FIN_BLOCK_ROWS);
        qre += m * (fabs(sre) + blk[b][2]); qim += m * (fabs(sim) + blk[b][3]);
        sre += blk[b][0]; sim += blk[b][1]; are += blk[b][2]; aim += blk[b][3];
    }
    constexpr double k = u / (1.0 - (n + 1.0) * u) * (1.0 + 0x1p-30);
    constexpr double dsum = n * 0x1p-51;                              // this path's own (double precision) summation errors, generously
    const double ere = k * qre * (1.0 + dsum) + dsum * are + 1e-30, eim = k * qim * (1.0 + dsum) + dsum * aim + 1e-30;
    const double r_lo = sre - ere, r_hi = sre + ere, i_lo = sim - eim, i_hi = sim + eim;
    if (!(r_lo > -1e30) || !(r_hi < 1e30) || !(i_lo > -1e30) || !(i_hi < 1e30)) return false;    // (also NaN)
    const float xl = f32_down(r_lo), xh = f32_up(r_hi), yl = f32_down(i_lo), yh = f32_up(i_hi);
    // the box must avoid the origin and the branch cut: then atan2 is monotone along every edge and its extremes sit in the corners
    if (!(xl > 0.0f || yl > 0.0f || yh < 0.0f)) return false;
    const float c0 = fdlibm_atan2f(yl, xl), c1 = fdlibm_atan2f(yl, xh), c2 = fdlibm_atan2f(yh, xl), c3 = fdlibm_atan2f(yh, xh);
    float a_lo = fminf(fminf(c0, c1), fminf(c2, c3)), a_hi = fmaxf(fmaxf(c0, c1), fmaxf(c2, c3));
#pragma unroll
    for (int i = 0; i < 8; i++) { a_lo = f32_step(a_lo, false); a_hi = f32_step(a_hi, true); }    // atan2f's own error (< 2 ulp) at the corners and at the true point, with room for a binade change
    const int32_t n_lo = fine_from_arg(fine_old, a_lo), n_hi = fine_from_arg(fine_old, a_hi);
    fine_new = n_lo;
    return n_lo == n_hi;
}

} // namespace dabphy
