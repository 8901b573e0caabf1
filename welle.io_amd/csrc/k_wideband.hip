// welle.io_amd/csrc/k_wideband.hip -- wideband front end: one capture at D x 2.048 MS/s -> the sample ring rows of the handle's ensembles.
//
// The reference has no channeliser (its one rate conversion is the Airspy's pair average, input/airspy_sdr.cpp:187-202); this is the
// polyphase decimator a multi-block SDR capture needs in front of k_ingest's ring.  WidebandArgs (dabphy_kernels.h) states the sum;
// the capture is read through capture_sample (there too), the carry behind a call is k_capture_carry's (k_ingest.hip).
//
// Form: filter with per-ensemble complex taps, rotate each output once.  A work-group converts one tile of the capture into LDS once
// (T D + halo samples, read from HBM once) and serves every ensemble from it: WB_ENS_STEP ensembles at a time, WB_OUT_STEP outputs
// per lane (a tile of fewer than 512 outputs: the 512 / T groups of waves share the ensembles).  Per tap that is one LDS read per
// output and one wave-uniform 32-byte load of the four taps, for 4 WB_ENS_STEP WB_OUT_STEP FMAs.  Mixing first would need 36 D
// instead of 64 D FMAs per output, but with one output per lane it reads LDS once per TWO FMAs and sits on the LDS rate, not on the
// vector rate.  (What a register-blocked mix-then-filter would gain is left on the table: DESIGN.md section 4.0.)
//
// Tile layout: by polyphase branch.  Entry l of the tile (l = 0 is `halo` samples in front of the tile's first new sample; halo is a
// multiple of D that covers wideband_reach(n_taps) - 1 samples, so l mod D is the capture index mod D) lies in row l mod D, column
// l div D, rows W apart (W odd).  Tap k = j D + r of output t reads row D - 1 - r, column halo / D + t - j: lanes with consecutive
// outputs read consecutive 8-byte cells.
//
// Order of summation: every output adds its taps k = 0, 1, ... n_taps - 1 (and then the table's zero rows up to a multiple of
// WB_TAP_STEP) with fmaf into one accumulator per component, samples in front of the stream being zeros from the (cleared) carry --
// nothing depends on the tile, the call or the lane, so a capture written in any pieces gives the same bits.  fmaf rounds once on the
// device and in the CPU execution model alike.
#include "dabphy_kernels.h"
#include <dabphy_wave_ops.h>

namespace dabphy {

template <int SMAX>
__global__ void __launch_bounds__(256) k_wideband(WidebandArgs A)
{
    __shared__ cf32 tile[SMAX];
    // T outputs per tile, WB_OUT_STEP per lane (lane t: outputs t, t + T / 2): the 256 threads are 512 / T groups of T / 2 lanes (whole
    // waves: T >= 128) that share the tile and take turns at the ensembles
    const uint32_t T = A.T, D = A.D, W = A.W, lanes = T / WB_OUT_STEP, t = threadIdx.x % lanes;
    const uint32_t grp = (uint32_t)uniform_i32((int)(threadIdx.x / lanes)), n_grp = 256 / lanes;
    const uint64_t m0 = (uint64_t)blockIdx.x * T;                       // the tile's first output
    const int64_t c0 = (int64_t)(m0 * D) - (int64_t)A.halo;             // capture index (in this call) of tile entry 0

    // ---- the tile, converted once (capture_sample: the call's samples, the carry in front of them, zeros behind them in the last tile)
    {
        const uint32_t L = A.halo + T * D, step_row = 256 % D, step_col = 256 / D;
        uint32_t row = threadIdx.x % D, col = threadIdx.x / D;
        for (uint32_t l = threadIdx.x; l < L; l += 256) {
            tile[row * W + col] = capture_sample(A.src, c0 + (int64_t)l);
            row += step_row; col += step_col;
            if (row >= D) { row -= D; col++; }
        }
    }
    __syncthreads();

    const auto ctaps = as_constant(reinterpret_cast<const float*>(A.ctaps));      // wave-uniform reads of a table nobody writes: scalar loads
    const cf32* x_first = tile + (size_t)(D - 1) * W + A.halo / D + t;      // tap 0 of the lane's first output: its newest sample

    for (uint32_t e0 = grp * WB_ENS_STEP; e0 < A.e_pad; e0 += n_grp * WB_ENS_STEP) {
        float ar[WB_OUT_STEP][WB_ENS_STEP], ai[WB_OUT_STEP][WB_ENS_STEP];
#pragma unroll
        for (int o = 0; o < WB_OUT_STEP; o++)
#pragma unroll
            for (int q = 0; q < WB_ENS_STEP; q++) { ar[o][q] = 0.0f; ai[o][q] = 0.0f; }
        const cf32* xp = x_first;
        auto g = ctaps + 2 * e0;                                          // (re, im) of WB_ENS_STEP ensembles' tap k, e_pad pairs per k
        uint32_t r = 0;                                                 // branch of tap k: k mod D
        // Taps go WB_TAP_STEP at a time, and the next step's operands -- samples from LDS, taps by wave-uniform loads that miss the
        // scalar cache once the table outgrows it -- are fetched while this step is added.  The table ends in rows of zeros up to
        // wideband_reach(n_taps) and the halo covers as many samples: what the last steps fetch beyond n_taps exists, and a zero tap
        // adds nothing to the sum.
        cf32 x[WB_TAP_STEP][WB_OUT_STEP]; float gk[WB_TAP_STEP][2 * WB_ENS_STEP];
        const auto fetch = [&](cf32 (&xo)[WB_TAP_STEP][WB_OUT_STEP], float (&go)[WB_TAP_STEP][2 * WB_ENS_STEP]) {
#pragma unroll
            for (int u = 0; u < WB_TAP_STEP; u++) {
#pragma unroll
                for (int o = 0; o < WB_OUT_STEP; o++) xo[u][o] = xp[o * lanes];
#pragma unroll
                for (int q = 0; q < 2 * WB_ENS_STEP; q++) go[u][q] = g[q];
                g += 2 * A.e_pad;
                if (++r == D) { r = 0; xp += (size_t)(D - 1) * W; xp -= 1; } else xp -= W;      // one branch up, or back to the last branch one column earlier
            }
        };
        fetch(x, gk);
        for (uint32_t k = 0; k < A.n_taps; k += WB_TAP_STEP) {
            cf32 xn[WB_TAP_STEP][WB_OUT_STEP]; float gn[WB_TAP_STEP][2 * WB_ENS_STEP];
            fetch(xn, gn);
#pragma unroll
            for (int u = 0; u < WB_TAP_STEP; u++) {
#pragma unroll
                for (int o = 0; o < WB_OUT_STEP; o++) {
#pragma unroll
                    for (int q = 0; q < WB_ENS_STEP; q++) {
                        const float g_re = gk[u][2 * q], g_im = gk[u][2 * q + 1];
                        ar[o][q] = fmaf(g_re, x[u][o].re, ar[o][q]); ar[o][q] = fmaf(-g_im, x[u][o].im, ar[o][q]);
                        ai[o][q] = fmaf(g_re, x[u][o].im, ai[o][q]); ai[o][q] = fmaf(g_im, x[u][o].re, ai[o][q]);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < WB_TAP_STEP; u++) {
#pragma unroll
                for (int o = 0; o < WB_OUT_STEP; o++) x[u][o] = xn[u][o];
#pragma unroll
                for (int q = 0; q < 2 * WB_ENS_STEP; q++) gk[u][q] = gn[u][q];
            }
        }
#pragma unroll
        for (int o = 0; o < WB_OUT_STEP; o++) {
            const uint64_t m = m0 + t + o * lanes;
            if (m >= A.n_out) continue;                                 // (the last tile)
            uint64_t p = A.dst.w + m; if (p >= A.dst.ring) p -= A.dst.ring;
            // the oscillator's phase at the output's newest sample a = m D + D - 1: table index (om_e * (a mod P)) mod P, both factors below 4096
            const uint32_t a_mod = (uint32_t)(((uint64_t)A.abs_mod + (m * D + D - 1) % A.P) % A.P);
#pragma unroll
            for (int q = 0; q < WB_ENS_STEP; q++) {
                const uint32_t e = e0 + q;
                if (e < A.n_ens) {
                    cf32 acc; acc.re = ar[o][q]; acc.im = ai[o][q];
                    A.dst.iq[(size_t)e * A.dst.iq_stride + p] = cmul(acc, A.osc[(A.om[e] * a_mod) % A.P]);
                }
            }
        }
    }
}

bool wideband_geometry(WidebandArgs& a)
{
    a.halo = (wideband_reach(a.n_taps) - 1 + a.D - 1) / a.D * a.D;
    for (uint32_t T = 512; T >= 128; T /= 2) {
        const uint32_t W = (a.halo / a.D + T) | 1u;
        if ((size_t)a.D * W <= (size_t)WB_TILE_LARGE) { a.T = T; a.W = W; return true; }
    }
    return false;
}

void launch_wideband(const WidebandArgs& a, hipStream_t s)
{
    const unsigned tiles = (unsigned)((a.n_out + a.T - 1) / a.T);
    if ((size_t)a.D * a.W <= (size_t)WB_TILE_SMALL) hipLaunchKernelGGL(k_wideband<WB_TILE_SMALL>, dim3(tiles), dim3(256), 0, s, a);
    else if ((size_t)a.D * a.W <= (size_t)WB_TILE_MID) hipLaunchKernelGGL(k_wideband<WB_TILE_MID>, dim3(tiles), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_wideband<WB_TILE_LARGE>, dim3(tiles), dim3(256), 0, s, a);
    launch_capture_carry(a.src, a.carry_out, s);
}

} // namespace dabphy
