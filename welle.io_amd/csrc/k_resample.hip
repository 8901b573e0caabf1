// welle.io_amd/csrc/k_resample.hip -- wideband front end at a rational rate: one capture at 2.048 MS/s x M / L -> the sample ring rows of the
// handle's ensembles.  ResampleArgs (dabphy_kernels.h) states the sum; k_wideband.hip is the integer case (L = 1) in another form.  Both
// read the capture through capture_sample (dabphy_kernels.h); the carry behind a call is k_capture_carry's (k_ingest.hip).
//
// Form: mix first, then filter with the real taps.  Consecutive outputs have different phases r_m, so a tap is a per-lane value and the
// wave-uniform complex taps of k_wideband do not exist here; mixing first also halves the FMAs per tap (2 instead of 4 per ensemble).
// A work-group owns a tile of T consecutive outputs, one per lane.  Per pass over G ensembles it converts the span of capture samples
// the tile reaches (S = J + the samples T outputs advance over; capture_sample: carry in front of the call, zeros behind it) and writes it MIXED into
// LDS once per ensemble: G planes.  A thread walks its entries T apart and advances the capture index mod P by the constant T mod P
// with add / compare / subtract; the oscillator is the product of two table entries (below).  Each lane then adds its taps
// j = 0, 1, ... with one LDS read per ensemble and one tap load that serves all G (RS_TAP_STEP taps at a time, the next step's in
// flight): 2 G FMAs per G + 1 loads.  The prototype lies as the caller gave it, taps[j][r] = h[r + j L]: per tap a wave reads inside ONE
// row of L floats (a cache line at L = 32); a table by phase, every lane in a row of its own, timed within 10 % (profiles/resample.txt).
// The raw capture is read again for every pass (2 - 8 bytes per sample, from L2).
//
// Span layout: entry s lies at (s mod Q) W + s div Q with Q = round(M / L) and W odd: outputs advance by about Q samples, so the lanes
// of a wave read (nearly) consecutive 8-byte cells of one row instead of cells Q apart (Q = 4: a 4-way bank conflict).
//
// Order of summation: every output adds j = 0 ... J - 1 (zero taps from its phase's last real tap on) with fmaf into one accumulator per
// component.  Nothing depends on the tile, the call or the lane: the carry holds J - 1 samples, as many as the padded sum reaches, so a
// capture written in any pieces gives the same bits.  fmaf rounds once on the device and in the CPU execution model alike.
#include "dabphy_kernels.h"
#include <dabphy_wave_ops.h>

namespace dabphy {

template <int G, int SMAX>
__global__ void __launch_bounds__(256) k_resample(ResampleArgs A)
{
    __shared__ cf32 span[SMAX];
    const uint32_t T = A.T, L = A.L, M = A.M, J = A.J, P = A.P, Q = A.Q, W = A.W, plane = Q * W, t = threadIdx.x;
    // the tile's first output t0 (index in the call): its newest sample is a0 + ab in the call, lane t's is a0 + ab + (rb + t M) div L
    const uint64_t t0 = (uint64_t)blockIdx.x * T, q0 = (uint64_t)A.r0 + t0 * M, ab = q0 / L;
    const uint32_t rb = (uint32_t)(q0 % L);
    const int64_t c0 = (int64_t)A.a0 + (int64_t)ab - ((int64_t)J - 1);            // capture index (in this call) of span entry 0
    const uint32_t i0 = (uint32_t)(((int64_t)A.abs_mod + c0 % (int64_t)P + (int64_t)P) % (int64_t)P);   // its absolute index mod P

    const uint32_t qt = rb + t * M, r_t = qt % L, s_top = J - 1 + qt / L;         // the lane's phase; span entry of its tap 0
    const float* h_t = A.taps + r_t;                                              // taps[j][r]: the lanes of a wave read one row of L floats per tap
    const uint32_t row_top = s_top % Q, p_top = row_top * W + s_top / Q;
    const uint64_t m = t0 + t;
    uint64_t ring_pos = A.dst.w + m; if (ring_pos >= A.dst.ring) ring_pos -= A.dst.ring;

    for (uint32_t e0 = 0; e0 < A.n_ens; e0 += G) {
        if (e0) __syncthreads();                                                  // the pass before has read its planes
        // ---- the span, converted once per pass and mixed per ensemble
        {
            // the oscillator at absolute index i, i mod P = hi RS_OSC_LO + lo: osc_hi[e][hi] * osc_lo[e][lo], a function of i alone (the
            // tile and the call do not enter, so neither do they enter the bits).  Lanes with consecutive entries read consecutive
            // osc_lo entries and one or two osc_hi entries: ONE table indexed by (step_e i) mod P has every lane on a cache line of its own
            const cf32* t_hi[G]; const cf32* t_lo[G];
#pragma unroll
            for (int g = 0; g < G; g++) {
                const uint32_t e = e0 + g < A.n_ens ? e0 + g : A.n_ens - 1;      // (a plane nobody stores from)
                t_hi[g] = A.osc_hi + (size_t)e * A.n_hi; t_lo[g] = A.osc_lo + (size_t)e * RS_OSC_LO;
            }
            uint32_t im = (i0 + t % P) % P;                                       // the entry's absolute index mod P
            const uint32_t im_step = T % P;
            const uint32_t step_row = T % Q, step_col = T / Q;
            uint32_t row = t % Q, col = t / Q;
            // RS_MIX_STEP entries per turn, the samples of a turn in flight before the first is used: with the few waves a span of this
            // size leaves room for, a turn per entry waits out one memory latency per entry
            for (uint32_t l = t; l < A.S; l += RS_MIX_STEP * T) {
                cf32 v[RS_MIX_STEP]; uint32_t p[RS_MIX_STEP], ix[RS_MIX_STEP];
#pragma unroll
                for (int u = 0; u < RS_MIX_STEP; u++) {
                    const uint32_t lu = l + u * T;
                    v[u].re = 0.0f; v[u].im = 0.0f;
                    if (lu < A.S) v[u] = capture_sample(A.src, c0 + (int64_t)lu);
                    p[u] = row * W + col; ix[u] = im;
                    im += im_step; if (im >= P) im -= P;
                    row += step_row; col += step_col;
                    if (row >= Q) { row -= Q; col++; }
                }
#pragma unroll
                for (int u = 0; u < RS_MIX_STEP; u++) {
                    if (l + u * T < A.S) {
#pragma unroll
                        for (int g = 0; g < G; g++) span[g * plane + p[u]] = cmul(v[u], cmul(t_hi[g][ix[u] / RS_OSC_LO], t_lo[g][ix[u] % RS_OSC_LO]));
                    }
                }
            }
        }
        __syncthreads();

        // ---- the lane's output: taps j = 0, 1, ... on span entries s_top, s_top - 1, ...
        float ar[G], ai[G];
#pragma unroll
        for (int g = 0; g < G; g++) { ar[g] = 0.0f; ai[g] = 0.0f; }
        uint32_t row = row_top, p = p_top;
        const float* hp = h_t;
        float hk[RS_TAP_STEP];
#pragma unroll
        for (int u = 0; u < RS_TAP_STEP; u++) { hk[u] = *hp; hp += L; }
        for (uint32_t j = 0; j < J; j += RS_TAP_STEP) {
            float hn[RS_TAP_STEP];                                                // (the table ends in one more step of zero rows: the fetch ahead)
#pragma unroll
            for (int u = 0; u < RS_TAP_STEP; u++) { hn[u] = *hp; hp += L; }
#pragma unroll
            for (int u = 0; u < RS_TAP_STEP; u++) {
#pragma unroll
                for (int g = 0; g < G; g++) {
                    const cf32 x = span[g * plane + p];
                    ar[g] = fmaf(hk[u], x.re, ar[g]); ai[g] = fmaf(hk[u], x.im, ai[g]);
                }
                if (row == 0) { row = Q - 1; p += (Q - 1) * W; p -= 1; } else { row--; p -= W; }      // one entry back
            }
#pragma unroll
            for (int u = 0; u < RS_TAP_STEP; u++) hk[u] = hn[u];
        }
        if (m < A.n_out) {                                                        // (the last tile)
#pragma unroll
            for (int g = 0; g < G; g++)
                if (e0 + g < A.n_ens) { cf32 y; y.re = ar[g]; y.im = ai[g]; A.dst.iq[(size_t)(e0 + g) * A.dst.iq_stride + ring_pos] = y; }
        }
    }
}

// The tile with the most outputs x ensembles whose planes fit RS_TILE_LARGE; of two such the one with more outputs (less of the span is
// converted twice).
bool resample_geometry(ResampleArgs& a)
{
    static const uint32_t forms[][2] = {{256, 4}, {256, 2}, {128, 4}, {256, 1}, {128, 2}, {64, 4}, {128, 1}, {64, 2}, {64, 1}};
    a.Q = (a.M + a.L / 2) / a.L;
    if (a.Q < 1 || a.J < 1 || a.J % RS_TAP_STEP) return false;
    for (const auto& f : forms) {
        const uint32_t T = f[0], G = f[1];
        const uint64_t S = (uint64_t)a.J + ((uint64_t)(a.L - 1) + (uint64_t)(T - 1) * a.M) / a.L, W = ((S + a.Q - 1) / a.Q) | 1u;
        if (G * a.Q * W <= (uint64_t)RS_TILE_LARGE) { a.T = T; a.G = G; a.S = (uint32_t)S; a.W = (uint32_t)W; return true; }
    }
    return false;
}

template <int G>
static void launch_resample_g(const ResampleArgs& a, unsigned tiles, hipStream_t s)
{
    const size_t need = (size_t)G * a.Q * a.W;
    if (need <= (size_t)RS_TILE_SMALL) hipLaunchKernelGGL((k_resample<G, RS_TILE_SMALL>), dim3(tiles), dim3(a.T), 0, s, a);
    else if (need <= (size_t)RS_TILE_MID) hipLaunchKernelGGL((k_resample<G, RS_TILE_MID>), dim3(tiles), dim3(a.T), 0, s, a);
    else hipLaunchKernelGGL((k_resample<G, RS_TILE_LARGE>), dim3(tiles), dim3(a.T), 0, s, a);
}

void launch_resample(const ResampleArgs& a, hipStream_t s)
{
    if (a.n_out) {
        const unsigned tiles = (unsigned)((a.n_out + a.T - 1) / a.T);
        if (a.G == 4) launch_resample_g<4>(a, tiles, s);
        else if (a.G == 2) launch_resample_g<2>(a, tiles, s);
        else launch_resample_g<1>(a, tiles, s);
    }
    launch_capture_carry(a.src, a.carry_out, s);
}

} // namespace dabphy
