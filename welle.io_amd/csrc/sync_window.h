// welle.io_amd/csrc/sync_window.h -- PhaseReference::findIndex (phasereference.cpp:73-256) for one work-group of FFT_THREADS threads:
// the impulse response of the phase reference symbol and the three FFTPlacementMethods that pick the window index from it.
// The LDS buffers belong to the caller (k_sync.hip: sync_find_body) and come in as pointers.
#pragma once
#include "fft2048.h"
#include "dabphy_kernels.h"
#include "mix2048.h"
#include "block_reduce.h"

namespace dabphy {

// ---- the impulse response (phasereference.cpp:73-92): FFT of the T_u samples at pos, multiply by conj(refTable), IFFT (scaled by 1/N);
// its magnitudes (:214-215) go to lbuf[0 .. T_u) (+ 128 zeros behind them), and to cir when asked.  tile is the FFT's workspace and
// becomes lbuf: they share their LDS.  ts(k): the caller's timing stamps 1 .. 4 (samples, FFT, IFFT, cir), a no-op outside the
// SYNC_CHAIN_TS experiment.
template <class Stamp>
__device__ __forceinline__ void prs_impulse_response(const SyncArgs& A, const cf32* __restrict__ iq, const FrameDesc& d, const FftTwiddles& w,
                                                     cf32* tile, float* lbuf, float* cir, const int t, const Stamp ts)
{
    cf32 v[16], u[16];
    load_mix2048(v, iq, A.ring, d.pos, 0, A.tab.nco, d.L0, d.f_prs, 0, t);
#ifdef SYNC_CHAIN_TS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    ts(1);
    fft2048_wg<false>(v, tile, w, t);
    ts(2);
#pragma unroll
    for (int j = 0; j < 16; j++) v[j] = cmul(v[j], cconj(A.tab.ref[t + 128 * j]));
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
        for (int j = 0; j < 8; j++) u[8 * h + j] = v[h + 2 * j];          // bin t + 128 (h + 2j) = input t + 128h + 256j
    fft2048_wg<true>(u, tile, w, t);
    ts(3);
    __syncthreads();                                                       // all round-C reads of the tile are done: it becomes lbuf / pa
    const float factor = 1.0f / (float)T_U;                                // fft.cpp:154
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const float a = hypotf_exact(u[j].re * factor, u[j].im * factor);  // phasereference.cpp:214-215
        lbuf[t + 128 * j] = a;
        if (cir) cir[t + 128 * j] = a;
    }
    if (t < 128) lbuf[T_U + t] = 0.0f;
    __syncthreads();
    ts(4);
}

// ---- FFTPlacementMethod::StrongestPeak (phasereference.cpp:99-129): sum in order, first maximum
__device__ __forceinline__ int window_strongest_peak(const float* lbuf, float* redf, int* redi, float* s_sum, const int t)
{
    if (t == 0) { float s = 0; for (int i = 0; i < T_U; i++) s += lbuf[i]; *s_sum = s; }
    float mx = -10000.0f;
#pragma unroll
    for (int j = 0; j < 16; j++) mx = fmaxf(mx, lbuf[16 * t + j]);
    const float gmax = block_max(mx, redf, t);
    int cand = T_U;
    for (int j = 15; j >= 0; j--) if (lbuf[16 * t + j] == gmax) cand = 16 * t + j;
    const int first = block_min_int(cand, redi, t);
    const float sum = *s_sum;
    if (sum == 0) return -1;
    if (gmax < 3 * sum / T_U) return (int)(-fabsf(gmax * T_U / sum) - 1);
    return first;
}

// ---- FFTPlacementMethod::EarliestPeakWithBinning (phasereference.cpp:125-211): peaks over 102 bins of 20 samples (2040..2047 are
// never looked at), the highest peak, the 4 highest bins within 500 samples of it, those above 3 * mean, the earliest.
// pa: T_U floats of LDS behind lbuf (bin peaks and their indices).
__device__ __forceinline__ int window_earliest_peak_binned(const float* lbuf, float* pa, int* redi, float* s_sum, float* cir, const int t)
{
    float* const bval = pa; int* const bidx = reinterpret_cast<int*>(pa + 128);
    if (t == 0) { float s = 0; for (int i = 0; i < 2040; i++) s += lbuf[i]; *s_sum = s; }    // `mean += value` in index order
    if (t < 102) {
        float pv = 0.0f; int pi = -1;
        for (int j = 0; j < 20; j++) { const float v2 = lbuf[20 * t + j]; if (v2 > pv) { pv = v2; pi = 20 * t + j; } }
        bval[t] = pv; bidx[t] = pi;
    }
    if (cir && t < 8) cir[2040 + t] = 0.0f;                                                  // the reference's buffer keeps its zeros there
    __syncthreads();
    if (t == 0) {
        const float mean = *s_sum / T_U;
        // std::sort by value (descending) is replaced by selection: the order among exactly equal peaks is the bin order
        int top = 0;
        for (int k = 1; k < 102; k++) if (bval[k] > bval[top]) top = k;
        const int peak_index = bidx[top];
        unsigned long long used_lo = 0, used_hi = 0;
        int found = 0, mn = 0;
        for (int pass = 0; pass < 4; pass++) {
            int best = -1;
            for (int k = 0; k < 102; k++) {
                const bool used = k < 64 ? (used_lo >> k) & 1 : (used_hi >> (k - 64)) & 1;
                const int dist = bidx[k] - peak_index;
                if (used || (dist < 0 ? -dist : dist) > 500) continue;
                if (best < 0 || bval[k] > bval[best]) best = k;
            }
            if (best < 0) break;
            if (best < 64) used_lo |= 1ull << best; else used_hi |= 1ull << (best - 64);
            if (bval[best] < 3 * mean) continue;
            if (!found || bidx[best] < mn) { mn = bidx[best]; found = 1; }
        }
        redi[0] = found ? mn : -1;
    }
    __syncthreads();
    const int startIndex = redi[0];
    __syncthreads();
    return startIndex;
}

// ---- FFTPlacementMethod::ThresholdBeforePeak (phasereference.cpp:212-252).  pa: T_U floats of LDS behind lbuf (peak_averages).
__device__ __forceinline__ int window_threshold_before_peak(const float* lbuf, float* pa, float* redf, int* redi, float* s_sum, const int t)
{
    if (t == 0) {                                                                          // :214-218, in order
        float s = 0; const float4* l4 = reinterpret_cast<const float4*>(lbuf);
        for (int i = 0; i < T_U / 4; i += 4) {
            const float4 q0 = l4[i], q1 = l4[i + 1], q2 = l4[i + 2], q3 = l4[i + 3];
            s += q0.x; s += q0.y; s += q0.z; s += q0.w; s += q1.x; s += q1.y; s += q1.z; s += q1.w;
            s += q2.x; s += q2.y; s += q2.z; s += q2.w; s += q3.x; s += q3.y; s += q3.z; s += q3.w;
        }
        *s_sum = s;
    }
    // peak_averages[i] = max(lbuf[i .. i+99]) for i < 1948; thread t owns i = 16t .. 16t+15
    float mx = -10000.0f;
    if (16 * t < T_U - 100) {
        float common = -10000.0f;                                   // lbuf[16t+15 .. 16t+99]
        for (int k = 16 * t + 15; k <= 16 * t + 99; k++) common = fmaxf(common, lbuf[k]);
        float suf[16];                                              // suf[k] = max(lbuf[16t+k .. 16t+14])
        float run = -10000.0f;
#pragma unroll
        for (int k = 14; k >= 0; k--) { run = fmaxf(run, lbuf[16 * t + k]); suf[k] = run; }
        suf[15] = -10000.0f;
        run = -10000.0f;                                            // prefix over lbuf[16t+100 .. 16t+99+k]
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const int i = 16 * t + k;
            if (k > 0) run = fmaxf(run, lbuf[16 * t + 99 + k]);
            float m = fmaxf(common, suf[k]);
            if (k > 0) m = fmaxf(m, run);
            if (i + 100 < T_U) { pa[i] = m; mx = fmaxf(mx, m); } else pa[i] = 0.0f;
        }
    } else {
        for (int k = 0; k < 16; k++) pa[16 * t + k] = 0.0f;
    }
    const float gmax = block_max(mx, redf, t);                       // contains the barriers that publish pa / s_sum
    const float sum = *s_sum;
    int cand = T_U;
    if (gmax > 3 * sum / T_U) {                                      // :238-239
        const float thresh = gmax / 2;
        for (int k = 15; k >= 0; k--) {
            const int i = 16 * t + k;
            if (i + 100 < T_U && pa[i + 100] > thresh) cand = i;    // :241-245
        }
    }
    const int first = block_min_int(cand, redi, t);
    return first < T_U ? first : -1;
}

} // namespace dabphy
