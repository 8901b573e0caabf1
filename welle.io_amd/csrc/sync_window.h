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

// ---- the order std::sort leaves the bin peaks in (phasereference.cpp:172-175: descending by value).  Among bit-identical peaks -- equal
// echoes give them -- it is whatever the C++ library's sort does, and which of them land among the first four decides the window index:
// this is that sort as libstdc++ runs it (introsort: median-of-three partitions down to 16 elements, heap sort below the depth limit,
// one insertion pass at the end), comparison for comparison, on bin numbers.  One thread; ord: the n bin numbers in ascending order on
// entry; stk: 3 ints per pending partition (at most 2 lg n + 1 of them).  The equal-echo families of tests/sync_cases.py need it; the
// restatement it is checked against calls std::sort itself (oracle/sort_order.cpp).  Out of line on purpose: it runs for tied peaks only, and
// inlined it changed how the compiler lays out the window search around it (measured 0.2 % on the headline; out of line: level).
__device__ __attribute__((noinline)) void std_sort_bins_desc(const float* val, int* ord, int* stk, const int n)
{
    const auto before = [&](int a, int b) { return val[a] > val[b]; };          // comp(lhs, rhs) on bin numbers
    const auto swp = [&](int i, int j) { const int x = ord[i]; ord[i] = ord[j]; ord[j] = x; };
    // std::__adjust_heap and the __push_heap at its end
    const auto adjust_heap = [&](int first, int hole, int len, int value) {
        const int top = hole;
        int child = hole;
        while (child < (len - 1) / 2) {
            child = 2 * (child + 1);
            if (before(ord[first + child], ord[first + child - 1])) child--;
            ord[first + hole] = ord[first + child]; hole = child;
        }
        if ((len & 1) == 0 && child == (len - 2) / 2) { child = 2 * (child + 1); ord[first + hole] = ord[first + child - 1]; hole = child - 1; }
        int parent = (hole - 1) / 2;
        while (hole > top && before(ord[first + parent], value)) { ord[first + hole] = ord[first + parent]; hole = parent; parent = (hole - 1) / 2; }
        ord[first + hole] = value;
    };
    const auto unguarded_linear_insert = [&](int last) {
        const int value = ord[last];
        int next = last - 1;
        while (before(value, ord[next])) { ord[last] = ord[next]; last = next; next--; }
        ord[last] = value;
    };
    // std::__introsort_loop, its recursion on the upper part kept on a stack
    int sp = 0;
    stk[0] = 0; stk[1] = n; stk[2] = 2 * (31 - __builtin_clz((unsigned)n)); sp = 1;
    while (sp > 0) {
        sp--;
        const int first = stk[3 * sp];
        int last = stk[3 * sp + 1], depth = stk[3 * sp + 2];
        while (last - first > 16) {
            if (depth == 0) {                                                     // std::__partial_sort(first, last, last): make_heap, sort_heap
                const int len = last - first;
                for (int parent = (len - 2) / 2; parent >= 0; parent--) adjust_heap(first, parent, len, ord[first + parent]);
                while (last - first > 1) { last--; const int value = ord[last]; ord[last] = ord[first]; adjust_heap(first, 0, last - first, value); }
                break;
            }
            depth--;
            const int a = first + 1, b = first + (last - first) / 2, c = last - 1;      // std::__move_median_to_first
            if (before(ord[a], ord[b])) {
                if (before(ord[b], ord[c])) swp(first, b); else if (before(ord[a], ord[c])) swp(first, c); else swp(first, a);
            } else if (before(ord[a], ord[c])) swp(first, a);
            else if (before(ord[b], ord[c])) swp(first, c);
            else swp(first, b);
            int lo = first + 1, hi = last;                                        // std::__unguarded_partition around ord[first]
            for (;;) {
                while (before(ord[lo], ord[first])) lo++;
                hi--;
                while (before(ord[first], ord[hi])) hi--;
                if (!(lo < hi)) break;
                swp(lo, hi); lo++;
            }
            stk[3 * sp] = lo; stk[3 * sp + 1] = last; stk[3 * sp + 2] = depth; sp++;
            last = lo;
        }
    }
    // std::__final_insertion_sort
    const int head = n > 16 ? 16 : n;
    for (int i = 1; i < head; i++) {
        if (before(ord[i], ord[0])) { const int value = ord[i]; for (int j = i; j > 0; j--) ord[j] = ord[j - 1]; ord[0] = value; }
        else unguarded_linear_insert(i);
    }
    for (int i = head; i < n; i++) unguarded_linear_insert(i);
}

// ---- FFTPlacementMethod::EarliestPeakWithBinning (phasereference.cpp:125-211): peaks over 102 bins of 20 samples (2040..2047 are
// never looked at), the highest peak, the 4 highest bins within 500 samples of it, those above 3 * mean, the earliest.
// pa: T_U floats of LDS behind lbuf (bin peaks and their indices; the sort's permutation and stack when it is needed).
__device__ __forceinline__ int window_earliest_peak_binned(const float* lbuf, float* pa, int* redi, float* s_sum, float* cir, const int t)
{
    constexpr int NB = 102;
    float* const bval = pa; int* const bidx = reinterpret_cast<int*>(pa + 128);
    int* const ord = reinterpret_cast<int*>(pa + 256); int* const stk = reinterpret_cast<int*>(pa + 384);
    if (t == 0) { float s = 0; for (int i = 0; i < 2040; i++) s += lbuf[i]; *s_sum = s; }    // `mean += value` in index order
    if (t < NB) {
        float pv = 0.0f; int pi = -1;
        for (int j = 0; j < 20; j++) { const float v2 = lbuf[20 * t + j]; if (v2 > pv) { pv = v2; pi = 20 * t + j; } }
        bval[t] = pv; bidx[t] = pi; ord[t] = t;
    }
    if (cir && t < 8) cir[2040 + t] = 0.0f;                                                  // the reference's buffer keeps its zeros there
    __syncthreads();
    if (t == 0) {
        const float mean = *s_sum / T_U;
        // std::sort by value (descending) is replaced by selection -- as long as no two peaks that matter are bit-identical: the highest
        // one (the distances are taken from it), and the fourth against the fifth of those within 500 samples (the first four are kept).
        // `ties` counts the bins that equal the one selected and were passed over, in those two places.
        int top = 0, ties = 0, ties4 = 0;
        for (int k = 1; k < NB; k++) { if (bval[k] > bval[top]) { top = k; ties = 0; } else if (bval[k] == bval[top]) ties++; }
        const int peak_index = bidx[top];
        unsigned long long used_lo = 0, used_hi = 0;
        int found = 0, mn = 0;
        for (int pass = 0; pass < 4 && bval[top] != 0.0f; pass++) {
            int best = -1;
            for (int k = 0; k < NB; k++) {
                const bool used = k < 64 ? (used_lo >> k) & 1 : (used_hi >> (k - 64)) & 1;
                const int dist = bidx[k] - peak_index;
                if (used || (dist < 0 ? -dist : dist) > 500) continue;
                if (best < 0 || bval[k] > bval[best]) { best = k; ties4 = 0; }
                else if (pass == 3 && bval[k] == bval[best]) ties4++;
            }
            if (best < 0) break;
            if (best < 64) used_lo |= 1ull << best; else used_hi |= 1ull << (best - 64);
            if (bval[best] < 3 * mean) continue;
            if (!found || bidx[best] < mn) { mn = bidx[best]; found = 1; }
        }
        if ((ties | ties4) != 0 && bval[top] != 0.0f) {
            // bit-identical peaks where it matters: the library's order decides (std_sort_bins_desc), then phasereference.cpp:177-209 as written
            std_sort_bins_desc(bval, ord, stk, NB);
            const int peak2 = bidx[ord[0]];
            found = 0; mn = 0;
            for (int a = 0, kept = 0; a < NB && kept < 4; a++) {
                const int k = ord[a], dist = bidx[k] - peak2;
                if ((dist < 0 ? -dist : dist) > 500) continue;
                kept++;
                if (bval[k] < 3 * mean) continue;
                if (!found || bidx[k] < mn) { mn = bidx[k]; found = 1; }
            }
        }
        // (an all-zero response: every bin holds index -1 and passes `0 < 3 * 0`: min_element gives -1, which is also "no peak")
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
