/*
 * bpmx_rollmean.h — pandas' centred rolling mean, stated once: the window
 * bounds and the roll_mean recursion.  Used by the reference-mode envelope
 * (k_envelope_ref.hip), the rectified-mode envelope (k_rect.hip) and, on the
 * host, by tests/rect_core_driver.cpp (no HIP header needed).
 */
#ifndef BPMX_ROLLMEAN_H
#define BPMX_ROLLMEAN_H

#include "bpmx_pcm.h"

namespace bpmx {

/* pandas centered fixed window (pandas/core/indexers/objects.py:93-120) */
BPMX_HDI void win_bounds(int64_t i, int64_t n, int64_t w, int64_t &s, int64_t &e) {
    int64_t off = (w - 1) / 2;
    int64_t ee = i + 1 + off, ss = ee - w;
    e = ee < 0 ? 0 : (ee > n ? n : ee);
    s = ss < 0 ? 0 : (ss > n ? n : ss);
}

/* pandas roll_mean state (aggregations.pyx add_mean / remove_mean / calc_mean) */
struct RollMean {
    double sum = 0, cadd = 0, crem = 0, prev = 0;
    int32_t nobs = 0, neg = 0, same = 0;   /* <= recording length (< 2^31, host-checked) */
    BPMX_HDI void add(double v) {
        if (v == v) {
            nobs++;
            double y = v - cadd, t = sum + y;
            cadd = t - sum - y;
            sum = t;
            if (__builtin_signbit(v)) neg++;
            if (v == prev) same++; else same = 1;
            prev = v;
        }
    }
    BPMX_HDI void remove(double v) {
        if (v == v) {
            nobs--;
            double y = -v - crem, t = sum + y;
            crem = t - sum - y;
            sum = t;
            if (__builtin_signbit(v)) neg--;
        }
    }
    BPMX_HDI double mean() const {
        if (nobs >= 1) {
            double r = sum / (double)nobs;
            if (same >= nobs) r = prev;
            else if (neg == 0 && r < 0) r = 0;
            else if (neg == nobs && r > 0) r = 0;
            return r;
        }
        return __builtin_nan("");
    }
#if defined(__HIPCC__)
    /* exact copies across the launches of a chunked pass: 6 doubles */
    __device__ __forceinline__ void save(double *z) const {
        z[0] = sum; z[1] = cadd; z[2] = crem; z[3] = prev;
        z[4] = __longlong_as_double(((long long)nobs << 32) | (unsigned)neg); z[5] = __longlong_as_double(same);
    }
    __device__ __forceinline__ void load(const double *z) {
        sum = z[0]; cadd = z[1]; crem = z[2]; prev = z[3];
        const long long a = __double_as_longlong(z[4]);
        nobs = (int32_t)(a >> 32); neg = (int32_t)(unsigned)(a & 0xFFFFFFFFll); same = (int32_t)__double_as_longlong(z[5]);
    }
    /* branch-free forms (selects instead of the NaN / tie branches), the same
     * rounded operations when they apply: one basic block per prefetch block */
    __device__ __forceinline__ void add_sel(double v) {
        const bool ok = v == v;
        const double y = v - cadd, t = sum + y;
        cadd = ok ? (t - sum) - y : cadd;
        sum = ok ? t : sum;
        nobs += ok ? 1 : 0;
        neg += (ok && __signbit(v)) ? 1 : 0;
        int32_t sn = v == prev ? same + 1 : 1;
        __asm__ volatile("" : "+v"(sn));          /* keep it a select, not a branch */
        same = ok ? sn : same;
        prev = ok ? v : prev;
    }
    __device__ __forceinline__ void remove_sel(double v) {
        const bool ok = v == v;
        const double y = -v - crem, t = sum + y;
        crem = ok ? (t - sum) - y : crem;
        sum = ok ? t : sum;
        nobs -= ok ? 1 : 0;
        neg -= (ok && __signbit(v)) ? 1 : 0;
    }
    __device__ __forceinline__ double mean_sel() const {
        double r = sum / (double)nobs;
        __asm__ volatile("" : "+v"(r));           /* divide every step (its latency overlaps), no branch */
        r = same >= nobs ? prev : ((neg == 0 && r < 0) || (neg == nobs && r > 0) ? 0.0 : r);
        return nobs >= 1 ? r : __builtin_nan("");
    }
#endif
};

}  // namespace bpmx

#endif
