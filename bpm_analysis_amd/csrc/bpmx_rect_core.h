/*
 * bpmx_rect_core.h — the arithmetic of the rectified-mode envelope, stated
 * once for the kernels (k_rect.hip) and for the host driver
 * (tests/rect_core_driver.cpp; no HIP header needed).
 *
 * The mode restates heartbeat_labeler.py:53-67 on a filtered WAV:
 *   x = frame value (wavfile.read, np.mean(axis=1) for more than one channel)
 *   a = np.abs(x) in x's dtype
 *   env = pd.Series(a).rolling(window=w, min_periods=1, center=True).mean()
 */
#ifndef BPMX_RECT_CORE_H
#define BPMX_RECT_CORE_H

#include "bpmx_rollmean.h"

namespace bpmx {

/* np.abs on the integer sample types.  The most negative value has no
 * positive counterpart and numpy's abs wraps to itself, so it stays a negative
 * sample (np.abs(np.int16(-32768)) == -32768); negating it in C++ is undefined,
 * so it is tested for.  u8 is unsigned: unchanged. */
BPMX_HDI int64_t rect_abs_int(int dtype, int64_t v) {
    if (dtype == BPMX_DT_I16) return v == -32768 ? v : (v < 0 ? -v : v);
    if (dtype == BPMX_DT_I32) return v == -(int64_t)2147483648LL ? v : (v < 0 ? -v : v);
    return v;
}

/* The rectified value of an integer frame as an integer: a for one channel,
 * 2 a = |l + r| for two (x = (l + r) / 2 in f64 is exact, and so is its abs). */
template <typename T>
BPMX_HDI int64_t rect_int_frame(int dtype, bool stereo, const T *p) {
    if (!stereo) return rect_abs_int(dtype, (int64_t)p[0]);
    const int64_t s = (int64_t)p[0] + (int64_t)p[1];
    return s < 0 ? -s : s;
}

/* pandas maps +-inf to NaN before the window functions see the values
 * (_prep_values, pandas/core/window/rolling.py:375-378) */
BPMX_HDI double rect_inf_to_nan(double v) {
    return (v - v) == (v - v) ? v : __builtin_nan("");      /* v - v is NaN for NaN and +-inf */
}

/* a[i] as the f64 that pandas' window function adds, any dtype and channel
 * count: abs in the working dtype (work_dtype), widened, inf -> NaN */
BPMX_HDI double rect_value(const void *pcm, int dtype, int channels, int64_t frame) {
    const double x = frame_value(pcm, dtype, channels, frame);
    double a;
    switch (work_dtype(dtype, channels)) {
    case BPMX_DT_U8: a = x; break;
    case BPMX_DT_I16:
    case BPMX_DT_I32: a = (double)rect_abs_int(work_dtype(dtype, 1), (int64_t)x); break;
    case BPMX_DT_F32: a = (double)__builtin_fabsf((float)x); break;
    default: a = __builtin_fabs(x); break;
    }
    return rect_inf_to_nan(a);
}

/* The mean of a window whose sum is exact: S the int64 sum of the window's
 * rectified integer frames (rect_int_frame), nobs = e - s its length.  One
 * IEEE division; S * 0.5 is exact. */
BPMX_HDI double rect_mean_exact(int64_t S, int64_t nobs, bool stereo) {
    if (nobs < 1) return __builtin_nan("");
    const double s = stereo ? (double)S * 0.5 : (double)S;
    return s / (double)nobs;
}

/* Windows for which the exact-integer route holds: a frame's integer is at
 * most 2^32 in magnitude, so every partial sum pandas forms is an integer (or
 * half-integer) below 2^53 while w * 2^32 < 2^53. */
constexpr int64_t RECT_W_EXACT_MAX = (int64_t(1) << 21) - 1;

/* The general route on one recording: pandas' roll_mean recursion (variable
 * algorithm over the centred bounds) on values v(j), j in [0, n).  Removes
 * come before adds, a window that starts at or past the previous end (w == 1)
 * starts afresh. */
template <typename VF, typename OF>
BPMX_HDI void rect_roll_mean(int64_t n, int64_t w, VF v, OF out) {
    const int64_t off = (w - 1) / 2;
    RollMean R;
    for (int64_t i = 0; i < n; ++i) {
        if (i == 0 || w == 1) {
            int64_t s, e;
            win_bounds(i, n, w, s, e);
            R = RollMean();
            R.prev = v(s);
            for (int64_t j = s; j < e; ++j) R.add(v(j));
        } else {
            const int64_t s = i + 1 + off - w;      /* unclipped start; remove when it advances */
            if (s > 0) R.remove(v(s - 1));
            if (i + off < n) R.add(v(i + off));
        }
        out(i, R.mean());
    }
}

}  // namespace bpmx

#endif
