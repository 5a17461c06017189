/*
 * bpmx_beats_core.h — the beat stages after the hot path (bpm_analysis.py
 * :1734-1757: preliminary pass, PeakClassifier, _refine_and_correct_peaks,
 * calculate_bpm_series) stated once for host and device.
 *
 * It restates bpmx_beats of host/beats_host.cpp in the same IEEE operation
 * order, over the packed form only: idx[n], env_pk[n], floor_pk[n] (bpmx_pack's
 * per-peak tables; idx strictly increasing).  Wherever the host code reads
 * env[raw[k]] or floor[raw[k]] this reads table entry k, and beats are carried
 * as table positions (their samples are idx[k]); with strictly increasing idx
 * the host's searches of a beat among the raw peaks are the position itself.
 *
 * No std:: containers and no allocation: every temporary lives in a workspace
 * the caller supplies (beats_ws_bytes / beats_ws_layout).  Functions carry
 * BPMX_HD: __host__ __device__ under hipcc, nothing under a plain C++ compiler,
 * so the text k_beats.hip runs on a wave is the text a CPU test and a host
 * sanitizer build exercise.
 *
 * Execution: an executor X gives lane(), width() and sync().  The order-
 * dependent parts (the classifier walk, the Kahan rolling means, the
 * refinement passes) run on lane 0 between two sync()s; the gathers (strength,
 * raw deviation, dev_t, the RR arrays, window bounds of the fixed window, the
 * copies out) and the sort are BPMX_PAR_FOR loops over all lanes.  Scalars a
 * serial part decides travel through the workspace header, read after a
 * sync().  beats_serial is the host instantiation (one lane, sync a no-op).
 * Every call must be made by all lanes of the executor with the same
 * arguments.
 *
 * Workspace slots are reused by phase (n8 = n rounded up to 8):
 *   S0..S3  f64[n8]   classifier: strength, smoothed deviation, dev_t, raw
 *                     deviation; BPM series: bpm, beat times, curve (first the
 *                     sort buffer of the median), ns (as int64); refinement:
 *                     RR, sorted RR
 *   I0..I2  i32[n8]   beats (table positions) | rolling-window start / gap
 *                     candidates | window end / merged beats
 *   tag, paired, mark  i8[n8]
 * The classifier's arrays are made twice (before the anchor pass and before
 * the main pass, as the host code constructs its Classifier twice), which lets
 * the anchor pass' BPM series reuse their slots.
 */
#ifndef BPMX_BEATS_CORE_H
#define BPMX_BEATS_CORE_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/bpmx_host.h"
#include "../../include/bpmx.h" /* bpmx_trace_field, bpmx_trace_code: the layout of the decision trace */

#if defined(__HIPCC__)
#define BPMX_HD __host__ __device__
#else
#define BPMX_HD
#endif

/* the "parallel for" hook: lanes stride over [0, n); follow it with x.sync() */
#define BPMX_PAR_FOR(x, i, n) for (int64_t i = (x).lane(); i < (int64_t)(n); i += (x).width())

namespace bpmx {

struct beats_serial {
    BPMX_HD int lane() const { return 0; }
    BPMX_HD int width() const { return 1; }
    BPMX_HD void sync() const {}
};

/* ---- workspace ---------------------------------------------------------- */
enum {
    BEATS_WS_HDR = 128,          /* 8 doubles, 16 int32 */
    BEATS_WS_PER_PEAK = 4 * 8 + 3 * 4 + 3,   /* S0..S3, I0..I2, tag/paired/mark */
    BEATS_WS_STAGE = 4 + 8,      /* a copy of idx and env_pk in front (the LDS path) */
    /* bytes(n, false) <= BEATS_WS_FIXED + BEATS_WS_STRIDE * n: recording f's
     * slice of a shared buffer starts at f * FIXED + STRIDE * pk_off[f] */
    BEATS_WS_STRIDE = 48,
    BEATS_WS_FIXED = BEATS_WS_HDR + 7 * BEATS_WS_STRIDE
};

BPMX_HD constexpr int64_t beats_n8(int64_t n) { return (n + 7) & ~(int64_t)7; }
BPMX_HD constexpr size_t beats_ws_bytes(int64_t n, bool stage) {
    return (size_t)BEATS_WS_HDR + (size_t)beats_n8(n) * (size_t)(BEATS_WS_PER_PEAK + (stage ? BEATS_WS_STAGE : 0));
}
/* the most peaks whose staged workspace fits `budget` bytes */
BPMX_HD constexpr int64_t beats_ws_max_peaks(size_t budget) {
    return budget < (size_t)BEATS_WS_HDR
               ? 0
               : (int64_t)((budget - BEATS_WS_HDR) / (BEATS_WS_PER_PEAK + BEATS_WS_STAGE)) & ~(int64_t)7;
}

struct beats_ws {
    double *hd;                  /* header doubles [8] */
    int32_t *hi;                 /* header ints [16] */
    double *S[4];
    int32_t *I[3];
    int8_t *tag, *paired, *mark;
    double *env_stage;           /* stage only */
    int32_t *idx_stage;
};
enum { BH_START = 0, BH_TPK = 1, BH_TEND = 2, BH_EST = 3 };                       /* hd */
enum { BH_NA = 0, BH_REC = 1, BH_NS1 = 2, BH_M = 3, BH_OK = 4, BH_NFIX = 5, BH_NT = 6, BH_NC = 7 };  /* hi */

/* base must be 8-byte aligned */
BPMX_HD inline beats_ws beats_ws_layout(void *base, int64_t n, bool stage) {
    const int64_t n8 = beats_n8(n);
    char *p = (char *)base;
    beats_ws w;
    w.hd = (double *)p;
    w.hi = (int32_t *)(p + 64);
    p += BEATS_WS_HDR;
    for (int k = 0; k < 4; ++k) { w.S[k] = (double *)p; p += 8 * n8; }
    w.env_stage = nullptr;
    w.idx_stage = nullptr;
    if (stage) { w.env_stage = (double *)p; p += 8 * n8; }
    for (int k = 0; k < 3; ++k) { w.I[k] = (int32_t *)p; p += 4 * n8; }
    if (stage) { w.idx_stage = (int32_t *)p; p += 4 * n8; }
    w.tag = (int8_t *)p; p += n8;
    w.paired = (int8_t *)p; p += n8;
    w.mark = (int8_t *)p;
    return w;
}

/* ---- scalar helpers (beats_host.cpp, same order) ------------------------- */
BPMX_HD inline double bc_nan() { return __builtin_nan(""); }
BPMX_HD inline double py_min(double a, double b) { return b < a ? b : a; }
BPMX_HD inline double py_max(double a, double b) { return b > a ? b : a; }
BPMX_HD inline double clipv(double x, double lo, double hi) {      /* numpy.clip on a scalar */
    if (x != x) return x;
    if (x < lo) return lo;
    if (x > hi) return hi;
    return x;
}
/* first position whose value is > x (std::upper_bound) */
BPMX_HD inline int64_t bc_upper(const double *a, int64_t n, double x) {
    int64_t lo = 0, len = n;
    while (len > 0) {
        const int64_t half = len >> 1;
        if (!(x < a[lo + half])) { lo += half + 1; len -= half + 1; } else len = half;
    }
    return lo;
}
/* a[k] of a small table for a run-time k, as selects over constant positions:
 * the table stays in registers (a local array indexed at run time would live
 * in scratch memory on the device, a round trip per probe on the serial lane) */
template <int N, int I>
struct bc_sel {                  /* positions I..N-1: constant indices from the start, not after unrolling */
    BPMX_HD static double get(const double (&a)[N], int k, double r) {
        return bc_sel<N, I + 1>::get(a, k, k == I ? a[I] : r);
    }
};
template <int N>
struct bc_sel<N, N> {
    BPMX_HD static double get(const double (&)[N], int, double r) { return r; }
};
template <int N>
BPMX_HD inline double bc_at(const double (&a)[N], int k) {
    return bc_sel<N, 1>::get(a, k, a[0]);
}
/* numpy.interp for one x (compiled_base.c arr_interp); the bracket by
 * std::upper_bound's own probes */
template <int N>
BPMX_HD inline double interp1(double x, const double (&xp)[N], const double (&fp)[N]) {
    if (x != x) return x;
    if (x < xp[0]) return fp[0];
    if (x > xp[N - 1]) return fp[N - 1];
    int lo = 0, len = N;
    while (len > 0) {
        const int half = len >> 1;
        if (!(x < bc_at(xp, lo + half))) { lo += half + 1; len -= half + 1; } else len = half;
    }
    const int j = lo - 1;
    const double xj = bc_at(xp, j), fj = bc_at(fp, j);
    if (j == N - 1 || xj == x) return fj;
    const double xj1 = bc_at(xp, j + 1), fj1 = bc_at(fp, j + 1);
    const double slope = (fj1 - fj) / (xj1 - xj);
    double r = slope * (x - xj) + fj;
    if (r != r) {
        r = slope * (x - xj1) + fj1;
        if (r != r && fj == fj1) r = fj;
    }
    return r;
}
BPMX_HD inline double blend(double bpm, const bpmx_beat_params &p) {
    return clipv((bpm - p.contractility_bpm_low) / (p.contractility_bpm_high - p.contractility_bpm_low), 0, 1);
}
BPMX_HD inline double blended_confidence(double dev, double bpm, const bpmx_beat_params &p) {
    const double DEV_X[5] = {0.0, 0.25, 0.40, 0.80, 1.0};
    const double CURVE_LO[5] = {0.9, 0.9, 0.7, 0.1, 0.1};
    const double CURVE_HI[5] = {0.1, 0.5, 0.75, 0.65, 0.0};
    const double b = blend(bpm, p);
    double fp[5];
    for (int i = 0; i < 5; ++i) fp[i] = CURVE_LO[i] + (CURVE_HI[i] - CURVE_LO[i]) * b;
    return interp1(dev, DEV_X, fp);
}
BPMX_HD inline double update_long_term_bpm(double rr, double ltb, const bpmx_beat_params &p) {
    const double target = (1 - 0.05) * ltb + 0.05 * (60.0 / rr);
    const double lim = 3.0 * rr;
    const double step = clipv(target - ltb, -lim, lim);
    return py_max(p.min_bpm, py_min(ltb + step, p.max_bpm));
}
/* numpy.median of a sorted array */
BPMX_HD inline double median_sorted(const double *s, int64_t n) {
    if (n & 1) return s[n / 2];
    return (s[n / 2 - 1] + s[n / 2]) / 2.0;
}
/* numpy.percentile(v, q) 'linear' (numpy _lerp) of a sorted array */
BPMX_HD inline double percentile_sorted(const double *s, int64_t n, double q) {
    const double vi = (double)(n - 1) * (q / 100.0);
    double lo = ::floor(vi);
    if (lo > (double)(n - 1)) lo = (double)(n - 1);
    const int64_t l = (int64_t)lo, h = l + 1 < n ? l + 1 : n - 1;
    const double g = vi - lo, a = s[l], b = s[h], d = b - a;
    return g >= 0.5 ? b - d * (1 - g) : a + d * g;
}
/* datetime.timedelta(seconds=x) in microseconds (CPython: modf, then the
 * fractional part times 1e6 rounded half to even) */
BPMX_HD inline int64_t timedelta_us(double x) {
    double ip;
    const double fr = ::modf(x, &ip);
    return (int64_t)ip * 1000000 + (int64_t)::nearbyint(fr * 1e6);
}

/* pandas roll_mean over [st[i], en[i]) with monotone bounds (Kahan add /
 * remove, 'same value' and sign rules: pandas/_libs/window/aggregations.pyx).
 * Order-dependent: one lane. */
struct bc_roll {
    double sum, ca, cr, prev;
    int64_t nobs, neg, same;
    BPMX_HD void add(double x) {
        if (x != x) return;
        nobs++;
        const double y = x - ca, t = sum + y;
        ca = t - sum - y;
        sum = t;
        if (__builtin_signbit(x)) neg++;
        if (x == prev) same++; else same = 1;
        prev = x;
    }
    BPMX_HD void rem(double x) {
        if (x != x) return;
        nobs--;
        const double y = -x - cr, t = sum + y;
        cr = t - sum - y;
        sum = t;
        if (__builtin_signbit(x)) neg--;
    }
};
BPMX_HD inline void roll_mean(const double *v, const int32_t *st, const int32_t *en, int64_t n, int64_t minp,
                              double *out) {
    bc_roll R;
    R.sum = R.ca = R.cr = 0;
    R.prev = bc_nan();
    R.nobs = R.neg = R.same = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t s = st[i], e = en[i];
        if (i == 0 || s >= en[i - 1]) {
            R.sum = R.ca = R.cr = 0;
            R.nobs = R.neg = 0;
            R.prev = v[s];
            R.same = 0;
            for (int64_t j = s; j < e; ++j) R.add(v[j]);
        } else {
            for (int64_t j = st[i - 1]; j < s; ++j) R.rem(v[j]);
            for (int64_t j = en[i - 1]; j < e; ++j) R.add(v[j]);
        }
        double r;
        if (R.nobs >= minp && R.nobs > 0) {
            r = R.sum / (double)R.nobs;
            if (R.same >= R.nobs) r = R.prev;
            else if (R.neg == 0 && r < 0) r = 0;
            else if (R.neg == R.nobs && r > 0) r = 0;
        } else {
            r = bc_nan();
        }
        out[i] = r;
    }
}

/* ---- the sort: all lanes ------------------------------------------------- */
/* An exact ascending sort of n finite values: the bitonic network with every
 * comparison directed low to high (a block's first step pairs i with its
 * mirror i ^ (k - 1)), over the next power of two with the positions at and
 * beyond n standing for +inf, which such a network never moves, so pairs
 * that reach them are skipped.  Entered with a[] visible to all lanes; ends
 * with a sync(). */
template <class X>
BPMX_HD inline void beats_sort(const X &x, double *a, int64_t n) {
    if (n < 2) return;
    int64_t N = 2;
    while (N < n) N <<= 1;
    const int64_t half = N >> 1;
    for (int64_t k = 2; k <= N; k <<= 1) {
        for (int64_t j = k >> 1; j >= 1; j >>= 1) {
            const bool flip = j == (k >> 1);
            BPMX_PAR_FOR(x, t, half) {
                const int64_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int64_t l = flip ? (i ^ (k - 1)) : (i | j);
                if (l < n) {
                    const double u = a[i], v = a[l];
                    if (v < u) { a[i] = v; a[l] = u; }
                }
            }
            x.sync();
        }
    }
}

/* ---- the classifier ------------------------------------------------------ */
enum { BT_NONE = 0, BT_S1 = 1, BT_S2 = 2, BT_LONE = 3, BT_NOISE = 4 };

/* ---- the decision trace (optional) --------------------------------------- */
/* What the main classification pass and the gap fill decide, kept for the
 * reference's per-peak debug strings (beats.PeakClassifier._pair / ._lone,
 * fix_rhythmic_discontinuities): a trace sink T is a policy of the functions
 * below.  bc_notrace (the default) has on == 0 and empty members, so every
 * `if (T::on)` block falls away and the instantiation is the code without a
 * trace.  beats_trace stores into one recording's slices (all at pk_off[f]):
 *   rec   f64[n][BPMX_TR_NFIELDS]  the values a peak's strings format; only the
 *                                  fields its code announces are written
 *   code  i32[n]   BPMX_TR_* outcome | BPMX_TRF_* optional lines
 *   lt_pos / lt_bpm [n_lt]  after every classifier iteration with a beat: the
 *                                  table position of the last beat, the belief
 *   dev_t / dev [n - 1]     the main pass' smoothed deviation series
 *   gap   i32[n]   the label pass `it` of the gap fill gave the peak in bits
 *                  2 it .. 2 it + 1 (BPMX_TR_GAP_*)
 * The serial parts store from lane 0 where they decide; dev_t, dev and the
 * zeroes of gap are written by all lanes. */
struct bc_notrace {
    enum { on = 0 };
    BPMX_HD void put(int64_t, int, double) const {}
    BPMX_HD void code_at(int64_t, int32_t) const {}
    BPMX_HD void belief(int64_t, int32_t, double) const {}
    BPMX_HD void beliefs(int64_t) const {}
    BPMX_HD void gap_label(int64_t, int, int) const {}
    BPMX_HD void gap_clear(int64_t) const {}
    BPMX_HD void deviation(int64_t, double, double) const {}
};
struct beats_trace {
    enum { on = 1 };
    double *rec;
    int32_t *code, *lt_pos;
    double *lt_bpm;
    int32_t *n_lt;                                    /* this recording's count */
    double *dev_t, *dev;
    int32_t *gap;
    BPMX_HD void put(int64_t j, int field, double v) const { rec[j * BPMX_TR_NFIELDS + field] = v; }
    BPMX_HD void code_at(int64_t j, int32_t v) const { code[j] = v; }
    BPMX_HD void belief(int64_t k, int32_t pos, double bpm) const { lt_pos[k] = pos; lt_bpm[k] = bpm; }
    BPMX_HD void beliefs(int64_t k) const { *n_lt = (int32_t)k; }
    BPMX_HD void gap_label(int64_t j, int it, int label) const { gap[j] |= label << (2 * it); }
    BPMX_HD void gap_clear(int64_t j) const { gap[j] = 0; }
    BPMX_HD void deviation(int64_t i, double t, double v) const { dev_t[i] = t; dev[i] = v; }
};

/* strength, the smoothed deviation series and its times (PeakClassifier's
 * constructor): gathers on all lanes, the Kahan rolling mean on lane 0 */
template <class X>
BPMX_HD inline void beats_prepare(const X &x, int64_t n, const int32_t *idx, const double *env, const double *flo,
                                  int32_t sr, const bpmx_beat_params &p, const beats_ws &w) {
    double *str = w.S[0], *dev = w.S[1], *dev_t = w.S[2], *raw = w.S[3];
    int32_t *st = w.I[1], *en = w.I[2];
    const int64_t nd = n > 1 ? n - 1 : 0;
    int64_t win = (int64_t)((double)nd * p.deviation_smoothing_factor);
    if (win < 5) win = 5;
    const int64_t off = (win - 1) / 2;
    BPMX_PAR_FOR(x, i, n) {
        const double s = env[i] - flo[i];
        str[i] = s > 0 ? s : 0.0;                          /* max(0, e - f) */
    }
    BPMX_PAR_FOR(x, i, nd) {
        const double sa = env[i] - flo[i], sb = env[i + 1] - flo[i + 1];
        const double a = sa < 0 ? 0 : sa, b = sb < 0 ? 0 : sb;         /* strength[strength < 0] = 0 */
        const double mx = (a != a || b != b) ? bc_nan() : (a > b ? a : b);     /* np.maximum */
        raw[i] = ::fabs(b - a) / (mx + 1e-9);
        dev_t[i] = (double)((int64_t)idx[i] + (int64_t)idx[i + 1]) / 2 / sr;
        const int64_t e = i + 1 + off, s = e - win;
        en[i] = (int32_t)(e < 0 ? 0 : (e > nd ? nd : e));
        st[i] = (int32_t)(s < 0 ? 0 : (s > nd ? nd : s));
    }
    x.sync();
    if (x.lane() == 0 && nd > 0) roll_mean(raw, st, en, nd, 1, dev);
    x.sync();
}

struct bc_cls {
    int64_t n;
    const int32_t *idx;
    const double *envpk, *str, *dev, *dev_t;
    int32_t sr;
    double thr;                                       /* pairing confidence threshold */
    bool have_rec;
    double t_pk, t_end;
};

BPMX_HD inline double bc_dev_asof(const bc_cls &c, double t) {
    const int64_t nd = c.n > 1 ? c.n - 1 : 0;
    int64_t k = bc_upper(c.dev_t, nd, t) - 1;
    while (k >= 0 && c.dev[k] != c.dev[k]) --k;
    return k >= 0 ? c.dev[k] : bc_nan();
}

/* *flags: the BPMX_TRF_* lines the attempt has (written with a trace only) */
template <class T = bc_notrace>
BPMX_HD inline bool bc_pair(const bc_cls &c, const bpmx_beat_params &p, int64_t j, double ratio, double ltb,
                            int64_t n_beats, const T &tr = T(), int32_t *flags = nullptr) {
    int32_t fl = 0;
    const int64_t s1 = c.idx[j], s2 = c.idx[j + 1];
    const int32_t sr = c.sr;
    const double gap = (double)(s2 - s1) / (double)sr;
    double conf = blended_confidence(bc_dev_asof(c, (double)s1 / (double)sr), ltb, p);
    if (T::on) { tr.put(j, BPMX_TR_BLEND, blend(ltb, p)); tr.put(j, BPMX_TR_BASE_CONF, conf); }
    if (n_beats >= 5) {
        const double xs[2] = {0.0, 1.0}, ys[2] = {p.stability_confidence_floor, p.stability_confidence_ceiling};
        const double sf = interp1(ratio, xs, ys);
        conf *= sf;
        if (T::on) { fl |= BPMX_TRF_STABILITY; tr.put(j, BPMX_TR_STAB_FACTOR, sf); tr.put(j, BPMX_TR_STAB_RATIO, ratio); }
    }
    const double a1 = c.str[j], a2 = c.str[j + 1];
    const double r21 = a2 / (a1 + 1e-9);
    const double lo = p.contractility_bpm_low;
    const double t1s = (double)s1 / (double)sr;
    const bool recovering = c.have_rec && c.t_pk < t1s && t1s < c.t_end;
    const double xs[2] = {lo, p.contractility_bpm_high}, ys[2] = {p.s2_s1_ratio_low_bpm, p.s2_s1_ratio_high_bpm};
    const double r_max = interp1(recovering ? py_max(ltb, lo) : ltb, xs, ys);
    const double boost_at = p.s1_s2_boost_ratio;
    if (r21 > r_max) {
        const double amt = p.penalty_amount_min + clipv((r21 / r_max - 1.0) / 2.0, 0, 1) *
                                                      (p.penalty_amount_max - p.penalty_amount_min);
        conf -= amt;
        if (T::on) {
            fl |= BPMX_TRF_PENALIZED;
            tr.put(j, BPMX_TR_ADJ_AMOUNT, amt); tr.put(j, BPMX_TR_ADJ_RATIO, r21); tr.put(j, BPMX_TR_ADJ_RMAX, r_max);
        }
    } else if (a1 > a2 * boost_at) {
        const double r12 = a1 / (a2 + 1e-9);
        const double amt = p.boost_amount_min + clipv((r12 - boost_at) / (4.0 - boost_at), 0, 1) *
                                                    (p.boost_amount_max - p.boost_amount_min);
        conf += amt;
        if (T::on) { fl |= BPMX_TRF_BOOSTED; tr.put(j, BPMX_TR_ADJ_AMOUNT, amt); tr.put(j, BPMX_TR_ADJ_RATIO, r12); }
    }
    conf = py_max(0.0, py_min(1.0, conf));
    const double cap = py_min(p.s1_s2_interval_cap_sec, (60.0 / ltb) * p.s1_s2_interval_rr_fraction);
    if (p.enable_interval_penalty && gap > cap) {
        const double z0 = cap * p.interval_penalty_start_factor, z1 = cap * p.interval_penalty_full_factor;
        if (gap > z0) {
            const double amt = clipv((gap - z0) / (z1 - z0 + 1e-9), 0, 1) * p.interval_max_penalty;
            conf = py_max(0, conf - amt);
            if (T::on) {
                fl |= BPMX_TRF_INTERVAL;
                tr.put(j, BPMX_TR_IV_AMOUNT, amt); tr.put(j, BPMX_TR_IV_GAP, gap); tr.put(j, BPMX_TR_IV_CAP, cap);
            }
        }
    }
    if (T::on) { tr.put(j, BPMX_TR_FINAL, conf); *flags = fl; }
    return conf >= c.thr;
}

/* (valid, rejected on rhythm) */
template <class T = bc_notrace>
BPMX_HD inline void bc_lone(const bc_cls &c, const bpmx_beat_params &p, int64_t j, int64_t jl, double ltb,
                            bool &valid, bool &on_rhythm, const T &tr = T()) {
    const double RHYTHM_X[4] = {0.0, 0.15, 0.30, 0.50}, RHYTHM_Y[4] = {1.0, 0.8, 0.4, 0.0};
    const double AMP_X[4] = {0.0, 0.4, 0.7, 1.0}, AMP_Y[4] = {0.0, 0.4, 0.8, 1.0};
    const int64_t cur = c.idx[j], last = c.idx[jl];
    const int32_t sr = c.sr;
    const double exp_rr = 60.0 / ltb;
    const double rr = (double)(cur - last) / (double)sr;
    const double rs = interp1(::fabs(rr - exp_rr) / exp_rr, RHYTHM_X, RHYTHM_Y);
    const double ar = c.str[j] / (c.str[jl] + 1e-9);
    const double am = interp1(ar, AMP_X, AMP_Y);
    const double conf = (rs * p.lone_s1_rhythm_weight) + (am * p.lone_s1_amplitude_weight);
    if (T::on) {
        tr.put(j, BPMX_TR_L_RHYTHM, rs); tr.put(j, BPMX_TR_L_RR, rr); tr.put(j, BPMX_TR_L_EXPECTED, exp_rr);
        tr.put(j, BPMX_TR_L_AMP, am); tr.put(j, BPMX_TR_L_RATIO, ar); tr.put(j, BPMX_TR_L_CONF, conf);
    }
    if (conf < p.lone_s1_confidence_threshold) { valid = false; on_rhythm = true; return; }
    on_rhythm = false;
    if (j < c.n - 1) {
        const double fwd = (double)((int64_t)c.idx[j + 1] - cur) / (double)sr;
        if (fwd < exp_rr * p.lone_s1_forward_check_pct && !(c.envpk[j] > (c.envpk[j + 1] * 1.7))) {
            valid = false;
            if (T::on) tr.put(j, BPMX_TR_L_IMPLIED, fwd > 0 ? 60.0 / fwd : (double)INFINITY);
            return;
        }
    }
    valid = true;
}

/* classify_peaks on one lane: the beats as table positions (ascending) into
 * `beats`, one tag per raw peak; returns the number of beats */
template <class T = bc_notrace>
BPMX_HD inline int64_t bc_classify(const bc_cls &c, const bpmx_beat_params &p, double start_bpm, int32_t *beats,
                                   int8_t *paired, int8_t *tag, const T &tr = T()) {
    const int64_t n = c.n;
    for (int64_t i = 0; i < n; ++i) tag[i] = BT_NONE;
    int64_t n_lt = 0;
    int32_t fl = 0;
    if (n < 2) {
        if (T::on) tr.beliefs(0);
        for (int64_t i = 0; i < n; ++i) beats[i] = (int32_t)i;
        return n;
    }
    const int64_t hist_w = p.stability_history_window;
    int64_t nb = 0, n_paired_win = 0, rr_fails = 0;
    double ltb = start_bpm;
    int64_t j = 0;
    while (j < n) {
        const double ratio = nb < hist_w ? 0.5 : (double)n_paired_win / (double)hist_w;
        int64_t add = -1;
        bool is_pair = false;
        if (j >= n - 1) {
            add = j;
            tag[j] = BT_LONE;
            if (T::on) tr.code_at(j, BPMX_TR_LAST_PEAK);
            j += 1;
        } else if (bc_pair(c, p, j, ratio, ltb, nb, tr, &fl)) {
            add = j;
            is_pair = true;
            tag[j] = BT_S1;
            tag[j + 1] = BT_S2;
            if (T::on) { tr.code_at(j, BPMX_TR_S1_PAIRED | fl); tr.code_at(j + 1, BPMX_TR_S2_PAIRED); }
            rr_fails = 0;
            j += 2;
        } else {
            bool valid = true, on_rhythm = false;
            if (nb > 0) bc_lone(c, p, j, beats[nb - 1], ltb, valid, on_rhythm, tr);
            if (valid) {
                add = j;
                tag[j] = BT_LONE;
                rr_fails = 0;
                if (T::on) tr.code_at(j, (nb > 0 ? BPMX_TR_LONE_VALID : BPMX_TR_FIRST_BEAT) | fl);
            } else {
                rr_fails = on_rhythm ? rr_fails + 1 : 0;
                const int32_t rej = on_rhythm ? 0 : BPMX_TRF_FORWARD;
                if (rr_fails >= p.cascade_reset_trigger_count) {
                    add = j;
                    tag[j] = BT_LONE;
                    rr_fails = 0;
                    if (T::on) tr.code_at(j, BPMX_TR_CASCADE | rej | fl);
                } else {
                    tag[j] = BT_NOISE;
                    if (T::on) tr.code_at(j, BPMX_TR_NOISE | rej | fl);
                }
            }
            j += 1;
        }
        if (add >= 0) {
            beats[nb] = (int32_t)add;
            paired[nb] = is_pair;
            nb++;
            n_paired_win += is_pair;
            if (nb > hist_w) {
                const int64_t q = nb - hist_w - 1;
                if (q >= 0 && q < nb) n_paired_win -= paired[q];
            }
        }
        if (nb > 1) {
            const double rr = (double)((int64_t)c.idx[beats[nb - 1]] - (int64_t)c.idx[beats[nb - 2]]) / (double)c.sr;
            if (rr > 0) ltb = update_long_term_bpm(rr, ltb, p);
        }
        if (T::on && nb > 0) { tr.belief(n_lt, beats[nb - 1], ltb); ++n_lt; }
    }
    if (T::on) tr.beliefs(n_lt);
    return nb;
}

/* ---- RR gathers and the BPM series --------------------------------------- */
/* d[i] = (idx[bt[i + 1]] - idx[bt[i]]) / sr for i < nb - 1: all lanes; ends with a sync() */
template <class X>
BPMX_HD inline void beats_rr(const X &x, const int32_t *idx, const int32_t *bt, int64_t nb, int32_t sr, double *d) {
    BPMX_PAR_FOR(x, i, nb - 1) d[i] = (double)((int64_t)idx[bt[i + 1]] - (int64_t)idx[bt[i]]) / (double)sr;
    x.sync();
}

/* beats.bpm_series: instantaneous BPM between beats, then the centred '<w>s'
 * time-window mean (min_periods 1) on the beat-time index.  bpm in S0, the
 * beat times of the kept intervals in S1, the curve in S2; returns the
 * curve's length (0: empty) and the number of beat times in *n_t. */
template <class X>
BPMX_HD inline int64_t beats_series(const X &x, const int32_t *idx, const int32_t *bt, int64_t nb, int32_t sr,
                                    double window_sec, const beats_ws &w, int64_t *n_t) {
    double *bpm = w.S[0], *t_ok = w.S[1], *curve = w.S[2];
    int64_t *ns = (int64_t *)w.S[3];
    int32_t *st = w.I[1], *en = w.I[2];
    *n_t = 0;
    if (nb < 2) return 0;
    BPMX_PAR_FOR(x, i, nb - 1) {
        const double t0 = (double)idx[bt[i]] / (double)sr, t1 = (double)idx[bt[i + 1]] / (double)sr;
        const double dt = t1 - t0;
        bpm[i] = dt > 1e-6 ? 60.0 / dt : -1.0;        /* 60 / dt is positive: -1 marks a dropped interval */
        t_ok[i] = t1;
    }
    x.sync();
    if (x.lane() == 0) {
        int64_t k = 0;
        for (int64_t i = 0; i < nb - 1; ++i)
            if (bpm[i] != -1.0) { bpm[k] = bpm[i]; t_ok[k] = t_ok[i]; ++k; }
        w.hi[BH_M] = (int32_t)k;
    }
    x.sync();
    const int64_t m = w.hi[BH_M];
    if (m == 0) return 0;
    BPMX_PAR_FOR(x, i, m) curve[i] = bpm[i];
    x.sync();
    beats_sort(x, curve, m);
    if (x.lane() == 0) w.hi[BH_OK] = median_sorted(curve, m) > 0;
    x.sync();
    *n_t = m;
    if (!w.hi[BH_OK]) return 0;                       /* the reference leaves the curve empty */
    BPMX_PAR_FOR(x, i, m) ns[i] = timedelta_us(t_ok[i]) * 1000;
    x.sync();
    if (x.lane() == 0) {
        const int64_t half = (int64_t)::llround(window_sec * 1e9) / 2;
        /* pandas calculate_variable_window_bounds, center=True, closed='right':
         * (t_i - w/2, t_i + w/2] */
        int64_t s = 0, e = 0;
        for (int64_t i = 0; i < m; ++i) {
            const int64_t lo = ns[i] - half, hi = ns[i] + half;
            while (s < i && ns[s] <= lo) ++s;
            if (e < i + 1) e = i + 1;
            while (e < m && ns[e] <= hi) ++e;
            st[i] = (int32_t)s;
            en[i] = (int32_t)e;
        }
        roll_mean(bpm, st, en, m, 1, curve);
    }
    x.sync();
    return m;
}

/* ---- refinement ---------------------------------------------------------- */
/* correct_peaks_by_rhythm on the beats in I0 (in place); returns the new count */
template <class X>
BPMX_HD inline int64_t beats_correct_by_rhythm(const X &x, int64_t ns1, const int32_t *idx, const double *env,
                                               int32_t sr, const bpmx_beat_params &p, const beats_ws &w) {
    if (ns1 < 5) return ns1;
    int32_t *bt = w.I[0];
    double *d = w.S[0];
    beats_rr(x, idx, bt, ns1, sr, d);
    beats_sort(x, d, ns1 - 1);
    if (x.lane() == 0) {
        const double thr = median_sorted(d, ns1 - 1) * p.rr_correction_threshold_pct;
        int64_t nk = 1;                               /* kept = [peaks[0]] */
        for (int64_t i = 1; i < ns1; ++i) {
            const int32_t q = bt[i], last = bt[nk - 1];
            if ((double)((int64_t)idx[q] - (int64_t)idx[last]) / (double)sr < thr) {
                if (env[q] > env[last]) bt[nk - 1] = q;
            } else {
                bt[nk++] = q;
            }
        }
        w.hi[BH_NC] = (int32_t)nk;
    }
    x.sync();
    return w.hi[BH_NC];
}

/* one gap-fill + short-interval pass over the beats in I0 (count *ns1, in
 * place); a raw peak counts as noisy when its tag is Noise (a gap correction
 * keeps it so).  Returns the number of corrections. */
template <class X, class T = bc_notrace>
BPMX_HD inline int beats_fix_discontinuities(const X &x, int64_t *ns1, int64_t n, const int32_t *idx,
                                             const double *env, const double *flo, int32_t sr,
                                             const bpmx_beat_params &p, const beats_ws &w, int it = 0,
                                             const T &tr = T()) {
    const int64_t m = 3, cnt = *ns1;
    if (cnt < 2 * m) return 0;
    int32_t *s1 = w.I[0], *added = w.I[1], *merged = w.I[2];
    double *rr = w.S[0], *srt = w.S[1];
    const int8_t *tag = w.tag;
    int8_t *mark = w.mark;
    beats_rr(x, idx, s1, cnt, sr, rr);
    BPMX_PAR_FOR(x, i, cnt - 1) srt[i] = rr[i];
    BPMX_PAR_FOR(x, i, n) mark[i] = 0;
    x.sync();
    beats_sort(x, srt, cnt - 1);
    if (x.lane() == 0) {
        int n_fix = 0;
        int64_t n_out = cnt;
        const double q1 = percentile_sorted(srt, cnt - 1, 25), q3 = percentile_sorted(srt, cnt - 1, 75);
        const double iqr = q3 - q1;
        /* the stable intervals, sorted: the sorted RR filtered in order */
        int64_t nst = 0;
        for (int64_t i = 0; i < cnt - 1; ++i) {
            const double v = srt[i];
            if (v > (q1 - 1.5 * iqr) && v < (q3 + 1.5 * iqr)) srt[nst++] = v;
        }
        if (nst > 0) {
            const double med = median_sorted(srt, nst);
            const double short_thr = med * p.rr_correction_threshold_pct;
            const double long_thr = med * p.rr_correction_long_interval_pct;
            const double waiver = p.penalty_waiver_strength_ratio, max_ratio = p.penalty_waiver_max_s2_s1_ratio;
            int64_t na = 0;
            for (int64_t i = m; i < cnt - 1 - m; ++i) {
                const int64_t ka = s1[i], kb = s1[i + 1];
                if (!((double)((int64_t)idx[kb] - (int64_t)idx[ka]) / (double)sr > long_thr)) continue;
                /* the raw peaks strictly between the two beats */
                for (int64_t k = ka + 1; k < kb; ++k) {
                    if (tag[k] != BT_NOISE || k + 1 >= n) continue;
                    if (k + 1 >= kb || tag[k + 1] != BT_NOISE) continue;
                    const double ex = env[k] - flo[k];
                    if (py_max(0, ex) > waiver * flo[k] && (env[k + 1] / (env[k] + 1e-9)) < max_ratio) {
                        n_fix += 1;
                        added[na++] = (int32_t)k;
                        if (T::on) { tr.gap_label(k, it, BPMX_TR_GAP_S1); tr.gap_label(k + 1, it, BPMX_TR_GAP_S2); }
                        break;
                    }
                }
            }
            /* sorted union of the beats and the added peaks (both ascending) */
            int64_t a = 0, b = 0, nm = 0;
            while (a < cnt || b < na) {
                int32_t v;
                if (b >= na || (a < cnt && s1[a] <= added[b])) {
                    v = s1[a++];
                    if (b < na && added[b] == v) ++b;
                } else {
                    v = added[b++];
                }
                merged[nm++] = v;
            }
            for (int64_t i = m; i < nm - 1 - m; ++i) {
                const int32_t ka = merged[i], kb = merged[i + 1];
                if (mark[ka] || mark[kb]) continue;
                if ((double)((int64_t)idx[kb] - (int64_t)idx[ka]) / (double)sr < short_thr) {
                    mark[env[kb] > env[ka] ? ka : kb] = 1;
                    n_fix += 1;
                }
            }
            n_out = 0;
            for (int64_t i = 0; i < nm; ++i)
                if (!mark[merged[i]]) s1[n_out++] = merged[i];
        }
        w.hi[BH_NFIX] = n_fix;
        w.hi[BH_NS1] = (int32_t)n_out;
    }
    x.sync();
    *ns1 = w.hi[BH_NS1];
    return w.hi[BH_NFIX];
}

/* ---- bpmx_beats over one recording's table slice ------------------------- */
/* hint: NaN = None.  Outputs as bpmx_beats': final_out[n] (samples), bpm_t /
 * bpm[n], pass_out[3] and tags_out[n] optional.  Returns BPMX_HOST_OK or
 * BPMX_HOST_E_FEW_PEAKS (every lane the same value).  The workspace `w` holds
 * beats_ws_bytes(n, .) bytes; idx / env may point into it (staged copies). */
template <class X, class T = bc_notrace>
BPMX_HD inline int beats_core(const X &x, int64_t n, const int32_t *idx, const double *env, const double *flo,
                              int32_t sr, const bpmx_beat_params &p, double hint, const beats_ws &w,
                              int32_t *final_out, int32_t *n_final, double *bpm_t_out, double *bpm_out,
                              int32_t *n_bpm, double *pass_out, int8_t *tags_out, const T &tr = T()) {
    const bool have_hint = hint == hint;
    const bool lead = x.lane() == 0;
    if (lead) { *n_final = 0; *n_bpm = 0; }
    bc_cls c;
    c.n = n; c.idx = idx; c.envpk = env; c.str = w.S[0]; c.dev = w.S[1]; c.dev_t = w.S[2]; c.sr = sr;
    /* preliminary anchor pass at pairing threshold 0.75 (:1623-1652) */
    beats_prepare(x, n, idx, env, flo, sr, p, w);
    if (lead) {
        c.thr = 0.75; c.have_rec = false; c.t_pk = 0; c.t_end = 0;
        w.hi[BH_NA] = (int32_t)bc_classify(c, p, (have_hint && hint != 0) ? hint : 80.0, w.I[0], w.paired, w.tag);
        w.hd[BH_EST] = bc_nan();
    }
    x.sync();
    const int64_t na = w.hi[BH_NA];
    if (na >= 10) {
        beats_rr(x, idx, w.I[0], na, sr, w.S[0]);
        beats_sort(x, w.S[0], na - 1);
        if (lead) {
            const double med = median_sorted(w.S[0], na - 1);
            if (med > 0) w.hd[BH_EST] = 60.0 / med;
        }
        x.sync();
    }
    int64_t n_t = 0;
    const int64_t mc = beats_series(x, idx, w.I[0], na, sr, p.output_smoothing_window_sec, w, &n_t);
    if (lead) {
        const double est = w.hd[BH_EST];
        /* start_bpm_hint or est or 80.0 (Python truthiness: 0 and None fall through) */
        const double start = (have_hint && hint != 0) ? hint : ((est == est && est != 0) ? est : 80.0);
        bool have_rec = false;
        double t_pk = bc_nan(), t_end = bc_nan();
        if (n_t >= 2) {                               /* find_recovery_phase (:1612-1620) */
            const double *curve = w.S[2];
            int64_t am = 0;                           /* numpy.argmax: the first maximum (a NaN wins) */
            for (int64_t i = 1; i < mc; ++i) {
                if (curve[am] != curve[am]) break;
                if (curve[i] != curve[i] || curve[i] > curve[am]) am = i;
            }
            t_pk = w.S[1][am];
            t_end = t_pk + p.recovery_phase_duration_sec;
            have_rec = true;
        }
        if (pass_out) { pass_out[0] = start; pass_out[1] = t_pk; pass_out[2] = t_end; }
        w.hd[BH_START] = start; w.hd[BH_TPK] = t_pk; w.hd[BH_TEND] = t_end;
        w.hi[BH_REC] = have_rec;
    }
    x.sync();
    /* main classifier */
    beats_prepare(x, n, idx, env, flo, sr, p, w);
    if (lead) {
        c.thr = p.pairing_confidence_threshold;
        c.have_rec = w.hi[BH_REC] != 0; c.t_pk = w.hd[BH_TPK]; c.t_end = w.hd[BH_TEND];
        w.hi[BH_NS1] = (int32_t)bc_classify(c, p, w.hd[BH_START], w.I[0], w.paired, w.tag, tr);
    }
    x.sync();
    if (tags_out) BPMX_PAR_FOR(x, i, n) tags_out[i] = w.tag[i];
    if (T::on && n >= 2) {                            /* before the refinement reuses S1 / S2 */
        BPMX_PAR_FOR(x, i, n - 1) tr.deviation(i, w.S[2][i], w.S[1][i]);
        BPMX_PAR_FOR(x, i, n) tr.gap_clear(i);
        x.sync();
    }
    if (n < 2) return BPMX_HOST_E_FEW_PEAKS;          /* the reference's refinement raises KeyError here */
    /* refinement (:1655-1698) */
    int64_t nf = beats_correct_by_rhythm(x, w.hi[BH_NS1], idx, env, sr, p, w);
    for (int it = 0; it < 5; ++it)
        if (beats_fix_discontinuities(x, &nf, n, idx, env, flo, sr, p, w, it, tr) == 0) break;
    BPMX_PAR_FOR(x, i, nf) final_out[i] = idx[w.I[0][i]];
    if (lead) *n_final = (int32_t)nf;
    /* final BPM curve (:1463-1484), only when >= 2 beats survive (:1749-1757) */
    if (nf >= 2) {
        const int64_t m2 = beats_series(x, idx, w.I[0], nf, sr, p.output_smoothing_window_sec, w, &n_t);
        BPMX_PAR_FOR(x, i, m2) { bpm_t_out[i] = w.S[1][i]; bpm_out[i] = w.S[2][i]; }
        if (lead) *n_bpm = (int32_t)m2;
    }
    return BPMX_HOST_OK;
}

}  // namespace bpmx

#endif
