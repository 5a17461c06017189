/*
 * bpmx_hrvspec_core.h — the per-window arithmetic of the HRV spectrum
 * (bpmx_hrvspec_device), stated once for host and device.  There is no
 * reference implementation: include/bpmx.h is the definition,
 * bpm_analysis_amd/hrv_spectrum.py (spectrum_ints) the same in numpy.
 *
 *   hrvspec_plan     the argument checks, the most intervals of a window and
 *                    the LDS they need
 *   hrvspec_stage    a window's kept intervals from the beats, in order: the
 *                    span by bisection, the compaction, the code, the centred
 *                    values u_j, the times s_j and the grid step's rotation
 *                    (cos, sin)(dom * s_j)
 *   hrvspec_accum    the six sums of B consecutive frequencies over a slice of
 *                    the intervals: one sincos per term (ROT false), or one
 *                    per interval and a rotation along the grid (ROT true)
 *   hrvspec_power    q from the six sums: the floating-mean terms, tau removed
 *                    by rotating the sums, the clamp at 2^-53
 *   hrvspec_band     a band's sum and its peak, the smallest index among equals
 *   hrvspec_record   the 8 doubles of a recording, added in window order
 *
 * Which lane owns which frequencies and which slice of the intervals is the
 * caller's (k_hrvspec.hip; tests/hrvspec_core_driver.cpp).  Same pattern as
 * the other cores: BPMX_HD functions over an executor with lane(), width(),
 * sync() and count(flag, ws) (how many lanes before this one set flag, and in
 * all), no allocation, caller-supplied workspaces.  Every call must be made by
 * all lanes with the same arguments.
 */
#ifndef BPMX_HRVSPEC_CORE_H
#define BPMX_HRVSPEC_CORE_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/bpmx.h"

#if defined(__HIPCC__)
#define BPMX_HD __host__ __device__
#else
#define BPMX_HD
#endif
#if defined(__clang__)
#define HS_UNROLL _Pragma("unroll")
#else
#define HS_UNROLL
#endif

namespace bpmx {

enum {
    HRVSPEC_T = 256,            /* threads of a window's workgroup */
    HRVSPEC_B = 8,              /* consecutive frequencies a lane rotates through from one sincos */
    HRVSPEC_PARTS = 8,          /* adjacent lanes that share a block and split the intervals */
    HRVSPEC_MAX_FREQ = 1024,
    HRVSPEC_PER = 32,           /* LDS bytes per kept interval: s, u, cos and sin of dom * s */
    HRVSPEC_LDS_MAX = 48 * 1024, /* dynamic LDS of a workgroup: 64 KB less the static arrays (q of 1024
                                   frequencies, one sum, count and pick per thread: 15 KB) */
    HRVSPEC_REC_T = 64          /* one wave per recording makes the record */
};

struct HrvspecPlan {
    int32_t status;             /* BPMX_OK, BPMX_E_ARG or BPMX_E_LIMIT */
    int32_t nmax;               /* win / dmin + 1: the most kept intervals of a window */
    size_t lds;                 /* bytes: HRVSPEC_PER * nmax */
};

BPMX_HD inline bool hs_finite(double v) {
    uint64_t b;
    __builtin_memcpy(&b, &v, 8);
    return (b & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}
BPMX_HD inline double hs_nan() { return __builtin_nan(""); }

BPMX_HD inline HrvspecPlan hrvspec_plan(const bpmx_hrvspec_params &P) {
    HrvspecPlan G{};
    G.status = BPMX_E_ARG;
    if (P.hop < 1 || P.dmin < 1 || P.dmax < P.dmin || P.min_intervals < 3 || P.n_freq < 1 ||
        P.n_freq > (int32_t)HRVSPEC_MAX_FREQ)
        return G;
    if (P.lf_a < 0 || P.lf_b < P.lf_a || P.lf_b > P.n_freq || P.hf_a < 0 || P.hf_b < P.hf_a || P.hf_b > P.n_freq)
        return G;
    if (!hs_finite(P.om0) || !hs_finite(P.dom) || !(P.om0 > 0.0) || !(P.dom >= 0.0)) return G;
    G.status = BPMX_E_LIMIT;
    const int64_t nmax = P.win < 1 ? 1 : (int64_t)P.win / P.dmin + 1;
    if (nmax * (int64_t)HRVSPEC_PER > (int64_t)HRVSPEC_LDS_MAX) return G;
    G.status = BPMX_OK;
    G.nmax = (int32_t)nmax;
    G.lds = (size_t)nmax * HRVSPEC_PER;
    return G;
}

BPMX_HD inline int64_t hrvspec_windows(int64_t nd, int32_t win, int32_t hop) {
    if (nd <= 0 || win < 1 || hop < 1) return 0;
    if (nd <= (int64_t)win) return 1;
    return (nd - win) / hop + 1;
}

BPMX_HD inline void hs_sincos(double a, double *s, double *c) {
#if defined(__HIP_DEVICE_COMPILE__)
    ::sincos(a, s, c);
#else
    *s = ::sin(a);
    *c = ::cos(a);
#endif
}

/* ---- workspaces ------------------------------------------------------------ */
struct hrvspec_pick {
    double q;
    int32_t m;                  /* -1: none */
    int32_t pad;
};
struct hrvspec_ws {
    double *s, *u, *cd, *sd;    /* [nmax] each: HRVSPEC_PER bytes per interval */
    double *dw;                 /* [width] */
    int32_t *iw;                /* [width] */
    hrvspec_pick *pk;           /* [width] */
};
BPMX_HD inline void hrvspec_ws_intervals(hrvspec_ws &w, void *base, int32_t nmax) {
    w.s = (double *)base;
    w.u = w.s + nmax;
    w.cd = w.u + nmax;
    w.sd = w.cd + nmax;
}

/* the sum of v over the lanes by a tree, the same value in every lane */
template <class X>
BPMX_HD inline double hrvspec_sum(const X &x, double v, double *dw) {
    dw[x.lane()] = v;
    x.sync();
    int top = 1;
    while (top < x.width()) top <<= 1;
    for (int st = top >> 1; st > 0; st >>= 1) {
        if (x.lane() < st && x.lane() + st < x.width()) dw[x.lane()] += dw[x.lane() + st];
        x.sync();
    }
    const double r = dw[0];
    x.sync();
    return r;
}

/* first k in [0, n) with idx[k] >= v, n with none */
BPMX_HD inline int64_t hs_lower(const int32_t *idx, int64_t n, int64_t v) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)idx[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

/* ---- a window's intervals --------------------------------------------------- */
struct hrvspec_head {
    int32_t n, code;
    double e_first, e_last;     /* exact integers */
    double t_mid, var, Y, YY;   /* var = sum w u^2, Y = sum w u, YY = var - Y^2 */
};

/* idx[0 .. nf): the recording's final beats (nf < 2: no interval); the window
 * is [lo, lo + win).  Leaves s, u (and cd, sd with `rot`) of a valid window in
 * w; at most nmax intervals are staged. */
template <class X>
BPMX_HD inline hrvspec_head hrvspec_stage(const X &x, const int32_t *idx, int64_t nf, int64_t lo,
                                          const bpmx_hrvspec_params &P, int32_t sr, int32_t nmax, bool rot,
                                          const hrvspec_ws &w) {
    hrvspec_head H{};
    const int64_t hi = lo + P.win;
    int64_t k0 = 1, k1 = 1;
    if (nf >= 2) {
        k0 = hs_lower(idx, nf, lo);
        k1 = hs_lower(idx, nf, hi);
        if (k0 < 1) k0 = 1;
    }
    int32_t n = 0;
    for (int64_t base = k0; base < k1; base += x.width()) {
        const int64_t k = base + x.lane();
        int64_t d = 0, e = 0;
        int keep = 0;
        if (k < k1) {
            e = idx[k];
            d = e - (int64_t)idx[k - 1];
            keep = (d >= P.dmin && d <= P.dmax && e >= lo && e < hi) ? 1 : 0;
        }
        int total = 0;
        const int pos = n + x.count(keep, w.iw, &total);
        if (keep && pos < nmax) {
            w.s[pos] = (double)e;
            w.u[pos] = (double)d * 1000.0 / (double)sr;
        }
        n += total;
    }
    if (n > nmax) n = nmax;
    x.sync();
    H.n = n;
    H.t_mid = H.var = H.Y = H.YY = hs_nan();
    if (n > 0) {
        H.e_first = w.s[0];
        H.e_last = w.s[n - 1];
        H.t_mid = (H.e_first + H.e_last) / (2.0 * (double)sr);
    }
    H.code = 0;
    if (n < P.min_intervals) {
        H.code = 1;
    } else if (H.e_last - H.e_first < (double)P.min_span) {
        H.code = 2;
    } else {
        int differs = 0;
        const double y0 = w.u[0];
        for (int j = x.lane(); j < n; j += x.width()) differs |= (w.u[j] != y0) ? 1 : 0;
        int total = 0;
        (void)x.count(differs, w.iw, &total);
        if (total == 0) H.code = 3;
    }
    if (H.code != 0) {
        x.sync();
        return H;
    }
    const double dn = (double)n;
    double a = 0.0;
    for (int j = x.lane(); j < n; j += x.width()) a += w.u[j];
    const double my = hrvspec_sum(x, a, w.dw) / dn;
    double su = 0.0, sq = 0.0;
    for (int j = x.lane(); j < n; j += x.width()) {
        const double u = w.u[j] - my, s = w.s[j] - H.e_first;
        w.u[j] = u;
        w.s[j] = s;
        su += u;
        sq = __builtin_fma(u, u, sq);
        if (rot) hs_sincos(P.dom * s, &w.sd[j], &w.cd[j]);
    }
    H.Y = hrvspec_sum(x, su, w.dw) / dn;
    H.var = hrvspec_sum(x, sq, w.dw) / dn;
    H.YY = H.var - H.Y * H.Y;
    return H;                   /* hrvspec_sum's barriers order the writes of w before the reads that follow */
}

/* ---- the six sums ------------------------------------------------------------ */
enum { HS_C = 0, HS_S, HS_CC, HS_CS, HS_YC, HS_YS, HS_NSUM };

/* adds the intervals j0, j0 + step, ... < n to acc[HS_NSUM][B] for the
 * frequencies m0 .. m0 + B - 1 */
template <int B, bool ROT>
BPMX_HD inline void hrvspec_accum(const hrvspec_ws &w, int32_t n, int32_t j0, int32_t step, int32_t m0,
                                  const bpmx_hrvspec_params &P, double (*acc)[B]) {
    double om[B];
    HS_UNROLL
    for (int k = 0; k < B; ++k) om[k] = P.om0 + (double)(m0 + k) * P.dom;
    for (int32_t j = j0; j < n; j += step) {
        const double s = w.s[j], u = w.u[j];
        double c = 0.0, sn = 0.0, cd = 0.0, sd = 0.0;
        if (ROT) {
            hs_sincos(om[0] * s, &sn, &c);
            cd = w.cd[j];
            sd = w.sd[j];
        }
        HS_UNROLL
        for (int k = 0; k < B; ++k) {
            if (!ROT) {
                hs_sincos(om[k] * s, &sn, &c);
            } else if (k > 0) {
                const double c2 = __builtin_fma(c, cd, -(sn * sd)), s2 = __builtin_fma(sn, cd, c * sd);
                c = c2;
                sn = s2;
            }
            acc[HS_C][k] += c;
            acc[HS_S][k] += sn;
            acc[HS_CC][k] = __builtin_fma(c, c, acc[HS_CC][k]);
            acc[HS_CS][k] = __builtin_fma(c, sn, acc[HS_CS][k]);
            acc[HS_YC][k] = __builtin_fma(u, c, acc[HS_YC][k]);
            acc[HS_YS][k] = __builtin_fma(u, sn, acc[HS_YS][k]);
        }
    }
}

/* q of one frequency from its six sums over all n intervals */
BPMX_HD inline double hrvspec_power(const double *sum, int32_t n, double Y, double YY) {
    const double dn = (double)n;
    const double C = sum[HS_C] / dn, S = sum[HS_S] / dn, CC0 = sum[HS_CC] / dn;
    const double CC = CC0 - C * C, SS = (1.0 - CC0) - S * S, CS = sum[HS_CS] / dn - C * S;
    const double YC = sum[HS_YC] / dn - Y * C, YS = sum[HS_YS] / dn - Y * S;
    const double tau = 0.5 * ::atan2(2.0 * CS, CC - SS);
    double st, ct;
    hs_sincos(tau, &st, &ct);
    const double YCt = YC * ct + YS * st, YSt = YS * ct - YC * st;
    const double xx = 2.0 * CS * ct * st, eps = 0x1p-53;
    double CCt = CC * ct * ct + xx + SS * st * st, SSt = SS * ct * ct - xx + CC * st * st;
    CCt = CCt < eps ? eps : CCt;
    SSt = SSt < eps ? eps : SSt;
    return (YCt * YCt / CCt + YSt * YSt / SSt) / YY;
}

/* ---- bands -------------------------------------------------------------------- */
struct hrvspec_bandval {
    double sum;
    int32_t peak;
};
BPMX_HD inline void hrvspec_pick_take(hrvspec_pick &b, double q, int32_t m) {
    if (m >= 0 && (b.m < 0 || q > b.q || (q == b.q && m < b.m))) { b.q = q; b.m = m; }
}
/* q[a .. b): the sum by lane-strided partials and a tree, the peak by the
 * total order on (q, index), so any tree gives the same pick */
template <class X>
BPMX_HD inline hrvspec_bandval hrvspec_band(const X &x, const double *q, int32_t a, int32_t b, const hrvspec_ws &w) {
    hrvspec_pick p{0.0, -1, 0};
    double s = 0.0;
    for (int32_t m = a + x.lane(); m < b; m += x.width()) {
        s += q[m];
        hrvspec_pick_take(p, q[m], m);
    }
    hrvspec_bandval r;
    r.sum = hrvspec_sum(x, s, w.dw);
    w.pk[x.lane()] = p;
    x.sync();
    int top = 1;
    while (top < x.width()) top <<= 1;
    for (int st = top >> 1; st > 0; st >>= 1) {
        if (x.lane() < st && x.lane() + st < x.width()) {
            const hrvspec_pick o = w.pk[x.lane() + st];
            hrvspec_pick_take(p, o.q, o.m);
            w.pk[x.lane()] = p;
        }
        x.sync();
    }
    r.peak = w.pk[0].m;
    x.sync();
    if (b <= a) r.sum = 0.0;
    return r;
}

/* ---- the record of a recording -------------------------------------------------- */
/* nw windows as the window stage wrote them; st: [3 * width] doubles.  The
 * lanes stage width() windows at a time, lane 0 adds them in window order. */
template <class X>
BPMX_HD inline void hrvspec_record(const X &x, int64_t nw, const int32_t *code, const double *lf, const double *hf,
                                   double *st, double *rec) {
    double s_lf = 0.0, s_hf = 0.0, s_r = 0.0, s_n = 0.0;
    int64_t nv = 0, n_r = 0, n_n = 0;
    const int W = x.width();
    for (int64_t base = 0; base < nw; base += W) {
        const int64_t i = base + x.lane();
        if (i < nw) {
            st[x.lane()] = code[i] == 0 ? 1.0 : 0.0;
            st[W + x.lane()] = lf[i];
            st[2 * W + x.lane()] = hf[i];
        }
        x.sync();
        if (x.lane() == 0) {
            const int64_t m = nw - base < W ? nw - base : W;
            for (int64_t k = 0; k < m; ++k) {
                if (st[k] == 0.0) continue;
                const double a = st[W + k], b = st[2 * W + k];
                ++nv;
                s_lf += a;
                s_hf += b;
                if (b > 0.0) { s_r += a / b; ++n_r; }
                if (a + b > 0.0) { s_n += a / (a + b); ++n_n; }
            }
        }
        x.sync();
    }
    if (x.lane() == 0) {
        rec[0] = (double)nv;
        rec[1] = nv > 0 ? s_lf / (double)nv : hs_nan();
        rec[2] = nv > 0 ? s_hf / (double)nv : hs_nan();
        rec[3] = n_r > 0 ? s_r / (double)n_r : hs_nan();
        rec[4] = n_n > 0 ? s_n / (double)n_n : hs_nan();
        rec[5] = rec[6] = rec[7] = hs_nan();
    }
    x.sync();
}

}  // namespace bpmx

#endif
