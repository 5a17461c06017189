/*
 * bpmx_tempo_core.h — the decisions of the tempogram (bpmx_tempo_device),
 * stated once for host and device.  There is no reference implementation:
 * include/bpmx.h is the definition, bpm_analysis_amd/tempo.py (tempogram) the
 * same in numpy.  The lag sums themselves (mean removal, padding, r[k]) are
 * the kernel's arithmetic (k_tempo.hip); what must not differ between two
 * statements is here:
 *
 *   tempo_scan     step 1: a window is invalid if a sample is not finite or
 *                  max == min; exact tests on the inputs, merged in any order
 *   tempo_pick     step 4: the candidates k in [kmin, kmax] with r[k] > r[k-1]
 *                  and r[k] >= r[k+1], the largest r[k], the smallest k among
 *                  equals
 *   tempo_outputs  steps 5 and 6: rho, the parabolic offset, bpm; lag 0,
 *                  rho 0.0, bpm NaN for an invalid window
 *   tempo_record   per recording: counts, the median of the strong windows'
 *                  bpm by rank counting (any window count), the mean of rho,
 *                  the hint
 *   tempo_plan     the kernel's geometry and its limit
 *
 * Same pattern as the other cores: BPMX_HD functions over an executor with
 * lane(), width() and sync(), no allocation, caller-supplied workspaces.
 * Every call must be made by all lanes with the same arguments.
 */
#ifndef BPMX_TEMPO_CORE_H
#define BPMX_TEMPO_CORE_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/bpmx.h"

#if defined(__HIPCC__)
#define BPMX_HD __host__ __device__
#else
#define BPMX_HD
#endif

namespace bpmx {

/* ---- geometry ------------------------------------------------------------ */
enum {
    TEMPO_T = 256,              /* threads of a window's workgroup: four waves, each a quarter of the window */
    TEMPO_WAVES = TEMPO_T / 64,
    TEMPO_U = 4,                /* window samples per step of the lag loop */
    TEMPO_PAD = 8,              /* zeros behind win4 + kmax: the most lags a lane holds */
    TEMPO_LDS_MAX = 152 * 1024, /* dynamic LDS of a workgroup: a CU's 160 KB less the static arrays (one pick
                                   per thread, the scans and sums of the waves: under 5 KB) */
    TEMPO_REC_T = 64            /* one wave per recording makes the record */
};

struct TempoPlan {
    int32_t status;             /* BPMX_OK, BPMX_E_ARG or BPMX_E_LIMIT */
    int32_t nlag;               /* kmax - kmin + 3: the lags kmin - 1 .. kmax + 1 */
    int32_t lags;               /* consecutive lags per lane: 5 or 7, the fewest idle lanes (odd, so that the
                                   lanes' 8-byte LDS reads at a stride of `lags` doubles fall on distinct banks) */
    int32_t win4;               /* win rounded up to TEMPO_U */
    int32_t chunk;              /* window samples per wave, a multiple of TEMPO_U */
    int32_t elen;               /* doubles of the padded window */
    int32_t pstride;            /* doubles of one wave's partial sums */
    size_t lds;                 /* bytes: the padded window, then TEMPO_WAVES partial sums per lag */
};

BPMX_HD inline TempoPlan tempo_plan(int32_t win, int32_t hop, int32_t kmin, int32_t kmax) {
    TempoPlan P{};
    P.status = BPMX_E_ARG;
    if (hop < 1 || kmin < 2 || kmax < kmin || win < 1 || (int64_t)kmax + 1 >= (int64_t)win) return P;
    P.status = BPMX_E_LIMIT;
    const int64_t nlag = (int64_t)kmax - kmin + 3;
    const int64_t win4 = ((int64_t)win + TEMPO_U - 1) / TEMPO_U * TEMPO_U;
    const int64_t elen = win4 + kmax + TEMPO_PAD, pstride = nlag + 1;
    const int64_t bytes = 8 * (elen + TEMPO_WAVES * pstride);
    if (bytes > (int64_t)TEMPO_LDS_MAX) return P;
    P.status = BPMX_OK;
    P.nlag = (int32_t)nlag;
    int32_t best = 0, cost = 0;
    for (int32_t l = 5; l <= 7; l += 2) {
        const int32_t c = (int32_t)((nlag + 64 * l - 1) / (64 * l)) * l;
        if (best == 0 || c <= cost) { best = l; cost = c; }
    }
    P.lags = best;
    P.win4 = (int32_t)win4;
    P.chunk = (int32_t)(((win4 / TEMPO_U + TEMPO_WAVES - 1) / TEMPO_WAVES) * TEMPO_U);
    P.elen = (int32_t)elen;
    P.pstride = (int32_t)pstride;
    P.lds = (size_t)bytes;
    return P;
}

BPMX_HD inline int64_t tempo_windows(int64_t nd, int32_t win, int32_t hop) {
    if (win < 1 || hop < 1 || nd < win) return 0;
    return (nd - win) / hop + 1;
}

/* ---- step 1 -------------------------------------------------------------- */
BPMX_HD inline double tp_nan() { return __builtin_nan(""); }
BPMX_HD inline bool tp_finite(double v) {
    uint64_t b;
    __builtin_memcpy(&b, &v, 8);
    return (b & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

struct tempo_scan {
    double mn, mx;
    int32_t bad;                /* a sample that is not finite */
};
BPMX_HD inline tempo_scan tempo_scan_init() { return tempo_scan{__builtin_inf(), -__builtin_inf(), 0}; }
BPMX_HD inline void tempo_scan_add(tempo_scan &s, double v) {
    if (!tp_finite(v)) { s.bad = 1; return; }
    s.mn = v < s.mn ? v : s.mn;
    s.mx = v > s.mx ? v : s.mx;
}
BPMX_HD inline void tempo_scan_merge(tempo_scan &a, const tempo_scan &b) {
    a.bad |= b.bad;
    a.mn = b.mn < a.mn ? b.mn : a.mn;
    a.mx = b.mx > a.mx ? b.mx : a.mx;
}
BPMX_HD inline bool tempo_scan_valid(const tempo_scan &s) { return !s.bad && s.mx != s.mn; }

/* ---- step 4 -------------------------------------------------------------- */
struct tempo_best {
    double r;
    int32_t k;                  /* 0: no candidate */
    int32_t pad;
};
BPMX_HD inline void tempo_best_take(tempo_best &b, double r, int32_t k) {
    if (b.k == 0 || r > b.r || (r == b.r && k < b.k)) { b.r = r; b.k = k; }
}
/* r[j] is the sum of lag kmin - 1 + j, j in [0, kmax - kmin + 3).  ws holds
 * width() entries.  Every lane returns the same pick. */
template <class X>
BPMX_HD inline tempo_best tempo_pick(const X &x, const double *r, int32_t kmin, int32_t kmax, tempo_best *ws) {
    tempo_best b{0.0, 0, 0};
    const int64_t n = (int64_t)kmax - kmin + 1;
    for (int64_t j = x.lane(); j < n; j += x.width()) {
        const double rm = r[j], rk = r[j + 1], rp = r[j + 2];
        if (rk > rm && rk >= rp) tempo_best_take(b, rk, (int32_t)(kmin + j));
    }
    ws[x.lane()] = b;
    x.sync();
    int top = 1;
    while (top < x.width()) top <<= 1;
    for (int s = top >> 1; s > 0; s >>= 1) {    /* the rule is a total order on (r, k): any tree gives the same pick */
        if (x.lane() < s && x.lane() + s < x.width()) {
            const tempo_best o = ws[x.lane() + s];
            if (o.k != 0) tempo_best_take(b, o.r, o.k);
            ws[x.lane()] = b;
        }
        x.sync();
    }
    b = ws[0];
    x.sync();
    return b;
}

/* ---- steps 5 and 6 --------------------------------------------------------- */
struct tempo_val {
    int32_t lag;
    double rho, bpm;
};
/* k = 0: an invalid window; rm, rk, rp = r[k - 1], r[k], r[k + 1] */
BPMX_HD inline tempo_val tempo_outputs(int32_t k, double rm, double rk, double rp, double r0, int32_t sr) {
    if (k == 0) return tempo_val{0, 0.0, tp_nan()};
    const double d = rm - 2.0 * rk + rp;        /* strictly negative at a candidate */
    const double delta = 0.5 * (rm - rp) / d;
    return tempo_val{k, rk / r0, 60.0 * (double)sr / ((double)k + delta)};
}

/* ---- the record of a recording ------------------------------------------- */
struct tempo_rec_ws {
    double *sum;                /* [width] */
    int32_t *nv, *ns;           /* [width] */
    double *mid;                /* [2] */
};
BPMX_HD constexpr size_t tempo_rec_ws_bytes(int lanes) { return (size_t)lanes * 16 + 16; }
/* base: 8-byte aligned, tempo_rec_ws_bytes(lanes) bytes */
BPMX_HD inline tempo_rec_ws tempo_rec_ws_layout(void *base, int lanes) {
    tempo_rec_ws w;
    w.sum = (double *)base;
    w.mid = w.sum + lanes;
    w.nv = (int32_t *)(w.mid + 2);
    w.ns = w.nv + lanes;
    return w;
}
struct tempo_rec {
    int32_t *n_valid, *n_strong;
    double *median_bpm, *mean_rho, *hint;
};
BPMX_HD inline bool tempo_strong(int32_t lag, double rho, double min_strength) { return lag != 0 && rho >= min_strength; }

/* nw windows (lag, rho, bpm as tempo_outputs wrote them).  The median is
 * numpy's: the strong window of rank (ns - 1) / 2 in the order (bpm, window),
 * averaged with the one of rank ns / 2. */
template <class X>
BPMX_HD inline void tempo_record(const X &x, int64_t nw, const int32_t *lag, const double *rho, const double *bpm,
                                 double min_strength, int32_t start_windows, const tempo_rec_ws &w,
                                 const tempo_rec &o) {
    const int me = x.lane();
    {
        double s = 0.0;
        int32_t nv = 0, ns = 0;
        for (int64_t i = me; i < nw; i += x.width()) {
            if (lag[i] == 0) continue;
            ++nv;
            s += rho[i];
            ns += tempo_strong(lag[i], rho[i], min_strength) ? 1 : 0;
        }
        w.sum[me] = s; w.nv[me] = nv; w.ns[me] = ns;
    }
    x.sync();
    int64_t nv = 0, ns = 0;
    for (int l = 0; l < x.width(); ++l) { nv += w.nv[l]; ns += w.ns[l]; }
    const int64_t lo = (ns - 1) / 2, hi = ns / 2;
    for (int64_t i = me; i < nw; i += x.width()) {
        if (!tempo_strong(lag[i], rho[i], min_strength)) continue;
        const double v = bpm[i];
        int64_t rank = 0;
        for (int64_t j = 0; j < nw; ++j) {
            if (!tempo_strong(lag[j], rho[j], min_strength)) continue;
            const double u = bpm[j];
            rank += (u < v || (u == v && j < i)) ? 1 : 0;
        }
        if (rank == lo) w.mid[0] = v;
        if (rank == hi) w.mid[1] = v;
    }
    x.sync();
    if (me == 0) {
        double s = 0.0;
        for (int l = 0; l < x.width(); ++l) s += w.sum[l];
        double hint = tp_nan();
        for (int64_t i = 0; i < nw && i < (int64_t)start_windows; ++i)
            if (tempo_strong(lag[i], rho[i], min_strength)) { hint = bpm[i]; break; }
        *o.n_valid = (int32_t)nv;
        *o.n_strong = (int32_t)ns;
        *o.mean_rho = nv > 0 ? s / (double)nv : tp_nan();
        *o.median_bpm = ns > 0 ? (lo == hi ? w.mid[0] : (w.mid[0] + w.mid[1]) / 2.0) : tp_nan();
        *o.hint = hint;
    }
    x.sync();
}

}  // namespace bpmx

#endif
