/*
 * bpmx_metrics_core.h — the final metrics (bpm_analysis.py:1701-1722
 * _calculate_final_metrics with :1414-1461 and :1486-1610: the windowed HRV
 * table, the summary, heart-rate recovery, the steepest recovery and exertion
 * slopes, the major inclines and declines) stated once for host and device.
 *
 * It restates beats.final_metrics and its helpers in the same IEEE operation
 * order, over what bpmx_beats_core.h leaves: the final beats as sample indices
 * and the smoothed BPM curve (bpm_t, bpm).  Results are curve positions,
 * counts and doubles; the host turns positions into timestamps by indexing.
 *
 * Same pattern as the beats core: BPMX_HD functions over an executor with
 * lane(), width() and sync(), no allocation, a caller-supplied workspace
 * (metrics_ws_bytes / metrics_ws_layout).  Parallel over all lanes: the index
 * times, one HRV window per lane, the minimum / maximum of the curve, one
 * start of the steepest-slope search per lane, the extrema scan, the ranks
 * behind the distance filter's visiting order, the prominence walks, the tie
 * test, the run pairing and the runs' stable sort (by rank).  Serial on lane
 * 0: the pairwise sums of the summary (numpy's summation tree), the HRR
 * interpolation, the compactions and the greedy distance filter.  Scalars a
 * serial part decides travel through the workspace header and are read after
 * a sync().  Every call must be made by all lanes with the same arguments.
 *
 * Sums are numpy's pairwise sum (numpy/_core/src/umath/loops_utils.h.src):
 * fewer than 8 elements left to right, up to 128 eight accumulators, beyond
 * that split at n/2 rounded down to a multiple of 8.  The recursion is an
 * explicit stack of pw_frame in the workspace, so the device needs neither
 * calls nor a run-time-indexed local array.
 */
#ifndef BPMX_METRICS_CORE_H
#define BPMX_METRICS_CORE_H

#include "bpmx_beats_core.h"
#include "../../include/bpmx.h"

namespace bpmx {

/* ---- pairwise sum -------------------------------------------------------- */
struct pw_frame {
    double acc;                  /* the left half's sum while the right half runs */
    int32_t off, n, state, pad;  /* state 0: new, 1: left half running, 2: right half running */
};

/* Frames that hold the stack of a sum of n elements (0: n <= 128, no stack);
 * non-decreasing in n.  A half has at most n/2 + 8 elements, so after k
 * levels a node has at most n/2^k + 16 and is a leaf once n/2^k <= 112: the
 * deepest path has at most ceil(log2(n/112)) + 1 nodes.  (The exact depth is
 * not monotone in n: 255 splits into 120 + 135, 256 into 128 + 128.) */
BPMX_HD constexpr int pw_frames(int64_t n) {
    if (n <= 128) return 0;
    int d = 2;
    for (int64_t q = (n + 111) / 112; q > 1; q = (q + 1) / 2) ++d;
    return d;
}
enum { MX_PW_DEPTH = 28 };       /* >= pw_frames(2^31) */
static_assert(pw_frames((int64_t)1 << 31) <= MX_PW_DEPTH, "stack of lane 0's sums");

template <class F>
BPMX_HD inline double pw_leaf(const F &f, int64_t off, int64_t n) {
    if (n < 8) {
        double r = 0.;
        for (int64_t i = 0; i < n; ++i) r += f(off + i);
        return r;
    }
    double r0 = f(off), r1 = f(off + 1), r2 = f(off + 2), r3 = f(off + 3);
    double r4 = f(off + 4), r5 = f(off + 5), r6 = f(off + 6), r7 = f(off + 7);
    int64_t i = 8;
    for (; i < n - (n % 8); i += 8) {
        r0 += f(off + i);     r1 += f(off + i + 1); r2 += f(off + i + 2); r3 += f(off + i + 3);
        r4 += f(off + i + 4); r5 += f(off + i + 5); r6 += f(off + i + 6); r7 += f(off + i + 7);
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) res += f(off + i);
    return res;
}

/* sum of f(0) .. f(n-1); stk holds pw_frames(n) frames (unused for n <= 128) */
template <class F>
BPMX_HD inline double pw_sum(const F &f, int64_t n, pw_frame *stk) {
    if (n <= 128) return pw_leaf(f, 0, n);
    int sp = 1;
    stk[0].off = 0; stk[0].n = (int32_t)n; stk[0].state = 0;
    for (;;) {
        pw_frame &t = stk[sp - 1];
        if (t.n > 128) {         /* descend into the left half */
            int32_t n2 = t.n / 2;
            n2 -= n2 % 8;
            t.state = 1;
            stk[sp].off = t.off; stk[sp].n = n2; stk[sp].state = 0;
            ++sp;
            continue;
        }
        double r = pw_leaf(f, t.off, t.n);
        --sp;
        for (;;) {               /* hand r to the parents */
            if (sp == 0) return r;
            pw_frame &p = stk[sp - 1];
            if (p.state == 1) {
                int32_t n2 = p.n / 2;
                n2 -= n2 % 8;
                p.acc = r;
                p.state = 2;
                stk[sp].off = p.off + n2; stk[sp].n = p.n - n2; stk[sp].state = 0;
                ++sp;
                break;
            }
            r = p.acc + r;
            --sp;
        }
    }
}

/* ---- workspace ----------------------------------------------------------- */
enum {
    MX_HDR = 256,                /* 16 doubles, 32 int32 */
    MX_LANE = 24,                /* per lane: two doubles, two int32 */
    MX_PER = 8 + 8 + 8 + 5 * 4 + 2,   /* ns, rs, rd; c1, c2, ord, ra, rb; keep, fl */
    MX_STAGE = 8 + 4,            /* a copy of the curve and of the beats in front (the LDS path) */
    MX_STRIDE = 48               /* a global slice: metrics_ws_fixed + MX_STRIDE * pk_off[f] */
};
enum { MH_AVG = 0, MH_MIN, MH_MAX, MH_A, MH_B, MH_SLOPE, MH_DUR };                  /* hd */
enum { MI_AM = 0, MI_FOUND, MI_NC, MI_TIE, MI_NP, MI_NT, MI_NRUN, MI_DIST };        /* hi */

BPMX_HD constexpr size_t metrics_ws_head(int lanes, int fw) {
    return (size_t)MX_HDR + (size_t)lanes * MX_LANE + ((size_t)MX_PW_DEPTH + (size_t)lanes * (size_t)fw) * sizeof(pw_frame);
}
/* lanes: the executor's width; fw: pw_frames(hrv window), the stack each lane's window sums need */
BPMX_HD constexpr size_t metrics_ws_bytes(int64_t n, int lanes, int fw, bool stage) {
    return metrics_ws_head(lanes, fw) + (size_t)beats_n8(n) * (size_t)(MX_PER + (stage ? MX_STAGE : 0));
}
BPMX_HD constexpr size_t metrics_ws_fixed(int lanes, int fw) { return metrics_ws_head(lanes, fw) + 8 * MX_STRIDE; }
BPMX_HD constexpr int64_t metrics_ws_max_n(size_t budget, int lanes, int fw) {
    return budget < metrics_ws_head(lanes, fw)
               ? 0
               : (int64_t)((budget - metrics_ws_head(lanes, fw)) / (MX_PER + MX_STAGE)) & ~(int64_t)7;
}

struct metrics_ws {
    double *hd;
    int32_t *hi;
    double *ld, *ld2;            /* per lane */
    int32_t *li, *li2;
    pw_frame *stk0, *stkL;       /* lane 0's sums; fw frames per lane */
    int fw;
    int64_t *ns;                 /* the curve's index in ns since 1970 */
    double *rs, *rd;             /* unsorted runs: slope, duration */
    int32_t *c1, *c2, *ord, *ra, *rb;   /* maxima, minima (curve positions); visiting order; runs' ends */
    int8_t *keep, *fl;
    double *v_stage;             /* stage only */
    int32_t *fin_stage;
};

/* base must be 8-byte aligned */
BPMX_HD inline metrics_ws metrics_ws_layout(void *base, int64_t n, int lanes, int fw, bool stage) {
    const int64_t n8 = beats_n8(n);
    char *p = (char *)base;
    metrics_ws w;
    w.hd = (double *)p;
    w.hi = (int32_t *)(p + 128);
    p += MX_HDR;
    w.ld = (double *)p; p += 8 * (size_t)lanes;
    w.ld2 = (double *)p; p += 8 * (size_t)lanes;
    w.li = (int32_t *)p; p += 4 * (size_t)lanes;
    w.li2 = (int32_t *)p; p += 4 * (size_t)lanes;
    w.stk0 = (pw_frame *)p; p += sizeof(pw_frame) * MX_PW_DEPTH;
    w.stkL = (pw_frame *)p; p += sizeof(pw_frame) * (size_t)lanes * (size_t)fw;
    w.fw = fw;
    w.ns = (int64_t *)p; p += 8 * n8;
    w.rs = (double *)p; p += 8 * n8;
    w.rd = (double *)p; p += 8 * n8;
    w.v_stage = nullptr;
    w.fin_stage = nullptr;
    if (stage) { w.v_stage = (double *)p; p += 8 * n8; }
    w.c1 = (int32_t *)p; p += 4 * n8;
    w.c2 = (int32_t *)p; p += 4 * n8;
    w.ord = (int32_t *)p; p += 4 * n8;
    w.ra = (int32_t *)p; p += 4 * n8;
    w.rb = (int32_t *)p; p += 4 * n8;
    if (stage) { w.fin_stage = (int32_t *)p; p += 4 * n8; }
    w.keep = (int8_t *)p; p += n8;
    w.fl = (int8_t *)p;
    return w;
}

/* one recording's outputs: the slices at pk_off[f] and the per-file entries */
struct metrics_io {
    double *hrv_time, *hrv_rmssdc, *hrv_sdnn, *hrv_bpm;
    int32_t *n_hrv;
    int32_t *inc_a, *inc_b, *dec_a, *dec_b;
    double *inc_slope, *inc_dur, *dec_slope, *dec_dur;
    int32_t *n_inc, *n_dec;
    double *record;              /* [BPMX_METRICS_RECORD] */
};

/* ---- accessors of the sums ----------------------------------------------- */
struct mx_arr {                  /* a[k] */
    const double *a;
    BPMX_HD double operator()(int64_t k) const { return a[k]; }
};
struct mx_ms {                   /* (np.diff(s1) / sr)[i0 + k] * 1000 */
    const int32_t *fin;
    int64_t i0;
    double sr;
    BPMX_HD double operator()(int64_t k) const {
        return ((double)((int64_t)fin[i0 + k + 1] - (int64_t)fin[i0 + k]) / sr) * 1000;
    }
};
struct mx_dsq {                  /* np.diff(ms) ** 2 */
    mx_ms ms;
    BPMX_HD double operator()(int64_t k) const {
        const double d = ms(k + 1) - ms(k);
        return d * d;
    }
};
struct mx_dev {                  /* (ms - mean) * (ms - mean) */
    mx_ms ms;
    double mean;
    BPMX_HD double operator()(int64_t k) const {
        const double d = ms(k) - mean;
        return d * d;
    }
};
struct mx_step {                 /* index.to_series().diff().dt.total_seconds() with its leading NaN as 0 (nanmean) */
    const int64_t *ns;
    BPMX_HD double operator()(int64_t k) const { return k == 0 ? 0.0 : (double)(ns[k] - ns[k - 1]) / 1e9; }
};

BPMX_HD inline int64_t mx_floordiv(int64_t a, int64_t b) {      /* Python's //, b > 0 */
    int64_t q = a / b;
    if ((a % b) < 0) --q;
    return q;
}
/* seconds of curve position j after position b0: (index - index[b0]).total_seconds() */
BPMX_HD inline double mx_tsec(const int64_t *ns, int64_t b0, int64_t j) { return (double)(ns[b0 + j] - ns[b0]) / 1e9; }

/* ---- the windowed HRV table: one lane per window -------------------------- */
template <class X>
BPMX_HD inline int64_t metrics_hrv(const X &x, const int32_t *fin, int64_t nf, int32_t sr,
                                   const bpmx_metric_params &P, const metrics_ws &w, const metrics_io &io) {
    const int64_t win = P.hrv_window_size_beats, step = P.hrv_step_size_beats, nrr = nf - 1;
    const int64_t rows = (win >= 2 && step >= 1 && nrr >= win) ? (nrr - win) / step + 1 : 0;
    pw_frame *stk = w.stkL + (size_t)x.lane() * (size_t)w.fw;
    const double srd = (double)sr;
    BPMX_PAR_FOR(x, r, rows) {
        const int64_t i = r * step;
        mx_ms ms;
        ms.fin = fin; ms.i0 = i; ms.sr = srd;
        const double mean_ms = pw_sum(ms, win, stk) / (double)win;
        const double mean_s = mean_ms / 1000.0;
        mx_dsq dq;
        dq.ms = ms;
        const double rmssd = ::sqrt(pw_sum(dq, win - 1, stk) / (double)(win - 1));
        mx_dev dv;
        dv.ms = ms; dv.mean = mean_ms;
        const double sdnn = ::sqrt(pw_sum(dv, win, stk) / (double)win);
        io.hrv_time[r] = ((double)fin[i] / srd + (double)fin[i + win] / srd) / 2.0;
        io.hrv_rmssdc[r] = mean_s > 0 ? rmssd / mean_s : 0.0;
        io.hrv_sdnn[r] = sdnn;
        io.hrv_bpm[r] = mean_s > 0 ? 60 / mean_s : 0.0;
    }
    x.sync();
    return rows;
}

/* ---- _steepest: one start per lane, then the first maximum ---------------- */
/* over the curve positions [b0, b0 + k); the winner in hi[MI_FOUND], hd[MH_A..MH_DUR]; ends with a sync() */
template <class X>
BPMX_HD inline void metrics_steepest(const X &x, double sign, int64_t b0, int64_t k, const double *v,
                                     double window, const metrics_ws &w) {
    const int64_t *ns = w.ns;
    const bool run = !(mx_tsec(ns, b0, k - 1) < window);
    double best = 0;
    int32_t bi = -1;
    if (run) {
        BPMX_PAR_FOR(x, i, k - 1) {
            const double ti = mx_tsec(ns, b0, i), target = ti + window;
            int64_t lo = 0, len = k;                  /* np.searchsorted(t, target, 'left') */
            while (len > 0) {
                const int64_t half = len >> 1;
                if (mx_tsec(ns, b0, lo + half) < target) { lo += half + 1; len -= half + 1; } else len = half;
            }
            if (lo >= k) continue;                    /* the reference's loop has ended here */
            const double dur = mx_tsec(ns, b0, lo) - ti;
            if (!(dur > 0)) continue;
            const double key = sign * ((v[b0 + lo] - v[b0 + i]) / dur);
            if (key > 0 && (bi < 0 || key > best)) { best = key; bi = (int32_t)i; }
        }
    }
    w.ld[x.lane()] = best;
    w.li[x.lane()] = bi;
    x.sync();
    if (x.lane() == 0) {
        double b = 0;
        int32_t at = -1;
        for (int l = 0; l < x.width(); ++l) {
            const int32_t i = w.li[l];
            if (i < 0) continue;
            if (at < 0 || w.ld[l] > b || (w.ld[l] == b && i < at)) { b = w.ld[l]; at = i; }
        }
        w.hi[MI_FOUND] = at >= 0;
        if (at >= 0) {                                /* the winner's row again, as the reference forms it */
            const double ti = mx_tsec(ns, b0, at), target = ti + window;
            int64_t lo = 0, len = k;
            while (len > 0) {
                const int64_t half = len >> 1;
                if (mx_tsec(ns, b0, lo + half) < target) { lo += half + 1; len -= half + 1; } else len = half;
            }
            const double dur = mx_tsec(ns, b0, lo) - ti;
            w.hd[MH_A] = (double)(b0 + at);
            w.hd[MH_B] = (double)(b0 + lo);
            w.hd[MH_SLOPE] = (v[b0 + lo] - v[b0 + at]) / dur;
            w.hd[MH_DUR] = dur;
        }
    }
    x.sync();
}

/* ---- find_peaks(sign * v, prominence, distance) on the candidates c[nc] ---- */
/* c: the local maxima of sign * v, ascending.  Leaves the survivors in c and
 * returns their count; sets hi[MI_TIE] when the visiting order among equal
 * heights decided a removal.  Ends with a sync(). */
template <class X>
BPMX_HD inline int64_t metrics_select(const X &x, double sign, int32_t *c, int64_t nc, const double *v, int64_t m,
                                      int64_t dist, double pmin, const metrics_ws &w) {
    int32_t *ord = w.ord;
    int8_t *keep = w.keep, *ok = w.fl;
    /* np.argsort(priority), stable: the later of two equal heights ranks higher and is visited first */
    BPMX_PAR_FOR(x, j, nc) {
        const double pj = sign * v[c[j]];
        int64_t r = 0;
        for (int64_t k = 0; k < nc; ++k) {
            const double pk = sign * v[c[k]];
            r += (pk < pj || (pk == pj && k < j)) ? 1 : 0;
        }
        ord[r] = (int32_t)j;
        keep[j] = 1;
    }
    x.sync();
    if (x.lane() == 0) {                              /* _select_by_peak_distance */
        for (int64_t i = nc - 1; i >= 0; --i) {
            const int64_t j = ord[i];
            if (!keep[j]) continue;
            for (int64_t k = j - 1; k >= 0 && (int64_t)c[j] - (int64_t)c[k] < dist; --k) keep[k] = 0;
            for (int64_t k = j + 1; k < nc && (int64_t)c[k] - (int64_t)c[j] < dist; ++k) keep[k] = 0;
        }
    }
    x.sync();
    int32_t tie = 0;
    BPMX_PAR_FOR(x, j, nc) {
        const int64_t p = c[j];
        const double h = sign * v[p];
        if (keep[j]) {                                /* _peak_prominences, wlen None */
            double lmin = h, rmin = h;
            for (int64_t i = p; i >= 0 && sign * v[i] <= h; --i)
                if (sign * v[i] < lmin) lmin = sign * v[i];
            for (int64_t i = p; i < m && sign * v[i] <= h; ++i)
                if (sign * v[i] < rmin) rmin = sign * v[i];
            ok[j] = (h - py_max(lmin, rmin)) >= pmin;
        } else {                                      /* removed: by a strictly higher kept one? */
            bool higher = false;
            for (int64_t k = j - 1; k >= 0 && p - (int64_t)c[k] < dist; --k)
                if (keep[k] && sign * v[c[k]] > h) higher = true;
            for (int64_t k = j + 1; k < nc && (int64_t)c[k] - p < dist; ++k)
                if (keep[k] && sign * v[c[k]] > h) higher = true;
            if (!higher) tie = 1;
            ok[j] = 0;
        }
    }
    w.li[x.lane()] = tie;
    x.sync();
    if (x.lane() == 0) {
        int64_t n = 0;
        for (int64_t j = 0; j < nc; ++j)
            if (keep[j] && ok[j]) c[n++] = c[j];
        for (int l = 0; l < x.width(); ++l)
            if (w.li[l]) w.hi[MI_TIE] = 1;
        w.hi[MI_NC] = (int32_t)n;
    }
    x.sync();
    return w.hi[MI_NC];
}

/* ---- _runs: each start with the first end behind it, sorted by slope ------ */
template <class X>
BPMX_HD inline int64_t metrics_runs(const X &x, bool rising, const int32_t *starts, int64_t n_s, const int32_t *ends,
                                    int64_t n_e, const double *v, const bpmx_metric_params &P, const metrics_ws &w,
                                    int32_t *out_a, int32_t *out_b, double *out_slope, double *out_dur) {
    int32_t *rb = w.rb;
    double *rs = w.rs, *rd = w.rd;
    BPMX_PAR_FOR(x, i, n_s) {
        const int32_t a = starts[i];
        int64_t lo = 0, len = n_e;                    /* ends[ends > a][0] */
        while (len > 0) {
            const int64_t half = len >> 1;
            if (!(a < ends[lo + half])) { lo += half + 1; len -= half + 1; } else len = half;
        }
        rb[i] = -1;
        if (lo >= n_e) continue;
        const int32_t b = ends[lo];
        const double v0 = v[a], v1 = v[b];
        const double dur = (double)(w.ns[b] - w.ns[a]) / 1e9;
        const double change = rising ? v1 - v0 : v0 - v1;
        if (dur >= P.min_duration_sec && change >= P.min_bpm_change) {
            rb[i] = b;
            rs[i] = rising ? change / dur : (v1 - v0) / dur;
            rd[i] = dur;
        }
    }
    x.sync();
    int32_t cnt = 0;
    BPMX_PAR_FOR(x, i, n_s) {
        if (rb[i] < 0) continue;
        ++cnt;
        const double si = rs[i];
        int64_t r = 0;                                /* list.sort is stable: equal slopes keep the starts' order */
        for (int64_t k = 0; k < n_s; ++k) {
            if (rb[k] < 0) continue;
            const bool first = rising ? rs[k] > si : rs[k] < si;
            r += (first || (rs[k] == si && k < i)) ? 1 : 0;
        }
        out_a[r] = starts[i];
        out_b[r] = rb[i];
        out_slope[r] = si;
        out_dur[r] = rd[i];
    }
    w.li[x.lane()] = cnt;
    x.sync();
    if (x.lane() == 0) {
        int32_t n = 0;
        for (int l = 0; l < x.width(); ++l) n += w.li[l];
        w.hi[MI_NRUN] = n;
    }
    x.sync();
    return w.hi[MI_NRUN];
}

/* ---- final_metrics over one recording ------------------------------------ */
/* fin[nf]: the final beats (samples); bt / v[m]: the curve.  The workspace
 * holds metrics_ws_bytes(n, x.width(), pw_frames(window), .) bytes for some
 * n >= nf; fin / v may point into it (staged copies).  Returns the status
 * (every lane the same value): BPMX_METRICS_NONE for fewer than two beats,
 * else BPMX_METRICS_TIE / BPMX_METRICS_E_DISTANCE bits. */
template <class X>
BPMX_HD inline int metrics_core(const X &x, int64_t nf, const int32_t *fin, int64_t m, const double *bt,
                                const double *v, int32_t sr, const bpmx_metric_params &P, int64_t epoch_us,
                                const metrics_ws &w, const metrics_io &io) {
    const bool lead = x.lane() == 0;
    if (lead) {
        *io.n_hrv = 0; *io.n_inc = 0; *io.n_dec = 0;
        for (int k = 0; k < BPMX_METRICS_RECORD; ++k) io.record[k] = bc_nan();
        w.hi[MI_TIE] = 0;
    }
    if (nf < 2) return BPMX_METRICS_NONE;
    int64_t *ns = w.ns;
    BPMX_PAR_FOR(x, i, m) ns[i] = (epoch_us + timedelta_us(bt[i])) * 1000;
    const int64_t rows = metrics_hrv(x, fin, nf, sr, P, w, io);      /* syncs */
    if (lead) {
        *io.n_hrv = (int32_t)rows;
        if (rows > 0) {
            mx_arr a;
            a.a = io.hrv_rmssdc;
            io.record[BPMX_MR_AVG_RMSSDC] = pw_sum(a, rows, w.stk0) / (double)rows;
            a.a = io.hrv_sdnn;
            io.record[BPMX_MR_AVG_SDNN] = pw_sum(a, rows, w.stk0) / (double)rows;
        }
    }
    if (m < 1) return BPMX_METRICS_OK;
    /* the curve's minimum, maximum and first maximum */
    {
        double lo = 0, hi = 0;
        int32_t at = -1;
        BPMX_PAR_FOR(x, i, m) {
            const double c = v[i];
            if (at < 0) { lo = hi = c; at = (int32_t)i; continue; }
            if (c < lo) lo = c;
            if (c > hi) { hi = c; at = (int32_t)i; }
        }
        w.ld[x.lane()] = hi; w.ld2[x.lane()] = lo; w.li[x.lane()] = at;
        x.sync();
        if (lead) {
            int32_t am = -1;
            for (int l = 0; l < x.width(); ++l) {
                const int32_t i = w.li[l];
                if (i < 0) continue;
                if (am < 0) { hi = w.ld[l]; lo = w.ld2[l]; am = i; continue; }
                if (w.ld2[l] < lo) lo = w.ld2[l];
                if (w.ld[l] > hi || (w.ld[l] == hi && i < am)) { hi = w.ld[l]; am = i; }
            }
            mx_arr a;
            a.a = v;
            io.record[BPMX_MR_AVG_BPM] = pw_sum(a, m, w.stk0) / (double)m;
            io.record[BPMX_MR_MIN_BPM] = lo;
            io.record[BPMX_MR_MAX_BPM] = hi;
            w.hi[MI_AM] = am;
        }
        x.sync();
    }
    if (m < 2) return BPMX_METRICS_OK;
    const int64_t am = w.hi[MI_AM];
    /* calculate_hrr */
    if (lead) {
        const double top = v[am];
        const int64_t chk = ns[am] + (int64_t)::llround(P.hrr_interval_sec * 1e9);
        if (!(chk > ns[m - 1])) {
            const double xq = (double)chk / 1e9;
            const int64_t G = 1000000000;
            double r;
            if (xq < (double)mx_floordiv(ns[0], G)) r = v[0];
            else if (xq > (double)mx_floordiv(ns[m - 1], G)) r = v[m - 1];
            else {
                int64_t lo = 0, len = m;              /* bisect_right(xp, x) */
                while (len > 0) {
                    const int64_t half = len >> 1;
                    if (!(xq < (double)mx_floordiv(ns[lo + half], G))) { lo += half + 1; len -= half + 1; } else len = half;
                }
                const int64_t j = lo - 1;
                const double xj = (double)mx_floordiv(ns[j], G), fj = v[j];
                if (j == m - 1 || xj == xq) r = fj;
                else {
                    const double xj1 = (double)mx_floordiv(ns[j + 1], G), fj1 = v[j + 1];
                    const double slope = (fj1 - fj) / (xj1 - xj);
                    r = slope * (xq - xj) + fj;
                    if (r != r) {
                        r = slope * (xq - xj1) + fj1;
                        if (r != r && fj == fj1) r = fj;
                    }
                }
            }
            io.record[BPMX_MR_HRR_PEAK] = (double)am;
            io.record[BPMX_MR_HRR_RECOVERY_BPM] = r;
            io.record[BPMX_MR_HRR_VALUE] = top - r;
        }
    }
    /* find_peak_recovery_rate: from the first maximum on; find_peak_exertion_rate: the whole curve */
    metrics_steepest(x, -1.0, am, m - am, v, P.slope_window_sec, w);
    if (lead && w.hi[MI_FOUND])
        for (int k = 0; k < 4; ++k) io.record[BPMX_MR_RECOVERY + k] = w.hd[MH_A + k];
    x.sync();
    metrics_steepest(x, 1.0, 0, m, v, P.slope_window_sec, w);
    if (lead && w.hi[MI_FOUND])
        for (int k = 0; k < 4; ++k) io.record[BPMX_MR_EXERTION + k] = w.hd[MH_A + k];
    x.sync();
    /* _turning_points */
    if (lead) {
        mx_step s;
        s.ns = ns;
        const double step = pw_sum(s, m, w.stk0) / (double)(m - 1);
        int32_t dist = 5;
        if (step == step && step != 0) {
            const double q = (P.min_duration_sec / 2) / step;         /* int(): towards zero */
            dist = q >= 2147483647.0 ? 2147483647 : (q <= -2147483647.0 ? -2147483647 : (int32_t)q);
        }
        w.hi[MI_DIST] = dist;
    }
    BPMX_PAR_FOR(x, i, m) w.fl[i] = 0;
    x.sync();
    const int64_t dist = w.hi[MI_DIST];
    if (dist < 1) return BPMX_METRICS_E_DISTANCE;     /* scipy raises ValueError */
    /* _local_maxima_1d of v and of -v: plateau midpoints */
    BPMX_PAR_FOR(x, i, m - 1) {
        if (i < 1) continue;
        const double c = v[i], b = v[i - 1];
        if (b < c || b > c) {
            int64_t j = i + 1;
            while (j < m - 1 && v[j] == c) ++j;
            if (b < c ? v[j] < c : v[j] > c) w.fl[(i + j - 1) / 2] = b < c ? 1 : 2;
        }
    }
    x.sync();
    if (lead) {
        int32_t np = 0, nt = 0;
        for (int64_t i = 0; i < m; ++i) {
            if (w.fl[i] == 1) w.c1[np++] = (int32_t)i;
            else if (w.fl[i] == 2) w.c2[nt++] = (int32_t)i;
        }
        w.hi[MI_NP] = np; w.hi[MI_NT] = nt;
    }
    x.sync();
    const int64_t np = metrics_select(x, 1.0, w.c1, w.hi[MI_NP], v, m, dist, P.prominence, w);
    const int64_t nt = metrics_select(x, -1.0, w.c2, w.hi[MI_NT], v, m, dist, P.prominence, w);
    const int st = w.hi[MI_TIE] ? BPMX_METRICS_TIE : BPMX_METRICS_OK;
    if (np == 0 || nt == 0) return st;
    const int64_t ni = metrics_runs(x, true, w.c2, nt, w.c1, np, v, P, w, io.inc_a, io.inc_b, io.inc_slope, io.inc_dur);
    const int64_t nd = metrics_runs(x, false, w.c1, np, w.c2, nt, v, P, w, io.dec_a, io.dec_b, io.dec_slope, io.dec_dur);
    if (lead) { *io.n_inc = (int32_t)ni; *io.n_dec = (int32_t)nd; }
    return st;
}

}  // namespace bpmx

#endif
