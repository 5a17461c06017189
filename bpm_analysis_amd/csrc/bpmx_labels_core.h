/*
 * bpmx_labels_core.h — the labeler's output (heartbeat_labeler.py: the S1 / S2
 * label table of <base>_labels.csv, :530-546; the S1->S2 pairs, :198-217; the
 * groups of marks separated by pauses and their statistics, :244-308; the
 * per-file mean interval, :219-242) stated once for host and device.
 *
 * It restates bpm_analysis_amd/labels.py in the same IEEE operation order,
 * over what bpmx_beats_core.h leaves: the raw peaks, the main pass' tags, the
 * gap-fill labels of the trace, the final beats and the smoothed BPM curve.
 *
 * Which peaks get a label: every final beat is an S1; a raw peak that is not
 * a final beat is an S2 when its final debug string says S2 — the label of
 * the highest gap-fill pass that touched it, else the main pass' tag.
 * Nothing else is labelled.
 *
 * Same pattern as the metrics core: BPMX_HD functions over an executor with
 * lane(), width() and sync(), no allocation, a caller-supplied workspace
 * (labels_ws_bytes / labels_ws_layout).  Parallel over all lanes: the final
 * types (one binary search of the final beats per raw peak), the compactions
 * (every lane counts a contiguous piece, lane 0 scans the lanes' counts), the
 * decimal roundings, the nearest curve row (binary search), the statistics
 * (one group per lane).  Serial on lane 0: the greedy pair walk with the
 * running sums of the summary, and the group boundaries.  Scalars a serial
 * part decides travel through the workspace header and are read after a
 * sync().  Every call must be made by all lanes with the same arguments.
 */
#ifndef BPMX_LABELS_CORE_H
#define BPMX_LABELS_CORE_H

#include <math.h>

#include "bpmx_beats_core.h"
#include "../../include/bpmx.h"

namespace bpmx {

/* ---- round(x, 3) --------------------------------------------------------- */
/* Python's round(x, 3) and float(f"{x:.3f}"): the double nearest to the
 * decimal that the exact value of x rounds to at three places, ties (of the
 * exact value) to even.  q = x * 1000 is off its exact product by e, which one
 * FMA gives exactly; n = rint(q) is the nearest integer of the exact product
 * unless q lies exactly halfway, where the sign of e decides (a double that is
 * not halfway has no halfway point between it and the exact product: halfway
 * points below 2^51 are doubles).  n / 1000.0 is one correctly rounded
 * division, which is what strtod makes of the decimal text. */
BPMX_HD inline double lb_round3(double x) {
    const double q = x * 1000.0;
    double n = rint(q);
    const double d = q - n;
    if (d == 0.5 || d == -0.5) {
        const double e = fma(x, 1000.0, -q);
        if (d == 0.5 && e > 0) n += 1.0;           /* rint went down to the even integer, the product is above half */
        else if (d == -0.5 && e < 0) n -= 1.0;     /* rint went up to the even integer, the product is below half */
    }
    return n / 1000.0;
}

/* ---- workspace ----------------------------------------------------------- */
enum {
    LB_HDR = 128,                /* 8 doubles, 16 int32 */
    LB_LANE = 4,                 /* per lane: one int32 */
    LB_PER = 4 * 8 + 6 * 4 + 3,  /* ct, cb, lt, lv; ga, gz, gc, gs, pa, pb; ty, lty, gv */
    LB_STRIDE = 64               /* a global slice: labels_ws_fixed + LB_STRIDE * pk_off[f] */
};
enum { LH_SDT = 0, LH_SBPM };                                             /* hd */
enum { LI_NL = 0, LI_NC, LI_NS1, LI_NS2, LI_NP, LI_NG, LI_NGOUT };        /* hi */

BPMX_HD constexpr size_t labels_ws_head(int lanes) { return (size_t)LB_HDR + (((size_t)lanes * LB_LANE + 7) & ~(size_t)7); }
BPMX_HD constexpr size_t labels_ws_bytes(int64_t n, int lanes) {
    return labels_ws_head(lanes) + (size_t)beats_n8(n) * (size_t)LB_PER;
}
BPMX_HD constexpr size_t labels_ws_fixed(int lanes) { return labels_ws_head(lanes) + 8 * LB_STRIDE; }
BPMX_HD constexpr int64_t labels_ws_max_n(size_t budget, int lanes) {
    return budget < labels_ws_head(lanes) ? 0 : (int64_t)((budget - labels_ws_head(lanes)) / LB_PER) & ~(int64_t)7;
}
static_assert(LB_PER <= LB_STRIDE, "a global slice holds the per-peak arrays");

struct labels_ws {
    double *hd;
    int32_t *hi;
    int32_t *li;                 /* per lane */
    double *ct, *cb;             /* the CSV's rows: rounded times and values of the non-NaN curve rows; later the
                                    groups' mean interval and mean BPM */
    double *lt, *lv;             /* the labels' times and BPM */
    int32_t *ga, *gz, *gc, *gs;  /* per group: first and last S1 label, pairs, S1 marks */
    int32_t *pa, *pb;            /* per pair: the two labels */
    int8_t *ty, *lty, *gv;       /* the type per raw peak and per label; per group: has statistics */
};

/* base must be 8-byte aligned */
BPMX_HD inline labels_ws labels_ws_layout(void *base, int64_t n, int lanes) {
    const int64_t n8 = beats_n8(n);
    char *p = (char *)base;
    labels_ws w;
    w.hd = (double *)p;
    w.hi = (int32_t *)(p + 64);
    w.li = (int32_t *)(p + LB_HDR);
    p += labels_ws_head(lanes);
    w.ct = (double *)p; p += 8 * n8;
    w.cb = (double *)p; p += 8 * n8;
    w.lt = (double *)p; p += 8 * n8;
    w.lv = (double *)p; p += 8 * n8;
    w.ga = (int32_t *)p; p += 4 * n8;
    w.gz = (int32_t *)p; p += 4 * n8;
    w.gc = (int32_t *)p; p += 4 * n8;
    w.gs = (int32_t *)p; p += 4 * n8;
    w.pa = (int32_t *)p; p += 4 * n8;
    w.pb = (int32_t *)p; p += 4 * n8;
    w.ty = (int8_t *)p; p += n8;
    w.lty = (int8_t *)p; p += n8;
    w.gv = (int8_t *)p;
    return w;
}

/* one recording's outputs: the slices at pk_off[f] and the per-file entries */
struct labels_io {
    int32_t *lb_pos, *lb_type;
    double *lb_time, *lb_bpm;
    int32_t *pr_s1, *pr_s2;
    double *pr_dt;
    int32_t *gr_id, *gr_first, *gr_last, *gr_s1, *gr_pairs;
    double *gr_dt, *gr_bpm;
    int32_t *n_labels, *n_pairs, *n_groups;
    double *record;              /* [BPMX_LABELS_RECORD] */
};

/* ---- compaction ---------------------------------------------------------- */
/* Exclusive positions of the kept entries of [0, n): every lane owns the
 * contiguous piece [lane * c, lane * c + c), c = ceil(n / width), counts its
 * kept entries into li, lane 0 turns the counts into offsets; afterwards a lane
 * walks its piece again from li[lane].  Returns the piece length; the total is
 * left in w.hi[slot]. */
template <class X, class K>
BPMX_HD inline int64_t lb_scan(const X &x, int64_t n, const K &keep, const labels_ws &w, int slot) {
    const int64_t c = (n + x.width() - 1) / x.width();
    const int64_t a = (int64_t)x.lane() * c, b = a + c < n ? a + c : n;
    int32_t cnt = 0;
    for (int64_t i = a; i < b; ++i) cnt += keep(i) ? 1 : 0;
    w.li[x.lane()] = cnt;
    x.sync();
    if (x.lane() == 0) {
        int32_t s = 0;
        for (int l = 0; l < x.width(); ++l) {
            const int32_t v = w.li[l];
            w.li[l] = s;
            s += v;
        }
        w.hi[slot] = s;
    }
    x.sync();
    return c;
}

/* the final type of raw peak i: 1 = S1 (a final beat), 2 = S2, 0 = no label */
BPMX_HD inline int lb_final_type(int32_t sample, int8_t tag, int32_t gap, const int32_t *fin, int64_t nf) {
    int64_t lo = 0, hi = nf;                          /* the first final beat >= sample */
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (fin[mid] < sample) lo = mid + 1; else hi = mid;
    }
    if (lo < nf && fin[lo] == sample) return BPMX_LABEL_S1;
    if (gap != 0) {
        for (int it = 4; it >= 0; --it) {             /* the outermost ORIGINAL_REASON wrapper */
            const int v = (gap >> (2 * it)) & 3;
            if (v) return v == BPMX_TR_GAP_S2 ? BPMX_LABEL_S2 : 0;
        }
    }
    return tag == BPMX_TAG_S2 ? BPMX_LABEL_S2 : 0;
}

/* np.argmin(np.abs(T - x)) over a non-decreasing T[0 .. m), m >= 1: the rounded
 * distances fall to the first T >= x and rise behind it, so the minimum is
 * one of its two neighbours; the first of equal distances wins */
BPMX_HD inline int64_t lb_nearest(const double *T, int64_t m, double x) {
    int64_t lo = 0, hi = m;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (T[mid] < x) lo = mid + 1; else hi = mid;
    }
    int64_t c;
    if (lo >= m) c = m - 1;
    else if (lo == 0) c = 0;
    else c = fabs(T[lo - 1] - x) <= fabs(T[lo] - x) ? lo - 1 : lo;
    const double d = fabs(T[c] - x);
    while (c > 0 && fabs(T[c - 1] - x) == d) --c;
    return c;
}

struct lb_keep_type {
    const int8_t *ty;
    BPMX_HD bool operator()(int64_t i) const { return ty[i] != 0; }
};
struct lb_keep_value {
    const double *v;
    BPMX_HD bool operator()(int64_t i) const { return v[i] == v[i]; }
};
struct lb_keep_flag {
    const int8_t *gv;
    BPMX_HD bool operator()(int64_t i) const { return gv[i] != 0; }
};

BPMX_HD inline void lb_none(bool lead, const labels_io &io) {
    if (!lead) return;
    *io.n_labels = 0; *io.n_pairs = 0; *io.n_groups = 0;
    for (int k = 0; k < BPMX_LABELS_RECORD; ++k) io.record[k] = bc_nan();
}

/* ---- one recording -------------------------------------------------------- */
/* n raw peaks (idx, tags, gap), nf final beats (fin, samples, ascending), m
 * curve rows (bt, bv).  The caller passes nf = m = 0 for a recording whose
 * beat stages did not finish.  Returns BPMX_LABELS_OK or BPMX_LABELS_NONE
 * (every lane the same value).  Outputs hold n entries each. */
template <class X>
BPMX_HD inline int labels_core(const X &x, int64_t n, const int32_t *idx, const int8_t *tags, const int32_t *gap,
                               int64_t nf, const int32_t *fin, int64_t m, const double *bt, const double *bv,
                               int32_t sr, const bpmx_label_params &P, const labels_ws &w, const labels_io &io) {
    const bool lead = x.lane() == 0;
    if (nf < 2 || m < 1) {
        lb_none(lead, io);
        return BPMX_LABELS_NONE;
    }
    /* the CSV's rows: float(f"{v:.3f}") of the rows whose BPM is not NaN */
    {
        const lb_keep_value keep{bv};
        const int64_t c = lb_scan(x, m, keep, w, LI_NC);
        const int64_t a = (int64_t)x.lane() * c, b = a + c < m ? a + c : m;
        int64_t o = w.li[x.lane()];
        for (int64_t i = a; i < b; ++i)
            if (keep(i)) { w.ct[o] = lb_round3(bt[i]); w.cb[o] = lb_round3(bv[i]); ++o; }
        x.sync();
    }
    const int64_t mc = w.hi[LI_NC];
    if (mc < 1) {
        lb_none(lead, io);
        return BPMX_LABELS_NONE;
    }
    /* final types, then the label rows in table order */
    BPMX_PAR_FOR(x, i, n) w.ty[i] = (int8_t)lb_final_type(idx[i], tags[i], gap[i], fin, nf);
    x.sync();
    {
        const lb_keep_type keep{w.ty};
        const int64_t c = lb_scan(x, n, keep, w, LI_NL);
        const int64_t a = (int64_t)x.lane() * c, b = a + c < n ? a + c : n;
        int64_t o = w.li[x.lane()];
        for (int64_t i = a; i < b; ++i) {
            if (!keep(i)) continue;
            const double t = (double)idx[i] / (double)sr;
            const double tr = lb_round3(t), v = lb_round3(w.cb[lb_nearest(w.ct, mc, t)]);
            io.lb_pos[o] = (int32_t)i; io.lb_type[o] = w.ty[i];
            io.lb_time[o] = tr; io.lb_bpm[o] = v;
            w.lt[o] = tr; w.lv[o] = v; w.lty[o] = w.ty[i];
            ++o;
        }
        x.sync();
    }
    const int64_t nl = w.hi[LI_NL];
    /* pairs (calculate_s1_s2_diffs) with the summary's running sums, and the groups' boundaries */
    if (lead) {
        int64_t i = 0, j = 0, np = 0, ns1 = 0, ns2 = 0;
        double sdt = 0., sb = 0.;
        for (int64_t k = 0; k < nl; ++k) { if (w.lty[k] == BPMX_LABEL_S1) ++ns1; else ++ns2; }
        while (i < nl && w.lty[i] != BPMX_LABEL_S1) ++i;
        while (j < nl && w.lty[j] != BPMX_LABEL_S2) ++j;
        while (i < nl && j < nl) {
            if (w.lt[j] > w.lt[i]) {
                const double dt = w.lt[j] - w.lt[i];
                w.pa[np] = (int32_t)i; w.pb[np] = (int32_t)j;
                io.pr_s1[np] = (int32_t)i; io.pr_s2[np] = (int32_t)j; io.pr_dt[np] = dt;
                sdt = np ? sdt + dt : dt;
                sb = np ? sb + w.lv[i] : w.lv[i];
                ++np;
                do ++i; while (i < nl && w.lty[i] != BPMX_LABEL_S1);
            }
            do ++j; while (j < nl && w.lty[j] != BPMX_LABEL_S2);
        }
        /* detect_labeling_groups: split where the step between S1 marks is >= gap */
        int64_t ng = 0;
        if (ns1 >= 2) {
            int64_t prev = -1;
            for (int64_t k = 0; k < nl; ++k) {
                if (w.lty[k] != BPMX_LABEL_S1) continue;
                if (prev < 0 || !(w.lt[k] - w.lt[prev] < P.gap_sec)) { w.ga[ng] = (int32_t)k; w.gs[ng] = 0; ++ng; }
                w.gz[ng - 1] = (int32_t)k;
                w.gs[ng - 1] += 1;
                prev = k;
            }
        }
        w.hi[LI_NS1] = (int32_t)ns1; w.hi[LI_NS2] = (int32_t)ns2; w.hi[LI_NP] = (int32_t)np; w.hi[LI_NG] = (int32_t)ng;
        w.hd[LH_SDT] = sdt; w.hd[LH_SBPM] = sb;
    }
    x.sync();
    const int64_t np = w.hi[LI_NP], ng = w.hi[LI_NG];
    /* calculate_group_statistics: one group per lane; the pairs whose S1 time lies in [start, end] are
       consecutive, as the S1 times of the pairs ascend.  The curve rows are done with: ct / cb take the means. */
    BPMX_PAR_FOR(x, g, ng) {
        const double start = w.lt[w.ga[g]], end = w.lt[w.gz[g]];
        int64_t lo = 0, hi = np;
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (w.lt[w.pa[mid]] < start) lo = mid + 1; else hi = mid;
        }
        int32_t cnt = 0;
        double sdt = 0., sb = 0.;
        for (int64_t p = lo; p < np && w.lt[w.pa[p]] <= end; ++p) {
            const double dt = w.lt[w.pb[p]] - w.lt[w.pa[p]], b = w.lv[w.pa[p]];
            sdt = cnt ? sdt + dt : dt;
            sb = cnt ? sb + b : b;
            ++cnt;
        }
        w.gv[g] = w.gs[g] >= 2 && cnt > 0;
        w.ct[g] = cnt ? sdt / (double)cnt : 0.;
        w.cb[g] = cnt ? sb / (double)cnt : 0.;
        w.gc[g] = cnt;
    }
    x.sync();
    {
        const lb_keep_flag keep{w.gv};
        const int64_t c = lb_scan(x, ng, keep, w, LI_NGOUT);
        const int64_t a = (int64_t)x.lane() * c, b = a + c < ng ? a + c : ng;
        int64_t o = w.li[x.lane()];
        for (int64_t g = a; g < b; ++g) {
            if (!keep(g)) continue;
            io.gr_id[o] = (int32_t)g + 1; io.gr_first[o] = w.ga[g]; io.gr_last[o] = w.gz[g];
            io.gr_s1[o] = w.gs[g]; io.gr_pairs[o] = w.gc[g];
            io.gr_dt[o] = w.ct[g]; io.gr_bpm[o] = w.cb[g];
            ++o;
        }
    }
    if (lead) {
        *io.n_labels = (int32_t)nl; *io.n_pairs = (int32_t)np; *io.n_groups = w.hi[LI_NGOUT];
        io.record[BPMX_LR_AVG_DT] = np ? w.hd[LH_SDT] / (double)np : bc_nan();
        io.record[BPMX_LR_AVG_BPM] = np ? w.hd[LH_SBPM] / (double)np : bc_nan();
        io.record[BPMX_LR_N_S1] = (double)w.hi[LI_NS1];
        io.record[BPMX_LR_N_S2] = (double)w.hi[LI_NS2];
    }
    return BPMX_LABELS_OK;
}

}  // namespace bpmx

#endif
