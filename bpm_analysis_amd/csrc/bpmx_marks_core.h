/*
 * bpmx_marks_core.h — a person's corrected marks of one recording (its slice
 * of a bpmx_ref_marks table) as the rows of a peak table, the final beats and
 * the BPM curve, stated once for host and device.  There is no reference
 * implementation of the conversion: include/bpmx.h (bpmx_marks_device) is the
 * definition, bpm_analysis_amd/labels.py (rows_from_marks) the same in numpy.
 * The rows are integers only; the curve is beats_series of
 * bpmx_beats_core.h, the text the beat stages run.
 *
 *   marks_rows    kept marks (type S1 / S2, ms >= 0, idx = (ms * sr + 500) /
 *                 1000 <= INT32_MAX and < nd) compacted in table order, then
 *                 the heads of the runs of equal idx compacted again: a row
 *                 per run, S1 if any of its marks is S1.  Counts in cnt[].
 *   marks_finish  the rows moved to their table slice with tags, zero gap and
 *                 NaN env / floor, the S1 rows compacted into final_idx, the
 *                 curve, the counts.
 *
 * Same pattern as the other cores: BPMX_HD functions over an executor with
 * lane(), width() and sync(), no allocation, caller-supplied workspaces.
 * Every lane takes a contiguous piece in the compactions (marks_scan); the
 * serial parts are beats_series' own.  Every call must be made by all lanes
 * with the same arguments.
 */
#ifndef BPMX_MARKS_CORE_H
#define BPMX_MARKS_CORE_H

#include "bpmx_beats_core.h"
#include "../../include/bpmx.h"

namespace bpmx {

/* ---- workspace ----------------------------------------------------------- */
enum {
    MK_HDR = 64,                 /* 16 int32 */
    MK_LANE = 3 * 4,             /* per lane: three int32 */
    MK_STRIDE = BEATS_WS_STRIDE, /* a global slice: marks_ws_fixed + MK_STRIDE * rf_off[f] */
    MK_SCRATCH = 2 * (4 + 1)     /* bytes of row scratch per mark: kept idx / type, row idx / tag */
};
enum { MH_TOTAL = 0 };           /* hi */
/* the counts of marks_rows, per recording; the first six are the record's */
enum { MC_BAD = 6, MC_PER_FILE = 8 };

BPMX_HD constexpr size_t marks_ws_head(int lanes) { return (size_t)MK_HDR + (((size_t)lanes * MK_LANE + 7) & ~(size_t)7); }
/* the workspace of marks_finish for n_s1 S1 rows */
BPMX_HD constexpr size_t marks_ws_bytes(int64_t n_s1, int lanes) { return marks_ws_head(lanes) + beats_ws_bytes(n_s1, false); }
BPMX_HD constexpr size_t marks_ws_fixed(int lanes) { return marks_ws_head(lanes) + (size_t)BEATS_WS_FIXED; }
/* the most S1 rows a budget holds */
BPMX_HD constexpr int64_t marks_ws_max_n(size_t budget, int lanes) {
    return budget < marks_ws_head(lanes) + (size_t)BEATS_WS_HDR
               ? -1
               : (int64_t)((budget - marks_ws_head(lanes) - BEATS_WS_HDR) / BEATS_WS_PER_PEAK) & ~(int64_t)7;
}

struct marks_head {
    int32_t *hi;                 /* [16] */
    int32_t *la, *lb, *lc;       /* per lane */
};

/* base must be 8-byte aligned and hold marks_ws_head(lanes) bytes */
BPMX_HD inline marks_head marks_head_layout(void *base, int lanes) {
    marks_head h;
    h.hi = (int32_t *)base;
    h.la = h.hi + 16;
    h.lb = h.la + lanes;
    h.lc = h.lb + lanes;
    return h;
}

/* ---- pieces -------------------------------------------------------------- */
/* a mark's sample index, or -1 for a mark that is dropped (nd < 0: no length given) */
BPMX_HD inline int64_t mk_idx(int32_t ms, int32_t sr, int64_t nd) {
    if (ms < 0) return -1;
    const int64_t idx = ((int64_t)ms * (int64_t)sr + 500) / 1000;
    if (idx > (int64_t)INT32_MAX || (nd >= 0 && idx >= nd)) return -1;
    return idx;
}
BPMX_HD inline bool mk_typed(int32_t t) { return t == BPMX_LABEL_S1 || t == BPMX_LABEL_S2; }

/* Exclusive positions of the kept entries of [0, n): every lane counts its
 * contiguous piece into la, lane 0 turns the counts into offsets.  Returns
 * the piece length; the total is left in h.hi[MH_TOTAL]. */
template <class X, class K>
BPMX_HD inline int64_t marks_scan(const X &x, int64_t n, const K &keep, const marks_head &h) {
    const int64_t c = (n + x.width() - 1) / x.width();
    const int64_t a = (int64_t)x.lane() * c, b = a + c < n ? a + c : n;
    int32_t cnt = 0;
    for (int64_t i = a; i < b; ++i) cnt += keep(i) ? 1 : 0;
    h.la[x.lane()] = cnt;
    x.sync();
    if (x.lane() == 0) {
        int32_t s = 0;
        for (int l = 0; l < x.width(); ++l) {
            const int32_t v = h.la[l];
            h.la[l] = s;
            s += v;
        }
        h.hi[MH_TOTAL] = s;
    }
    x.sync();
    return c;
}

struct mk_keep_mark {
    const int32_t *ms, *type;
    int32_t sr;
    int64_t nd;
    BPMX_HD bool operator()(int64_t i) const { return mk_typed(type[i]) && mk_idx(ms[i], sr, nd) >= 0; }
};
struct mk_keep_head {
    const int32_t *idx;
    BPMX_HD bool operator()(int64_t i) const { return i == 0 || idx[i] != idx[i - 1]; }
};
struct mk_keep_s1 {
    const int8_t *tag;
    BPMX_HD bool operator()(int64_t i) const { return tag[i] == BPMX_TAG_S1; }
};

/* ---- rows from marks ----------------------------------------------------- */
/* nr marks (rf_ms, rf_type) at rate sr, nd < 0: no length.  k_idx / k_type and
 * r_idx / r_tag are scratch of nr entries each; the rows are left in r_idx /
 * r_tag, the counts in cnt[MC_PER_FILE] (cnt[MC_BAD] = 0). */
template <class X>
BPMX_HD inline void marks_rows(const X &x, int64_t nr, const int32_t *rf_ms, const int32_t *rf_type, int32_t sr,
                               int64_t nd, const marks_head &h, int32_t *k_idx, int8_t *k_type, int32_t *r_idx,
                               int8_t *r_tag, int32_t *cnt) {
    const mk_keep_mark keep{rf_ms, rf_type, sr, nd};
    /* the kept marks, in table order; every lane counts what it leaves out */
    {
        const int64_t c = marks_scan(x, nr, keep, h);
        const int64_t a = (int64_t)x.lane() * c, b = a + c < nr ? a + c : nr;
        int64_t o = h.la[x.lane()];
        int32_t other = 0, dropped = 0;
        for (int64_t i = a; i < b; ++i) {
            if (!mk_typed(rf_type[i])) { ++other; continue; }
            const int64_t idx = mk_idx(rf_ms[i], sr, nd);
            if (idx < 0) { ++dropped; continue; }
            k_idx[o] = (int32_t)idx;
            k_type[o] = (int8_t)rf_type[i];
            ++o;
        }
        h.lb[x.lane()] = other;
        h.lc[x.lane()] = dropped;
    }
    x.sync();
    const int64_t nk = h.hi[MH_TOTAL];
    if (x.lane() == 0) {
        int32_t other = 0, dropped = 0;
        for (int l = 0; l < x.width(); ++l) { other += h.lb[l]; dropped += h.lc[l]; }
        cnt[BPMX_MK_N_OTHER] = other;
        cnt[BPMX_MK_N_DROPPED] = dropped;
    }
    x.sync();
    /* a row per run of equal idx */
    {
        const mk_keep_head head{k_idx};
        const int64_t c = marks_scan(x, nk, head, h);
        const int64_t a = (int64_t)x.lane() * c, b = a + c < nk ? a + c : nk;
        int64_t o = h.la[x.lane()];
        int32_t s1 = 0;
        for (int64_t i = a; i < b; ++i) {
            if (!head(i)) continue;
            bool any = false;
            for (int64_t j = i; j < nk && k_idx[j] == k_idx[i]; ++j) any = any || k_type[j] == BPMX_LABEL_S1;
            r_idx[o] = k_idx[i];
            r_tag[o] = any ? BPMX_TAG_S1 : BPMX_TAG_S2;
            s1 += any ? 1 : 0;
            ++o;
        }
        h.lb[x.lane()] = s1;
    }
    x.sync();
    if (x.lane() == 0) {
        const int32_t rows = h.hi[MH_TOTAL];
        int32_t s1 = 0;
        for (int l = 0; l < x.width(); ++l) s1 += h.lb[l];
        cnt[BPMX_MK_N_ROWS] = rows;
        cnt[BPMX_MK_N_S1] = s1;
        cnt[BPMX_MK_N_S2] = rows - s1;
        cnt[BPMX_MK_N_MERGED] = (int32_t)nk - rows;
        cnt[MC_BAD] = 0;
        cnt[7] = 0;
    }
    x.sync();
}

/* ---- rows to tables, beats and curve -------------------------------------- */
/* one recording's outputs, every pointer at the recording's slice */
struct marks_io {
    int32_t *pk_idx;
    double *pk_env, *pk_floor;   /* optional */
    int8_t *tags;
    int32_t *gap;
    int32_t *final_idx, *n_final;
    double *bpm_t, *bpm;
    int32_t *n_bpm;
    double *pass;                /* optional [3] */
    int32_t *record;             /* [BPMX_MARKS_RECORD] */
};

/* n rows (r_idx, r_tag) with the counts cnt of marks_rows.  The workspace w
 * holds beats_ws_bytes(cnt[BPMX_MK_N_S1], false) bytes.  Returns BPMX_HOST_OK
 * or BPMX_MARKS_FEW (every lane the same value). */
template <class X>
BPMX_HD inline int marks_finish(const X &x, int64_t n, const int32_t *r_idx, const int8_t *r_tag, const int32_t *cnt,
                                int32_t sr, double window_sec, const marks_head &h, const beats_ws &w,
                                const marks_io &io) {
    const bool lead = x.lane() == 0;
    const int64_t ns1 = cnt[BPMX_MK_N_S1];
    BPMX_PAR_FOR(x, i, n) {
        io.pk_idx[i] = r_idx[i];
        io.tags[i] = r_tag[i];
        io.gap[i] = 0;
        if (io.pk_env) io.pk_env[i] = bc_nan();
        if (io.pk_floor) io.pk_floor[i] = bc_nan();
    }
    if (lead) {
        for (int k = 0; k < BPMX_MARKS_RECORD; ++k) io.record[k] = k < MC_BAD ? cnt[k] : 0;
        if (io.pass) io.pass[0] = io.pass[1] = io.pass[2] = bc_nan();
    }
    if (ns1 < 2) {
        if (lead) { *io.n_final = 0; *io.n_bpm = 0; }
        return BPMX_MARKS_FEW;
    }
    /* the S1 rows, ascending */
    {
        const mk_keep_s1 keep{r_tag};
        const int64_t c = marks_scan(x, n, keep, h);
        const int64_t a = (int64_t)x.lane() * c, b = a + c < n ? a + c : n;
        int64_t o = h.la[x.lane()];
        for (int64_t i = a; i < b; ++i)
            if (keep(i)) io.final_idx[o++] = r_idx[i];
    }
    BPMX_PAR_FOR(x, i, ns1) w.I[0][i] = (int32_t)i;
    x.sync();
    int64_t n_t = 0;
    const int64_t m = beats_series(x, io.final_idx, w.I[0], ns1, sr, window_sec, w, &n_t);
    BPMX_PAR_FOR(x, i, m) { io.bpm_t[i] = w.S[1][i]; io.bpm[i] = w.S[2][i]; }
    if (lead) { *io.n_final = (int32_t)ns1; *io.n_bpm = (int32_t)m; }
    return BPMX_HOST_OK;
}

}  // namespace bpmx

#endif
