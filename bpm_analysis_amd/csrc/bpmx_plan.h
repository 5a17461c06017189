/*
 * bpmx_plan.h — which kernels a run takes and how they are sized, as pure host
 * arithmetic over the run's parameters and the batch's shape: no HIP runtime
 * call, no context, no allocation.  bpmx_run.hip sequences the launches over
 * these plans; tests/plan_driver.hip prints them without a GPU.  The native
 * envelope's block-kernel plan is bpmx_native_plan.h, which
 * k_envelope_native.hip includes with the kernels it sizes.
 */
#ifndef BPMX_PLAN_H
#define BPMX_PLAN_H

#include <algorithm>
#include <climits>
#include <cstdio>

#include "bpmx_beats_core.h"
#include "bpmx_metrics_core.h"
#include "bpmx_labels_core.h"
#include "bpmx_score_core.h"
#include "bpmx_marks_core.h"
#include "bpmx_rect_core.h"
#include "bpmx_kernels.h"

namespace bpmx {

/* the sorted-union rolling-quantile kernel that serves need_merge */
enum { RQ_UNION_16 = 0, RQ_UNION_32 = 1, RQ_UNION_G = 2 };   /* <RQ_T,16>, <RQ_T,32>, k_rolling_quantile_g */

/* dynamic LDS the global-union kernel may ask for */
constexpr size_t RQ_G_LDS_MAX = 160 * 1024;

/* FLOOR and PEAKS: every path decision and launch geometry of a run */
struct DetectPlan {
    bool do_floor, do_peaks;
    /* noise window < min_periods: pandas' rolling() raises ValueError, but only
     * for recordings that reach it (>= 5 troughs, :1073-1085); those get
     * BPMX_F_BAD_WINDOW and the rest of the batch runs normally */
    bool bad_window;
    /* find_peaks: k_find_peaks_lds for every recording it holds; the others
     * (longer than FPL_NMIN, or more than FL_MC maxima) take the multi-
     * workgroup k_fpl_* path when the batch has long recordings, else the
     * one-workgroup k_find_peaks (BPMX_OPT_PEAKS_GLOBAL, or an ordered run,
     * whose candidate export and visiting ranks k_find_peaks implements:
     * k_find_peaks for all) */
    bool long_files;            /* some recording is beyond k_quantile_reg */
    bool fp_global, fp_long;
    int32_t fp_nu;              /* k_fpl_*: scan units per recording */
    dim3 g_unit, g_prom, g_dch;
    unsigned bs_gy;             /* k_block_stats: a few workgroups per long recording when the batch is small */
    /* the draft bracket (k_draft_bounds, k_draft_points) unless BPMX_OPT_DRAFT_FULL */
    bool bounds;
    unsigned db_gy, dp_gy;
    /* recordings of <= WM_MMAX samples: everything after the draft bracket
     * in one launch (k_floor_wm), the static floor's quantile included */
    bool floor_wm;
    /* ... its final rolling quantile by two half-recording workgroups per
     * recording that share a CU (k_floor_wm_half), then k_floor_wm over the
     * recordings they hand back: when the longest recording is eligible by
     * length (shorter ones are handed back one by one), unless
     * BPMX_OPT_FLOOR_ONEWG; the run also asks the context whether two of the
     * workgroups are resident per CU */
    bool floor_split;
    size_t wmh_lds;
    /* rolling-quantile geometry: T outputs per step, sorted union in LDS */
    int64_t W;
    int cap;
    size_t lds;
    /* wavelet-matrix kernel for recordings that fit its LDS budget; the
     * sorted-union kernel for longer ones (or when forced) */
    bool use_wm, need_merge;
    /* windows beyond the LDS sorted-union kernel: the same algorithm with
     * the union in global scratch (any window, any length) */
    bool merge_g;
    int64_t gcap;
    size_t lds_g;
    int64_t wm_n;
    size_t wm_lds_p, wm_lds;    /* pruned and unpruned layouts */
    /* long recordings: the pruned wavelet matrix over chunks of wm_c outputs
     * (a chunk's windows reach wm_c + W - 1 samples); a recording with a
     * chunk it cannot take falls to the sorted-union kernel */
    int64_t wm_c, wm_nch;
    bool wm_chunks;
    /* the union kernels (need_merge): outputs per workgroup, chunks per recording, which kernel */
    int64_t chunk, nch;
    int rq_union;
    /* k_interp / k_floor_final stride over a recording with gx workgroups:
     * 8, or more when the batch has few recordings */
    dim3 g2, gi, gf;
    char err[96];               /* the message that goes with BPMX_E_LIMIT */
};

inline int too_long(DetectPlan &D) {
    std::snprintf(D.err, sizeof D.err, "recording too long for the chunked rolling quantile");
    return BPMX_E_LIMIT;
}

inline int detect_plan(const bpmx_params &P, int F, int64_t maxnd, bool ordered, DetectPlan *out) {
    DetectPlan &D = *out;
    D = DetectPlan{};
    D.do_floor = P.stages & BPMX_STAGE_FLOOR;
    D.do_peaks = P.stages & BPMX_STAGE_PEAKS;
    D.bad_window = D.do_floor && P.noise_window < P.min_periods;
    D.bounds = D.do_floor && !(P.options & BPMX_OPT_DRAFT_FULL);

    D.long_files = maxnd > QR_MAX;
    D.fp_global = (P.options & BPMX_OPT_PEAKS_GLOBAL) != 0 || ordered;
    D.fp_long = !D.fp_global && maxnd > FPL_NMIN;
    D.fp_nu = (int32_t)((maxnd - 2 + FPL_U - 1) / FPL_U);
    D.g_unit = dim3((unsigned)((((maxnd - 2 + FPL_U - 1) / FPL_U) + 3) / 4), (unsigned)F);
    D.g_prom = dim3((unsigned)((maxnd / 2 + 1 + 255) / 256), (unsigned)F);
    D.g_dch = dim3((unsigned)((maxnd / 2 + 1 + FPC_S - 1) / FPC_S), (unsigned)F);
    D.bs_gy = (unsigned)std::min<int64_t>((((maxnd + 63) >> 6) + 3) / 4, std::max<int64_t>(1, 2048 / F));
    if (!D.do_floor) return BPMX_OK;

    D.floor_wm = !(P.options & (BPMX_OPT_ROLLQ_MERGE | BPMX_OPT_ROLLQ_GLOBAL | BPMX_OPT_ROLLQ_NOPRUNE)) &&
                 maxnd <= WM_MMAX;
    const int64_t W = D.bad_window ? P.min_periods : P.noise_window;
    D.W = W;
    D.cap = (int)((W + RQ_T - 1 + 63) / 64 * 64);
    D.lds = rollq_lds_bytes(RQ_T, D.cap);
    D.use_wm = !(P.options & (BPMX_OPT_ROLLQ_MERGE | BPMX_OPT_ROLLQ_GLOBAL));
    D.need_merge = !D.use_wm || maxnd > WM_MMAX;
    D.merge_g = D.need_merge && (D.cap > 32 * RQ_T || W + RQ_T >= 65000 || (P.options & BPMX_OPT_ROLLQ_GLOBAL));
    D.gcap = (std::min<int64_t>(W + RQ_T, maxnd + 64) + 63) / 64 * 64;
    D.lds_g = rollq_g_lds_bytes(RQ_T, D.gcap);
    if (D.merge_g && D.lds_g > RQ_G_LDS_MAX) {
        std::snprintf(D.err, sizeof D.err, "noise window and recording both longer than %d samples",
                      (160 * 1024 - 16384) / 4 * 64);
        return BPMX_E_LIMIT;
    }
    D.wm_n = std::min<int64_t>(maxnd, WM_MMAX);
    D.wm_lds_p = wm_layout(D.wm_n, true).total;
    D.wm_lds = wm_layout(D.wm_n, false).total;
    D.floor_split = D.floor_wm && !(P.options & BPMX_OPT_FLOOR_ONEWG) && wmh_eligible(maxnd, W);
    D.wmh_lds = wmh_layout().total;
    D.wm_c = (WM_MMAX - W + 1) / 64 * 64;
    D.wm_chunks = D.use_wm && maxnd > WM_MMAX && !(P.options & BPMX_OPT_ROLLQ_NOPRUNE) && D.wm_c >= 2048;
    D.wm_nch = D.wm_chunks ? (maxnd + D.wm_c - 1) / D.wm_c : 1;
    if (D.wm_nch > 65535) return too_long(D);
    D.g2 = dim3((unsigned)std::min<int64_t>((maxnd + 255) / 256, std::max<int64_t>(8, 2048 / F)), F);
    /* with no long recording only those with > WM_TRMAX troughs (rare): two workgroups each */
    D.gi = maxnd <= WM_MMAX && D.use_wm ? dim3(2, (unsigned)F) : D.g2;
    /* one workgroup per recording unless they are long: most recordings
     * exit at once, and a static or draft floor is a short fill */
    D.gf = dim3(maxnd > 65536 ? D.g2.x : 1u, (unsigned)F);
    if (D.need_merge) {
        /* long recordings: a workgroup per chunk of outputs (each chunk pays
         * one extra window fill: ~13 merge rounds against 32 or 16 tiles).
         * 8192 outputs per chunk, halved (down to 1024) while the batch
         * gives fewer than 1024 workgroups: a chunk's first-window fill is
         * fixed overhead, worth paying only when CUs would sit idle */
        D.chunk = 8192;
        while (D.chunk > 1024 && (int64_t)F * ((maxnd + D.chunk - 1) / D.chunk) < 1024) D.chunk >>= 1;
        /* the global-union kernel pays a window-sized fill per chunk: chunks of at least W */
        if (D.merge_g) D.chunk = std::max<int64_t>(D.chunk, (W + RQ_T - 1) / RQ_T * RQ_T);
        D.nch = (maxnd + D.chunk - 1) / D.chunk;
        if (D.nch > 65535) return too_long(D);
        D.rq_union = D.merge_g ? RQ_UNION_G : D.cap <= 16 * RQ_T ? RQ_UNION_16 : RQ_UNION_32;
    }
    if (D.bounds) {
        /* find_peaks' distance spaces the troughs, so a recording has at most Nd / distance + 1 */
        const int64_t trmax = maxnd / std::max<int64_t>(1, P.distance) + 1;
        D.db_gy = (unsigned)std::max<int64_t>(1, (trmax + DB_T - 1) / DB_T);
        /* at most 4 workgroups per recording, each taking every
         * gridDim.y-th chunk of 32 troughs */
        D.dp_gy = (unsigned)std::max<int64_t>(1, std::min<int64_t>(4, (trmax + DP_CHUNK - 1) / DP_CHUNK));
    }
    return BPMX_OK;
}

/* Reference-mode envelope: the forward pass in row chunks while k_ref_pick
 * gathers the next chunks on a side stream, and (chain mode) the Kahan pass in
 * row chunks whose means k_ref_env_mean forms on the side stream.  The run
 * takes the unsplit form when wants_split is 0 or the side stream or its
 * events cannot be had. */
struct RefEnvPlan {
    /* chain mode (the rolling mean's outputs formed in parallel afterwards) */
    bool chain;
    int64_t rows;               /* maxnd + 30: the padded signal */
    /* chunk k: rows [R (2^k - 1), R (2^(k+1) - 1)): the first gather is
     * short (it is not overlapped), the later ones grow while the
     * gather (faster per row than the sequential pass) stays ahead */
    int64_t nfc;
    int64_t fwd_row(int64_t k) const { return std::min(rows, REF_FWD_ROWS * ((int64_t(1) << k) - 1)); }
    bool wants_split;           /* nfc >= 2 and not BPMX_OPT_REF_NOSPLIT */
    /* chain mode of a split run: the Kahan pass in row chunks ending at 1/2,
     * 3/4, 7/8 and all of the rows (nkc 0: one pass) */
    int64_t kend[4];
    int nkc;
};

inline RefEnvPlan ref_env_plan(int64_t maxnd, int32_t env_window, int32_t options) {
    RefEnvPlan R{};
    R.chain = !(options & BPMX_OPT_REF_SERIAL_MEAN) && env_window > 1;
    R.rows = maxnd + 30;
    R.nfc = 1;
    while (R.fwd_row(R.nfc) < R.rows) ++R.nfc;
    R.wants_split = R.nfc >= 2 && !(options & BPMX_OPT_REF_NOSPLIT);
    if (R.chain && R.wants_split && maxnd >= 4096) {
        for (int k = 1; k <= 3; ++k) R.kend[R.nkc++] = (maxnd - (maxnd >> k)) & ~(int64_t)63;
        R.kend[R.nkc++] = maxnd;
    }
    return R;
}

/* Rectified-mode envelope (k_rect.hip): the route and its launch geometry.
 *
 * Exact-integer route.  For u8 / i16 / i32 PCM of one or two channels the
 * rectified frame a[i] (2 a[i] for two channels, bpmx_rect_core.h) is an
 * integer of magnitude at most 2^32.  pandas' roll_mean only ever holds sums
 * of at most w such values in its Kahan add/remove recursion, so while
 * w * 2^32 < 2^53 (w <= RECT_W_EXACT_MAX) every partial sum is exactly
 * representable, both compensation terms stay 0, and the running sum is the
 * exact window sum (+0.0 when it is zero).  calc_mean's corrections are then
 * no-ops: a run of equal values returns prev, which is the exact quotient;
 * neg_ct == 0 with a negative result and neg_ct == nobs with a positive one
 * cannot happen with an exact sum.  So env[i] = (double)S_i [* 0.5] / nobs_i
 * with S_i the int64 window sum: no sequential pass, S_i from prefix sums.
 *   LDS variant (chunk + w <= RECT_LDS_N): one workgroup per chunk of outputs
 *     loads the chunk and its halo, scans in LDS and writes the outputs.
 *   Global-prefix variant (longer windows): per-chunk sums, an exclusive scan
 *     of each recording's chunk sums, then a pass that rebuilds the chunk-
 *     local prefixes around the window ends and starts.  Three stream-ordered
 *     launches; no workgroup waits on another.
 * General route (f32 / f64, more than two channels, a window beyond the bound,
 * BPMX_OPT_RECT_SEQ): the pandas recursion, one lane per recording, over rows
 * gathered as [frame][recording]. */
enum { RECT_INT_LDS = 0, RECT_INT_GLOBAL = 1, RECT_GENERAL = 2 };

struct RectPlan {
    int route;
    bool integer;               /* the exact-integer route (either variant) */
    int64_t chunk;              /* outputs per workgroup; inputs per chunk sum */
    int64_t nch;                /* chunks of the longest recording */
    size_t lds;                 /* dynamic LDS bytes of k_rect_lds / k_rect_gout: 4 per prefix entry, 8 for int32 PCM */
    size_t csum_bytes;          /* global-prefix variant: the chunk-sum table [F][nch] */
    size_t rows_bytes;          /* general route: the row scratch [64-padded frames][F] */
    dim3 grid;                  /* integer route: (nch, F) */
    dim3 g_pick, g_seq;         /* general route */
};

inline RectPlan rect_plan(int dtype, int channels, int64_t w, int32_t options, int F, int64_t maxn) {
    RectPlan R{};
    R.chunk = RECT_CHUNK;
    R.nch = std::max<int64_t>(1, (maxn + R.chunk - 1) / R.chunk);
    const bool wide = dtype == BPMX_DT_I32 || dtype == BPMX_DT_I24;          /* I24 is the int32 sample v << 8 */
    R.integer = (dtype <= BPMX_DT_I32 || wide) && channels <= 2 && w <= RECT_W_EXACT_MAX && !(options & BPMX_OPT_RECT_SEQ);
    R.grid = dim3((unsigned)R.nch, (unsigned)F);
    const size_t entry = wide ? 8 : 4;       /* a workgroup's local prefix sums (k_rect.hip RPcm) */
    if (!R.integer) {
        R.route = RECT_GENERAL;
        const int64_t rows = (maxn + 63) / 64 * 64;
        R.rows_bytes = (size_t)rows * (size_t)F * 8;
        R.g_pick = dim3((unsigned)(rows / 64), (unsigned)((F + 63) / 64));
        R.g_seq = dim3((unsigned)((F + 63) / 64));
    } else if (R.chunk + w <= RECT_LDS_N) {
        R.route = RECT_INT_LDS;
        R.lds = (size_t)std::min<int64_t>(R.chunk + w, maxn + 1) * entry;    /* prefix entries 0 .. inputs */
    } else {
        R.route = RECT_INT_GLOBAL;
        R.lds = (size_t)(2 * R.chunk) * entry;
        R.csum_bytes = (size_t)F * (size_t)R.nch * 8;
    }
    return R;
}

/* bpmx_beats_device: one wave64 workgroup per recording (k_beats).  A
 * recording's workspace (bpmx_beats_core.h) with its copy of idx and env_pk
 * lives in LDS when it fits BEATS_LDS_BUDGET: a quarter of a CU's 160 KB, so
 * four workgroups (one wave per SIMD) share a CU, and the 605 peaks a 60 s
 * recording can have (peak_capacity(18124, 30)) are inside it.  Longer tables
 * take a slice of one global buffer at f * BEATS_WS_FIXED + BEATS_WS_STRIDE *
 * pk_off[f].  Sized from the table capacity and the file count alone: the
 * kernel reads pk_off itself, the launch needs no host synchronisation. */
constexpr size_t BEATS_LDS_BUDGET = 40 * 1024;

struct BeatsPlan {
    unsigned grid;              /* workgroups: one per recording */
    int64_t lds_n;              /* most peaks of an LDS-path recording (-1: every recording goes global) */
    size_t lds;                 /* dynamic LDS bytes per workgroup */
    bool any_global;            /* the capacity allows a recording beyond lds_n */
    size_t gws;                 /* bytes of the global workspace buffer (0: none) */
};

inline BeatsPlan beats_plan(int F, int64_t cap_peaks, int32_t options, size_t budget = BEATS_LDS_BUDGET) {
    BeatsPlan B{};
    B.grid = (unsigned)F;
    const bool forced = (options & BPMX_OPT_BEATS_GLOBAL) != 0;
    B.lds_n = forced ? -1 : std::min<int64_t>(cap_peaks, beats_ws_max_peaks(budget));
    B.lds = forced ? 0 : beats_ws_bytes(B.lds_n, true);
    B.any_global = forced || cap_peaks > B.lds_n;
    B.gws = B.any_global ? (size_t)F * BEATS_WS_FIXED + (size_t)cap_peaks * BEATS_WS_STRIDE : 0;
    return B;
}

/* bpmx_metrics_device: one workgroup of METRICS_T threads per recording
 * (k_metrics).  A recording's workspace (bpmx_metrics_core.h) with its copy of
 * the curve and the beats lives in LDS when it fits METRICS_LDS_BUDGET: 48 KB,
 * so three workgroups share a CU's 160 KB, and the 605 peaks a 60 s recording
 * can have are inside it at the default HRV window.  A window beyond 128 beats
 * gives every thread a stack for its pairwise sums, which takes from the
 * budget.  Longer tables take a slice of one global buffer at f * fixed +
 * MX_STRIDE * pk_off[f].  Sized like beats_plan from the capacity and the file
 * count alone. */
constexpr size_t METRICS_LDS_BUDGET = 48 * 1024;

struct MetricsPlan {
    unsigned grid;              /* workgroups: one per recording */
    int fw;                     /* pairwise-sum frames per thread */
    int64_t lds_n;              /* most peaks of an LDS-path recording (-1: every recording goes global) */
    size_t lds;                 /* dynamic LDS bytes per workgroup */
    bool any_global;
    size_t fixed;               /* metrics_ws_fixed(METRICS_T, fw) */
    size_t gws;                 /* bytes of the global workspace buffer (0: none) */
};

inline MetricsPlan metrics_plan(int F, int64_t cap_peaks, int32_t options, int32_t hrv_window,
                                size_t budget = METRICS_LDS_BUDGET) {
    MetricsPlan M{};
    M.grid = (unsigned)F;
    M.fw = pw_frames(hrv_window);
    const bool forced = (options & BPMX_OPT_METRICS_GLOBAL) != 0;
    M.lds_n = forced ? -1 : std::min<int64_t>(cap_peaks, metrics_ws_max_n(budget, METRICS_T, M.fw));
    if (!forced && metrics_ws_head(METRICS_T, M.fw) > budget) M.lds_n = -1;   /* the stacks alone exceed the budget */
    M.lds = M.lds_n < 0 ? 0 : metrics_ws_bytes(M.lds_n, METRICS_T, M.fw, true);
    M.any_global = cap_peaks > M.lds_n;
    M.fixed = metrics_ws_fixed(METRICS_T, M.fw);
    M.gws = M.any_global ? (size_t)F * M.fixed + (size_t)cap_peaks * MX_STRIDE : 0;
    return M;
}

/* bpmx_labels_device: one workgroup of LABELS_T threads per recording
 * (k_labels).  A recording's workspace (bpmx_labels_core.h) lives in LDS when
 * it fits LABELS_LDS_BUDGET: 40 KB, so four workgroups share a CU's 160 KB,
 * and the 605 peaks a 60 s recording can have are inside it.  Longer tables
 * take a slice of one global buffer at f * fixed + LB_STRIDE * pk_off[f].
 * Sized like beats_plan from the capacity and the file count alone. */
constexpr size_t LABELS_LDS_BUDGET = 40 * 1024;

struct LabelsPlan {
    unsigned grid;              /* workgroups: one per recording */
    int64_t lds_n;              /* most peaks of an LDS-path recording (-1: every recording goes global) */
    size_t lds;                 /* dynamic LDS bytes per workgroup */
    bool any_global;
    size_t fixed;               /* labels_ws_fixed(LABELS_T) */
    size_t gws;                 /* bytes of the global workspace buffer (0: none) */
};

inline LabelsPlan labels_plan(int F, int64_t cap_peaks, int32_t options, size_t budget = LABELS_LDS_BUDGET) {
    LabelsPlan L{};
    L.grid = (unsigned)F;
    const bool forced = (options & BPMX_OPT_LABELS_GLOBAL) != 0;
    L.lds_n = forced ? -1 : std::min<int64_t>(cap_peaks, labels_ws_max_n(budget, LABELS_T));
    L.lds = L.lds_n < 0 ? 0 : labels_ws_bytes(L.lds_n, LABELS_T);
    L.any_global = cap_peaks > L.lds_n;
    L.fixed = labels_ws_fixed(LABELS_T);
    L.gws = L.any_global ? (size_t)F * L.fixed + (size_t)cap_peaks * LB_STRIDE : 0;
    return L;
}

/* bpmx_score_device: one workgroup of SCORE_T threads per recording
 * (k_score).  A recording's workspace (bpmx_score_core.h: 17 bytes per label
 * row, 21 per reference mark) lives in LDS when it fits SCORE_LDS_BUDGET:
 * 32 KB, so five workgroups share a CU's 160 KB, and the 605 labels a 60 s
 * recording can have with as many reference marks are inside it.  Longer
 * tables take a slice of one global buffer at
 * f * fixed + SC_STRIDE * (pk_off[f] + rf_off[f]).  Sized from the two
 * capacities and the file count alone. */
constexpr size_t SCORE_LDS_BUDGET = 32 * 1024;

struct ScorePlan {
    unsigned grid;              /* workgroups: one per recording */
    size_t lds;                 /* dynamic LDS bytes per workgroup: the largest workspace of an LDS-path recording
                                   (0: every recording goes global) */
    bool any_global;
    size_t fixed;               /* score_ws_fixed(SCORE_T) */
    size_t gws;                 /* bytes of the global workspace buffer (0: none) */
};

inline ScorePlan score_plan(int F, int64_t cap_peaks, int64_t cap_ref, int32_t options,
                            size_t budget = SCORE_LDS_BUDGET) {
    ScorePlan S{};
    S.grid = (unsigned)F;
    const bool forced = (options & BPMX_OPT_SCORE_GLOBAL) != 0;
    const size_t all = score_ws_bytes(cap_peaks, cap_ref, SCORE_T);     /* the largest workspace a recording can need */
    S.lds = forced || budget < score_ws_bytes(0, 0, SCORE_T) ? 0 : std::min(all, budget);
    S.any_global = all > S.lds;
    S.fixed = score_ws_fixed(SCORE_T);
    S.gws = S.any_global ? (size_t)F * S.fixed + (size_t)(cap_peaks + cap_ref) * SC_STRIDE : 0;
    return S;
}

/* bpmx_marks_device: three launches (k_marks.hip).  k_marks_rows and
 * k_marks_finish run one workgroup of MARKS_T threads per recording; the row
 * scratch (MK_SCRATCH bytes per mark) and the counts are one context buffer.
 * k_marks_finish' workspace (bpmx_marks_core.h: the lane counts and
 * beats_series' 47 bytes per S1 row) lives in LDS when it fits
 * MARKS_LDS_BUDGET: 32 KB, so five workgroups share a CU's 160 KB, and the
 * 605 beats a 60 s recording can have are inside it.  Longer tables take a
 * slice of one global buffer at f * fixed + MK_STRIDE * rf_off[f].  Sized
 * from the marks' capacity and the file count alone. */
constexpr size_t MARKS_LDS_BUDGET = 32 * 1024;

struct MarksPlan {
    unsigned grid;              /* workgroups of the two per-recording launches */
    int64_t lds_n;              /* most S1 rows of an LDS-path recording (-1: every recording goes global) */
    size_t lds;                 /* dynamic LDS bytes per workgroup of k_marks_finish */
    bool any_global;
    size_t fixed;               /* marks_ws_fixed(MARKS_T) */
    size_t gws;                 /* bytes of the global workspace buffer (0: none) */
    size_t rows;                /* bytes of the row scratch: k_idx, r_idx, k_type, r_tag, cnt in this order */
    size_t o_ridx, o_ktype, o_rtag, o_cnt;   /* their offsets (k_idx at 0) */
};

inline MarksPlan marks_plan(int F, int64_t cap_ref, int32_t options, size_t budget = MARKS_LDS_BUDGET) {
    MarksPlan M{};
    M.grid = (unsigned)F;
    const bool forced = (options & BPMX_OPT_MARKS_GLOBAL) != 0;
    M.lds_n = forced ? -1 : std::min<int64_t>(cap_ref, marks_ws_max_n(budget, MARKS_T));
    M.lds = M.lds_n < 0 ? 0 : marks_ws_bytes(M.lds_n, MARKS_T);
    M.any_global = cap_ref > M.lds_n;
    M.fixed = marks_ws_fixed(MARKS_T);
    M.gws = M.any_global ? (size_t)F * M.fixed + (size_t)cap_ref * MK_STRIDE : 0;
    const size_t c8 = (size_t)beats_n8(cap_ref);
    M.o_ridx = 4 * c8;
    M.o_ktype = 8 * c8;
    M.o_rtag = 9 * c8;
    M.o_cnt = 10 * c8;
    M.rows = M.o_cnt + (size_t)F * MC_PER_FILE * 4;
    return M;
}

}  // namespace bpmx

#endif
