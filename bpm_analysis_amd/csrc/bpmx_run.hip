/*
 * bpmx_run.hip — one run: the stages in order, a short function each, over
 * the plans of bpmx_plan.h (which kernel, what geometry).
 *
 * Stage order follows analyze_wav_file (bpm_analysis.py:1731-1732) and the
 * classifier's raw-peak call (:89 -> :223-229):
 *   ENVELOPE  k_envelope_ref | native kernels (k_envelope_native.hip) | k_rect_* (rectified mode)
 *   FLOOR     k_block_stats, k_quantile, k_find_peaks(-env), k_interp,
 *             k_rolling_quantile (draft), k_sanitize, k_interp,
 *             k_rolling_quantile (final), k_floor_final
 *   PEAKS     k_find_peaks(env, height=floor)
 * Everything is enqueued on one stream; no host synchronisation inside a run
 * except the (cached) upload of the batch geometry.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <mutex>
#include <vector>

#include "bpmx_common.h"
#include "bpmx_kernels.h"
#include "bpmx_ctx.h"
#include "bpmx_run.h"
#include "bpmx_plan.h"
#include "bpmx_native.h"
#include "bpmx_fpscan.h"

#include <rocprofiler-sdk-roctx/roctx.h>

using namespace bpmx;

namespace {

/* Per-stage roctx ranges (SURVEY.md §5 tracing): a run's ENVELOPE, FLOOR and
 * PEAKS launches are enqueued inside "bpmx:<stage>" ranges, so a profile taken
 * with rocprofv3 --marker-trace --kernel-trace groups each kernel under its
 * stage (the reference itself only logs a total time, bpm_analysis.py:1727,
 * :1767-1768).  The ranges cover host-side enqueueing; the kernels they
 * correlate with run asynchronously after. */
struct StageRange {
    explicit StageRange(const char *name) { roctxRangePushA(name); }
    ~StageRange() { roctxRangePop(); }
    StageRange(const StageRange &) = delete;
    StageRange &operator=(const StageRange &) = delete;
};

/* per-run output init from the cached device geometry (no pageable H2D copy
 * on the run path): flags = TOO_SHORT for inactive recordings, counts 0 */
__global__ __launch_bounds__(256) void k_init_out(InitOutArgs I) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f < I.n_files) init_out_one(I, f);
}

/* recordings with >= 5 raw troughs reach the rolling quantile: with a noise
 * window below min_periods pandas raises there (bpm_analysis.py:1085) */
__global__ __launch_bounds__(256) void k_flag_window(int n_files, const int32_t *run, int32_t *flags) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f < n_files && run[f]) flags[f] |= BPMX_F_BAD_WINDOW;
}

/* the rolling-quantile kernels' dynamic-LDS limit, raised once per device
 * (the attribute applies to the current device) to the largest layout they
 * take, not per launch on the run path */
void wm_lds_attr(int device) {
    static std::mutex mu;
    static std::vector<char> done;
    std::lock_guard<std::mutex> lk(mu);
    if (device < 0) return;
    if ((int)done.size() <= device) done.resize((size_t)device + 1, 0);
    if (done[(size_t)device]) return;
    const int mx = (int)wm_layout(WM_MMAX, false).total;
    (void)hipFuncSetAttribute((const void *)k_rollq_wm_t<true>, hipFuncAttributeMaxDynamicSharedMemorySize, mx);
    (void)hipFuncSetAttribute((const void *)k_rollq_wm_t<false>, hipFuncAttributeMaxDynamicSharedMemorySize, mx);
    (void)hipFuncSetAttribute((const void *)k_floor_wm, hipFuncAttributeMaxDynamicSharedMemorySize, mx);
    done[(size_t)device] = 1;
}

/* whether two k_floor_wm_half workgroups are resident per CU, asked once per
 * device (the current one) with its dynamic-LDS limit raised; when the
 * runtime answers anything else the split launch has no point and the run
 * takes k_floor_wm alone */
bool wmh_two_resident(int device) {
    static std::mutex mu;
    static std::vector<signed char> ans;
    std::lock_guard<std::mutex> lk(mu);
    if (device < 0) return false;
    if ((int)ans.size() <= device) ans.resize((size_t)device + 1, -1);
    if (ans[(size_t)device] < 0) {
        const size_t lds = wmh_layout().total;
        int nb = 0;
        const bool ok =
            hipFuncSetAttribute((const void *)k_floor_wm_half, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) ==
                hipSuccess &&
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)k_floor_wm_half, WMH_T, lds) == hipSuccess;
        if (!ok) (void)hipGetLastError();
        ans[(size_t)device] = ok && nb == 2 ? 1 : 0;
    }
    return ans[(size_t)device] == 1;
}

/* one run's state, handed from stage to stage */
struct Run {
    bpmx_ctx *ctx;
    const bpmx_params *P;
    const bpmx_out *O;
    const bpmx_peak_order *ord;
    bpmx_batch B;                      /* the caller's batch, its PCM base realigned (build_geometry) */
    bool do_env, env_active;
    RunGeo G;
    DetectPlan D;
    int64_t *d_stats;                  /* BPMX_OPT_STATS counters, or null */
    InitOutArgs io;
    /* the detection stages' quantile levels; noise_lazy: the noise-floor level
     * (static fallback, < 5 troughs) is computed after the trough search */
    QuantArgs qa;
    bool noise_lazy;
    bool q_in_env;                     /* every active recording's quantiles came with its envelope */
    double *qv;
    int32_t *draft_masks, *draft_vfl;  /* the draft bracket's per-recording masks and counters */
    /* find_peaks' candidate lists and the run's scan record (bpmx_fpscan.h:
     * the trough launch's scan, reused by the peak launch) */
    int32_t *cand, *vcand, *fp_scan, *fp_fb;
    double *cval, *vval, *bmax, *bmin;
    uint8_t *state;
    BlockStatArgs bs;
    FplArgs fl;
    /* FLOOR: raw troughs, and env at the raw and at the sanitised troughs,
     * beside the indices (the trough search and k_sanitize write them; the
     * floor kernels read them instead of gathering a cache line of env per
     * trough); the interpolated troughs; the draft floor */
    int64_t *rawt;
    double *rawv, *trv, *dense, *draft;
    uint16_t *wm_pos, *wm_pos_ch;      /* wavelet matrix: rank -> index, per recording and per chunk */
    int32_t *wm_full, *wm_fail;
    int32_t *wm_redo;                  /* [F] recordings k_floor_wm_half hands to k_floor_wm */
};

int check_args(bpmx_ctx *ctx, const bpmx_params *P, const bpmx_batch *B, const bpmx_out *O) {
    if (!ctx || !P || !B || !O) return fail(BPMX_E_ARG, "NULL argument");
    if (B->n_files < 1 || !B->frame_offsets) return fail(BPMX_E_ARG, "empty batch");
    if (P->mode != BPMX_MODE_REFERENCE && P->mode != BPMX_MODE_NATIVE && P->mode != BPMX_MODE_RECTIFIED)
        return fail(BPMX_E_ARG, "bad mode");
    if (P->dtype < BPMX_DT_U8 || P->dtype > BPMX_DT_I24) return fail(BPMX_E_ARG, "bad dtype");
    if (P->channels < 1 || P->ds < 1 || P->sr < 1) return fail(BPMX_E_ARG, "bad channels/ds/sr");
    const int st = P->stages;
    if (st <= 0 || st > BPMX_STAGE_ALL) return fail(BPMX_E_ARG, "bad stage mask");
    const bool do_env = st & BPMX_STAGE_ENVELOPE, do_floor = st & BPMX_STAGE_FLOOR, do_peaks = st & BPMX_STAGE_PEAKS;
    if (do_env && !B->pcm) return fail(BPMX_E_ARG, "ENVELOPE stage needs pcm");
    if (!O->env || !O->n_troughs || !O->n_peaks || !O->flags) return fail(BPMX_E_ARG, "missing output arrays");
    if ((do_floor || do_peaks) && !O->floor) return fail(BPMX_E_ARG, "floor array required");
    if (do_floor && !O->troughs) return fail(BPMX_E_ARG, "troughs array required");
    if (do_peaks && !O->peaks) return fail(BPMX_E_ARG, "peaks array required");
    if ((do_floor || do_peaks) && P->distance < 1) return fail(BPMX_E_ARG, "`distance` must be greater or equal to 1");
    if (do_floor && P->min_periods < 1) return fail(BPMX_E_ARG, "min_periods must be >= 1");
    if (do_env && P->env_window < 1) return fail(BPMX_E_ARG, "envelope window must be >= 1");
    if (P->mode == BPMX_MODE_RECTIFIED) {
        /* the envelope of the samples as they are: no decimation, no filtered signal */
        if (P->ds != 1) return fail(BPMX_E_ARG, "rectified mode: ds must be 1");
        if (O->y) return fail(BPMX_E_ARG, "rectified mode has no filtered signal: out.y must be NULL");
    }
    return BPMX_OK;
}

/* offsets and lengths of the batch on the host (boff: the 64-sample block tables') */
int build_geometry(Run &R, std::vector<int64_t> &boff) {
    RunGeo &G = R.G; const bpmx_params *P = R.P;
    const int F = G.F = R.B.n_files;
    G.foff.resize(F + 1); G.doff.resize(F + 1); boff.resize(F + 1);
    G.active.resize(F);
    G.maxnd = 0;
    G.foff[0] = 0; G.doff[0] = 0; boff[0] = 0;
    for (int f = 0; f < F; ++f) {
        const int64_t n = R.B.frame_offsets[f + 1] - R.B.frame_offsets[f];
        if (n < 0) return fail(BPMX_E_ARG, "frame offsets must be non-decreasing");
        const int64_t nd = bpmx_decimated_length(n, P->ds);
        G.foff[f + 1] = G.foff[f] + n;
        G.doff[f + 1] = G.doff[f] + nd;
        boff[f + 1] = boff[f] + (nd + 63) / 64;
        G.maxnd = std::max(G.maxnd, nd);
        /* rectified mode has no filtfilt pad: active like a run that starts from env */
        const bool ok = ((R.do_env || R.env_active) && P->mode != BPMX_MODE_RECTIFIED) ? nd > 15 : nd >= 1;
        G.active[f] = ok ? 1 : 0;
        if (nd >= (int64_t)INT_MAX / 2) return fail(BPMX_E_LIMIT, "recording too long");
    }
    G.sumnd = G.doff[F]; G.sumb = boff[F];
    if (G.sumnd == 0) return fail(BPMX_E_ARG, "empty recordings");
    /* int16 PCM whose base is not 16-byte aligned but sits a whole number of
     * frames past a 16-byte boundary (e.g. a pipelined chunk or any sub-range
     * of an aligned buffer): the kernels read from that boundary and every
     * recording's frame offset moves up by the difference, so the matrix-core
     * block kernel (16-byte aligned base) serves it.  Its projections are exact
     * integer sums and its tiles start at each recording's own first block, so
     * a recording's envelope does not depend on where it lies in the buffer
     * (include/bpmx.h, bpmx_set_pipeline).  The boundary is in the same page as
     * the base, and the kernels drop what lies before a recording's start. */
    if (R.do_env && P->dtype == BPMX_DT_I16 && R.B.pcm) {
        const uintptr_t mis = (uintptr_t)R.B.pcm & 15;
        const uintptr_t fb = (uintptr_t)2 * (uintptr_t)P->channels;
        if (mis != 0 && mis % fb == 0) {
            const int64_t sh = (int64_t)(mis / fb);
            for (int f = 0; f <= F; ++f) G.foff[f] += sh;
            R.B.pcm = (const void *)((const char *)R.B.pcm - mis);
        }
    }
    return BPMX_OK;
}

/* the geometry on the device: uploaded (one synchronisation) when it differs
 * from the context's last */
int upload_geometry(Run &R, const std::vector<int64_t> &boff) {
    RunGeo &G = R.G; bpmx_ctx *ctx = R.ctx; const int F = G.F;
    int rc = BPMX_OK;
    std::vector<int64_t> geo;
    geo.reserve(3 * (F + 1));
    geo.insert(geo.end(), G.foff.begin(), G.foff.end());
    geo.insert(geo.end(), G.doff.begin(), G.doff.end());
    geo.insert(geo.end(), boff.begin(), boff.end());
    bool g1 = false, g2 = false;
    int64_t *dgeo = (int64_t *)ctx->buf("geo", geo.size() * 8, &rc, &g1);
    int32_t *di = (int32_t *)ctx->buf("geo_i", (size_t)F * 4 * 8, &rc, &g2);
    if (rc != BPMX_OK) return rc;
    if (g1 || g2) ctx->g_key.clear();
    std::vector<int64_t> key = geo;
    key.push_back(F);
    key.push_back(R.do_env);
    if (key != ctx->g_key) {
        HIP_TRY(hipMemcpyAsync(dgeo, geo.data(), geo.size() * 8, hipMemcpyHostToDevice, G.s));
        HIP_TRY(hipMemcpyAsync(di, G.active.data(), (size_t)F * 4, hipMemcpyHostToDevice, G.s));
        HIP_TRY(hipStreamSynchronize(G.s));
        ctx->g_key = key;
    }
    G.d_foff = dgeo; G.d_doff = dgeo + F + 1; G.d_boff = dgeo + 2 * (F + 1);
    G.d_active = di;
    G.d_run1 = di + F; G.d_run2 = di + 2 * F; G.d_an1 = di + 3 * F; G.d_an2 = di + 4 * F;
    /* raw-trough counts go straight into the caller's array when it asks for them */
    G.d_nraw = (R.D.do_floor && R.O->n_raw_troughs) ? (int32_t *)R.O->n_raw_troughs : di + 5 * F;
    return BPMX_OK;
}

/* the run's outputs and counters reset (k_init_out, or left to a native
 * envelope stage's k_native_carry: one launch fewer) */
int init_outputs(Run &R) {
    const RunGeo &G = R.G; const DetectPlan &D = R.D; bpmx_ctx *ctx = R.ctx; const int F = G.F;
    int rc = BPMX_OK;
    /* the draft bracket's per-recording masks and counters (FLOOR below) are
     * zeroed here, with the outputs, instead of by two memset launches */
    if (D.bounds) {
        R.draft_masks = (int32_t *)ctx->buf("draft_masks", (size_t)F * 8, &rc);
        R.draft_vfl = (int32_t *)ctx->buf("draft_vfl", (size_t)F * 16, &rc);
        if (rc != BPMX_OK) return rc;
    }
    if (D.do_floor || D.do_peaks) {
        R.cand = (int32_t *)ctx->buf("cand", (size_t)G.sumnd * 4, &rc);
        R.vcand = (int32_t *)ctx->buf("vcand", (size_t)G.sumnd * 4, &rc);
        R.cval = (double *)ctx->buf("cval", (size_t)G.sumnd * 8, &rc);
        R.vval = (double *)ctx->buf("vval", (size_t)G.sumnd * 8, &rc);
        R.fp_scan = (int32_t *)ctx->buf("fp_scan", (size_t)F * 4 * (1 + 2 * FPS_NW), &rc);
        if (rc != BPMX_OK) return rc;
    }
    InitOutArgs &io = R.io;
    io.active = G.d_active; io.flags = (int32_t *)R.O->flags; io.n_files = F;
    io.ntr = D.do_floor ? (int32_t *)R.O->n_troughs : nullptr;
    io.npk = D.do_peaks ? (int32_t *)R.O->n_peaks : nullptr;
    io.runs = G.d_run1;
    io.nraw = G.d_nraw == R.O->n_raw_troughs ? G.d_nraw : nullptr;       /* the caller's raw-trough counts */
    io.z1 = R.draft_masks; io.z2 = D.bounds ? R.draft_vfl + 2 * F : nullptr; io.z3 = R.fp_scan;
    const bool init_in_carry = R.do_env && R.P->mode == BPMX_MODE_NATIVE;
    if (!init_in_carry) LAUNCH(ctx, G.s, "k_init_out", k_init_out, dim3((F + 255) / 256), dim3(256), 0, G.s, io);
    return BPMX_OK;
}

/* the detection stages' quantile levels, built before the envelope stage so
 * that the fused native Hilbert kernel can compute them from the envelope it
 * writes */
int quant_levels(Run &R) {
    const bpmx_params *P = R.P; const DetectPlan &D = R.D;
    int rc = BPMX_OK;
    R.qv = (double *)R.ctx->buf("qv", (size_t)R.G.F * Q_SLOTS * 8, &rc);
    if (rc != BPMX_OK) return rc;
    QuantArgs &qa = R.qa;
    qa.env = R.O->env; qa.doff = R.G.d_doff; qa.active = R.G.d_active; qa.n_files = R.G.F; qa.qv = R.qv;
    qa.skip_le = QR_MAX;
    int L = 0;
    auto add = [&](double q, int slot) {      /* one radix select per distinct level */
        for (int l = 0; l < L; ++l)
            if (qa.q[l] == q) { qa.slot[l] |= 1 << slot; return; }
        qa.q[L] = q; qa.slot[L] = 1 << slot; ++L;
    };
    /* the noise-floor level (static fallback, < 5 troughs) is computed
     * lazily after the trough search unless it coincides with a level
     * needed anyway */
    if (D.do_floor) { add(P->trough_prom_q, Q_TROUGH); add(P->fallback_q, Q_FALLBACK); }
    if (D.do_peaks) add(P->peak_prom_q, Q_PEAK);
    if (D.do_floor) {
        R.noise_lazy = true;
        for (int l = 0; l < L; ++l)
            if (qa.q[l] == P->noise_floor_q) { qa.slot[l] |= 1 << Q_NOISE; R.noise_lazy = false; }
    }
    qa.n_levels = L;                      /* stats 0: k_find_peaks builds its own block tables when it runs */
    return BPMX_OK;
}

/* the lazy noise-floor level alone (at most three distinct levels before it,
 * so it always fits in Q_SLOTS) */
QuantArgs noise_level(const Run &R) {
    QuantArgs a{};
    a.env = R.O->env; a.doff = R.G.d_doff; a.active = R.G.d_active; a.n_files = R.G.F; a.qv = R.qv;
    a.skip_le = QR_MAX; a.n_levels = 1; a.q[0] = R.P->noise_floor_q; a.slot[0] = 1 << Q_NOISE;
    return a;
}

/* ---- ENVELOPE, reference mode ---- */

struct RefKernels {
    void (*pick)(EnvRefArgs);
    void (*body)(EnvRefArgs);
    void (*fwd)(EnvRefArgs);
};
/* zb: b = b0 (1, 0, -2, 0, 1) exactly with integer PCM (always finite):
 * the filter step's short form (k_envelope_ref.hip, Df2t::step) */
template <int DT, bool MULTI>
RefKernels ref_kernels_m(bool zb) {
    constexpr bool Z = DT <= BPMX_DT_I32;
    if (zb && Z) return {k_ref_pick<DT, MULTI>, k_envelope_ref_t<DT, MULTI, Z>, k_ref_fwd<Z>};
    return {k_ref_pick<DT, MULTI>, k_envelope_ref_t<DT, MULTI, false>, k_ref_fwd<false>};
}
template <int DT>
RefKernels ref_kernels(bool multi, bool zb) {
    return multi ? ref_kernels_m<DT, true>(zb) : ref_kernels_m<DT, false>(zb);
}

/* gather, forward pass and the rest of k_envelope_ref_t; split: the forward
 * pass in row chunks while k_ref_pick gathers the next chunks on a side
 * stream (else one gather, then the whole pass in k_envelope_ref_t) */
int ref_passes(Run &R, const RefEnvPlan &E, bool split, const RefKernels &K, const EnvRefArgs &a) {
    bpmx_ctx *ctx = R.ctx; hipStream_t s = R.G.s; const int F = R.G.F;
    const dim3 g((F + 63) / 64), b(64);
    if (!split) {
        const dim3 gp((unsigned)((R.G.maxnd + 30 + 63) / 64), (unsigned)((F + 63) / 64));
        LAUNCH(ctx, s, "k_ref_pick", K.pick, gp, dim3(256), 0, s, a);
        LAUNCH(ctx, s, "k_envelope_ref", K.body, g, b, 0, s, a);
        return BPMX_OK;
    }
    EnvRefArgs c = a;
    hipStream_t s2 = ctx->side[0];
    HIP_TRY(hipEventRecord(ctx->side_fork, s));
    HIP_TRY(hipStreamWaitEvent(s2, ctx->side_fork, 0));
    for (int64_t k = 0; k < E.nfc; ++k) {
        const int64_t r0 = E.fwd_row(k), r1 = E.fwd_row(k + 1);
        c.pick_r0 = r0;
        const dim3 gk((unsigned)((r1 - r0 + 63) / 64), (unsigned)((F + 63) / 64));
        hipStream_t sk = k == 0 ? s : s2;
        LAUNCH(ctx, sk, "k_ref_pick", K.pick, gk, dim3(256), 0, sk, c);
        if (k > 0) HIP_TRY(hipEventRecord(ctx->ref_ev[k], s2));
    }
    for (int64_t k = 0; k < E.nfc; ++k) {
        if (k > 0) HIP_TRY(hipStreamWaitEvent(s, ctx->ref_ev[k], 0));
        c.fwd_rb = E.fwd_row(k);
        c.fwd_re = E.fwd_row(k + 1);
        LAUNCH(ctx, s, "k_ref_fwd", K.fwd, g, b, 0, s, c);
    }
    LAUNCH(ctx, s, "k_envelope_ref", K.body, g, b, 0, s, c);
    return BPMX_OK;
}

/* chain mode: the rolling mean's outputs after the sequential pass; nkc > 0:
 * the Kahan pass in nkc row chunks, each finished chunk's means formed by
 * k_ref_env_mean on the side stream while the next chunk runs */
int ref_means(Run &R, const RefEnvPlan &E, int nkc, const EnvRefArgs &a) {
    bpmx_ctx *ctx = R.ctx; hipStream_t s = R.G.s; const int F = R.G.F;
    const dim3 g((F + 63) / 64), b(64);
    auto mean = a.y ? k_ref_env_mean<true> : k_ref_env_mean<false>;
    if (!nkc) {
        const dim3 gm((unsigned)((R.G.maxnd + 63) / 64), (unsigned)((F + 63) / 64));
        LAUNCH(ctx, s, "k_ref_env_mean", mean, gm, dim3(256), 0, s, a);
        return BPMX_OK;
    }
    hipStream_t s2 = ctx->side[0];
    EnvRefArgs c = a;
    for (int k = 0; k < nkc; ++k) {
        if (k > 0) {                             /* steps [kend[k-1], kend[k]) */
            c.kahan_ib = E.kend[k - 1];
            c.kahan_ie = E.kend[k];
            LAUNCH(ctx, s, "k_ref_kahan", k_ref_kahan, g, b, 0, s, c);
        }
        hipEvent_t ek = ctx->ref_ev[E.nfc + k];
        HIP_TRY(hipEventRecord(ek, s));
        HIP_TRY(hipStreamWaitEvent(s2, ek, 0));
        const int64_t r0 = k > 0 ? E.kend[k - 1] : 0;
        EnvRefArgs mk = a;
        mk.mean_r0 = r0;
        const dim3 gm((unsigned)((E.kend[k] - r0 + 63) / 64), (unsigned)((F + 63) / 64));
        LAUNCH(ctx, s2, "k_ref_env_mean", mean, gm, dim3(256), 0, s2, mk);
    }
    hipEvent_t ej = ctx->ref_ev[E.nfc + 4];
    HIP_TRY(hipEventRecord(ej, s2));
    HIP_TRY(hipStreamWaitEvent(s, ej, 0));
    return BPMX_OK;
}

int envelope_ref(Run &R) {
    bpmx_ctx *ctx = R.ctx; const bpmx_params *P = R.P; const RunGeo &G = R.G; const int F = G.F;
    int rc = BPMX_OK;
    const RefEnvPlan E = ref_env_plan(G.maxnd, P->env_window, P->options);
    EnvRefArgs a{};
    a.scratch = (double *)ctx->buf("ref_scratch", (size_t)((G.maxnd + 30 + 63) / 64 * 64) * F * 8, &rc);
    if (rc != BPMX_OK) return rc;
    a.pcm = R.B.pcm; a.foff = G.d_foff; a.doff = G.d_doff; a.active = G.d_active;
    a.n_files = F; a.dtype = P->dtype; a.channels = P->channels; a.ds = P->ds; a.env_window = P->env_window;
    std::memcpy(a.b, P->ba_b, sizeof a.b);
    std::memcpy(a.a, P->ba_a, sizeof a.a);
    std::memcpy(a.zi, P->ba_zi, sizeof a.zi);
    a.env = R.O->env; a.y = R.O->y;
    a.sums = E.chain ? (double *)ctx->buf("ref_sums", (size_t)(std::max<int64_t>(G.maxnd, 1) + 1) * F * 8, &rc) : nullptr;
    a.chain = (int32_t *)ctx->buf("ref_chain", (size_t)F * 4, &rc);
    if (rc != BPMX_OK) return rc;
    const bool zb = P->ba_b[1] == 0.0 && P->ba_b[3] == 0.0 && P->ba_b[4] == P->ba_b[0] &&
                    P->ba_b[2] == -2.0 * P->ba_b[0] &&
                    (P->dtype == BPMX_DT_U8 || P->dtype == BPMX_DT_I16 || P->dtype == BPMX_DT_I32 ||
                     P->dtype == BPMX_DT_I24);
    /* without a side stream or its events: the unsplit form */
    const bool split = E.wants_split && ctx->side_ready() && ctx->ref_events((size_t)E.nfc);
    if (split) {
        a.fwd_z = (double *)ctx->buf("ref_fwd_z", (size_t)F * 4 * 8, &rc);
        if (rc != BPMX_OK) return rc;
    }
    const int nkc = split && E.nkc && ctx->ref_events((size_t)E.nfc + 8) ? E.nkc : 0;
    if (nkc) {
        a.kahan_z = (double *)ctx->buf("ref_kahan_z", (size_t)F * 6 * 8, &rc);
        if (rc != BPMX_OK) return rc;
        a.kahan_ie = E.kend[0];
    }
    const bool multi = P->channels > 1;
    RefKernels K;
    switch (P->dtype) {
    case BPMX_DT_U8: K = ref_kernels<BPMX_DT_U8>(multi, zb); break;
    case BPMX_DT_I16: K = ref_kernels<BPMX_DT_I16>(multi, zb); break;
    case BPMX_DT_I32: K = ref_kernels<BPMX_DT_I32>(multi, zb); break;
    case BPMX_DT_F32: K = ref_kernels<BPMX_DT_F32>(multi, zb); break;
    case BPMX_DT_I24:                              /* its own gather; the passes are int32's (same samples) */
        K = ref_kernels<BPMX_DT_I32>(multi, zb);
        K.pick = multi ? k_ref_pick<BPMX_DT_I24, true> : k_ref_pick<BPMX_DT_I24, false>;
        break;
    default: K = ref_kernels<BPMX_DT_F64>(multi, zb); break;
    }
    if ((rc = ref_passes(R, E, split, K, a)) != BPMX_OK) return rc;
    return E.chain ? ref_means(R, E, nkc, a) : BPMX_OK;
}

/* ---- ENVELOPE, rectified mode ---- */

struct RectKernels {
    void (*lds)(RectArgs);
    void (*csum)(RectArgs);
    void (*gout)(RectArgs);
};
template <int DT>
RectKernels rect_kernels(bool stereo) {
    if (stereo) return {k_rect_lds<DT, true>, k_rect_csum<DT, true>, k_rect_gout<DT, true>};
    return {k_rect_lds<DT, false>, k_rect_csum<DT, false>, k_rect_gout<DT, false>};
}

/* the route and its geometry are rect_plan's (bpmx_plan.h, with the argument
 * for the exact-integer route) */
int envelope_rect(Run &R) {
    bpmx_ctx *ctx = R.ctx; const bpmx_params *P = R.P; const RunGeo &G = R.G; hipStream_t s = G.s; const int F = G.F;
    int rc = BPMX_OK;
    const RectPlan E = rect_plan(P->dtype, P->channels, P->env_window, P->options, F, G.maxnd);
    RectArgs a{};
    a.pcm = R.B.pcm; a.foff = G.d_foff; a.doff = G.d_doff; a.active = G.d_active;
    a.n_files = F; a.dtype = P->dtype; a.channels = P->channels; a.window = P->env_window;
    a.env = R.O->env; a.nch = E.nch;
    if (E.route == RECT_GENERAL) {
        a.rows = (double *)ctx->buf("rect_rows", E.rows_bytes, &rc);
        if (rc != BPMX_OK) return rc;
        LAUNCH(ctx, s, "k_rect_pick", k_rect_pick, E.g_pick, dim3(256), 0, s, a);
        LAUNCH(ctx, s, "k_rect_seq", k_rect_seq, E.g_seq, dim3(64), 0, s, a);
        return BPMX_OK;
    }
    const bool stereo = P->channels == 2;
    const RectKernels K = P->dtype == BPMX_DT_U8    ? rect_kernels<BPMX_DT_U8>(stereo)
                          : P->dtype == BPMX_DT_I16 ? rect_kernels<BPMX_DT_I16>(stereo)
                          : P->dtype == BPMX_DT_I24 ? rect_kernels<BPMX_DT_I24>(stereo)
                                                    : rect_kernels<BPMX_DT_I32>(stereo);
    if (E.route == RECT_INT_LDS) {
        LAUNCH(ctx, s, "k_rect_lds", K.lds, E.grid, dim3(RECT_T), E.lds, s, a);
        return BPMX_OK;
    }
    a.csum = (int64_t *)ctx->buf("rect_csum", E.csum_bytes, &rc);
    if (rc != BPMX_OK) return rc;
    LAUNCH(ctx, s, "k_rect_csum", K.csum, E.grid, dim3(RECT_T), 0, s, a);
    LAUNCH(ctx, s, "k_rect_cscan", k_rect_cscan, dim3(F), dim3(RECT_T), 0, s, a);
    LAUNCH(ctx, s, "k_rect_gout", K.gout, E.grid, dim3(RECT_T), E.lds, s, a);
    return BPMX_OK;
}

int envelope_stage(Run &R) {
    StageRange range("bpmx:envelope");
    if (R.P->mode == BPMX_MODE_REFERENCE) return envelope_ref(R);
    if (R.P->mode == BPMX_MODE_RECTIFIED) return envelope_rect(R);
    const bool detect = R.D.do_floor || R.D.do_peaks;
    int rc = native_envelope(R.ctx, R.P, &R.B, R.O, R.G, detect ? &R.qa : nullptr, &R.io);
    if (rc != BPMX_OK) return rc;
    if (detect) {
        R.q_in_env = true;
        for (int f = 0; f < R.G.F && R.q_in_env; ++f) R.q_in_env = !R.G.active[f] || R.ctx->nat_fused[f];
    }
    return BPMX_OK;
}

/* ---- shared detection inputs: block tables, quantiles ---- */

/* long recordings' quantiles over many workgroups: five launches, two passes
 * over env (k_qv_*) */
int quantile_long(Run &R, const QuantArgs &q) {
    bpmx_ctx *ctx = R.ctx; const RunGeo &G = R.G; hipStream_t s = G.s; const int F = G.F;
    int rc = BPMX_OK;
    QvArgs V;
    V.Q = q;
    V.boff = G.d_boff; V.bmax = R.bmax; V.bmin = R.bmin;
    V.rg = (QvRange *)ctx->buf("qv_range", (size_t)F * sizeof(QvRange), &rc);
    V.st = (QvState *)ctx->buf("qv_state", (size_t)F * Q_SLOTS * sizeof(QvState), &rc);
    V.hist = (unsigned int *)ctx->buf("qv_hist", (size_t)F * QV_BINS * 4, &rc);
    V.cand = (unsigned long long *)ctx->buf("qv_cand", (size_t)G.sumnd * Q_SLOTS * 8, &rc);
    if (rc != BPMX_OK) return rc;
    HIP_TRY(hipMemsetAsync(V.hist, 0, (size_t)F * QV_BINS * 4, s));
    const dim3 gv((unsigned)((G.maxnd + QV_CHUNK - 1) / QV_CHUNK), (unsigned)F);
    LAUNCH(ctx, s, "k_quantile", k_qv_range, dim3(F), dim3(64), 0, s, V);
    LAUNCH(ctx, s, "k_quantile", k_qv_hist, gv, dim3(256), 0, s, V);
    LAUNCH(ctx, s, "k_quantile", k_qv_select, dim3(F, q.n_levels), dim3(256), 0, s, V);
    LAUNCH(ctx, s, "k_quantile", k_qv_collect, gv, dim3(256), 0, s, V);
    LAUNCH(ctx, s, "k_quantile", k_qv_final, dim3(F, q.n_levels), dim3(256), 0, s, V);
    return BPMX_OK;
}

int detection_inputs(Run &R) {
    StageRange range("bpmx:detection-inputs");
    bpmx_ctx *ctx = R.ctx; const RunGeo &G = R.G; const DetectPlan &D = R.D; hipStream_t s = G.s;
    const int F = G.F;
    int rc = BPMX_OK;
    R.bmax = (double *)ctx->buf("bmax", (size_t)G.sumb * 8, &rc);
    R.bmin = (double *)ctx->buf("bmin", (size_t)G.sumb * 8, &rc);
    R.fp_fb = (int32_t *)ctx->buf("fp_fallback", (size_t)F * 4, &rc);
    R.state = (uint8_t *)ctx->buf("state", (size_t)G.sumnd, &rc);
    if (rc != BPMX_OK) return rc;
    BlockStatArgs &bs = R.bs;
    bs.env = R.O->env; bs.doff = G.d_doff; bs.boff = G.d_boff; bs.active = G.d_active; bs.n_files = F;
    bs.bmax = R.bmax; bs.bmin = R.bmin; bs.skip_le = QR_MAX;     /* k_quantile_reg writes those tables */
    FplArgs &fl = R.fl;
    if (D.fp_long) {
        const int64_t sumnd = G.sumnd;
        fl.nu = D.fp_nu;
        fl.cnt = (int32_t *)ctx->buf("fpl_cnt", (size_t)F * fl.nu * 8, &rc);
        fl.mtot = (int32_t *)ctx->buf("fpl_mtot", (size_t)F * 4, &rc);
        fl.mp = (int32_t *)ctx->buf("fpl_mp", (size_t)sumnd * 4, &rc);
        fl.mh = (double *)ctx->buf("fpl_mh", (size_t)sumnd * 8, &rc);
        fl.vv = (double *)ctx->buf("fpl_vv", (size_t)(sumnd + F) * 8, &rc);
        const size_t n32 = (size_t)(sumnd >> 5) + 4 * (size_t)F + 4, n1k = (size_t)(sumnd >> 10) + 4 * (size_t)F + 4;
        double *b32 = (double *)ctx->buf("fpl_b32", n32 * 3 * 8, &rc);
        double *b1k = (double *)ctx->buf("fpl_b1k", n1k * 3 * 8, &rc);
        if (rc != BPMX_OK) return rc;
        fl.b32h = b32; fl.b32l = b32 + n32; fl.b32r = b32 + 2 * n32;
        fl.b1kh = b1k; fl.b1kl = b1k + n1k; fl.b1kr = b1k + 2 * n1k;
        fl.dfail = (int32_t *)ctx->buf("fpl_dfail", (size_t)F * 4, &rc);
        if (rc != BPMX_OK) return rc;
        fl.dchunk = 1;
    }
    if (D.long_files) LAUNCH(ctx, s, "k_block_stats", k_block_stats, dim3(F, D.bs_gy), dim3(256), 0, s, bs);
    if (!R.q_in_env) LAUNCH(ctx, s, "k_quantile_reg", k_quantile_reg, dim3(F), dim3(QR_T), 0, s, R.qa, bs);
    if (D.long_files) {
        /* long recordings take the noise-floor level in the same passes (one
         * more compare per key) instead of a second round of launches later */
        QuantArgs al = R.qa;
        if (R.noise_lazy) {
            al.q[al.n_levels] = R.P->noise_floor_q;
            al.slot[al.n_levels] = 1 << Q_NOISE;
            al.n_levels++;
        }
        if ((rc = quantile_long(R, al)) != BPMX_OK) return rc;
    }
    return BPMX_OK;
}

/* ---- find_peaks ---- */

struct FpLabels {
    const char *lds, *scan, *place, *fill, *dist_ch, *distance, *prom, *compact, *gm;
};
#define FP_LABELS(TAG)                                                                                    \
    {"k_find_peaks[" TAG "]", "k_fpl_scan[" TAG "]", "k_fpl_place[" TAG "]", "k_fpl_fill[" TAG "]",       \
     "k_fpl_dist_ch[" TAG "]", "k_fpl_distance[" TAG "]", "k_fpl_prom[" TAG "]", "k_fpl_compact[" TAG "]", \
     "k_find_peaks[" TAG ",gm]"}
const FpLabels FP_TROUGHS = FP_LABELS("troughs"), FP_PEAKS = FP_LABELS("peaks");
#undef FP_LABELS

/* what the trough and the peak search share of their arguments; search 0: troughs, 1: peaks */
PeakArgs peak_args(const Run &R, int search) {
    const RunGeo &G = R.G;
    PeakArgs a{};
    a.env = R.O->env; a.doff = G.d_doff; a.boff = G.d_boff; a.active = G.d_active;
    a.bmax = R.bmax; a.bmin = R.bmin; a.qv = R.qv; a.n_files = G.F; a.distance = R.P->distance;
    a.cand = R.cand; a.state = R.state;
    a.scan_ok = R.fp_scan; a.scan_cnt = R.fp_scan + G.F;   /* the run's scan record: the trough launch's */
    a.vcand = R.vcand; a.cval = R.cval; a.vval = R.vval; a.fallback = R.fp_fb; a.flags = (int32_t *)R.O->flags;
    a.lds_nmax = R.D.fp_long ? FPL_NMIN : INT64_MAX;
    if (R.ord) {
        a.cand_out = R.ord->cand[search];
        a.ncand_out = R.ord->n_cand[search];
        a.rank = R.ord->rank[search];
        a.use_rank = R.ord->use_rank[search];
        a.ordered_bit = search == 0 ? BPMX_F_TROUGH_ORDERED : BPMX_F_PEAK_ORDERED;
    }
    return a;
}

int find_peaks(Run &R, PeakArgs &a, const FpLabels &L) {
    bpmx_ctx *ctx = R.ctx; const DetectPlan &D = R.D; hipStream_t s = R.G.s; const int F = R.G.F;
    const FplArgs &fl = R.fl;
    if (!D.fp_global) {
        LAUNCH(ctx, s, L.lds, k_find_peaks_lds, dim3(F), dim3(1024), 0, s, a);
        a.only = R.fp_fb;             /* recordings the LDS kernel hands over */
    }
    if (D.fp_long) {
        LAUNCH(ctx, s, L.scan, k_fpl_scan, D.g_unit, dim3(256), 0, s, a, fl);
        LAUNCH(ctx, s, L.place, k_fpl_place, dim3(F), dim3(256), 0, s, a, fl);
        LAUNCH(ctx, s, L.fill, k_fpl_fill, D.g_unit, dim3(256), 0, s, a, fl);
        LAUNCH(ctx, s, L.dist_ch, k_fpl_dist_ch, D.g_dch, dim3(FPC_T), 0, s, a, fl);
        LAUNCH(ctx, s, L.distance, k_fpl_distance, dim3(F), dim3(1024), 0, s, a, fl);
        LAUNCH(ctx, s, L.prom, k_fpl_prom, D.g_prom, dim3(256), 0, s, a, fl);
        LAUNCH(ctx, s, L.compact, k_fpl_compact, dim3(F), dim3(1024), 0, s, a, fl);
    } else {
        LAUNCH(ctx, s, L.gm, k_find_peaks, dim3(F), dim3(1024), 0, s, a);
    }
    return BPMX_OK;
}

/* ---- FLOOR ---- */

/* dense = np.interp of the troughs, for the recordings the rolling-quantile
 * kernels do not interpolate themselves (the wavelet matrix stages up to
 * WM_TRMAX troughs, or a long recording's chunk) */
int interp(Run &R, const int32_t *run, const int64_t *tr, const int32_t *ntr, int64_t skip_gt) {
    InterpArgs a;
    a.env = R.O->env; a.doff = R.G.d_doff; a.troughs = tr; a.ntr = ntr; a.run = run; a.n_files = R.G.F;
    a.dense = R.dense; a.skip_n = R.D.use_wm ? WM_MMAX : -1; a.skip_gt = skip_gt;
    LAUNCH(R.ctx, R.G.s, "k_interp", k_interp, R.D.gi, dim3(256), 0, R.G.s, a);
    return BPMX_OK;
}

/* the rolling-quantile settings of the run */
RollqArgs rollq_args(const Run &R) {
    const DetectPlan &D = R.D;
    RollqArgs a{};
    a.dense = R.dense; a.doff = R.G.d_doff; a.n_files = R.G.F; a.env = R.O->env;
    a.window = (int32_t)D.W; a.min_periods = R.P->min_periods; a.cap = D.cap; a.q = R.P->noise_floor_q;
    a.wm_max = D.use_wm ? WM_MMAX : 0;
    return a;
}

/* rolling quantile of the interpolated troughs `tr` (values tv) for the
 * recordings in `run` */
int rollq(Run &R, const int32_t *run, const int64_t *tr, const int32_t *ntr, double *outp, int32_t *allnan,
          const double *tv) {
    bpmx_ctx *ctx = R.ctx; const DetectPlan &D = R.D; hipStream_t s = R.G.s; const int F = R.G.F;
    RollqArgs a = rollq_args(R);
    a.troughs = tr; a.tv = tv; a.run = run; a.ntr = ntr; a.out = outp; a.allnan = allnan;
    a.wm_fail = R.wm_fail; a.wm_pos_ch = R.wm_pos_ch;
    int rc = BPMX_OK;
    if (D.need_merge) {
        a.vfirst = (int32_t *)ctx->buf("rollq_valid", (size_t)F * 8, &rc);
        if (rc != BPMX_OK) return rc;
        a.vlast = a.vfirst + F;
        HIP_TRY(hipMemsetAsync(a.vfirst, 0x7F, (size_t)F * 4, s));      /* 0x7F7F7F7F: above any index */
        HIP_TRY(hipMemsetAsync(a.vlast, 0xFF, (size_t)F * 4, s));       /* -1 */
    }
    if (D.wm_chunks) {
        HIP_TRY(hipMemsetAsync(R.wm_fail, 0, (size_t)F * 4, s));
        a.wm_chunk = (int32_t)D.wm_c;
    }
    /* the wavelet-matrix kernels interpolate every recording <= WM_MMAX
     * themselves (from the troughs in LDS, or over global memory past
     * WM_TRMAX troughs): dense only for the sorted-union kernels */
    if (D.need_merge && (rc = interp(R, run, tr, ntr, D.wm_chunks ? WM_MMAX : INT64_MAX)) != BPMX_OK) return rc;
    if (D.use_wm) {
        /* the pruned structure; a recording it cannot take (too many
         * kept samples, > WM_TRMAX troughs, a compact-key collision)
         * runs unpruned in the same workgroup, so its LDS is the
         * larger layout (BPMX_OPT_ROLLQ_NOPRUNE: unpruned for all) */
        wm_lds_attr(ctx->device);
        if (!(R.P->options & BPMX_OPT_ROLLQ_NOPRUNE))
            LAUNCH(ctx, s, "k_rollq_wm", k_rollq_wm_t<true>, dim3(F, (unsigned)D.wm_nch), dim3(WM_T),
                   std::max(D.wm_lds_p, D.wm_lds), s, a, R.wm_pos, R.wm_full);
        else
            LAUNCH(ctx, s, "k_rollq_wm[full]", k_rollq_wm_t<false>, dim3(F), dim3(WM_T), D.wm_lds, s, a, R.wm_pos,
                   R.wm_full);
    }
    if (!D.need_merge) return BPMX_OK;
    /* long recordings: a workgroup per chunk of outputs; after the chunked
     * wavelet matrix only the recordings it gave up */
    RollqArgs fill = a;
    if (D.wm_chunks) {
        a.run = R.wm_fail;
        if ((rc = interp(R, R.wm_fail, tr, ntr, INT64_MAX)) != BPMX_OK) return rc;
    }
    a.chunk = D.chunk;
    const dim3 gq((unsigned)F, (unsigned)D.nch);
    if (D.rq_union == RQ_UNION_G) {
        a.gcap = D.gcap;
        a.gv = (double *)ctx->buf("rollq_gv", (size_t)F * D.nch * 2 * D.gcap * 8, &rc);
        a.gp = (int32_t *)ctx->buf("rollq_gp", (size_t)F * D.nch * 2 * D.gcap * 4, &rc);
        if (rc != BPMX_OK) return rc;
        (void)hipFuncSetAttribute((const void *)k_rolling_quantile_g<RQ_T>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)D.lds_g);
        LAUNCH(ctx, s, "k_rolling_quantile", (k_rolling_quantile_g<RQ_T>), gq, dim3(RQ_T), D.lds_g, s, a);
    } else if (D.rq_union == RQ_UNION_16) {
        (void)hipFuncSetAttribute((const void *)k_rolling_quantile<RQ_T, 16>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)D.lds);
        LAUNCH(ctx, s, "k_rolling_quantile", (k_rolling_quantile<RQ_T, 16>), gq, dim3(RQ_T), D.lds, s, a);
    } else {
        (void)hipFuncSetAttribute((const void *)k_rolling_quantile<RQ_T, 32>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)D.lds);
        LAUNCH(ctx, s, "k_rolling_quantile", (k_rolling_quantile<RQ_T, 32>), gq, dim3(RQ_T), D.lds, s, a);
    }
    LAUNCH(ctx, s, "k_rollq_fill", k_rollq_fill, dim3(4, (unsigned)F), dim3(256), 0, s, fill);
    return BPMX_OK;
}

/* Draft floor: sanitize reads it at the raw troughs only, so the
 * recordings whose every keep decision follows from k_draft_bounds'
 * bracket skip the full rolling quantile; the others (and, after
 * sanitize, bounded ones left with <= 2 troughs, whose floor IS the
 * draft) get it exactly.  BPMX_OPT_DRAFT_FULL forces it for all.
 * Writes the keep decisions to tdec and the recordings left open to exact. */
int draft_bracket(Run &R, uint8_t *tdec, int32_t *exact) {
    bpmx_ctx *ctx = R.ctx; const RunGeo &G = R.G; const DetectPlan &D = R.D; hipStream_t s = G.s;
    const int F = G.F;
    DraftBoundArgs a{};
    a.env = R.O->env; a.doff = G.d_doff; a.raw = R.rawt; a.rawv = R.rawv; a.nraw = G.d_nraw; a.run = G.d_run1;
    a.n_files = F;
    a.window = (int32_t)D.W; a.min_periods = R.P->min_periods; a.q = R.P->noise_floor_q; a.mult = R.P->reject_mult;
    a.dec = tdec; a.exact = exact;
    a.local_m = (R.P->options & BPMX_OPT_DRAFT_GLOBAL_RANK) ? INT_MAX : DB_LOCAL_M;
    a.stats = R.d_stats;
    a.vfl = R.draft_vfl;
    a.nund = R.draft_vfl + 2 * F;                      /* zeroed by k_init_out */
    LAUNCH(ctx, s, "k_draft_bounds", k_draft_bounds, dim3(F, D.db_gy), dim3(DB_T), 0, s, a);
    LAUNCH(ctx, s, "k_draft_points", k_draft_points<1>, dim3(F, D.dp_gy), dim3(DB_T), 0, s, a);
    LAUNCH(ctx, s, "k_draft_points[wide]", k_draft_points<4>, dim3(F, D.dp_gy), dim3(DB_T), 0, s, a);
    return BPMX_OK;
}

int floor_buffers(Run &R) {
    bpmx_ctx *ctx = R.ctx; const DetectPlan &D = R.D; const int F = R.G.F; const int64_t sumnd = R.G.sumnd;
    int rc = BPMX_OK;
    R.rawt = (int64_t *)ctx->buf("raw_troughs", (size_t)sumnd * 8, &rc);
    R.rawv = (double *)ctx->buf("raw_trough_vals", (size_t)sumnd * 8, &rc);
    R.trv = (double *)ctx->buf("trough_vals", (size_t)sumnd * 8, &rc);
    R.dense = (double *)ctx->buf("dense", (size_t)sumnd * 8, &rc);
    R.draft = (double *)ctx->buf("draft", (size_t)sumnd * 8, &rc);
    if (D.use_wm) {
        R.wm_pos = (uint16_t *)ctx->buf("wm_pos", (size_t)sumnd * 2, &rc);
        R.wm_full = (int32_t *)ctx->buf("wm_full", (size_t)F * 4, &rc);
        if (D.floor_split) R.wm_redo = (int32_t *)ctx->buf("wm_redo", (size_t)F * 4, &rc);
    }
    if (D.wm_chunks) {
        R.wm_fail = (int32_t *)ctx->buf("wm_fail", (size_t)F * 4, &rc);
        R.wm_pos_ch = (uint16_t *)ctx->buf("wm_pos_ch", (size_t)F * D.wm_nch * WM_PMAX * 2, &rc);
    }
    return rc;
}

int floor_stage(Run &R) {
    StageRange range("bpmx:floor");
    bpmx_ctx *ctx = R.ctx; const bpmx_params *P = R.P; const bpmx_out *O = R.O; const RunGeo &G = R.G;
    const DetectPlan &D = R.D; hipStream_t s = G.s; const int F = G.F;
    int rc = floor_buffers(R);
    if (rc != BPMX_OK) return rc;
    {
        PeakArgs a = peak_args(R, 0);
        a.qslot = Q_TROUGH; a.sign = -1.0; a.out = R.rawt; a.outv = R.rawv; a.nout = G.d_nraw;
        a.run_out = G.d_run1; a.run_min = 5; a.tie_bit = BPMX_F_TROUGH_TIE;
        if ((rc = find_peaks(R, a, FP_TROUGHS)) != BPMX_OK) return rc;
    }
    if (D.bad_window)
        LAUNCH(ctx, s, "k_flag_window", k_flag_window, dim3((F + 255) / 256), dim3(256), 0, s, F, G.d_run1,
               (int32_t *)O->flags);
    if (R.noise_lazy && !D.floor_wm) {    /* the static-floor quantile, for recordings with < 5 troughs */
        QuantArgs a = noise_level(R);
        a.skip = G.d_run1;                /* long recordings computed this level with the others */
        LAUNCH(ctx, s, "k_quantile_reg", k_quantile_reg, dim3(F), dim3(QR_T), 0, s, a, R.bs);
    }
    uint8_t *tdec = nullptr;
    int32_t *d_exact = G.d_run1, *d_runfb = nullptr;
    if (D.bounds) {
        tdec = (uint8_t *)ctx->buf("trough_dec", (size_t)G.sumnd, &rc);
        if (rc != BPMX_OK) return rc;
        d_exact = R.draft_masks;                             /* zeroed by k_init_out */
        d_runfb = R.draft_masks + F;
        if ((rc = draft_bracket(R, tdec, d_exact)) != BPMX_OK) return rc;
    }
    SanitizeArgs sa{};
    sa.env = O->env; sa.draft = R.draft; sa.doff = G.d_doff; sa.active = G.d_active; sa.raw = R.rawt;
    sa.nraw = G.d_nraw; sa.rawv = R.rawv; sa.outv = R.trv;
    sa.n_files = F; sa.mult = P->reject_mult; sa.out = O->troughs; sa.nout = O->n_troughs; sa.flags = O->flags;
    sa.run2 = G.d_run2; sa.dec = tdec; sa.exact = d_exact; sa.run_fb = d_runfb;
    /* the draft in full, for the recordings the bracket left open */
    if ((rc = rollq(R, d_exact, R.rawt, G.d_nraw, R.draft, G.d_an1, R.rawv)) != BPMX_OK) return rc;
    if (D.floor_wm) {
        FloorWmArgs a{};
        a.rq = rollq_args(R);
        a.sa = sa;
        a.sa.run2 = nullptr; a.sa.run_fb = nullptr;
        a.exact = d_exact;
        a.qv = R.qv;
        if (R.noise_lazy) a.qn = noise_level(R);
        a.floor = O->floor; a.draft = R.draft; a.an_draft = G.d_an1; a.an_final = G.d_an2; a.full = R.wm_full;
        wm_lds_attr(ctx->device);
        if (D.floor_split && wmh_two_resident(ctx->device)) {
            /* two half-recording workgroups per recording, then the whole-
             * recording kernel over what they handed back: it exits at once
             * for the others and is the last writer of the rest */
            HIP_TRY(hipMemsetAsync(R.wm_redo, 0, (size_t)F * 4, s));
            LAUNCH(ctx, s, "k_floor_wm", k_floor_wm_half, dim3(F, 2), dim3(WMH_T), D.wmh_lds, s, a, R.wm_redo);
            if (R.d_stats)
                LAUNCH(ctx, s, "k_count_flags", k_count_flags, dim3(1), dim3(256), 0, s, R.wm_redo, F,
                       R.d_stats + BPMX_STAT_FLOOR_WHOLE);
            a.sa.active = R.wm_redo;
            LAUNCH(ctx, s, "k_floor_wm[whole]", k_floor_wm, dim3(F), dim3(WM_T), std::max(D.wm_lds_p, D.wm_lds), s, a);
            return BPMX_OK;
        }
        LAUNCH(ctx, s, "k_floor_wm", k_floor_wm, dim3(F), dim3(WM_T), std::max(D.wm_lds_p, D.wm_lds), s, a);
        return BPMX_OK;
    }
    LAUNCH(ctx, s, "k_sanitize", k_sanitize, dim3(F), dim3(256), 0, s, sa);
    if (D.bounds && (rc = rollq(R, d_runfb, R.rawt, G.d_nraw, R.draft, G.d_an1, R.rawv)) != BPMX_OK) return rc;
    if ((rc = rollq(R, G.d_run2, O->troughs, O->n_troughs, O->floor, G.d_an2, R.trv)) != BPMX_OK) return rc;
    FinalArgs a;
    a.draft = R.draft; a.doff = G.d_doff; a.active = G.d_active; a.qv = R.qv; a.allnan_draft = G.d_an1;
    a.allnan_final = G.d_an2; a.n_files = F; a.floor = O->floor; a.flags = O->flags;
    LAUNCH(ctx, s, "k_floor_final", k_floor_final, D.gf, dim3(256), 0, s, a);
    return BPMX_OK;
}

/* ---- PEAKS ---- */

int peaks_stage(Run &R) {
    StageRange range("bpmx:peaks");
    PeakArgs a = peak_args(R, 1);
    a.height = R.O->floor; a.qslot = Q_PEAK; a.sign = 1.0; a.out = R.O->peaks; a.nout = R.O->n_peaks;
    a.tie_bit = BPMX_F_PEAK_TIE;
    return find_peaks(R, a, FP_PEAKS);
}

}  // namespace

namespace bpmx {

int run_impl(bpmx_ctx *ctx, const bpmx_params *P, const bpmx_batch *B, const bpmx_out *O, void *stream,
             bool env_active, const bpmx_peak_order *ord) {
    int rc = check_args(ctx, P, B, O);
    if (rc != BPMX_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    Run R{};
    R.ctx = ctx; R.P = P; R.O = O; R.ord = ord; R.B = *B;
    R.do_env = P->stages & BPMX_STAGE_ENVELOPE;
    R.env_active = env_active;
    R.G.s = (hipStream_t)stream;
    if (P->options & BPMX_OPT_STATS) {
        R.d_stats = (int64_t *)ctx->pr()->buf("stats", BPMX_NSTATS * 8, &rc);
        if (rc != BPMX_OK) return rc;
        if (!ctx->root)                                /* a pipelined run zeroes them once */
            HIP_TRY(hipMemsetAsync(R.d_stats, 0, BPMX_NSTATS * 8, R.G.s));
    }
    std::vector<int64_t> boff;
    if ((rc = build_geometry(R, boff)) != BPMX_OK) return rc;
    if ((rc = detect_plan(*P, R.G.F, R.G.maxnd, ord != nullptr, &R.D)) != BPMX_OK) return fail(rc, R.D.err);
    if ((rc = upload_geometry(R, boff)) != BPMX_OK) return rc;
    if ((rc = init_outputs(R)) != BPMX_OK) return rc;
    const bool detect = R.D.do_floor || R.D.do_peaks;
    if (detect && (rc = quant_levels(R)) != BPMX_OK) return rc;
    if (R.do_env && (rc = envelope_stage(R)) != BPMX_OK) return rc;
    if (!detect) return BPMX_OK;
    if ((rc = detection_inputs(R)) != BPMX_OK) return rc;
    if (R.D.do_floor && (rc = floor_stage(R)) != BPMX_OK) return rc;
    if (R.D.do_peaks && (rc = peaks_stage(R)) != BPMX_OK) return rc;
    return BPMX_OK;
}

}  // namespace bpmx
