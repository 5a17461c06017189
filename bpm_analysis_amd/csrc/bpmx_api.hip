/*
 * bpmx_api.hip — host side of the C ABI (include/bpmx.h): context, scratch,
 * synthetic input, per-kernel event timing, the pipelined run, bpmx_pack,
 * bpmx_pack_trough_floor, bpmx_pack_plot, bpmx_beats_device,
 * bpmx_beats_device_ex, bpmx_metrics_device, bpmx_labels_device,
 * bpmx_score_device, bpmx_marks_device, bpmx_tempo_device and
 * bpmx_hrvspec_device.
 * A run's stages are sequenced by bpmx_run.hip (run_impl).
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "bpmx_common.h"
#include "bpmx_kernels.h"
#include "bpmx_ctx.h"
#include "bpmx_run.h"
#include "bpmx_plan.h"
#include "bpmx_native.h"
#include "bpmx_synth.h"

using namespace bpmx;

namespace bpmx {
thread_local std::string g_err;
int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
}  // namespace bpmx

namespace {

__global__ __launch_bounds__(64) void k_synth_beats(uint64_t seed0, int n_files, const int64_t *foff,
                                                    const int64_t *boff, int32_t fs, int64_t *s1, int64_t *s2,
                                                    int32_t *nb) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= n_files) return;
    const int cap = (int)(boff[f + 1] - boff[f]);
    nb[f] = bpmx_synth_beats(seed0 + (uint64_t)f, foff[f + 1] - foff[f], fs, s1 + boff[f], s2 + boff[f], cap);
}

__global__ __launch_bounds__(256) void k_synth_pcm(uint64_t seed0, int n_files, const int64_t *foff,
                                                   const int64_t *boff, int32_t fs, int channels,
                                                   const int64_t *s1, const int64_t *s2, const int32_t *nb,
                                                   int16_t *pcm) {
    const int f = blockIdx.y;
    const int64_t n = foff[f + 1] - foff[f];
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
        for (int c = 0; c < channels; ++c)
            pcm[(foff[f] + i) * channels + c] =
                bpmx_synth_sample(seed0 + (uint64_t)f, c, i, fs, s1 + boff[f], s2 + boff[f], nb[f]);
}

int beats_cap(int64_t n_frames, int32_t fs) {
    int64_t q = fs / 4 > 0 ? fs / 4 : 1;
    return (int)(n_frames / q) + 16;
}

/* the beat stages over the peak table: one launch sized by the plan; the
 * global workspace (recordings beyond the LDS budget) is context scratch */
int beats_stage(bpmx_ctx *ctx, const BeatsPlan &B, BeatsArgs &a, hipStream_t s, const BeatsExArgs *ex = nullptr) {
    int rc = BPMX_OK;
    a.lds_n = B.lds_n;
    a.gws = nullptr;
    if (B.any_global) {
        a.gws = (unsigned char *)ctx->buf("beats_ws", B.gws, &rc);
        if (rc != BPMX_OK) return rc;
    }
    if (!ex) {
        LAUNCH(ctx, s, "k_beats", k_beats, dim3(B.grid), dim3(BEATS_T), B.lds, s, a);
    } else if (ex->record) {
        LAUNCH(ctx, s, "k_beats_trace", k_beats_trace, dim3(B.grid), dim3(BEATS_T), B.lds, s, a, *ex);
    } else {
        LAUNCH(ctx, s, "k_beats_hints", k_beats_hints, dim3(B.grid), dim3(BEATS_T), B.lds, s, a, *ex);
    }
    return BPMX_OK;
}

/* the final metrics behind the beat stages: one launch sized by the plan */
int metrics_stage(bpmx_ctx *ctx, const MetricsPlan &M, int32_t n_files, int32_t sr, const bpmx_metric_params &P,
                  int64_t epoch_us, const bpmx_packed &t, const bpmx_beats_out &b, const bpmx_metrics_out &o,
                  hipStream_t s) {
    int rc = BPMX_OK;
    MetricsArgs a{};
    a.n_files = n_files; a.sr = sr; a.cap = t.cap_peaks; a.lds_n = M.lds_n; a.epoch_us = epoch_us;
    a.fw = M.fw; a.fixed = M.fixed; a.pk_off = t.pk_off;
    a.final_idx = b.final_idx; a.n_final = b.n_final; a.n_bpm = b.n_bpm; a.b_status = b.status;
    a.bpm_t = b.bpm_t; a.bpm = b.bpm;
    a.P = P; a.O = o;
    if (M.any_global) {
        a.gws = (unsigned char *)ctx->buf("metrics_ws", M.gws, &rc);
        if (rc != BPMX_OK) return rc;
    }
    LAUNCH(ctx, s, "k_metrics", k_metrics, dim3(M.grid), dim3(METRICS_T), M.lds, s, a);
    return BPMX_OK;
}

/* the labels behind the traced beat stages: one launch sized by the plan */
int labels_stage(bpmx_ctx *ctx, const LabelsPlan &L, int32_t n_files, int32_t sr, const bpmx_label_params &P,
                 const bpmx_packed &t, const bpmx_beats_out &b, const int32_t *gap, const bpmx_labels_out &o,
                 hipStream_t s) {
    int rc = BPMX_OK;
    LabelsArgs a{};
    a.n_files = n_files; a.sr = sr; a.cap = t.cap_peaks; a.lds_n = L.lds_n; a.fixed = L.fixed;
    a.pk_off = t.pk_off; a.pk_idx = t.pk_idx;
    a.final_idx = b.final_idx; a.n_final = b.n_final; a.n_bpm = b.n_bpm; a.b_status = b.status;
    a.bpm_t = b.bpm_t; a.bpm = b.bpm; a.tags = b.tags; a.gap = gap;
    a.P = P; a.O = o;
    if (L.any_global) {
        a.gws = (unsigned char *)ctx->buf("labels_ws", L.gws, &rc);
        if (rc != BPMX_OK) return rc;
    }
    LAUNCH(ctx, s, "k_labels", k_labels, dim3(L.grid), dim3(LABELS_T), L.lds, s, a);
    return BPMX_OK;
}

/* the scores behind the labels: one launch sized by the plan */
int score_stage(bpmx_ctx *ctx, const ScorePlan &S, int32_t n_files, const bpmx_score_params &P, const bpmx_packed &t,
                const bpmx_labels_out &l, const bpmx_ref_marks &r, const bpmx_score_out &o, hipStream_t s) {
    int rc = BPMX_OK;
    ScoreArgs a{};
    a.n_files = n_files; a.cap = t.cap_peaks; a.cap_ref = r.cap_ref; a.lds = S.lds; a.fixed = S.fixed;
    a.pk_off = t.pk_off;
    a.lb_time = l.lb_time; a.lb_type = l.lb_type; a.n_labels = l.n_labels; a.l_status = l.status;
    a.rf_off = r.rf_off; a.rf_ms = r.rf_ms; a.rf_type = r.rf_type;
    a.P = P; a.O = o;
    if (S.any_global) {
        a.gws = (unsigned char *)ctx->buf("score_ws", S.gws, &rc);
        if (rc != BPMX_OK) return rc;
    }
    LAUNCH(ctx, s, "k_score", k_score, dim3(S.grid), dim3(SCORE_T), S.lds, s, a);
    return BPMX_OK;
}

/* a person's marks as tables, beats and curve: three launches sized by the plan */
int marks_stage(bpmx_ctx *ctx, const MarksPlan &M, int32_t n_files, int32_t sr, const bpmx_marks_params &P,
                const bpmx_ref_marks &r, const int64_t *nd, const bpmx_packed &t, const bpmx_beats_out &b,
                int32_t *gap, int32_t *record, hipStream_t s) {
    int rc = BPMX_OK;
    MarksArgs a{};
    a.n_files = n_files; a.sr = sr; a.cap = t.cap_peaks; a.cap_ref = r.cap_ref; a.lds_n = M.lds_n; a.fixed = M.fixed;
    a.window_sec = P.smoothing_window_sec;
    a.rf_off = r.rf_off; a.rf_ms = r.rf_ms; a.rf_type = r.rf_type; a.nd = nd;
    unsigned char *rows = (unsigned char *)ctx->buf("marks_rows", M.rows, &rc);
    if (rc != BPMX_OK) return rc;
    a.k_idx = (int32_t *)rows; a.r_idx = (int32_t *)(rows + M.o_ridx);
    a.k_type = (int8_t *)(rows + M.o_ktype); a.r_tag = (int8_t *)(rows + M.o_rtag);
    a.cnt = (int32_t *)(rows + M.o_cnt);
    if (M.any_global) {
        a.gws = (unsigned char *)ctx->buf("marks_ws", M.gws, &rc);
        if (rc != BPMX_OK) return rc;
    }
    a.pk_off = t.pk_off; a.pk_idx = t.pk_idx; a.pk_env = t.pk_env; a.pk_floor = t.pk_floor;
    a.B = b; a.gap = gap; a.record = record;
    LAUNCH(ctx, s, "k_marks_rows", k_marks_rows, dim3(M.grid), dim3(MARKS_T), 0, s, a);
    LAUNCH(ctx, s, "k_marks_scan", k_marks_scan, dim3(1), dim3(MARKS_T), 0, s, a);
    LAUNCH(ctx, s, "k_marks_finish", k_marks_finish, dim3(M.grid), dim3(MARKS_T), M.lds, s, a);
    return BPMX_OK;
}

}  // namespace

extern "C" {

int bpmx_abi_version(void) { return BPMX_ABI_VERSION; }

const char *bpmx_last_error(void) { return g_err.c_str(); }

int bpmx_create(int device, bpmx_ctx **out) {
    if (!out) return fail(BPMX_E_ARG, "out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(BPMX_E_NODEV, "no HIP device visible");
    if (device < 0 || device >= n) return fail(BPMX_E_ARG, "device index out of range");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(BPMX_E_NODEV, std::string("libbpmx is built for gfx950, device is ") + prop.gcnArchName);
    bpmx_ctx *c = new bpmx_ctx();
    c->device = device;
    *out = c;
    return BPMX_OK;
}

void bpmx_destroy(bpmx_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    for (auto &kv : ctx->bufs)
        if (kv.second.first) (void)hipFree(kv.second.first);
    for (auto &r : ctx->recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto e : ctx->pool) (void)hipEventDestroy(e);
    for (int i = 0; i < bpmx_ctx::NSIDE && !ctx->root; ++i) {   /* a pipeline sub-context borrows its root's */
        if (ctx->side[i]) (void)hipStreamDestroy(ctx->side[i]);
        if (ctx->side_join[i]) (void)hipEventDestroy(ctx->side_join[i]);
    }
    if (ctx->side_fork && !ctx->root) (void)hipEventDestroy(ctx->side_fork);
    if (ctx->stats_ev) (void)hipEventDestroy(ctx->stats_ev);
    for (bpmx_ctx *c : ctx->pipe_sub) bpmx_destroy(c);
    bpmx::longfft_free(ctx);
    if (ctx->pipe_env) (void)hipStreamDestroy(ctx->pipe_env);
    if (ctx->pipe_det) (void)hipStreamDestroy(ctx->pipe_det);
    for (auto e : ctx->pipe_ev) (void)hipEventDestroy(e);
    delete ctx;
}

int64_t bpmx_decimated_length(int64_t n_frames, int32_t ds) {
    if (ds < 1) ds = 1;
    return n_frames <= 0 ? 0 : (n_frames + ds - 1) / ds;
}

int64_t bpmx_plot_length(int64_t nd, int32_t factor) {
    if (nd <= 0) return 0;
    const int64_t kf = (factor > 1 && nd >= factor) ? factor : 1;
    return (nd + kf - 1) / kf;
}

void bpmx_synth_host(uint64_t seed, int64_t n_frames, int32_t fs, int32_t channels, int16_t *out) {
    const int cap = beats_cap(n_frames, fs);
    std::vector<int64_t> s1(cap), s2(cap);
    const int nb = bpmx_synth_beats(seed, n_frames, fs, s1.data(), s2.data(), cap);
    for (int64_t i = 0; i < n_frames; ++i)
        for (int c = 0; c < channels; ++c)
            out[i * channels + c] = bpmx_synth_sample(seed, c, i, fs, s1.data(), s2.data(), nb);
}

int bpmx_synth(bpmx_ctx *ctx, uint64_t seed0, int32_t n_files, const int64_t *frame_offsets, int32_t fs,
               int32_t channels, int16_t *pcm, void *stream) {
    if (!ctx || !frame_offsets || !pcm || n_files < 1 || fs < 4 || channels < 1)
        return fail(BPMX_E_ARG, "bpmx_synth: bad argument");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    std::vector<int64_t> geo(2 * (n_files + 1));
    int64_t acc = 0, maxn = 0;
    for (int f = 0; f <= n_files; ++f) {
        geo[f] = frame_offsets[f] - frame_offsets[0];
        if (f < n_files) {
            int64_t n = frame_offsets[f + 1] - frame_offsets[f];
            if (n < 0) return fail(BPMX_E_ARG, "bpmx_synth: frame offsets must be non-decreasing");
            geo[n_files + 1 + f] = acc;
            acc += beats_cap(n, fs);
            maxn = std::max(maxn, n);
        }
    }
    geo[n_files + 1 + n_files] = acc;
    int rc = BPMX_OK;
    int64_t *dgeo = (int64_t *)ctx->buf("synth_geo", geo.size() * 8, &rc);
    int64_t *s1 = (int64_t *)ctx->buf("synth_s1", (size_t)acc * 8, &rc);
    int64_t *s2 = (int64_t *)ctx->buf("synth_s2", (size_t)acc * 8, &rc);
    int32_t *nb = (int32_t *)ctx->buf("synth_nb", (size_t)n_files * 4, &rc);
    if (rc != BPMX_OK) return rc;
    HIP_TRY(hipMemcpyAsync(dgeo, geo.data(), geo.size() * 8, hipMemcpyHostToDevice, s));
    const int64_t *foff = dgeo, *boff = dgeo + n_files + 1;
    int16_t *base = pcm + frame_offsets[0] * channels;
    LAUNCH(ctx, s, "k_synth_beats", k_synth_beats, dim3((n_files + 63) / 64), dim3(64), 0, s, seed0, n_files, foff,
           boff, fs, s1, s2, nb);
    int gx = (int)std::min<int64_t>((maxn + 255) / 256, 512);
    LAUNCH(ctx, s, "k_synth_pcm", k_synth_pcm, dim3(std::max(gx, 1), n_files), dim3(256), 0, s, seed0, n_files,
           foff, boff, fs, channels, s1, s2, nb, base);
    return BPMX_OK;
}

int bpmx_profile(bpmx_ctx *ctx, int on) {
    if (!ctx) return fail(BPMX_E_ARG, "ctx is NULL");
    ctx->prof = on != 0;
    if (on) {
        ctx->totals.clear();
        /* events created now, not inside the profiled launches (hipEventCreate
         * on the launch path leaves the GPU waiting on the host) */
        HIP_TRY(hipSetDevice(ctx->device));
        while (ctx->pool.size() < 4096) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            ctx->pool.push_back(e);
        }
    }
    return BPMX_OK;
}

int bpmx_profile_only(bpmx_ctx *ctx, const char *label) {
    if (!ctx) return fail(BPMX_E_ARG, "ctx is NULL");
    ctx->prof_only = label ? label : "";
    return BPMX_OK;
}

int bpmx_profile_read(bpmx_ctx *ctx, char *buf, int len) {
    if (!ctx) return fail(BPMX_E_ARG, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    for (auto &r : ctx->recs) {
        HIP_TRY(hipEventSynchronize(r.b));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, r.a, r.b));
        auto &t = ctx->totals[r.name];
        t.first += 1;
        t.second += ms;
        ctx->pool.push_back(r.a);
        ctx->pool.push_back(r.b);
    }
    ctx->recs.clear();
    std::string s;
    char line[256];
    for (auto &kv : ctx->totals) {
        std::snprintf(line, sizeof line, "%s %ld %.6f\n", kv.first.c_str(), kv.second.first, kv.second.second);
        s += line;
    }
    if (buf && len > 0) {
        std::strncpy(buf, s.c_str(), (size_t)len - 1);
        buf[len - 1] = 0;
    }
    return (int)s.size();
}

int bpmx_stats(bpmx_ctx *ctx, int64_t *out, int n) {
    if (!ctx || !out || n < 0) return fail(BPMX_E_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(ctx->device));
    int64_t h[BPMX_NSTATS] = {};
    auto it = ctx->bufs.find("stats");
    if (it != ctx->bufs.end()) {
        if (ctx->stats_ev) HIP_TRY(hipEventSynchronize(ctx->stats_ev));
        HIP_TRY(hipMemcpy(h, it->second.first, sizeof h, hipMemcpyDeviceToHost));
    }
    for (int i = 0; i < n; ++i) out[i] = i < BPMX_NSTATS ? h[i] : 0;
    return BPMX_NSTATS;
}

/* ---------------------------------------------------------------------------
 * Pipelined run (bpmx_set_pipeline): the batch in `chunks` runs of whole
 * recordings.  Chunk k's envelope stage (native mode: the HBM-bound block
 * kernel and the per-recording transforms) runs on an internal stream that may
 * be restricted to `env_cus` CUs; its detection stages (quantiles, troughs,
 * noise floor, peaks: latency-bound per-recording kernels) run on the caller's
 * stream (or an internal one restricted to the other CUs) once its envelope is
 * done, while chunk k+1's envelope streams its PCM.  Each chunk slot has its
 * own contexts (scratch, geometry) for the two stages, so the only data the
 * streams share are the output arrays, ordered by events.  Outputs are those
 * of one run over the whole batch.
 * ------------------------------------------------------------------------- */
static int pipe_ready(bpmx_ctx *ctx, int K) {
    if ((int)ctx->pipe_sub.size() < 2 * K) {
        while ((int)ctx->pipe_sub.size() < 2 * K) {
            bpmx_ctx *c = new bpmx_ctx();
            c->device = ctx->device;
            c->root = ctx;
            ctx->pipe_sub.push_back(c);
        }
    }
    while ((int)ctx->pipe_ev.size() < K + 1) {
        hipEvent_t e;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ctx->pipe_ev.push_back(e);
    }
    auto mk = [&](hipStream_t *st, int lo, int ncu) -> int {
        if (*st) return BPMX_OK;
        int total = 0;
        HIP_TRY(hipDeviceGetAttribute(&total, hipDeviceAttributeMultiprocessorCount, ctx->device));
        if (ncu <= 0 || ncu >= total) {
            HIP_TRY(hipStreamCreateWithFlags(st, hipStreamNonBlocking));
            return BPMX_OK;
        }
        /* mask bits [lo, lo + ncu): the driver deals the bits of a stream's CU
         * mask round-robin over the XCDs (bit c -> XCD c % 8, the (c / 8)-th CU
         * there), so a contiguous run of a multiple of 8 bits keeps the same
         * share of CUs on every XCD, as the workgroups are dealt too */
        std::vector<uint32_t> mask((total + 31) / 32, 0u);
        if (std::getenv("BPMX_CUMASK_PER_WORD")) {
            /* diagnostic: the other reading, one 32-bit word per XCD */
            const int X = (total + 31) / 32;
            for (int x = 0; x < X; ++x)
                for (int c = lo / X; c < (lo + ncu) / X && c < 32; ++c) mask[x] |= 1u << c;
        } else {
            for (int c = lo; c < lo + ncu && c < total; ++c) mask[c / 32] |= 1u << (c % 32);
        }
        HIP_TRY(hipExtStreamCreateWithCUMask(st, (uint32_t)mask.size(), mask.data()));
        return BPMX_OK;
    };
    int rc = mk(&ctx->pipe_env, 0, ctx->pipe_env_cus);
    if (rc != BPMX_OK) return rc;
    if (ctx->pipe_det_cus > 0 && (rc = mk(&ctx->pipe_det, ctx->pipe_env_cus, ctx->pipe_det_cus)) != BPMX_OK) return rc;
    return BPMX_OK;
}

static size_t dtype_bytes(int dt) {
    switch (dt) {
    case BPMX_DT_U8: return 1;
    case BPMX_DT_I16: return 2;
    case BPMX_DT_I24: return 3;
    case BPMX_DT_F64: return 8;
    default: return 4;
    }
}

static int run_pipelined(bpmx_ctx *ctx, const bpmx_params *P, const bpmx_batch *B, const bpmx_out *O,
                         hipStream_t s) {
    const int F = B->n_files;
    const int K = std::min(ctx->pipe_chunks, F);
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = pipe_ready(ctx, K);
    if (rc != BPMX_OK) return rc;
    if (P->options & BPMX_OPT_STATS) {
        int64_t *d_stats = (int64_t *)ctx->buf("stats", BPMX_NSTATS * 8, &rc);
        if (rc != BPMX_OK) return rc;
        HIP_TRY(hipMemsetAsync(d_stats, 0, BPMX_NSTATS * 8, s));
    }
    /* chunk boundaries by frames (recordings are whole), decimated offsets */
    const int64_t *fo = B->frame_offsets;
    const int64_t total = fo[F] - fo[0];
    std::vector<int> fb(K + 1, F);
    fb[0] = 0;
    for (int k = 1, f = 0; k < K; ++k) {
        const int64_t want = fo[0] + total * k / K;
        while (f < F && fo[f] < want) ++f;
        fb[k] = std::max(fb[k - 1] + 1, std::min(f, F - (K - k)));
    }
    std::vector<int64_t> doff(F + 1, 0);
    for (int f = 0; f < F; ++f) doff[f + 1] = doff[f] + bpmx_decimated_length(fo[f + 1] - fo[f], P->ds);
    /* the envelope stream starts after everything already queued on the caller's stream */
    hipEvent_t start = ctx->pipe_ev[K];
    HIP_TRY(hipEventRecord(start, s));
    HIP_TRY(hipStreamWaitEvent(ctx->pipe_env, start, 0));
    if (ctx->pipe_det) HIP_TRY(hipStreamWaitEvent(ctx->pipe_det, start, 0));
    const size_t fbytes = dtype_bytes(P->dtype) * (size_t)P->channels;
    bpmx_params pe = *P, pd = *P;
    pe.stages = BPMX_STAGE_ENVELOPE;
    pd.stages = P->stages & ~BPMX_STAGE_ENVELOPE;
    for (int k = 0; k < K; ++k) {
        const int f0 = fb[k], f1 = fb[k + 1];
        bpmx_batch b;
        b.n_files = f1 - f0;
        b.reserved = 0;
        b.pcm = (const char *)B->pcm + (size_t)(fo[f0] - fo[0]) * fbytes;
        b.frame_offsets = fo + f0;
        const int64_t d0 = doff[f0];
        bpmx_out o;
        o.env = O->env + d0;
        o.floor = O->floor ? O->floor + d0 : nullptr;
        o.y = O->y ? O->y + d0 : nullptr;
        o.troughs = O->troughs ? O->troughs + d0 : nullptr;
        o.peaks = O->peaks ? O->peaks + d0 : nullptr;
        o.n_troughs = O->n_troughs + f0;
        o.n_peaks = O->n_peaks + f0;
        o.flags = O->flags + f0;
        o.n_raw_troughs = O->n_raw_troughs ? O->n_raw_troughs + f0 : nullptr;
        if ((rc = run_impl(ctx->pipe_sub[2 * k], &pe, &b, &o, ctx->pipe_env, true)) != BPMX_OK) return rc;
        HIP_TRY(hipEventRecord(ctx->pipe_ev[k], ctx->pipe_env));
        /* detection: the restricted stream while later envelopes run, the
         * caller's stream for the last chunk (every CU free by then) */
        hipStream_t sd = (ctx->pipe_det && k + 1 < K) ? ctx->pipe_det : s;
        HIP_TRY(hipStreamWaitEvent(sd, ctx->pipe_ev[k], 0));
        if (pd.stages && (rc = run_impl(ctx->pipe_sub[2 * k + 1], &pd, &b, &o, sd, true)) != BPMX_OK) return rc;
    }
    if (ctx->pipe_det) {
        /* the caller's stream completes after every chunk's detection */
        hipEvent_t done = ctx->pipe_ev[K];
        HIP_TRY(hipEventRecord(done, ctx->pipe_det));
        HIP_TRY(hipStreamWaitEvent(s, done, 0));
    }
    return BPMX_OK;
}

int bpmx_set_pipeline(bpmx_ctx *ctx, int chunks, int env_cus, int det_cus) {
    if (!ctx || ctx->root) return fail(BPMX_E_ARG, "bad context");
    if (chunks < 0 || chunks > 64 || env_cus < 0 || det_cus < 0) return fail(BPMX_E_ARG, "bad pipeline shape");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipDeviceSynchronize());
    if (env_cus != ctx->pipe_env_cus || det_cus != ctx->pipe_det_cus) {
        if (ctx->pipe_env) (void)hipStreamDestroy(ctx->pipe_env);
        if (ctx->pipe_det) (void)hipStreamDestroy(ctx->pipe_det);
        ctx->pipe_env = ctx->pipe_det = nullptr;
    }
    ctx->pipe_chunks = chunks;
    ctx->pipe_env_cus = env_cus;
    ctx->pipe_det_cus = det_cus;
    return BPMX_OK;
}

int bpmx_run_ordered(bpmx_ctx *ctx, const bpmx_params *P, const bpmx_batch *B, const bpmx_out *O,
                     const bpmx_peak_order *order, void *stream) {
    if (!order) return bpmx_run(ctx, P, B, O, stream);
    for (int s = 0; s < 2; ++s) {
        if ((order->cand[s] != nullptr) != (order->n_cand[s] != nullptr))
            return fail(BPMX_E_ARG, "bpmx_peak_order: cand and n_cand go together");
        if ((order->rank[s] != nullptr) != (order->use_rank[s] != nullptr))
            return fail(BPMX_E_ARG, "bpmx_peak_order: rank and use_rank go together");
    }
    if (P && (P->options & BPMX_OPT_STATS)) return fail(BPMX_E_ARG, "bpmx_run_ordered: no BPMX_OPT_STATS");
    return run_impl(ctx, P, B, O, stream, false, order);
}

int bpmx_run(bpmx_ctx *ctx, const bpmx_params *P, const bpmx_batch *B, const bpmx_out *O, void *stream) {
    int rc;
    if (ctx && P && B && O && !ctx->root && ctx->pipe_chunks >= 2 && B->n_files >= 2 * ctx->pipe_chunks &&
        P->mode != BPMX_MODE_RECTIFIED &&        /* rectified mode is not pipelined */
        (P->stages & BPMX_STAGE_ENVELOPE) && (P->stages & (BPMX_STAGE_FLOOR | BPMX_STAGE_PEAKS)) &&
        B->frame_offsets && B->pcm && O->env && O->n_troughs && O->n_peaks && O->flags)
        rc = run_pipelined(ctx, P, B, O, (hipStream_t)stream);
    else
        rc = run_impl(ctx, P, B, O, stream, false);
    if (rc == BPMX_OK && (P->options & BPMX_OPT_STATS)) {
        /* bpmx_stats waits for this context-owned event, not for the caller's
         * stream, which the caller may destroy in between */
        if (!ctx->stats_ev) HIP_TRY(hipEventCreateWithFlags(&ctx->stats_ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(ctx->stats_ev, (hipStream_t)stream));
    }
    return rc;
}

int bpmx_pack(bpmx_ctx *ctx, int32_t n_files, const int64_t *frame_offsets, int32_t ds, const bpmx_out *in,
              const bpmx_packed *out, void *stream) {
    if (!ctx || !frame_offsets || !in || !out) return fail(BPMX_E_ARG, "bpmx_pack: NULL argument");
    const int F = n_files;
    if (F < 1 || ds < 1) return fail(BPMX_E_ARG, "bpmx_pack: bad n_files/ds");
    const bool tab[2] = {out->pk_off != nullptr, out->tr_off != nullptr};
    const bool y16 = out->y16 != nullptr;
    if (!tab[0] && !tab[1] && !y16) return fail(BPMX_E_ARG, "bpmx_pack: nothing to pack");
    if (tab[0] && (!in->peaks || !in->n_peaks || !in->env || !in->floor || !out->pk_idx || !out->pk_env ||
                   !out->pk_floor || out->cap_peaks < 0))
        return fail(BPMX_E_ARG, "bpmx_pack: the peak table needs peaks, n_peaks, env, floor and its three arrays");
    if (tab[1] && (!in->troughs || !in->n_troughs || !in->env || !out->tr_idx || !out->tr_env || out->cap_troughs < 0))
        return fail(BPMX_E_ARG, "bpmx_pack: the trough table needs troughs, n_troughs, env and its two arrays");
    if (y16 && (!in->y || !out->y_max)) return fail(BPMX_E_ARG, "bpmx_pack: y16 needs y and y_max");
    std::vector<int64_t> doff((size_t)F + 1);
    int64_t maxnd = 0;
    doff[0] = 0;
    for (int f = 0; f < F; ++f) {
        const int64_t n = frame_offsets[f + 1] - frame_offsets[f];
        if (n < 0) return fail(BPMX_E_ARG, "frame offsets must be non-decreasing");
        const int64_t nd = bpmx_decimated_length(n, ds);
        if (nd >= (int64_t)INT_MAX / 2) return fail(BPMX_E_LIMIT, "recording too long");
        doff[f + 1] = doff[f] + nd;
        maxnd = std::max(maxnd, nd);
    }
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    int rc = BPMX_OK;
    bool grew = false;
    int64_t *d_doff = (int64_t *)ctx->buf("pack_geo", doff.size() * 8, &rc, &grew);
    if (rc != BPMX_OK) return rc;
    if (grew || doff != ctx->pack_key) {
        /* stream-ordered: launches of an earlier pack still read the old offsets */
        ctx->pack_key.swap(doff);
        HIP_TRY(hipMemcpyAsync(d_doff, ctx->pack_key.data(), ctx->pack_key.size() * 8, hipMemcpyHostToDevice, s));
    }
    if (tab[0] || tab[1]) {
        PackArgs a{};
        a.doff = d_doff; a.n_files = F; a.env = in->env; a.floor = in->floor;
        if (tab[0]) {
            a.cnt[0] = in->n_peaks; a.idx[0] = in->peaks; a.off[0] = out->pk_off; a.cap[0] = out->cap_peaks;
            a.oidx[0] = out->pk_idx; a.oenv[0] = out->pk_env; a.ofloor = out->pk_floor;
        }
        if (tab[1]) {
            a.cnt[1] = in->n_troughs; a.idx[1] = in->troughs; a.off[1] = out->tr_off; a.cap[1] = out->cap_troughs;
            a.oidx[1] = out->tr_idx; a.oenv[1] = out->tr_env;
        }
        LAUNCH(ctx, s, "k_pack_scan", k_pack_scan, dim3(2), dim3(PK_SCAN_T), 0, s, a);
        LAUNCH(ctx, s, "k_pack_gather", k_pack_gather, dim3(F, 2), dim3(PK_GATHER_T), 0, s, a);
    }
    if (y16) {
        Y16Args a{};
        a.doff = d_doff; a.y = in->y; a.ymax = (unsigned long long *)out->y_max; a.y16 = out->y16;
        HIP_TRY(hipMemsetAsync(out->y_max, 0, (size_t)F * 8, s));
        /* a few elements (quant: pairs) per thread; the second grid dimension is a 16-bit one */
        const unsigned gm = (unsigned)std::min<int64_t>(std::max<int64_t>((maxnd + PK_Y16_T * 8 - 1) / (PK_Y16_T * 8), 1), 65535);
        LAUNCH(ctx, s, "k_y16_max", k_y16_max, dim3(F, gm), dim3(PK_Y16_T), 0, s, a);
        LAUNCH(ctx, s, "k_y16_quant", k_y16_quant, dim3(F, gm), dim3(PK_Y16_T), 0, s, a);
    }
    return BPMX_OK;
}

int bpmx_set_options(bpmx_ctx *ctx, int32_t options) {
    if (!ctx) return fail(BPMX_E_ARG, "bpmx_set_options: ctx is NULL");
    ctx->options = options;
    return BPMX_OK;
}

namespace {
/* bpmx_beats_device and bpmx_beats_device_ex (`who` names the caller in the messages) */
int beats_device(const char *who, bpmx_ctx *ctx, int32_t n_files, int32_t sr, const bpmx_beat_params *params,
                 double start_bpm_hint, const bpmx_packed *in, const int32_t *flags, const bpmx_beats_out *out,
                 const double *hints, const bpmx_trace_out *trace, void *stream) {
    const std::string w(who);
    if (!ctx || !params || !in || !out) return fail(BPMX_E_ARG, w + ": NULL argument");
    if (n_files < 1 || sr < 1) return fail(BPMX_E_ARG, w + ": bad n_files/sr");
    if (!in->pk_off || !in->pk_idx || !in->pk_env || !in->pk_floor || in->cap_peaks < 0 ||
        in->cap_peaks >= (int64_t)INT_MAX)
        return fail(BPMX_E_ARG, w + ": needs the peak table (pk_off, pk_idx, pk_env, pk_floor) and "
                                    "0 <= cap_peaks < 2^31");
    if (!out->final_idx || !out->n_final || !out->bpm_t || !out->bpm || !out->n_bpm || !out->status)
        return fail(BPMX_E_ARG, w + ": final_idx, n_final, bpm_t, bpm, n_bpm and status are required");
    if (trace && (!trace->record || !trace->code || !trace->lt_pos || !trace->lt_bpm || !trace->n_lt ||
                  !trace->dev_t || !trace->dev || !trace->gap))
        return fail(BPMX_E_ARG, w + ": every pointer of bpmx_trace_out is required");
    HIP_TRY(hipSetDevice(ctx->device));
    BeatsArgs a{};
    a.n_files = n_files; a.sr = sr; a.cap = in->cap_peaks;
    a.pk_off = in->pk_off; a.pk_idx = in->pk_idx; a.pk_env = in->pk_env; a.pk_floor = in->pk_floor;
    a.flags = flags; a.hint = start_bpm_hint; a.P = *params;
    a.final_idx = out->final_idx; a.n_final = out->n_final; a.bpm_t = out->bpm_t; a.bpm = out->bpm;
    a.n_bpm = out->n_bpm; a.pass = out->pass; a.tags = out->tags; a.status = out->status;
    const BeatsPlan plan = beats_plan(n_files, in->cap_peaks, ctx->options);
    if (!hints && !trace) return beats_stage(ctx, plan, a, (hipStream_t)stream);
    BeatsExArgs e{};
    e.hints = hints;
    if (trace) {
        e.record = trace->record; e.code = trace->code; e.lt_pos = trace->lt_pos; e.lt_bpm = trace->lt_bpm;
        e.n_lt = trace->n_lt; e.dev_t = trace->dev_t; e.dev = trace->dev; e.gap = trace->gap;
    }
    return beats_stage(ctx, plan, a, (hipStream_t)stream, &e);
}
}  // namespace

int bpmx_beats_device(bpmx_ctx *ctx, int32_t n_files, int32_t sr, const bpmx_beat_params *params,
                      double start_bpm_hint, const bpmx_packed *in, const int32_t *flags,
                      const bpmx_beats_out *out, void *stream) {
    return beats_device("bpmx_beats_device", ctx, n_files, sr, params, start_bpm_hint, in, flags, out, nullptr,
                        nullptr, stream);
}

int bpmx_beats_device_ex(bpmx_ctx *ctx, int32_t n_files, int32_t sr, const bpmx_beat_params *params,
                         double start_bpm_hint, const bpmx_packed *in, const int32_t *flags,
                         const bpmx_beats_out *out, const double *hints, const bpmx_trace_out *trace,
                         void *stream) {
    return beats_device("bpmx_beats_device_ex", ctx, n_files, sr, params, start_bpm_hint, in, flags, out, hints,
                        trace, stream);
}

int bpmx_pack_trough_floor(bpmx_ctx *ctx, const bpmx_out *in, const int64_t *frame_offsets, int32_t n_files,
                           int32_t ds, const bpmx_packed *tables, double *tr_floor, void *stream) {
    if (!ctx || !in || !frame_offsets || !tables || !tr_floor)
        return fail(BPMX_E_ARG, "bpmx_pack_trough_floor: NULL argument");
    if (n_files < 1 || ds < 1) return fail(BPMX_E_ARG, "bpmx_pack_trough_floor: bad n_files/ds");
    if (!in->floor || !tables->tr_off || !tables->tr_idx || tables->cap_troughs < 0)
        return fail(BPMX_E_ARG, "bpmx_pack_trough_floor: needs floor and the trough table (tr_off, tr_idx, "
                                "cap_troughs >= 0)");
    std::vector<int64_t> doff((size_t)n_files + 1);
    doff[0] = 0;
    for (int f = 0; f < n_files; ++f) {
        const int64_t n = frame_offsets[f + 1] - frame_offsets[f];
        if (n < 0) return fail(BPMX_E_ARG, "frame offsets must be non-decreasing");
        const int64_t nd = bpmx_decimated_length(n, ds);
        if (nd >= (int64_t)INT_MAX / 2) return fail(BPMX_E_LIMIT, "recording too long");
        doff[f + 1] = doff[f] + nd;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    int rc = BPMX_OK;
    bool grew = false;
    /* bpmx_pack's offsets buffer and its key: behind the pack of the same batch nothing is copied */
    int64_t *d_doff = (int64_t *)ctx->buf("pack_geo", doff.size() * 8, &rc, &grew);
    if (rc != BPMX_OK) return rc;
    if (grew || doff != ctx->pack_key) {
        ctx->pack_key.swap(doff);
        HIP_TRY(hipMemcpyAsync(d_doff, ctx->pack_key.data(), ctx->pack_key.size() * 8, hipMemcpyHostToDevice, s));
    }
    TroughFloorArgs a{};
    a.doff = d_doff; a.tr_off = tables->tr_off; a.tr_idx = tables->tr_idx; a.floor = in->floor;
    a.cap = tables->cap_troughs; a.out = tr_floor;
    LAUNCH(ctx, s, "k_pack_trough_floor", k_pack_trough_floor, dim3(n_files), dim3(PK_GATHER_T), 0, s, a);
    return BPMX_OK;
}

int bpmx_pack_plot(bpmx_ctx *ctx, int32_t n_files, const int64_t *frame_offsets, int32_t ds, int32_t factor,
                   const bpmx_out *in, double *pl_env, double *pl_floor, int64_t cap, void *stream) {
    if (!ctx || !frame_offsets || !in || !pl_env) return fail(BPMX_E_ARG, "bpmx_pack_plot: NULL argument");
    const int64_t F = n_files;
    if (F < 1 || ds < 1 || cap < 0) return fail(BPMX_E_ARG, "bpmx_pack_plot: bad n_files/ds/cap");
    if (!in->env || (pl_floor && !in->floor)) return fail(BPMX_E_ARG, "bpmx_pack_plot: needs env, and floor for pl_floor");
    /* doff | poff | boff | kf | file of each workgroup (PlotArgs) */
    std::vector<int64_t> geo((size_t)(4 * F + 3));
    int64_t *doff = geo.data(), *poff = doff + F + 1, *boff = poff + F + 1, *kfs = boff + F + 1;
    doff[0] = poff[0] = boff[0] = 0;
    for (int64_t f = 0; f < F; ++f) {
        const int64_t n = frame_offsets[f + 1] - frame_offsets[f];
        if (n < 0) return fail(BPMX_E_ARG, "frame offsets must be non-decreasing");
        const int64_t nd = bpmx_decimated_length(n, ds);
        if (nd >= (int64_t)INT_MAX / 2) return fail(BPMX_E_LIMIT, "recording too long");
        const int64_t np = bpmx_plot_length(nd, factor);
        kfs[f] = (factor > 1 && nd >= factor) ? factor : 1;
        doff[f + 1] = doff[f] + nd;
        poff[f + 1] = poff[f] + np;
        boff[f + 1] = boff[f] + (np + PK_PLOT_CHUNK - 1) / PK_PLOT_CHUNK;
    }
    const int64_t total = poff[F], nb = boff[F];
    if (total > cap)
        return fail(BPMX_E_ARG, "bpmx_pack_plot: " + std::to_string(total) + " kept entries exceed cap " +
                                    std::to_string(cap));
    if (nb >= (int64_t)INT_MAX) return fail(BPMX_E_LIMIT, "bpmx_pack_plot: batch too long");
    if (nb == 0) return BPMX_OK;
    geo.resize((size_t)(4 * F + 3 + nb));
    boff = geo.data() + 2 * (F + 1);
    for (int64_t f = 0; f < F; ++f)
        for (int64_t b = boff[f]; b < boff[f + 1]; ++b) geo[(size_t)(4 * F + 3 + b)] = f;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    int rc = BPMX_OK;
    bool grew = false;
    int64_t *d_geo = (int64_t *)ctx->buf("plot_geo", geo.size() * 8, &rc, &grew);
    if (rc != BPMX_OK) return rc;
    if (grew || geo != ctx->plot_key) {
        /* stream-ordered: launches of an earlier call still read the old geometry */
        ctx->plot_key.swap(geo);
        HIP_TRY(hipMemcpyAsync(d_geo, ctx->plot_key.data(), ctx->plot_key.size() * 8, hipMemcpyHostToDevice, s));
    }
    PlotArgs a{};
    a.geo = d_geo; a.n_files = n_files;
    a.src[0] = in->env; a.dst[0] = pl_env;
    a.src[1] = in->floor; a.dst[1] = pl_floor;
    LAUNCH(ctx, s, "k_pack_plot", k_pack_plot, dim3((unsigned)nb, pl_floor ? 2 : 1), dim3(PK_PLOT_T), 0, s, a);
    return BPMX_OK;
}

int bpmx_metrics_device(bpmx_ctx *ctx, int32_t n_files, int32_t sr, const bpmx_metric_params *params,
                        int64_t epoch_us, const bpmx_packed *tables, const bpmx_beats_out *beats,
                        const bpmx_metrics_out *out, void *stream) {
    if (!ctx || !params || !tables || !beats || !out) return fail(BPMX_E_ARG, "bpmx_metrics_device: NULL argument");
    if (n_files < 1 || sr < 1) return fail(BPMX_E_ARG, "bpmx_metrics_device: bad n_files/sr");
    if (params->hrv_window_size_beats < 2 || params->hrv_step_size_beats < 1)
        return fail(BPMX_E_ARG, "bpmx_metrics_device: needs hrv_window_size_beats >= 2 and hrv_step_size_beats >= 1");
    if (!tables->pk_off || tables->cap_peaks < 0 || tables->cap_peaks >= (int64_t)INT_MAX)
        return fail(BPMX_E_ARG, "bpmx_metrics_device: needs pk_off and 0 <= cap_peaks < 2^31");
    if (!beats->final_idx || !beats->n_final || !beats->bpm_t || !beats->bpm || !beats->n_bpm || !beats->status)
        return fail(BPMX_E_ARG, "bpmx_metrics_device: the beats' final_idx, n_final, bpm_t, bpm, n_bpm and status "
                                "are required");
    if (!out->hrv_time || !out->hrv_rmssdc || !out->hrv_sdnn || !out->hrv_bpm || !out->n_hrv || !out->inc_a ||
        !out->inc_b || !out->dec_a || !out->dec_b || !out->inc_slope || !out->inc_dur || !out->dec_slope ||
        !out->dec_dur || !out->n_inc || !out->n_dec || !out->record || !out->status)
        return fail(BPMX_E_ARG, "bpmx_metrics_device: every pointer of bpmx_metrics_out is required");
    HIP_TRY(hipSetDevice(ctx->device));
    return metrics_stage(ctx, metrics_plan(n_files, tables->cap_peaks, ctx->options, params->hrv_window_size_beats),
                         n_files, sr, *params, epoch_us, *tables, *beats, *out, (hipStream_t)stream);
}

int bpmx_labels_device(bpmx_ctx *ctx, int32_t n_files, int32_t sr, const bpmx_label_params *params,
                       const bpmx_packed *tables, const bpmx_beats_out *beats, const int32_t *gap,
                       const bpmx_labels_out *out, void *stream) {
    if (!ctx || !params || !tables || !beats || !gap || !out)
        return fail(BPMX_E_ARG, "bpmx_labels_device: NULL argument (gap, the trace of bpmx_beats_device_ex, is required)");
    if (n_files < 1 || sr < 1) return fail(BPMX_E_ARG, "bpmx_labels_device: bad n_files/sr");
    if (!tables->pk_off || !tables->pk_idx || tables->cap_peaks < 0 || tables->cap_peaks >= (int64_t)INT_MAX)
        return fail(BPMX_E_ARG, "bpmx_labels_device: needs pk_off, pk_idx and 0 <= cap_peaks < 2^31");
    if (!beats->final_idx || !beats->n_final || !beats->bpm_t || !beats->bpm || !beats->n_bpm || !beats->tags ||
        !beats->status)
        return fail(BPMX_E_ARG, "bpmx_labels_device: the beats' final_idx, n_final, bpm_t, bpm, n_bpm, tags and "
                                "status are required");
    if (!out->lb_pos || !out->lb_type || !out->lb_time || !out->lb_bpm || !out->pr_s1 || !out->pr_s2 || !out->pr_dt ||
        !out->gr_id || !out->gr_first || !out->gr_last || !out->gr_s1 || !out->gr_pairs || !out->gr_dt ||
        !out->gr_bpm || !out->n_labels || !out->n_pairs || !out->n_groups || !out->record || !out->status)
        return fail(BPMX_E_ARG, "bpmx_labels_device: every pointer of bpmx_labels_out is required");
    HIP_TRY(hipSetDevice(ctx->device));
    return labels_stage(ctx, labels_plan(n_files, tables->cap_peaks, ctx->options), n_files, sr, *params, *tables,
                        *beats, gap, *out, (hipStream_t)stream);
}

int bpmx_score_device(bpmx_ctx *ctx, int32_t n_files, const bpmx_score_params *params, const bpmx_packed *tables,
                      const bpmx_labels_out *labels, const bpmx_ref_marks *ref, const bpmx_score_out *out,
                      void *stream) {
    if (!ctx || !params || !tables || !labels || !ref || !out)
        return fail(BPMX_E_ARG, "bpmx_score_device: NULL argument");
    if (n_files < 0) return fail(BPMX_E_ARG, "bpmx_score_device: bad n_files");
    if (params->tol_ms < 0) return fail(BPMX_E_ARG, "bpmx_score_device: needs tol_ms >= 0");
    if ((int64_t)params->gap_ms <= 2 * (int64_t)params->tol_ms)
        return fail(BPMX_E_ARG, "bpmx_score_device: needs gap_ms > 2 * tol_ms (the labelled spans must stay apart)");
    if (n_files == 0) return BPMX_OK;
    if (!tables->pk_off || tables->cap_peaks < 0 || tables->cap_peaks >= (int64_t)INT_MAX)
        return fail(BPMX_E_ARG, "bpmx_score_device: needs pk_off and 0 <= cap_peaks < 2^31");
    if (!labels->lb_time || !labels->lb_type || !labels->n_labels || !labels->status)
        return fail(BPMX_E_ARG, "bpmx_score_device: the labels' lb_time, lb_type, n_labels and status are required");
    if (!ref->rf_off || ref->cap_ref < 0 || ref->cap_ref >= (int64_t)INT_MAX ||
        (ref->cap_ref > 0 && (!ref->rf_ms || !ref->rf_type)))
        return fail(BPMX_E_ARG, "bpmx_score_device: needs rf_off, 0 <= cap_ref < 2^31 and, with cap_ref > 0, rf_ms "
                                "and rf_type");
    const int rows = (out->sc_kind != nullptr) + (out->sc_ref != nullptr) + (out->rf_kind != nullptr) +
                     (out->rf_det != nullptr);
    if (rows != 0 && rows != 4)
        return fail(BPMX_E_ARG, "bpmx_score_device: sc_kind, sc_ref, rf_kind and rf_det are given together or not "
                                "at all");
    if (!out->record || !out->status) return fail(BPMX_E_ARG, "bpmx_score_device: record and status are required");
    HIP_TRY(hipSetDevice(ctx->device));
    return score_stage(ctx, score_plan(n_files, tables->cap_peaks, ref->cap_ref, ctx->options), n_files, *params,
                       *tables, *labels, *ref, *out, (hipStream_t)stream);
}

int bpmx_marks_device(bpmx_ctx *ctx, int32_t n_files, int32_t sr, const bpmx_marks_params *params,
                      const bpmx_ref_marks *marks, const int64_t *nd, const bpmx_packed *tables,
                      const bpmx_beats_out *beats, int32_t *gap, int32_t *record, void *stream) {
    if (!ctx || !params || !marks || !tables || !beats || !gap || !record)
        return fail(BPMX_E_ARG, "bpmx_marks_device: NULL argument (gap and record are required)");
    if (n_files < 0 || sr < 1) return fail(BPMX_E_ARG, "bpmx_marks_device: bad n_files/sr");
    if (!(params->smoothing_window_sec > 0))
        return fail(BPMX_E_ARG, "bpmx_marks_device: needs smoothing_window_sec > 0");
    if (n_files == 0) return BPMX_OK;
    if (!marks->rf_off || marks->cap_ref < 0 || marks->cap_ref >= (int64_t)INT_MAX ||
        (marks->cap_ref > 0 && (!marks->rf_ms || !marks->rf_type)))
        return fail(BPMX_E_ARG, "bpmx_marks_device: needs rf_off, 0 <= cap_ref < 2^31 and, with cap_ref > 0, rf_ms "
                                "and rf_type");
    if (!tables->pk_off || !tables->pk_idx || tables->cap_peaks < 0 || tables->cap_peaks >= (int64_t)INT_MAX)
        return fail(BPMX_E_ARG, "bpmx_marks_device: needs pk_off, pk_idx and 0 <= cap_peaks < 2^31");
    if (!beats->final_idx || !beats->n_final || !beats->bpm_t || !beats->bpm || !beats->n_bpm || !beats->tags ||
        !beats->status)
        return fail(BPMX_E_ARG, "bpmx_marks_device: the beats' final_idx, n_final, bpm_t, bpm, n_bpm, tags and "
                                "status are required");
    HIP_TRY(hipSetDevice(ctx->device));
    return marks_stage(ctx, marks_plan(n_files, marks->cap_ref, ctx->options), n_files, sr, *params, *marks, nd,
                       *tables, *beats, gap, record, (hipStream_t)stream);
}

int64_t bpmx_tempo_windows(int64_t nd, int32_t win, int32_t hop) { return tempo_windows(nd, win, hop); }

int bpmx_tempo_device(bpmx_ctx *ctx, int32_t n_files, const int64_t *frame_offsets, int32_t ds, int32_t sr,
                      const bpmx_tempo_params *params, const bpmx_out *in, const bpmx_tempo_out *out, void *stream) {
    if (!ctx || !frame_offsets || !params || !in || !out) return fail(BPMX_E_ARG, "bpmx_tempo_device: NULL argument");
    if (n_files < 0 || ds < 1 || sr < 1) return fail(BPMX_E_ARG, "bpmx_tempo_device: bad n_files/ds/sr");
    const TempoPlan G = tempo_plan(params->win, params->hop, params->kmin, params->kmax);
    if (G.status == BPMX_E_ARG)
        return fail(BPMX_E_ARG, "bpmx_tempo_device: needs hop >= 1, 2 <= kmin <= kmax and kmax + 1 < win");
    if (G.status != BPMX_OK)
        return fail(BPMX_E_LIMIT, "bpmx_tempo_device: the window and its lag range exceed a workgroup's LDS "
                                  "(8 * (win4 + kmax + 8 + 4 * (kmax - kmin + 4)) > " +
                                      std::to_string((int)TEMPO_LDS_MAX) + " bytes)");
    if (!(params->min_strength == params->min_strength) || params->start_windows < 0)
        return fail(BPMX_E_ARG, "bpmx_tempo_device: needs a min_strength that is not NaN and start_windows >= 0");
    if (n_files == 0) return BPMX_OK;
    if (!in->env) return fail(BPMX_E_ARG, "bpmx_tempo_device: needs env");
    if (!out->lag || !out->rho || !out->bpm || !out->n_valid || !out->n_strong || !out->median_bpm ||
        !out->mean_rho || !out->hint)
        return fail(BPMX_E_ARG, "bpmx_tempo_device: every pointer of bpmx_tempo_out is required");
    /* doff | woff */
    const size_t F = (size_t)n_files;
    std::vector<int64_t> geo(2 * (F + 1));
    int64_t *doff = geo.data(), *woff = doff + F + 1;
    doff[0] = woff[0] = 0;
    for (size_t f = 0; f < F; ++f) {
        const int64_t n = frame_offsets[f + 1] - frame_offsets[f];
        if (n < 0) return fail(BPMX_E_ARG, "frame offsets must be non-decreasing");
        const int64_t nd = bpmx_decimated_length(n, ds);
        if (nd >= (int64_t)INT_MAX / 2) return fail(BPMX_E_LIMIT, "recording too long");
        doff[f + 1] = doff[f] + nd;
        woff[f + 1] = woff[f] + tempo_windows(nd, params->win, params->hop);
    }
    const int64_t total = woff[F];
    if (total >= (int64_t)INT_MAX) return fail(BPMX_E_LIMIT, "bpmx_tempo_device: too many windows");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    int rc = BPMX_OK;
    bool grew = false;
    int64_t *d_geo = (int64_t *)ctx->buf("tempo_geo", geo.size() * 8, &rc, &grew);
    if (rc != BPMX_OK) return rc;
    if (grew || geo != ctx->tempo_key) {
        /* stream-ordered: launches of an earlier call still read the old geometry */
        ctx->tempo_key.swap(geo);
        HIP_TRY(hipMemcpyAsync(d_geo, ctx->tempo_key.data(), ctx->tempo_key.size() * 8, hipMemcpyHostToDevice, s));
    }
    TempoArgs a{};
    a.n_files = n_files; a.sr = sr; a.P = *params; a.G = G;
    a.doff = d_geo; a.woff = d_geo + F + 1; a.env = in->env; a.O = *out;
    if (total > 0) {
        if (G.lags == 5) {
            (void)hipFuncSetAttribute((const void *)k_tempo_valu<5>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TEMPO_LDS_MAX);
            LAUNCH(ctx, s, "k_tempo_valu", k_tempo_valu<5>, dim3((unsigned)total), dim3(TEMPO_T), G.lds, s, a);
        } else {
            (void)hipFuncSetAttribute((const void *)k_tempo_valu<7>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TEMPO_LDS_MAX);
            LAUNCH(ctx, s, "k_tempo_valu", k_tempo_valu<7>, dim3((unsigned)total), dim3(TEMPO_T), G.lds, s, a);
        }
    }
    LAUNCH(ctx, s, "k_tempo_record", k_tempo_record, dim3((unsigned)n_files), dim3(TEMPO_REC_T), 0, s, a);
    return BPMX_OK;
}

int64_t bpmx_hrvspec_windows(int64_t nd, int32_t win, int32_t hop) { return hrvspec_windows(nd, win, hop); }

int bpmx_hrvspec_device(bpmx_ctx *ctx, int32_t n_files, const int64_t *frame_offsets, int32_t ds, int32_t sr,
                        const bpmx_hrvspec_params *params, const bpmx_packed *tables, const bpmx_beats_out *beats,
                        const bpmx_hrvspec_out *out, void *stream) {
    if (!ctx || !frame_offsets || !params || !tables || !beats || !out)
        return fail(BPMX_E_ARG, "bpmx_hrvspec_device: NULL argument");
    if (n_files < 0 || ds < 1 || sr < 1) return fail(BPMX_E_ARG, "bpmx_hrvspec_device: bad n_files/ds/sr");
    const HrvspecPlan G = hrvspec_plan(*params);
    if (G.status == BPMX_E_ARG)
        return fail(BPMX_E_ARG, "bpmx_hrvspec_device: needs hop >= 1, 1 <= dmin <= dmax, min_intervals >= 3, "
                                "1 <= n_freq <= 1024, 0 <= a <= b <= n_freq for both bands, om0 and dom finite, "
                                "om0 > 0 and dom >= 0");
    if (G.status != BPMX_OK)
        return fail(BPMX_E_LIMIT, "bpmx_hrvspec_device: a window's intervals exceed a workgroup's LDS "
                                  "(32 * (win / dmin + 1) > " + std::to_string((int)HRVSPEC_LDS_MAX) + " bytes)");
    if (n_files == 0) return BPMX_OK;
    if (!tables->pk_off || tables->cap_peaks < 0 || tables->cap_peaks >= (int64_t)INT_MAX)
        return fail(BPMX_E_ARG, "bpmx_hrvspec_device: needs pk_off and 0 <= cap_peaks < 2^31");
    if (!beats->final_idx || !beats->n_final || !beats->status)
        return fail(BPMX_E_ARG, "bpmx_hrvspec_device: the beats' final_idx, n_final and status are required");
    if (!out->code || !out->n_rr || !out->lf_peak || !out->hf_peak || !out->t_mid || !out->var || !out->lf ||
        !out->hf || !out->record || !out->status)
        return fail(BPMX_E_ARG, "bpmx_hrvspec_device: every pointer of bpmx_hrvspec_out but q is required");
    const size_t F = (size_t)n_files;
    std::vector<int64_t> geo(F + 1);
    geo[0] = 0;
    for (size_t f = 0; f < F; ++f) {
        const int64_t n = frame_offsets[f + 1] - frame_offsets[f];
        if (n < 0) return fail(BPMX_E_ARG, "frame offsets must be non-decreasing");
        const int64_t nd = bpmx_decimated_length(n, ds);
        if (nd >= (int64_t)INT_MAX / 2) return fail(BPMX_E_LIMIT, "recording too long");
        geo[f + 1] = geo[f] + hrvspec_windows(nd, params->win, params->hop);
    }
    const int64_t total = geo[F];
    if (total >= (int64_t)INT_MAX) return fail(BPMX_E_LIMIT, "bpmx_hrvspec_device: too many windows");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    int rc = BPMX_OK;
    bool grew = false;
    int64_t *d_geo = (int64_t *)ctx->buf("hrvspec_geo", geo.size() * 8, &rc, &grew);
    if (rc != BPMX_OK) return rc;
    if (grew || geo != ctx->hrvspec_key) {
        /* stream-ordered: launches of an earlier call still read the old geometry */
        ctx->hrvspec_key.swap(geo);
        HIP_TRY(hipMemcpyAsync(d_geo, ctx->hrvspec_key.data(), ctx->hrvspec_key.size() * 8, hipMemcpyHostToDevice, s));
    }
    HrvspecArgs a{};
    a.n_files = n_files; a.sr = sr; a.cap = tables->cap_peaks; a.P = *params; a.G = G;
    a.woff = d_geo; a.pk_off = tables->pk_off;
    a.final_idx = beats->final_idx; a.n_final = beats->n_final; a.b_status = beats->status; a.O = *out;
    if (total > 0) {
        if (ctx->options & BPMX_OPT_HRVSPEC_DIRECT)
            LAUNCH(ctx, s, "k_hrvspec_direct", (k_hrvspec<1, 1, false>), dim3((unsigned)total), dim3(HRVSPEC_T), G.lds, s, a);
        else
            LAUNCH(ctx, s, "k_hrvspec", (k_hrvspec<HRVSPEC_B, HRVSPEC_PARTS, true>), dim3((unsigned)total), dim3(HRVSPEC_T), G.lds, s, a);
    }
    LAUNCH(ctx, s, "k_hrvspec_record", k_hrvspec_record, dim3((unsigned)n_files), dim3(HRVSPEC_REC_T), 0, s, a);
    return BPMX_OK;
}

}  // extern "C"
