/*
 * bpmx.h — C ABI of the MI355X-native heartbeat preprocessing + detection path.
 *
 * One shared library (bpm_analysis_amd/libbpmx.so, HIP for gfx950) behind the
 * reference's own operator surface for this path.  The reference has no
 * plugin/FFI layer of its own (pure Python); these entry points
 * replace, one for one, the computation inside:
 *
 *   bpmx_run(stages=ENVELOPE)  <- bpm_analysis.py:1007-1062  preprocess_audio
 *                                 (wavfile.read result -> mean(axis=1) -> [::ds]
 *                                  -> butter/filtfilt -> |x| rolling mean)
 *   bpmx_run(stages=FLOOR)     <- bpm_analysis.py:1064-1117  _calculate_dynamic_noise_floor
 *   bpmx_run(stages=PEAKS)     <- bpm_analysis.py:223-229    PeakClassifier._find_raw_peaks
 *   bpmx_run(stages=ALL)       <- the three above in sequence, as analyze_wav_file
 *                                 runs them (bpm_analysis.py:1731-1732, :89)
 *   bpmx_pack                  the results as per-peak / per-trough tables
 *   bpmx_beats_device          <- bpm_analysis.py:1734-1757  analyze_wav_file stages 2-5 on
 *                                 those tables (_run_preliminary_pass, PeakClassifier,
 *                                 _refine_and_correct_peaks, calculate_bpm_series)
 *   bpmx_beats_device_ex       the same with one start hint per file and the decision trace: the
 *                                 numbers behind analysis_data's debug strings, belief curve and
 *                                 deviation series (:64-330), for the reference's Debug_Log.md
 *   bpmx_pack_trough_floor     the floor at the packed troughs (the debug log prints it)
 *   bpmx_pack_plot             <- bpm_analysis.py:518-524  the plot's line traces: env and floor at every
 *                                 plot_downsample_factor-th sample
 *   bpmx_metrics_device        <- bpm_analysis.py:1701-1722  _calculate_final_metrics on the beats and
 *                                 the curve (HRV table, summary, HRR, slopes, inclines and declines)
 *   bpmx_labels_device         <- heartbeat_labeler.py  the labeler's output from the beat stages'
 *                                 decisions: the S1 / S2 table of <base>_labels.csv (:530-546), the
 *                                 S1-S2 pairs (:198-217), the groups and their statistics (:244-308)
 *   bpmx_score_device          (no counterpart in the reference: defined here)  the label rows scored
 *                                 against a person's corrected <base>_labels.csv: TP, SWAP, FP, FN
 *   bpmx_synth / bpmx_synth_host   deterministic synthetic recordings (bench/tests)
 *
 * Plain C types only.  PCM and result arrays are DEVICE pointers (HBM); the
 * per-file frame offsets are a HOST array.  A batch shares one sample rate,
 * dtype and channel count; lengths may be ragged.  Filter coefficients
 * (butter / lfilter_zi / sosfilt_zi) are designed on the host exactly as the
 * reference designs them and passed in bpmx_params.
 *
 * Thread-safety: one bpmx_ctx per thread (or per stream); bpmx_last_error is
 * thread-local.  Calls may come from a non-main thread (gui.py:181-183).
 */
#ifndef BPMX_H
#define BPMX_H

#include <stdint.h>

#include "bpmx_host.h" /* bpmx_beat_params, bpmx_beat_tag, bpmx_host_status (bpmx_beats_device) */

#ifdef __cplusplus
extern "C" {
#endif

/* Added within version 4 (no existing call changes): BPMX_MODE_RECTIFIED and
 * BPMX_OPT_RECT_SEQ; bpmx_labels_device and BPMX_OPT_LABELS_GLOBAL;
 * bpmx_score_device and BPMX_OPT_SCORE_GLOBAL; bpmx_marks_device and
 * BPMX_OPT_MARKS_GLOBAL; BPMX_DT_I24; bpmx_tempo_windows and bpmx_tempo_device;
 * bpmx_hrvspec_windows, bpmx_hrvspec_device and BPMX_OPT_HRVSPEC_DIRECT. */
#define BPMX_ABI_VERSION 4

/* sample formats of scipy.io.wavfile.read (bpm_analysis.py:1014) */
enum bpmx_dtype { BPMX_DT_U8 = 0, BPMX_DT_I16 = 1, BPMX_DT_I32 = 2, BPMX_DT_F32 = 3, BPMX_DT_F64 = 4,
                  BPMX_DT_I24 = 5 };
/* BPMX_DT_I24: packed 24-bit PCM as it lies in a WAV file: 3 bytes per element,
 * little-endian, two's complement, frames interleaved; pcm may have any byte
 * alignment and frame_offsets stay in frames.  In every mode and stage the
 * batch means exactly the BPMX_DT_I32 batch whose samples are v << 8, v the
 * sign-extended 24-bit value (what scipy.io.wavfile.read returns for the
 * file).  Nothing is read past the 16-byte boundary at or above the batch's
 * last byte. */

/* REFERENCE: the shipped pipeline, bit-exact (stride pick, b/a filtfilt at the
 *            decimated rate, rolling-mean envelope; bpm_analysis.py:1031-1054).
 * NATIVE:    the north_star ordering (sosfiltfilt at the native rate -> pick
 *            -> |Hilbert| -> rolling mean); envelope within 1e-9 relative of the
 *            scipy composition, detection stages identical.
 * RECTIFIED: the labeler's envelope of an already filtered WAV, bit-exact
 *            (heartbeat_labeler.py:48-67): the frame value as in the other
 *            modes, np.abs in its dtype (the most negative int16 / int32 stays
 *            itself, u8 is unchanged), no decimation and no filter, then
 *            pd.Series(a).rolling(fs // 10, min_periods=1, center=True).mean()
 *            with +-inf counted as NaN.  Rules of the mode:
 *              - ds must be 1 (sr == fs, Nd == N), else BPMX_E_ARG;
 *              - out.y must be NULL (there is no filtered signal), else BPMX_E_ARG;
 *              - a recording is active when it has >= 1 frame, as in a run that
 *                starts from env; there is no filtfilt pad, so BPMX_F_TOO_SHORT
 *                only marks an empty recording;
 *              - FLOOR and PEAKS run unchanged on that envelope at rate fs, with
 *                the limits of an env-level run of the same length and window;
 *              - bpmx_set_pipeline does not apply: the run is not pipelined.
 *            Integer PCM of one or two channels is computed from exact int64
 *            window sums in parallel; other inputs by the pandas recursion, one
 *            lane per recording (only meant to be right). */
enum bpmx_mode { BPMX_MODE_REFERENCE = 0, BPMX_MODE_NATIVE = 1, BPMX_MODE_RECTIFIED = 2 };

enum bpmx_stage {
    BPMX_STAGE_ENVELOPE = 1, /* PCM -> env (and y)        */
    BPMX_STAGE_FLOOR = 2,    /* env -> floor, troughs     */
    BPMX_STAGE_PEAKS = 4,    /* env, floor -> raw peaks   */
    BPMX_STAGE_ALL = 7
};

/* return codes */
enum bpmx_status {
    BPMX_OK = 0,
    BPMX_E_ARG = -1,     /* bad argument (message in bpmx_last_error) */
    BPMX_E_HIP = -2,     /* HIP runtime error */
    BPMX_E_LIMIT = -3,   /* a size exceeds what the kernels support */
    BPMX_E_NODEV = -4    /* no usable gfx950 device */
};

/* per-file result flags (bpmx_out.flags) */
enum bpmx_file_flag {
    BPMX_F_STATIC_FLOOR = 1, /* < 5 troughs: constant quantile floor, troughs unsanitised (:1073-1077) */
    BPMX_F_DRAFT_FLOOR = 2,  /* <= 2 sanitised troughs: draft floor kept (:1107-1110) */
    BPMX_F_NAN_FLOOR = 4,    /* all-NaN floor replaced by quantile(env, 0.1) (:1113-1115) */
    BPMX_F_TOO_SHORT = 8,    /* Nd <= 15: scipy filtfilt raises ValueError; no outputs (its slices of the
                                output arrays are left as they were; counts are 0) */
    BPMX_F_BAD_WINDOW = 16,  /* noise_window < min_periods and >= 5 troughs: pandas rolling() raises
                                ValueError (:1085); floor/peaks of this recording are not meaningful */
    /* find_peaks' distance filter visits candidates in np.argsort(height) order
     * (scipy/signal/_peak_finding.py:976-978), which is unstable: for equal
     * heights the order is numpy's implementation detail (x86-simd-sort on
     * AVX-512, introsort elsewhere).  bpmx keeps the stable order (the later
     * index first among equals) and sets these bits exactly when that choice
     * decided a removal: some candidate was removed by an equal-height kept one
     * with no strictly higher kept one within `distance`.  Without the bit the
     * indices are those of every argsort order, so the reference's; with it
     * they may differ from the reference's on that machine. */
    BPMX_F_TROUGH_TIE = 32,  /* in the trough search find_peaks(-env) (:1070) */
    BPMX_F_PEAK_TIE = 64,    /* in the raw-peak search find_peaks(env, height=floor) (:227) */
    /* the distance filter of that search visited the candidates in the order
     * the caller supplied (bpmx_run_ordered: np.argsort of the heights, as
     * scipy's _select_by_peak_distance does); the matching TIE bit is then
     * never set, since the order is the reference's and nothing is left open */
    BPMX_F_TROUGH_ORDERED = 128,
    BPMX_F_PEAK_ORDERED = 256
};

enum bpmx_option {
    BPMX_OPT_ROLLQ_MERGE = 1, /* force the sorted-union rolling quantile (test/diagnostic; default picks the
                                 wavelet-matrix kernel for recordings of <= 18432 decimated samples) */
    BPMX_OPT_NATIVE_F64 = 2,  /* native mode: f64 VALU block projections instead of the exact-integer
                                 matrix-core kernel (test/diagnostic) */
    BPMX_OPT_HILBERT_ROCFFT = 4, /* native mode: rocFFT R2C/C2R Hilbert instead of the fused in-LDS transform
                                    (test/diagnostic; recordings the fused kernel cannot plan always use it) */
    BPMX_OPT_DRAFT_FULL = 8,     /* compute the draft floor (first rolling quantile) in full for every recording
                                    instead of deciding troughs from its bounds first (test/diagnostic) */
    BPMX_OPT_ROLLQ_NOPRUNE = 16, /* wavelet-matrix rolling quantile over every sample, without first dropping
                                    the samples no window's quantile can reach (test/diagnostic) */
    BPMX_OPT_DRAFT_GLOBAL_RANK = 32, /* draft-floor bounds from the recording-wide segment order even for
                                       recordings of > 512 troughs (test/diagnostic; default ranks per window) */
    BPMX_OPT_ROLLQ_GLOBAL = 64,  /* force the global-memory sorted-union rolling quantile (test/diagnostic;
                                    default: only for windows beyond the LDS kernel on long recordings) */
    BPMX_OPT_NATIVE_DMA = 128,   /* native mode, int16 mono without the matrix-core path: the LDS-DMA f64
                                    block kernel (default for int16 stereo) instead of the register-prefetch one */
    BPMX_OPT_PEAKS_GLOBAL = 256, /* find_peaks by sample walks over global memory (k_find_peaks) for every
                                    recording instead of the LDS-resident extrema (test/diagnostic) */
    BPMX_OPT_HILBERT_R2C = 512,  /* native mode, recordings outside the fused Hilbert kernel: one rocFFT
                                    R2C/C2R plan per distinct length instead of the batched Bluestein
                                    transform (test/diagnostic) */
    BPMX_OPT_REF_SERIAL_MEAN = 1024, /* reference mode: form the rolling mean's outputs inside the sequential
                                        pass instead of from its running sums in parallel (test/diagnostic) */
    BPMX_OPT_STATS = 2048,           /* count the run's path decisions for bpmx_stats (diagnostic) */
    BPMX_OPT_HILBERT_BLUESTEIN = 4096, /* native mode, long recordings: rocFFT Bluestein instead of the exact-
                                         length four-step transform (test/diagnostic) */
    BPMX_OPT_REF_NOSPLIT = 8192,     /* reference mode: gather every decimated sample first, then the forward
                                        pass inside k_envelope_ref, instead of forward-pass row chunks
                                        overlapping the next chunks' gather on a side stream (diagnostic) */
    BPMX_OPT_BEATS_GLOBAL = 16384,   /* bpmx_beats_device (set with bpmx_set_options): every recording's
                                        workspace in global memory instead of LDS for the tables that fit
                                        there (test/diagnostic) */
    BPMX_OPT_METRICS_GLOBAL = 32768, /* bpmx_metrics_device (set with bpmx_set_options): every recording's
                                        workspace in global memory, the curve and beats read where they lie
                                        (test/diagnostic) */
    BPMX_OPT_RECT_SEQ = 65536,       /* rectified mode: the general route (the pandas recursion, one lane per
                                        recording) for every recording, also where the exact-integer route
                                        applies (test/diagnostic) */
    BPMX_OPT_SCORE_GLOBAL = 262144,  /* bpmx_score_device (set with bpmx_set_options): every recording's
                                        workspace in global memory instead of LDS (test/diagnostic) */
    BPMX_OPT_MARKS_GLOBAL = 524288,  /* bpmx_marks_device (set with bpmx_set_options): every recording's
                                        workspace in global memory instead of LDS (test/diagnostic) */
    BPMX_OPT_LABELS_GLOBAL = 131072, /* bpmx_labels_device (set with bpmx_set_options): every recording's
                                        workspace in global memory instead of LDS (test/diagnostic) */
    BPMX_OPT_FLOOR_ONEWG = 1048576,  /* the floor after the draft by one 1024-thread workgroup per recording
                                        (k_floor_wm alone) instead of two half-recording workgroups of 512
                                        threads that share a compute unit, with k_floor_wm over the recordings
                                        they hand back (test/diagnostic; the results are bit-identical) */
    BPMX_OPT_HRVSPEC_DIRECT = 2097152 /* bpmx_hrvspec_device (set with bpmx_set_options): one sincos per term
                                        instead of one per interval and block of 8 frequencies with a rotation
                                        along the grid (test/diagnostic; the same tolerance binds both forms) */
};

/* bpmx_stats counters of the last run with BPMX_OPT_STATS */
enum bpmx_stat {
    BPMX_STAT_RAW_TROUGHS = 0,   /* raw troughs of the recordings whose draft floor was bracketed */
    BPMX_STAT_UNDECIDED = 1,     /* of those, troughs the bracket left open: draft evaluated there exactly */
    BPMX_STAT_FULL_DRAFT = 2,    /* trough chunks whose recording fell back to the whole draft floor */
    BPMX_STAT_FLOOR_WHOLE = 3,   /* recordings the half-recording floor launch handed to the whole-recording one */
    BPMX_NSTATS = 8
};

typedef struct bpmx_ctx bpmx_ctx;

typedef struct {
    int32_t mode;          /* bpmx_mode */
    int32_t stages;        /* bpmx_stage mask */
    int32_t dtype;         /* bpmx_dtype of the PCM */
    int32_t channels;      /* >= 1, frames are interleaved */
    int32_t fs;            /* native sample rate */
    int32_t ds;            /* downsample factor after the clamp (:1021-1029), >= 1 */
    int32_t sr;            /* decimated rate fs // ds (:1032) */
    int32_t env_window;    /* sr // 10 (:1053) */
    int32_t distance;      /* int(min_peak_distance_sec * sr) (:1066, :226), >= 1 */
    int32_t noise_window;  /* int(noise_window_sec * sr) (:1084) */
    int32_t min_periods;   /* 3 (:1085, :1105) */
    int32_t options;       /* bpmx_option bits (0 = defaults) */
    double trough_prom_q;  /* trough_prominence_quantile (:1067) */
    double peak_prom_q;    /* peak_prominence_quantile (:225) */
    double noise_floor_q;  /* noise_floor_quantile (:1075, :1085) */
    double fallback_q;     /* 0.1 (:1114) */
    double reject_mult;    /* trough_rejection_multiplier (:1091) */
    double ba_b[5], ba_a[5], ba_zi[4];  /* butter(2,[lo,hi],'band') at sr + lfilter_zi (reference mode) */
    double sos[12], sos_zi[4];          /* butter(...,output='sos') at fs + sosfilt_zi (native mode) */
} bpmx_params;

typedef struct {
    int32_t n_files;
    int32_t reserved;
    const void *pcm;              /* device: frames of all files back to back, interleaved channels.
                                     The library may read from the 16-byte boundary at or below pcm
                                     (an int16 base a whole number of frames past it is read from
                                     there; the bytes before pcm are read and discarded, never used),
                                     so that a recording's outputs do not depend on its alignment */
    const int64_t *frame_offsets; /* host: n_files+1 frame offsets into pcm */
} bpmx_batch;

/* Result arrays (device).  Per-file slices start at the decimated offsets
 * D_f = sum_{g<f} Nd_g, Nd_g = bpmx_decimated_length(frames_g, ds); every
 * array below has sum(Nd) elements, except the three per-file ones.
 * env / floor are inputs when the stage that produces them is not requested. */
typedef struct {
    double *env;        /* f64 envelope */
    double *floor;      /* f64 dynamic noise floor */
    double *y;          /* optional (NULL): filtered decimated signal (debug WAV, :1047-1060).
                         * Native mode: asking for it keeps a separate yd pass (~0.05 ms per
                         * 1024 x 60 s batch on MI355X); left NULL, the envelope kernel makes
                         * yd itself. */
    int64_t *troughs;   /* sanitised trough indices, per-file slice, n_troughs[f] valid */
    int64_t *peaks;     /* raw peak indices, per-file slice, n_peaks[f] valid */
    int32_t *n_troughs; /* [n_files] */
    int32_t *n_peaks;   /* [n_files] */
    int32_t *flags;     /* [n_files] bpmx_file_flag bits */
    int32_t *n_raw_troughs; /* optional [n_files]: troughs before sanitisation (:1099 log line) */
} bpmx_out;

int bpmx_abi_version(void);
const char *bpmx_last_error(void);

int bpmx_create(int device, bpmx_ctx **out);
void bpmx_destroy(bpmx_ctx *ctx);

/* ceil(n_frames / ds): length of x[::ds] (:1033) */
int64_t bpmx_decimated_length(int64_t n_frames, int32_t ds);

/* Run the requested stages over a batch, asynchronously on `stream`
 * (a hipStream_t; NULL = default stream). */
int bpmx_run(bpmx_ctx *ctx, const bpmx_params *params, const bpmx_batch *batch, const bpmx_out *out,
             void *stream);

/* Resolving decisive ties in the reference's own order (BPMX_F_*_TIE).
 *
 * scipy's distance filter (_peak_finding_utils._select_by_peak_distance,
 * called at scipy/signal/_peak_finding.py:976-980 from bpm_analysis.py:1070 and
 * :227) visits the candidates in np.argsort(x[peaks]) order, highest last
 * index first.  That order is numpy's, so only the host can produce it:
 * a run with cand[s] set writes each recording's candidate list of search s
 * (the local maxima, plateau midpoints, left by the height filter; ascending
 * positions, per-file slices at D_f, n_cand[s][f] of them); the host computes
 * rank = inverse of np.argsort(x[cand]) per recording; a run with rank[s] set
 * (and use_rank[s][f] != 0) then decides the distance filter of recording f by
 * rank alone — candidate k removes candidate j within `distance` iff
 * rank[k] > rank[j] and k is kept — which is scipy's greedy loop exactly.
 * Search 0 is the trough search find_peaks(-env) (:1070), 1 the raw-peak search
 * find_peaks(env, height=floor) (:227).  The candidates of a search depend only
 * on env (and the floor for search 1), so a rank computed from one run's list
 * applies to any run on the same env (and floor).  All pointers are device
 * pointers and optional (NULL: that part is not used); a run with an order
 * object takes the one-workgroup find_peaks kernel for every recording.  Meant
 * for the few recordings that carry a TIE bit (engine.Detector.resolve_ties).
 */
typedef struct {
    int32_t *cand[2];           /* out: candidate positions, sum(Nd) entries, per-file slices at D_f */
    int32_t *n_cand[2];         /* out: [n_files] candidate counts (with cand[s]) */
    const int32_t *rank[2];     /* in: per candidate (same order as cand), its index in np.argsort(x[cand]) */
    const int32_t *use_rank[2]; /* in: [n_files] nonzero = recording f's slice of rank[s] is set */
} bpmx_peak_order;

/* bpmx_run with a find_peaks visiting order / candidate export (above); order
 * NULL = bpmx_run.  Never pipelined. */
int bpmx_run_ordered(bpmx_ctx *ctx, const bpmx_params *params, const bpmx_batch *batch, const bpmx_out *out,
                     const bpmx_peak_order *order, void *stream);

/* Compact results, packed on the device (bpmx_pack).
 *
 * A finished run leaves env, floor, troughs and peaks as sum(Nd)-long 8-byte
 * arrays, but the stages after it read env and floor only at the raw peaks
 * and the troughs (a few hundred positions per minute of recording).  These
 * tables hold exactly that, ragged, file after file:
 *
 *   pk_off[f]  = sum_{g<f} n_peaks[g]    (pk_off[n_files] = the total)
 *   for k < n_peaks[f], i = peaks[D_f + k], j = pk_off[f] + k:
 *     pk_idx[j] = i,  pk_env[j] = env[D_f + i],  pk_floor[j] = floor[D_f + i]
 *
 * and the same from troughs / n_troughs into tr_off, tr_idx, tr_env.  Values
 * are copied bit for bit.  The offsets always hold the true totals; an entry
 * whose table position j is >= the table's capacity is not written, so a
 * caller detects an overflow from off[n_files] > cap.  Each table is optional:
 * it is built when its offsets pointer is set (its other pointers are then
 * required, with in->peaks / in->troughs, the matching count and in->env, and
 * in->floor for the peak table).
 *
 * y16 (optional; needs in->y and y_max): the debug WAV's samples
 * (bpm_analysis.py:1057-1060, np.int16(y / np.max(np.abs(y)) * 32767)).  Per
 * file, m = max|y| over its slice (the largest |y| bit pattern, so a NaN wins),
 * y_max[f] = m, and y16[D_f + i] = (int16_t)trunc((y[D_f + i] / m) * 32767.0),
 * the division and the multiplication rounded separately; a file whose m is
 * 0, NaN or inf gets zeros.  y16 needs 2-byte alignment only. */
typedef struct {
    int64_t cap_peaks, cap_troughs; /* table capacities, entries */
    int64_t *pk_off, *tr_off;       /* device [n_files + 1] */
    int32_t *pk_idx;                /* device [cap_peaks] */
    double *pk_env, *pk_floor;      /* device [cap_peaks] */
    int32_t *tr_idx;                /* device [cap_troughs] */
    double *tr_env;                 /* device [cap_troughs] */
    int16_t *y16;                   /* optional device [sum(Nd)] */
    double *y_max;                  /* device [n_files] (with y16) */
} bpmx_packed;

/* Pack the outputs `in` of a finished bpmx_run / bpmx_run_ordered over the
 * batch geometry (n_files, host frame_offsets, ds: the D_f of bpmx_out) into
 * `out`, asynchronously on `stream` (the run's stream, or one ordered after
 * it).  No host synchronisation; scratch comes from ctx. */
int bpmx_pack(bpmx_ctx *ctx, int32_t n_files, const int64_t *frame_offsets, int32_t ds, const bpmx_out *in,
              const bpmx_packed *out, void *stream);

/* The beat stages on the device (bpmx_beats_device).
 *
 * What the reference runs per file after the hot path (bpm_analysis.py
 * :1734-1757: _run_preliminary_pass, PeakClassifier.classify_peaks,
 * _refine_and_correct_peaks, calculate_bpm_series), computed from bpmx_pack's
 * peak table where it lies.  The arithmetic is that of bpmx_beats
 * (bpmx_host.h), one statement of it for both (csrc/bpmx_beats_core.h):
 * every index, label, count and pass value equals the host library's, and
 * the curves are the same IEEE f64 operations in the same order.
 *
 * Per-file output slices start at pk_off[f], like the peak table's; a file
 * writes n_final[f] / n_bpm[f] entries of its slices and nothing else (tags:
 * one per raw peak).  pass and tags are optional (NULL). */
enum bpmx_beats_status {        /* bpmx_beats_out.status, beside BPMX_HOST_OK and BPMX_HOST_E_FEW_PEAKS
                                   (< 2 raw peaks: counts 0, tags still written, as on the host) */
    BPMX_BEATS_SKIPPED = -16,   /* flags given and the file carries BPMX_F_TOO_SHORT or BPMX_F_BAD_WINDOW:
                                   counts 0, pass NaN, no tags */
    BPMX_BEATS_OVERFLOW = -17   /* the file's table slice reaches past cap_peaks (or its offsets are not
                                   ascending): counts 0, pass NaN, nothing read or written beyond the capacity */
};

typedef struct {            /* device; per-file slices start at pk_off[f], like the peak table */
    int32_t *final_idx;     /* [cap_peaks] final beats (subset of the raw peaks, ascending) */
    int32_t *n_final;       /* [n_files] */
    double  *bpm_t, *bpm;   /* [cap_peaks] curve rows, n_bpm[f] valid */
    int32_t *n_bpm;         /* [n_files] */
    double  *pass;          /* optional [n_files][3]: start BPM, peak-BPM time, recovery end (NaN = None) */
    int8_t  *tags;          /* optional [cap_peaks] bpmx_beat_tag per raw peak */
    int32_t *status;        /* [n_files] */
} bpmx_beats_out;

/* The beat stages of n_files recordings at decimated rate sr from the peak
 * table `in` (pk_off, pk_idx, pk_env, pk_floor and cap_peaks < 2^31 required;
 * pk_idx strictly increasing per file, as bpmx_pack writes it), asynchronously
 * on `stream`, ordered after the pack.  start_bpm_hint: NaN = None.  flags:
 * optional device [n_files] (bpmx_out.flags).  Never synchronises the host;
 * scratch comes from ctx (grown on the first call of a capacity).  One wave64
 * workgroup per recording; see csrc/k_beats.hip. */
int bpmx_beats_device(bpmx_ctx *ctx, int32_t n_files, int32_t sr, const bpmx_beat_params *params,
                      double start_bpm_hint, const bpmx_packed *in, const int32_t *flags,
                      const bpmx_beats_out *out, void *stream);

/* The decision trace of the beat stages (bpmx_beats_device_ex).
 *
 * What the reference keeps per file to explain its decisions (analysis_data:
 * beat_debug_info, long_term_bpm_series, deviation_series), as numbers: the
 * main classification pass stores every value its debug strings format, and
 * the gap fill which label each of its passes gave a peak.  The host turns
 * them into the reference's strings (bpm_analysis_amd/explain.py); values are
 * f64 because the strings round them and only identical doubles give
 * identical text.  Thresholds and weights are parameters the host has.
 *
 * record: BPMX_TR_NFIELDS doubles per raw peak.  A field is written only when
 * the peak's code announces it (everything else is left as it was):
 *   every peak but the last and an S2: BLEND, BASE_CONF, FINAL
 *   BPMX_TRF_STABILITY: STAB_FACTOR, STAB_RATIO    (>= 5 beats so far)
 *   BPMX_TRF_PENALIZED: ADJ_AMOUNT, ADJ_RATIO (S2/S1), ADJ_RMAX
 *   BPMX_TRF_BOOSTED:   ADJ_AMOUNT, ADJ_RATIO (S1/S2)
 *   BPMX_TRF_INTERVAL:  IV_AMOUNT, IV_GAP, IV_CAP
 *   LONE_VALID, CASCADE, NOISE: the six L_* fields of the Lone-S1 test, and
 *   L_IMPLIED with BPMX_TRF_FORWARD (the failed forward check)
 * An S2 (BPMX_TR_S2_PAIRED) has no record: its string is that of the S1 one
 * table position before it. */
enum bpmx_trace_field {
    BPMX_TR_BLEND = 0,          /* share of the high-BPM confidence curve */
    BPMX_TR_BASE_CONF = 1,      /* blended pairing confidence, may be NaN */
    BPMX_TR_STAB_FACTOR = 2, BPMX_TR_STAB_RATIO = 3,
    BPMX_TR_ADJ_AMOUNT = 4, BPMX_TR_ADJ_RATIO = 5, BPMX_TR_ADJ_RMAX = 6,
    BPMX_TR_IV_AMOUNT = 7, BPMX_TR_IV_GAP = 8, BPMX_TR_IV_CAP = 9,
    BPMX_TR_FINAL = 10,         /* the score compared with the pairing threshold */
    BPMX_TR_L_RHYTHM = 11, BPMX_TR_L_RR = 12, BPMX_TR_L_EXPECTED = 13, BPMX_TR_L_AMP = 14, BPMX_TR_L_RATIO = 15,
    BPMX_TR_L_CONF = 16,
    BPMX_TR_L_IMPLIED = 17,     /* BPM the next raw peak would imply */
    BPMX_TR_NFIELDS = 18
};
enum bpmx_trace_code {          /* code = outcome | optional lines */
    BPMX_TR_S1_PAIRED = 1, BPMX_TR_S2_PAIRED = 2, BPMX_TR_LONE_VALID = 3, BPMX_TR_FIRST_BEAT = 4,
    BPMX_TR_LAST_PEAK = 5, BPMX_TR_CASCADE = 6, BPMX_TR_NOISE = 7,
    BPMX_TR_OUTCOME = 15,       /* mask */
    BPMX_TRF_STABILITY = 16, BPMX_TRF_PENALIZED = 32, BPMX_TRF_BOOSTED = 64, BPMX_TRF_INTERVAL = 128,
    BPMX_TRF_FORWARD = 256      /* NOISE: rejected by the forward check, not by confidence */
};
enum bpmx_trace_gap {           /* gap[j] >> (2 * pass) & 3, pass 0..4 of the gap fill */
    BPMX_TR_GAP_NONE = 0, BPMX_TR_GAP_S1 = 1, BPMX_TR_GAP_S2 = 2
};

typedef struct {            /* device; per-file slices start at pk_off[f], like the peak table */
    double  *record;        /* [cap_peaks][BPMX_TR_NFIELDS] */
    int32_t *code;          /* [cap_peaks] bpmx_trace_code per raw peak */
    int32_t *lt_pos;        /* [cap_peaks] table position of the last beat after each classifier iteration */
    double  *lt_bpm;        /* [cap_peaks] the long-term BPM after it; n_lt[f] valid */
    int32_t *n_lt;          /* [n_files] */
    double  *dev_t, *dev;   /* [cap_peaks] smoothed deviation series of the main pass, n - 1 valid */
    int32_t *gap;           /* [cap_peaks] bpmx_trace_gap of each gap-fill pass */
} bpmx_trace_out;

/* bpmx_beats_device with per-file hints and the decision trace, both optional
 * (both NULL: bpmx_beats_device).  hints: device [n_files], NaN = None; file
 * f starts from hints[f] when that is neither NaN nor 0, as start_bpm_hint
 * does for all files.  trace: every pointer required.  A recording of >= 2
 * raw peaks writes a code and a gap entry per raw peak, n - 1 deviations and
 * n_lt[f] beliefs; one of fewer writes n_lt[f] = 0 only; one that reports
 * BPMX_BEATS_SKIPPED or BPMX_BEATS_OVERFLOW writes nothing of the trace. */
int bpmx_beats_device_ex(bpmx_ctx *ctx, int32_t n_files, int32_t sr, const bpmx_beat_params *params,
                         double start_bpm_hint, const bpmx_packed *in, const int32_t *flags,
                         const bpmx_beats_out *out, const double *hints, const bpmx_trace_out *trace,
                         void *stream);

/* tr_floor[j] = floor[D_f + tr_idx[j]] for the trough table of a bpmx_pack
 * (tr_off, tr_idx; `in` as given to that pack: in->floor is read), copied bit
 * for bit; an entry at or beyond cap_troughs is not written.  Asynchronous on
 * `stream`, ordered after the pack.  frame_offsets / ds as for bpmx_pack. */
int bpmx_pack_trough_floor(bpmx_ctx *ctx, const bpmx_out *in, const int64_t *frame_offsets, int32_t n_files,
                           int32_t ds, const bpmx_packed *tables, double *tr_floor, void *stream);

/* The analysis plot's two line traces (bpmx_pack_plot).
 *
 * The figure reads the envelope and the floor at the raw peaks and the
 * troughs (bpmx_pack's tables) and, for its two line traces, at every k-th
 * sample, k = plot_downsample_factor (bpm_analysis.py:518-524).  Per file the
 * reference's rule: kf = factor when factor > 1 and Nd_f >= factor, else 1;
 * n_f = bpmx_plot_length(Nd_f, factor) = ceil(Nd_f / kf) entries are kept:
 *
 *   P_f = sum_{g<f} n_g
 *   for j < n_f:  pl_env[P_f + j] = env[D_f + j * kf]   (pl_floor likewise)
 *
 * copied as 64-bit patterns.  The offsets follow from frame_offsets, ds and
 * factor alone, so the host knows them (and the total, P_{n_files}) without
 * asking the device.  File flags are not consulted. */
int64_t bpmx_plot_length(int64_t nd, int32_t factor);

/* in->env (required) and in->floor (read when pl_floor is set; pl_floor NULL:
 * no floor series) -> pl_env, pl_floor: device [cap] entries.  A total above
 * cap is BPMX_E_ARG, before anything is launched; nothing outside [0, total)
 * of either output is written.  One launch, asynchronous on `stream` (the
 * run's, or one ordered after it), no host synchronisation; scratch comes
 * from ctx.  frame_offsets / ds as for bpmx_pack. */
int bpmx_pack_plot(bpmx_ctx *ctx, int32_t n_files, const int64_t *frame_offsets, int32_t ds, int32_t factor,
                   const bpmx_out *in, double *pl_env, double *pl_floor, int64_t cap, void *stream);

/* The final metrics on the device (bpmx_metrics_device).
 *
 * What the reference computes per file from the final beats and the curve
 * (bpm_analysis.py:1701-1722 _calculate_final_metrics with :1414-1461 and
 * :1486-1610): the windowed HRV table, the summary, heart-rate recovery, the
 * steepest recovery and exertion slopes, the major inclines and declines.
 * Computed from bpmx_beats_device's outputs where they lie; the arithmetic is
 * csrc/bpmx_metrics_core.h, the same IEEE f64 operations in the same order as
 * numpy, pandas and scipy apply them.  Timestamps are returned as positions
 * into the file's curve (bpm_t / bpm), which the host indexes. */
typedef struct {
    int32_t hrv_window_size_beats, hrv_step_size_beats;   /* DEFAULT_PARAMS (:1414-1461), window >= 2, step >= 1 */
    double min_duration_sec;    /* 10: find_major_hr_inclines / declines; the find_peaks distance is half of it */
    double min_bpm_change;      /* 15 */
    double prominence;          /* 5 (find_peaks) */
    double slope_window_sec;    /* 20: peak recovery / exertion rate */
    double hrr_interval_sec;    /* 60: calculate_hrr */
} bpmx_metric_params;

enum bpmx_metrics_status {      /* bpmx_metrics_out.status: 0, or the two bits below, or a negative code */
    BPMX_METRICS_OK = 0,
    BPMX_METRICS_TIE = 1,         /* the distance filter of find_peaks on the curve removed a candidate that no
                                     strictly higher kept one covers: among equal heights the later index was
                                     visited first (as for BPMX_F_*_TIE), numpy's argsort may differ */
    BPMX_METRICS_E_DISTANCE = 2,  /* the find_peaks distance int(5 / mean step) is < 1: scipy raises ValueError;
                                     no inclines or declines, everything else is written */
    BPMX_METRICS_NONE = -18,      /* fewer than two final beats, or the file's beats status is not OK: counts
                                     0, record NaN (the reference makes no metrics) */
    BPMX_METRICS_OVERFLOW = -19   /* the file's slice reaches past cap_peaks: nothing written but the status */
};

/* bpmx_metrics_out.record: 16 doubles per file, NaN = absent.  Positions are
 * indices into the file's curve. */
enum bpmx_metrics_record {
    BPMX_MR_AVG_BPM = 0, BPMX_MR_MIN_BPM = 1, BPMX_MR_MAX_BPM = 2, BPMX_MR_AVG_RMSSDC = 3, BPMX_MR_AVG_SDNN = 4,
    BPMX_MR_HRR_PEAK = 5,           /* position of the maximum */
    BPMX_MR_HRR_RECOVERY_BPM = 6, BPMX_MR_HRR_VALUE = 7,
    BPMX_MR_RECOVERY = 8,           /* start position, end position, slope (BPM/s), duration (s) */
    BPMX_MR_EXERTION = 12,          /* the same four */
    BPMX_METRICS_RECORD = 16
};

typedef struct {            /* device; per-file slices start at pk_off[f] (rows and runs never outnumber raw peaks) */
    double *hrv_time, *hrv_rmssdc, *hrv_sdnn, *hrv_bpm;   /* [cap_peaks] windowed HRV rows, n_hrv[f] valid */
    int32_t *n_hrv;                                       /* [n_files] */
    int32_t *inc_a, *inc_b, *dec_a, *dec_b;               /* [cap_peaks] curve positions of each run's start and
                                                             end, in report order (steepest first) */
    double *inc_slope, *inc_dur, *dec_slope, *dec_dur;    /* [cap_peaks] */
    int32_t *n_inc, *n_dec;                               /* [n_files] */
    double *record;                                       /* [n_files][BPMX_METRICS_RECORD] */
    int32_t *status;                                      /* [n_files] bpmx_metrics_status */
} bpmx_metrics_out;

/* The final metrics of n_files recordings from `beats` (the outputs of
 * bpmx_beats_device over `tables`: pk_off and cap_peaks are read from there),
 * asynchronously on `stream`, ordered after the beat stages.  epoch_us: the
 * origin of the curve's datetime index in microseconds since 1970 (the
 * reference's datetime.fromtimestamp(0): 0 on a UTC machine).  Never
 * synchronises the host; scratch comes from ctx.  Every pointer of `out` is
 * required.  One workgroup per recording; see csrc/k_metrics.hip. */
int bpmx_metrics_device(bpmx_ctx *ctx, int32_t n_files, int32_t sr, const bpmx_metric_params *params,
                        int64_t epoch_us, const bpmx_packed *tables, const bpmx_beats_out *beats,
                        const bpmx_metrics_out *out, void *stream);

/* The labeler's output on the device (bpmx_labels_device).
 *
 * heartbeat_labeler.py exists to produce <base>_labels.csv (a table of S1 and
 * S2 marks: time, average BPM, type) and the S1-S2 interval analysis over it.
 * There a person clicks every mark; here the marks are the beat stages' own
 * decisions, read where bpmx_beats_device_ex left them:
 *
 *   S1: every final beat (final_idx).
 *   S2: every raw peak that is not a final beat and whose final debug string
 *       is an S2: the label of the highest gap-fill pass that touched it
 *       (trace gap), else the main pass' tag.  Nothing else is labelled.
 *
 * A label is what the labeler appends for a click exactly on the peak
 * (:530-546), x = idx / sr:  time = round(x, 3) (Python's round, the correctly
 * rounded decimal), BPM = round(B[argmin |T - x|], 3) over the rows (T, B) of
 * <base>_bpm_plot.csv (the curve rows whose BPM is not NaN, each value as
 * float(f"{v:.3f}"); the first minimum wins).  Labels ascend in time.  Pairs
 * are calculate_s1_s2_diffs' greedy walk (:198-217), groups
 * detect_labeling_groups (:244-276) at gap_sec, their statistics
 * calculate_group_statistics (:278-308): sums added left to right.  The
 * arithmetic is csrc/bpmx_labels_core.h.
 *
 * A recording never has more labels than raw peaks, nor more pairs or groups,
 * so every output slice starts at pk_off[f].  Label positions (pr_*, gr_first,
 * gr_last) index the file's label rows; lb_pos is the raw peak's position in
 * the file's slice of the peak table. */
typedef struct {
    double gap_sec;             /* detect_labeling_groups' gap_threshold; the labeler's group panel starts at 5 */
} bpmx_label_params;

enum bpmx_label_type { BPMX_LABEL_S1 = 1, BPMX_LABEL_S2 = 2 };

enum bpmx_labels_status {       /* bpmx_labels_out.status */
    BPMX_LABELS_OK = 0,
    BPMX_LABELS_NONE = -20,     /* the beat stages did not finish with BPMX_HOST_OK, fewer than two final beats
                                   (the reference writes no CSV), or no curve row that is not NaN: counts 0,
                                   record NaN */
    BPMX_LABELS_OVERFLOW = -21  /* the file's slice reaches past cap_peaks: nothing written but the status */
};

/* bpmx_labels_out.record: 4 doubles per file */
enum bpmx_labels_record {
    BPMX_LR_AVG_DT = 0,         /* mean S1-S2 interval over all pairs (calculate_avg_delta_t_in_range over the
                                   whole table), NaN without pairs */
    BPMX_LR_AVG_BPM = 1,        /* mean BPM of the pairs' S1 rows, NaN without pairs */
    BPMX_LR_N_S1 = 2, BPMX_LR_N_S2 = 3,   /* labels of each type */
    BPMX_LABELS_RECORD = 4
};

typedef struct {            /* device; per-file slices start at pk_off[f] */
    int32_t *lb_pos, *lb_type;            /* [cap_peaks] label rows: raw-peak position, bpmx_label_type */
    double *lb_time, *lb_bpm;             /* [cap_peaks] 'Time (s)', 'Average BPM'; n_labels[f] valid */
    int32_t *pr_s1, *pr_s2;               /* [cap_peaks] pairs: the two label rows */
    double *pr_dt;                        /* [cap_peaks] S2 time - S1 time, unrounded; n_pairs[f] valid */
    int32_t *gr_id, *gr_first, *gr_last;  /* [cap_peaks] groups with statistics: group_id (may jump), first and
                                             last S1 label row */
    int32_t *gr_s1, *gr_pairs;            /* [cap_peaks] s1_count, pairs_count */
    double *gr_dt, *gr_bpm;               /* [cap_peaks] avg_delta_t, avg_bpm; n_groups[f] valid */
    int32_t *n_labels, *n_pairs, *n_groups;   /* [n_files] */
    double *record;                       /* [n_files][BPMX_LABELS_RECORD] */
    int32_t *status;                      /* [n_files] bpmx_labels_status */
} bpmx_labels_out;

/* The labels of n_files recordings from `beats` (the outputs of
 * bpmx_beats_device_ex over `tables`: pk_off, pk_idx and cap_peaks are read
 * from the tables; final_idx, n_final, bpm_t, bpm, n_bpm, tags and status from
 * the beats) and `gap` (bpmx_trace_out.gap of the same launch, required),
 * asynchronously on `stream`, ordered after the beat stages.  Never
 * synchronises the host; scratch comes from ctx.  Every pointer of `out` is
 * required.  One workgroup per recording; see csrc/k_labels.hip. */
int bpmx_labels_device(bpmx_ctx *ctx, int32_t n_files, int32_t sr, const bpmx_label_params *params,
                       const bpmx_packed *tables, const bpmx_beats_out *beats, const int32_t *gap,
                       const bpmx_labels_out *out, void *stream);

/* Beats scored against corrected labels on the device (bpmx_score_device).
 *
 * Once a person has corrected the marks of <base>_labels.csv in the labeler,
 * the question is how well some settings reproduce them.  The reference has no
 * scoring; this is the definition (csrc/bpmx_score_core.h states it for host
 * and device, labels.score in Python).  Everything is integer milliseconds.
 *
 *   Detected marks: the label rows of bpmx_labels_device (lb_time, lb_type,
 *       n_labels, ascending), ms = llrint(lb_time * 1000.0) saturated to
 *       int32.  A labels status other than BPMX_LABELS_OK gives an empty list
 *       and sets the bit BPMX_SCORE_NO_LABELS.
 *   Reference marks: the S1 / S2 rows of the corrected file, prepared on the
 *       host (labels.marks_from_table): ms = rint(time * 1000), sorted stably
 *       by ms, uploaded as a ragged table.
 *   Spans: the reference marks of both types together; a new span starts
 *       where the step is >= gap_ms; a span is [first - tol_ms, last + tol_ms].
 *       A detected mark in no span is outside: counted, scored no further.
 *   The walk over two ascending lists D, R from i = j = 0: |D[j] - R[i]| <=
 *       tol_ms is a match (both step), else the smaller one steps.  It gives a
 *       maximum matching.
 *   Pass 1, per type: the in-span detected marks of the type against the
 *       reference marks of the type: TP, with the error e = D - R.
 *   Pass 2, per type: the detected marks left against the reference marks of
 *       the other type left: SWAP (the beat was heard, but given the other
 *       name).  A detected mark still unmatched is FP, a reference mark FN.
 *
 * N_DET = TP + SWAP + FP, N_REF = TP + SWAP[other type] + FN and
 * N_OUTSIDE + N_DET[S1] + N_DET[S2] = n_labels.  Precision, recall and the
 * mean errors are left to the host (labels.score_summary). */
typedef struct {
    int32_t tol_ms;             /* >= 0: two marks this close are the same beat */
    int32_t gap_ms;             /* > 2 * tol_ms: a pause this long between reference marks ends a labelled span */
} bpmx_score_params;

typedef struct {
    int64_t cap_ref;            /* capacity of rf_ms / rf_type and of the rf_* outputs, entries */
    const int64_t *rf_off;      /* [n_files + 1] ascending */
    const int32_t *rf_ms;       /* [cap_ref] ascending within a file */
    const int32_t *rf_type;     /* [cap_ref] bpmx_label_type; any other value takes part in the spans only */
} bpmx_ref_marks;

enum bpmx_score_kind {          /* sc_kind; rf_kind (0 there: a type that is neither S1 nor S2) */
    BPMX_SCORE_OUTSIDE = 0, BPMX_SCORE_TP = 1, BPMX_SCORE_SWAP = 2, BPMX_SCORE_FP = 3, BPMX_SCORE_FN = 3
};

enum bpmx_score_status {        /* bpmx_score_out.status: 0, the bit, or a negative code */
    BPMX_SCORE_OK = 0,
    BPMX_SCORE_NO_LABELS = 1,   /* bit: the labels stage made no labels; every reference mark is an FN */
    BPMX_SCORE_NONE = -22,      /* no reference mark: the record is zeros apart from N_OUTSIDE = n_labels, no rows
                                   are written */
    BPMX_SCORE_OVERFLOW = -23   /* a slice reaches past cap_peaks or cap_ref, or rf_off is not ascending: nothing
                                   written but the status */
};

/* bpmx_score_out.record: 20 int64 per file; nine fields for S1, nine for S2, two for the file */
enum bpmx_score_record {
    BPMX_SR_N_REF = 0,          /* reference marks of the type */
    BPMX_SR_N_DET = 1,          /* detected marks of the type in a span */
    BPMX_SR_TP = 2, BPMX_SR_SWAP = 3, /* SWAP: detected as this type, matched to a reference mark of the other */
    BPMX_SR_FP = 4, BPMX_SR_FN = 5,
    BPMX_SR_SUM_ERR = 6,        /* over the TP: sum of e, sum of |e|, largest |e| (0 without TP), ms */
    BPMX_SR_SUM_ABS = 7, BPMX_SR_MAX_ABS = 8,
    BPMX_SR_PER_TYPE = 9,       /* the S2 fields start here */
    BPMX_SR_N_OUTSIDE = 18, BPMX_SR_N_SPANS = 19,
    BPMX_SCORE_RECORD = 20
};

typedef struct {
    int32_t *sc_kind, *sc_ref;  /* [cap_peaks] per label row, slices at pk_off[f]: bpmx_score_kind, the matched
                                   reference row within the file or -1 */
    int32_t *rf_kind, *rf_det;  /* [cap_ref] per reference row, slices at rf_off[f]: bpmx_score_kind, the matched
                                   label row or -1 */
    int64_t *record;            /* [n_files][BPMX_SCORE_RECORD] */
    int32_t *status;            /* [n_files] bpmx_score_status */
} bpmx_score_out;

/* The scores of n_files recordings: `labels` (lb_time, lb_type, n_labels and
 * status of bpmx_labels_device over `tables`, of which pk_off and cap_peaks are
 * read) against `ref`, asynchronously on `stream`, ordered after the labels
 * stage.  Never synchronises the host; scratch comes from ctx.  The four row
 * pointers of `out` are optional as a group (all NULL: record and status
 * only); nothing outside a file's used entries is written.  n_files = 0 does
 * nothing.  One workgroup per recording; see csrc/k_score.hip. */
int bpmx_score_device(bpmx_ctx *ctx, int32_t n_files, const bpmx_score_params *params, const bpmx_packed *tables,
                      const bpmx_labels_out *labels, const bpmx_ref_marks *ref, const bpmx_score_out *out,
                      void *stream);

/* A person's corrected marks as beats on the device (bpmx_marks_device).
 *
 * The reference computes the BPM curve, the HRV table, HRR, slopes and the
 * summary from nothing but the final S1 indices (_calculate_final_metrics,
 * bpm_analysis.py:1701-1722).  This stage turns a table of a person's marks
 * (bpmx_ref_marks, as for bpmx_score_device) into the peak-table and
 * bpmx_beats_out layouts that bpmx_metrics_device, bpmx_labels_device and
 * bpmx_score_device consume, so those run unchanged on the corrected beats.
 * There is no reference implementation of the conversion; this is the
 * definition (csrc/bpmx_marks_core.h states it for host and device,
 * labels.rows_from_marks in Python).  Integers only, so both agree exactly.
 *
 *   Rows from marks, per recording, in table order:
 *     - a mark whose type is neither S1 nor S2 is skipped (N_OTHER);
 *     - a mark with ms < 0 is dropped (N_DROPPED);
 *     - idx = (ms * sr + 500) / 1000 in int64; a mark with idx > INT32_MAX or,
 *       with nd, idx >= nd[f] is dropped (N_DROPPED);
 *     - a run of kept marks with equal idx becomes one row, S1 if any mark of
 *       the run is S1, else S2; the removed marks are counted (N_MERGED).
 *   With rf_ms ascending the rows are strictly ascending in idx, which is what
 *   bpmx_labels_device requires of pk_idx.  N_ROWS + N_MERGED + N_DROPPED +
 *   N_OTHER is the number of marks of the file.
 *
 *   Outputs, in the existing layouts (slices start at pk_off[f]):
 *     pk_off[n_files + 1]: the exclusive prefix sums of the row counts, the
 *         true totals even when they exceed cap_peaks (as bpmx_pack);
 *     pk_idx: the rows' idx; pk_env / pk_floor (optional): quiet NaN;
 *     tags: BPMX_TAG_S1 / BPMX_TAG_S2 per row; gap: 0 per row, so the labels
 *         stage takes the type from the tag;
 *     final_idx, n_final: the S1 rows' idx, ascending;
 *     bpm_t, bpm, n_bpm: calculate_bpm_series of those (beats_series of
 *         csrc/bpmx_beats_core.h, the text bpmx_beats_device runs) at
 *         smoothing_window_sec (output_smoothing_window_sec);
 *     pass (optional): NaN;
 *     record: 8 int32 per file (bpmx_marks_record).
 *
 * The label times the later stages make are round(idx / sr, 3): the person's
 * own millisecond for sr >= 1000, and any time the labeler or a label file of
 * this project can hold for sr < 1000; a hand-typed time off the sample grid
 * snaps to the nearest sample.  A recording never has more rows than marks:
 * cap_peaks = cap_ref always suffices. */
typedef struct {
    double smoothing_window_sec;    /* > 0: output_smoothing_window_sec */
} bpmx_marks_params;

enum bpmx_marks_status {        /* bpmx_beats_out.status as bpmx_marks_device writes it, beside BPMX_HOST_OK */
    BPMX_MARKS_FEW = -24,       /* fewer than two S1 rows: n_final and n_bpm are 0; rows, tags, gap and the record
                                   are still written (the later stages then answer *_NONE) */
    BPMX_MARKS_OVERFLOW = -25   /* a slice reaches past cap_peaks or cap_ref, or rf_off descends: nothing written
                                   but the status */
};

enum bpmx_marks_record {        /* record: 8 int32 per file */
    BPMX_MK_N_ROWS = 0, BPMX_MK_N_S1 = 1, BPMX_MK_N_S2 = 2,
    BPMX_MK_N_MERGED = 3,       /* marks removed because they fell on the sample of the mark before them */
    BPMX_MK_N_DROPPED = 4,      /* ms < 0, idx > INT32_MAX or idx >= nd[f] */
    BPMX_MK_N_OTHER = 5,        /* a type that is neither S1 nor S2 */
    BPMX_MARKS_RECORD = 8       /* 6 and 7 are reserved zeros */
};

/* The marks of n_files recordings at decimated rate sr as rows, beats and
 * curve, asynchronously on `stream`.  marks: rf_off and cap_ref < 2^31 (with
 * cap_ref > 0, rf_ms and rf_type).  nd: optional device [n_files], the
 * recordings' envelope lengths.  tables (out): cap_peaks < 2^31, pk_off and
 * pk_idx required, pk_env / pk_floor optional, the rest ignored.  beats (out):
 * final_idx, n_final, bpm_t, bpm, n_bpm, tags and status required, pass
 * optional.  gap [cap_peaks] and record [n_files][BPMX_MARKS_RECORD] are
 * required.  Nothing outside a file's used entries is written, and nothing is
 * read or written beyond cap_ref and cap_peaks.  Never synchronises the host;
 * scratch comes from ctx.  n_files = 0 does nothing.  Three launches: rows per
 * recording, the scan of the counts, beats and curve per recording; see
 * csrc/k_marks.hip. */
int bpmx_marks_device(bpmx_ctx *ctx, int32_t n_files, int32_t sr, const bpmx_marks_params *params,
                      const bpmx_ref_marks *marks, const int64_t *nd, const bpmx_packed *tables,
                      const bpmx_beats_out *beats, int32_t *gap, int32_t *record, void *stream);

/* The tempogram on the device (bpmx_tempo_device).
 *
 * A BPM per window from the short-time autocorrelation of the envelope, which
 * uses neither find_peaks nor the classifier: a second opinion on the BPM
 * curve (an octave error shows as a factor of two) and, from the first
 * windows, a start hint per recording that bpmx_beats_device_ex reads where it
 * lies.  The reference has no such stage; this is the definition
 * (csrc/bpmx_tempo_core.h states the decisions for host and device,
 * tempo.tempogram in Python the whole of it).
 *
 *   Windows: window w of a recording of nd envelope samples starts at s = w *
 *       hop; there are bpmx_tempo_windows(nd, win, hop) = 0 if nd < win, else
 *       (nd - win) / hop + 1 of them.
 *   Per window: invalid if any of its win samples is not finite or if
 *       max == min.  Else m = sum / win, e[i] = x[s + i] - m for i < win and 0
 *       beyond, r[k] = sum_{i < win} e[i] * e[i + k] for k = kmin - 1 .. kmax + 1
 *       and k = 0.  The candidates are the k in [kmin, kmax] with r[k] > r[k - 1]
 *       and r[k] >= r[k + 1]; none: invalid.  The lag is the candidate of the
 *       largest r[k], the smallest k among equals.  rho = r[k] / r[0],
 *       delta = 0.5 * (r[k - 1] - r[k + 1]) / (r[k - 1] - 2 * r[k] + r[k + 1]),
 *       bpm = 60.0 * sr / (k + delta).  An invalid window has lag 0, rho 0.0,
 *       bpm NaN.
 *   Per recording: n_valid counts the valid windows, n_strong the strong ones
 *       (valid and rho >= min_strength); median_bpm is numpy's median of the
 *       strong windows' bpm and mean_rho the mean of rho over the valid windows
 *       (NaN with none); hint is the bpm of the first strong window among the
 *       windows 0 .. start_windows - 1, NaN with none: what
 *       bpmx_beats_device_ex reads as "no hint".
 *
 * The sums are f64 in an order of the kernel's own (products fused into the
 * running sums): rho agrees with another order of summation to about
 * win * 2^-52 * (1 + (m / sigma)^2), so a decision between lags closer than
 * that may differ.  min_strength and start_windows are judgement (0.3 and 3 in
 * the Python layer), not measurement.
 *
 * Limits: hop >= 1, kmin >= 2, kmin <= kmax and kmax + 1 < win, else BPMX_E_ARG.
 * A workgroup keeps the padded window and four partial sums per lag in LDS:
 * with win4 = win rounded up to a multiple of 4,
 *   8 * (win4 + kmax + 8 + 4 * (kmax - kmin + 4)) <= 155648 bytes (152 KB),
 * else BPMX_E_LIMIT.  That is 8 s windows down to 30 BPM at rates up to about
 * 1 kHz; envelopes at audio rates are not the target. */
typedef struct {
    int32_t win, hop;           /* window and step, samples */
    int32_t kmin, kmax;         /* lag range, samples: ceil(60 sr / max_bpm), floor(60 sr / min_bpm) */
    double min_strength;        /* a window is strong when rho >= this */
    int32_t start_windows;      /* the hint comes from the first this many windows */
    int32_t reserved;           /* 0 */
} bpmx_tempo_params;

typedef struct {            /* device */
    int32_t *lag;               /* per window; a file's slice starts at the sum of the windows before it */
    double *rho, *bpm;          /* per window */
    int32_t *n_valid, *n_strong;            /* [n_files] */
    double *median_bpm, *mean_rho, *hint;   /* [n_files] */
} bpmx_tempo_out;

int64_t bpmx_tempo_windows(int64_t nd, int32_t win, int32_t hop);

/* The tempogram of n_files recordings at rate sr from their envelopes in->env
 * (per-file slices at the decimated offsets of frame_offsets and ds, as for
 * bpmx_pack; nothing else of `in` is read), asynchronously on `stream`, ordered
 * after the run.  Every pointer of `out` is required.  Nothing beyond the
 * window total of the per-window arrays is written.  Never synchronises the
 * host; scratch comes from ctx.  n_files = 0 does nothing.  Two launches: one
 * workgroup per window, one wave per recording; see csrc/k_tempo.hip. */
int bpmx_tempo_device(bpmx_ctx *ctx, int32_t n_files, const int64_t *frame_offsets, int32_t ds, int32_t sr,
                      const bpmx_tempo_params *params, const bpmx_out *in, const bpmx_tempo_out *out, void *stream);

/* The HRV spectrum on the device (bpmx_hrvspec_device): per window of a
 * recording the Lomb-Scargle periodogram of its RR intervals, the power in a
 * low- and a high-frequency band and the band peaks.  The reference has no
 * such stage; this is the definition (csrc/bpmx_hrvspec_core.h states the
 * per-window arithmetic for host and device, hrv_spectrum.spectrum_ints in
 * Python the whole of it).
 *
 *   Inputs, per recording: the ascending final beats final_idx[0 .. n_final)
 *       (int32 samples at rate sr, from bpmx_beats_out, in slices at pk_off[f],
 *       with the beats status) and the recording's envelope length nd, which
 *       the host takes from frame_offsets and ds as bpmx_pack does.
 *   Intervals: interval j runs from beat j to beat j + 1; its length is d_j =
 *       idx[j + 1] - idx[j] samples and its position e_j = idx[j + 1].  It is
 *       kept iff dmin <= d_j <= dmax.  Its value is y_j = d_j * 1000.0 / sr, ms.
 *   Windows: bpmx_hrvspec_windows(nd, win, hop) = 0 for nd <= 0, win < 1 or
 *       hop < 1, 1 for nd <= win, else (nd - win) / hop + 1.  Window w holds the
 *       kept intervals with w * hop <= e_j < w * hop + win.  Outputs are ragged
 *       per window; a file's slice starts at the sum of the windows before it.
 *   Validity: the window code is the first that applies of 1 (few: fewer than
 *       min_intervals kept intervals), 2 (short: S = e_last - e_first < min_span
 *       samples), 3 (constant: all y_j equal), 0 (valid).  Every window writes
 *       n_rr and t_mid = (double)(e_first + e_last) / (2.0 * sr), NaN when n_rr
 *       is 0.  An invalid window writes NaN for var, lf, hf (and its row of q,
 *       if asked for) and -1 for both peak indices.
 *   Spectrum, for a valid window of n kept intervals: s_j = e_j - e_first (exact
 *       integers), m_y = (sum y_j) / n, u_j = y_j - m_y, w = 1 / n, omega_m =
 *       om0 + m * dom rad per sample for m < n_freq.  q[m] is the floating-mean
 *       generalised Lomb-Scargle power normalised to [0, 1]: Zechmeister and
 *       Kuerster (2009), equations 7 to 20, what scipy.signal.lombscargle(s, u,
 *       omega, normalize=True, floating_mean=True) computes, with its clamp of
 *       CC and SS at epsneg (2^-53).  var = sum w u_j^2.
 *   Bands: index ranges [lf_a, lf_b) and [hf_a, hf_b) on the grid.  lf = scale *
 *       S * var * sum_{m in LF} q[m], likewise hf.  With scale = df_hz / sr,
 *       var * q * T is the periodogram's usual A^2 T / 2, summed over the band in
 *       ms^2; that scaling is a convention, and lf / hf does not depend on it.
 *       An empty band gives 0.0 and peak -1.  The peak of a band is the index of
 *       its largest q, the smallest index among equals.
 *   Per recording: record[0] the count of valid windows, [1] and [2] the means
 *       of lf and hf over them, [3] the mean of lf / hf over the valid windows
 *       with hf > 0, [4] the mean of lf / (lf + hf) over those with lf + hf > 0,
 *       [5 .. 7] reserved NaN.  Means are added in window order and are NaN with
 *       nothing to average.
 *   Status: BPMX_HRVSPEC_OK; BPMX_HRVSPEC_NONE when the beats status is not OK
 *       or n_final < 2 (every window then has code 1 and n_rr 0);
 *       BPMX_HRVSPEC_OVERFLOW when the slice reaches past cap_peaks (nothing is
 *       written but the status).
 *
 * The order of summation, how tau is removed and how the sines are made are the
 * kernel's own: one pass over the intervals for six sums per frequency, tau
 * removed by rotating the sums, and one sincos per interval and block of 8
 * consecutive frequencies with a rotation by dom * s_j along the grid
 * (BPMX_OPT_HRVSPEC_DIRECT: one sincos per term).  q agrees with another
 * statement to (16 n + 8 omega_m S) * 2^-52 / min(CC_tau[m], SS_tau[m]), so a
 * peak decision between values closer than that may differ.
 *
 * Limits: hop >= 1, 1 <= dmin <= dmax, min_intervals >= 3, 1 <= n_freq <= 1024,
 * 0 <= a <= b <= n_freq for both bands, om0 and dom finite with om0 > 0 and
 * dom >= 0, else BPMX_E_ARG.  A window holds at most win / dmin + 1 kept
 * intervals, and a workgroup keeps four doubles of each in LDS:
 *   32 * (win / dmin + 1) <= 49152 bytes (48 KB),
 * else BPMX_E_LIMIT, before any launch.  The Python layer's defaults (120 s
 * windows, 240 BPM at most) need 15 KB. */
enum bpmx_hrvspec_status {      /* bpmx_hrvspec_out.status */
    BPMX_HRVSPEC_OK = 0,
    BPMX_HRVSPEC_NONE = -26,    /* the beats status is not OK, or fewer than two final beats */
    BPMX_HRVSPEC_OVERFLOW = -27 /* the file's slice reaches past cap_peaks: nothing written but the status */
};

enum { BPMX_HRVSPEC_RECORD = 8 };

typedef struct {
    int32_t win, hop;           /* window and step, samples */
    int32_t dmin, dmax;         /* kept intervals, samples: ceil(60 sr / max_bpm), floor(60 sr / min_bpm) */
    int32_t min_intervals;      /* a window with fewer kept intervals has code 1 */
    int32_t min_span;           /* a window spanning fewer samples has code 2: ceil(sr / f0) */
    int32_t n_freq;             /* grid points */
    int32_t lf_a, lf_b;         /* the LF band [lf_a, lf_b) on the grid */
    int32_t hf_a, hf_b;         /* the HF band [hf_a, hf_b) */
    int32_t reserved;           /* 0 */
    double om0, dom;            /* omega_m = om0 + m * dom, rad per sample */
    double scale;               /* df_hz / sr */
} bpmx_hrvspec_params;

typedef struct {            /* device */
    int32_t *code, *n_rr;       /* per window; a file's slice starts at the sum of the windows before it */
    int32_t *lf_peak, *hf_peak; /* per window: grid index or -1 */
    double *t_mid, *var, *lf, *hf;  /* per window */
    double *q;                  /* optional [windows][n_freq] */
    double *record;             /* [n_files][BPMX_HRVSPEC_RECORD] */
    int32_t *status;            /* [n_files] bpmx_hrvspec_status */
} bpmx_hrvspec_out;

int64_t bpmx_hrvspec_windows(int64_t nd, int32_t win, int32_t hop);

/* The HRV spectrum of n_files recordings at rate sr from their final beats
 * (`beats`: final_idx, n_final and status of bpmx_beats_device or
 * bpmx_marks_device over `tables`, of which pk_off and cap_peaks < 2^31 are
 * read) and their envelope lengths (frame_offsets and ds, as for bpmx_pack),
 * asynchronously on `stream`, ordered after the beat stages.  Every pointer of
 * `out` but q is required.  Nothing beyond the window total of the per-window
 * arrays or the file count of the per-file ones is written.  Never synchronises
 * the host; scratch comes from ctx.  n_files = 0 does nothing.  Two launches:
 * one workgroup per window, one wave per recording; see csrc/k_hrvspec.hip. */
int bpmx_hrvspec_device(bpmx_ctx *ctx, int32_t n_files, const int64_t *frame_offsets, int32_t ds, int32_t sr,
                        const bpmx_hrvspec_params *params, const bpmx_packed *tables, const bpmx_beats_out *beats,
                        const bpmx_hrvspec_out *out, void *stream);

/* bpmx_option bits for the entry points that take no bpmx_params
 * (BPMX_OPT_BEATS_GLOBAL, BPMX_OPT_METRICS_GLOBAL, BPMX_OPT_LABELS_GLOBAL, BPMX_OPT_SCORE_GLOBAL,
 * BPMX_OPT_MARKS_GLOBAL, BPMX_OPT_HRVSPEC_DIRECT);
 * they hold until set again. */
int bpmx_set_options(bpmx_ctx *ctx, int32_t options);

/* Synthetic int16 recordings straight into HBM: file f gets seed seed0+f,
 * frames [frame_offsets[f], frame_offsets[f+1]) of pcm (device). */
int bpmx_synth(bpmx_ctx *ctx, uint64_t seed0, int32_t n_files, const int64_t *frame_offsets, int32_t fs,
               int32_t channels, int16_t *pcm, void *stream);
/* The same generator on the host (bit-identical). */
void bpmx_synth_host(uint64_t seed, int64_t n_frames, int32_t fs, int32_t channels, int16_t *out);

/* Per-kernel device timing with HIP events recorded on the launch stream.
 * bpmx_profile(ctx, 1) starts recording; bpmx_profile_read() synchronises,
 * and writes "name launches total_ms\n" lines into buf (returns bytes). */
int bpmx_profile(bpmx_ctx *ctx, int on);
int bpmx_profile_read(bpmx_ctx *ctx, char *buf, int len);
/* Record events only around launches labelled `label` (NULL or "": every
 * launch), so a timed run can carry one kernel's device time without
 * bracketing every launch. */
int bpmx_profile_only(bpmx_ctx *ctx, const char *label);

/* Pipelined runs: batches of at least 2 * chunks recordings with ENVELOPE and
 * a detection stage run as `chunks` consecutive groups of recordings; group
 * k's envelope runs on an internal stream restricted to env_cus CUs (0: no
 * restriction) while group k-1's detection runs beside it (on an internal
 * stream restricted to det_cus other CUs when det_cus > 0, else on the
 * caller's stream), so the HBM-bound envelope kernels overlap the
 * latency-bound detection kernels.  Same outputs as an unpipelined run: every
 * index, count and flag identical, env, y and floor bit-identical, in both
 * modes (a recording's outputs do not depend on where its PCM lies: an int16
 * base a whole number of frames past a 16-byte boundary is read from that
 * boundary, so a chunk keeps the matrix-core block kernel).
 * Pipeline sub-contexts share the root context's side streams, which carry no
 * CU mask.  chunks = 0 (the default) turns it off.  Waits for the device. */
int bpmx_set_pipeline(bpmx_ctx *ctx, int chunks, int env_cus, int det_cus);

/* Counters (enum bpmx_stat) of the last bpmx_run on ctx that had
 * BPMX_OPT_STATS set: waits for that run, copies min(n, BPMX_NSTATS) of them
 * into out (zeros if none), returns BPMX_NSTATS or an error code. */
int bpmx_stats(bpmx_ctx *ctx, int64_t *out, int n);

#ifdef __cplusplus
}
#endif

#endif /* BPMX_H */
