"""ctypes binding of libbpmx.so (include/bpmx.h).

The shared library is built in-tree (``bpm_analysis_amd/libbpmx.so``, see
``csrc/Makefile`` / ``__graft_entry__.build()``).  There is no fallback: if the
library is missing or cannot be loaded this module raises, so a GPU run can
never silently compute on the CPU.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# BPMX_LIB: another build of the same library (diagnostic A/B runs of kernel variants)
LIB_PATH = os.environ.get("BPMX_LIB") or os.path.join(_HERE, "libbpmx.so")

ABI_VERSION = 4

DT_U8, DT_I16, DT_I32, DT_F32, DT_F64 = 0, 1, 2, 3, 4
DT_I24 = 5                          # packed 24-bit PCM: the int32 samples v << 8 (pcm24.Pcm24)
MODE_REFERENCE, MODE_NATIVE, MODE_RECTIFIED = 0, 1, 2
STAGE_ENVELOPE, STAGE_FLOOR, STAGE_PEAKS, STAGE_ALL = 1, 2, 4, 7
F_STATIC_FLOOR, F_DRAFT_FLOOR, F_NAN_FLOOR, F_TOO_SHORT, F_BAD_WINDOW = 1, 2, 4, 8, 16
F_TROUGH_TIE, F_PEAK_TIE = 32, 64      # decisive height tie in find_peaks' distance filter (bpmx.h)
F_TROUGH_ORDERED, F_PEAK_ORDERED = 128, 256   # that filter ran in the caller's np.argsort order (bpmx_run_ordered)
OPT_ROLLQ_MERGE = 1
OPT_NATIVE_F64 = 2
OPT_HILBERT_ROCFFT = 4
OPT_DRAFT_FULL = 8
OPT_ROLLQ_NOPRUNE = 16
OPT_DRAFT_GLOBAL_RANK = 32
OPT_ROLLQ_GLOBAL = 64
OPT_NATIVE_DMA = 128
OPT_PEAKS_GLOBAL = 256
OPT_HILBERT_R2C = 512
OPT_REF_SERIAL_MEAN = 1024
OPT_STATS = 2048
OPT_HILBERT_BLUESTEIN = 4096
OPT_REF_NOSPLIT = 8192
OPT_BEATS_GLOBAL = 16384           # bpmx_beats_device, through bpmx_set_options (test/diagnostic)
OPT_METRICS_GLOBAL = 32768         # bpmx_metrics_device, through bpmx_set_options (test/diagnostic)
OPT_RECT_SEQ = 65536               # rectified mode: the pandas recursion for every recording (test/diagnostic)
OPT_LABELS_GLOBAL = 131072          # bpmx_labels_device, through bpmx_set_options (test/diagnostic)
OPT_SCORE_GLOBAL = 262144           # bpmx_score_device, through bpmx_set_options (test/diagnostic)
OPT_MARKS_GLOBAL = 524288           # bpmx_marks_device, through bpmx_set_options (test/diagnostic)
OPT_FLOOR_ONEWG = 1048576           # the floor by one workgroup per recording, not two halves (test/diagnostic)
OPT_HRVSPEC_DIRECT = 2097152        # bpmx_hrvspec_device: one sincos per term, no rotation along the grid (test/diagnostic)
STAT_RAW_TROUGHS, STAT_UNDECIDED, STAT_FULL_DRAFT, NSTATS = 0, 1, 2, 8
STAT_FLOOR_WHOLE = 3                # recordings the half-recording floor launch handed to the whole-recording one
OK, E_ARG, E_HIP, E_LIMIT, E_NODEV = 0, -1, -2, -3, -4
BEATS_SKIPPED, BEATS_OVERFLOW = -16, -17      # bpmx_beats_out.status, beside _host.OK / _host.E_FEW_PEAKS
# bpmx_metrics_out.status: 0, the two bits, or a negative code
METRICS_OK, METRICS_TIE, METRICS_E_DISTANCE, METRICS_NONE, METRICS_OVERFLOW = 0, 1, 2, -18, -19
# bpmx_metrics_out.record (16 doubles per file, NaN = absent)
MR_AVG_BPM, MR_MIN_BPM, MR_MAX_BPM, MR_AVG_RMSSDC, MR_AVG_SDNN = 0, 1, 2, 3, 4
MR_HRR_PEAK, MR_HRR_RECOVERY_BPM, MR_HRR_VALUE, MR_RECOVERY, MR_EXERTION, METRICS_RECORD = 5, 6, 7, 8, 12, 16
# bpmx_labels_out.status, the label types and .record (4 doubles per file)
LABELS_OK, LABELS_NONE, LABELS_OVERFLOW = 0, -20, -21
LABEL_S1, LABEL_S2 = 1, 2
LR_AVG_DT, LR_AVG_BPM, LR_N_S1, LR_N_S2, LABELS_RECORD = 0, 1, 2, 3, 4
# bpmx_score_out.status (0, the bit, or a negative code), the mark kinds and .record (20 int64 per file)
SCORE_OK, SCORE_NO_LABELS, SCORE_NONE, SCORE_OVERFLOW = 0, 1, -22, -23
SCORE_OUTSIDE, SCORE_TP, SCORE_SWAP, SCORE_FP, SCORE_FN = 0, 1, 2, 3, 3
SR_N_REF, SR_N_DET, SR_TP, SR_SWAP, SR_FP, SR_FN, SR_SUM_ERR, SR_SUM_ABS, SR_MAX_ABS = 0, 1, 2, 3, 4, 5, 6, 7, 8
SR_PER_TYPE, SR_N_OUTSIDE, SR_N_SPANS, SCORE_RECORD = 9, 18, 19, 20
# bpmx_marks_device: the two statuses it adds to bpmx_beats_out.status, and its record (8 int32 per file)
MARKS_FEW, MARKS_OVERFLOW = -24, -25
MK_N_ROWS, MK_N_S1, MK_N_S2, MK_N_MERGED, MK_N_DROPPED, MK_N_OTHER, MARKS_RECORD = 0, 1, 2, 3, 4, 5, 8
# bpmx_trace_out.record (bpmx_trace_field: 18 doubles per raw peak), .code (bpmx_trace_code) and .gap
TR_BLEND, TR_BASE_CONF, TR_STAB_FACTOR, TR_STAB_RATIO, TR_ADJ_AMOUNT, TR_ADJ_RATIO, TR_ADJ_RMAX = 0, 1, 2, 3, 4, 5, 6
TR_IV_AMOUNT, TR_IV_GAP, TR_IV_CAP, TR_FINAL = 7, 8, 9, 10
TR_L_RHYTHM, TR_L_RR, TR_L_EXPECTED, TR_L_AMP, TR_L_RATIO, TR_L_CONF, TR_L_IMPLIED, TR_NFIELDS = 11, 12, 13, 14, 15, 16, 17, 18
TR_S1_PAIRED, TR_S2_PAIRED, TR_LONE_VALID, TR_FIRST_BEAT, TR_LAST_PEAK, TR_CASCADE, TR_NOISE, TR_OUTCOME = 1, 2, 3, 4, 5, 6, 7, 15
TRF_STABILITY, TRF_PENALIZED, TRF_BOOSTED, TRF_INTERVAL, TRF_FORWARD = 16, 32, 64, 128, 256
TR_GAP_NONE, TR_GAP_S1, TR_GAP_S2 = 0, 1, 2

EXPORTS = ["bpmx_abi_version", "bpmx_last_error", "bpmx_create", "bpmx_destroy", "bpmx_decimated_length",
           "bpmx_run", "bpmx_run_ordered", "bpmx_pack", "bpmx_synth", "bpmx_synth_host", "bpmx_profile", "bpmx_profile_read", "bpmx_profile_only",
           "bpmx_stats", "bpmx_set_pipeline", "bpmx_beats_device", "bpmx_set_options", "bpmx_metrics_device",
           "bpmx_beats_device_ex", "bpmx_pack_trough_floor", "bpmx_plot_length", "bpmx_pack_plot",
           "bpmx_labels_device", "bpmx_score_device", "bpmx_marks_device", "bpmx_tempo_windows",
           "bpmx_tempo_device", "bpmx_hrvspec_windows", "bpmx_hrvspec_device"]


class Params(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int32), ("stages", ctypes.c_int32), ("dtype", ctypes.c_int32),
                ("channels", ctypes.c_int32), ("fs", ctypes.c_int32), ("ds", ctypes.c_int32),
                ("sr", ctypes.c_int32), ("env_window", ctypes.c_int32), ("distance", ctypes.c_int32),
                ("noise_window", ctypes.c_int32), ("min_periods", ctypes.c_int32), ("options", ctypes.c_int32),
                ("trough_prom_q", ctypes.c_double), ("peak_prom_q", ctypes.c_double),
                ("noise_floor_q", ctypes.c_double), ("fallback_q", ctypes.c_double),
                ("reject_mult", ctypes.c_double),
                ("ba_b", ctypes.c_double * 5), ("ba_a", ctypes.c_double * 5), ("ba_zi", ctypes.c_double * 4),
                ("sos", ctypes.c_double * 12), ("sos_zi", ctypes.c_double * 4)]


class Batch(ctypes.Structure):
    _fields_ = [("n_files", ctypes.c_int32), ("reserved", ctypes.c_int32), ("pcm", ctypes.c_void_p),
                ("frame_offsets", ctypes.POINTER(ctypes.c_int64))]


class Out(ctypes.Structure):
    _fields_ = [("env", ctypes.c_void_p), ("floor", ctypes.c_void_p), ("y", ctypes.c_void_p),
                ("troughs", ctypes.c_void_p), ("peaks", ctypes.c_void_p), ("n_troughs", ctypes.c_void_p),
                ("n_peaks", ctypes.c_void_p), ("flags", ctypes.c_void_p), ("n_raw_troughs", ctypes.c_void_p)]


class PeakOrder(ctypes.Structure):
    """bpmx_peak_order: per search (0 = troughs, 1 = raw peaks) the candidate
    export and the caller's visiting ranks (device pointers or None)."""
    _fields_ = [("cand", ctypes.c_void_p * 2), ("n_cand", ctypes.c_void_p * 2),
                ("rank", ctypes.c_void_p * 2), ("use_rank", ctypes.c_void_p * 2)]


class PackedOut(ctypes.Structure):
    """bpmx_packed: the ragged per-peak / per-trough tables and the int16 debug
    samples bpmx_pack writes (device pointers; None leaves that part out)."""
    _fields_ = [("cap_peaks", ctypes.c_int64), ("cap_troughs", ctypes.c_int64),
                ("pk_off", ctypes.c_void_p), ("tr_off", ctypes.c_void_p),
                ("pk_idx", ctypes.c_void_p), ("pk_env", ctypes.c_void_p), ("pk_floor", ctypes.c_void_p),
                ("tr_idx", ctypes.c_void_p), ("tr_env", ctypes.c_void_p),
                ("y16", ctypes.c_void_p), ("y_max", ctypes.c_void_p)]


class BeatsOut(ctypes.Structure):
    """bpmx_beats_out: the device arrays bpmx_beats_device fills (per-file
    slices at pk_off[f]; pass and tags may be None)."""
    _fields_ = [("final_idx", ctypes.c_void_p), ("n_final", ctypes.c_void_p), ("bpm_t", ctypes.c_void_p),
                ("bpm", ctypes.c_void_p), ("n_bpm", ctypes.c_void_p), ("pass_", ctypes.c_void_p),
                ("tags", ctypes.c_void_p), ("status", ctypes.c_void_p)]


class TraceOut(ctypes.Structure):
    """bpmx_trace_out: the device arrays of the decision trace
    bpmx_beats_device_ex fills (per-file slices at pk_off[f]; every pointer
    required)."""
    _fields_ = [(k, ctypes.c_void_p) for k in ("record", "code", "lt_pos", "lt_bpm", "n_lt", "dev_t", "dev", "gap")]


class MetricParams(ctypes.Structure):
    """bpmx_metric_params: the two HRV keys of DEFAULT_PARAMS and the defaults
    the reference calls its slope, HRR and incline / decline functions with."""
    _fields_ = [("hrv_window_size_beats", ctypes.c_int32), ("hrv_step_size_beats", ctypes.c_int32),
                ("min_duration_sec", ctypes.c_double), ("min_bpm_change", ctypes.c_double),
                ("prominence", ctypes.c_double), ("slope_window_sec", ctypes.c_double),
                ("hrr_interval_sec", ctypes.c_double)]


def metric_params(params: dict) -> MetricParams:
    return MetricParams(int(params["hrv_window_size_beats"]), int(params["hrv_step_size_beats"]),
                        10.0, 15.0, 5.0, 20.0, 60.0)


class MetricsOut(ctypes.Structure):
    """bpmx_metrics_out: the device arrays bpmx_metrics_device fills (per-file
    slices at pk_off[f]; every pointer required)."""
    _fields_ = [(k, ctypes.c_void_p) for k in (
        "hrv_time", "hrv_rmssdc", "hrv_sdnn", "hrv_bpm", "n_hrv", "inc_a", "inc_b", "dec_a", "dec_b",
        "inc_slope", "inc_dur", "dec_slope", "dec_dur", "n_inc", "n_dec", "record", "status")]


class LabelParams(ctypes.Structure):
    """bpmx_label_params: the gap that separates two groups of S1 marks."""
    _fields_ = [("gap_sec", ctypes.c_double)]


class LabelsOut(ctypes.Structure):
    """bpmx_labels_out: the device arrays bpmx_labels_device fills (per-file
    slices at pk_off[f]; every pointer required)."""
    _fields_ = [(k, ctypes.c_void_p) for k in (
        "lb_pos", "lb_type", "lb_time", "lb_bpm", "pr_s1", "pr_s2", "pr_dt", "gr_id", "gr_first", "gr_last",
        "gr_s1", "gr_pairs", "gr_dt", "gr_bpm", "n_labels", "n_pairs", "n_groups", "record", "status")]


class ScoreParams(ctypes.Structure):
    """bpmx_score_params: the matching tolerance and the pause that ends a labelled span, milliseconds."""
    _fields_ = [("tol_ms", ctypes.c_int32), ("gap_ms", ctypes.c_int32)]


class RefMarks(ctypes.Structure):
    """bpmx_ref_marks: the corrected marks as a ragged device table (labels.marks_from_table)."""
    _fields_ = [("cap_ref", ctypes.c_int64), ("rf_off", ctypes.c_void_p), ("rf_ms", ctypes.c_void_p),
                ("rf_type", ctypes.c_void_p)]


class ScoreOut(ctypes.Structure):
    """bpmx_score_out: the device arrays bpmx_score_device fills (the four
    row arrays in slices at pk_off[f] / rf_off[f], all of them or none)."""
    _fields_ = [(k, ctypes.c_void_p) for k in ("sc_kind", "sc_ref", "rf_kind", "rf_det", "record", "status")]


class MarksParams(ctypes.Structure):
    """bpmx_marks_params: the curve's smoothing window (output_smoothing_window_sec), seconds."""
    _fields_ = [("smoothing_window_sec", ctypes.c_double)]


class TempoParams(ctypes.Structure):
    """bpmx_tempo_params: window, step and lag range in samples, the strength a
    window counts from, and how many windows the hint may come from."""
    _fields_ = [("win", ctypes.c_int32), ("hop", ctypes.c_int32), ("kmin", ctypes.c_int32), ("kmax", ctypes.c_int32),
                ("min_strength", ctypes.c_double), ("start_windows", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class TempoOut(ctypes.Structure):
    """bpmx_tempo_out: the device arrays bpmx_tempo_device fills (per window,
    then per file; every pointer required)."""
    _fields_ = [(k, ctypes.c_void_p) for k in ("lag", "rho", "bpm", "n_valid", "n_strong", "median_bpm", "mean_rho",
                                               "hint")]


class HrvspecParams(ctypes.Structure):
    """bpmx_hrvspec_params: window, step, interval range, validity limits, the
    frequency grid and the two bands as index ranges on it."""
    _fields_ = [(k, ctypes.c_int32) for k in ("win", "hop", "dmin", "dmax", "min_intervals", "min_span", "n_freq",
                                              "lf_a", "lf_b", "hf_a", "hf_b", "reserved")] + \
               [(k, ctypes.c_double) for k in ("om0", "dom", "scale")]


class HrvspecOut(ctypes.Structure):
    """bpmx_hrvspec_out: the device arrays bpmx_hrvspec_device fills (per
    window, then per file; q is optional)."""
    _fields_ = [(k, ctypes.c_void_p) for k in ("code", "n_rr", "lf_peak", "hf_peak", "t_mid", "var", "lf", "hf", "q",
                                               "record", "status")]


HRVSPEC_OK, HRVSPEC_NONE, HRVSPEC_OVERFLOW, HRVSPEC_RECORD = 0, -26, -27, 8


def hrvspec_params(g: dict) -> HrvspecParams:
    """``hrv_spectrum.geometry``'s dict as the structure."""
    return HrvspecParams(*[int(g[k]) for k in ("win", "hop", "dmin", "dmax", "min_intervals", "min_span", "n_freq",
                                               "lf_a", "lf_b", "hf_a", "hf_b")], 0,
                         float(g["om0"]), float(g["dom"]), float(g["scale"]))


class BpmxError(RuntimeError):
    """A libbpmx failure.  ``code`` is the BPMX_E_* status (None when raised by
    the host side).  Only argument and size-limit errors belong to the
    recordings of one call (``per_file``); a HIP or device failure means the
    GPU path itself failed and must stop the run."""

    def __init__(self, msg: str = "", code: int = None):
        super().__init__(msg)
        self.code = code

    @property
    def per_file(self) -> bool:
        return self.code in (E_ARG, E_LIMIT)


class BpmxArgError(BpmxError, ValueError):
    """BPMX_E_ARG: an argument the reference's own calls reject with ValueError
    (scipy find_peaks' distance check, pandas' rolling-window checks); the
    message is the library's, which repeats the reference-side wording."""


_lib = None


def load() -> ctypes.CDLL:
    """Load libbpmx.so (raises if it is missing: there is no CPU fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BpmxError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        f"or `make -C bpm_analysis_amd/csrc` (there is no CPU fallback)")
    L = ctypes.CDLL(LIB_PATH)
    P, I32, I64, U64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64
    L.bpmx_abi_version.restype = ctypes.c_int
    L.bpmx_last_error.restype = ctypes.c_char_p
    L.bpmx_create.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    L.bpmx_create.restype = ctypes.c_int
    L.bpmx_destroy.argtypes = [P]
    L.bpmx_destroy.restype = None
    L.bpmx_decimated_length.argtypes = [I64, I32]
    L.bpmx_decimated_length.restype = I64
    L.bpmx_run.argtypes = [P, ctypes.POINTER(Params), ctypes.POINTER(Batch), ctypes.POINTER(Out), P]
    L.bpmx_run.restype = ctypes.c_int
    L.bpmx_run_ordered.argtypes = [P, ctypes.POINTER(Params), ctypes.POINTER(Batch), ctypes.POINTER(Out),
                                   ctypes.POINTER(PeakOrder), P]
    L.bpmx_run_ordered.restype = ctypes.c_int
    L.bpmx_pack.argtypes = [P, I32, ctypes.POINTER(ctypes.c_int64), I32, ctypes.POINTER(Out),
                            ctypes.POINTER(PackedOut), P]
    L.bpmx_pack.restype = ctypes.c_int
    L.bpmx_synth.argtypes = [P, U64, I32, ctypes.POINTER(ctypes.c_int64), I32, I32, P, P]
    L.bpmx_synth.restype = ctypes.c_int
    L.bpmx_synth_host.argtypes = [U64, I64, I32, I32, P]
    L.bpmx_synth_host.restype = None
    L.bpmx_profile.argtypes = [P, ctypes.c_int]
    L.bpmx_profile.restype = ctypes.c_int
    L.bpmx_profile_read.argtypes = [P, ctypes.c_char_p, ctypes.c_int]
    L.bpmx_profile_read.restype = ctypes.c_int
    L.bpmx_profile_only.argtypes = [P, ctypes.c_char_p]
    L.bpmx_profile_only.restype = ctypes.c_int
    L.bpmx_stats.argtypes = [P, ctypes.POINTER(ctypes.c_int64), ctypes.c_int]
    L.bpmx_stats.restype = ctypes.c_int
    L.bpmx_set_pipeline.argtypes = [P, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.bpmx_set_pipeline.restype = ctypes.c_int
    if hasattr(L, "bpmx_beats_device"):      # an older build fails the ABI check below, not here
        from ._host import BeatParams
        L.bpmx_beats_device.argtypes = [P, I32, I32, ctypes.POINTER(BeatParams), ctypes.c_double,
                                        ctypes.POINTER(PackedOut), P, ctypes.POINTER(BeatsOut), P]
        L.bpmx_beats_device.restype = ctypes.c_int
        L.bpmx_set_options.argtypes = [P, I32]
        L.bpmx_set_options.restype = ctypes.c_int
    if hasattr(L, "bpmx_metrics_device"):
        L.bpmx_metrics_device.argtypes = [P, I32, I32, ctypes.POINTER(MetricParams), I64, ctypes.POINTER(PackedOut),
                                          ctypes.POINTER(BeatsOut), ctypes.POINTER(MetricsOut), P]
        L.bpmx_metrics_device.restype = ctypes.c_int
    if hasattr(L, "bpmx_beats_device_ex"):
        from ._host import BeatParams
        L.bpmx_beats_device_ex.argtypes = [P, I32, I32, ctypes.POINTER(BeatParams), ctypes.c_double,
                                           ctypes.POINTER(PackedOut), P, ctypes.POINTER(BeatsOut), P,
                                           ctypes.POINTER(TraceOut), P]
        L.bpmx_beats_device_ex.restype = ctypes.c_int
        L.bpmx_pack_trough_floor.argtypes = [P, ctypes.POINTER(Out), ctypes.POINTER(ctypes.c_int64), I32, I32,
                                             ctypes.POINTER(PackedOut), P, P]
        L.bpmx_pack_trough_floor.restype = ctypes.c_int
    if hasattr(L, "bpmx_pack_plot"):
        L.bpmx_plot_length.argtypes = [I64, I32]
        L.bpmx_plot_length.restype = I64
        L.bpmx_pack_plot.argtypes = [P, I32, ctypes.POINTER(ctypes.c_int64), I32, I32, ctypes.POINTER(Out), P, P,
                                     I64, P]
        L.bpmx_pack_plot.restype = ctypes.c_int
    if hasattr(L, "bpmx_labels_device"):
        L.bpmx_labels_device.argtypes = [P, I32, I32, ctypes.POINTER(LabelParams), ctypes.POINTER(PackedOut),
                                         ctypes.POINTER(BeatsOut), P, ctypes.POINTER(LabelsOut), P]
        L.bpmx_labels_device.restype = ctypes.c_int
    if hasattr(L, "bpmx_score_device"):
        L.bpmx_score_device.argtypes = [P, I32, ctypes.POINTER(ScoreParams), ctypes.POINTER(PackedOut),
                                        ctypes.POINTER(LabelsOut), ctypes.POINTER(RefMarks),
                                        ctypes.POINTER(ScoreOut), P]
        L.bpmx_score_device.restype = ctypes.c_int
    if hasattr(L, "bpmx_marks_device"):
        L.bpmx_marks_device.argtypes = [P, I32, I32, ctypes.POINTER(MarksParams), ctypes.POINTER(RefMarks), P,
                                        ctypes.POINTER(PackedOut), ctypes.POINTER(BeatsOut), P, P, P]
        L.bpmx_marks_device.restype = ctypes.c_int
    if hasattr(L, "bpmx_tempo_device"):
        L.bpmx_tempo_windows.argtypes = [I64, I32, I32]
        L.bpmx_tempo_windows.restype = I64
        L.bpmx_tempo_device.argtypes = [P, I32, ctypes.POINTER(ctypes.c_int64), I32, I32,
                                        ctypes.POINTER(TempoParams), ctypes.POINTER(Out), ctypes.POINTER(TempoOut), P]
        L.bpmx_tempo_device.restype = ctypes.c_int
    if hasattr(L, "bpmx_hrvspec_device"):
        L.bpmx_hrvspec_windows.argtypes = [I64, I32, I32]
        L.bpmx_hrvspec_windows.restype = I64
        L.bpmx_hrvspec_device.argtypes = [P, I32, ctypes.POINTER(ctypes.c_int64), I32, I32,
                                          ctypes.POINTER(HrvspecParams), ctypes.POINTER(PackedOut),
                                          ctypes.POINTER(BeatsOut), ctypes.POINTER(HrvspecOut), P]
        L.bpmx_hrvspec_device.restype = ctypes.c_int
    if L.bpmx_abi_version() != ABI_VERSION:
        raise BpmxError(f"libbpmx ABI {L.bpmx_abi_version()} != expected {ABI_VERSION}; rebuild")
    _lib = L
    return L


def check(rc: int, what: str) -> None:
    if rc != OK:
        msg = load().bpmx_last_error().decode(errors="replace")
        if rc == E_ARG:
            raise BpmxArgError(msg, rc)
        raise BpmxError(f"{what} failed ({rc}): {msg}", rc)
