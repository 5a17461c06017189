"""Drop-in replacements for the reference's hot-path functions.

Same names, arguments, return types, log lines and exceptions as
pixeru/bpm_analysis (bpm_analysis.py):

* ``preprocess_audio(file_path, params, output_directory) -> (env, sr)``   :1007-1062
* ``_calculate_dynamic_noise_floor(env, sr, params) -> (pd.Series, troughs)`` :1064-1117
* ``find_raw_peaks(env, sr, params, height_threshold) -> peaks``          :223-229
  (the body of ``PeakClassifier._find_raw_peaks``)

plus the batch entry points the reference lacks (``analyze_batch``,
``analyze_wav_files``), the labeler's envelope of a filtered WAV
(``labeler_envelope``, heartbeat_labeler.py:53-67) and
``patch_reference(module)``, which rebinds an imported reference module's
three hot-path functions to these so its unchanged ``analyze_wav_file``
(and therefore gui.py / main.py / the Gradio app) runs on the GPU.

All numerics run in libbpmx.so; this module only reads files, moves arrays
and formats results.
"""
from __future__ import annotations

import logging
import os
import threading
import warnings
from typing import Dict, List, Sequence, Tuple

import numpy as np

from . import _native as N
from .config import DEFAULT_PARAMS
from .engine import default_detector, mode_design

RECTIFIED = "rectified"
NO_DEBUG_WAV_MSG = "Rectified mode reads an already filtered WAV: 'save_filtered_wav' is ignored."

PADLEN_MSG = "The length of the input vector x must be greater than padlen, which is 15."
DISTANCE_MSG = "`distance` must be greater or equal to 1"          # scipy find_peaks (:1070, :227)


def _window_error(params: Dict, sample_rate: int) -> ValueError:
    """pandas' rolling() check of the noise window (bpm_analysis.py:1084-1085)."""
    return ValueError(f"min_periods 3 must be <= window {int(params['noise_window_sec'] * sample_rate)}")


def _file_error(flags: int, params: Dict, sr: int):
    """The exception the reference raises for a recording flagged by the library, or None."""
    if flags & N.F_TOO_SHORT:
        return ValueError(PADLEN_MSG)
    if flags & N.F_BAD_WINDOW:
        return _window_error(params, sr)
    return None


TIE_MSG = ("find_peaks' distance filter met equal-height {what} closer than `distance`: numpy's argsort order "
           "for equal heights is implementation-defined, so these {what} may differ from the reference's on "
           "this machine (bpmx keeps the later index).")
ORDERED_MSG = ("find_peaks' distance filter met equal-height {what} closer than `distance`; decided in numpy's "
               "argsort order, as the reference's own call does on this machine.")


def _warn_ties(flags: int, what: str) -> None:
    """Report a decisive tie (include/bpmx.h BPMX_F_TROUGH_TIE / BPMX_F_PEAK_TIE).

    The drop-in entry points run with ``resolve_ties`` (engine.Detector.resolve_ties),
    so a flagged recording has been re-decided in numpy's order and carries
    F_*_ORDERED instead (a debug line); the warning is left for a result that
    still holds the library's stable order."""
    tie = N.F_TROUGH_TIE if what == "troughs" else N.F_PEAK_TIE
    ordered = N.F_TROUGH_ORDERED if what == "troughs" else N.F_PEAK_ORDERED
    if flags & tie:
        logging.warning(TIE_MSG.format(what=what))
    elif flags & ordered:
        logging.debug(ORDERED_MSG.format(what=what))


def _read_wav(file_path: str, packed24: bool = False):
    """scipy's read; packed24: a plain 24-bit PCM file as ``pcm24.Pcm24``, its samples not expanded."""
    if packed24:
        from .pcm24 import read_wav
        return read_wav(file_path)
    from scipy.io import wavfile
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return wavfile.read(file_path)


def _write_debug_wavs(file_path: str, output_directory: str, sr: int, y16: np.ndarray) -> None:
    """Both debug WAVs of the reference (next to the input, :1047-1050, and in
    the output directory, :1056-1060) from the samples the device quantised
    (bpmx_pack's y16: np.int16(y / np.max(np.abs(y)) * 32767), value for value)."""
    from scipy.io import wavfile
    y16 = np.ascontiguousarray(y16, dtype=np.int16)
    wavfile.write(f"{os.path.splitext(file_path)[0]}_filtered_debug.wav", sr, y16)
    base = os.path.basename(os.path.splitext(file_path)[0])
    wavfile.write(os.path.join(output_directory, f"{base}_filtered_debug.wav"), sr, y16)


# ---------------------------------------------------------------- one GPU run per file
# analyze_wav_file calls preprocess_audio (:1731), then _calculate_dynamic_noise_floor
# on the envelope it returned (:1732), then _find_raw_peaks with that floor twice (the
# preliminary pass :1635 and the main pass :1740, both via :89).  preprocess_audio
# therefore runs every stage in one batch and keeps this thread's last recording; the
# later calls are answered from it when their envelope is byte-identical to the one
# returned, their parameters give the same detection settings and (for the peaks) the
# height is that floor.  Anything else runs on the GPU as before.
class _LastRecording(threading.local):
    def __init__(self):
        self.rec = None


_last = _LastRecording()


def _floor_key(params: Dict, sr: int):
    return (sr, int(params["min_peak_distance_sec"] * sr), float(params["trough_prominence_quantile"]),
            int(params["noise_window_sec"] * sr), float(params["noise_floor_quantile"]),
            float(params.get("trough_rejection_multiplier", 4.0)))


def _peak_key(params: Dict, sr: int):
    return (sr, int(params["min_peak_distance_sec"] * sr), float(params["peak_prominence_quantile"]))


def _same_bytes(a: np.ndarray, b: np.ndarray) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _cached(env: np.ndarray, sr: int, key_name: str, key) -> dict:
    rec = _last.rec
    if rec is None or rec[key_name] != key or not _same_bytes(rec["env"], env):
        return None
    return rec


def preprocess_audio(file_path: str, params: Dict, output_directory: str, mode: str = None,
                     device: int = 0) -> Tuple[np.ndarray, int]:
    """Reads, filters, and prepares the audio envelope for analysis (on the GPU).

    ``mode`` (or ``params["bpmx_mode"]`` when called through the reference's
    unchanged ``analyze_wav_file``): "reference" (default, bit-exact with the
    shipped pipeline), "native" (sosfiltfilt at fs -> decimate -> |hilbert|) or
    "rectified" (the file is an already filtered WAV: the labeler's envelope
    |x| -> rolling mean at the file's own rate; no filter, so no debug WAV, no
    padlen error and no Nyquist check).
    The noise floor, troughs and raw peaks of the same recording are computed
    in the same GPU run and kept for the calls that follow (see _LastRecording)."""
    if mode is None:
        mode = params.get("bpmx_mode", "reference")
    rect = mode == RECTIFIED
    save_debug_file = params["save_filtered_wav"]
    if rect and save_debug_file:
        logging.info(NO_DEBUG_WAV_MSG)
        save_debug_file = False
    sample_rate, audio = _read_wav(file_path)
    d = mode_design(sample_rate, params, mode, log=True)
    n = audio.shape[0]
    if not rect and -(-n // d.ds) <= 15:
        raise ValueError(PADLEN_MSG)
    _last.rec = None
    stages = N.STAGE_ALL if d.distance >= 1 else N.STAGE_ENVELOPE     # distance < 1 raises in the later calls
    det = default_detector(device)

    def run(st):
        if save_debug_file:
            return det.run_host_y16([audio], sample_rate, params, mode=mode, stages=st, resolve_ties=True)[0]
        return det.run_host([audio], sample_rate, params, mode=mode, stages=st, resolve_ties=True)[0]

    try:
        r = run(stages)
    except N.BpmxError as exc:
        if stages == N.STAGE_ENVELOPE or not exc.per_file:
            raise
        # a detection-stage limit (e.g. a noise window beyond the kernels): the
        # envelope alone now, so the error surfaces from the floor call as in
        # the reference (:1732), after the debug WAV is written
        stages = N.STAGE_ENVELOPE
        r = run(stages)
    if save_debug_file:
        _write_debug_wavs(file_path, output_directory, d.sr, r["y16"])
    env = np.array(r["env"])
    if stages == N.STAGE_ALL:
        _last.rec = {"env": env.copy(), "floor_key": _floor_key(params, d.sr), "peak_key": _peak_key(params, d.sr),
                     "floor": np.array(r["floor"]), "troughs": np.array(r["troughs"]), "peaks": np.array(r["peaks"]),
                     "flags": r["flags"], "n_raw_troughs": r["n_raw_troughs"]}
    return env, d.sr


def _series(values: np.ndarray):
    import pandas as pd
    return pd.Series(values, index=np.arange(len(values)))


def _calculate_dynamic_noise_floor(audio_envelope: np.ndarray, sample_rate: int, params: Dict, device: int = 0):
    """Calculates a dynamic noise floor based on a sanitized set of audio troughs (on the GPU)."""
    env = np.ascontiguousarray(audio_envelope, dtype=np.float64)
    if int(params["min_peak_distance_sec"] * sample_rate) < 1:
        raise ValueError(DISTANCE_MSG)
    r = _cached(env, sample_rate, "floor_key", _floor_key(params, sample_rate))
    if r is None:
        r = default_detector(device).run_env_host([env], sample_rate, params, N.STAGE_FLOOR, resolve_ties=True)[0]
    fl = r["flags"]
    if fl & N.F_BAD_WINDOW:
        raise _window_error(params, sample_rate)
    _warn_ties(fl, "troughs")
    if fl & N.F_STATIC_FLOOR:
        logging.warning("Not enough troughs found for sanitization. Using a static noise floor.")
        return _series(np.array(r["floor"])), np.array(r["troughs"], dtype=np.int64)
    logging.info(f"Trough Sanitization: Kept {len(r['troughs'])} of {r['n_raw_troughs']} initial troughs.")
    if fl & N.F_DRAFT_FLOOR:
        logging.warning("Not enough sanitized troughs remaining. Using non-sanitized floor as fallback.")
    troughs = [np.int64(t) for t in r["troughs"]]
    return _series(np.array(r["floor"])), np.array(troughs)


def find_raw_peaks(audio_envelope: np.ndarray, sample_rate: int, params: Dict, height_threshold: np.ndarray,
                   device: int = 0) -> np.ndarray:
    """Finds all potential peaks above the given height threshold (on the GPU)."""
    env = np.ascontiguousarray(audio_envelope, dtype=np.float64)
    if int(params["min_peak_distance_sec"] * sample_rate) < 1:
        raise ValueError(DISTANCE_MSG)
    floor = np.ascontiguousarray(np.broadcast_to(np.asarray(height_threshold, dtype=np.float64), env.shape))
    r = _cached(env, sample_rate, "peak_key", _peak_key(params, sample_rate))
    if r is None or not _same_bytes(r["floor"], floor):
        r = default_detector(device).run_env_host([env], sample_rate, params, N.STAGE_PEAKS, floors=[floor],
                                                  resolve_ties=True)[0]
    peaks = np.array(r["peaks"], dtype=np.int64)
    _warn_ties(r["flags"], "peaks")
    logging.info(f"Found {len(peaks)} raw peaks using dynamic height threshold.")
    return peaks


def labeler_envelope(file_path: str, device: int = 0) -> Tuple[np.ndarray, int]:
    """The envelope heartbeat_labeler.py:53-67 shows for a filtered WAV, on the
    GPU: channel mean, ``np.abs``, the centred pandas rolling mean over
    ``sample_rate // 10`` samples, bit for bit -> (envelope, sample_rate)."""
    sample_rate, audio = _read_wav(file_path)
    r = default_detector(device).run_host([audio], sample_rate, DEFAULT_PARAMS, mode=RECTIFIED,
                                          stages=N.STAGE_ENVELOPE)[0]
    return np.array(r["env"]), sample_rate


def detect(pcm: np.ndarray, fs: int, params: Dict, mode: str = "reference", device: int = 0) -> dict:
    """The whole hot path for one in-memory recording -> dict(env, floor, troughs, peaks, sr, flags)."""
    return analyze_batch([pcm], fs, params, mode=mode, device=device)[0]


def analyze_batch(recordings: Sequence[np.ndarray], fs: int, params: Dict, mode: str = "reference",
                  device: int = 0) -> List[dict]:
    """Filter -> envelope -> noise floor -> raw peaks for many recordings in one launch sequence.

    Recordings share fs, sample format and channel count; lengths may differ.
    A recording too short for filtfilt (Nd <= 15) comes back with
    ``flags & F_TOO_SHORT`` and no outputs instead of failing the batch.
    """
    mode_design(fs, params, mode, log=True)   # Nyquist check / clamp warnings once per batch (none when rectified)
    return default_detector(device).run_host(list(recordings), fs, params, mode=mode, stages=N.STAGE_ALL,
                                             resolve_ties=True)


def analyze_wav_files(file_paths: Sequence[str], params: Dict, output_directory: str, mode: str = None,
                      device: int = 0, packed24: bool = False) -> List[dict]:
    """Batched file entry point: what ``preprocess_audio`` + the noise floor +
    the raw-peak call do per file (bpm_analysis.py:1007-1062, :1064-1117,
    :223-229), for many WAV files in few launch sequences.

    Files are read with ``scipy.io.wavfile`` (the reference's dtype rules:
    u8 / i16 / i32 (PCM24 and PCM32) / f32 / f64, stereo averaged on the
    device), grouped by (sample rate, sample format, channels) and run as one
    ragged batch per group.  With ``params["save_filtered_wav"]`` both debug
    WAVs of the reference are written (next to the input and into
    ``output_directory``).  Returns one dict per path, in order: env, floor,
    troughs, peaks, sr, flags, or ``error`` (the exception the reference would
    raise for that file, e.g. the filtfilt padlen ValueError).

    ``packed24=True``: 24-bit PCM files are read by ``pcm24.read_wav`` and
    uploaded as they lie in the file (3 bytes per sample, a format group of
    their own); the results are those of the int32 array scipy makes of them."""
    if mode is None:
        mode = params.get("bpmx_mode", "reference")
    rect = mode == RECTIFIED
    save = bool(params.get("save_filtered_wav", False))
    if rect and save:
        logging.info(NO_DEBUG_WAV_MSG)
        save = False
    out: List[dict] = [None] * len(file_paths)
    groups: Dict[tuple, List[int]] = {}
    audio = []
    for k, path in enumerate(file_paths):
        try:
            fs, a = _read_wav(path, packed24)
        except Exception as exc:                      # wavfile errors propagate per file, as in the GUI loop
            out[k] = {"error": exc}
            audio.append(None)
            continue
        audio.append((fs, a))
        key = (fs, a.dtype.str, 1 if a.ndim == 1 else a.shape[1])
        groups.setdefault(key, []).append(k)
    det = default_detector(device)
    for (fs, _, _), idx in groups.items():
        try:
            d = mode_design(fs, params, mode, log=True)   # clamp warnings / Nyquist ValueError, once per group
        except ValueError as exc:
            for k in idx:
                out[k] = {"error": exc}
            continue
        try:
            if d.distance < 1:
                raise ValueError(DISTANCE_MSG)
            run = det.run_host_y16 if save else det.run_host      # the debug WAV's int16 samples, not y as f64
            res = run([audio[k][1] for k in idx], fs, params, mode=mode, stages=N.STAGE_ALL, resolve_ties=True)
        except (ValueError, N.BpmxError) as exc:      # reported per file, as the GUI loop does (gui.py:247-251)
            if isinstance(exc, N.BpmxError) and not exc.per_file:
                raise                                 # HIP / device failure: not a per-file error
            for k in idx:                             # (a too-short file fails first, in filtfilt)
                short = not rect and -(-audio[k][1].shape[0] // d.ds) <= 15
                out[k] = {"error": ValueError(PADLEN_MSG) if short else exc}
            continue
        for k, r in zip(idx, res):
            err = _file_error(r["flags"], params, d.sr)
            if err is not None:
                out[k] = {"error": err}
                continue
            if save:
                _write_debug_wavs(file_paths[k], output_directory, d.sr, r["y16"])
            out[k] = {key: r[key] for key in ("env", "floor", "troughs", "peaks", "sr", "flags")}
    return out


def analyze_wav_files_to_reports(file_paths: Sequence[str], params: Dict, output_directory: str,
                                 start_bpm_hints: Sequence = None, original_file_paths: Sequence[str] = None,
                                 mode: str = None, device: int = 0, plot: bool = False, labels: bool = False,
                                 label_gap_sec: float = 5.0, labels_overwrite: bool = False,
                                 packed24: bool = False, tempo: bool = False,
                                 hrv_spectrum: bool = False) -> List[dict]:
    """``beats.analyze_wav_file`` for many WAV files with every stage on the
    device: per file ``<base>_bpm_plot.csv``, ``<base>_Analysis_Summary.md``,
    ``<base>_Debug_Log.md`` and ``<base>_Analysis_Settings.json`` (and both
    debug WAVs with ``params["save_filtered_wav"]``), byte for byte what
    ``analyze_wav_file`` writes apart from the markdown files' timestamp line.
    With ``plot=True`` the interactive plot ``<base>_bpm_plot.html`` is written
    too, before the other files as ``analyze_wav_file`` does, and the figure is
    returned as the dict's ``figure`` (what the Gradio app displays): its two
    line traces come from ``Detector.pack_plot`` (the envelope and the floor at
    every ``plot_downsample_factor``-th sample), everything else from the
    tables, through ``plot.write_plot_packed``.

    Files are read and grouped as ``analyze_wav_files`` does (``packed24``
    included); each group is one
    ``Detector.run_host_reports``: hot path, tables, beat stages with one start
    hint per file and the decision trace, final metrics, all on the GPU, and
    ``explain`` + ``reports.write_reports_packed`` on the host.  No
    ``beats.PeakClassifier`` runs.  A file whose metrics met a decisive
    find_peaks tie or an invalid distance has them recomputed on the host
    (``Metrics.to_host``).  ``start_bpm_hints``: one per file (None = none);
    ``original_file_paths`` name the reports (default: ``file_paths``).

    With ``labels=True`` the labeler's output is made on the device as well
    (``Detector.labels_device``: the analysis' final beats as S1 marks, its S2
    marks, the S1-S2 pairs, the groups separated by pauses of
    ``label_gap_sec`` and their statistics): each dict gains ``labels`` and
    ``<base>_labels.csv`` is written as the labeler's ``save_labels`` writes it
    (``labels.write_labels``), so the file opens in the labeler beside the CSV
    and the debug WAV of the same run.  That file is where the labeler keeps
    hand labels: an existing one is left as it is and the dict says
    ``labels_written=False``, unless ``labels_overwrite=True``.  A file without
    reports gets no label file.

    ``start_bpm_hints="auto"``: the tempo stage (``Detector.tempo_device``:
    a BPM per 8 s window from the envelope's autocorrelation) runs on the
    device and the beat stages start from its hint per file, read where it
    lies; ``_Analysis_Settings.json`` records the value used, as it records a
    typed hint.  ``tempo=True``: each dict gains ``tempo`` (the table and the
    record, ``tempo.tempogram``'s dict) and ``tempo_check`` (``tempo.compare``
    of the analysed BPM curve against it: the fractions of strong windows
    where the curve agrees, is at twice or at half the window's BPM; None
    without a strong window), and ``<base>_tempo.csv`` is written beside the
    reports (``tempo.write_csv``).  With neither, the stage does not run and
    every byte written is as before.

    ``hrv_spectrum=True``: the HRV spectrum (``Detector.hrv_spectrum_device``:
    per 120 s window, every 30 s, the Lomb-Scargle periodogram of the RR
    intervals, LF and HF power and the band peaks) runs on the device behind
    the beat stages; each dict gains ``hrv_spectrum``
    (``hrv_spectrum.spectrum``'s dict) and ``<base>_hrv_spectrum.csv`` is
    written beside the reports (``hrv_spectrum.write_csv``).  Left false, the
    stage does not run and every byte written is as before.

    Returns one dict per path, in order: ``run_host_reports``' dict, or
    ``error`` with the exception the reference raises for that file; as there,
    a file with fewer than two final beats gets no reports
    (``final_metrics`` None)."""
    from .plot import write_plot_packed
    from .reports import write_reports_packed
    from . import labels as LB
    from . import tempo as TP
    from . import hrv_spectrum as HS
    if mode is None:
        mode = params.get("bpmx_mode", "reference")
    n = len(file_paths)
    auto = isinstance(start_bpm_hints, str)
    if auto and start_bpm_hints != "auto":
        raise ValueError('start_bpm_hints is one entry per file or "auto"')
    hints = [None] * n if start_bpm_hints is None or auto else list(start_bpm_hints)
    names = list(file_paths) if original_file_paths is None else list(original_file_paths)
    if len(hints) != n or len(names) != n:
        raise ValueError("start_bpm_hints and original_file_paths need one entry per file")
    rect = mode == RECTIFIED
    save = bool(params.get("save_filtered_wav", False))
    if rect and save:
        logging.info(NO_DEBUG_WAV_MSG)
        save = False
    out: List[dict] = [None] * n
    groups: Dict[tuple, List[int]] = {}
    audio = []
    for k, path in enumerate(file_paths):
        try:
            fs, a = _read_wav(path, packed24)
        except Exception as exc:                      # wavfile errors propagate per file, as in the GUI loop
            out[k] = {"error": exc}
            audio.append(None)
            continue
        audio.append((fs, a))
        groups.setdefault((fs, a.dtype.str, 1 if a.ndim == 1 else a.shape[1]), []).append(k)
    det = default_detector(device)
    for (fs, _, _), idx in groups.items():
        try:
            d = mode_design(fs, params, mode, log=True)   # clamp warnings / Nyquist ValueError, once per group
        except ValueError as exc:
            for k in idx:
                out[k] = {"error": exc}
            continue
        try:
            if d.distance < 1:
                raise ValueError(DISTANCE_MSG)
            run_params = dict(params, save_filtered_wav=False) if rect else params
            res = det.run_host_reports([audio[k][1] for k in idx], fs, run_params, mode=mode,
                                       hints="auto" if auto else [hints[k] for k in idx], plot=plot,
                                       **(dict(labels=True, label_gap_sec=label_gap_sec) if labels else {}),
                                       **(dict(tempo=True) if tempo else {}),
                                       **(dict(hrv_spectrum=True) if hrv_spectrum else {}))
        except (ValueError, N.BpmxError) as exc:      # reported per file, as the GUI loop does (gui.py:247-251)
            if isinstance(exc, N.BpmxError) and not exc.per_file:
                raise                                 # HIP / device failure: not a per-file error
            for k in idx:                             # (a too-short file fails first, in filtfilt)
                short = not rect and -(-audio[k][1].shape[0] // d.ds) <= 15
                out[k] = {"error": ValueError(PADLEN_MSG) if short else exc}
            continue
        for k, r in zip(idx, res):
            err = _file_error(r["flags"], params, d.sr)
            if err is not None:
                out[k] = {"error": err}
                continue
            if save:
                _write_debug_wavs(file_paths[k], output_directory, d.sr, r["y16"])
            if "error" in r:                          # < 2 raw peaks (KeyError), scipy's ValueError in the metrics
                out[k] = {"error": r["error"]}
                continue
            if labels:
                r["labels_written"] = False
            if auto:
                hints[k] = r["start_bpm_hint"]
            if tempo:
                r["tempo_check"] = TP.compare(r["tempo"], r.get("bpm_times", ()), r.get("bpm", ()))
            if r["final_metrics"] is not None:
                if plot:
                    r["figure"] = write_plot_packed(names[k], output_directory, params, r)
                write_reports_packed(names[k], output_directory, r, hints[k])
                if tempo:
                    TP.write_csv(TP.tempo_path(names[k], output_directory), r["tempo"], r["tempo_check"])
                if hrv_spectrum:
                    HS.write_csv(HS.spectrum_path(names[k], output_directory), r["hrv_spectrum"])
                if labels and r["labels"] is not None:
                    r["labels_written"] = LB.write_labels(LB.labels_path(names[k], output_directory), r["labels"],
                                                          overwrite=labels_overwrite)
            out[k] = r
    return out


def score_wav_files(file_paths: Sequence[str], params_list: Sequence[Dict], label_paths: Sequence[str] = None,
                    mode: str = None, device: int = 0, tol_sec: float = 0.05, label_gap_sec: float = 5.0,
                    start_bpm_hints: Sequence = None) -> List[dict]:
    """How well each setting of `params_list` reproduces the corrected labels
    of an archive: every file is analysed with every setting on the device
    (``Detector.score_sweep``: the envelope once per file, then detection,
    beat stages, labels and the scoring per setting) and only the integer
    records come back.  With ``mode="rectified"`` the files are the
    ``_filtered_debug.wav`` files of an earlier run, so the original audio is
    not needed.

    ``label_paths``: one corrected ``_labels.csv`` per file (default:
    ``labels.labels_path`` beside the WAV, which is where
    ``analyze_wav_files_to_reports(labels=True)`` writes it and the labeler
    saves it).  A file that cannot be read, or whose label file is missing,
    unreadable or without an S1 / S2 mark, is a per-file ``error`` entry; the
    others still score.  Files are grouped by (rate, format, channels) as
    ``analyze_wav_files`` groups them.  ``start_bpm_hints="auto"``: the tempo
    stage runs once per group on the shared envelope and feeds its hints.

    Returns one dict per setting, in order: ``params``, ``files`` (per path
    ``labels.score_summary``'s dict with ``record`` and ``status``, or
    ``error``) and ``total`` (the summary of the files' records added,
    ``labels.score_total``) with its ``record`` and ``n_files``."""
    from . import labels as LB
    params_list = [dict(p) for p in params_list]
    if mode is None:
        mode = params_list[0].get("bpmx_mode", "reference") if params_list else "reference"
    n = len(file_paths)
    auto = isinstance(start_bpm_hints, str)
    if auto and start_bpm_hints != "auto":
        raise ValueError('start_bpm_hints is one entry per file or "auto"')
    hints = [None] * n if start_bpm_hints is None or auto else list(start_bpm_hints)
    if label_paths is None:
        label_paths = [LB.labels_path(p, os.path.dirname(p)) for p in file_paths]
    if len(hints) != n or len(label_paths) != n:
        raise ValueError("start_bpm_hints and label_paths need one entry per file")
    LB.score_ms(tol_sec, label_gap_sec)
    errors: Dict[int, Exception] = {}
    groups: Dict[tuple, List[int]] = {}
    audio, refs = [None] * n, [None] * n
    for k, path in enumerate(file_paths):
        try:
            if not os.path.exists(label_paths[k]):
                raise FileNotFoundError(f"no label file {label_paths[k]}")
            refs[k] = LB.marks_from_table(LB.read_labels(label_paths[k]))
            if len(refs[k]["ms"]) == 0:
                raise ValueError(f"{label_paths[k]} holds no S1 or S2 mark")
            fs, a = _read_wav(path)
        except Exception as exc:                      # per file, as in the GUI loop
            errors[k] = exc
            continue
        audio[k] = a
        groups.setdefault((fs, a.dtype.str, 1 if a.ndim == 1 else a.shape[1]), []).append(k)
    det = default_detector(device)
    records = np.zeros((len(params_list), n, N.SCORE_RECORD), np.int64)
    status = np.zeros((len(params_list), n), np.int32)
    for (fs, _, _), idx in groups.items():
        try:
            rec, st = det.score_sweep([audio[k] for k in idx], fs, params_list, [refs[k] for k in idx], mode=mode,
                                      hints="auto" if auto else [hints[k] for k in idx], tol_sec=tol_sec,
                                      gap_sec=label_gap_sec)
        except (ValueError, N.BpmxError) as exc:
            if isinstance(exc, N.BpmxError) and not exc.per_file:
                raise                                 # HIP / device failure: not a per-file error
            if len({p["downsample_factor"] for p in params_list}) > 1:
                raise                                 # the caller's grid, not a file
            for k in idx:
                errors[k] = exc
            continue
        records[:, idx], status[:, idx] = rec, st
    good = [k for k in range(n) if k not in errors]
    out = []
    for p, params in enumerate(params_list):
        files = []
        for k in range(n):
            if k in errors:
                files.append({"error": errors[k]})
            else:
                files.append(dict(LB.score_summary(records[p, k]), record=records[p, k].copy(),
                                  status=int(status[p, k])))
        tot = LB.score_total(records[p, good])
        out.append({"params": params, "files": files,
                    "total": dict(LB.score_summary(tot), record=tot, n_files=len(good))})
    return out


def _label_rates(n: int, sample_rates, wav_paths, params: Dict, mode: str) -> List:
    """The decimated rate of every label file: an int for all, one per file,
    or from the headers of `wav_paths` (the rate the analysis of that WAV
    runs at).  An entry that cannot be had is the exception."""
    if wav_paths is not None:
        from scipy.io import wavfile
        if len(wav_paths) != n:
            raise ValueError("wav_paths needs one entry per label file")
        out = []
        for p in wav_paths:
            try:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    fs, _ = wavfile.read(p, mmap=True)
                out.append(int(mode_design(int(fs), params, mode).sr))
            except Exception as exc:                  # per file, as in the GUI loop
                out.append(exc)
        return out
    if sample_rates is None:
        raise ValueError("sample_rates or wav_paths is required")
    if np.ndim(sample_rates) == 0:
        return [int(sample_rates)] * n
    if len(sample_rates) != n:
        raise ValueError("sample_rates needs one entry per label file")
    return [int(r) for r in sample_rates]


def _read_marks(path: str, rate):
    """(marks, None) of a label file, or (None, the exception) where it is missing or unreadable."""
    from . import labels as LB
    try:
        if isinstance(rate, Exception):
            raise rate
        if rate < 1:
            raise ValueError(f"sample rate {rate} of {path}")
        if not os.path.exists(path):
            raise FileNotFoundError(f"no label file {path}")
        return LB.marks_from_table(LB.read_labels(path)), None
    except Exception as exc:
        return None, exc


def revise_from_labels(label_paths: Sequence[str], sample_rates=None, params: Dict = None,
                       output_directory: str = None, gap_sec: float = 5.0, suffix: str = "_corrected",
                       overwrite: bool = False, device: int = 0, wav_paths: Sequence[str] = None,
                       mode: str = None, hrv_spectrum: bool = False) -> List[dict]:
    """The analysis of a person's own marks: every corrected
    ``<base>_labels.csv`` goes through ``Detector.marks_device``,
    ``metrics_device`` and ``labels_device``, so the BPM curve, the HRV table,
    HRR, slopes, inclines and declines, the summary, the ``Average BPM`` column
    and the S1-S2 group statistics follow the corrected beats.  The times are
    restated on the sample grid of the decimated rate (``labels.rows_from_marks``).

    ``sample_rates``: the decimated rate the label times refer to, an int for
    all files or one per file; or ``wav_paths``, from whose headers it is
    worked out as the analysis does (``mode_design`` with `params` and `mode`).
    Files are grouped by rate; a missing or unreadable label file is that
    file's ``error``.

    Returns one dict per file: ``final_peaks``, ``bpm_times``, ``bpm``,
    ``final_metrics`` (as ``Metrics.to_host`` gives it; None with fewer than
    two S1 marks), ``labels``, ``marks_record`` (bpmx_marks_record's counts)
    and ``sr``.  With ``output_directory`` it writes
    ``<base><suffix>_Analysis_Summary.md``, ``<base><suffix>_bpm_plot.csv``
    and ``<base><suffix>_labels.csv`` (``written``: the paths), where <base> is
    the label file's name without ``_labels.csv``; an existing file is left as
    it is unless `overwrite` (``skipped``: those paths).

    ``hrv_spectrum=True``: the HRV spectrum follows the corrected beats
    (``Detector.hrv_spectrum_device`` behind ``marks_device``); a label file
    carries no recording length, so the recording is taken to end one sample
    after its last mark.  Each dict gains ``hrv_spectrum``, and
    ``<base><suffix>_hrv_spectrum.csv`` is written with the others."""
    from . import beats as B
    from . import hrv_spectrum as HS
    from . import labels as LB
    from . import reports as R
    params = dict(DEFAULT_PARAMS if params is None else params)
    if mode is None:
        mode = params.get("bpmx_mode", "reference")
    n = len(label_paths)
    rates = _label_rates(n, sample_rates, wav_paths, params, mode)
    out: List[dict] = [None] * n
    groups: Dict[int, List[int]] = {}
    marks = [None] * n
    for k, path in enumerate(label_paths):
        marks[k], err = _read_marks(path, rates[k])
        if err is not None:
            out[k] = {"error": err}
            continue
        groups.setdefault(rates[k], []).append(k)
    det = default_detector(device)
    torch = __import__("torch")
    for sr, idx in groups.items():
        with det.lock, torch.cuda.stream(det.host_stream()):
            beats = det.marks_device([marks[k] for k in idx], sr, params)
            res = det.metrics_device(beats, params).to_host()
            labs = det.labels_device(beats, gap_sec).to_host()
            if hrv_spectrum:
                ends = [(int(max(marks[k]["ms"], default=-1)) * sr + 500) // 1000 + 1 for k in idx]
                specs = det.hrv_spectrum_device(beats, lengths=ends, params=params).to_host()
            det.host_stream().synchronize()
        for j, (k, r, lab) in enumerate(zip(idx, res, labs)):
            r = dict(r, labels=lab, sr=sr)
            if hrv_spectrum:
                r["hrv_spectrum"] = specs[j]
            out[k] = r
            if output_directory is None:
                continue
            name = os.path.basename(label_paths[k])
            base = (name[:-len("_labels.csv")] if name.endswith("_labels.csv") else os.path.splitext(name)[0]) + suffix
            r["written"], r["skipped"] = [], []
            m = r["final_metrics"]
            if m is None:
                continue
            jobs = ((f"{base}_Analysis_Summary.md", lambda p: _write_text(p, R.summary_text(base, m))),
                    (f"{base}_bpm_plot.csv", lambda p: B.write_bpm_csv(p, m)),
                    (f"{base}_labels.csv", lambda p: lab is not None and LB.write_labels(p, lab, overwrite=True)))
            if hrv_spectrum:
                jobs += ((f"{base}_hrv_spectrum.csv", lambda p: HS.write_csv(p, r["hrv_spectrum"]) is None),)
            for fname, write in jobs:
                p = os.path.join(output_directory, fname)
                if os.path.exists(p) and not overwrite:
                    r["skipped"].append(p)
                elif write(p):
                    r["written"].append(p)
    return out


def _write_text(path: str, text: str) -> bool:
    with open(path, "w", encoding="utf-8") as f:
        f.write(text)
    return True


def score_label_files(label_paths: Sequence[str], ref_label_paths: Sequence[str], sample_rates=None,
                      tol_sec: float = 0.05, gap_sec: float = 5.0, device: int = 0,
                      params: Dict = None) -> List[dict]:
    """One person's labels scored against another's (inter-rater agreement):
    the files of `label_paths` go through ``Detector.marks_device`` and
    ``labels_device``, which restates them as the analysis' own label rows,
    the files of `ref_label_paths` through ``upload_marks``, both into the
    unchanged ``score_device``.  ``sample_rates``: the decimated rate, an int
    or one per pair.  Returns per pair ``labels.score_summary``'s dict with
    ``record`` and ``status``, or ``error`` where either file is missing or
    unreadable."""
    from . import labels as LB
    params = dict(DEFAULT_PARAMS if params is None else params)
    n = len(label_paths)
    if len(ref_label_paths) != n:
        raise ValueError("ref_label_paths needs one entry per label file")
    LB.score_ms(tol_sec, gap_sec)
    rates = _label_rates(n, sample_rates, None, params, "reference")
    out: List[dict] = [None] * n
    groups: Dict[int, List[int]] = {}
    marks, refs = [None] * n, [None] * n
    for k in range(n):
        marks[k], err = _read_marks(label_paths[k], rates[k])
        if err is None:
            refs[k], err = _read_marks(ref_label_paths[k], rates[k])
        if err is not None:
            out[k] = {"error": err}
            continue
        groups.setdefault(rates[k], []).append(k)
    det = default_detector(device)
    torch = __import__("torch")
    for sr, idx in groups.items():
        with det.lock, torch.cuda.stream(det.host_stream()):
            labs = det.labels_device(det.marks_device([marks[k] for k in idx], sr, params), gap_sec)
            sc = det.score_device(labs, det.upload_marks([refs[k] for k in idx]), tol_sec, gap_sec, rows=False)
            rec, st = sc.download()
            det.host_stream().synchronize()
        for j, k in enumerate(idx):
            out[k] = dict(LB.score_summary(rec[j]), record=rec[j].copy(), status=int(st[j]))
    return out


def patch_reference(module) -> None:
    """Rebind an imported reference ``bpm_analysis`` module's hot path to the GPU.

    After ``patch_reference(bpm_analysis)``, the reference's own
    ``analyze_wav_file`` (and gui.py / main.py / app.py on top of it) runs
    preprocess_audio, _calculate_dynamic_noise_floor and
    PeakClassifier._find_raw_peaks through libbpmx.so.
    """
    module.preprocess_audio = preprocess_audio
    module._calculate_dynamic_noise_floor = _calculate_dynamic_noise_floor

    def _find_raw_peaks(self, height_threshold):
        return find_raw_peaks(self.audio_envelope, self.sample_rate, self.params, height_threshold)

    module.PeakClassifier._find_raw_peaks = _find_raw_peaks
