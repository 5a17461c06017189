"""Batch engine: device buffers (torch), the C-ABI call, per-file results.

PyTorch is used here only as plumbing — device memory, streams and copies.
All arithmetic runs in libbpmx.so's HIP kernels.

A batch is a set of recordings with one sample rate, sample format and
channel count (the reference processes one WAV at a time: gui.py:202-251; a
batch is the MI355X unit of work).  Lengths may be ragged.  Recordings are
laid out back to back in HBM; results use the decimated offsets
``doff[f] = sum(Nd[:f])``.
"""
from __future__ import annotations

import ctypes
import threading
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import _native as N
from .design import Design, design, detect_design, dtype_code, make_params

MODES = {"reference": N.MODE_REFERENCE, "native": N.MODE_NATIVE, "rectified": N.MODE_RECTIFIED}


def mode_design(fs: int, params: dict, mode: str = "reference", log: bool = False) -> Design:
    """The host derivations a run in `mode` needs.  Rectified mode takes the
    samples as they are (heartbeat_labeler.py:53-67): ``detect_design`` at
    `fs`, so ds 1, sr fs, no filter design, no Nyquist check and no clamp
    warnings; the other modes ``design``."""
    if mode == "rectified":
        return detect_design(fs, params)
    return design(fs, params, log=log)


def _no_filtered_signal(mode: str, wanted: bool) -> None:
    if wanted and mode == "rectified":
        raise N.BpmxArgError("rectified mode has no filtered signal: y / y16 cannot be requested", N.E_ARG)


def _torch():
    import torch
    return torch


_TORCH_DT = None


def _flatten_batch(recordings):
    """A host batch as one flat array -> (host, frame offsets, channels,
    sample_format).  Recordings are numpy arrays (frames,) / (frames, channels)
    or ``pcm24.Pcm24``; a batch is one sample format and channel count."""
    from .pcm24 import Pcm24
    packed = isinstance(recordings[0], Pcm24)
    dt = recordings[0].dtype
    ch = 1 if recordings[0].ndim == 1 else recordings[0].shape[1]
    for r in recordings:
        if isinstance(r, Pcm24) != packed or (not packed and r.dtype != dt) or \
                (1 if r.ndim == 1 else r.shape[1]) != ch:
            raise ValueError("a batch needs one sample format and channel count")
    fo = np.zeros(len(recordings) + 1, dtype=np.int64)
    fo[1:] = np.cumsum([r.shape[0] for r in recordings])
    if packed:
        return np.concatenate([r.data for r in recordings]), fo, ch, "i24"
    return np.concatenate([np.ascontiguousarray(r).reshape(-1) for r in recordings]), fo, ch, None


def torch_dtype(np_dtype):
    global _TORCH_DT
    torch = _torch()
    if _TORCH_DT is None:
        _TORCH_DT = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int16): torch.int16,
                     np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32,
                     np.dtype(np.float64): torch.float64}
    return _TORCH_DT[np.dtype(np_dtype)]


@dataclass
class Result:
    """Device-resident outputs of one batch (torch tensors on the GPU)."""
    sr: int
    ds: int
    frame_offsets: np.ndarray      # host int64 [F+1]
    doff: np.ndarray               # host int64 [F+1] decimated offsets
    env: "object"
    floor: "object"
    y: "object"
    troughs: "object"
    peaks: "object"
    n_troughs: "object"
    n_peaks: "object"
    n_raw_troughs: "object"
    flags: "object"

    @property
    def n_files(self) -> int:
        return len(self.doff) - 1

    def to_host(self) -> List[dict]:
        """Per-file numpy views after one D2H copy of each array."""
        env = self.env.cpu().numpy()
        floor = self.floor.cpu().numpy() if self.floor is not None else None
        y = self.y.cpu().numpy() if self.y is not None else None
        tr = self.troughs.cpu().numpy() if self.troughs is not None else None
        pk = self.peaks.cpu().numpy() if self.peaks is not None else None
        ntr = self.n_troughs.cpu().numpy()
        npk = self.n_peaks.cpu().numpy()
        nraw = self.n_raw_troughs.cpu().numpy()
        flags = self.flags.cpu().numpy()
        out = []
        for f in range(self.n_files):
            a, b = int(self.doff[f]), int(self.doff[f + 1])
            if flags[f] & N.F_TOO_SHORT:
                b = a           # no outputs (include/bpmx.h): empty slices, not the buffers' old contents
            out.append(dict(
                sr=self.sr, env=env[a:b], floor=None if floor is None else floor[a:b],
                y=None if y is None else y[a:b],
                troughs=None if tr is None else tr[a:a + int(ntr[f])].copy(),
                peaks=None if pk is None else pk[a:a + int(npk[f])].copy(),
                n_raw_troughs=int(nraw[f]), flags=int(flags[f])))
        return out


def peak_capacity(nd: int, distance: int) -> int:
    """Most peaks ``find_peaks(distance=d)`` can keep in ``nd`` samples: kept
    peaks are pairwise at least ``distance`` apart (and sanitised troughs are a
    subset of such a set), so (nd - 1) // distance + 1.  Summed over a batch it
    sizes the packed tables with no device round trip."""
    nd, distance = int(nd), max(int(distance), 1)
    return (nd - 1) // distance + 1 if nd >= 1 else 0


@dataclass
class Packed:
    """bpmx_pack's outputs for one batch (device tensors): the raw peaks and
    troughs of every recording as two ragged tables (index, envelope and floor
    at that index; recording f's entries are ``[off[f], off[f + 1])``), the
    per-file counters of the run, and optionally the debug WAV's int16
    samples.  What ``to_host`` downloads is a few MB where ``Result.to_host``
    moves four sum(Nd)-long 8-byte arrays."""
    det: "object"
    sr: int
    doff: np.ndarray               # host int64 [F+1] decimated offsets
    cap_peaks: int
    cap_troughs: int
    safe_peaks: int                # sum of peak_capacity over the files: a run's totals never exceed it
    safe_troughs: int
    pk_off: "object"
    tr_off: "object"
    pk_idx: "object"
    pk_env: "object"
    pk_floor: "object"
    tr_idx: "object"
    tr_env: "object"
    y16: "object"
    y_max: "object"
    n_raw_troughs: "object" = None
    flags: "object" = None
    tr_floor: "object" = None      # the floor at the troughs (pack(want_tr_floor=True)), like tr_env

    @property
    def n_files(self) -> int:
        return len(self.doff) - 1

    def _check(self, tp: int, tt: int) -> None:
        if tp > self.cap_peaks or tt > self.cap_troughs:
            raise N.BpmxError(f"packed tables too small: {tp} peaks (capacity {self.cap_peaks}), "
                              f"{tt} troughs (capacity {self.cap_troughs})", N.E_LIMIT)

    def to_host(self) -> List[dict]:
        """Per-file dicts: sr, n_env, peaks, env_pk, floor_pk, troughs, env_tr,
        n_raw_troughs, flags (and y16, y_max, floor_tr when packed).  Two rounds of
        asynchronous copies into pinned staging on the current stream, each
        ended by one stream synchronise: the per-file offsets and counters
        first, then the used prefix of each table (and y16), whose length
        only the offsets tell.  Raises BpmxError (E_LIMIT) when a table's
        total exceeds its capacity."""
        torch = _torch()
        det, F = self.det, self.n_files
        with det.lock:
            st = torch.cuda.current_stream(det.device)
            small = {"pk_off": self.pk_off, "tr_off": self.tr_off, "flags": self.flags,
                     "n_raw_troughs": self.n_raw_troughs, "y_max": self.y_max}
            pin = {k: det.staging(k, t.numel(), t.dtype) for k, t in small.items() if t is not None}
            for k, h in pin.items():
                h.copy_(small[k], non_blocking=True)
            st.synchronize()
            meta = {k: h.numpy().copy() for k, h in pin.items()}
            pko, tro = meta["pk_off"], meta["tr_off"]
            tp, tt, tot = int(pko[F]), int(tro[F]), int(self.doff[F])
            self._check(tp, tt)
            big = {"pk_idx": (self.pk_idx, tp), "pk_env": (self.pk_env, tp), "pk_floor": (self.pk_floor, tp),
                   "tr_idx": (self.tr_idx, tt), "tr_env": (self.tr_env, tt)}
            if self.y16 is not None:
                big["y16"] = (self.y16, tot)
            if self.tr_floor is not None:
                big["tr_floor"] = (self.tr_floor, tt)
            pin = {k: det.staging(k, n, t.dtype) for k, (t, n) in big.items() if n > 0}
            for k, h in pin.items():
                h.copy_(big[k][0][:big[k][1]], non_blocking=True)
            st.synchronize()
            tab = {k: (pin[k].numpy().copy() if k in pin else np.zeros(0, _NP_OF[str(t.dtype)]))
                   for k, (t, n) in big.items()}
        flags = meta["flags"] if "flags" in meta else np.zeros(F, np.int32)
        nraw = meta["n_raw_troughs"] if "n_raw_troughs" in meta else np.zeros(F, np.int32)
        pki, tri = tab["pk_idx"].astype(np.int64), tab["tr_idx"].astype(np.int64)
        out = []
        for f in range(F):
            a, b = int(self.doff[f]), int(self.doff[f + 1])
            p0, p1, t0, t1 = int(pko[f]), int(pko[f + 1]), int(tro[f]), int(tro[f + 1])
            if flags[f] & N.F_TOO_SHORT:
                b, p1, t1 = a, p0, t0           # no outputs (include/bpmx.h): empty slices
            r = dict(sr=self.sr, n_env=b - a, peaks=pki[p0:p1], env_pk=tab["pk_env"][p0:p1],
                     floor_pk=tab["pk_floor"][p0:p1], troughs=tri[t0:t1], env_tr=tab["tr_env"][t0:t1],
                     n_raw_troughs=int(nraw[f]), flags=int(flags[f]))
            if self.y16 is not None:
                r["y16"], r["y_max"] = tab["y16"][a:b], float(meta["y_max"][f])
            if self.tr_floor is not None:
                r["floor_tr"] = tab["tr_floor"][t0:t1]
            out.append(r)
        return out


_NP_OF = {"torch.int8": np.int8, "torch.int16": np.int16, "torch.int32": np.int32, "torch.int64": np.int64,
          "torch.float64": np.float64}


def plot_device_factor(factor) -> int:
    """The int32 factor bpmx_pack_plot takes for a ``plot_downsample_factor``
    as the reference's parameters hold it.  The reference strides by it only
    when ``factor > 1 and len(env) >= factor`` and fails in the slice when it
    is then not an integer, so whatever is not an integer above 1 keeps whole
    series (factor 1) for ``plot.build_figure`` to accept or refuse as it does
    dense arrays; an integer beyond int32 exceeds every recording."""
    if isinstance(factor, (int, np.integer)) and factor > 1:
        return int(min(int(factor), 2 ** 31 - 1))
    return 1


@dataclass
class PlotSeries:
    """The plot's two line traces for one batch (device tensors): per
    recording ``env[::kf]`` and ``floor[::kf]``, ragged, recording f's entries
    at ``[off[f], off[f + 1])``; `kf` and `off` are host arrays (the lengths
    follow from the decimated lengths and the factor alone).  When every kf
    is 1, `env` and `floor` are the Result's own tensors and `off` its
    decimated offsets: nothing was launched or copied on the device."""
    det: "object"
    factor: int
    kf: np.ndarray                 # host int64 [F]
    off: np.ndarray                # host int64 [F+1]
    env: "object"
    floor: "object"                # None without want_floor

    @property
    def n_files(self) -> int:
        return len(self.off) - 1

    def to_host(self) -> List[dict]:
        """Per-file dicts: ``env_plot``, ``floor_plot`` (None without the
        floor) and ``plot_factor`` (the kf used).  Asynchronous copies of the
        used prefixes into pinned staging on the current stream, one wait."""
        torch = _torch()
        det, F, tot = self.det, self.n_files, int(self.off[-1])
        with det.lock:
            st = torch.cuda.current_stream(det.device)
            src = {"pl_env": self.env, "pl_floor": self.floor}
            pin = {k: det.staging(k, tot, t.dtype) for k, t in src.items() if t is not None and tot > 0}
            for k, h in pin.items():
                h.copy_(src[k][:tot], non_blocking=True)
            st.synchronize()
            tab = {k: h.numpy().copy() for k, h in pin.items()}
        env = tab.get("pl_env", np.zeros(0))
        flo = tab.get("pl_floor", np.zeros(0)) if self.floor is not None else None
        out = []
        for f in range(F):
            a, b = int(self.off[f]), int(self.off[f + 1])
            out.append(dict(env_plot=env[a:b], floor_plot=None if flo is None else flo[a:b],
                            plot_factor=int(self.kf[f])))
        return out


@dataclass
class Trace:
    """bpmx_trace_out for one batch (device tensors): the decision trace of
    ``beats_device(trace=True)``, in slices at ``packed.pk_off[f]`` (record:
    N.TR_NFIELDS doubles per raw peak).  ``explain.assemble`` turns a
    recording's slices into the reference's ``analysis_data``."""
    record: "object"
    code: "object"
    lt_pos: "object"
    lt_bpm: "object"
    n_lt: "object"
    dev_t: "object"
    dev: "object"
    gap: "object"


_TRACE_ROWS = ("record", "code", "lt_pos", "lt_bpm", "dev_t", "dev", "gap")


@dataclass
class Beats:
    """bpmx_beats_device's outputs for one batch (device tensors): per
    recording the final beats, the smoothed BPM curve, the preliminary pass'
    values, one label per raw peak and a status, in slices that start at
    ``packed.pk_off[f]`` like the peak table's."""
    det: "object"
    packed: Packed
    final_idx: "object"
    n_final: "object"
    bpm_t: "object"
    bpm: "object"
    n_bpm: "object"
    pass_: "object"
    tags: "object"
    status: "object"
    trace: Optional[Trace] = None  # beats_device(trace=True)
    params: Optional[dict] = None  # the parameter dict of the launch (the trace's strings quote thresholds)
    hints: "object" = None         # device [F] per-file hints the launch reads (kept alive with its results)
    marks: "object" = None         # marks_device: the Marks the launch read
    marks_record: "object" = None  # marks_device: device [F * N.MARKS_RECORD] int32, the counts per recording

    def to_host(self, explain: bool = False) -> List[dict]:
        """Per-file dicts as ``_host.beats`` returns them (final_peaks,
        bpm_times, bpm, start_bpm, peak_time, recovery_time, tags, or
        ``error=KeyError(...)`` for < 2 raw peaks) plus ``raw_peaks`` and
        ``flags``; a recording the stage skipped (too short, bad window) gives
        ``skipped=True`` with its flags.  Two rounds of copies like
        ``Packed.to_host``: offsets, counts, status and pass values first, then
        the used prefix of each array.  Raises BpmxError (E_LIMIT) when the
        peak table was too small.  A result of ``marks_device`` gives the same
        dicts (``start_bpm`` NaN, no peak and recovery time) plus ``marks_record``,
        the counts of bpmx_marks_record; a recording with fewer than two S1
        marks (BPMX_MARKS_FEW) has empty ``final_peaks`` and curve.

        ``explain`` (needs ``beats_device(trace=True)`` with the parameter
        dict): the trace comes down in the same two rounds and every
        recording with beats gets ``analysis_data`` (``explain.assemble``: the
        reference's debug strings, belief curve and deviation series) and
        ``trace`` (its slices of the trace, as ``explain.assemble`` takes them)."""
        from . import _host
        torch = _torch()
        det, pk = self.det, self.packed
        F = pk.n_files
        if explain and (self.trace is None or self.params is None):
            raise N.BpmxError("explain needs beats_device(trace=True) with the parameter dict", N.E_ARG)
        with det.lock:
            st = torch.cuda.current_stream(det.device)
            small = {"pk_off": pk.pk_off, "flags": pk.flags, "b_n_final": self.n_final, "b_n_bpm": self.n_bpm,
                     "b_status": self.status, "b_pass": self.pass_, "b_marks": self.marks_record}
            if explain:
                small["t_n_lt"] = self.trace.n_lt
            pin = {k: det.staging(k, t.numel(), t.dtype) for k, t in small.items() if t is not None}
            for k, h in pin.items():
                h.copy_(small[k].reshape(-1), non_blocking=True)
            st.synchronize()
            meta = {k: h.numpy().copy() for k, h in pin.items()}
            pko = meta["pk_off"]
            tp = int(pko[F])
            if tp > pk.cap_peaks or np.isin(meta["b_status"], (N.BEATS_OVERFLOW, N.MARKS_OVERFLOW)).any():
                raise N.BpmxError(f"packed tables too small: {tp} peaks (capacity {pk.cap_peaks})", N.E_LIMIT)
            big = {"pk_idx": pk.pk_idx, "b_final": self.final_idx, "b_bpm_t": self.bpm_t, "b_bpm": self.bpm,
                   "b_tags": self.tags}
            per = {k: 1 for k in big}
            if explain:
                big.update({"t_" + k: getattr(self.trace, k) for k in _TRACE_ROWS})
                per.update({"t_" + k: (N.TR_NFIELDS if k == "record" else 1) for k in _TRACE_ROWS})
            pin = {k: det.staging(k, tp * per[k], t.dtype) for k, t in big.items() if tp > 0}
            for k, h in pin.items():
                h.copy_(big[k][:tp * per[k]], non_blocking=True)
            st.synchronize()
            tab = {k: (pin[k].numpy().copy() if k in pin else np.zeros(0, _NP_OF[str(t.dtype)]))
                   for k, t in big.items()}
        flags = meta["flags"] if "flags" in meta else np.zeros(F, np.int32)
        pas = meta["b_pass"].reshape(F, 3)
        raw, fin = tab["pk_idx"].astype(np.int64), tab["b_final"].astype(np.int64)
        nan2none = lambda x: None if x != x else float(x)  # noqa: E731
        out = []
        for f in range(F):
            a, s = int(pko[f]), int(meta["b_status"][f])
            n, nf, nb = int(pko[f + 1]) - a, int(meta["b_n_final"][f]), int(meta["b_n_bpm"][f])
            if s == N.BEATS_SKIPPED:
                out.append({"skipped": True, "raw_peaks": np.zeros(0, np.int64), "flags": int(flags[f])})
                continue
            r = {"raw_peaks": raw[a:a + n], "flags": int(flags[f])}
            if s == _host.E_FEW_PEAKS:
                r["error"] = KeyError("dynamic_noise_floor_series")
            elif s != _host.OK and s != N.MARKS_FEW:
                raise N.BpmxError(f"bpmx_beats_device: status {s} for recording {f}")
            else:
                r.update(final_peaks=fin[a:a + nf], bpm_times=tab["b_bpm_t"][a:a + nb], bpm=tab["b_bpm"][a:a + nb],
                         start_bpm=float(pas[f, 0]), peak_time=nan2none(pas[f, 1]),
                         recovery_time=nan2none(pas[f, 2]), tags=tab["b_tags"][a:a + n])
                if explain:
                    from . import explain as X
                    nl = int(meta["t_n_lt"][f])
                    tr = dict(record=tab["t_record"][a * N.TR_NFIELDS:(a + n) * N.TR_NFIELDS], code=tab["t_code"][a:a + n],
                              gap=tab["t_gap"][a:a + n], lt_pos=tab["t_lt_pos"][a:a + nl],
                              lt_bpm=tab["t_lt_bpm"][a:a + nl], dev_t=tab["t_dev_t"][a:a + n - 1],
                              dev=tab["t_dev"][a:a + n - 1])
                    r["trace"] = tr
                    r["analysis_data"] = X.assemble(r["raw_peaks"], int(pk.sr), self.params, tr)
            if "b_marks" in meta:
                r["marks_record"] = meta["b_marks"][f * N.MARKS_RECORD:(f + 1) * N.MARKS_RECORD]
            out.append(r)
        return out


_METRIC_ROWS = ("hrv_time", "hrv_rmssdc", "hrv_sdnn", "hrv_bpm", "inc_a", "inc_b", "dec_a", "dec_b",
                "inc_slope", "inc_dur", "dec_slope", "dec_dur")


@dataclass
class Metrics:
    """bpmx_metrics_device's outputs for one batch (device tensors): per
    recording the windowed HRV rows, the major inclines and declines as curve
    positions in report order, the 16-double record (summary, HRR, steepest
    recovery and exertion; NaN = absent) and a status, in slices that start
    at ``packed.pk_off[f]``."""
    det: "object"
    beats: Beats
    params: dict
    epoch_us: int
    hrv_time: "object"
    hrv_rmssdc: "object"
    hrv_sdnn: "object"
    hrv_bpm: "object"
    n_hrv: "object"
    inc_a: "object"
    inc_b: "object"
    dec_a: "object"
    dec_b: "object"
    inc_slope: "object"
    inc_dur: "object"
    dec_slope: "object"
    dec_dur: "object"
    n_inc: "object"
    n_dec: "object"
    record: "object"
    status: "object"

    def download(self, rows: bool = True):
        """(meta, tab): the per-file counts, status and records, then (with
        `rows`) the used prefix of each per-peak array, in two rounds of pinned
        copies."""
        torch = _torch()
        det, pk = self.det, self.beats.packed
        F = pk.n_files
        with det.lock:
            st = torch.cuda.current_stream(det.device)
            small = {"pk_off": pk.pk_off, "m_n_hrv": self.n_hrv, "m_n_inc": self.n_inc, "m_n_dec": self.n_dec,
                     "m_status": self.status, "m_record": self.record}
            pin = {k: det.staging(k, t.numel(), t.dtype) for k, t in small.items()}
            for k, h in pin.items():
                h.copy_(small[k].reshape(-1), non_blocking=True)
            st.synchronize()
            meta = {k: h.numpy().copy() for k, h in pin.items()}
            tp = int(meta["pk_off"][F])
            if tp > pk.cap_peaks or (meta["m_status"] == N.METRICS_OVERFLOW).any():
                raise N.BpmxError(f"packed tables too small: {tp} peaks (capacity {pk.cap_peaks})", N.E_LIMIT)
            big = {"m_" + k: getattr(self, k) for k in _METRIC_ROWS} if rows else {}
            pin = {k: det.staging(k, tp, t.dtype) for k, t in big.items() if tp > 0}
            for k, h in pin.items():
                h.copy_(big[k][:tp], non_blocking=True)
            st.synchronize()
            tab = {k[2:]: (pin[k].numpy().copy() if k in pin else np.zeros(0, _NP_OF[str(t.dtype)]))
                   for k, t in big.items()}
        meta["m_record"] = meta["m_record"].reshape(F, N.METRICS_RECORD)
        return meta, tab

    def to_host(self, assemble: bool = True, explain: bool = False) -> List[dict]:
        """``Beats.to_host(explain)``'s per-file dicts plus ``final_metrics`` (the dict
        ``beats.final_metrics`` returns, assembled from the device's positions
        and values; None where the reference makes none: fewer than two final
        beats, an error, a skipped recording) and ``metrics_source``.  A
        recording whose find_peaks met a decisive tie or an invalid distance
        is recomputed by ``beats.final_metrics`` on the host (numpy's order,
        scipy's ValueError as ``error``): ``metrics_source`` is then "host",
        else "device".  ``beats._epoch()`` must be what it was at the launch.
        ``assemble=False`` leaves the pandas objects out: instead of
        ``final_metrics`` each dict gets ``metrics_record`` (the 16 doubles of
        bpmx_metrics_out) and ``n_hrv``, which is all ``run_sharded`` gathers."""
        from . import beats as B
        from . import metrics as MH
        out = self.beats.to_host(explain=explain)
        meta, tab = self.download(rows=assemble)
        pko, sr = meta["pk_off"], int(self.beats.packed.sr)
        for f, r in enumerate(out):
            s, a = int(meta["m_status"][f]), int(pko[f])
            r["metrics_source"] = "device"
            if s < 0 and s != N.METRICS_NONE:
                raise N.BpmxError(f"bpmx_metrics_device: status {s} for recording {f}")
            if s > 0:                                  # TIE or E_DISTANCE: numpy's order, scipy's exception
                r["metrics_source"] = "host"
                try:
                    m = B.final_metrics(r["final_peaks"], sr, self.params)
                except ValueError as e:
                    m, r["error"] = None, e
                if assemble:
                    r["final_metrics"] = m
                else:
                    r["metrics_record"], r["n_hrv"] = MH.record_of(m)
            elif not assemble:
                r["metrics_record"], r["n_hrv"] = meta["m_record"][f].copy(), int(meta["m_n_hrv"][f])
            elif s == N.METRICS_NONE:
                r["final_metrics"] = None
            else:
                nh, ni, nd = int(meta["m_n_hrv"][f]), int(meta["m_n_inc"][f]), int(meta["m_n_dec"][f])
                hrv = {c: tab["hrv_" + c][a:a + nh] for c in MH.HRV_COLS}
                inc = {c: tab["inc_" + c][a:a + ni] for c in ("a", "b", "slope", "dur")}
                dec = {c: tab["dec_" + c][a:a + nd] for c in ("a", "b", "slope", "dur")}
                r["final_metrics"] = MH.assemble(r["bpm_times"], r["bpm"], meta["m_record"][f], hrv, inc, dec)
        return out


_LABEL_ROWS = ("lb_pos", "lb_type", "lb_time", "lb_bpm", "pr_s1", "pr_s2", "pr_dt", "gr_id", "gr_first", "gr_last",
               "gr_s1", "gr_pairs", "gr_dt", "gr_bpm")
_LABEL_COUNT = {"lb": "n_labels", "pr": "n_pairs", "gr": "n_groups"}


@dataclass
class Labels:
    """bpmx_labels_device's outputs for one batch (device tensors): per
    recording the S1 / S2 label rows, the S1-S2 pairs, the groups that have
    statistics, the three counts, the 4-double record (mean interval and BPM
    over all pairs, labels of each type) and a status, in slices that start at
    ``packed.pk_off[f]``."""
    det: "object"
    beats: Beats
    gap_sec: float
    lb_pos: "object"
    lb_type: "object"
    lb_time: "object"
    lb_bpm: "object"
    pr_s1: "object"
    pr_s2: "object"
    pr_dt: "object"
    gr_id: "object"
    gr_first: "object"
    gr_last: "object"
    gr_s1: "object"
    gr_pairs: "object"
    gr_dt: "object"
    gr_bpm: "object"
    n_labels: "object"
    n_pairs: "object"
    n_groups: "object"
    record: "object"
    status: "object"

    def to_host(self) -> List[Optional[dict]]:
        """Per recording the labels dict of ``labels.assemble`` (table, pairs,
        groups, summary, gap_sec), or None where the stage made no labels
        (BPMX_LABELS_NONE).  Two rounds of pinned copies like the other
        results: offsets, counts, status and records first, then the used
        prefix of each array.  Raises BpmxError (E_LIMIT) when the peak table
        was too small."""
        from . import labels as LB
        torch = _torch()
        det, pk = self.det, self.beats.packed
        F = pk.n_files
        with det.lock:
            st = torch.cuda.current_stream(det.device)
            small = {"pk_off": pk.pk_off, "l_n_labels": self.n_labels, "l_n_pairs": self.n_pairs,
                     "l_n_groups": self.n_groups, "l_status": self.status, "l_record": self.record}
            pin = {k: det.staging(k, t.numel(), t.dtype) for k, t in small.items()}
            for k, h in pin.items():
                h.copy_(small[k].reshape(-1), non_blocking=True)
            st.synchronize()
            meta = {k: h.numpy().copy() for k, h in pin.items()}
            pko = meta["pk_off"]
            tp = int(pko[F])
            if tp > pk.cap_peaks or (meta["l_status"] == N.LABELS_OVERFLOW).any():
                raise N.BpmxError(f"packed tables too small: {tp} peaks (capacity {pk.cap_peaks})", N.E_LIMIT)
            # the used prefix of each kind of row: up to the last entry any file wrote
            cnt = {c: meta["l_" + name] for c, name in _LABEL_COUNT.items()}
            top = {c: int(max((int(pko[f]) + int(v[f]) for f in range(F) if v[f] > 0), default=0))
                   for c, v in cnt.items()}
            big = {"l_" + k: getattr(self, k) for k in _LABEL_ROWS}
            pin = {k: det.staging(k, top[k[2:4]], t.dtype) for k, t in big.items() if top[k[2:4]] > 0}
            for k, h in pin.items():
                h.copy_(big[k][:top[k[2:4]]], non_blocking=True)
            st.synchronize()
            tab = {k[2:]: (pin[k].numpy().copy() if k in pin else np.zeros(0, _NP_OF[str(t.dtype)]))
                   for k, t in big.items()}
        rec = meta["l_record"].reshape(F, N.LABELS_RECORD)
        out: List[Optional[dict]] = []
        for f in range(F):
            s, a = int(meta["l_status"][f]), int(pko[f])
            if s == N.LABELS_NONE:
                out.append(None)
                continue
            if s != N.LABELS_OK:
                raise N.BpmxError(f"bpmx_labels_device: status {s} for recording {f}")
            dev = {k: tab[k][a:a + int(cnt[k[:2]][f])] for k in _LABEL_ROWS}
            dev["record"] = rec[f]
            out.append(LB.assemble(dev, self.gap_sec))
        return out


@dataclass
class Marks:
    """A person's corrected marks of one batch on the device
    (``Detector.upload_marks``): the ragged table bpmx_ref_marks takes, with
    the host's copy (``labels.marks_from_table`` per recording)."""
    det: "object"
    host: List[dict]
    off: np.ndarray              # [F + 1] int64
    rf_off: "object"
    rf_ms: "object"
    rf_type: "object"

    @property
    def n_files(self) -> int:
        return len(self.host)

    @property
    def cap_ref(self) -> int:
        return int(self.off[-1])


@dataclass
class Scores:
    """bpmx_score_device's outputs for one batch (device tensors): per
    recording the 20-int64 record and a status and, with rows, the kind and
    partner of every label row (slices at ``pk_off[f]``) and of every
    reference mark (slices at ``marks.off[f]``)."""
    det: "object"
    labels: Labels
    marks: Marks
    tol_ms: int
    gap_ms: int
    record: "object"
    status: "object"
    sc_kind: "object" = None
    sc_ref: "object" = None
    rf_kind: "object" = None
    rf_det: "object" = None

    def download(self):
        """(record [F, 20] int64, status [F] int32) on the host: the one
        small copy a settings sweep needs.  Raises BpmxError (E_LIMIT) where a
        table was too small."""
        torch = _torch()
        det, F = self.det, self.marks.n_files
        with det.lock:
            st = torch.cuda.current_stream(det.device)
            hr = det.staging("s_record", F * N.SCORE_RECORD, self.record.dtype)
            hs = det.staging("s_status", F, self.status.dtype)
            hr[:F * N.SCORE_RECORD].copy_(self.record.reshape(-1), non_blocking=True)
            hs[:F].copy_(self.status, non_blocking=True)
            st.synchronize()
            rec = hr[:F * N.SCORE_RECORD].numpy().copy().reshape(F, N.SCORE_RECORD)
            status = hs[:F].numpy().copy()
        if (status == N.SCORE_OVERFLOW).any():
            raise N.BpmxError("bpmx_score_device: a label or reference table was too small", N.E_LIMIT)
        return rec, status

    def to_host(self) -> List[dict]:
        """Per recording the dict of ``labels.score``: ``record``, ``status``,
        ``marks`` and, with rows, ``sc_kind``, ``sc_ref``, ``rf_kind``,
        ``rf_det`` (empty where the status is BPMX_SCORE_NONE)."""
        torch = _torch()
        rec, status = self.download()
        F = self.marks.n_files
        rows = None
        if self.sc_kind is not None:
            det, pk = self.det, self.labels.beats.packed
            with det.lock:
                t = {"pk_off": pk.pk_off, "n_labels": self.labels.n_labels, "l_status": self.labels.status,
                     "sc_kind": self.sc_kind, "sc_ref": self.sc_ref, "rf_kind": self.rf_kind, "rf_det": self.rf_det}
                rows = {k: v.cpu().numpy() for k, v in t.items()}     # .cpu() waits for the current stream
                torch.cuda.current_stream(det.device).synchronize()
        out = []
        e32 = np.zeros(0, np.int32)
        for f in range(F):
            r = {"record": rec[f], "status": int(status[f]), "marks": self.marks.host[f], "tol_ms": self.tol_ms,
                 "gap_ms": self.gap_ms}
            if rows is not None:
                if status[f] < 0:
                    r.update(sc_kind=e32, sc_ref=e32, rf_kind=e32, rf_det=e32)
                else:
                    a, ra, rz = int(rows["pk_off"][f]), int(self.marks.off[f]), int(self.marks.off[f + 1])
                    n = int(rows["n_labels"][f]) if rows["l_status"][f] == N.LABELS_OK else 0
                    r.update(sc_kind=rows["sc_kind"][a:a + n], sc_ref=rows["sc_ref"][a:a + n],
                             rf_kind=rows["rf_kind"][ra:rz], rf_det=rows["rf_det"][ra:rz])
            out.append(r)
        return out


@dataclass
class Tempo:
    """bpmx_tempo_device's outputs for one batch (device tensors): per window
    the lag, its strength and BPM (recording f's windows are
    ``[woff[f], woff[f + 1])``), per recording the record.  ``hint`` is what
    ``Detector.beats_device(hints=tempo)`` hands to the beat stages where it
    lies."""
    det: "object"
    sr: int
    win: int
    hop: int
    kmin: int
    kmax: int
    min_strength: float
    start_windows: int
    woff: np.ndarray             # [F + 1] int64, host
    lag: "object"
    rho: "object"
    bpm: "object"
    n_valid: "object"
    n_strong: "object"
    median_bpm: "object"
    mean_rho: "object"
    hint: "object"

    @property
    def n_files(self) -> int:
        return len(self.woff) - 1

    def to_host(self) -> List[dict]:
        """Per recording the dict of ``tempo.tempogram``: ``time`` (the window
        centres), ``lag``, ``rho``, ``bpm`` and the record."""
        torch = _torch()
        det = self.det
        with det.lock:
            t = {k: getattr(self, k).cpu().numpy() for k in ("lag", "rho", "bpm", "n_valid", "n_strong",
                                                             "median_bpm", "mean_rho", "hint")}
            torch.cuda.current_stream(det.device).synchronize()
        out = []
        for f in range(self.n_files):
            a, b = int(self.woff[f]), int(self.woff[f + 1])
            out.append(dict(sr=self.sr, win=self.win, hop=self.hop, kmin=self.kmin, kmax=self.kmax,
                            min_strength=self.min_strength, start_windows=self.start_windows,
                            time=(np.arange(b - a) * self.hop + self.win / 2) / self.sr,
                            lag=t["lag"][a:b].copy(), rho=t["rho"][a:b].copy(), bpm=t["bpm"][a:b].copy(),
                            n_valid=int(t["n_valid"][f]), n_strong=int(t["n_strong"][f]),
                            median_bpm=float(t["median_bpm"][f]), mean_rho=float(t["mean_rho"][f]),
                            hint=float(t["hint"][f])))
        return out


@dataclass
class HrvSpectrum:
    """bpmx_hrvspec_device's outputs for one batch (device tensors): per window
    the code, the interval count, the centre time, the variance, LF and HF
    power and the band peaks (recording f's windows are
    ``[woff[f], woff[f + 1])``), optionally the rows of ``q``, per recording the
    8-double record and a status."""
    det: "object"
    beats: "object"
    sr: int
    g: dict                      # hrv_spectrum.geometry's dict
    lengths: np.ndarray          # [F] int64 envelope lengths, host
    woff: np.ndarray             # [F + 1] int64, host
    code: "object"
    n_rr: "object"
    lf_peak: "object"
    hf_peak: "object"
    t_mid: "object"
    var: "object"
    lf: "object"
    hf: "object"
    q: "object"                  # None without want_q
    record: "object"
    status: "object"

    @property
    def n_files(self) -> int:
        return len(self.woff) - 1

    def to_host(self) -> List[dict]:
        """Per recording the dict of ``hrv_spectrum.spectrum``: the settings,
        ``time``, ``n_rr``, ``code``, ``var``, ``lf``, ``hf``, ``lf_peak``,
        ``hf_peak`` (``q`` with want_q), ``record`` and ``status``.  Raises
        BpmxError (E_LIMIT) when the peak table was too small."""
        torch = _torch()
        det = self.det
        names = ["code", "n_rr", "lf_peak", "hf_peak", "t_mid", "var", "lf", "hf", "record", "status"]
        if self.q is not None:
            names.append("q")
        with det.lock:
            t = {k: getattr(self, k).cpu().numpy() for k in names}
            torch.cuda.current_stream(det.device).synchronize()
        if (t["status"][:self.n_files] == N.HRVSPEC_OVERFLOW).any():
            raise N.BpmxError("packed tables too small for the beats' slices", N.E_LIMIT)
        nq = self.g["n_freq"]
        out = []
        for f in range(self.n_files):
            a, b = int(self.woff[f]), int(self.woff[f + 1])
            d = dict(self.g, sr=self.sr, status=int(t["status"][f]), time=t["t_mid"][a:b].copy(),
                     record=t["record"][f * N.HRVSPEC_RECORD:(f + 1) * N.HRVSPEC_RECORD].copy())
            for k in ("n_rr", "code", "var", "lf", "hf", "lf_peak", "hf_peak"):
                d[k] = t[k][a:b].copy()
            if self.q is not None:
                d["q"] = t["q"][a * nq:b * nq].reshape(b - a, nq).copy()
            out.append(d)
        return out


class Detector:
    """One libbpmx context on one GPU.

    Threading (the reference is called from a GUI worker thread, gui.py:181-187,
    and Gradio may call concurrently): ``run`` enqueues under ``lock`` on the
    caller's current stream; the host entry points (``run_host``,
    ``run_env_host``) hold the lock from upload to download on the detector's
    own stream, so a context's scratch is never shared by two calls in flight.
    ``default_detector`` gives each thread its own Detector (context + stream),
    so concurrent threads also run concurrently on the GPU."""

    def __init__(self, device: int = 0):
        torch = _torch()
        if not torch.cuda.is_available():
            raise N.BpmxError("no GPU visible to torch: the bpmx path runs only on an MI355X (gfx950)")
        self.L = N.load()
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        torch.empty(1, device=self.device)      # initialise the HIP runtime on this device
        ctx = ctypes.c_void_p()
        N.check(self.L.bpmx_create(device, ctypes.byref(ctx)), "bpmx_create")
        self.ctx = ctx
        self.lock = threading.RLock()
        self._stream = None
        self._pinned = {}

    def close(self):
        if getattr(self, "ctx", None):
            self.L.bpmx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ #
    def host_stream(self):
        """The stream of the host entry points (created on first use)."""
        if self._stream is None:
            self._stream = _torch().cuda.Stream(self.device)
        return self._stream

    def stream_handle(self) -> ctypes.c_void_p:
        return ctypes.c_void_p(_torch().cuda.current_stream(self.device).cuda_stream)

    def alloc(self, frame_offsets: Sequence[int], ds: int, sr: int, want_y: bool = False,
              want_floor: bool = True, want_troughs: bool = True, want_peaks: bool = True) -> Result:
        torch = _torch()
        fo = np.ascontiguousarray(frame_offsets, dtype=np.int64)
        lens = np.diff(fo)
        nd = np.where(lens > 0, (lens + ds - 1) // ds, 0)
        doff = np.zeros(len(fo), dtype=np.int64)
        doff[1:] = np.cumsum(nd)
        tot, F = int(doff[-1]), len(fo) - 1
        dev = self.device
        e = lambda dt: torch.empty(max(tot, 1), dtype=dt, device=dev)
        return Result(sr=sr, ds=ds, frame_offsets=fo, doff=doff, env=e(torch.float64),
                      floor=e(torch.float64) if want_floor else None, y=e(torch.float64) if want_y else None,
                      troughs=e(torch.int64) if want_troughs else None, peaks=e(torch.int64) if want_peaks else None,
                      n_troughs=torch.zeros(F, dtype=torch.int32, device=dev),
                      n_peaks=torch.zeros(F, dtype=torch.int32, device=dev),
                      n_raw_troughs=torch.zeros(F, dtype=torch.int32, device=dev),
                      flags=torch.zeros(F, dtype=torch.int32, device=dev))

    def run(self, pcm, frame_offsets: Sequence[int], fs: int, params: dict, mode: str = "reference",
            stages: int = N.STAGE_ALL, channels: int = 1, out: Optional[Result] = None, want_y: bool = False,
            d: Optional[Design] = None, log: bool = False, options: int = 0,
            order: Optional[N.PeakOrder] = None, sample_format: Optional[str] = None) -> Result:
        """Run `stages` over a device batch.  `pcm` is a CUDA tensor (or None when
        ENVELOPE is not requested and `out.env` already holds the envelopes).
        `sample_format="i24"`: `pcm` is a uint8 tensor of packed 24-bit samples
        (3 bytes each, little-endian; BPMX_DT_I24), at any byte offset.
        `order`: bpmx_run_ordered's candidate export / visiting ranks (see
        ``resolve_ties``)."""
        _no_filtered_signal(mode, want_y or (out is not None and out.y is not None))
        if d is None:
            d = mode_design(fs, params, mode, log=log)
        fo = np.ascontiguousarray(frame_offsets, dtype=np.int64)
        if out is None:
            out = self.alloc(fo, d.ds, d.sr, want_y=want_y)
        if sample_format not in (None, "i24"):
            raise ValueError(f"unknown sample_format {sample_format!r} (None or 'i24')")
        if pcm is not None:
            np_dt = {v: k for k, v in _torch_np_map().items()}[pcm.dtype]
            dt, width = dtype_code(np_dt), 1
            if sample_format == "i24":
                if np_dt != np.dtype(np.uint8):
                    raise TypeError("sample_format='i24' needs a uint8 tensor of packed samples")
                dt, width = N.DT_I24, 3
            assert pcm.is_cuda and pcm.is_contiguous()
            assert pcm.numel() >= int(fo[-1]) * channels * width, "pcm shorter than frame_offsets[-1] * channels"
            pcm_ptr = pcm.data_ptr()
        else:
            dt, pcm_ptr = N.DT_I16, None
        p = make_params(d, params, MODES[mode], stages, dt, channels)
        p.options = options
        b = N.Batch()
        b.n_files = len(fo) - 1
        b.pcm = pcm_ptr
        b.frame_offsets = fo.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        o = N.Out()
        ptr = lambda t: None if t is None else t.data_ptr()
        o.env, o.floor, o.y = ptr(out.env), ptr(out.floor), ptr(out.y)
        o.troughs, o.peaks = ptr(out.troughs), ptr(out.peaks)
        o.n_troughs, o.n_peaks, o.flags = ptr(out.n_troughs), ptr(out.n_peaks), ptr(out.flags)
        o.n_raw_troughs = ptr(out.n_raw_troughs)
        with self.lock:
            if order is None:
                N.check(self.L.bpmx_run(self.ctx, ctypes.byref(p), ctypes.byref(b), ctypes.byref(o),
                                        self.stream_handle()), "bpmx_run")
            else:
                N.check(self.L.bpmx_run_ordered(self.ctx, ctypes.byref(p), ctypes.byref(b), ctypes.byref(o),
                                                ctypes.byref(order), self.stream_handle()), "bpmx_run_ordered")
        return out

    def resolve_ties(self, out: Result, params: dict, stages: int = N.STAGE_ALL, options: int = 0) -> int:
        """Re-decide find_peaks' distance filter in numpy's own argsort order for
        the recordings of `out` that carry a decisive-tie bit (F_TROUGH_TIE /
        F_PEAK_TIE), so their troughs, floor and raw peaks are the reference's
        on this machine.

        scipy visits the distance filter's candidates in ``np.argsort(x[peaks])``
        order (``_select_by_peak_distance``, scipy/signal/_peak_finding.py:976-980,
        called from bpm_analysis.py:1070 and :227).  Among equal heights that
        order is numpy's implementation detail, so it is computed here, by numpy,
        from the candidate list the library exports; the library then decides the
        filter by those ranks (include/bpmx.h ``bpmx_run_ordered``).  Troughs
        first: a new trough set changes the floor and so the peak search's
        candidates, whose order is taken after.  The flagged recordings run as a
        sub-batch (ds = 1, envelopes gathered on the device); their results are
        written back into `out` and their flags carry F_*_ORDERED instead of
        F_*_TIE.  `options`: the run's bpmx_option bits, forwarded to the
        sub-batch runs (BPMX_OPT_STATS, which bpmx_run_ordered rejects, masked
        off) so they take the same floor kernels as the original run.  Returns
        the number of recordings re-run (0: nothing to do, no launch).
        Synchronises the current stream."""
        torch = _torch()
        det_st = stages & (N.STAGE_FLOOR | N.STAGE_PEAKS)
        bits = (N.F_TROUGH_TIE if det_st & N.STAGE_FLOOR else 0) | (N.F_PEAK_TIE if det_st & N.STAGE_PEAKS else 0)
        if not bits:
            return 0
        flags = out.flags.cpu().numpy()
        sel = np.flatnonzero(flags & bits)
        if sel.size == 0:
            return 0
        F = int(sel.size)
        lens = out.doff[sel + 1] - out.doff[sel]
        fo = np.zeros(F + 1, dtype=np.int64)
        fo[1:] = np.cumsum(lens)
        tot = int(fo[-1])
        d = detect_design(out.sr, params)
        dev = self.device
        idx = torch.from_numpy(np.concatenate([np.arange(out.doff[f], out.doff[f + 1]) for f in sel])).to(dev)
        sub = self.alloc(fo, 1, d.sr)
        sub.env.copy_(out.env[idx])
        if not det_st & N.STAGE_FLOOR:
            sub.floor.copy_(out.floor[idx])
        env_h = sub.env.cpu().numpy()
        i32 = lambda k: torch.zeros(max(k, 1), dtype=torch.int32, device=dev)
        cand, ncand = [i32(tot), i32(tot)], [i32(F), i32(F)]
        rank, use = [i32(tot), i32(tot)], [i32(F), i32(F)]

        def order(export, ranked):
            o = N.PeakOrder()
            for s in export:
                o.cand[s], o.n_cand[s] = cand[s].data_ptr(), ncand[s].data_ptr()
            for s in ranked:
                o.rank[s], o.use_rank[s] = rank[s].data_ptr(), use[s].data_ptr()
            return o

        def set_ranks(s, files, sign):
            c, nc = cand[s].cpu().numpy(), ncand[s].cpu().numpy()
            r, u = np.zeros(max(tot, 1), dtype=np.int32), np.zeros(F, dtype=np.int32)
            for k in files:
                a, m = int(fo[k]), int(nc[k])
                x = env_h[a:int(fo[k + 1])]
                x = -x if sign < 0 else x                     # find_peaks(-env) negates the array (:1070)
                perm = np.argsort(x[c[a:a + m]])              # the call _select_by_peak_distance makes
                r[a + perm] = np.arange(m, dtype=np.int32)
                u[k] = 1
            rank[s].copy_(torch.from_numpy(r))
            use[s].copy_(torch.from_numpy(u))

        opts = options & ~N.OPT_STATS
        run = lambda st, o: self.run(None, fo, d.sr, params, stages=st, out=sub, d=d, order=o, options=opts)
        ranked = set()
        if det_st & N.STAGE_FLOOR and (flags[sel] & N.F_TROUGH_TIE).any():
            run(det_st, order({0}, ()))
            set_ranks(0, np.flatnonzero(flags[sel] & N.F_TROUGH_TIE), -1.0)
            ranked.add(0)
        run(det_st, order({1} if det_st & N.STAGE_PEAKS else (), ranked))
        fl = sub.flags.cpu().numpy().copy()
        if det_st & N.STAGE_PEAKS and (fl & N.F_PEAK_TIE).any():
            p2 = np.flatnonzero(fl & N.F_PEAK_TIE)
            set_ranks(1, p2, 1.0)
            run(N.STAGE_PEAKS, order((), {1}))
            pb = N.F_PEAK_TIE | N.F_PEAK_ORDERED
            fl = (fl & ~pb) | (sub.flags.cpu().numpy() & pb)
        if det_st & N.STAGE_FLOOR:
            out.floor[idx] = sub.floor[:tot]
            out.troughs[idx] = sub.troughs[:tot]
            out.n_troughs[sel] = sub.n_troughs
            out.n_raw_troughs[sel] = sub.n_raw_troughs
        if det_st & N.STAGE_PEAKS:
            out.peaks[idx] = sub.peaks[:tot]
            out.n_peaks[sel] = sub.n_peaks
        out.flags[torch.from_numpy(sel).to(dev)] = torch.from_numpy(fl).to(dev)
        return F

    def tie_check_start(self, out: Result):
        """Start the flags read-back that ``tie_check_finish`` decides on: an
        asynchronous copy of ``out.flags`` into pinned host memory and an event
        behind it on the current stream, so the host need not wait for the run
        before queuing the next one (a batch pipeline keeps two ``Result`` sets
        and checks run k while run k + 1 is queued)."""
        torch = _torch()
        host = torch.empty(out.flags.shape, dtype=out.flags.dtype, pin_memory=True)
        host.copy_(out.flags, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        return host, ev

    def tie_check_finish(self, handle, out: Result, params: dict, stages: int = N.STAGE_ALL,
                         options: int = 0) -> int:
        """Wait for the read-back ``tie_check_start`` began; if any recording of
        `out` carries a decisive-tie bit, re-decide them (``resolve_ties``: a
        launch and a host sort only then).  Returns the recordings re-run."""
        host, ev = handle
        ev.synchronize()
        bits = N.F_TROUGH_TIE | N.F_PEAK_TIE
        if not (host.numpy() & bits).any():
            return 0
        return self.resolve_ties(out, params, stages, options)

    def synth(self, frame_offsets: Sequence[int], fs: int, channels: int = 1, seed0: int = 0,
              seeds: Optional[Sequence[int]] = None):
        """Synthetic int16 batch generated in HBM (bit-identical to bpmx_synth_host):
        recording f gets seed ``seed0 + f``, or ``seeds[f]`` when given."""
        torch = _torch()
        fo = np.ascontiguousarray(frame_offsets, dtype=np.int64)
        pcm = torch.empty(int(fo[-1]) * channels, dtype=torch.int16, device=self.device)
        runs = [(seed0, 0, len(fo) - 1)] if seeds is None else [(int(sd), f, f + 1) for f, sd in enumerate(seeds)]
        with self.lock:
            for sd, a, b in runs:
                sub = np.ascontiguousarray(fo[a:b + 1])
                N.check(self.L.bpmx_synth(self.ctx, sd, b - a, sub.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                          fs, channels, ctypes.c_void_p(pcm.data_ptr()), self.stream_handle()),
                        "bpmx_synth")
        return pcm

    def profile(self, on: bool):
        N.check(self.L.bpmx_profile(self.ctx, 1 if on else 0), "bpmx_profile")

    def profile_only(self, label: str = ""):
        """Restrict profiling events to launches labelled `label` ("" = all)."""
        N.check(self.L.bpmx_profile_only(self.ctx, label.encode()), "bpmx_profile_only")

    def profile_read(self) -> dict:
        buf = ctypes.create_string_buffer(1 << 16)
        n = self.L.bpmx_profile_read(self.ctx, buf, len(buf))
        if n < 0:
            N.check(n, "bpmx_profile_read")
        out = {}
        for line in buf.value.decode().splitlines():
            name, cnt, ms = line.rsplit(" ", 2)
            out[name] = (int(cnt), float(ms))
        return out

    def set_pipeline(self, chunks: int, env_cus: int = 0, det_cus: int = 0):
        """bpmx_set_pipeline: overlap chunk k's envelope with chunk k-1's detection (0 = off)."""
        N.check(self.L.bpmx_set_pipeline(self.ctx, chunks, env_cus, det_cus), "bpmx_set_pipeline")

    def stats(self) -> dict:
        """Path counters of the last run with options | OPT_STATS (bpmx_stats)."""
        buf = (ctypes.c_int64 * N.NSTATS)()
        rc = self.L.bpmx_stats(self.ctx, buf, N.NSTATS)
        if rc < 0:
            N.check(rc, "bpmx_stats")
        return {"raw_troughs": int(buf[N.STAT_RAW_TROUGHS]), "undecided": int(buf[N.STAT_UNDECIDED]),
                "full_draft_chunks": int(buf[N.STAT_FULL_DRAFT])}

    def floor_whole(self) -> int:
        """Recordings that the half-recording floor launch of the last run with
        options | OPT_STATS handed to the whole-recording one
        (BPMX_STAT_FLOOR_WHOLE).  Not among stats(): it depends on how the
        batch was cut into runs (a pipelined run's chunk with no eligible
        recording takes the one-workgroup launch and counts none)."""
        buf = (ctypes.c_int64 * N.NSTATS)()
        rc = self.L.bpmx_stats(self.ctx, buf, N.NSTATS)
        if rc < 0:
            N.check(rc, "bpmx_stats")
        return int(buf[N.STAT_FLOOR_WHOLE])

    # ------------------------------------------------------------------ #
    def run_host(self, recordings: List[np.ndarray], fs: int, params: dict, mode: str = "reference",
                 stages: int = N.STAGE_ALL, want_y: bool = False, log: bool = False,
                 options: int = 0, longest_first: bool = True, resolve_ties: bool = False) -> List[dict]:
        """Host arrays in, per-file host results out (H2D + run + D2H).

        A ragged batch runs longest recording first (shard.longest_first: LPT
        over the CUs, since recording f is workgroup f of every per-recording
        kernel); results come back in the caller's order.  `resolve_ties`:
        decisive find_peaks ties re-decided in numpy's order (``resolve_ties``;
        the drop-in entry points set it)."""
        torch = _torch()
        if not recordings:
            return []
        if longest_first and len({r.shape[0] for r in recordings}) > 1:
            from .shard import longest_first as _lf
            perm = _lf([r.shape[0] for r in recordings])
            res = self.run_host([recordings[i] for i in perm], fs, params, mode=mode, stages=stages,
                                want_y=want_y, log=log, options=options, longest_first=False,
                                resolve_ties=resolve_ties)
            out: List[dict] = [None] * len(recordings)
            for k, i in enumerate(perm):
                out[i] = res[k]
            return out
        host, fo, ch, fmt = _flatten_batch(recordings)
        with self.lock, torch.cuda.stream(self.host_stream()):
            pcm = torch.from_numpy(host).to(self.device)
            res = self.run(pcm, fo, fs, params, mode=mode, stages=stages, channels=ch, want_y=want_y, log=log,
                           options=options, sample_format=fmt)
            if resolve_ties:
                self.resolve_ties(res, params, stages, options)
            out = res.to_host()          # .cpu() waits for this stream only
            self.host_stream().synchronize()
        return out

    def staging(self, name: str, n: int, dtype):
        """A pinned host tensor of `n` elements for the packed download (one
        grow-only buffer per name: pinning is far dearer than the copies)."""
        torch = _torch()
        t = self._pinned.get(name)
        if t is None or t.numel() < n or t.dtype != dtype:
            t = self._pinned[name] = torch.empty(max(n + n // 8, 16), dtype=dtype, pin_memory=True)
        return t[:n]

    def alloc_packed(self, res: Result, distance: int, want_y16: bool = False, cap_peaks: Optional[int] = None,
                     cap_troughs: Optional[int] = None) -> Packed:
        """Device tensors for ``pack``; the default capacities are the sum of
        ``peak_capacity`` over the files, which a run's totals cannot exceed."""
        torch = _torch()
        nd = np.diff(res.doff)
        safe = int(sum(peak_capacity(n, distance) for n in nd))
        cp = safe if cap_peaks is None else int(cap_peaks)
        ct = safe if cap_troughs is None else int(cap_troughs)
        F, tot, dev = res.n_files, int(res.doff[-1]), self.device
        e = lambda n, dt: torch.empty(max(int(n), 1), dtype=dt, device=dev)
        return Packed(det=self, sr=res.sr, doff=res.doff, cap_peaks=cp, cap_troughs=ct, safe_peaks=safe,
                      safe_troughs=safe, pk_off=e(F + 1, torch.int64), tr_off=e(F + 1, torch.int64),
                      pk_idx=e(cp, torch.int32), pk_env=e(cp, torch.float64), pk_floor=e(cp, torch.float64),
                      tr_idx=e(ct, torch.int32), tr_env=e(ct, torch.float64),
                      y16=e(tot, torch.int16) if want_y16 else None,
                      y_max=e(F, torch.float64) if want_y16 else None)

    def pack(self, res: Result, distance: int, want_y16: bool = False, out: Optional[Packed] = None,
             want_tr_floor: bool = False) -> Packed:
        """bpmx_pack on the current stream, behind the run (and any
        ``resolve_ties``) that filled `res`: the per-peak / per-trough tables
        and, with `want_y16` (``res.y`` required), the int16 debug samples.
        Asynchronous with the default capacities.  Tables smaller than those
        (an `out` from ``alloc_packed`` with its own capacities) are checked
        here, which waits for the stream: BpmxError (E_LIMIT) when a total
        exceeds its capacity; the offsets then still hold the true totals and
        nothing at or beyond the capacity was written.  `want_tr_floor`:
        ``out.tr_floor`` gets the floor at the troughs (bpmx_pack_trough_floor,
        behind the pack on the same stream), which the debug log reads."""
        if res.peaks is None or res.troughs is None or res.floor is None:
            raise N.BpmxError("pack needs a Result with floor, troughs and peaks", N.E_ARG)
        if out is None:
            out = self.alloc_packed(res, distance, want_y16=want_y16)
        if want_y16 and (res.y is None or out.y16 is None):
            raise N.BpmxError("want_y16 needs a Result that holds y (want_y=True)", N.E_ARG)
        out.n_raw_troughs, out.flags = res.n_raw_troughs, res.flags
        ptr = lambda t: None if t is None else t.data_ptr()
        o = N.Out()
        o.env, o.floor, o.y = ptr(res.env), ptr(res.floor), ptr(res.y)
        o.troughs, o.peaks = ptr(res.troughs), ptr(res.peaks)
        o.n_troughs, o.n_peaks, o.flags = ptr(res.n_troughs), ptr(res.n_peaks), ptr(res.flags)
        o.n_raw_troughs = ptr(res.n_raw_troughs)
        k = N.PackedOut()
        k.cap_peaks, k.cap_troughs = out.cap_peaks, out.cap_troughs
        k.pk_off, k.tr_off = ptr(out.pk_off), ptr(out.tr_off)
        k.pk_idx, k.pk_env, k.pk_floor = ptr(out.pk_idx), ptr(out.pk_env), ptr(out.pk_floor)
        k.tr_idx, k.tr_env = ptr(out.tr_idx), ptr(out.tr_env)
        if want_y16:
            k.y16, k.y_max = ptr(out.y16), ptr(out.y_max)
        fo = res.frame_offsets
        with self.lock:
            N.check(self.L.bpmx_pack(self.ctx, res.n_files, fo.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                     res.ds, ctypes.byref(o), ctypes.byref(k), self.stream_handle()), "bpmx_pack")
            if want_tr_floor:
                if not hasattr(self.L, "bpmx_pack_trough_floor"):
                    raise N.BpmxError("libbpmx.so has no bpmx_pack_trough_floor; rebuild")
                if out.tr_floor is None:
                    torch = _torch()
                    out.tr_floor = torch.empty(max(int(out.cap_troughs), 1), dtype=torch.float64, device=self.device)
                N.check(self.L.bpmx_pack_trough_floor(self.ctx, ctypes.byref(o),
                                                      fo.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), res.n_files,
                                                      res.ds, ctypes.byref(k), out.tr_floor.data_ptr(),
                                                      self.stream_handle()), "bpmx_pack_trough_floor")
        if out.cap_peaks < out.safe_peaks or out.cap_troughs < out.safe_troughs:
            F = res.n_files
            out._check(int(out.pk_off[F].item()), int(out.tr_off[F].item()))
        return out

    def pack_plot(self, res: Result, factor: int, want_floor: bool = True, out=None) -> PlotSeries:
        """The plot's line traces of `res` at ``plot_downsample_factor``
        `factor` (an integer): per recording ``env[::kf]`` and ``floor[::kf]``
        with the reference's rule for kf (bpmx_plot_length), made by
        bpmx_pack_plot on the current stream behind the run.  Asynchronous.
        When every recording's kf is 1 (the shipped factor) the series are
        ``res.env`` / ``res.floor`` themselves and nothing is launched.
        `out`: (env, floor) device float64 tensors to fill instead (floor None
        without `want_floor`); then the kernel always runs, and a total above
        their length is a BpmxArgError with nothing written."""
        if res.env is None or (want_floor and res.floor is None):
            raise N.BpmxError("pack_plot needs a Result with env (and floor)", N.E_ARG)
        if not hasattr(self.L, "bpmx_pack_plot"):
            raise N.BpmxError("libbpmx.so has no bpmx_pack_plot; rebuild")
        factor = int(factor)
        if not -2 ** 31 <= factor < 2 ** 31:
            raise N.BpmxError("pack_plot: factor outside int32 (plot_device_factor clamps it)", N.E_ARG)
        nd = np.diff(res.doff)
        n = np.array([self.L.bpmx_plot_length(int(x), factor) for x in nd], dtype=np.int64)
        kf = np.where(n == nd, 1, factor).astype(np.int64)
        off = np.zeros(res.n_files + 1, dtype=np.int64)
        off[1:] = np.cumsum(n)
        if out is None and bool((kf == 1).all()):
            return PlotSeries(det=self, factor=factor, kf=kf, off=off, env=res.env,
                              floor=res.floor if want_floor else None)
        torch = _torch()
        if out is None:
            e = lambda: torch.empty(max(int(off[-1]), 1), dtype=torch.float64, device=self.device)
            out = (e(), e() if want_floor else None)
        oe, of = out
        if of is not None and not want_floor:
            of = None
        cap = oe.numel() if of is None else min(oe.numel(), of.numel())
        o = N.Out()
        o.env = res.env.data_ptr()
        o.floor = None if res.floor is None else res.floor.data_ptr()
        fo = res.frame_offsets
        with self.lock:
            N.check(self.L.bpmx_pack_plot(self.ctx, res.n_files, fo.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                          res.ds, factor, ctypes.byref(o), oe.data_ptr(),
                                          None if of is None else of.data_ptr(), cap, self.stream_handle()),
                    "bpmx_pack_plot")
        return PlotSeries(det=self, factor=factor, kf=kf, off=off, env=oe, floor=of)

    def _batch_on_device(self, recordings: List[np.ndarray], fs: int, params: dict, mode: str, stages: int,
                         want_y: bool, resolve_ties: bool, options: int = 0):
        """Upload one batch, run it and re-decide its ties (the caller holds the
        lock and has the host stream current) -> (Result, Design)."""
        torch = _torch()
        host, fo, ch, fmt = _flatten_batch(recordings)
        _no_filtered_signal(mode, want_y)
        d = mode_design(fs, params, mode)
        pcm = torch.from_numpy(host).to(self.device)
        res = self.run(pcm, fo, fs, params, mode=mode, stages=stages, channels=ch, want_y=want_y, d=d,
                       options=options, sample_format=fmt)
        if resolve_ties:
            self.resolve_ties(res, params, stages, options)
        return res, d

    def _in_callers_order(self, fn, recordings: List[np.ndarray], longest_first: bool) -> List[dict]:
        """`fn(recordings)` with a ragged batch handed over longest first
        (``run_host``'s rule), results back in the caller's order."""
        if not (longest_first and len({r.shape[0] for r in recordings}) > 1):
            return fn(recordings)
        from .shard import longest_first as _lf
        perm = _lf([r.shape[0] for r in recordings])
        res = fn([recordings[i] for i in perm])
        out: List[dict] = [None] * len(recordings)
        for k, i in enumerate(perm):
            out[i] = res[k]
        return out

    def run_host_packed(self, recordings: List[np.ndarray], fs: int, params: dict, mode: str = "reference",
                        stages: int = N.STAGE_ALL, resolve_ties: bool = False, want_y16: bool = False,
                        longest_first: bool = True) -> List[dict]:
        """``run_host`` for consumers that read the envelope and the floor only
        at the raw peaks and troughs (the native beat stages, the result
        gather): upload, run, ``resolve_ties``, ``pack`` and the packed
        download (``Packed.to_host``'s per-file dicts).  env, floor, y and the
        sum(Nd)-long index arrays never leave the device.  Same lock, stream
        and longest-first rules as ``run_host``."""
        torch = _torch()
        if not recordings:
            return []

        def go(recs):
            with self.lock, torch.cuda.stream(self.host_stream()):
                res, d = self._batch_on_device(recs, fs, params, mode, stages, want_y16, resolve_ties)
                out = self.pack(res, d.distance, want_y16=want_y16).to_host()
                self.host_stream().synchronize()
            return out

        return self._in_callers_order(go, list(recordings), longest_first)

    def beats_device(self, packed: Packed, params, hint: Optional[float] = None,
                     hints: Optional[Sequence[Optional[float]]] = None, trace: bool = False) -> Beats:
        """bpmx_beats_device on the current stream, behind the ``pack`` that
        filled `packed`: the beat stages (preliminary pass, classifier,
        refinement, BPM curve) of every recording from its peak table, on the
        GPU.  ``params``: the parameter dict or a prepared _host.BeatParams.
        Asynchronous; outputs are sized by ``packed.cap_peaks``.

        ``hints``: one start BPM per recording (None = no hint) in place of
        `hint` for all of them, in the same launch, or the ``Tempo`` of
        ``tempo_device``, whose device ``hint`` array the launch then reads
        with no download.  ``trace``: the decision
        trace (``Beats.trace``; bpmx_beats_device_ex, kernel k_beats_trace)
        beside the same results, for ``Beats.to_host(explain=True)``."""
        from . import _host
        torch = _torch()
        bp = params if isinstance(params, _host.BeatParams) else _host.beat_params(params)
        F, cap, dev = packed.n_files, max(int(packed.cap_peaks), 1), self.device
        e = lambda n, dt: torch.empty(n, dtype=dt, device=dev)  # noqa: E731
        out = Beats(det=self, packed=packed, final_idx=e(cap, torch.int32), n_final=e(F, torch.int32),
                    bpm_t=e(cap, torch.float64), bpm=e(cap, torch.float64), n_bpm=e(F, torch.int32),
                    pass_=e(3 * F, torch.float64), tags=e(cap, torch.int8), status=e(F, torch.int32))
        k = N.PackedOut()
        k.cap_peaks = packed.cap_peaks
        k.pk_off, k.pk_idx = packed.pk_off.data_ptr(), packed.pk_idx.data_ptr()
        k.pk_env, k.pk_floor = packed.pk_env.data_ptr(), packed.pk_floor.data_ptr()
        o = N.BeatsOut()
        o.final_idx, o.n_final = out.final_idx.data_ptr(), out.n_final.data_ptr()
        o.bpm_t, o.bpm, o.n_bpm = out.bpm_t.data_ptr(), out.bpm.data_ptr(), out.n_bpm.data_ptr()
        o.pass_, o.tags, o.status = out.pass_.data_ptr(), out.tags.data_ptr(), out.status.data_ptr()
        flags = None if packed.flags is None else packed.flags.data_ptr()
        h0 = float("nan") if hint is None else float(hint)
        if hints is None and not trace:
            with self.lock:
                N.check(self.L.bpmx_beats_device(self.ctx, F, int(packed.sr), ctypes.byref(bp), h0, ctypes.byref(k),
                                                 flags, ctypes.byref(o), self.stream_handle()), "bpmx_beats_device")
            return out
        if not hasattr(self.L, "bpmx_beats_device_ex"):
            raise N.BpmxError("libbpmx.so has no bpmx_beats_device_ex; rebuild")
        if not isinstance(params, _host.BeatParams):
            out.params = dict(params)
        d_hints = None
        if isinstance(hints, Tempo):         # the tempo stage's hints, read where they lie
            if hints.n_files != F:
                raise N.BpmxError("beats_device: hints needs one entry per recording", N.E_ARG)
            d_hints = hints.hint
        elif hints is not None:
            if len(hints) != F:
                raise N.BpmxError("beats_device: hints needs one entry per recording", N.E_ARG)
            hh = np.array([np.nan if h is None else float(h) for h in hints], dtype=np.float64)
            d_hints = torch.from_numpy(hh).to(dev)
        t = None
        if trace:
            out.trace = Trace(record=e(cap * N.TR_NFIELDS, torch.float64), code=e(cap, torch.int32),
                              lt_pos=e(cap, torch.int32), lt_bpm=e(cap, torch.float64), n_lt=e(F, torch.int32),
                              dev_t=e(cap, torch.float64), dev=e(cap, torch.float64), gap=e(cap, torch.int32))
            t = N.TraceOut()
            for name, _ in N.TraceOut._fields_:
                setattr(t, name, getattr(out.trace, name).data_ptr())
        with self.lock:
            N.check(self.L.bpmx_beats_device_ex(self.ctx, F, int(packed.sr), ctypes.byref(bp), h0, ctypes.byref(k),
                                                flags, ctypes.byref(o), None if d_hints is None else d_hints.data_ptr(),
                                                None if t is None else ctypes.byref(t), self.stream_handle()),
                    "bpmx_beats_device_ex")
        out.hints = d_hints              # read by the launch: alive as long as its results
        return out

    def set_options(self, options: int) -> None:
        """Context-level option bits (N.OPT_BEATS_GLOBAL, N.OPT_METRICS_GLOBAL, N.OPT_LABELS_GLOBAL,
        N.OPT_SCORE_GLOBAL, N.OPT_MARKS_GLOBAL, N.OPT_HRVSPEC_DIRECT; test/diagnostic)."""
        with self.lock:
            N.check(self.L.bpmx_set_options(self.ctx, int(options)), "bpmx_set_options")

    def run_host_beats(self, recordings: List[np.ndarray], fs: int, params: dict, mode: str = "reference",
                       hint: Optional[float] = None, resolve_ties: bool = True,
                       longest_first: bool = True) -> List[dict]:
        """PCM on the host in, beats and BPM curves out, with no host stage in
        between: upload, run, ``resolve_ties``, ``pack``, ``beats_device`` and
        ``Beats.to_host``'s per-file dicts.  Same lock, stream and
        longest-first rules as ``run_host_packed``."""
        torch = _torch()
        if not recordings:
            return []

        def go(recs):
            with self.lock, torch.cuda.stream(self.host_stream()):
                res, d = self._batch_on_device(recs, fs, params, mode, N.STAGE_ALL, False, resolve_ties)
                out = self.beats_device(self.pack(res, d.distance), params, hint).to_host()
                self.host_stream().synchronize()
            return out

        return self._in_callers_order(go, list(recordings), longest_first)

    def metrics_device(self, beats: Beats, params: dict, epoch_us: Optional[int] = None) -> Metrics:
        """bpmx_metrics_device on the current stream, behind the
        ``beats_device`` that filled `beats`: the final metrics (windowed HRV
        table, summary, HRR, steepest slopes, major inclines and declines) of
        every recording from its beats and curve, on the GPU.  ``epoch_us``:
        the origin of the curve's index (default ``beats._epoch()``).
        Asynchronous; outputs are sized by the peak table's capacity."""
        from . import metrics as MH
        torch = _torch()
        packed = beats.packed
        mp = N.metric_params(params)
        eu = MH.epoch_us() if epoch_us is None else int(epoch_us)
        F, cap, dev = packed.n_files, max(int(packed.cap_peaks), 1), self.device
        e = lambda n, dt: torch.empty(n, dtype=dt, device=dev)  # noqa: E731
        rows = {k: e(cap, torch.int32 if k[4:] in ("a", "b") else torch.float64) for k in _METRIC_ROWS}
        out = Metrics(det=self, beats=beats, params=dict(params), epoch_us=eu, n_hrv=e(F, torch.int32),
                      n_inc=e(F, torch.int32), n_dec=e(F, torch.int32),
                      record=e(F * N.METRICS_RECORD, torch.float64), status=e(F, torch.int32), **rows)
        k = N.PackedOut()
        k.cap_peaks, k.pk_off = packed.cap_peaks, packed.pk_off.data_ptr()
        b = N.BeatsOut()
        b.final_idx, b.n_final = beats.final_idx.data_ptr(), beats.n_final.data_ptr()
        b.bpm_t, b.bpm, b.n_bpm = beats.bpm_t.data_ptr(), beats.bpm.data_ptr(), beats.n_bpm.data_ptr()
        b.status = beats.status.data_ptr()
        o = N.MetricsOut()
        for name, _ in N.MetricsOut._fields_:
            setattr(o, name, getattr(out, name).data_ptr())
        with self.lock:
            N.check(self.L.bpmx_metrics_device(self.ctx, F, int(packed.sr), ctypes.byref(mp), eu, ctypes.byref(k),
                                               ctypes.byref(b), ctypes.byref(o), self.stream_handle()),
                    "bpmx_metrics_device")
        return out

    def labels_device(self, beats: Beats, gap_sec: float = 5.0) -> Labels:
        """bpmx_labels_device on the current stream, behind the
        ``beats_device(trace=True)`` that filled `beats`: the labeler's output
        (S1 / S2 label table, S1-S2 pairs, groups of marks with their
        statistics, the mean interval) of every recording from its raw peaks,
        tags, gap-fill labels, final beats and curve, on the GPU.  ``gap_sec``:
        the pause that separates two groups.  Asynchronous; outputs are sized
        by the peak table's capacity."""
        torch = _torch()
        if not hasattr(self.L, "bpmx_labels_device"):
            raise N.BpmxError("libbpmx.so has no bpmx_labels_device; rebuild")
        if beats.trace is None:
            raise N.BpmxError("labels_device needs beats_device(trace=True): the gap-fill labels decide the types",
                              N.E_ARG)
        packed = beats.packed
        F, cap, dev = packed.n_files, max(int(packed.cap_peaks), 1), self.device
        e = lambda n, dt: torch.empty(n, dtype=dt, device=dev)  # noqa: E731
        rows = {k: e(cap, torch.float64 if k in ("lb_time", "lb_bpm", "pr_dt", "gr_dt", "gr_bpm") else torch.int32)
                for k in _LABEL_ROWS}
        out = Labels(det=self, beats=beats, gap_sec=float(gap_sec), n_labels=e(F, torch.int32),
                     n_pairs=e(F, torch.int32), n_groups=e(F, torch.int32),
                     record=e(F * N.LABELS_RECORD, torch.float64), status=e(F, torch.int32), **rows)
        k = N.PackedOut()
        k.cap_peaks, k.pk_off, k.pk_idx = packed.cap_peaks, packed.pk_off.data_ptr(), packed.pk_idx.data_ptr()
        b = N.BeatsOut()
        b.final_idx, b.n_final = beats.final_idx.data_ptr(), beats.n_final.data_ptr()
        b.bpm_t, b.bpm, b.n_bpm = beats.bpm_t.data_ptr(), beats.bpm.data_ptr(), beats.n_bpm.data_ptr()
        b.tags, b.status = beats.tags.data_ptr(), beats.status.data_ptr()
        o = N.LabelsOut()
        for name, _ in N.LabelsOut._fields_:
            setattr(o, name, getattr(out, name).data_ptr())
        lp = N.LabelParams(float(gap_sec))
        with self.lock:
            N.check(self.L.bpmx_labels_device(self.ctx, F, int(packed.sr), ctypes.byref(lp), ctypes.byref(k),
                                              ctypes.byref(b), beats.trace.gap.data_ptr(), ctypes.byref(o),
                                              self.stream_handle()), "bpmx_labels_device")
        return out

    def upload_marks(self, tables: Sequence[Optional[dict]]) -> Marks:
        """A person's corrected marks, one label table per recording
        (``labels.read_labels``; None or an empty table: no marks), prepared by
        ``labels.marks_from_table`` and uploaded as the ragged table
        bpmx_score_device takes."""
        from . import labels as LB
        torch = _torch()
        host = [t if t is not None and "ms" in t else LB.marks_from_table(t) for t in tables]
        off = np.zeros(len(host) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(m["ms"]) for m in host])
        cat = lambda k: np.concatenate([m[k] for m in host] + [np.zeros(1, np.int32)]).astype(np.int32)  # noqa: E731
        up = lambda a: torch.from_numpy(a).to(self.device)  # noqa: E731
        return Marks(det=self, host=host, off=off, rf_off=up(off), rf_ms=up(cat("ms")), rf_type=up(cat("type")))

    def score_device(self, labels: Labels, marks: Marks, tol_sec: float = 0.05, gap_sec: float = 5.0,
                     rows: bool = True) -> Scores:
        """bpmx_score_device on the current stream, behind the
        ``labels_device`` that filled `labels`: every recording's label rows
        scored against its corrected marks (``upload_marks``): per type TP,
        SWAP, FP, FN and the timing errors of the TP, in integer milliseconds
        (``labels.score`` is the same on the host).  ``tol_sec``: two marks
        this close are the same beat (the default ``min_peak_distance_sec``);
        ``gap_sec``: a pause this long between corrected marks ends a labelled
        span, outside which a detection is not a mistake.  ``rows=False``:
        record and status only.  Asynchronous."""
        from . import labels as LB
        torch = _torch()
        if not hasattr(self.L, "bpmx_score_device"):
            raise N.BpmxError("libbpmx.so has no bpmx_score_device; rebuild")
        tol, gap = LB.score_ms(tol_sec, gap_sec)
        packed = labels.beats.packed
        F, cap, dev = packed.n_files, max(int(packed.cap_peaks), 1), self.device
        if marks.n_files != F:
            raise N.BpmxError("score_device: marks needs one table per recording", N.E_ARG)
        e = lambda n, dt: torch.empty(n, dtype=dt, device=dev)  # noqa: E731
        out = Scores(det=self, labels=labels, marks=marks, tol_ms=tol, gap_ms=gap,
                     record=e(F * N.SCORE_RECORD, torch.int64), status=e(F, torch.int32))
        if rows:
            out.sc_kind, out.sc_ref = e(cap, torch.int32), e(cap, torch.int32)
            out.rf_kind, out.rf_det = e(max(marks.cap_ref, 1), torch.int32), e(max(marks.cap_ref, 1), torch.int32)
        k = N.PackedOut()
        k.cap_peaks, k.pk_off = packed.cap_peaks, packed.pk_off.data_ptr()
        lo = N.LabelsOut()
        lo.lb_time, lo.lb_type = labels.lb_time.data_ptr(), labels.lb_type.data_ptr()
        lo.n_labels, lo.status = labels.n_labels.data_ptr(), labels.status.data_ptr()
        r = N.RefMarks(marks.cap_ref, marks.rf_off.data_ptr(), marks.rf_ms.data_ptr(), marks.rf_type.data_ptr())
        o = N.ScoreOut()
        for name, _ in N.ScoreOut._fields_:
            t = getattr(out, name)
            setattr(o, name, None if t is None else t.data_ptr())
        sp = N.ScoreParams(tol, gap)
        with self.lock:
            N.check(self.L.bpmx_score_device(self.ctx, F, ctypes.byref(sp), ctypes.byref(k), ctypes.byref(lo),
                                             ctypes.byref(r), ctypes.byref(o), self.stream_handle()),
                    "bpmx_score_device")
        return out

    def marks_device(self, marks, sr: int, params: dict, nd: Optional[Sequence[int]] = None,
                     cap_peaks: Optional[int] = None) -> Beats:
        """bpmx_marks_device on the current stream: a person's corrected marks
        (``upload_marks``' Marks, or the label tables it takes) as the peak
        table, final beats and BPM curve of every recording at the decimated
        rate `sr`, on the GPU, in the layouts ``metrics_device``,
        ``labels_device`` and ``score_device`` consume (``labels.revise`` is the
        same on the host).  ``params``: the parameter dict
        (``output_smoothing_window_sec`` is read here; ``metrics_device`` reads
        the rest).  ``nd``: the recordings' envelope lengths; a mark at or
        beyond its recording's is dropped.  The result's ``packed`` holds the
        rows (``pk_env`` / ``pk_floor`` NaN, no trough table), its ``trace``
        the zero ``gap``, ``marks_record`` the counts.  ``cap_peaks`` defaults
        to the number of marks, which always suffices.  Asynchronous."""
        torch = _torch()
        if not hasattr(self.L, "bpmx_marks_device"):
            raise N.BpmxError("libbpmx.so has no bpmx_marks_device; rebuild")
        if not isinstance(marks, Marks):
            marks = self.upload_marks(marks)
        F, dev = marks.n_files, self.device
        if nd is not None and len(nd) != F:
            raise N.BpmxError("marks_device: nd needs one entry per recording", N.E_ARG)
        cap_ref = marks.cap_ref
        cap = cap_ref if cap_peaks is None else int(cap_peaks)
        n = max(cap, 1)
        e = lambda k, dt: torch.empty(k, dtype=dt, device=dev)  # noqa: E731
        doff = np.zeros(F + 1, dtype=np.int64)
        d_nd = None
        if nd is not None:
            doff[1:] = np.cumsum(np.asarray(nd, dtype=np.int64))
            d_nd = torch.from_numpy(np.asarray(nd, dtype=np.int64)).to(dev)
        packed = Packed(det=self, sr=int(sr), doff=doff, cap_peaks=cap, cap_troughs=0, safe_peaks=cap_ref,
                        safe_troughs=0, pk_off=e(F + 1, torch.int64), tr_off=None, pk_idx=e(n, torch.int32),
                        pk_env=e(n, torch.float64), pk_floor=e(n, torch.float64), tr_idx=None, tr_env=None,
                        y16=None, y_max=None)
        out = Beats(det=self, packed=packed, final_idx=e(n, torch.int32), n_final=e(F, torch.int32),
                    bpm_t=e(n, torch.float64), bpm=e(n, torch.float64), n_bpm=e(F, torch.int32),
                    pass_=e(3 * F, torch.float64), tags=e(n, torch.int8), status=e(F, torch.int32),
                    trace=Trace(record=None, code=None, lt_pos=None, lt_bpm=None, n_lt=None, dev_t=None, dev=None,
                                gap=e(n, torch.int32)),
                    params=dict(params), marks=marks, marks_record=e(F * N.MARKS_RECORD, torch.int32))
        out.hints = d_nd                 # read by the launch: alive as long as its results
        k = N.PackedOut()
        k.cap_peaks = cap
        k.pk_off, k.pk_idx = packed.pk_off.data_ptr(), packed.pk_idx.data_ptr()
        k.pk_env, k.pk_floor = packed.pk_env.data_ptr(), packed.pk_floor.data_ptr()
        o = N.BeatsOut()
        o.final_idx, o.n_final = out.final_idx.data_ptr(), out.n_final.data_ptr()
        o.bpm_t, o.bpm, o.n_bpm = out.bpm_t.data_ptr(), out.bpm.data_ptr(), out.n_bpm.data_ptr()
        o.pass_, o.tags, o.status = out.pass_.data_ptr(), out.tags.data_ptr(), out.status.data_ptr()
        r = N.RefMarks(cap_ref, marks.rf_off.data_ptr(), marks.rf_ms.data_ptr(), marks.rf_type.data_ptr())
        mp = N.MarksParams(float(params["output_smoothing_window_sec"]))
        with self.lock:
            N.check(self.L.bpmx_marks_device(self.ctx, F, int(sr), ctypes.byref(mp), ctypes.byref(r),
                                             None if d_nd is None else d_nd.data_ptr(), ctypes.byref(k),
                                             ctypes.byref(o), out.trace.gap.data_ptr(), out.marks_record.data_ptr(),
                                             self.stream_handle()), "bpmx_marks_device")
        return out

    def tempo_device(self, res: Result, params: Optional[dict] = None, win_sec: float = 8.0, hop_sec: float = 2.0,
                     min_strength: float = 0.3, start_windows: int = 3,
                     ints: Optional[Sequence[int]] = None) -> Tempo:
        """bpmx_tempo_device on the current stream, behind the run that made
        ``res.env``: the tempogram of every recording (``tempo.tempogram`` is
        the same on the host), a BPM per window from the envelope's
        autocorrelation and the record with the start hint.  The lag range is
        ``max_bpm`` .. ``min_bpm`` of `params` (DEFAULT_PARAMS without);
        ``ints``: (win, hop, kmin, kmax) in samples instead.  The defaults are
        judgement, not measurement.  Asynchronous."""
        from . import tempo as TP
        torch = _torch()
        if not hasattr(self.L, "bpmx_tempo_device"):
            raise N.BpmxError("libbpmx.so has no bpmx_tempo_device; rebuild")
        win, hop, kmin, kmax = [int(v) for v in (ints if ints is not None
                                                 else TP.geometry(res.sr, params, win_sec, hop_sec))]
        F, dev = res.n_files, self.device
        woff = np.zeros(F + 1, np.int64)
        woff[1:] = np.cumsum([TP.n_windows(int(res.doff[f + 1] - res.doff[f]), win, hop) for f in range(F)])
        tot = int(woff[-1])
        e = lambda n, dt: torch.empty(max(n, 1), dtype=dt, device=dev)  # noqa: E731
        out = Tempo(det=self, sr=int(res.sr), win=win, hop=hop, kmin=kmin, kmax=kmax,
                    min_strength=float(min_strength), start_windows=int(start_windows), woff=woff,
                    lag=e(tot, torch.int32), rho=e(tot, torch.float64), bpm=e(tot, torch.float64),
                    n_valid=e(F, torch.int32), n_strong=e(F, torch.int32), median_bpm=e(F, torch.float64),
                    mean_rho=e(F, torch.float64), hint=e(F, torch.float64))
        p = N.TempoParams(win, hop, kmin, kmax, float(min_strength), int(start_windows), 0)
        i = N.Out()
        i.env = res.env.data_ptr()
        o = N.TempoOut()
        for name, _ in N.TempoOut._fields_:
            setattr(o, name, getattr(out, name).data_ptr())
        fo = res.frame_offsets
        with self.lock:
            N.check(self.L.bpmx_tempo_device(self.ctx, F, fo.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), res.ds,
                                             int(res.sr), ctypes.byref(p), ctypes.byref(i), ctypes.byref(o),
                                             self.stream_handle()), "bpmx_tempo_device")
        return out

    def hrv_spectrum_device(self, beats: Beats, lengths: Optional[Sequence[int]] = None,
                            params: Optional[dict] = None, want_q: bool = False, g: Optional[dict] = None,
                            **kw) -> HrvSpectrum:
        """bpmx_hrvspec_device on the current stream, behind the
        ``beats_device`` or ``marks_device`` that filled `beats`: per window of
        every recording the Lomb-Scargle periodogram of its RR intervals, LF
        and HF power and the band peaks (``hrv_spectrum.spectrum`` is the same
        on the host).  ``lengths``: the recordings' envelope lengths in samples
        at the beats' rate; they default to those of the run behind
        ``beats.packed`` and are required for beats that came from
        ``marks_device`` (ValueError otherwise).  The interval range is
        ``max_bpm`` .. ``min_bpm`` of `params` (DEFAULT_PARAMS without); `kw`:
        the other arguments of ``hrv_spectrum.geometry`` (windows of 120 s
        every 30 s, 16 intervals, 256 frequencies from 0.04 to 0.40 Hz, LF up to
        0.15 Hz: judgement, not measurement); ``g``: its dict instead.
        ``want_q``: the rows of q as well.  Asynchronous."""
        from . import hrv_spectrum as HS
        torch = _torch()
        if not hasattr(self.L, "bpmx_hrvspec_device"):
            raise N.BpmxError("libbpmx.so has no bpmx_hrvspec_device; rebuild")
        packed = beats.packed
        F, dev, sr = packed.n_files, self.device, int(packed.sr)
        if lengths is None:
            if beats.marks is not None:
                raise ValueError("hrv_spectrum_device: beats from marks_device carry no recording lengths; "
                                 "pass lengths")
            lengths = np.diff(np.asarray(packed.doff, dtype=np.int64))
        lengths = np.ascontiguousarray(lengths, dtype=np.int64)
        if len(lengths) != F:
            raise ValueError("hrv_spectrum_device: lengths needs one entry per recording")
        g = dict(HS.geometry(sr, params, **kw) if g is None else g)
        HS.check_geometry(g)
        fo = np.zeros(F + 1, np.int64)
        fo[1:] = np.cumsum(lengths)
        woff = np.zeros(F + 1, np.int64)
        woff[1:] = np.cumsum([HS.n_windows(int(n), g["win"], g["hop"]) for n in lengths])
        tot = int(woff[-1])
        e = lambda n, dt: torch.empty(max(n, 1), dtype=dt, device=dev)  # noqa: E731
        out = HrvSpectrum(det=self, beats=beats, sr=sr, g=g, lengths=lengths, woff=woff,
                          code=e(tot, torch.int32), n_rr=e(tot, torch.int32), lf_peak=e(tot, torch.int32),
                          hf_peak=e(tot, torch.int32), t_mid=e(tot, torch.float64), var=e(tot, torch.float64),
                          lf=e(tot, torch.float64), hf=e(tot, torch.float64),
                          q=e(tot * g["n_freq"], torch.float64) if want_q else None,
                          record=e(F * N.HRVSPEC_RECORD, torch.float64), status=e(F, torch.int32))
        k = N.PackedOut()
        k.cap_peaks, k.pk_off = packed.cap_peaks, packed.pk_off.data_ptr()
        b = N.BeatsOut()
        b.final_idx, b.n_final, b.status = beats.final_idx.data_ptr(), beats.n_final.data_ptr(), beats.status.data_ptr()
        o = N.HrvspecOut()
        for name, _ in N.HrvspecOut._fields_:
            v = getattr(out, name)
            setattr(o, name, None if v is None else v.data_ptr())
        p = N.hrvspec_params(g)
        with self.lock:
            N.check(self.L.bpmx_hrvspec_device(self.ctx, F, fo.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 1, sr,
                                               ctypes.byref(p), ctypes.byref(k), ctypes.byref(b), ctypes.byref(o),
                                               self.stream_handle()), "bpmx_hrvspec_device")
        return out

    def score_sweep(self, recordings: List[np.ndarray], fs: int, params_list: Sequence[dict],
                    ref_tables: Sequence[Optional[dict]], mode: str = "reference",
                    hints: Optional[Sequence[Optional[float]]] = None, tol_sec: float = 0.05, gap_sec: float = 5.0,
                    resolve_ties: bool = True):
        """How well each setting of `params_list` reproduces a person's
        corrected marks (`ref_tables`: one label table per recording) on one
        batch: PCM is uploaded and the envelope stage run once; then, per
        setting, FLOOR | PEAKS on that envelope, ``resolve_ties``, ``pack``,
        ``beats_device(trace=True)``, ``labels_device`` and
        ``score_device(rows=False)``.  One download at the end returns
        ``(record [P, F, 20] int64, status [P, F] int32)`` in the caller's
        order of recordings.  ``hints="auto"``: ``tempo_device`` runs once on
        the shared envelope (lag range of the first setting) and every setting's
        beat stages read its hints on the device.  The settings must agree in ``downsample_factor``,
        the only key the envelope stage reads (ValueError otherwise, before
        anything runs).  Same lock, stream and longest-first rules as
        ``run_host_reports``."""
        from . import labels as LB
        torch = _torch()
        recordings, params_list = list(recordings), [dict(p) for p in params_list]
        nF, nP = len(recordings), len(params_list)
        if len({p["downsample_factor"] for p in params_list}) > 1:
            raise ValueError("score_sweep: the settings differ in downsample_factor, which the shared envelope "
                             "is made with; sweep each value on its own")
        if len(ref_tables) != nF:
            raise ValueError("score_sweep: ref_tables needs one entry per recording")
        auto = isinstance(hints, str)
        if auto and hints != "auto":
            raise ValueError('score_sweep: hints is a sequence or "auto"')
        hints = [None] * nF if hints is None or auto else list(hints)
        if len(hints) != nF:
            raise ValueError("score_sweep: hints needs one entry per recording")
        LB.score_ms(tol_sec, gap_sec)
        if nF == 0 or nP == 0:
            return np.zeros((nP, nF, N.SCORE_RECORD), np.int64), np.zeros((nP, nF), np.int32)
        designs = [mode_design(fs, p, mode) for p in params_list]
        for d in designs:
            if d.distance < 1:
                raise ValueError("`distance` must be greater or equal to 1")
        perm = list(range(nF))
        if len({r.shape[0] for r in recordings}) > 1:
            from .shard import longest_first as _lf
            perm = list(_lf([r.shape[0] for r in recordings]))
        recs, hh = [recordings[i] for i in perm], [hints[i] for i in perm]
        det_st = N.STAGE_FLOOR | N.STAGE_PEAKS
        with self.lock, torch.cuda.stream(self.host_stream()):
            marks = self.upload_marks([ref_tables[i] for i in perm])
            res, _ = self._batch_on_device(recs, fs, params_list[0], mode, N.STAGE_ENVELOPE, False, False)
            ch = 1 if recs[0].ndim == 1 else recs[0].shape[1]
            if auto:                             # once per sweep: the envelope is shared
                hh = self.tempo_device(res, params_list[0])
            got = []
            for p, d in zip(params_list, designs):
                self.run(None, res.frame_offsets, fs, p, mode=mode, stages=det_st, channels=ch, out=res, d=d)
                if resolve_ties:
                    self.resolve_ties(res, p, det_st)
                b = self.beats_device(self.pack(res, d.distance), p, hints=hh, trace=True)
                got.append(self.score_device(self.labels_device(b, gap_sec), marks, tol_sec, gap_sec, rows=False))
            rec = torch.stack([s.record for s in got]).reshape(-1)
            st = torch.stack([s.status for s in got]).reshape(-1)
            hr, hs = self.staging("sw_record", rec.numel(), rec.dtype), self.staging("sw_status", st.numel(), st.dtype)
            hr.copy_(rec, non_blocking=True)
            hs.copy_(st, non_blocking=True)
            self.host_stream().synchronize()
            record = hr.numpy().copy().reshape(nP, nF, N.SCORE_RECORD)
            status = hs.numpy().copy().reshape(nP, nF)
        if (status == N.SCORE_OVERFLOW).any():
            raise N.BpmxError("bpmx_score_device: a label or reference table was too small", N.E_LIMIT)
        inv = np.argsort(np.asarray(perm))
        return record[:, inv], status[:, inv]

    def run_host_metrics(self, recordings: List[np.ndarray], fs: int, params: dict, mode: str = "reference",
                         hint: Optional[float] = None, resolve_ties: bool = True,
                         longest_first: bool = True, assemble: bool = True) -> List[dict]:
        """``run_host_beats`` plus the final metrics on the device: PCM on the
        host in, per file the dicts of ``Beats.to_host()`` with
        ``final_metrics`` and ``metrics_source`` (``Metrics.to_host``) out;
        ``assemble=False``: ``metrics_record`` and ``n_hrv`` in its place."""
        torch = _torch()
        if not recordings:
            return []

        def go(recs):
            with self.lock, torch.cuda.stream(self.host_stream()):
                res, d = self._batch_on_device(recs, fs, params, mode, N.STAGE_ALL, False, resolve_ties)
                b = self.beats_device(self.pack(res, d.distance), params, hint)
                out = self.metrics_device(b, params).to_host(assemble=assemble)
                self.host_stream().synchronize()
            return out

        return self._in_callers_order(go, list(recordings), longest_first)

    def run_host_reports(self, recordings: List[np.ndarray], fs: int, params: dict, mode: str = "reference",
                         hints: Optional[Sequence[Optional[float]]] = None, resolve_ties: bool = True,
                         longest_first: bool = True, plot: bool = False, labels: bool = False,
                         label_gap_sec: float = 5.0, tempo: bool = False,
                         hrv_spectrum: bool = False) -> List[dict]:
        """Everything the reference's report set needs, with no classifier on
        the host: upload, run, ``resolve_ties``, ``pack`` (with the floor at
        the troughs, and the int16 debug samples when
        ``params['save_filtered_wav']``), ``beats_device`` with per-file
        `hints` and the decision trace, ``metrics_device``.  Per file the dict
        of ``Metrics.to_host(explain=True)`` (final_peaks, curve,
        ``final_metrics``, ``analysis_data``, ...) merged with
        ``Packed.to_host``'s (sr, n_env, peaks, env_pk, floor_pk, troughs,
        env_tr, floor_tr, y16, y_max), which is what
        ``reports.write_reports_packed`` takes.  With `plot`, each dict also
        carries ``env_plot``, ``floor_plot`` and ``plot_factor``
        (``pack_plot`` at ``params['plot_downsample_factor']``, default 5 as in
        the reference), which ``plot.build_figure_packed`` takes.  With
        `labels`, each dict also carries ``labels`` (``labels_device`` at
        `label_gap_sec`, ``Labels.to_host``: the labeler's table, pairs, groups
        and summary, or None where there are none).  ``hints="auto"``: the
        tempo stage (``tempo_device``) runs on the envelope and the beat stages
        read its hints on the device; each dict then carries
        ``start_bpm_hint`` (the value used, None where there was none).  With
        `tempo`, each dict carries ``tempo`` (``Tempo.to_host``).  With
        `hrv_spectrum`, each dict carries ``hrv_spectrum``
        (``hrv_spectrum_device`` at its defaults, ``HrvSpectrum.to_host``).
        Same lock, stream and longest-first rules as ``run_host_packed``."""
        torch = _torch()
        recordings = list(recordings)
        if not recordings:
            return []
        auto = isinstance(hints, str)
        if auto and hints != "auto":
            raise ValueError('run_host_reports: hints is a sequence or "auto"')
        hints = [None] * len(recordings) if hints is None or auto else list(hints)
        if len(hints) != len(recordings):
            raise ValueError("run_host_reports: hints needs one entry per recording")
        perm = list(range(len(recordings)))
        if longest_first and len({r.shape[0] for r in recordings}) > 1:
            from .shard import longest_first as _lf
            perm = list(_lf([r.shape[0] for r in recordings]))
        recs, hh = [recordings[i] for i in perm], [hints[i] for i in perm]
        y16 = bool(params.get("save_filtered_wav", False))
        with self.lock, torch.cuda.stream(self.host_stream()):
            res, d = self._batch_on_device(recs, fs, params, mode, N.STAGE_ALL, y16, resolve_ties)
            pk = self.pack(res, d.distance, want_y16=y16, want_tr_floor=True)
            if plot:
                ps = self.pack_plot(res, plot_device_factor(params.get("plot_downsample_factor", 5)))
            if auto or tempo:
                tp = self.tempo_device(res, params)
            b = self.beats_device(pk, params, hints=tp if auto else hh, trace=True)
            met = self.metrics_device(b, params)
            if labels:
                lab = self.labels_device(b, label_gap_sec)
            if hrv_spectrum:
                hs = self.hrv_spectrum_device(b, params=params)
            got = met.to_host(explain=True)
            if auto or tempo:
                tps = tp.to_host()
            if hrv_spectrum:
                hss = hs.to_host()
            if labels:
                labs = lab.to_host()
            tabs = pk.to_host()
            if plot:
                series = ps.to_host()
            self.host_stream().synchronize()
        out: List[dict] = [None] * len(recordings)
        for k, i in enumerate(perm):
            out[i] = dict(tabs[k], **got[k])
            if labels:
                out[i]["labels"] = labs[k]
            if auto:
                h = tps[k]["hint"]
                out[i]["start_bpm_hint"] = None if h != h else h
            if tempo:
                out[i]["tempo"] = tps[k]
            if hrv_spectrum:
                out[i]["hrv_spectrum"] = hss[k]
            if plot:
                if tabs[k]["flags"] & N.F_TOO_SHORT:    # no outputs: empty series, not the buffers' old contents
                    series[k]["env_plot"], series[k]["floor_plot"] = np.zeros(0), np.zeros(0)
                out[i].update(series[k])
        return out

    def run_host_y16(self, recordings: List[np.ndarray], fs: int, params: dict, mode: str = "reference",
                     stages: int = N.STAGE_ALL, resolve_ties: bool = False, longest_first: bool = True) -> List[dict]:
        """``run_host``'s per-file dicts (whole env, floor, troughs, peaks) with
        the debug WAV's samples quantised on the device: ``y16`` (int16) and
        ``y_max`` per file, ``y`` None.  The filtered signal is made in HBM
        and read there; 2 bytes per sample come back instead of 8."""
        torch = _torch()
        if not recordings:
            return []

        def go(recs):
            with self.lock, torch.cuda.stream(self.host_stream()):
                res, d = self._batch_on_device(recs, fs, params, mode, stages, True, resolve_ties)
                tot = int(res.doff[-1])
                d16 = torch.empty(max(tot, 1), dtype=torch.int16, device=self.device)
                dmx = torch.empty(res.n_files, dtype=torch.float64, device=self.device)
                self._pack_y16(res, d16, dmx)
                h16 = self.staging("y16", tot, d16.dtype)
                hmx = self.staging("y_max", res.n_files, dmx.dtype)
                h16.copy_(d16[:tot], non_blocking=True)
                hmx.copy_(dmx, non_blocking=True)
                res.y = None                     # stays on the device
                out = res.to_host()              # .cpu() waits for this stream, so the two copies above are done
                self.host_stream().synchronize()
                y16, ymax = h16.numpy().copy(), hmx.numpy().copy()
            for f, r in enumerate(out):
                a = int(res.doff[f])
                r["y16"], r["y_max"] = y16[a:a + len(r["env"])], float(ymax[f])
            return out

        return self._in_callers_order(go, list(recordings), longest_first)

    def _pack_y16(self, res: Result, y16, y_max) -> None:
        """bpmx_pack for the int16 debug samples alone (no tables)."""
        o = N.Out()
        o.y = res.y.data_ptr()
        k = N.PackedOut()
        k.y16, k.y_max = y16.data_ptr(), y_max.data_ptr()
        fo = res.frame_offsets
        with self.lock:
            N.check(self.L.bpmx_pack(self.ctx, res.n_files, fo.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                     res.ds, ctypes.byref(o), ctypes.byref(k), self.stream_handle()), "bpmx_pack")

    def run_env_host(self, envs: List[np.ndarray], sr: int, params: dict, stages: int,
                     floors: Optional[List[np.ndarray]] = None, options: int = 0,
                     resolve_ties: bool = False) -> List[dict]:
        """Detection stages on host envelopes (drop-in for the env-level functions)."""
        torch = _torch()
        fo = np.zeros(len(envs) + 1, dtype=np.int64)
        fo[1:] = np.cumsum([len(e) for e in envs])   # ds = 1: offsets == decimated offsets
        d = detect_design(sr, params)
        with self.lock, torch.cuda.stream(self.host_stream()):
            out = self.alloc(fo, 1, d.sr)
            out.env.copy_(torch.from_numpy(np.concatenate(envs).astype(np.float64)).to(self.device))
            if floors is not None:
                out.floor.copy_(torch.from_numpy(np.concatenate(floors).astype(np.float64)).to(self.device))
            self.run(None, fo, d.sr, params, stages=stages, out=out, d=d, options=options)
            if resolve_ties:
                self.resolve_ties(out, params, stages, options)
            res = out.to_host()
            self.host_stream().synchronize()
        return res


class BatchPipeline:
    """Batches of one geometry through the path back to back, batch k + 1's
    ENVELOPE stage overlapping batch k's detection (FLOOR | PEAKS and the
    decisive-tie check).

    Reference mode's envelope is three bit-exact sequential passes (DF2T
    forward and backward, pandas' Kahan rolling mean, bpm_analysis.py:1045-1054)
    with one lane per recording: 1024 recordings are 16 waves, so for ~2.8 ms
    per batch 240 of the 256 CUs idle, and the detection after it fills the
    chip for ~1.3 ms.  Two library contexts on two HIP streams run the two
    halves of consecutive batches at the same time (the streams' kernels do
    overlap on MI355X: tools/overlap_probe), so a stream of batches costs
    max(envelope, detection) per batch instead of their sum.  ``depth`` result
    sets rotate; batch k's envelope waits (an event, no host wait) until the
    detection that last used its result set is done.

    ``submit(pcm)`` enqueues one batch and returns its Result (complete once
    ``finish`` or a later ``submit`` has checked it); ``finish()`` drains.
    Every batch's outputs equal a single ``Detector.run`` of all stages."""

    def __init__(self, device: int, frame_offsets: Sequence[int], fs: int, params: dict, mode: str = "reference",
                 channels: int = 1, options: int = 0, depth: int = 2, d: Optional[Design] = None,
                 det_free_cus: int = 48, env_priority: bool = True, env_masked: bool = False):
        torch = _torch()
        self.fo = np.ascontiguousarray(frame_offsets, dtype=np.int64)
        self.fs, self.params, self.mode, self.channels, self.options = fs, params, mode, channels, options
        self.d = d if d is not None else design(fs, params, log=False)
        self.env_det, self.det_det = Detector(device), Detector(device)
        # The envelope chain is a sequence of small launches: each needs a free
        # CU when it starts, and a detection kernel's workgroups hold a whole
        # CU's LDS for ~0.1 ms each.  So the detection stream leaves
        # `det_free_cus` CUs out of its mask (spread over the XCDs), and the
        # envelope stream has the higher priority for the CUs that do free up.
        if env_masked:
            self.s_env = cu_masked_stream(self.env_det.device, det_free_cus, only=True)
        else:
            self.s_env = torch.cuda.Stream(self.env_det.device, priority=-1 if env_priority else 0)
        self.s_det = cu_masked_stream(self.det_det.device, det_free_cus)
        self._own = [s for s in (self.s_env, self.s_det) if isinstance(s, torch.cuda.ExternalStream)]
        self.outs = [self.det_det.alloc(self.fo, self.d.ds, self.d.sr) for _ in range(max(2, depth))]
        self.ev_free = [None] * len(self.outs)
        self.pending = None
        self.k = 0
        self.ties_resolved = 0

    def _check(self, pend):
        """Batch `pend`'s tie check (its read-back was queued behind its
        detection); a resolution runs on the detection stream and re-marks
        when the batch's result set is free."""
        if pend is None:
            return
        torch = _torch()
        h, o, i = pend
        with torch.cuda.stream(self.s_det):
            r = self.det_det.tie_check_finish(h, o, self.params, N.STAGE_FLOOR | N.STAGE_PEAKS, self.options)
            if r:
                ev = torch.cuda.Event()
                ev.record(self.s_det)
                self.ev_free[i] = ev
        self.ties_resolved += r

    def submit(self, pcm) -> Result:
        torch = _torch()
        i = self.k % len(self.outs)
        o = self.outs[i]
        with torch.cuda.stream(self.s_env):
            if self.ev_free[i] is not None:
                self.s_env.wait_event(self.ev_free[i])
            self.env_det.run(pcm, self.fo, self.fs, self.params, mode=self.mode, stages=N.STAGE_ENVELOPE,
                             channels=self.channels, out=o, d=self.d, options=self.options)
            ev_env = torch.cuda.Event()
            ev_env.record(self.s_env)
        with torch.cuda.stream(self.s_det):
            self.s_det.wait_event(ev_env)
            self.det_det.run(None, self.fo, self.fs, self.params, mode=self.mode,
                             stages=N.STAGE_FLOOR | N.STAGE_PEAKS, channels=self.channels, out=o, d=self.d,
                             options=self.options)
            h = self.det_det.tie_check_start(o)
            ev_free = torch.cuda.Event()
            ev_free.record(self.s_det)
            self.ev_free[i] = ev_free
        # batch k - 1's tie check, with batch k's envelope and detection already queued
        prev, self.pending = self.pending, (h, o, i)
        self._check(prev)
        self.k += 1
        return o

    def finish(self):
        torch = _torch()
        prev, self.pending = self.pending, None
        self._check(prev)
        self.s_env.synchronize()
        self.s_det.synchronize()
        torch.cuda.current_stream(self.det_det.device).wait_stream(self.s_det)

    def close(self):
        """Drain, free both contexts and destroy the CU-masked stream(s): a
        stream left to the HIP runtime's exit-time teardown can outlive the
        tools that hooked it (rocprofv3 faulted there)."""
        if self.env_det is None:
            return
        self.s_env.synchronize()
        self.s_det.synchronize()
        self.env_det.close()
        self.det_det.close()
        for s in self._own:
            destroy_stream(s)
        self._own, self.env_det, self.det_det = [], None, None


def destroy_stream(s):
    """hipStreamDestroy of a stream cu_masked_stream made (torch does not own
    an ExternalStream's handle)."""
    hip = ctypes.CDLL("libamdhip64.so")
    rc = hip.hipStreamDestroy(ctypes.c_void_p(s.cuda_stream))
    if rc != 0:
        raise N.BpmxError(f"hipStreamDestroy failed ({rc})")


def cu_masked_stream(device, free_cus: int, only: bool = False):
    """A torch stream on `device` whose kernels avoid the first `free_cus` CUs
    of the mask (or, with `only`, run on those alone).  hipExtStreamCreateWithCUMask:
    bit c of the mask is the (c / 8)-th CU of XCD c % 8, so the first
    `free_cus` bits are the same share of every XCD.  free_cus <= 0: an
    ordinary stream."""
    torch = _torch()
    if free_cus <= 0:
        return torch.cuda.Stream(device)
    hip = ctypes.CDLL("libamdhip64.so")
    total = torch.cuda.get_device_properties(device).multi_processor_count
    words = (total + 31) // 32
    mask = (ctypes.c_uint32 * words)()
    for c in (range(0, min(free_cus, total)) if only else range(min(free_cus, total), total)):
        mask[c // 32] |= 1 << (c % 32)
    st = ctypes.c_void_p()
    with torch.cuda.device(device):
        rc = hip.hipExtStreamCreateWithCUMask(ctypes.byref(st), ctypes.c_uint32(words), mask)
    if rc != 0:
        raise N.BpmxError(f"hipExtStreamCreateWithCUMask failed ({rc})")
    return torch.cuda.ExternalStream(st.value, device=device)


def _torch_np_map():
    torch = _torch()
    return {np.dtype(np.uint8): torch.uint8, np.dtype(np.int16): torch.int16, np.dtype(np.int32): torch.int32,
            np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}


class _PerThread(threading.local):
    def __init__(self):
        self.dets = {}


_default = _PerThread()


def default_detector(device: int = 0) -> Detector:
    """This thread's Detector on `device` (created on first use, in this thread:
    gui.py runs the analysis on a daemon worker thread, gui.py:181-187)."""
    det = _default.dets.get(device)
    if det is None:
        det = _default.dets[device] = Detector(device)
    return det
