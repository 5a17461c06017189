"""The tempogram on the host: a BPM per window from the short-time
autocorrelation of the envelope, which uses neither ``find_peaks`` nor the
classifier.  ``tempogram`` is the definition of include/bpmx.h
(bpmx_tempo_device) in numpy, the host statement of the stage as ``labels.py``
is for the labels, and the oracle of its tests; ``compare`` holds a window's
BPM against an analysed BPM curve (agree, double, half, other); ``write_csv``
writes ``<base>_tempo.csv``.

The defaults (8 s windows every 2 s, a window is strong from rho 0.3, the hint
comes from the first 3 windows) are judgement, not measurement.
"""
from __future__ import annotations

import csv
import math
import os
from typing import Optional

import numpy as np

from .config import DEFAULT_PARAMS

WIN_SEC, HOP_SEC, MIN_STRENGTH, START_WINDOWS = 8.0, 2.0, 0.3, 3


def geometry(sr: int, params: Optional[dict] = None, win_sec: float = WIN_SEC, hop_sec: float = HOP_SEC):
    """(win, hop, kmin, kmax) in samples at rate `sr`: the lag range is
    ``max_bpm`` .. ``min_bpm`` of `params` (DEFAULT_PARAMS: 240 and 40)."""
    p = DEFAULT_PARAMS if params is None else params
    return (int(win_sec * sr), int(hop_sec * sr), int(math.ceil(60 * sr / p["max_bpm"])),
            int(math.floor(60 * sr / p["min_bpm"])))


def check_geometry(win: int, hop: int, kmin: int, kmax: int) -> None:
    if not (hop >= 1 and kmin >= 2 and kmin <= kmax and kmax + 1 < win):
        raise ValueError("tempogram: needs hop >= 1, 2 <= kmin <= kmax and kmax + 1 < win")


def n_windows(nd: int, win: int, hop: int) -> int:
    """bpmx_tempo_windows."""
    return 0 if win < 1 or hop < 1 or nd < win else (nd - win) // hop + 1


def tempogram_ints(env, sr: int, win: int, hop: int, kmin: int, kmax: int, min_strength: float = MIN_STRENGTH,
                   start_windows: int = START_WINDOWS, detail: bool = False) -> dict:
    """The definition for given integers.  Per window ``time`` (the centre,
    ``(s + win / 2) / sr``), ``lag``, ``rho``, ``bpm``; per recording
    ``n_valid``, ``n_strong``, ``median_bpm``, ``mean_rho``, ``hint``.

    `detail` adds, per window and in units of r[0], how far the decisions were
    from going another way: ``gap`` (best candidate minus the second best, inf
    with one), ``d_lo`` and ``d_hi`` (r[k] - r[k -+ 1]), ``curv`` (the
    parabola's r[k-1] - 2 r[k] + r[k+1]) and ``m_sigma`` (|mean| / standard
    deviation of the window); NaN for an invalid window."""
    check_geometry(win, hop, kmin, kmax)
    x = np.ascontiguousarray(env, dtype=np.float64)
    nw = n_windows(len(x), win, hop)
    lag, rho, bpm = np.zeros(nw, np.int32), np.zeros(nw), np.full(nw, np.nan)
    det = {k: np.full(nw, np.nan) for k in ("gap", "d_lo", "d_hi", "curv", "m_sigma")}
    ks = np.arange(kmin - 1, kmax + 2)
    for w in range(nw):
        seg = x[w * hop:w * hop + win]
        if not np.isfinite(seg).all() or seg.max() == seg.min():
            continue
        m = seg.sum() / win
        e = np.concatenate([seg - m, np.zeros(kmax + 1)])
        r = np.lib.stride_tricks.sliding_window_view(e, win)[kmin - 1:kmax + 2] @ e[:win]
        r0 = float(e[:win] @ e[:win])
        mid = r[1:-1]
        cand = np.flatnonzero((mid > r[:-2]) & (mid >= r[2:]))
        if len(cand) == 0:
            continue
        j = int(cand[np.argmax(mid[cand])]) + 1          # argmax: the first of equal values, the smallest k
        k = int(ks[j])
        d = r[j - 1] - 2 * r[j] + r[j + 1]
        delta = 0.5 * (r[j - 1] - r[j + 1]) / d
        lag[w], rho[w], bpm[w] = k, r[j] / r0, 60.0 * sr / (k + delta)
        if detail:
            v = np.sort(mid[cand])
            det["gap"][w] = (v[-1] - v[-2]) / r0 if len(v) > 1 else np.inf
            det["d_lo"][w], det["d_hi"][w] = (r[j] - r[j - 1]) / r0, (r[j] - r[j + 1]) / r0
            det["curv"][w] = d / r0
            det["m_sigma"][w] = abs(m) / math.sqrt(r0 / win) if r0 > 0 else np.inf
    valid = lag != 0
    strong = valid & (rho >= min_strength)
    first = np.flatnonzero(strong[:max(int(start_windows), 0)])
    out = dict(sr=int(sr), win=int(win), hop=int(hop), kmin=int(kmin), kmax=int(kmax),
               min_strength=float(min_strength), start_windows=int(start_windows),
               time=(np.arange(nw) * hop + win / 2) / sr, lag=lag, rho=rho, bpm=bpm,
               n_valid=int(valid.sum()), n_strong=int(strong.sum()),
               median_bpm=float(np.median(bpm[strong])) if strong.any() else float("nan"),
               mean_rho=float(np.mean(rho[valid])) if valid.any() else float("nan"),
               hint=float(bpm[first[0]]) if len(first) else float("nan"))
    if detail:
        out.update(det)
    return out


def tempogram(env, sr: int, params: Optional[dict] = None, win_sec: float = WIN_SEC, hop_sec: float = HOP_SEC,
              min_strength: float = MIN_STRENGTH, start_windows: int = START_WINDOWS, detail: bool = False) -> dict:
    """The tempogram of one envelope at rate `sr` (``tempogram_ints`` at ``geometry``)."""
    return tempogram_ints(env, sr, *geometry(sr, params, win_sec, hop_sec), min_strength=min_strength,
                          start_windows=start_windows, detail=detail)


def compare(tempo_dict: dict, bpm_times, bpm_values, tol: float = 0.1) -> Optional[dict]:
    """The analysed curve (`bpm_times`, `bpm_values`) against the tempogram
    over its strong windows: the curve is evaluated by ``np.interp`` at the
    window centres, and a window counts as ``agree`` when the curve is within
    `tol` (relative) of the window's BPM, ``double`` / ``half`` when it is
    within `tol` of twice / half of it, else ``other``.  Returns the four
    fractions and ``n``, or None with no strong window or an empty curve."""
    t, v = np.asarray(bpm_times, np.float64), np.asarray(bpm_values, np.float64)
    ok = np.isfinite(t) & np.isfinite(v)
    t, v = t[ok], v[ok]
    strong = (tempo_dict["lag"] != 0) & (tempo_dict["rho"] >= tempo_dict["min_strength"])
    if not strong.any() or len(t) == 0:
        return None
    o = np.argsort(t, kind="stable")
    c = np.interp(tempo_dict["time"][strong], t[o], v[o])
    b = tempo_dict["bpm"][strong]
    near = lambda f: np.abs(c - f * b) <= tol * f * b  # noqa: E731
    agree = near(1.0)
    double = near(2.0) & ~agree
    half = near(0.5) & ~agree & ~double
    n = int(strong.sum())
    return dict(n=n, agree=float(agree.sum() / n), double=float(double.sum() / n), half=float(half.sum() / n),
                other=float((~agree & ~double & ~half).sum() / n), tol=float(tol))


def tempo_path(original_file_path: str, output_directory: str) -> str:
    base = os.path.basename(os.path.splitext(original_file_path)[0])
    return os.path.join(output_directory, f"{base}_tempo.csv")


CSV_HEADER = ["Time (s)", "Lag (samples)", "Strength", "BPM"]


def write_csv(path: str, tempo_dict: dict, cmp: Optional[dict] = None) -> None:
    """``<base>_tempo.csv``: a row per window (floats by ``repr``, so they
    read back as they were), then the record and, with `cmp`, the check as
    ``# key,value`` lines."""
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(CSV_HEADER)
        for t, k, r, b in zip(tempo_dict["time"], tempo_dict["lag"], tempo_dict["rho"], tempo_dict["bpm"]):
            w.writerow([repr(float(t)), int(k), repr(float(r)), repr(float(b))])
        for k in ("sr", "win", "hop", "kmin", "kmax", "min_strength", "start_windows", "n_valid", "n_strong",
                  "median_bpm", "mean_rho", "hint"):
            v = tempo_dict[k]
            w.writerow([f"# {k}", repr(float(v)) if isinstance(v, float) else int(v)])
        if cmp is not None:
            for k in ("n", "agree", "double", "half", "other", "tol"):
                w.writerow([f"# check_{k}", repr(float(cmp[k])) if k != "n" else int(cmp[k])])


def read_csv(path: str):
    """``(tempo_dict, cmp)`` as ``write_csv`` wrote them (cmp None without a check)."""
    rows, rec, chk = [], {}, {}
    with open(path, newline="") as f:
        r = csv.reader(f)
        assert next(r) == CSV_HEADER
        for row in r:
            if row[0].startswith("# check_"):
                chk[row[0][8:]] = int(row[1]) if row[0] == "# check_n" else float(row[1])
            elif row[0].startswith("# "):
                k = row[0][2:]
                rec[k] = float(row[1]) if k in ("min_strength", "median_bpm", "mean_rho", "hint") else int(row[1])
            else:
                rows.append(row)
    d = dict(time=np.array([float(x[0]) for x in rows]), lag=np.array([int(x[1]) for x in rows], np.int32),
             rho=np.array([float(x[2]) for x in rows]), bpm=np.array([float(x[3]) for x in rows]), **rec)
    return d, (chk or None)
