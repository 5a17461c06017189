"""The HRV spectrum on the host: per window of a recording the Lomb-Scargle
periodogram of its RR intervals, the power in the low- and high-frequency
bands and the band peaks.  ``spectrum_ints`` is the definition of
include/bpmx.h (bpmx_hrvspec_device) in numpy, the host statement of the stage
and the oracle of its tests; ``spectrum`` the same from Hz and seconds;
``write_csv`` writes ``<base>_hrv_spectrum.csv``.

The periodogram works on the unevenly spaced intervals as they are: an interval
outside ``min_bpm`` .. ``max_bpm`` (a missed or an extra beat) is left out and
nothing is interpolated over the gap.  ``q`` is the floating-mean generalised
Lomb-Scargle power of Zechmeister and Kuerster (2009), equations 7 to 20,
normalised to [0, 1]: what ``scipy.signal.lombscargle(s, u, omega,
normalize=True, floating_mean=True)`` computes, here in one pass with the
rotation by tau done analytically.

The defaults (windows of 120 s every 30 s, 16 intervals at least, 256
frequencies from 0.04 to 0.40 Hz, LF 0.04 to 0.15 Hz and HF 0.15 to 0.40 Hz) are
judgement, not measurement: the bands are the usual ones for people, and every
one is an argument, since animals breathe faster than people.  The scale of
``lf`` and ``hf`` (``scale = df_hz / sr``, so that ``var * q * T`` is the
periodogram's usual ``A^2 T / 2`` summed over the band, in ms^2) is a
convention; their ratio does not depend on it.
"""
from __future__ import annotations

import csv
import math
import os
from typing import Optional

import numpy as np

from .config import DEFAULT_PARAMS

WIN_SEC, HOP_SEC, MIN_INTERVALS, N_FREQ = 120.0, 30.0, 16, 256
F_LO, F_HI, LF_BAND, HF_BAND = 0.04, 0.40, (0.04, 0.15), (0.15, 0.40)
OK, NONE, OVERFLOW = 0, -26, -27
CODE_VALID, CODE_FEW, CODE_SHORT, CODE_CONSTANT = 0, 1, 2, 3
RECORD = 8
INT_KEYS = ("win", "hop", "dmin", "dmax", "min_intervals", "min_span", "n_freq", "lf_a", "lf_b", "hf_a", "hf_b")
FLOAT_KEYS = ("om0", "dom", "scale")
EPSNEG = float(np.finfo(np.float64).epsneg)


def geometry(sr: int, params: Optional[dict] = None, win_sec: float = WIN_SEC, hop_sec: float = HOP_SEC,
             min_intervals: int = MIN_INTERVALS, n_freq: int = N_FREQ, f_lo: float = F_LO, f_hi: float = F_HI,
             lf_band=LF_BAND, hf_band=HF_BAND) -> dict:
    """The integers and doubles of bpmx_hrvspec_params at rate `sr`: window and
    step in samples, the interval range ``dmin`` .. ``dmax`` from ``max_bpm``
    and ``min_bpm`` of `params` (DEFAULT_PARAMS: 240 and 40; the integers of
    ``tempo.geometry``), ``min_span`` one period of `f_lo`, the grid of
    `n_freq` frequencies from `f_lo` to `f_hi` inclusive in rad per sample, and
    the bands as index ranges on it: a band takes the grid points from its
    lower edge up to, not including, its upper edge, except that a band whose
    upper edge is `f_hi` takes the last point too."""
    p = DEFAULT_PARAMS if params is None else params
    n_freq = int(n_freq)
    df = (f_hi - f_lo) / (n_freq - 1) if n_freq > 1 else (f_hi - f_lo)

    def at(f, top=False):                 # the first grid index at or above f; past f with `top`
        if df <= 0:
            return n_freq if top else 0
        k = math.floor((f - f_lo) / df + 1e-9) + 1 if top else math.ceil((f - f_lo) / df - 1e-9)
        return min(max(int(k), 0), n_freq)

    def band(b):
        lo, hi = at(b[0]), at(b[1], top=b[1] >= f_hi)
        return lo, max(lo, hi)

    (lf_a, lf_b), (hf_a, hf_b) = band(lf_band), band(hf_band)
    return dict(win=int(win_sec * sr), hop=int(hop_sec * sr), dmin=int(math.ceil(60 * sr / p["max_bpm"])),
                dmax=int(math.floor(60 * sr / p["min_bpm"])), min_intervals=int(min_intervals),
                min_span=int(math.ceil(sr / f_lo)), n_freq=n_freq, lf_a=lf_a, lf_b=lf_b, hf_a=hf_a, hf_b=hf_b,
                om0=2.0 * math.pi * f_lo / sr, dom=2.0 * math.pi * df / sr, scale=df / sr)


def check_geometry(g: dict) -> None:
    """The conditions bpmx_hrvspec_device answers BPMX_E_ARG to."""
    ok = (g["hop"] >= 1 and 1 <= g["dmin"] <= g["dmax"] and g["min_intervals"] >= 3 and 1 <= g["n_freq"] <= 1024
          and 0 <= g["lf_a"] <= g["lf_b"] <= g["n_freq"] and 0 <= g["hf_a"] <= g["hf_b"] <= g["n_freq"]
          and math.isfinite(g["om0"]) and math.isfinite(g["dom"]) and g["om0"] > 0 and g["dom"] >= 0)
    if not ok:
        raise ValueError("hrv spectrum: needs hop >= 1, 1 <= dmin <= dmax, min_intervals >= 3, 1 <= n_freq <= 1024, "
                         "0 <= a <= b <= n_freq for both bands, om0 > 0 and dom >= 0, both finite")


def n_windows(nd: int, win: int, hop: int) -> int:
    """bpmx_hrvspec_windows."""
    if nd <= 0 or win < 1 or hop < 1:
        return 0
    return 1 if nd <= win else (nd - win) // hop + 1


def omegas(g: dict) -> np.ndarray:
    return g["om0"] + np.arange(g["n_freq"], dtype=np.float64) * g["dom"]


def power(s: np.ndarray, u: np.ndarray, om: np.ndarray):
    """(q, CC_tau, SS_tau) of the centred values `u` at the integer times `s`:
    the six sums in one pass, tau removed by rotating the sums."""
    n = len(s)
    a = s[:, None] * om[None, :]
    c, sn = np.cos(a), np.sin(a)
    w = 1.0 / n
    Y = u.sum() * w
    YY = (u * u).sum() * w - Y * Y
    C, S = c.sum(0) * w, sn.sum(0) * w
    CC0 = (c * c).sum(0) * w
    CC, SS, CS = CC0 - C * C, (1.0 - CC0) - S * S, (c * sn).sum(0) * w - C * S
    YC, YS = (u[:, None] * c).sum(0) * w - Y * C, (u[:, None] * sn).sum(0) * w - Y * S
    tau = 0.5 * np.arctan2(2.0 * CS, CC - SS)
    ct, st = np.cos(tau), np.sin(tau)
    YCt, YSt = YC * ct + YS * st, YS * ct - YC * st
    x = 2.0 * CS * ct * st
    CCt = np.maximum(CC * ct * ct + x + SS * st * st, EPSNEG)
    SSt = np.maximum(SS * ct * ct - x + CC * st * st, EPSNEG)
    return (YCt * YCt / CCt + YSt * YSt / SSt) / YY, CCt, SSt


def _band(q, a, b):
    if b <= a:
        return 0.0, -1, math.inf
    seg = q[a:b]
    k = int(np.argmax(seg))                        # the first of equal values: the smallest index
    v = np.sort(seg)
    return float(seg.sum()), a + k, (float(v[-1] - v[-2]) if len(v) > 1 else math.inf)


def spectrum_ints(final_idx, nd: int, sr: int, g: dict, beats_ok: bool = True, detail: bool = False) -> dict:
    """The definition for given integers (`g`: ``geometry``'s dict).  Per
    window ``time`` (t_mid), ``n_rr``, ``code``, ``var``, ``lf``, ``hf``,
    ``lf_peak``, ``hf_peak`` (grid indices, -1 for none) and the row of ``q``;
    per recording ``record`` (valid windows, the means of lf, hf, lf / hf and
    lf / (lf + hf), three reserved NaN) and ``status``.

    `detail` adds per window and frequency ``cc`` and ``ss`` (the normal
    equations' diagonals after the rotation by tau) and ``tol`` (the bound on
    an absolute error of q: ``(16 n + 8 omega S) * 2^-52 / min(cc, ss)``), and
    per window ``lf_gap`` / ``hf_gap``, the band's largest q minus its second
    largest (inf with fewer than two)."""
    check_geometry(g)
    idx = np.ascontiguousarray(final_idx, dtype=np.int64)
    nw, nq = n_windows(int(nd), g["win"], g["hop"]), g["n_freq"]
    none = not beats_ok or len(idx) < 2
    out = dict(g, sr=int(sr), status=NONE if none else OK,
               time=np.full(nw, np.nan), n_rr=np.zeros(nw, np.int32), code=np.full(nw, CODE_FEW, np.int32),
               var=np.full(nw, np.nan), lf=np.full(nw, np.nan), hf=np.full(nw, np.nan),
               lf_peak=np.full(nw, -1, np.int32), hf_peak=np.full(nw, -1, np.int32), q=np.full((nw, nq), np.nan))
    det = dict(cc=np.full((nw, nq), np.nan), ss=np.full((nw, nq), np.nan), tol=np.full((nw, nq), np.nan),
               lf_gap=np.full(nw, np.nan), hf_gap=np.full(nw, np.nan))
    om = omegas(g)
    if not none:
        d, e = np.diff(idx), idx[1:]
        keep = (d >= g["dmin"]) & (d <= g["dmax"])
        d, e = d[keep], e[keep]
        for w in range(nw):
            lo = w * g["hop"]
            a, b = np.searchsorted(e, lo, "left"), np.searchsorted(e, lo + g["win"], "left")
            n = int(b - a)
            out["n_rr"][w] = n
            if n:
                out["time"][w] = float(e[a] + e[b - 1]) / (2.0 * sr)
            y = d[a:b] * 1000.0 / sr
            if n < g["min_intervals"]:
                continue
            S = int(e[b - 1] - e[a])
            if S < g["min_span"]:
                out["code"][w] = CODE_SHORT
                continue
            if (y == y[0]).all():
                out["code"][w] = CODE_CONSTANT
                continue
            out["code"][w] = CODE_VALID
            s = (e[a:b] - e[a]).astype(np.float64)
            u = y - y.sum() / n
            var = float((u * u).sum() / n)
            q, cc, ss = power(s, u, om)
            out["q"][w], out["var"][w] = q, var
            k = g["scale"] * S * var
            sl, out["lf_peak"][w], det["lf_gap"][w] = _band(q, g["lf_a"], g["lf_b"])
            sh, out["hf_peak"][w], det["hf_gap"][w] = _band(q, g["hf_a"], g["hf_b"])
            out["lf"][w], out["hf"][w] = k * sl, k * sh
            det["cc"][w], det["ss"][w] = cc, ss
            det["tol"][w] = (16.0 * n + 8.0 * om * S) * 2.0 ** -52 / np.minimum(cc, ss)
    out["record"] = record_of(out["code"], out["lf"], out["hf"])
    if detail:
        out.update(det)
    return out


def record_of(code, lf, hf) -> np.ndarray:
    """The 8 doubles of a recording: means added in window order, NaN with
    nothing to average."""
    rec = np.full(RECORD, np.nan)
    nv = n_r = n_s = 0
    s_lf = s_hf = s_r = s_s = 0.0
    for c, a, b in zip(code, lf, hf):
        if c != CODE_VALID:
            continue
        a, b = float(a), float(b)
        nv += 1
        s_lf += a
        s_hf += b
        if b > 0:
            s_r += a / b
            n_r += 1
        if a + b > 0:
            s_s += a / (a + b)
            n_s += 1
    rec[0] = nv
    if nv:
        rec[1], rec[2] = s_lf / nv, s_hf / nv
    if n_r:
        rec[3] = s_r / n_r
    if n_s:
        rec[4] = s_s / n_s
    return rec


def spectrum(final_idx, nd: int, sr: int, params: Optional[dict] = None, detail: bool = False, **kw) -> dict:
    """The HRV spectrum of one recording's final beats (samples at rate `sr`,
    envelope length `nd`): ``spectrum_ints`` at ``geometry(sr, params, **kw)``."""
    return spectrum_ints(final_idx, nd, sr, geometry(sr, params, **kw), detail=detail)


def peak_hz(d: dict, k) -> np.ndarray:
    """The grid frequencies of peak indices, NaN for -1."""
    k = np.asarray(k, np.int64)
    f = (d["om0"] + k * d["dom"]) * d["sr"] / (2.0 * math.pi)
    return np.where(k < 0, np.nan, f)


def spectrum_path(original_file_path: str, output_directory: str) -> str:
    base = os.path.basename(os.path.splitext(original_file_path)[0])
    return os.path.join(output_directory, f"{base}_hrv_spectrum.csv")


CSV_HEADER = ["Time (s)", "Intervals", "Code", "LF (ms^2)", "HF (ms^2)", "LF/HF", "LF peak (Hz)", "HF peak (Hz)"]
RECORD_KEYS = ("n_valid", "mean_lf", "mean_hf", "mean_lf_hf", "mean_lf_norm")


def write_csv(path: str, d: dict) -> None:
    """``<base>_hrv_spectrum.csv``: a row per window (floats by ``repr``, so
    they read back as they were), then the settings, the status and the record
    as ``# key,value`` lines."""
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(d["hf"] > 0, d["lf"] / d["hf"], np.nan)
    lp, hp = peak_hz(d, d["lf_peak"]), peak_hz(d, d["hf_peak"])
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(CSV_HEADER)
        for i in range(len(d["code"])):
            w.writerow([repr(float(d["time"][i])), int(d["n_rr"][i]), int(d["code"][i]), repr(float(d["lf"][i])),
                        repr(float(d["hf"][i])), repr(float(ratio[i])), repr(float(lp[i])), repr(float(hp[i]))])
        w.writerow(["# sr", int(d["sr"])])
        for k in INT_KEYS:
            w.writerow([f"# {k}", int(d[k])])
        for k in FLOAT_KEYS:
            w.writerow([f"# {k}", repr(float(d[k]))])
        w.writerow(["# status", int(d["status"])])
        for k, v in zip(RECORD_KEYS, d["record"]):
            w.writerow([f"# {k}", repr(float(v))])


def read_csv(path: str) -> dict:
    """The columns and ``# key,value`` lines as ``write_csv`` wrote them:
    ``time``, ``n_rr``, ``code``, ``lf``, ``hf``, ``lf_hf``, ``lf_peak_hz``,
    ``hf_peak_hz``, the settings, ``status`` and ``record``."""
    rows, kv = [], {}
    with open(path, newline="") as f:
        r = csv.reader(f)
        assert next(r) == CSV_HEADER
        for row in r:
            if row[0].startswith("# "):
                kv[row[0][2:]] = row[1]
            else:
                rows.append(row)
    col = lambda i, t: np.array([t(x[i]) for x in rows], np.int32 if t is int else np.float64)  # noqa: E731
    d = dict(time=col(0, float), n_rr=col(1, int), code=col(2, int), lf=col(3, float), hf=col(4, float),
             lf_hf=col(5, float), lf_peak_hz=col(6, float), hf_peak_hz=col(7, float), sr=int(kv["sr"]),
             status=int(kv["status"]))
    d.update({k: int(kv[k]) for k in INT_KEYS})
    d.update({k: float(kv[k]) for k in FLOAT_KEYS})
    rec = np.full(RECORD, np.nan)
    rec[:len(RECORD_KEYS)] = [float(kv[k]) for k in RECORD_KEYS]
    d["record"] = rec
    return d
