"""Shared by test_hrv_spectrum.py, test_hrvspec_core.py (CPU) and
test_gpu_hrv_spectrum.py: beat lists for the HRV spectrum around every guard of
its definition, ``hrv_spectrum.spectrum_ints`` on them (computed once), the
comparison at the derived tolerance, and the binary exchange with
hrvspec_core_driver.

The tolerance is not tuned.  On q, absolutely,

    tol[m] = (16 n + 8 omega_m S) * 2^-52 / min(CC_tau[m], SS_tau[m])

with CC and SS from the oracle: each of the six weighted sums of n terms is
bounded by 1 in the normalised units, the argument omega * s carries
omega S 2^-53 of rounding, and both are divided by the smaller diagonal of the
normal equations.  var, lf and hf: the band sum of tol (in their units) plus
(n_freq + 16) * 2^-52 relative.  A peak index must be equal wherever the
oracle's top-two gap in the band exceeds twice the band's largest tol; the
cases are built so that this holds everywhere (``open_peaks``).  Counts,
codes, n_rr, statuses, window counts and t_mid are exact."""
from __future__ import annotations

import functools
import os
import struct

import numpy as np

from bpm_analysis_amd import _native as N
from bpm_analysis_amd import hrv_spectrum as HS
from tests import metrics_cases as MC

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "beats")
GOLDENS = ("vulpine", "long_6k_8min", "long_8k_5min_hint", "ref_44k_60s_mono", "env_random_rough")
EPS = 2.0 ** -52

# a small geometry at 100 samples/s: 30 s windows every 7.5 s, 37 frequencies 0.04 .. 0.40 Hz
SR = 100
G = dict(win=3000, hop=750, dmin=25, dmax=150, min_intervals=8, min_span=2500, n_freq=37, lf_a=0, lf_b=11, hf_a=11,
         hf_b=37, om0=2 * np.pi * 0.04 / SR, dom=2 * np.pi * 0.01 / SR, scale=0.01 / SR)


def grid(n_freq, **kw):
    """G with `n_freq` points over the same 0.04 .. 0.40 Hz (one point: 0.04 Hz)."""
    df = 0.36 / (n_freq - 1) if n_freq > 1 else 0.36
    a = min(n_freq, int(np.ceil(0.11 / df - 1e-9)))
    return dict(G, n_freq=n_freq, lf_a=0, lf_b=a, hf_a=a, hf_b=n_freq, dom=2 * np.pi * df / SR, scale=df / SR, **kw)


def rhythm(n, seed, sr=SR, base=0.8, resp=0.25, depth=0.06, slow=0.09, noise=0.01, t0=0.3):
    """Beat samples of a heart with respiratory (HF) and slow (LF) modulation."""
    rng = np.random.default_rng(seed)
    t, out = t0, [t0]
    for _ in range(n):
        rr = base + depth * np.sin(2 * np.pi * resp * t + seed) + 0.04 * np.sin(2 * np.pi * slow * t) \
            + noise * rng.standard_normal()
        t += rr
        out.append(t)
    idx = np.round(np.array(out) * sr).astype(np.int64)
    assert np.all(np.diff(idx) > 0)
    return idx


def case(name, idx, nd, sr=SR, g=None, ok=True):
    return dict(name=name, idx=np.ascontiguousarray(idx, np.int64), nd=int(nd), sr=int(sr), g=dict(G if g is None else g),
                ok=bool(ok))


def golden_beats(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=True)
    return z["final_peaks"].astype(np.int64), int(z["sr"])


def pairs(n, seed, jump=300):
    """n kept intervals, each followed by an excluded one of `jump` samples: few intervals over a long span."""
    rng = np.random.default_rng(seed)
    t, out = 10, []
    for _ in range(n):
        out += [t, t + int(rng.integers(70, 110))]
        t = out[-1] + jump
    return np.array(out, np.int64)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for seed in range(3):                                    # the defaults at the usual rate, missing beats included
        idx = MC.beats_of(MC.wander(700 + 60 * seed, seed, lo=55.0, hi=110.0, noise=0.03), sr=302)
        if seed == 1:
            idx = np.delete(idx, np.arange(17, len(idx), 23))            # 4 % missed beats: the long intervals drop out
        out.append(case(f"wander{seed}", idx, int(idx[-1]) + 302, sr=302, g=HS.geometry(302)))
    for name in GOLDENS:
        idx, sr = golden_beats(name)
        out.append(case("golden_" + name, idx, int(idx[-1]) + sr, sr=sr, g=HS.geometry(sr)))
    base = rhythm(160, 1)                                    # about 128 s: 14 windows of 30 s
    nd = int(base[-1]) + 50
    out.append(case("rhythm", base, nd))
    out.append(case("rhythm_odd_nd", rhythm(97, 2), 7777))
    # every code
    few = rhythm(6, 3)
    out.append(case("few", few, 3000))
    out.append(case("short_span", np.arange(12) * 100 + 5 + (np.arange(12) % 3), 3000))     # 11 intervals within 11 s
    out.append(case("constant", np.arange(200) * 80 + 3, 200 * 80))
    out.append(case("all_excluded", np.arange(60) * 200, 12000))                           # every interval > dmax
    out.append(case("excluded_then_rhythm", np.concatenate([np.arange(20) * 200, 4000 + rhythm(150, 4)]), 16000))
    # exactly min_intervals and one fewer, over a span that suffices
    p8, p7 = pairs(8, 5), pairs(7, 5)
    out.append(case("min_intervals_exact", p8, 3000))
    out.append(case("min_intervals_less", p7, 3000))
    # a span of exactly min_span and one sample less
    e = p8[1::2]
    span = int(e[-1] - e[0])
    out.append(case("span_exact", p8, 3000, g=dict(G, min_span=span)))
    out.append(case("span_less", p8, 3000, g=dict(G, min_span=span + 1)))
    # intervals of exactly dmin, dmin - 1, dmax, dmax + 1 among ordinary ones
    rng = np.random.default_rng(6)
    d = rng.integers(60, 100, 240)
    d[3::8], d[5::8], d[6::8], d[7::8] = 25, 24, 150, 151
    edge = np.concatenate([[7], 7 + np.cumsum(d)])
    out.append(case("interval_edges", edge, int(edge[-1]) + 1))
    # the window count at its edges
    for n in (0, G["win"] - 1, G["win"], G["win"] + 1, G["win"] + G["hop"] - 1, G["win"] + G["hop"]):
        out.append(case(f"nd_{n}", base, n))
    # the grid: 1, 37 (above), 256 and 300 frequencies
    for nq in (1, 256, 300):
        out.append(case(f"n_freq_{nq}", rhythm(80, 7 + nq), 6000, g=grid(nq)))
    # an empty band, and bands that touch the grid's ends
    out.append(case("lf_empty_hf_all", rhythm(80, 8), 6000, g=dict(G, lf_a=0, lf_b=0, hf_a=0, hf_b=37)))
    out.append(case("hf_empty_at_end", rhythm(80, 9), 6000, g=dict(G, lf_a=5, lf_b=37, hf_a=37, hf_b=37)))
    out.append(case("one_point_bands", rhythm(80, 10), 6000, g=dict(G, lf_a=0, lf_b=1, hf_a=36, hf_b=37)))
    # no beats to use
    for n in (0, 1, 2):
        out.append(case(f"n_final_{n}", base[:n], 4000))
    out.append(case("bad_status", base, nd, ok=False))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected():
    return tuple(HS.spectrum_ints(c["idx"], c["nd"], c["sr"], c["g"], beats_ok=c["ok"], detail=True) for c in cases())


def band_tol(want, w, a, b):
    """(the bound on the band's sum of q, twice its largest tol) of window w."""
    t = want["tol"][w, a:b]
    return (float(t.sum()), 2.0 * float(t.max())) if b > a else (0.0, 0.0)


def open_peaks(want):
    """Windows whose LF or HF peak the tolerance leaves open, from the oracle's values alone."""
    bad = []
    for w in np.flatnonzero(want["code"] == 0):
        for k, a, b in (("lf", want["lf_a"], want["lf_b"]), ("hf", want["hf_a"], want["hf_b"])):
            if b > a and not want[k + "_gap"][w] > band_tol(want, w, a, b)[1]:
                bad.append((int(w), k))
    return bad


def assert_close(got, want, name, q=True):
    """A result (driver or device form) against the oracle's dict at the derived tolerance -> the largest
    share of the bound on q that was used."""
    assert int(got["status"]) == int(want["status"]), (name, got["status"])
    assert len(got["code"]) == len(want["code"]), (name, len(got["code"]))
    for k in ("code", "n_rr"):
        assert np.array_equal(got[k], want[k]), (name, k, got[k], want[k])
    assert np.array_equal(got["time"], want["time"], equal_nan=True), (name, "time")
    used = 0.0
    nq, S_all = want["n_freq"], None
    for w in range(len(want["code"])):
        if want["code"][w] != 0:
            assert np.isnan(got["var"][w]) and np.isnan(got["lf"][w]) and np.isnan(got["hf"][w]), (name, w)
            assert got["lf_peak"][w] == -1 and got["hf_peak"][w] == -1, (name, w)
            if q and "q" in got:
                assert np.isnan(got["q"][w]).all(), (name, w)
            continue
        rel = (nq + 16) * EPS
        assert abs(got["var"][w] - want["var"][w]) <= rel * want["var"][w], (name, w, "var")
        if q and "q" in got:
            err = np.abs(got["q"][w] - want["q"][w]) / want["tol"][w]
            used = max(used, float(err.max()))
            assert (err <= 1.0).all(), (name, w, "q", float(err.max()), int(err.argmax()))
        for k, a, b in (("lf", want["lf_a"], want["lf_b"]), ("hf", want["hf_a"], want["hf_b"])):
            sum_tol, peak_tol = band_tol(want, w, a, b)
            if b <= a:
                assert got[k][w] == 0.0 and got[k + "_peak"][w] == -1, (name, w, k)
                continue
            unit = want[k][w] / want["q"][w, a:b].sum()              # scale * S * var
            bound = unit * sum_tol + rel * abs(want[k][w])
            assert abs(got[k][w] - want[k][w]) <= bound, (name, w, k, got[k][w], want[k][w], bound)
            if want[k + "_gap"][w] > peak_tol:
                assert got[k + "_peak"][w] == want[k + "_peak"][w], (name, w, k + "_peak")
            else:
                assert a <= got[k + "_peak"][w] < b, (name, w, k + "_peak")
    # the record is the definition's arithmetic on the result's own windows, in window order
    assert np.array_equal(got["record"], HS.record_of(got["code"], got["lf"], got["hf"]), equal_nan=True), (name, "record")
    assert got["record"][0] == want["record"][0], (name, "valid windows")
    return used


# ---- hrvspec_core_driver's files ------------------------------------------------ #
def write_cases(path, cs=None):
    cs = cases() if cs is None else cs
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cs)))
        for c in cs:
            f.write(struct.pack("<iiiiq", len(c["idx"]), c["sr"], 0 if c["ok"] else -2, 0, c["nd"]))
            f.write(bytes(N.hrvspec_params(c["g"])))
            f.write(c["idx"].astype(np.int32).tobytes())


def read_results(path, cs=None):
    cs = cases() if cs is None else cs
    buf = open(path, "rb").read()
    o, out = 0, []

    def take(dt, n):
        nonlocal o
        a = np.frombuffer(buf, dt, n, o)
        o += a.nbytes
        return a

    for c in cs:
        st, nw = (int(v) for v in take(np.int32, 2))
        nq = c["g"]["n_freq"]
        r = dict(status=st)
        for k in ("code", "n_rr", "lf_peak", "hf_peak"):
            r[k] = take(np.int32, nw)
        for k in ("time", "var", "lf", "hf"):
            r[k] = take(np.float64, nw)
        r["q"] = take(np.float64, nw * nq).reshape(nw, nq)
        r["record"] = take(np.float64, HS.RECORD)
        out.append(r)
    assert o == len(buf)
    return out
